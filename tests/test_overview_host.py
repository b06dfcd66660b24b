"""The overview render (sgz_overview_step, sgz_stage_overview, sgz_spectrogram_overview_device / _host; csrc/overview.hip) without a GPU: the
exports, the column arithmetic against a brute-force count, the refusals every call makes before it touches the device, the three kernels
in the built gfx950 code object (no scratch, no spill), and the numpy restatement of the ordering that tests/test_gpu_overview.py holds
the kernels to (tests/overview_ref.py) on hand-made groups."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import overview_ref as ov  # noqa: E402

NAMES = ("sgz_overview_step", "sgz_stage_overview", "sgz_spectrogram_overview_device", "sgz_spectrogram_overview_host")


@pytest.fixture(scope="module")
def plan():
    return api.Plan(config.spectrum_config(window_size=64, hop=16, axis_points=33))        # host tables only: never uploaded here


@pytest.fixture(scope="module")
def buf():
    """a host block that stands for any non-NULL buffer: every call here is refused before a buffer is looked at"""
    b = np.zeros(4096, np.float32)
    return b, b.ctypes.data_as(C.c_void_p)


def test_exports_exist():
    L = api.lib()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(L, name), name
    for name in ("overview_columns", "overview"):
        assert callable(getattr(api.Plan, name))
    with open(os.path.join(ROOT, "include", "sgz.h")) as f:
        header = f.read()
    assert all(name + "(" in header for name in NAMES) and "#define SGZ_ABI_VERSION 5" in header
    assert "#define SGZ_OPT_OVERVIEW_SLAB 10u" in header and api.OPT_OVERVIEW_SLAB == 10
    assert api.lib().sgz_abi_version() == 5


def test_overview_slab_is_a_plan_option(plan):
    for value in (0, 1, 3, 1 << 20):
        assert api.lib().sgz_plan_set_option(plan.h, api.OPT_OVERVIEW_SLAB, value) == api.SGZ_OK
    assert api.lib().sgz_plan_set_option(plan.h, api.OPT_OVERVIEW_SLAB, 0) == api.SGZ_OK


def _brute_step(k, held, frames, flush):
    """count the columns one frame at a time"""
    columns, open_frames = 0, held
    for _ in range(frames):
        open_frames += 1
        if open_frames == k:
            columns, open_frames = columns + 1, 0
    if flush and open_frames:
        columns, open_frames = columns + 1, 0
    return columns, open_frames


def test_overview_step_equals_a_brute_force_count():
    rng = np.random.default_rng(7)
    sequences = 0
    while sequences < 2000:
        k = int(rng.choice([1, 2, 3, 7, 8, 9, 64, 1000, int(rng.integers(1, 300))]))
        held, total, columns = 0, 0, 0
        calls = int(rng.integers(1, 6))
        for call in range(calls):                                              # chained calls: the held count of one is the next one's
            frames = int(rng.choice([0, 1, k - 1, k, k + 1, int(rng.integers(0, 3 * k + 2))]))
            flush = call == calls - 1 and bool(rng.integers(0, 2))
            got = api.overview_step(k, held, frames, flush)
            assert got == _brute_step(k, held, frames, flush), (k, held, frames, flush, got)
            columns, total, held = columns + got[0], total + frames, got[1]
            sequences += 1
        assert columns * k + held >= total and (columns == -(-total // k) if flush else columns == total // k), (k, total, columns, held)
    assert api.overview_step(5, 4, 2 ** 40, False) == ((2 ** 40 + 4) // 5, (2 ** 40 + 4) % 5)


def test_overview_step_refusals():
    L = api.lib()
    c, h = C.c_uint64(77), C.c_uint64(78)
    assert L.sgz_overview_step(0, 0, 10, 0, C.byref(c), C.byref(h)) == api.SGZ_EINVAL
    assert L.sgz_overview_step(4, 4, 10, 0, C.byref(c), C.byref(h)) == api.SGZ_EINVAL
    assert L.sgz_overview_step(4, 5, 10, 1, C.byref(c), C.byref(h)) == api.SGZ_EINVAL
    assert L.sgz_overview_step(4, 0, 10, 0, None, C.byref(h)) == api.SGZ_EINVAL
    assert L.sgz_overview_step(4, 0, 10, 0, C.byref(c), None) == api.SGZ_EINVAL
    assert (c.value, h.value) == (77, 78)
    assert L.sgz_overview_step(4, 3, 0, 1, C.byref(c), C.byref(h)) == api.SGZ_OK and (c.value, h.value) == (1, 0)


def test_stage_call_refusals_before_the_device(plan, buf):
    L = api.lib()
    b, p = buf
    E = api.SGZ_EINVAL
    #                                      lines frames k held flush slices carry rgba peaks stream
    assert L.sgz_stage_overview(None, p, 4, 2, 0, 1, 0, p, p, p, None) == E
    assert L.sgz_stage_overview(plan.h, None, 4, 2, 0, 1, 0, p, p, p, None) == E
    assert L.sgz_stage_overview(plan.h, p, 4, 0, 0, 1, 0, p, p, p, None) == E              # k == 0
    assert L.sgz_stage_overview(plan.h, p, 4, 2, 2, 1, 0, p, p, p, None) == E              # held >= k
    assert L.sgz_stage_overview(plan.h, p, 4, 2, 3, 1, 0, p, p, p, None) == E
    assert L.sgz_stage_overview(plan.h, p, 4, 1, 1, 1, 0, p, p, p, None) == E
    assert L.sgz_stage_overview(plan.h, p, 4, 2, 0, 1, 65, p, p, p, None) == E             # slices > 64
    assert L.sgz_stage_overview(plan.h, p, 4, 2, 0, 1, 0xffffffff, p, p, p, None) == E
    assert L.sgz_stage_overview(plan.h, p, 4, 2, 0, 1, 0, p, None, None, None) == E        # both outputs NULL
    assert L.sgz_stage_overview(plan.h, p, 4, 2, 1, 1, 0, None, p, p, None) == E           # the carry is read
    assert L.sgz_stage_overview(plan.h, p, 3, 2, 0, 0, 0, None, p, p, None) == E           # the carry is written
    assert L.sgz_stage_overview(plan.h, p, 0, 2, 1, 1, 0, None, p, None, None) == E        # a flush of the held column reads it
    # nothing arrives and no column to flush: SGZ_OK before the plan is looked at any further (it stays without device tables)
    assert L.sgz_stage_overview(plan.h, p, 0, 2, 0, 1, 0, None, p, None, None) == api.SGZ_OK
    assert L.sgz_stage_overview(plan.h, p, 0, 2, 0, 0, 0, None, p, None, None) == api.SGZ_OK
    assert L.sgz_stage_overview(plan.h, p, 0, 3, 2, 0, 0, p, p, None, None) == api.SGZ_OK
    assert not b.any()


def test_render_refusals_before_the_device(plan, buf):
    L = api.lib()
    b, p = buf
    ch = (C.c_void_p * 2)(p, p)
    E = api.SGZ_EINVAL
    assert L.sgz_spectrogram_overview_device(None, p, 1024, 1024, 2, p, p, None, None) == E
    assert L.sgz_spectrogram_overview_device(plan.h, None, 1024, 1024, 2, p, p, None, None) == E
    assert L.sgz_spectrogram_overview_device(plan.h, p, 1024, 1024, 0, p, p, None, None) == E
    assert L.sgz_spectrogram_overview_device(plan.h, p, 1024, 1024, 2, None, None, None, None) == E
    assert L.sgz_spectrogram_overview_host(None, ch, 2, 1024, 2, p, p, None) == E
    assert L.sgz_spectrogram_overview_host(plan.h, None, 2, 1024, 2, p, p, None) == E
    assert L.sgz_spectrogram_overview_host(plan.h, ch, 2, 1024, 0, p, p, None) == E
    assert L.sgz_spectrogram_overview_host(plan.h, ch, 2, 1024, 2, None, None, None) == E
    assert L.sgz_spectrogram_overview_host(plan.h, ch, 3, 1024, 2, p, p, None) == E          # 2 * num_pairs channels, as the render
    assert L.sgz_spectrogram_overview_host(plan.h, (C.c_void_p * 2)(p, None), 2, 1024, 2, p, p, None) == E
    assert not b.any()


def test_overview_kernels_in_the_code_object_without_scratch():
    import codeobj_report as cr
    lib = api.LIB_PATH
    api.lib()
    if not (os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("llvm tools not present")
    rows = cr.kernels(lib)
    for kernel in ("overviewColumnsKernel", "overviewSliceKernel", "overviewEmitKernel"):
        mine = [r for r in rows if kernel + "(" in r["demangled"]]
        assert len(mine) == 1, [r["demangled"] for r in mine]
        for r in mine:
            assert not r.get("private_segment_fixed_size", 0) and not r.get("vgpr_spill_count", 0) and not r.get("sgpr_spill_count", 0), r


# ---- the ordering's numpy restatement on hand-made groups ---------------------------------------------------------------------------------
def _bits(*values):
    return np.array(values, np.float32).view(np.uint32)


def _f(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


NAN_A, NAN_B = _f(0x7FC12345), _f(0xFFC00001)              # a positive and a negative NaN with payloads
PZ, NZ = np.float32(0.0), np.float32(-0.0)
INF = np.float32(np.inf)
GROUPS = [
    # (group, bits of the greatest)
    ([NZ, PZ], 0x00000000), ([PZ, NZ], 0x00000000), ([NZ, NZ], 0x80000000), ([NZ], 0x80000000),         # -0 below +0, in both orders
    ([NAN_A, 1.5, -2.0], _bits(1.5)[0]), ([1.5, -2.0, NAN_A], _bits(1.5)[0]), ([-2.0, NAN_B, -3.0], _bits(-2.0)[0]),   # NaN first / last / inside
    ([NAN_A], 0x7FC00000), ([NAN_B], 0x7FC00000), ([NAN_A, NAN_B, NAN_A], 0x7FC00000),                  # alone / everywhere: the quiet NaN
    ([-INF, NAN_B], 0xFF800000), ([-INF, INF, 3.0], 0x7F800000), ([-INF, -1e38], _bits(-1e38)[0]), ([INF, NAN_A], 0x7F800000),
    ([-1.0, -2.0, -0.5], _bits(-0.5)[0]), ([-1e-45, -1.0], _bits(-1e-45)[0]), ([-1e-45, NZ], 0x80000000), ([1e-45, PZ], _bits(1e-45)[0]),
    ([0.25, 0.999, 0.9989999], _bits(0.999)[0]), ([2.0, 2.0, 2.0], _bits(2.0)[0]),
]


def test_the_ordering_on_hand_made_groups():
    for group, want in GROUPS:
        g = np.array(group, np.float32)
        for order in (g, g[::-1], np.roll(g, 1)):
            got = ov.greatest(order.reshape(-1, 1), axis=0)
            assert got.dtype == np.uint32 and int(got[0]) == int(want), (group, hex(int(got[0])), hex(int(want)))
        # any split gives the same bits: the greatest of the parts' greatest values
        for cut in range(1, len(g)):
            parts = np.array([ov.greatest(g[:cut]), ov.greatest(g[cut:])], np.uint32).view(np.float32)
            assert int(ov.greatest(parts)) == int(want), (group, cut)


def test_the_ordering_is_ieee_order_on_ordinary_values():
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.standard_normal(4000).astype(np.float32), np.float32([0, 1, -1, np.inf, -np.inf, 1e-45, -1e-45, 3e38, -3e38])])
    k = ov.order_key(v)
    assert k.min() > 0 and np.array_equal(ov.key_value(k), v.view(np.uint32))
    a, b = v[:-1], v[1:]
    assert np.array_equal(k[:-1] < k[1:], a < b) and np.array_equal(k[:-1] == k[1:], a.view(np.uint32) == b.view(np.uint32))
    assert int(ov.order_key(np.float32([-np.inf]))[0]) == 0x007FFFFF


def test_columns_of_with_a_carry_equals_columns_of_the_whole():
    rng = np.random.default_rng(11)
    x = rng.standard_normal((23, 2, 5)).astype(np.float32)
    x[rng.random(x.shape) < 0.2] = np.nan
    x[3:9, 0, 2] = np.nan
    for k in (1, 2, 5, 7, 23, 26):
        whole, none, left = ov.columns_of(x, k)
        assert none is None and left == 0 and whole.shape[0] == -(-23 // k)
        for cut in (1, 6, 10, 22):
            a, carry, held = ov.columns_of(x[:cut], k, flush=False)
            assert held == cut % k and (carry is None) == (held == 0)
            b, none, _ = ov.columns_of(x[cut:], k, held=held, carry=carry)
            assert np.array_equal(np.concatenate([a, b]), whole), (k, cut)
