"""The file lane without a GPU (sgz_overview_view_columns, sgz_stage_overview_view, sgz_overview_view_host; sgz_pcm_stream_feed_overview,
sgz_pcm_stream_columns_for, sgz_pcm_stream_open_frames, sgz_spectrogram_overview_pcm): the exports, the view's column boundaries
ceil(b m / cols) against a brute-force assignment of every source column to its output column, the refusals every call makes before
it touches the device, and the three view kernels in the built gfx950 code object (no scratch, no spill)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("sgz_overview_view_columns", "sgz_stage_overview_view", "sgz_overview_view_host", "sgz_pcm_stream_feed_overview",
         "sgz_pcm_stream_columns_for", "sgz_pcm_stream_open_frames", "sgz_spectrogram_overview_pcm")


@pytest.fixture(scope="module")
def plan():
    return api.Plan(config.spectrum_config(window_size=64, hop=16, axis_points=33))        # host tables only: never uploaded here


@pytest.fixture(scope="module")
def buf():
    """a host block that stands for any non-NULL buffer: every call here is refused before a buffer is looked at"""
    b = np.zeros(8192, np.float32)
    return b, b.ctypes.data_as(C.c_void_p)


def test_exports_exist():
    L = api.lib()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(L, name), name
    assert callable(api.overview_view_columns) and callable(api.overview_pcm) and callable(api.Plan.overview_view)
    for name in ("feed_overview", "feed_overview_into", "columns_for", "open_frames"):
        assert callable(getattr(api.PcmStream, name)), name
    with open(os.path.join(ROOT, "include", "sgz.h")) as f:
        header = f.read()
    assert all(name + "(" in header for name in NAMES) and "#define SGZ_ABI_VERSION 5" in header
    assert api.lib().sgz_abi_version() == 5


def _check_against_brute_force(n, x0, x1, out_columns):
    m = x1 - x0
    cols, bounds = api.overview_view_columns(n, x0, x1, out_columns, want_bounds=True)
    assert cols == min(out_columns, m) == api.overview_view_columns(n, x0, x1, out_columns), (n, x0, x1, out_columns)
    bounds = [int(v) for v in bounds]
    assert len(bounds) == cols + 1 and bounds[0] == x0 and bounds[-1] == x1, (n, x0, x1, out_columns, bounds)
    assert all(a < b for a, b in zip(bounds[:-1], bounds[1:])), (n, x0, x1, out_columns, bounds)      # strictly increasing: never empty
    return m, cols, bounds


def test_view_columns_equal_a_brute_force_assignment():
    """source column j of the range belongs to the output column b with ceil(b m / cols) <= j - x0 < ceil((b + 1) m / cols): the greatest b
    with b m <= (j - x0) cols, i.e. floor((j - x0) cols / m) -- every source column assigned by itself, in Python integers; the
    assignment depends on (m, cols) alone, so it is made once for each and compared at every (n, x0, x1) that has them"""
    L = api.lib()
    relative = {}
    for m in range(1, 65):
        for cols in range(1, m + 1):
            owner = [(j * cols) // m for j in range(m)]
            assert sorted(set(owner)) == list(range(cols))                                  # no output column is empty
            r = relative[m, cols] = [owner.index(b) for b in range(cols)] + [m]
            assert r[0] == 0 and all(p < q for p, q in zip(r[:-1], r[1:]))                  # strictly increasing, from x0 to x1
    got, out = C.c_uint64(0), (C.c_uint64 * 70)()
    cases = 0
    for n in range(1, 65):
        for x0 in range(n):
            for x1 in range(x0 + 1, n + 1):
                m = x1 - x0
                for out_columns in range(1, m + 3):
                    assert L.sgz_overview_view_columns(n, x0, x1, out_columns, C.byref(got), out) == api.SGZ_OK
                    cols = got.value
                    assert cols == min(out_columns, m), (n, x0, x1, out_columns, cols)
                    bounds = out[:cols + 1]
                    assert bounds == [x0 + r for r in relative[m, cols]], (n, x0, x1, out_columns, bounds)
                    cases += 1
    assert cases > 700000
    _check_against_brute_force(64, 3, 60, 7)                                                # (the wrapper returns the same)


def test_view_columns_on_random_large_ranges():
    rng = np.random.default_rng(17)
    for _ in range(2000):
        n = int(rng.integers(1, 10 ** 6 + 1))
        x0 = int(rng.integers(0, n))
        x1 = int(rng.integers(x0 + 1, n + 1))
        m = x1 - x0
        out_columns = int(rng.choice([1, 2, 3, m - 1 if m > 1 else 1, m, m + 1, int(rng.integers(1, m + 1)), int(rng.integers(1, 5000))]))
        cols, bounds = api.overview_view_columns(n, x0, x1, out_columns, want_bounds=True)
        bounds = bounds.astype(np.int64)
        assert cols == min(out_columns, m) and bounds.shape == (cols + 1,) and bounds[0] == x0 and bounds[-1] == x1, (n, x0, x1, out_columns)
        assert (np.diff(bounds) > 0).all(), (n, x0, x1, out_columns)                        # strictly increasing: never empty
        owner = (np.arange(m, dtype=np.int64) * cols) // m                                  # (m, cols <= 10^6: the products fit int64)
        first = np.searchsorted(owner, np.arange(cols), side="left")                        # (owner never decreases)
        assert owner[0] == 0 and owner[-1] == cols - 1 and np.array_equal(first + x0, bounds[:-1]), (n, x0, x1, out_columns)
    assert api.overview_view_columns(2 ** 31 - 1, 0, 2 ** 31 - 1, 3, want_bounds=True)[1].tolist() == [0, 715827883, 1431655765, 2 ** 31 - 1]


def test_view_columns_refusals():
    L = api.lib()
    c = C.c_uint64(77)
    b = np.full(8, 78, np.uint64)
    bp = b.ctypes.data_as(C.c_void_p)
    E = api.SGZ_EINVAL
    assert L.sgz_overview_view_columns(10, 4, 4, 3, C.byref(c), bp) == E                   # x0 >= x1
    assert L.sgz_overview_view_columns(10, 5, 4, 3, C.byref(c), bp) == E
    assert L.sgz_overview_view_columns(10, 4, 11, 3, C.byref(c), bp) == E                  # x1 > n
    assert L.sgz_overview_view_columns(10, 4, 8, 0, C.byref(c), bp) == E                   # out_columns == 0
    assert L.sgz_overview_view_columns(2 ** 31, 4, 8, 3, C.byref(c), bp) == E              # n >= 2^31
    assert L.sgz_overview_view_columns(2 ** 40, 4, 8, 3, C.byref(c), bp) == E
    assert L.sgz_overview_view_columns(10, 4, 8, 3, None, bp) == E                         # a null result
    assert c.value == 77 and (b == 78).all()
    assert L.sgz_overview_view_columns(10, 4, 8, 3, C.byref(c), None) == api.SGZ_OK and c.value == 3
    assert L.sgz_overview_view_columns(10, 4, 8, 3, C.byref(c), bp) == api.SGZ_OK and b.tolist() == [4, 6, 7, 8, 78, 78, 78, 78]


def test_view_calls_refuse_before_the_device(plan, buf):
    L = api.lib()
    b, p = buf
    E = api.SGZ_EINVAL
    col = plan.C * plan.P * 4                                                # bytes of a source column

    def at(offset):
        return C.c_void_p(p.value + offset)

    far = at(20 * col)
    #                                       peaks n x0 x1 out slices rgba peaks_out stream
    assert L.sgz_stage_overview_view(None, p, 10, 0, 10, 4, 0, far, None, None) == E
    assert L.sgz_stage_overview_view(plan.h, None, 10, 0, 10, 4, 0, far, None, None) == E
    assert L.sgz_stage_overview_view(plan.h, p, 10, 4, 4, 4, 0, far, None, None) == E       # x0 >= x1
    assert L.sgz_stage_overview_view(plan.h, p, 10, 4, 11, 4, 0, far, None, None) == E      # x1 > n
    assert L.sgz_stage_overview_view(plan.h, p, 10, 0, 10, 0, 0, far, None, None) == E      # out_columns == 0
    assert L.sgz_stage_overview_view(plan.h, p, 2 ** 31, 0, 10, 4, 0, far, None, None) == E
    assert L.sgz_stage_overview_view(plan.h, p, 10, 0, 10, 4, 65, far, None, None) == E     # slices > 64
    assert L.sgz_stage_overview_view(plan.h, p, 10, 0, 10, 4, 0xffffffff, far, None, None) == E
    assert L.sgz_stage_overview_view(plan.h, p, 10, 0, 10, 4, 0, None, None, None) == E     # both outputs NULL
    # an output inside the source columns it is made from: the image or the peaks, at the front, inside, and by its last byte only
    assert L.sgz_stage_overview_view(plan.h, p, 10, 0, 10, 4, 0, p, None, None) == E
    assert L.sgz_stage_overview_view(plan.h, p, 10, 0, 10, 4, 0, None, p, None) == E
    assert L.sgz_stage_overview_view(plan.h, p, 10, 2, 6, 4, 0, at(5 * col), None, None) == E
    assert L.sgz_stage_overview_view(plan.h, p, 10, 2, 6, 4, 0, None, at(6 * col - 4), None) == E
    assert L.sgz_stage_overview_view(plan.h, p, 10, 2, 6, 2, 0, None, at(4), None) == E                 # its end reaches column 2
    assert L.sgz_stage_overview_view(plan.h, p, 10, 2, 6, 2, 0, at(2 * col - 2 * plan.P * 4 + 1), None, None) == E
    assert L.sgz_overview_view_host(None, p, 10, 0, 10, 4, far, None, None) == E
    assert L.sgz_overview_view_host(plan.h, None, 10, 0, 10, 4, far, None, None) == E
    assert L.sgz_overview_view_host(plan.h, p, 10, 4, 4, 4, far, None, None) == E
    assert L.sgz_overview_view_host(plan.h, p, 10, 4, 11, 4, far, None, None) == E
    assert L.sgz_overview_view_host(plan.h, p, 10, 0, 10, 0, far, None, None) == E
    assert L.sgz_overview_view_host(plan.h, p, 2 ** 31, 0, 10, 4, far, None, None) == E
    assert L.sgz_overview_view_host(plan.h, p, 10, 0, 10, 4, None, None, None) == E
    assert not b.any()
    with pytest.raises(api.SgzError):
        api.overview_view_columns(10, 4, 4, 3)


def test_stream_overview_calls_refuse_without_a_stream(buf):
    L = api.lib()
    b, p = buf
    E = api.SGZ_EINVAL
    cols = C.c_uint64(77)
    assert L.sgz_pcm_stream_feed_overview(None, p, 100, 2, 1, p, p, 10, C.byref(cols), None) == E and cols.value == 77
    assert L.sgz_pcm_stream_columns_for(None, 100, 2, 1) == 0 and L.sgz_pcm_stream_open_frames(None) == 0
    cfg = api.config_from_dict(config.spectrum_config(window_size=64, hop=16, axis_points=33))
    #                                               cfg pcm format src map nsamples k rgba peaks timing
    assert L.sgz_spectrogram_overview_pcm(None, p, api.PCM_S16, 2, None, 1000, 2, p, p, None) == E
    assert L.sgz_spectrogram_overview_pcm(C.byref(cfg), None, api.PCM_S16, 2, None, 1000, 2, p, p, None) == E
    assert L.sgz_spectrogram_overview_pcm(C.byref(cfg), p, api.PCM_S16, 2, None, 1000, 0, p, p, None) == E      # k == 0
    assert L.sgz_spectrogram_overview_pcm(C.byref(cfg), p, api.PCM_S16, 2, None, 1000, 2, None, None, None) == E  # both outputs NULL
    assert not b.any()


def test_view_kernels_in_the_code_object_without_scratch():
    import codeobj_report as cr
    lib = api.LIB_PATH
    api.lib()
    if not (os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("llvm tools not present")
    rows = cr.kernels(lib)
    for kernel in ("overviewViewKernel", "overviewViewSliceKernel", "overviewViewEmitKernel"):
        mine = [r for r in rows if kernel + "(" in r["demangled"]]
        assert len(mine) == 1, [r["demangled"] for r in mine]
        for r in mine:
            assert not r.get("private_segment_fixed_size", 0) and not r.get("vgpr_spill_count", 0) and not r.get("sgpr_spill_count", 0), r
