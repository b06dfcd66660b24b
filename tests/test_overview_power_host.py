"""The power overview (sgz.h, "The power overview"; csrc/overview_power.hip) without a GPU: the exports, the record's layout, the six kernels in
the built gfx950 code object (no scratch, no spill), the refusals every call makes before it touches the device (Phase and RSNT plans among
them), the host helpers sgz_overview_power_quantise / _fold / _readout against the restatement (tests/overview_power_ref.py) on the edge
values and on hand-made records, sgz_overview_power_levels against the oracle's dB map, and the restatement itself against a brute-force
loop in exact rational arithmetic.  Every comparison is on bytes or bit patterns; no tolerance anywhere."""
import ctypes as C
import math
import os
import struct
import sys
from fractions import Fraction

import numpy as np
import pytest

from signalizer_amd import api, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import overview_power_ref as opr  # noqa: E402

NAMES = ("sgz_stage_overview_power", "sgz_spectrogram_overview_power_device", "sgz_spectrogram_overview_power_host",
         "sgz_stage_overview_power_view", "sgz_overview_power_view_host", "sgz_overview_power_quantise", "sgz_overview_power_fold",
         "sgz_overview_power_readout", "sgz_overview_power_levels", "sgz_pcm_stream_feed_overview_power", "sgz_spectrogram_overview_power_pcm")
KERNELS = ("overviewPowerColumnsKernel", "overviewPowerSliceKernel", "overviewPowerEmitKernel", "overviewPowerViewKernel",
           "overviewPowerViewSliceKernel", "overviewPowerViewEmitKernel")
QNAN = 0x7FC00000
E, U = api.SGZ_EINVAL, api.SGZ_EUNSUPPORTED
Q_MOST = 2 ** 64 - 2 ** 11


def _small(**over):
    return config.spectrum_config(window_size=64, hop=16, axis_points=33, **over)


@pytest.fixture(scope="module")
def plan():
    return api.Plan(_small())                                                                      # host tables only: never uploaded here


@pytest.fixture(scope="module")
def buf():
    """a host block that stands for any non-NULL buffer: every call here is refused before a buffer is looked at"""
    b = np.zeros(8192, np.float64)
    return b, b.ctypes.data_as(C.c_void_p)


def _f(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def _bits_of(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def test_exports_exist():
    L = api.lib()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(L, name), name
    for name in ("overview_power_columns", "overview_power", "overview_power_view", "overview_power_levels"):
        assert callable(getattr(api.Plan, name))
    for name in ("feed_overview_power", "feed_overview_power_into"):
        assert callable(getattr(api.PcmStream, name))
    for name in ("overview_power_pcm", "overview_power_fold", "overview_power_readout", "overview_power_quantise"):
        assert callable(getattr(api, name))
    with open(os.path.join(ROOT, "include", "sgz.h")) as f:
        header = f.read()
    assert all(name + "(" in header for name in NAMES) and "#define SGZ_ABI_VERSION 5" in header
    assert "(5, later: the power overview" in header and "The power overview:" in header
    assert "(5, later: the mean overview" in header and "The mean overview:" in header                 # the earlier entries stay
    assert "neither reads nor advances the stream's decay state" in header
    assert L.sgz_abi_version() == 5


def test_the_record_layout_is_the_dtype():
    for d in (api.OVERVIEW_POWER_DTYPE, opr.DTYPE):
        assert d.itemsize == 32 and d.names == ("sum", "count", "nans", "lo", "hi")
        assert [d.fields[n][1] for n in d.names] == [0, 16, 20, 24, 28]
        assert d.fields["sum"][0] == np.dtype(("<u8", (2,)))
        assert [d.fields[n][0] for n in d.names[1:]] == [np.dtype("<u4"), np.dtype("<u4"), np.dtype("<f4"), np.dtype("<f4")]
    # ... and the library's own: a record written field by field through the dtype reads back through the readout and survives a 1:1 fold
    r = np.zeros(2, api.OVERVIEW_POWER_DTYPE)
    r[1] = ((3 << 60, 0), 3, 2, -1.0, 1.0)                                                          # three frames of |x| = 1
    assert r.tobytes()[32:] == struct.pack("<QQIIff", 3 << 60, 0, 3, 2, -1.0, 1.0)
    ms, rms, lo, hi = api.overview_power_readout(r[1:])
    assert (ms[0], rms[0], lo[0], hi[0]) == (1.0, 1.0, -1.0, 1.0)
    assert api.overview_power_fold(r[1:], 1).tobytes() == r[1:].tobytes()
    with open(os.path.join(ROOT, "include", "sgz.h")) as f:
        header = f.read()
    assert "static_assert(sizeof(sgz_overview_power_record) == 32" in header and "offsetof(sgz_overview_power_record, hi) == 28" in header


def test_power_kernels_in_the_code_object_without_scratch():
    import codeobj_report as cr
    lib = api.LIB_PATH
    api.lib()
    if not (os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("llvm tools not present")
    rows = cr.kernels(lib)
    for kernel in KERNELS:
        mine = [r for r in rows if kernel + "(" in r["demangled"]]
        assert len(mine) == 1, (kernel, [r["demangled"] for r in mine])
        for r in mine:
            assert not r.get("private_segment_fixed_size", 0) and not r.get("vgpr_spill_count", 0) and not r.get("sgpr_spill_count", 0), r
            assert not r.get("group_segment_fixed_size", 0), r                                       # no LDS


# ---- refusals before the device ---------------------------------------------------------------------------------------------------------------
def test_stage_call_refusals_before_the_device(plan, buf):
    L = api.lib()
    b, p = buf
    #                                           mapped frames k held flush slices carry rgba power levels stream
    assert L.sgz_stage_overview_power(None, p, 4, 2, 0, 1, 0, p, p, p, p, None) == E
    assert L.sgz_stage_overview_power(plan.h, None, 4, 2, 0, 1, 0, p, p, p, p, None) == E
    assert L.sgz_stage_overview_power(plan.h, p, 4, 0, 0, 1, 0, p, p, p, p, None) == E              # k == 0
    assert L.sgz_stage_overview_power(plan.h, p, 4, 2, 2, 1, 0, p, p, p, p, None) == E              # held >= k
    assert L.sgz_stage_overview_power(plan.h, p, 4, 1, 1, 1, 0, p, p, p, p, None) == E
    assert L.sgz_stage_overview_power(plan.h, p, 4, 2, 0, 1, 65, p, p, p, p, None) == E             # slices > 64
    assert L.sgz_stage_overview_power(plan.h, p, 4, 2, 0, 1, 0xffffffff, p, p, p, p, None) == E
    assert L.sgz_stage_overview_power(plan.h, p, 4, 2, 0, 1, 0, p, None, None, None, None) == E     # all three outputs NULL
    assert L.sgz_stage_overview_power(plan.h, p, 4, 2, 1, 1, 0, None, p, p, p, None) == E           # the carry is read
    assert L.sgz_stage_overview_power(plan.h, p, 3, 2, 0, 0, 0, None, p, p, p, None) == E           # the carry is written
    assert L.sgz_stage_overview_power(plan.h, p, 0, 2, 1, 1, 0, None, p, None, None, None) == E     # a flush of the held column reads it
    # nothing arrives and no column to flush: SGZ_OK before the plan is looked at any further (it stays without device tables)
    assert L.sgz_stage_overview_power(plan.h, p, 0, 2, 0, 1, 0, None, None, None, p, None) == api.SGZ_OK
    assert L.sgz_stage_overview_power(plan.h, p, 0, 3, 2, 0, 0, p, None, p, None, None) == api.SGZ_OK
    assert not b.any()


def test_render_refusals_before_the_device(plan, buf):
    L = api.lib()
    b, p = buf
    ch = (C.c_void_p * 2)(p, p)
    assert L.sgz_spectrogram_overview_power_device(None, p, 1024, 1024, 2, p, p, p, None) == E
    assert L.sgz_spectrogram_overview_power_device(plan.h, None, 1024, 1024, 2, p, p, p, None) == E
    assert L.sgz_spectrogram_overview_power_device(plan.h, p, 1024, 1024, 0, p, p, p, None) == E
    assert L.sgz_spectrogram_overview_power_device(plan.h, p, 1024, 1024, 2, None, None, None, None) == E
    assert L.sgz_spectrogram_overview_power_host(None, ch, 2, 1024, 2, p, p, p, None) == E
    assert L.sgz_spectrogram_overview_power_host(plan.h, None, 2, 1024, 2, p, p, p, None) == E
    assert L.sgz_spectrogram_overview_power_host(plan.h, ch, 2, 1024, 0, p, p, p, None) == E
    assert L.sgz_spectrogram_overview_power_host(plan.h, ch, 2, 1024, 2, None, None, None, None) == E
    assert L.sgz_spectrogram_overview_power_host(plan.h, ch, 3, 1024, 2, p, p, p, None) == E          # 2 * num_pairs channels, as the render
    assert L.sgz_spectrogram_overview_power_host(plan.h, (C.c_void_p * 2)(p, None), 2, 1024, 2, p, p, p, None) == E
    cfg = api.config_from_dict(_small())
    for args in ((None, p, api.PCM_S16, 2, None, 100, 2, p, p, p), (cfg, None, api.PCM_S16, 2, None, 100, 2, p, p, p),
                 (cfg, p, api.PCM_S16, 2, None, 100, 0, p, p, p), (cfg, p, api.PCM_S16, 2, None, 100, 2, None, None, None)):
        assert L.sgz_spectrogram_overview_power_pcm(C.byref(args[0]) if args[0] is not None else None, *args[1:], None) == E
    assert L.sgz_pcm_stream_feed_overview_power(None, p, 10, 2, 0, p, p, p, 10, None, None) == E
    assert not b.any()


@pytest.mark.parametrize("over", [dict(channel_mode=config.CH_PHASE), dict(algorithm=config.ALGO_RSNT)], ids=["phase", "rsnt"])
def test_phase_and_rsnt_plans_are_refused_before_the_device(buf, over):
    """the render, host and pcm calls: SGZ_EUNSUPPORTED from a plan that was never uploaded, nothing written"""
    L = api.lib()
    b, p = buf
    plan = api.Plan(_small(**over))
    ch = (C.c_void_p * 2)(p, p)
    assert L.sgz_spectrogram_overview_power_device(plan.h, p, 1024, 1024, 2, p, p, p, None) == U
    assert b"power overview" in L.sgz_last_error()
    assert L.sgz_spectrogram_overview_power_host(plan.h, ch, 2, 1024, 2, p, p, p, None) == U
    cfg = api.config_from_dict(_small(**over))
    assert L.sgz_spectrogram_overview_power_pcm(C.byref(cfg), p, api.PCM_S16, 2, None, 1000, 2, p, p, p, None) == U
    # the argument refusals come first, as on any plan
    assert L.sgz_spectrogram_overview_power_device(plan.h, p, 1024, 1024, 0, p, p, p, None) == E
    assert L.sgz_spectrogram_overview_power_host(plan.h, ch, 2, 1024, 2, None, None, None, None) == E
    assert not b.any()


def test_view_refusals_before_the_device(plan, buf):
    L = api.lib()
    b, p = buf
    base = b.ctypes.data
    #                                               power n x0 x1 out_columns slices rgba power_out levels stream
    assert L.sgz_stage_overview_power_view(None, p, 8, 0, 8, 4, 0, p, p, p, None) == E
    assert L.sgz_stage_overview_power_view(plan.h, None, 8, 0, 8, 4, 0, p, p, p, None) == E
    for n, x0, x1, cols in ((8, 3, 3, 4), (8, 5, 4, 4), (8, 0, 9, 4), (8, 0, 8, 0), (1 << 31, 0, 8, 4)):
        assert L.sgz_stage_overview_power_view(plan.h, p, n, x0, x1, cols, 0, None, None, C.c_void_p(base + (1 << 15)), None) == E
        assert L.sgz_overview_power_view_host(plan.h, p, n, x0, x1, cols, p, p, p, None) == E
    assert L.sgz_stage_overview_power_view(plan.h, p, 8, 0, 8, 4, 65, p, p, p, None) == E
    assert L.sgz_stage_overview_power_view(plan.h, p, 8, 0, 8, 4, 0, None, None, None, None) == E
    assert L.sgz_overview_power_view_host(None, p, 8, 0, 8, 4, p, p, p, None) == E
    assert L.sgz_overview_power_view_host(plan.h, None, 8, 0, 8, 4, p, p, p, None) == E
    assert L.sgz_overview_power_view_host(plan.h, p, 8, 0, 8, 4, None, None, None, None) == E
    # outputs that overlap the source range [x0, x1): one column is pairs * sides * P = 66 records of 32 bytes
    column = 66 * 32
    src0, src1 = base + 2 * column, base + 6 * column                                               # the range 2 .. 6 of n = 8
    far = C.c_void_p(base + 16 * column)
    for inside in (src0, src1 - 1, src0 + column + 5):
        q = C.c_void_p(inside - inside % 8)
        assert L.sgz_stage_overview_power_view(plan.h, p, 8, 2, 6, 2, 0, q, None, None, None) == E
        assert L.sgz_stage_overview_power_view(plan.h, p, 8, 2, 6, 2, 0, far, q, None, None) == E
        assert L.sgz_stage_overview_power_view(plan.h, p, 8, 2, 6, 2, 0, None, None, q, None) == E
    assert not b.any()


# ---- the quantiser ------------------------------------------------------------------------------------------------------------------------------
NAN_A, NAN_B = _f(0x7FC12345), _f(0xFFC00001)
INF = np.float32(np.inf)
EDGE = np.array([0.0, -0.0, _f(1), _f(0x80000001), _f(0x007FFFFF), _f(0x00800000), 2.0 ** -31, 2.0 ** -30, 2.0 ** -7, 1.0, _f(0x407FFFFF), 4.0,
                 1e30, INF, -INF, NAN_A, NAN_B, -1.0, -2.0 ** -30, -_f(0x407FFFFF), -4.0, -0.75, 3.0 * 2.0 ** -31, 1.5 * 2.0 ** -30], np.float32)


def _random_values(n, seed):
    """seeded floats over 12 decades, both signs"""
    rng = np.random.default_rng(seed)
    return (np.sign(rng.standard_normal(n)) * 10.0 ** rng.uniform(-10.5, 1.5, n)).astype(np.float32)


def _exact_q(v):
    """q by the definition in exact rational arithmetic (None for a NaN): rint of x^2 2^60, where a tie would show as a remainder of 1/2"""
    if v != v:
        return None
    if v in (float("inf"), float("-inf")):
        return Q_MOST
    u = Fraction(float(v)) ** 2 * 2 ** 60
    if u >= Q_MOST:
        return Q_MOST
    whole, rest = divmod(u, 1)
    assert rest != Fraction(1, 2), v                                                                # a tie cannot occur
    return int(whole) + (1 if rest > Fraction(1, 2) else 0)


def test_quantise_equals_the_restatement_on_the_edge_values_and_randoms():
    assert _bits_of(EDGE[10]) == 0x407FFFFF and float(EDGE[10]) == 3.999999761581421                # "3.9999998"
    for x in (EDGE, _random_values(10000, 5)):
        got = api.overview_power_quantise(x)
        want, nan = opr.quantise(x)
        assert [int(g) for g in got] == [int(w) for w in want]
        assert np.array_equal(nan, np.isnan(x))
    got = [int(g) for g in api.overview_power_quantise(EDGE)]
    assert got[:2] == [0, 0] and got[2] == 0 and got[4] == 0                                        # zeros and denormals: below the resolution
    assert got[6] == 0 and got[7] == 1 and got[22] == 2 and got[23] == 2                            # 2^-62 2^60 = 1/4 -> 0;  9/4 -> 2;  2.25 -> 2
    assert got[8] == 2 ** 46 and got[9] == 2 ** 60 and got[17] == 2 ** 60
    assert got[10] == (2 ** 24 - 1) ** 2 * 2 ** 16 and got[10] < Q_MOST                             # the last value below the clamp
    assert got[11] == Q_MOST and got[12] == Q_MOST and got[13] == Q_MOST and got[14] == Q_MOST and got[20] == Q_MOST
    assert got[15] == 0 and got[16] == 0                                                            # a NaN has no q
    L = api.lib()
    assert L.sgz_overview_power_quantise(None, 3, EDGE.ctypes.data_as(C.c_void_p)) == E and L.sgz_overview_power_quantise(None, 0, None) == api.SGZ_OK


def test_the_restatements_quantiser_equals_exact_rational_arithmetic():
    x = np.concatenate([EDGE, _random_values(3000, 9)])
    want, _ = opr.quantise(x)
    for v, w in zip(x, want):
        e = _exact_q(float(v))
        assert (0 if e is None else e) == int(w), float(v)


# ---- the host helpers against the restatement ---------------------------------------------------------------------------------------------------
GROUPS = [
    [NAN_A], [NAN_B, NAN_A, NAN_A],                                                                  # all NaN: empty records
    [np.float32(0.0), np.float32(-0.0)], [np.float32(-0.0)], [np.float32(-0.0), np.float32(-0.0), NAN_A],
    [np.float32(2.0)] * 5,                                                                          # 5 * 2^62: the sum crosses 2^64
    [INF], [-INF, np.float32(4.0), np.float32(1e30)], [INF, -INF, np.float32(0.25), NAN_B],
    [np.float32(2.0 ** -31), np.float32(2.0 ** -30), np.float32(3.0 * 2.0 ** -31)],
    [_f(0x407FFFFF), -_f(0x407FFFFF), np.float32(1.0)],
    [np.float32(1e-45), np.float32(-1e-45), np.float32(1e-30)],
    [np.float32(0.999), np.float32(0.25), np.float32(0.5), np.float32(-3.75)],
]


def _check_helpers(records):
    """fold and readout of the library == the restatement's, on records [n][width]"""
    n = records.shape[0]
    ms, rms, lo, hi = api.overview_power_readout(records)
    assert np.array_equal(rms.view(np.uint32), opr.rms_bits(records))
    want_ms = opr.mean_square_scaled(records) * 2.0 ** -60
    ok = records["count"] > 0
    assert np.array_equal(ms[ok].view(np.uint64), want_ms[ok].view(np.uint64)) and np.isnan(ms[~ok]).all()
    assert np.array_equal(lo.view(np.uint32), records["lo"].view(np.uint32)) and np.array_equal(hi.view(np.uint32), records["hi"].view(np.uint32))
    for x0, x1 in ((0, n), (1, n), (0, n - 1), (n // 3, n - n // 4)):
        if x0 >= x1:
            continue
        for cols in (1, 2, 3, x1 - x0, x1 - x0 + 5):
            got = api.overview_power_fold(records, cols, x0, x1)
            assert opr.same(got, opr.view_of(records, x0, x1, cols)), (n, x0, x1, cols)
            assert np.array_equal(api.overview_power_readout(got)[1].view(np.uint32), opr.rms_bits(got))


def test_fold_and_readout_on_hand_made_records():
    # every group as one column of one-frame records, and every group folded to one record as a source column of its own
    per_frame = [opr.records_of(np.array(g, np.float32)) for g in GROUPS]
    folded = np.stack([opr.fold(r) for r in per_frame])
    assert int(folded[0]["count"]) == 0 and folded[0:1]["hi"].view(np.uint32)[0] == QNAN and folded[0:1]["lo"].view(np.uint32)[0] == QNAN
    assert folded[2:3]["lo"].view(np.uint32)[0] == 0x80000000 and folded[2:3]["hi"].view(np.uint32)[0] == 0             # -0 below +0
    assert [int(w) for w in folded[5]["sum"]] == [2 ** 62, 1] and int(folded[5]["count"]) == 5     # 5 * 2^62 = 2^64 + 2^62
    assert int(opr.sums(folded[7:8])[0]) == 3 * Q_MOST and int(opr.sums(folded[8:9])[0]) == 2 * Q_MOST + 2 ** 56
    assert [int(v) for v in opr.sums(per_frame[9])] == [0, 1, 2]
    for r in per_frame:
        _check_helpers(r.reshape(-1, 1))
        got = api.overview_power_fold(r.reshape(-1, 1), 1)
        assert opr.same(got, opr.fold(r).reshape(1, 1))
    _check_helpers(folded.reshape(-1, 1))
    # the rms of the column that crossed 2^64 is 2, of an empty one the quiet NaN, of the clamped ones 4 (to the float below 2^64's root)
    _, rms, _, _ = api.overview_power_readout(folded)
    assert rms[5] == 2.0 and rms.view(np.uint32)[0] == QNAN and rms.view(np.uint32)[1] == QNAN and rms[6] == 4.0 and rms[7] == 4.0
    L = api.lib()
    p = folded.ctypes.data_as(C.c_void_p)
    f = np.zeros(16, np.float64).ctypes.data_as(C.c_void_p)
    assert L.sgz_overview_power_readout(None, 2, f, f, f, f) == E and L.sgz_overview_power_readout(p, 2, None, None, None, None) == E
    for only in range(4):
        assert L.sgz_overview_power_readout(p, 2, *[f if i == only else None for i in range(4)]) == api.SGZ_OK


def test_k1_rms_is_the_magnitude_bit_for_bit():
    """k == 1 and 2^-7 <= |x| < 4: rms == |x|"""
    rng = np.random.default_rng(3)
    x = np.concatenate([np.float32([2.0 ** -7, -(2.0 ** -7), _f(0x407FFFFF), -_f(0x407FFFFF), 1.0]),
                        (np.sign(rng.standard_normal(5000)) * 2.0 ** rng.uniform(-7, 2, 5000)).astype(np.float32)])
    x = x[(np.abs(x) >= 2.0 ** -7) & (np.abs(x) < 4.0)]
    _, rms, _, _ = api.overview_power_readout(opr.records_of(x))
    assert np.array_equal(rms.view(np.uint32), np.abs(x).view(np.uint32))
    assert np.array_equal(opr.rms_bits(opr.records_of(x)), np.abs(x).view(np.uint32))


def test_readout_pins_the_conversions_of_the_two_words():
    r = opr.empty(6)
    words = [(2 ** 53 + 1, 0), (2 ** 64 - 1, 0), (2 ** 63 + 2 ** 10, 2 ** 31), (2 ** 64 - 1, 2 ** 32 - 1), (1, 1), (7, 0)]
    counts = [1, 3, 2 ** 31, 2 ** 32 - 1, 1, 3]
    r["sum"], r["count"] = words, counts
    r["lo"] = r["hi"] = np.float32(1.0)
    ms, rms, _, _ = api.overview_power_readout(r)
    assert np.array_equal(rms.view(np.uint32), opr.rms_bits(r))
    assert np.array_equal(ms.view(np.uint64), (opr.mean_square_scaled(r) * 2.0 ** -60).view(np.uint64))
    assert ms[0] == 2.0 ** -7 and ms[4] == 16.0                              # (double)(2^53 + 1) ties to even; 2^64 + 1 rounds to 2^64
    assert ms[1] == (2.0 ** 64 / 3.0) * 2.0 ** -60                           # (double)(2^64 - 1) = 2^64


def test_fold_at_the_count_limit():
    r = opr.empty((4, 2))
    r["count"][:, 0] = [2 ** 32 - 2, 1, 2 ** 32 - 2, 2]
    r["nans"][:, 1] = [2 ** 31, 2 ** 31 - 1, 1, 0]
    big = Q_MOST * (2 ** 32 - 2)
    r["sum"][:, 0] = [(big & opr.MASK64, big >> 64), (Q_MOST, 0), (5, 0), (6, 0)]
    r["lo"][:, 0] = r["hi"][:, 0] = 1.0
    ok = api.overview_power_fold(r, 1, 0, 2)                                                       # exactly 2^32 - 1 of each: allowed
    assert opr.same(ok, opr.view_of(r, 0, 2, 1)) and int(ok["count"][0, 0]) == 2 ** 32 - 1 and int(ok["nans"][0, 1]) == 2 ** 32 - 1
    assert int(opr.sums(ok)[0, 0]) == Q_MOST * (2 ** 32 - 1) < 2 ** 96
    out = np.full(4 * 2 * 32, 0x5A, np.uint8)
    L = api.lib()
    p = r.ctypes.data_as(C.c_void_p)
    o = out.ctypes.data_as(C.c_void_p)
    assert L.sgz_overview_power_fold(p, 4, 2, 0, 3, 1, o) == E and b"2^32 - 1" in L.sgz_last_error()       # the counts and the nans pass the limit
    assert (out == 0x5A).all()
    assert L.sgz_overview_power_fold(p, 4, 2, 1, 3, 2, o) == api.SGZ_OK and not (out[:128] == 0x5A).all()
    out[:] = 0x5A
    assert L.sgz_overview_power_fold(p, 4, 2, 0, 4, 2, o) == E                                      # column 0 = sources 0 .. 1 fits, column 1 = 2 .. 3 does not
    with pytest.raises(OverflowError):
        opr.view_of(r, 0, 3, 1)
    for args in ((None, 3, 2, 0, 3, 1, o), (p, 3, 2, 0, 3, 1, None), (p, 3, 0, 0, 3, 1, o), (p, 3, 2, 2, 2, 1, o), (p, 3, 2, 0, 4, 1, o), (p, 3, 2, 0, 3, 0, o)):
        assert L.sgz_overview_power_fold(*args) == E
    assert (out == 0x5A).all()


# ---- the levels against the oracle's dB map -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over", [dict(), dict(channel_mode=config.CH_LEFT, num_pairs=2), dict(channel_mode=config.CH_MIDSIDE, slope_a=3.0, slope_b=1.5)],
                         ids=["separate", "left_two_pairs", "midside_sloped"])
def test_levels_equal_the_oracles_db_map_at_the_rms_values(oracle, over):
    cfg = _small(**over)
    plan = api.Plan(cfg)
    params = oracle.params_from_dict(cfg)
    Cn, S, P = plan.C, plan.sides, plan.P
    rng = np.random.default_rng(21)
    x = (10.0 ** rng.uniform(-9, 0.5, (9, 3, Cn, S, P))).astype(np.float32)                        # 3 columns of 9 frames
    x[:, 1, 0, 0, 4] = np.nan                                                                       # an empty record
    x[:, 2, 0, 0, 5] = 0.0                                                                          # rms 0: the lower clip
    records = np.stack([opr.fold(opr.records_of(x[:, c])) for c in range(3)])
    rms = opr.rms_bits(records).view(np.float32)
    got = plan.overview_power_levels(records)
    assert got.shape == (3, Cn, S, P)
    for c in range(3):
        column = np.where(records[c]["count"] == 0, np.float32(0), rms[c])[None]                   # one frame [1][C][sides][P] from a zero state
        _, lines = oracle.decay_colour(params, column, want_lines=True)
        for s in range(S):
            want = np.ascontiguousarray(lines[0, :, 0, :].real if s == 0 else lines[0, :, 0, :].imag)
            ok = records[c]["count"][:, s] > 0
            assert np.array_equal(got[c, :, s][ok].view(np.uint32), want[ok].view(np.uint32)), (c, s)
            assert (got[c, :, s][~ok].view(np.uint32) == QNAN).all()
    assert got.view(np.uint32)[1, 0, 0, 4] == QNAN and got[2, 0, 0, 5] == np.float32(cfg["clip_db"])
    # one column without the leading axis
    assert np.array_equal(plan.overview_power_levels(records[0]).view(np.uint32), got[0].view(np.uint32))
    L = api.lib()
    assert L.sgz_overview_power_levels(None, records.ctypes.data_as(C.c_void_p), 3, got.ctypes.data_as(C.c_void_p)) == E
    assert L.sgz_overview_power_levels(plan.h, None, 3, got.ctypes.data_as(C.c_void_p)) == E
    assert L.sgz_overview_power_levels(plan.h, records.ctypes.data_as(C.c_void_p), 3, None) == E


# ---- the restatement against a brute-force loop --------------------------------------------------------------------------------------------------
def _brute_key(v):
    b = _bits_of(v)
    return b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)


def _brute_column(values, carry):
    """one record's worth of one column: (sum, count, nans, lo key, hi key) of `values` behind an optional carried tuple, in Python ints"""
    s, c, n, lo, hi = carry if carry is not None else (0, 0, 0, None, None)
    for v in values:
        if v != v:
            n += 1
            continue
        s, c = s + _exact_q(v), c + 1
        key = _brute_key(v)
        lo = key if lo is None or key < lo else lo
        hi = key if hi is None or key > hi else hi
    return s, c, n, lo, hi


def _as_tuple(rec):
    lo, hi = (np.array([rec[f]], np.float32).view(np.uint32)[0] for f in ("lo", "hi"))
    count = int(rec["count"])
    return (int(rec["sum"][0]) | (int(rec["sum"][1]) << 64), count, int(rec["nans"]), _brute_key(rec["lo"]) if count else None,
            _brute_key(rec["hi"]) if count else None, int(lo), int(hi))


def test_the_restatements_columns_equal_a_brute_force_loop():
    rng = np.random.default_rng(17)
    x = (10.0 ** rng.uniform(-8, 0.7, (23, 2, 6))).astype(np.float32) * np.sign(rng.standard_normal((23, 2, 6))).astype(np.float32)
    x[rng.random(x.shape) < 0.2] = np.nan
    x[3:9, 0, 2] = np.nan                                                                         # whole columns of NaN
    x[:, 1, 0] = rng.choice(np.float32([0.0, -0.0, np.inf, -np.inf, 4.0, -2.0, 2.0 ** -31, 3 * 2.0 ** -31]), 23)
    x[:, 1, 1] = 2.0                                                                              # carries into the high word at five frames
    for k in (1, 2, 5, 7, 23, 26):
        for held, flush in ((0, True), (0, False), (min(3, k - 1), True), (k - 1, False)):
            carry = opr.fold(opr.records_of(x[:max(held, 1), ::-1, ::-1].copy())) if held else None
            got, open_rec, left = opr.columns_of(x, k, held, carry, flush)
            assert (got.shape[0], left) == api.overview_step(k, held, 23, flush)
            columns = list(got) + ([open_rec] if open_rec is not None else [])
            for c, rec in enumerate(columns):
                a, b = max(c * k - held, 0), min((c + 1) * k - held, 23)
                for p in range(2):
                    for i in range(6):
                        cy = _as_tuple(carry[p, i])[:5] if held and c == 0 else None
                        s, n, nn, lo, hi = _brute_column([float(v) for v in x[a:b, p, i]], cy)
                        t = _as_tuple(rec[p, i])
                        assert t[:5] == (s, n, nn, lo, hi), (k, held, flush, c, p, i)
                        if n == 0:
                            assert t[5] == QNAN and t[6] == QNAN
                        # the rms' bits from Python's own floats: int -> float conversions, the division and the root are correctly rounded
                        if n:
                            S = float(s >> 64) * 2.0 ** 64 + float(s & opr.MASK64)
                            assert int(opr.rms_bits(rec[p:p + 1, i:i + 1])[0, 0]) == _bits_of(np.float32(math.sqrt(S / float(n)) * 2.0 ** -30))
                        else:
                            assert int(opr.rms_bits(rec[p:p + 1, i:i + 1])[0, 0]) == QNAN
    assert int(opr.sums(opr.columns_of(x, 23)[0])[0, 1, 1]) == 23 * 2 ** 62 > 2 ** 64


def test_columns_with_a_carry_equal_columns_of_the_whole_and_folds_nest():
    rng = np.random.default_rng(11)
    x = (10.0 ** rng.uniform(-6, 0.6, (24, 2, 5))).astype(np.float32)
    x[rng.random(x.shape) < 0.2] = np.nan
    for k in (1, 2, 5, 7, 24, 26):
        whole, none, left = opr.columns_of(x, k)
        assert none is None and left == 0 and whole.shape[0] == -(-24 // k)
        for cut in (1, 6, 10, 23):
            a, carry, held = opr.columns_of(x[:cut], k, flush=False)
            assert held == cut % k and (carry is None) == (held == 0)
            b, none, _ = opr.columns_of(x[cut:], k, held=held, carry=carry)
            assert opr.same(np.concatenate([a, b]), whole), (k, cut)
    # a fold of a fold is the direct fold where boundaries nest: 24 frames -> columns of 2 -> 12 -> 4 -> 1, through the library and the restatement
    fine = opr.columns_of(x, 2)[0]
    for cols in (12, 6, 4, 3, 2, 1):
        direct = opr.columns_of(x, 24 // cols)[0]
        assert opr.same(opr.view_of(fine, 0, 12, cols), direct)
        assert opr.same(api.overview_power_fold(fine, cols), direct)
        for again in (c for c in (1, 2, 3) if cols % c == 0):
            assert opr.same(api.overview_power_fold(api.overview_power_fold(fine, cols), again), opr.columns_of(x, 24 // again)[0]), (cols, again)
    # ... and over a sub-range
    assert opr.same(api.overview_power_fold(fine, 2, 2, 10), opr.columns_of(x[4:20], 8)[0])
