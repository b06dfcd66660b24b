"""The mean overview (sgz.h, "The mean overview"; csrc/overview_stats.hip) without a GPU: the exports, the record's layout, the six kernels in
the built gfx950 code object (no scratch, no spill), the refusals every call makes before it touches the device, the host helpers
sgz_overview_stats_fold / _readout against the numpy restatement (tests/overview_stats_ref.py) on hand-made records, and the restatement
itself against a brute-force Python loop.  Every comparison is on bytes or bit patterns; no tolerance anywhere."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import overview_ref as ov  # noqa: E402
import overview_stats_ref as osr  # noqa: E402

NAMES = ("sgz_stage_overview_stats", "sgz_spectrogram_overview_stats_device", "sgz_spectrogram_overview_stats_host",
         "sgz_stage_overview_stats_view", "sgz_overview_stats_view_host", "sgz_overview_stats_fold", "sgz_overview_stats_readout",
         "sgz_pcm_stream_feed_overview_stats", "sgz_spectrogram_overview_stats_pcm")
KERNELS = ("overviewStatsColumnsKernel", "overviewStatsSliceKernel", "overviewStatsEmitKernel", "overviewStatsViewKernel",
           "overviewStatsViewSliceKernel", "overviewStatsViewEmitKernel")
QNAN = 0x7FC00000
E = api.SGZ_EINVAL


@pytest.fixture(scope="module")
def plan():
    return api.Plan(config.spectrum_config(window_size=64, hop=16, axis_points=33))        # host tables only: never uploaded here


@pytest.fixture(scope="module")
def buf():
    """a host block that stands for any non-NULL buffer: every call here is refused before a buffer is looked at"""
    b = np.zeros(4096, np.float64)
    return b, b.ctypes.data_as(C.c_void_p)


def test_exports_exist():
    L = api.lib()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(L, name), name
    for name in ("overview_stats_columns", "overview_stats", "overview_stats_view"):
        assert callable(getattr(api.Plan, name))
    for name in ("feed_overview_stats", "feed_overview_stats_into"):
        assert callable(getattr(api.PcmStream, name))
    for name in ("overview_stats_pcm", "overview_stats_fold", "overview_stats_readout"):
        assert callable(getattr(api, name))
    with open(os.path.join(ROOT, "include", "sgz.h")) as f:
        header = f.read()
    assert all(name + "(" in header for name in NAMES) and "#define SGZ_ABI_VERSION 5" in header
    assert "(5, later: the mean overview" in header and "The mean overview:" in header
    assert L.sgz_abi_version() == 5


def test_the_record_layout_is_the_dtype():
    for d in (api.OVERVIEW_STAT_DTYPE, osr.DTYPE):
        assert d.itemsize == 24 and d.names == ("sum", "count", "nans", "lo", "hi")
        assert [d.fields[n][1] for n in d.names] == [0, 8, 12, 16, 20]
        assert [d.fields[n][0] for n in d.names] == [np.dtype("<i8"), np.dtype("<u4"), np.dtype("<u4"), np.dtype("<f4"), np.dtype("<f4")]
    # ... and the library's own: a record written field by field through the dtype reads back through the readout and survives a 1:1 fold
    r = np.zeros(2, api.OVERVIEW_STAT_DTYPE)
    r[1] = (-(5 << 20), 4, 3, -2.5, 1.5)
    assert r.tobytes()[24:] == struct.pack("<qIIff", -(5 << 20), 4, 3, -2.5, 1.5)
    mean, lo, hi = api.overview_stats_readout(r[1:])
    assert (mean[0], lo[0], hi[0]) == (-1.25, -2.5, 1.5)
    assert api.overview_stats_fold(r[1:], 1).tobytes() == r[1:].tobytes()
    with open(os.path.join(ROOT, "include", "sgz.h")) as f:
        header = f.read()
    assert "static_assert(sizeof(sgz_overview_stat_record) == 24" in header and "offsetof(sgz_overview_stat_record, hi) == 20" in header


def test_stats_kernels_in_the_code_object_without_scratch():
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


# ---- refusals before the device ---------------------------------------------------------------------------------------------------------------
def test_stage_call_refusals_before_the_device(plan, buf):
    L = api.lib()
    b, p = buf
    #                                            lines frames k held flush slices carry rgba stats means stream
    assert L.sgz_stage_overview_stats(None, p, 4, 2, 0, 1, 0, p, p, p, p, None) == E
    assert L.sgz_stage_overview_stats(plan.h, None, 4, 2, 0, 1, 0, p, p, p, p, None) == E
    assert L.sgz_stage_overview_stats(plan.h, p, 4, 0, 0, 1, 0, p, p, p, p, None) == E              # k == 0
    assert L.sgz_stage_overview_stats(plan.h, p, 4, 2, 2, 1, 0, p, p, p, p, None) == E              # held >= k
    assert L.sgz_stage_overview_stats(plan.h, p, 4, 1, 1, 1, 0, p, p, p, p, None) == E
    assert L.sgz_stage_overview_stats(plan.h, p, 4, 2, 0, 1, 65, p, p, p, p, None) == E             # slices > 64
    assert L.sgz_stage_overview_stats(plan.h, p, 4, 2, 0, 1, 0xffffffff, p, p, p, p, None) == E
    assert L.sgz_stage_overview_stats(plan.h, p, 4, 2, 0, 1, 0, p, None, None, None, None) == E     # all three outputs NULL
    assert L.sgz_stage_overview_stats(plan.h, p, 4, 2, 1, 1, 0, None, p, p, p, None) == E           # the carry is read
    assert L.sgz_stage_overview_stats(plan.h, p, 3, 2, 0, 0, 0, None, p, p, p, None) == E           # the carry is written
    assert L.sgz_stage_overview_stats(plan.h, p, 0, 2, 1, 1, 0, None, p, None, None, None) == E     # a flush of the held column reads it
    # nothing arrives and no column to flush: SGZ_OK before the plan is looked at any further (it stays without device tables)
    assert L.sgz_stage_overview_stats(plan.h, p, 0, 2, 0, 1, 0, None, None, None, p, None) == api.SGZ_OK
    assert L.sgz_stage_overview_stats(plan.h, p, 0, 3, 2, 0, 0, p, None, p, None, None) == api.SGZ_OK
    assert not b.any()


def test_render_refusals_before_the_device(plan, buf):
    L = api.lib()
    b, p = buf
    ch = (C.c_void_p * 2)(p, p)
    assert L.sgz_spectrogram_overview_stats_device(None, p, 1024, 1024, 2, p, p, p, None, None) == E
    assert L.sgz_spectrogram_overview_stats_device(plan.h, None, 1024, 1024, 2, p, p, p, None, None) == E
    assert L.sgz_spectrogram_overview_stats_device(plan.h, p, 1024, 1024, 0, p, p, p, None, None) == E
    assert L.sgz_spectrogram_overview_stats_device(plan.h, p, 1024, 1024, 2, None, None, None, None, None) == E
    assert L.sgz_spectrogram_overview_stats_host(None, ch, 2, 1024, 2, p, p, p, None) == E
    assert L.sgz_spectrogram_overview_stats_host(plan.h, None, 2, 1024, 2, p, p, p, None) == E
    assert L.sgz_spectrogram_overview_stats_host(plan.h, ch, 2, 1024, 0, p, p, p, None) == E
    assert L.sgz_spectrogram_overview_stats_host(plan.h, ch, 2, 1024, 2, None, None, None, None) == E
    assert L.sgz_spectrogram_overview_stats_host(plan.h, ch, 3, 1024, 2, p, p, p, None) == E          # 2 * num_pairs channels, as the render
    assert L.sgz_spectrogram_overview_stats_host(plan.h, (C.c_void_p * 2)(p, None), 2, 1024, 2, p, p, p, None) == E
    cfg = api.config_from_dict(config.spectrum_config(window_size=64, hop=16, axis_points=33))
    for args in ((None, p, api.PCM_S16, 2, None, 100, 2, p, p, p), (cfg, None, api.PCM_S16, 2, None, 100, 2, p, p, p),
                 (cfg, p, api.PCM_S16, 2, None, 100, 0, p, p, p), (cfg, p, api.PCM_S16, 2, None, 100, 2, None, None, None)):
        assert L.sgz_spectrogram_overview_stats_pcm(C.byref(args[0]) if args[0] is not None else None, *args[1:], None) == E
    assert L.sgz_pcm_stream_feed_overview_stats(None, p, 10, 2, 0, p, p, p, 10, None, None) == E
    assert not b.any()


def test_view_refusals_before_the_device(plan, buf):
    L = api.lib()
    b, p = buf
    base = b.ctypes.data
    #                                               stats n x0 x1 out_columns slices rgba stats_out means stream
    assert L.sgz_stage_overview_stats_view(None, p, 8, 0, 8, 4, 0, p, p, p, None) == E
    assert L.sgz_stage_overview_stats_view(plan.h, None, 8, 0, 8, 4, 0, p, p, p, None) == E
    for n, x0, x1, cols in ((8, 3, 3, 4), (8, 5, 4, 4), (8, 0, 9, 4), (8, 0, 8, 0), (1 << 31, 0, 8, 4)):
        assert L.sgz_stage_overview_stats_view(plan.h, p, n, x0, x1, cols, 0, None, None, C.c_void_p(base + (1 << 14)), None) == E
        assert L.sgz_overview_stats_view_host(plan.h, p, n, x0, x1, cols, p, p, p, None) == E
    assert L.sgz_stage_overview_stats_view(plan.h, p, 8, 0, 8, 4, 65, p, p, p, None) == E
    assert L.sgz_stage_overview_stats_view(plan.h, p, 8, 0, 8, 4, 0, None, None, None, None) == E
    assert L.sgz_overview_stats_view_host(None, p, 8, 0, 8, 4, p, p, p, None) == E
    assert L.sgz_overview_stats_view_host(plan.h, None, 8, 0, 8, 4, p, p, p, None) == E
    assert L.sgz_overview_stats_view_host(plan.h, p, 8, 0, 8, 4, None, None, None, None) == E
    # outputs that overlap the source range [x0, x1): one column is pairs * P = 33 records of 24 bytes
    column = 33 * 24
    src0, src1 = base + 2 * column, base + 6 * column                                               # the range 2 .. 6 of n = 8
    far = C.c_void_p(base + 16 * column)
    for inside in (src0, src1 - 1, src0 + column + 5):
        q = C.c_void_p(inside - inside % 8)
        assert L.sgz_stage_overview_stats_view(plan.h, p, 8, 2, 6, 2, 0, q, None, None, None) == E
        assert L.sgz_stage_overview_stats_view(plan.h, p, 8, 2, 6, 2, 0, far, q, None, None) == E
        assert L.sgz_stage_overview_stats_view(plan.h, p, 8, 2, 6, 2, 0, None, None, q, None) == E
    assert not b.any()


# ---- the host helpers against the restatement ---------------------------------------------------------------------------------------------------
def _f(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


NAN_A, NAN_B = _f(0x7FC12345), _f(0xFFC00001)
INF = np.float32(np.inf)
HALF = np.float32(2.0 ** -21)                                                                     # q's tie: x 2^20 = 0.5
GROUPS = [
    [NAN_A], [NAN_B, NAN_A, NAN_A],                                                               # all NaN
    [np.float32(0.0), np.float32(-0.0)], [np.float32(-0.0)], [np.float32(-0.0), np.float32(-0.0), NAN_A],
    [INF], [-INF], [INF, -INF], [INF, -INF, np.float32(0.25), NAN_B],                             # both infinities cancel
    [np.float32(2047.9999), np.float32(2048.0), np.float32(2048.5), np.float32(3e38)],            # at and beyond +2048
    [np.float32(-2047.9999), np.float32(-2048.0), np.float32(-1e30)],
    [HALF, 3 * HALF, 5 * HALF, -HALF, -3 * HALF],                                                 # ties of rint: 0, 2, 2, -0, -2
    [np.float32(1e-45), np.float32(-1e-45), np.float32(1e-30)],
    [np.float32(0.999), np.float32(0.25), np.float32(0.5), np.float32(-3.75)],
]


def _check_helpers(records):
    """fold and readout of the library == the restatement's, on records [n][width]"""
    n = records.shape[0]
    mean, lo, hi = api.overview_stats_readout(records)
    assert np.array_equal(mean.view(np.uint32), osr.mean_bits(records))
    assert np.array_equal(lo.view(np.uint32), records["lo"].view(np.uint32)) and np.array_equal(hi.view(np.uint32), records["hi"].view(np.uint32))
    for x0, x1 in ((0, n), (1, n), (0, n - 1), (n // 3, n - n // 4)):
        if x0 >= x1:
            continue
        for cols in (1, 2, 3, x1 - x0, x1 - x0 + 5):
            got = api.overview_stats_fold(records, cols, x0, x1)
            assert osr.same(got, osr.view_of(records, x0, x1, cols)), (n, x0, x1, cols)
            assert np.array_equal(api.overview_stats_readout(got)[0].view(np.uint32), osr.mean_bits(got))


def test_fold_and_readout_on_hand_made_records():
    # every group as one column of one-frame records, and every group folded to one record as a source column of its own
    per_frame = [osr.records_of(np.array(g, np.float32)) for g in GROUPS]
    folded = np.stack([osr.fold(r) for r in per_frame])
    assert int(folded[7]["sum"]) == 0 and int(folded[7]["count"]) == 2                            # [inf, -inf]: the q cancel
    assert int(folded[0]["count"]) == 0 and folded[0:1]["hi"].view(np.uint32)[0] == QNAN and folded[0:1]["lo"].view(np.uint32)[0] == QNAN
    assert folded[2:3]["lo"].view(np.uint32)[0] == 0x80000000 and folded[2:3]["hi"].view(np.uint32)[0] == 0             # -0 below +0
    assert int(folded[9]["sum"]) == 2147483520 + 3 * (2 ** 31 - 1)
    assert [int(q) for q in per_frame[11]["sum"]] == [0, 2, 2, 0, -2]
    for r in per_frame:
        _check_helpers(r.reshape(-1, 1))
        got = api.overview_stats_fold(r.reshape(-1, 1), 1)
        assert osr.same(got, osr.fold(r).reshape(1, 1))
    _check_helpers(folded.reshape(-1, 1))
    _check_helpers(folded.reshape(-1, 2))
    # the mean's bits on the cancelling column and on an all-NaN one
    mean, _, _ = api.overview_stats_readout(folded)
    assert mean.view(np.uint32)[7] == 0 and mean.view(np.uint32)[0] == QNAN and mean.view(np.uint32)[1] == QNAN


def test_readout_pins_the_int64_to_double_rounding():
    r = osr.empty(8)
    sums = [2 ** 53 + 1, 2 ** 53 + 3, -(2 ** 53 + 1), 2 ** 62 + 2 ** 9 + 1, (2 ** 31 - 1) * (2 ** 32 - 1), -(2 ** 31 - 1) * (2 ** 32 - 1), 2 ** 53 + 2, 7]
    counts = [1, 3, 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 3]
    r["sum"], r["count"] = sums, counts
    r["lo"] = r["hi"] = np.float32(1.0)
    mean, _, _ = api.overview_stats_readout(r)
    assert np.array_equal(mean.view(np.uint32), osr.mean_bits(r))
    # (double)(2^53 + 1) ties to even, 2^53: the mean of that record is exactly 2^33, and 2^53 + 3 goes up to 2^53 + 4
    assert float(mean[0]) == 2.0 ** 33 and float(mean[2]) == -(2.0 ** 33)
    want = np.float32(np.float64(2 ** 53 + 4) / np.float64(3) * 2.0 ** -20)
    assert mean.view(np.uint32)[1] == np.array([want]).view(np.uint32)[0]
    assert float(mean[4]) == float(np.float32(2047.9999990463257)) and float(mean[5]) == -float(mean[4])


def test_fold_at_the_count_limit():
    r = osr.empty((4, 2))
    r["count"][:, 0] = [2 ** 32 - 2, 1, 2 ** 32 - 2, 2]
    r["nans"][:, 1] = [2 ** 31, 2 ** 31 - 1, 1, 0]
    r["sum"][:, 0] = [(2 ** 31 - 1) * (2 ** 32 - 2), 2 ** 31 - 1, 5, 6]
    r["lo"][:, 0] = r["hi"][:, 0] = 1.0
    ok = api.overview_stats_fold(r, 1, 0, 2)                                                       # exactly 2^32 - 1 of each: allowed
    assert osr.same(ok, osr.view_of(r, 0, 2, 1)) and int(ok["count"][0, 0]) == 2 ** 32 - 1 and int(ok["nans"][0, 1]) == 2 ** 32 - 1
    assert int(ok["sum"][0, 0]) == (2 ** 31 - 1) * (2 ** 32 - 1)
    out = np.full(4 * 2 * 24, 0x5A, np.uint8)
    L = api.lib()
    p = r.ctypes.data_as(C.c_void_p)
    o = out.ctypes.data_as(C.c_void_p)
    assert L.sgz_overview_stats_fold(p, 4, 2, 0, 3, 1, o) == E and b"2^32 - 1" in L.sgz_last_error()       # the counts and the nans pass the limit
    assert L.sgz_overview_stats_fold(p, 4, 2, 1, 3, 2, o) == api.SGZ_OK and not (out[:96] == 0x5A).all()
    out[:] = 0x5A
    assert L.sgz_overview_stats_fold(p, 4, 2, 0, 4, 2, o) == E                                      # column 0 = sources 0 .. 1 fits, column 1 = 2 .. 3 does not
    with pytest.raises(OverflowError):
        osr.view_of(r, 0, 3, 1)
    for args in ((None, 3, 2, 0, 3, 1, o), (p, 3, 2, 0, 3, 1, None), (p, 3, 0, 0, 3, 1, o), (p, 3, 2, 2, 2, 1, o), (p, 3, 2, 0, 4, 1, o), (p, 3, 2, 0, 3, 0, o)):
        assert L.sgz_overview_stats_fold(*args) == E
    assert (out == 0x5A).all()
    f = np.zeros(4, np.float32).ctypes.data_as(C.c_void_p)
    assert L.sgz_overview_stats_readout(None, 2, f, f, f) == E and L.sgz_overview_stats_readout(p, 2, None, None, None) == E
    assert L.sgz_overview_stats_readout(p, 2, None, f, None) == api.SGZ_OK


# ---- the restatement against a brute-force loop --------------------------------------------------------------------------------------------------
def _bits_of(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def _brute_q(v):
    """Python ints and floats only; round() of a float is ties-to-even on the exact value"""
    t = float(v) * 1048576.0
    if t >= 2147483647.0:
        return 2147483647
    if t <= -2147483647.0:
        return -2147483647
    return round(t)


def _brute_key(v):
    b = _bits_of(v)
    return b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)


def _brute_column(values, carry):
    """one (pair, pixel) of one column: (sum, count, nans, lo bits, hi bits) of `values` behind an optional carried tuple"""
    s, c, n, lo, hi = carry if carry is not None else (0, 0, 0, None, None)
    for v in values:
        if v != v:
            n += 1
            continue
        s, c = s + _brute_q(v), c + 1
        key = _brute_key(v)
        lo = key if lo is None or key < lo else lo
        hi = key if hi is None or key > hi else hi
    return s, c, n, lo, hi


def _as_tuple(rec):
    lo, hi = (np.array([rec[f]], np.float32).view(np.uint32)[0] for f in ("lo", "hi"))
    count = int(rec["count"])
    return (int(rec["sum"]), count, int(rec["nans"]), _brute_key(rec["lo"]) if count else None, _brute_key(rec["hi"]) if count else None,
            int(lo), int(hi))


def test_the_restatements_columns_equal_a_brute_force_loop():
    rng = np.random.default_rng(17)
    x = (rng.standard_normal((23, 2, 6)) * 3).astype(np.float32)
    x[rng.random(x.shape) < 0.2] = np.nan
    x[3:9, 0, 2] = np.nan                                                                         # whole columns of NaN
    x[:, 1, 0] = rng.choice(np.float32([0.0, -0.0, np.inf, -np.inf, 2048.0, -4096.0, 2.0 ** -21, 3 * 2.0 ** -21]), 23)
    for k in (1, 2, 5, 7, 23, 26):
        for held, flush in ((0, True), (0, False), (min(3, k - 1), True), (k - 1, False)):
            carry = osr.fold(osr.records_of(x[:max(held, 1), ::-1, ::-1].copy())) if held else None
            got, open_rec, left = osr.columns_of(x, k, held, carry, flush)
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
                        want_mean = QNAN if n == 0 else _bits_of(np.float32(s / n * 2.0 ** -20)) if abs(s) < 2 ** 53 else None
                        assert int(osr.mean_bits(rec[p:p + 1, i:i + 1])[0, 0]) == want_mean
    # k == 1: hi == lo == x bit for bit, sum == q(x), count == 1
    one, _, _ = osr.columns_of(x, 1)
    ok = ~np.isnan(x)
    assert np.array_equal(one["hi"].view(np.uint32)[ok], x.view(np.uint32)[ok]) and np.array_equal(one["lo"].view(np.uint32)[ok], x.view(np.uint32)[ok])
    assert (one["count"][ok] == 1).all() and (one["nans"][~ok] == 1).all() and (one["count"][~ok] == 0).all()
    # hi is the peak hold's V
    for k in (2, 5, 26):
        assert np.array_equal(osr.columns_of(x, k)[0]["hi"].view(np.uint32), ov.columns_of(x, k)[0])


def test_columns_with_a_carry_equal_columns_of_the_whole_and_folds_nest():
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((24, 2, 5)) * 2).astype(np.float32)
    x[rng.random(x.shape) < 0.2] = np.nan
    for k in (1, 2, 5, 7, 24, 26):
        whole, none, left = osr.columns_of(x, k)
        assert none is None and left == 0 and whole.shape[0] == -(-24 // k)
        for cut in (1, 6, 10, 23):
            a, carry, held = osr.columns_of(x[:cut], k, flush=False)
            assert held == cut % k and (carry is None) == (held == 0)
            b, none, _ = osr.columns_of(x[cut:], k, held=held, carry=carry)
            assert osr.same(np.concatenate([a, b]), whole), (k, cut)
    # a fold of a fold is the direct fold where boundaries nest: 24 frames -> columns of 2 -> 12 -> 4 -> 1, through the library and the restatement
    fine = osr.columns_of(x, 2)[0]
    for cols in (12, 6, 4, 3, 2, 1):
        direct = osr.columns_of(x, 24 // cols)[0]
        assert osr.same(osr.view_of(fine, 0, 12, cols), direct)
        assert osr.same(api.overview_stats_fold(fine, cols), direct)
        for again in (c for c in (1, 2, 3) if cols % c == 0):
            assert osr.same(api.overview_stats_fold(api.overview_stats_fold(fine, cols), again), osr.columns_of(x, 24 // again)[0]), (cols, again)
    # ... and over a sub-range
    assert osr.same(api.overview_stats_fold(fine, 2, 2, 10), osr.columns_of(x[4:20], 8)[0])
