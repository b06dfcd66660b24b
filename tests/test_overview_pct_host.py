"""The percentile overview (sgz.h, "The percentile overview"; csrc/overview_pct.hip) without a GPU: the exports, the record's layout, the
refusals every call makes before it touches the device, and the host helpers sgz_overview_pct_bucket / _fold / _readout against the numpy
restatement (tests/overview_pct_ref.py), which shares no code with the library.  Comparisons with the restatement are on bytes or bit
patterns; the one bound, 1/64 against np.sort's order statistic, is the definition's own (both values lie in one bucket of width 1/64)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import overview_pct_ref as opr  # noqa: E402

NAMES = ("sgz_stage_overview_pct", "sgz_spectrogram_overview_pct_device", "sgz_spectrogram_overview_pct_host", "sgz_overview_pct_bucket",
         "sgz_overview_pct_fold", "sgz_overview_pct_readout", "sgz_pcm_stream_feed_overview_pct", "sgz_spectrogram_overview_pct_pcm")
E = api.SGZ_EINVAL
QNAN = 0x7FC00000


def _f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def _adversarial():
    """every edge j/64 and both float neighbours of it, +-0, denormals, +-inf, negative clip values, values >= 1"""
    edges = (np.arange(65, dtype=np.float64) / 64.0).astype(np.float32)
    near = np.concatenate([edges, np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf))])
    other = np.float32([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.1754942e-38, -1.1754942e-38, np.inf, -np.inf, -1.0, -8.333333, -1000.0, -3e38,
                        1.0, 1.0000001, 1.5, 64.0, 3e38, 0.5, 0.015624999, 0.99999994])
    return np.concatenate([near, other]).astype(np.float32)


def test_exports_exist():
    L = api.lib()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(L, name), name
    for name in ("overview_pct_columns", "overview_pct"):
        assert callable(getattr(api.Plan, name))
    for name in ("feed_overview_pct", "feed_overview_pct_into"):
        assert callable(getattr(api.PcmStream, name))
    for name in ("overview_pct_pcm", "overview_pct_fold", "overview_pct_readout", "overview_pct_bucket", "pct_from_device", "pct_to_device"):
        assert callable(getattr(api, name))
    with open(os.path.join(ROOT, "include", "sgz.h")) as f:
        header = f.read()
    assert all(name + "(" in header for name in NAMES) and "#define SGZ_ABI_VERSION 5" in header
    assert "(5, later: the percentile overview" in header and "The percentile overview:" in header
    assert "#define SGZ_OVERVIEW_PCT_BUCKETS 66" in header and "#define SGZ_OVERVIEW_PCT_MAX_QUANTILES 8" in header
    assert L.sgz_abi_version() == 5


def test_the_record_layout_is_the_dtype():
    for d in (api.OVERVIEW_PCT_DTYPE, opr.DTYPE):
        assert d.itemsize == 272 and d.names == ("bucket", "nans", "reserved")
        assert [d.fields[n][1] for n in d.names] == [0, 264, 268]
        assert d.fields["bucket"][0] == np.dtype(("<u4", (66,))) and d.fields["nans"][0] == np.dtype("<u4")
    assert (api.OVERVIEW_PCT_BUCKETS, api.OVERVIEW_PCT_MAX_QUANTILES) == (66, 8)
    # ... and the library's own: words written through the dtype survive a 1:1 fold at their offsets
    r = np.zeros(1, api.OVERVIEW_PCT_DTYPE)
    r["bucket"][0] = np.arange(1, 67)
    r["nans"] = 77
    got = api.overview_pct_fold(r, 1)
    assert got.tobytes() == np.concatenate([np.arange(1, 67), [77, 0]]).astype("<u4").tobytes()


def test_bucket_equals_the_restatement():
    x = _adversarial()
    want = opr.bucket_of(x)
    assert (want >= 0).all() and set(want) == set(range(66))                  # every bucket is met
    got = np.array([api.overview_pct_bucket(float(v)) for v in x])
    assert np.array_equal(got, want), [(float(v), int(g), int(w)) for v, g, w in zip(x, got, want) if g != w][:5]
    # the definition's named cases
    for v, b in ((-0.0, 1), (0.0, 1), (1 / 64, 2), (63 / 64, 64), (float(np.nextafter(np.float32(1), np.float32(0))), 64), (1.0, 65), (np.inf, 65),
                 (-np.inf, 0), (-1e-45, 0), (1e-45, 1), (-8.3333, 0)):
        assert api.overview_pct_bucket(v) == b, (v, b)
    # a NaN and a null result are refused, the result untouched
    b = C.c_uint32(1234)
    assert api.lib().sgz_overview_pct_bucket(C.c_float(np.nan), C.byref(b)) == E and b.value == 1234
    assert api.lib().sgz_overview_pct_bucket(C.c_float(0.5), None) == E


def _random_records(rng, shape, most=50):
    r = opr.empty(shape)
    r["bucket"] = rng.integers(0, most, (*shape, 66)) * (rng.random((*shape, 66)) < 0.3)
    r["nans"] = rng.integers(0, 5, shape)
    r.reshape(-1)[::7]["bucket"] = 0                                         # records without values
    return r


def test_fold_equals_the_restatement():
    rng = np.random.default_rng(5)
    for n, width in ((1, 1), (7, 3), (40, 6), (33, 130)):
        kept = _random_records(rng, (n, width))
        for x0, x1 in {(0, n), (0, 1), (n - 1, n), (n // 3, n - n // 4)}:
            if x0 >= x1:
                continue
            m = x1 - x0
            for cols in sorted({1, 2, 3, m - 1, m, m + 5} - {0}):
                want = opr.view_of(kept, x0, x1, cols)
                got = api.overview_pct_fold(kept, cols, x0, x1)
                assert opr.same(got, want), (n, width, x0, x1, cols)
                assert got.shape[0] == api.overview_view_columns(n, x0, x1, cols)
    # a fold of folds is the direct fold wherever the boundaries coincide
    kept = _random_records(rng, (48, 5))
    for fine, coarse in ((24, 6), (12, 4), (16, 1), (48, 3)):
        assert opr.same(api.overview_pct_fold(api.overview_pct_fold(kept, fine), coarse), api.overview_pct_fold(kept, coarse)), (fine, coarse)
    # a folded word above 2^32 - 1 is refused and nothing is written: each of the words in turn
    L = api.lib()
    for word in ("bucket", "nans"):
        big = opr.empty((3, 2))
        if word == "bucket":
            big["bucket"][:2, 1, 65] = 0x80000000
        else:
            big["nans"][:2, 1] = 0x80000000
        out = np.full((2, 2, 68), 0x5A5AA5A5, np.uint32)
        assert L.sgz_overview_pct_fold(big.ctypes.data_as(C.c_void_p), 3, 2, 0, 3, 1, out.ctypes.data_as(C.c_void_p)) == E
        assert b"2^32 - 1" in L.sgz_last_error() and (out == 0x5A5AA5A5).all()
        # ... while 2^32 - 1 itself folds
        big[word][1, 1] = np.where(big[word][1, 1] == 0x80000000, 0x7FFFFFFF, big[word][1, 1])
        assert L.sgz_overview_pct_fold(big.ctypes.data_as(C.c_void_p), 3, 2, 0, 3, 1, out.ctypes.data_as(C.c_void_p)) == api.SGZ_OK
        assert opr.same(out[:1].view(opr.DTYPE).reshape(1, 2), opr.view_of(big, 0, 3, 1))
    # the other refusals, nothing written
    rec = opr.empty((4, 2))
    p, o = rec.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    out[:] = 0x5A5AA5A5
    for args in ((None, 4, 2, 0, 4, 2, o), (p, 4, 2, 0, 4, 2, None), (p, 4, 0, 0, 4, 2, o), (p, 4, 2, 2, 2, 2, o), (p, 4, 2, 0, 5, 2, o), (p, 4, 2, 0, 4, 0, o)):
        assert L.sgz_overview_pct_fold(*args) == E, args
    assert (out == 0x5A5AA5A5).all()


def test_readout_equals_the_restatement_bit_for_bit():
    rng = np.random.default_rng(11)
    recs = _random_records(rng, (300,))
    hand = opr.empty((6,))
    hand["bucket"][0, 0] = 9                                                 # everything below 0
    hand["bucket"][1, 65] = 4                                                # everything at or above 1
    hand["bucket"][2, [0, 30, 65]] = (2, 1, 2)
    hand["bucket"][3, 17] = 0xFFFFFFFF                                       # the greatest count
    hand["nans"][4] = 12                                                     # NaNs alone: no count
    hand["bucket"][5, 1:65] = 1
    recs = np.concatenate([recs, hand])
    qs = [0.0, 0.1, 0.25, 0.5, 0.75, 0.95, 1.0 - 2.0 ** -53, 1.0]
    got = api.overview_pct_readout(recs, qs)
    want = opr.quantile_bits(recs, qs)
    assert got.shape == (8, recs.size) and np.array_equal(got.view(np.uint32), want)
    assert (got.view(np.uint32)[:, -2] == QNAN).all() and (got[:, -6] == np.float32(-2.0 ** -6)).all() and (got[:, -5] == 1.0).all()
    for nq in (1, 3):
        assert np.array_equal(api.overview_pct_readout(recs, qs[:nq]).view(np.uint32), want[:nq])
    assert np.array_equal(api.overview_pct_readout(recs.reshape(2, -1), 0.5).view(np.uint32), opr.quantile_bits(recs, 0.5).reshape(1, 2, -1))
    # monotone in q for any record
    fine = np.linspace(0.0, 1.0, 8)
    v = api.overview_pct_readout(recs[:-2], fine)
    ok = ~np.isnan(v[0])
    assert (np.diff(v[:, ok], axis=0) >= 0).all()


def test_readout_against_a_plain_sort():
    """values in [0, 1): the readout is within 1/64 of sorted(x)[r - 1] (both lie in bucket b, whose width is 1/64), it is monotone in q, and
    q = 0 / q = 1 land in the buckets of the minimum / the maximum"""
    rng = np.random.default_rng(3)
    qs = np.array([0.0, 0.1, 0.3, 0.5, 0.77, 0.95, 0.999, 1.0])
    for n in (1, 2, 3, 10, 64, 1000):
        x = rng.random((n, 40)).astype(np.float32) ** np.float32(rng.choice([0.3, 1.0, 4.0]))
        x = np.minimum(x, np.float32(0.99999994))
        rec = opr.fold(opr.records_of(x), 0)
        assert np.array_equal(rec["bucket"].sum(axis=1), np.full(40, n))
        got = api.overview_pct_readout(rec, qs)
        srt = np.sort(x, axis=0)
        for j, q in enumerate(qs):
            r = int(min(max(np.ceil(q * n), 1), n))
            exact = srt[r - 1]
            assert (np.abs(got[j].astype(np.float64) - exact.astype(np.float64)) <= 1 / 64).all(), (n, q)
            assert np.array_equal(opr.bucket_of(got[j]), opr.bucket_of(exact)), (n, q)
        assert (np.diff(got, axis=0) >= 0).all()
        assert np.array_equal(opr.bucket_of(got[0]), opr.bucket_of(srt[0])) and np.array_equal(opr.bucket_of(got[-1]), opr.bucket_of(srt[-1]))


def test_readout_refusals_leave_the_values_untouched():
    L = api.lib()
    rec = opr.empty((3,))
    rec["bucket"][:, 5] = 1
    p = rec.ctypes.data_as(C.c_void_p)
    out = np.full((8, 3), 0x5A5AA5A5, np.uint32)
    o = out.ctypes.data_as(C.c_void_p)

    def q(*v):
        a = np.array(v, np.float64)
        return a, a.ctypes.data_as(C.c_void_p)
    good, gp = q(0.5)
    for args in ((None, 3, gp, 1, o), (p, 3, None, 1, o), (p, 3, gp, 0, o), (p, 3, gp, 9, o), (p, 3, gp, 1, None),
                 (p, 3, q(-0.001)[1], 1, o), (p, 3, q(1.0000001)[1], 1, o), (p, 3, q(np.nan)[1], 1, o), (p, 3, q(0.5, 0.2, np.nan)[1], 3, o)):
        assert L.sgz_overview_pct_readout(*args) == E, args
    over = opr.empty((2,))
    over["bucket"][1, :2] = 0x80000000                                       # the buckets sum above 2^32 - 1
    assert L.sgz_overview_pct_readout(over.ctypes.data_as(C.c_void_p), 2, gp, 1, o) == E
    assert (out == 0x5A5AA5A5).all()
    assert L.sgz_overview_pct_readout(None, 0, gp, 1, o) == api.SGZ_OK and (out == 0x5A5AA5A5).all()      # no records: nothing to do


def test_calls_refuse_before_the_device():
    """every SGZ_EINVAL of the stage call and the renders that needs no device: the plan is never uploaded here"""
    L = api.lib()
    plan = api.Plan(config.spectrum_config(window_size=64, hop=16, axis_points=33))
    b = np.zeros(65536, np.float64)
    p = b.ctypes.data_as(C.c_void_p)
    odd = C.c_void_p(b.ctypes.data + 8)                                      # 8-aligned, not 16
    good = np.array([0.5, 0.1], np.float64)
    gp = good.ctypes.data_as(C.c_void_p)
    bad = np.array([0.5, 1.5], np.float64).ctypes.data_as(C.c_void_p)
    stage = L.sgz_stage_overview_pct
    for args in ((None, p, 4, 2, 0, 1, 0, gp, 2, p, p, p, p, None), (plan.h, None, 4, 2, 0, 1, 0, gp, 2, p, p, p, p, None),
                 (plan.h, p, 4, 0, 0, 1, 0, gp, 2, p, p, p, p, None), (plan.h, p, 4, 2, 2, 1, 0, gp, 2, p, p, p, p, None),
                 (plan.h, p, 4, 2, 0, 1, 65, gp, 2, p, p, p, p, None), (plan.h, p, 4, 2, 0, 1, 0, None, 2, p, p, p, p, None),
                 (plan.h, p, 4, 2, 0, 1, 0, gp, 0, p, p, p, p, None), (plan.h, p, 4, 2, 0, 1, 0, gp, 9, p, p, p, p, None),
                 (plan.h, p, 4, 2, 0, 1, 0, bad, 2, p, p, p, p, None), (plan.h, p, 4, 2, 0, 1, 0, gp, 2, p, None, None, None, None),
                 (plan.h, p, 4, 2, 0, 1, 0, gp, 2, odd, p, p, p, None), (plan.h, p, 4, 2, 0, 1, 0, gp, 2, p, p, odd, p, None),
                 (plan.h, p, 3, 2, 0, 0, 0, gp, 2, None, p, p, p, None), (plan.h, p, 3, 2, 1, 1, 0, gp, 2, None, p, p, p, None)):
        assert stage(*args) == E, args
    assert not b.any()
    dev = L.sgz_spectrogram_overview_pct_device
    for args in ((None, p, 4096, 4096, 2, gp, 2, p, p, p, None, None), (plan.h, None, 4096, 4096, 2, gp, 2, p, p, p, None, None),
                 (plan.h, p, 4096, 4096, 0, gp, 2, p, p, p, None, None), (plan.h, p, 4096, 4096, 2, bad, 2, p, p, p, None, None),
                 (plan.h, p, 4096, 4096, 2, gp, 9, p, p, p, None, None), (plan.h, p, 4096, 4096, 2, gp, 2, None, None, None, None, None),
                 (plan.h, p, 4096, 4096, 2, gp, 2, p, odd, p, None, None)):
        assert dev(*args) == E, args
    ptrs = (C.c_void_p * 2)(b.ctypes.data, b.ctypes.data)
    host = L.sgz_spectrogram_overview_pct_host
    for args in ((None, ptrs, 2, 4096, 2, gp, 2, p, p, p, None), (plan.h, None, 2, 4096, 2, gp, 2, p, p, p, None), (plan.h, ptrs, 2, 4096, 0, gp, 2, p, p, p, None),
                 (plan.h, ptrs, 2, 4096, 2, None, 2, p, p, p, None), (plan.h, ptrs, 2, 4096, 2, bad, 2, p, p, p, None),
                 (plan.h, ptrs, 2, 4096, 2, gp, 2, None, None, None, None), (plan.h, ptrs, 3, 4096, 2, gp, 2, p, p, p, None)):
        assert host(*args) == E, args
    cfg = api._as_config(config.spectrum_config(window_size=64, hop=16, axis_points=33))
    shot = L.sgz_spectrogram_overview_pct_pcm
    for args in ((None, p, api.PCM_F32, 2, None, 4096, 2, gp, 2, p, p, p, None), (C.byref(cfg), None, api.PCM_F32, 2, None, 4096, 2, gp, 2, p, p, p, None),
                 (C.byref(cfg), p, api.PCM_F32, 2, None, 4096, 0, gp, 2, p, p, p, None), (C.byref(cfg), p, api.PCM_F32, 2, None, 4096, 2, bad, 2, p, p, p, None),
                 (C.byref(cfg), p, api.PCM_F32, 2, None, 4096, 2, gp, 2, None, None, None, None)):
        assert shot(*args) == E, args
    assert not b.any()
