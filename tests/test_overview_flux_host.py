"""The flux overview (sgz.h, "The flux overview"; csrc/overview_flux.hip) without a GPU: the exports, the record's layout, the refusals every
call makes before it touches the device (Phase and RSNT plans among them), and the host helpers sgz_overview_flux_quantise / _fold / _readout
/ _hz against the restatement (tests/overview_flux_ref.py) and against exact rational arithmetic.  Every comparison is on bytes or bit
patterns; no tolerance anywhere."""
import ctypes as C
import itertools
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from signalizer_amd import api, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import overview_flux_ref as ofr  # noqa: E402

NAMES = ("sgz_stage_overview_flux", "sgz_spectrogram_overview_flux_device", "sgz_spectrogram_overview_flux_host", "sgz_overview_flux_quantise",
         "sgz_overview_flux_fold", "sgz_overview_flux_readout", "sgz_overview_flux_hz", "sgz_pcm_stream_feed_overview_flux",
         "sgz_spectrogram_overview_flux_pcm")
E, U = api.SGZ_EINVAL, api.SGZ_EUNSUPPORTED


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
    return np.array(bits, np.uint32).view(np.float32)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_exports_exist():
    L = api.lib()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(L, name), name
    for name in ("overview_flux_columns", "overview_flux", "overview_flux_hz"):
        assert callable(getattr(api.Plan, name))
    for name in ("feed_overview_flux", "feed_overview_flux_into"):
        assert callable(getattr(api.PcmStream, name))
    for name in ("overview_flux_pcm", "overview_flux_fold", "overview_flux_readout", "overview_flux_quantise", "overview_flux_hz"):
        assert callable(getattr(api, name))
    with open(os.path.join(ROOT, "include", "sgz.h")) as f:
        header = f.read()
    assert all(name + "(" in header for name in NAMES) and "#define SGZ_ABI_VERSION 5" in header
    assert "(5, later: the flux overview" in header and "The flux overview:" in header
    assert "(5, later: the cross overview" in header and "(5, later: the power overview" in header  # the earlier entries stay
    assert L.sgz_abi_version() == 5


def test_the_record_layout_is_the_dtype():
    for d in (api.OVERVIEW_FLUX_DTYPE, ofr.DTYPE):
        assert d.itemsize == 88 and d.names == ("amp", "mom1", "mom2", "flux", "flux_max", "flux_at", "count", "nans")
        assert [d.fields[n][1] for n in d.names] == [0, 16, 32, 48, 64, 72, 80, 84]

    class Rec(C.Structure):
        _fields_ = [("amp", C.c_uint64 * 2), ("mom1", C.c_uint64 * 2), ("mom2", C.c_uint64 * 2), ("flux", C.c_uint64 * 2), ("flux_max", C.c_uint64),
                    ("flux_at", C.c_uint64), ("count", C.c_uint32), ("nans", C.c_uint32)]
    assert C.sizeof(Rec) == 88 and C.alignment(Rec) == 8
    assert [getattr(Rec, n).offset for n, _ in Rec._fields_] == [0, 16, 32, 48, 64, 72, 80, 84]
    # the library reads the same layout: a record written through ctypes folds to itself
    r = Rec((1, 2), (3, 4), (5, 6), (7, 8), 9, 10, 11, 12)
    one = np.frombuffer(bytes(r), api.OVERVIEW_FLUX_DTYPE).reshape(1, 1)
    assert _same(api.overview_flux_fold(one, 1), one)
    assert ofr.unpack(one[0, 0]) == {"amp": 1 | 2 << 64, "mom1": 3 | 4 << 64, "mom2": 5 | 6 << 64, "flux": 7 | 8 << 64, "flux_max": 9, "flux_at": 10,
                                     "count": 11, "nans": 12}


# ---- refusals before the device ---------------------------------------------------------------------------------------------------------------
def test_stage_call_refusals_before_the_device(plan, buf):
    L = api.lib()
    b, p = buf
    odd4, odd8 = C.c_void_p(p.value + 2), C.c_void_p(p.value + 4)
    #                                          mapped frames k held flush first slices prev carry flux stream
    assert L.sgz_stage_overview_flux(None, p, 4, 2, 0, 1, 0, 0, p, p, p, None) == E
    assert L.sgz_stage_overview_flux(plan.h, None, 4, 2, 0, 1, 0, 0, p, p, p, None) == E
    assert L.sgz_stage_overview_flux(plan.h, p, 4, 0, 0, 1, 0, 0, p, p, p, None) == E              # k == 0
    assert L.sgz_stage_overview_flux(plan.h, p, 4, 2, 2, 1, 0, 0, p, p, p, None) == E              # held >= k
    assert L.sgz_stage_overview_flux(plan.h, p, 4, 1, 1, 1, 0, 0, p, p, p, None) == E
    assert L.sgz_stage_overview_flux(plan.h, p, 4, 2, 0, 1, 0, 65, p, p, p, None) == E             # slices > 64
    assert L.sgz_stage_overview_flux(plan.h, p, 4, 2, 0, 1, 0, 0xffffffff, p, p, p, None) == E
    assert L.sgz_stage_overview_flux(plan.h, p, 4, 2, 0, 1, 0, 0, p, p, None, None) == E           # columns close and there is no d_flux
    assert L.sgz_stage_overview_flux(plan.h, p, 4, 2, 1, 1, 0, 0, p, None, p, None) == E           # the carry is read
    assert L.sgz_stage_overview_flux(plan.h, p, 3, 2, 0, 0, 0, 0, p, None, p, None) == E           # the carry is written
    assert L.sgz_stage_overview_flux(plan.h, p, 0, 2, 1, 1, 0, 0, None, None, p, None) == E        # a flush of the held column reads it
    assert L.sgz_stage_overview_flux(plan.h, odd4, 4, 2, 0, 1, 0, 0, p, p, p, None) == E           # alignment
    assert L.sgz_stage_overview_flux(plan.h, p, 4, 2, 0, 1, 0, 0, odd4, p, p, None) == E
    assert L.sgz_stage_overview_flux(plan.h, p, 4, 2, 0, 1, 0, 0, p, odd8, p, None) == E
    assert L.sgz_stage_overview_flux(plan.h, p, 4, 2, 0, 1, 0, 0, p, p, odd8, None) == E
    # nothing arrives and no column to flush: SGZ_OK before the plan is looked at any further
    assert L.sgz_stage_overview_flux(plan.h, p, 0, 2, 0, 1, 0, 0, None, None, None, None) == api.SGZ_OK
    assert L.sgz_stage_overview_flux(plan.h, p, 0, 3, 2, 0, 0, 0, p, p, None, None) == api.SGZ_OK
    assert not b.any()


def test_render_refusals_before_the_device(plan, buf):
    L = api.lib()
    b, p = buf
    ch = (C.c_void_p * 2)(p, p)
    assert L.sgz_spectrogram_overview_flux_device(None, p, 1024, 1024, 2, p, None) == E
    assert L.sgz_spectrogram_overview_flux_device(plan.h, None, 1024, 1024, 2, p, None) == E
    assert L.sgz_spectrogram_overview_flux_device(plan.h, p, 1024, 1024, 0, p, None) == E
    assert L.sgz_spectrogram_overview_flux_device(plan.h, p, 1024, 1024, 2, None, None) == E
    assert L.sgz_spectrogram_overview_flux_host(None, ch, 2, 1024, 2, p, None) == E
    assert L.sgz_spectrogram_overview_flux_host(plan.h, None, 2, 1024, 2, p, None) == E
    assert L.sgz_spectrogram_overview_flux_host(plan.h, ch, 2, 1024, 0, p, None) == E
    assert L.sgz_spectrogram_overview_flux_host(plan.h, ch, 2, 1024, 2, None, None) == E
    assert L.sgz_spectrogram_overview_flux_host(plan.h, ch, 3, 1024, 2, p, None) == E                 # 2 * num_pairs channels, as the render
    assert L.sgz_spectrogram_overview_flux_host(plan.h, (C.c_void_p * 2)(p, None), 2, 1024, 2, p, None) == E
    cfg = api.config_from_dict(_small())
    for args in ((None, p, api.PCM_S16, 2, None, 100, 2, p), (cfg, None, api.PCM_S16, 2, None, 100, 2, p),
                 (cfg, p, api.PCM_S16, 2, None, 100, 0, p), (cfg, p, api.PCM_S16, 2, None, 100, 2, None)):
        assert L.sgz_spectrogram_overview_flux_pcm(C.byref(args[0]) if args[0] is not None else None, *args[1:], None) == E
    assert L.sgz_pcm_stream_feed_overview_flux(None, p, 10, 2, 0, p, 10, None, None) == E
    assert not b.any()


@pytest.mark.parametrize("over", [dict(channel_mode=config.CH_PHASE), dict(algorithm=config.ALGO_RSNT)], ids=["phase", "rsnt"])
def test_phase_and_rsnt_plans_are_refused_before_the_device(buf, over):
    """the render, host and pcm calls: SGZ_EUNSUPPORTED from a plan that was never uploaded, nothing written"""
    L = api.lib()
    b, p = buf
    plan = api.Plan(_small(**over))
    ch = (C.c_void_p * 2)(p, p)
    assert L.sgz_spectrogram_overview_flux_device(plan.h, p, 1024, 1024, 2, p, None) == U
    assert b"flux overview" in L.sgz_last_error()
    assert L.sgz_spectrogram_overview_flux_host(plan.h, ch, 2, 1024, 2, p, None) == U
    cfg = api.config_from_dict(_small(**over))
    assert L.sgz_spectrogram_overview_flux_pcm(C.byref(cfg), p, api.PCM_S16, 2, None, 1000, 2, p, None) == U
    # the argument refusals come first, as on any plan
    assert L.sgz_spectrogram_overview_flux_device(plan.h, p, 1024, 1024, 0, p, None) == E
    assert L.sgz_spectrogram_overview_flux_host(plan.h, ch, 2, 1024, 2, None, None) == E
    assert not b.any()


# ---- the quantiser ----------------------------------------------------------------------------------------------------------------------------
def _exact(x):
    """a(x) in exact rational arithmetic: |x| 2^30 clamped at 2^34, to the nearest integer, ties to even"""
    if x != x:
        return 0
    if x in (float("inf"), float("-inf")):
        return 2 ** 34
    t = min(abs(Fraction(float(x))) * 2 ** 30, Fraction(2 ** 34))
    lo = t.numerator // t.denominator
    rest = t - lo
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2):
        lo += 1
    return lo


def _edge_values():
    ties = [np.float32((2 * m + 1) * 2.0 ** -31) for m in (0, 1, 2, 3, 4, 1000, 1001, 2 ** 22, 2 ** 22 + 1)]     # odd multiples of 2^-31: exact ties
    tiny = [np.float32(v) for v in (0.0, 2.0 ** -149, 2.0 ** -126, 2.0 ** -40, 2.0 ** -32, 2.0 ** -31, np.nextafter(np.float32(2.0 ** -31), np.float32(1)),
                                    np.nextafter(np.float32(2.0 ** -31), np.float32(0)), 2.0 ** -30, 3 * 2.0 ** -32)]
    clamp = [np.nextafter(np.float32(16), np.float32(0)), np.float32(16), np.nextafter(np.float32(16), np.float32(32)), np.float32(17), np.float32(1e30),
             np.float32(3.4028235e38)]
    special = list(_f([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x80000000]))
    vals = ties + tiny + clamp + special + [np.float32(1), np.float32(0.5), np.float32(0.1), np.float32(15.999)]
    return np.array(vals + [-v for v in vals], np.float32)


def test_quantise_equals_the_restatement_and_exact_arithmetic():
    x = _edge_values()
    rng = np.random.default_rng(7)
    x = np.concatenate([x, (2.0 ** rng.uniform(-35, 5, 4000)).astype(np.float32) * rng.choice([-1, 1], 4000).astype(np.float32)])
    a = api.overview_flux_quantise(x)
    assert a.dtype == np.uint64 and _same(a, ofr.quantise(x))
    assert [int(v) for v in a] == [_exact(float(v)) for v in x]
    # what the definition says about a few of them
    q = lambda v: int(api.overview_flux_quantise(np.array([v], np.float32))[0])
    assert q(2.0 ** -31) == 0 and q(3 * 2.0 ** -31) == 2 and q(5 * 2.0 ** -31) == 2 and q(7 * 2.0 ** -31) == 4      # ties go to even
    assert q(2.0 ** -30) == 1 and q(1.0) == 2 ** 30 and q(-1.0) == 2 ** 30 and q(-0.0) == 0
    assert q(16.0) == 2 ** 34 and q(1e30) == 2 ** 34 and q(float("inf")) == 2 ** 34 and q(float("-inf")) == 2 ** 34
    assert q(float("nan")) == 0
    assert api.lib().sgz_overview_flux_quantise(None, 1, None) == E
    assert api.lib().sgz_overview_flux_quantise(None, 0, None) == api.SGZ_OK


# ---- the fold -----------------------------------------------------------------------------------------------------------------------------------
def _random_records(rng, n, width, big=False):
    recs = []
    for _ in range(n):
        row = []
        for _ in range(width):
            top = 2 ** 100 if big else 2 ** 60
            fmax = int(rng.integers(0, 4))                                                       # few values: ties between columns
            row.append({"amp": int(rng.integers(0, 2 ** 62)) * (top >> 60), "mom1": int(rng.integers(0, 2 ** 62)) * (top >> 58),
                        "mom2": int(rng.integers(0, 2 ** 62)) * (top >> 56), "flux": int(rng.integers(0, 2 ** 62)), "flux_max": fmax,
                        "flux_at": int(rng.integers(0, 2 ** 40)), "count": int(rng.integers(1, 1000)), "nans": int(rng.integers(0, 5))})
        recs.append(row)
    return ofr.pack(recs)


def test_fold_equals_the_restatement_and_any_grouping_gives_the_same_bytes():
    rng = np.random.default_rng(11)
    recs = _random_records(rng, 12, 3, big=True)
    for out_columns, x0, x1 in ((1, 0, 12), (5, 0, 12), (12, 0, 12), (100, 0, 12), (4, 3, 10), (1, 11, 12)):
        assert _same(api.overview_flux_fold(recs, out_columns, x0, x1), ofr.fold_columns(recs, out_columns, x0, x1))
    whole = api.overview_flux_fold(recs, 1)
    # a fold of folds, in any order of the source columns and any grouping
    for perm in (np.arange(12)[::-1], rng.permutation(12), rng.permutation(12)):
        shuffled = recs[perm]
        assert _same(api.overview_flux_fold(shuffled, 1), whole)
        for groups in (2, 3, 4, 6):
            assert _same(api.overview_flux_fold(api.overview_flux_fold(shuffled, groups), 1), whole)
    assert _same(api.overview_flux_fold(np.concatenate([api.overview_flux_fold(recs, 1, 0, 5), api.overview_flux_fold(recs, 1, 5, 12)]), 1), whole)


def test_fold_tie_rule_and_empty_records():
    mk = lambda fmax, at, count=1: {"amp": 1, "mom1": 2, "mom2": 3, "flux": fmax, "flux_max": fmax, "flux_at": at, "count": count, "nans": 0}
    for order in itertools.permutations([mk(7, 50), mk(7, 20), mk(3, 1), mk(7, 90)]):
        out = ofr.unpack(api.overview_flux_fold(ofr.pack([[r] for r in order]), 1)[0, 0])
        assert (out["flux_max"], out["flux_at"]) == (7, 20), order                               # the greater maximum, then the earlier frame
        assert out["count"] == 4 and out["amp"] == 4 and out["flux"] == 24
    # an empty record (no frame: 0 and UINT64_MAX) never wins against a frame, not even one whose F is 0
    for order in itertools.permutations([ofr.empty(), mk(0, 5), ofr.empty()]):
        out = ofr.unpack(api.overview_flux_fold(ofr.pack([[r] for r in order]), 1)[0, 0])
        assert (out["flux_max"], out["flux_at"], out["count"]) == (0, 5, 1)
    out = ofr.unpack(api.overview_flux_fold(ofr.pack([[ofr.empty()], [ofr.empty()]]), 1)[0, 0])
    assert out == ofr.empty()
    # the 128-bit sums carry from the low word into the high
    big = dict(mk(1, 1), amp=2 ** 64 - 1, mom2=2 ** 127)
    out = ofr.unpack(api.overview_flux_fold(ofr.pack([[big], [dict(mk(1, 2), amp=2, mom2=5)]]), 1)[0, 0])
    assert out["amp"] == 2 ** 64 + 1 and out["mom2"] == 2 ** 127 + 5


def test_fold_refusals_write_nothing():
    L = api.lib()
    recs = ofr.pack([[dict(ofr.empty(), count=2 ** 32 - 1, flux_at=1)], [dict(ofr.empty(), count=1, flux_at=2)], [dict(ofr.empty(), nans=7, count=9, flux_at=3)]])
    out = np.frombuffer(bytearray(b"\x5a" * 88 * 3), api.OVERVIEW_FLUX_DTYPE)
    poison = out.tobytes()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.sgz_overview_flux_fold(None, 3, 1, 0, 3, 1, ptr(out)) == E
    assert L.sgz_overview_flux_fold(ptr(recs), 3, 1, 0, 3, 1, None) == E
    assert L.sgz_overview_flux_fold(ptr(recs), 3, 0, 0, 3, 1, ptr(out)) == E                      # width == 0
    assert L.sgz_overview_flux_fold(ptr(recs), 3, 1, 2, 2, 1, ptr(out)) == E                      # an empty range
    assert L.sgz_overview_flux_fold(ptr(recs), 3, 1, 0, 4, 1, ptr(out)) == E                      # past the end
    assert L.sgz_overview_flux_fold(ptr(recs), 3, 1, 0, 3, 0, ptr(out)) == E                      # no output column
    assert L.sgz_overview_flux_fold(ptr(recs), 3, 1, 0, 3, 2, ptr(out)) == E                      # columns 0 and 1 together count 2^32
    assert b"2^32 - 1" in L.sgz_last_error()
    assert out.tobytes() == poison
    assert L.sgz_overview_flux_fold(ptr(recs), 3, 1, 0, 3, 3, ptr(out)) == api.SGZ_OK             # each alone fits
    assert out.tobytes() == recs.tobytes()


# ---- the readout ------------------------------------------------------------------------------------------------------------------------------
def test_readout_equals_fp64_numpy_bit_for_bit():
    rng = np.random.default_rng(13)
    recs = np.concatenate([_random_records(rng, 40, 2).reshape(-1), _random_records(rng, 40, 2, big=True).reshape(-1),
                           ofr.pack([ofr.empty(), dict(ofr.empty(), count=3, flux_at=4), dict(ofr.empty(), count=2, amp=2 ** 64, mom1=2 ** 70, mom2=2 ** 80, flux=2 ** 64 + 1),
                                     dict(ofr.empty(), count=1, amp=2 ** 30 * 97, mom1=0, mom2=0, flux=0),
                                     dict(ofr.empty(), count=1, amp=3, mom1=2 ** 64 + 2 ** 11 + 1, mom2=2 ** 127 + 2 ** 64 - 1, flux=2 ** 64 - 1)])])
    assert any(ofr.unpack(r)["mom2"] >= 2 ** 64 for r in recs)
    for pixels in (1, 97, 2 ** 20):
        got = api.overview_flux_readout(recs, pixels)
        want = ofr.readout(recs, pixels)
        for g, w in zip(got, want):
            assert g.dtype == np.float64 and _same(np.where(np.isnan(g), np.nan, g), np.where(np.isnan(w), np.nan, w))
            assert (np.isnan(g) == np.isnan(w)).all()
    mean_amp, c, spread, mean_flux, rel = api.overview_flux_readout(recs[-5:], 97)
    assert np.isnan(mean_amp[0]) and np.isnan(c[0]) and np.isnan(spread[0]) and np.isnan(mean_flux[0]) and np.isnan(rel[0])      # count == 0
    assert mean_amp[1] == 0 and mean_flux[1] == 0 and np.isnan(c[1]) and np.isnan(spread[1]) and np.isnan(rel[1])                # amp == 0
    assert mean_amp[3] == 1.0 and c[3] == 0 and spread[3] == 0 and rel[3] == 0                                                    # a unit value in every pixel
    L = api.lib()
    p = recs.ctypes.data_as(C.c_void_p)
    o = np.zeros(recs.size).ctypes.data_as(C.c_void_p)
    assert L.sgz_overview_flux_readout(None, 1, 4, o, o, o, o, o) == E
    assert L.sgz_overview_flux_readout(p, 1, 4, None, None, None, None, None) == E
    assert L.sgz_overview_flux_readout(p, 1, 0, o, None, None, None, None) == E                    # the mean amplitude is per pixel
    assert L.sgz_overview_flux_readout(p, 1, 0, None, o, None, None, None) == api.SGZ_OK


def test_readout_of_a_hand_made_frame():
    """one frame of three pixels at k = 1: the numbers a reader would work out by hand"""
    x = np.array([[[0.0, 0.5, 0.25]]], np.float32)
    recs, _ = ofr.overview(x, 1, prev=np.array([[0.25, 0.25, 0.5]], np.float32))
    r = ofr.unpack(recs[0, 0])
    assert r["amp"] == 3 * 2 ** 28 and r["mom1"] == 2 ** 29 + 2 * 2 ** 28 and r["mom2"] == 2 ** 29 + 4 * 2 ** 28 and r["flux"] == 2 ** 28
    mean_amp, c, spread, mean_flux, rel = api.overview_flux_readout(recs, 3)
    assert mean_amp[0, 0] == 0.25 and c[0, 0] == 4 / 3 and mean_flux[0, 0] == 0.25 and rel[0, 0] == 1 / 3
    assert spread[0, 0] == np.sqrt(np.float64(2.0) - np.float64(4 / 3) * np.float64(4 / 3))


def test_hz_interpolates_the_mapped_frequencies(plan):
    f = plan.mapped_frequencies()
    rng = np.random.default_rng(17)
    x = np.concatenate([[-1.0, -0.0, 0.0, 0.5, 1.0, plan.P - 2, plan.P - 1.5, plan.P - 1, plan.P, 1e9, np.nan, np.inf, -np.inf], rng.uniform(0, plan.P - 1, 500)])
    got, want = api.overview_flux_hz(plan, x), ofr.hz(f, x)
    assert (np.isnan(got) == np.isnan(want)).all() and np.isnan(got[10])
    keep = ~np.isnan(want)
    assert _same(got[keep], want[keep])
    assert got[0] == f[0] and got[4] == f[1] and got[7] == f[-1] and got[9] == f[-1] and got[3] == np.float64(f[0]) + 0.5 * (np.float64(f[1]) - np.float64(f[0]))
    L = api.lib()
    assert L.sgz_overview_flux_hz(None, x.ctypes.data_as(C.c_void_p), 1, x.ctypes.data_as(C.c_void_p)) == E
    assert L.sgz_overview_flux_hz(plan.h, None, 1, None) == E


# ---- the restatement against a brute-force loop -------------------------------------------------------------------------------------------------
def test_the_restatements_columns_equal_a_brute_force_loop_and_nest():
    rng = np.random.default_rng(19)
    frames, rows, P, k = 11, 2, 7, 3
    x = (2.0 ** rng.uniform(-35, 5, (frames, rows, P))).astype(np.float32)
    x[3, 0, 2], x[5, 1, 0], x[6, 0, 6], x[7, 1, 1] = np.nan, np.inf, -np.inf, -0.0
    first = 2 ** 33 + 5
    recs, left = ofr.overview(x, k, first_frame=first)
    assert left is None and recs.shape == (4, rows)
    for col in range(4):
        for r in range(rows):
            want = ofr.empty()
            for f in range(col * k, min(frames, (col + 1) * k)):
                a = [_exact(float(v)) for v in x[f, r]]
                b = [_exact(float(v)) for v in x[f - 1, r]] if f else None
                F = sum(max(0, u - v) for u, v in zip(a, b)) if f else 0
                if F > want["flux_max"] or want["count"] == 0:
                    want["flux_max"], want["flux_at"] = F, first + f
                want["amp"] += sum(a)
                want["mom1"] += sum(i * v for i, v in enumerate(a))
                want["mom2"] += sum(i * i * v for i, v in enumerate(a))
                want["flux"] += F
                want["count"] += 1
                want["nans"] += int(np.isnan(x[f, r]).any())
            assert ofr.unpack(recs[col, r]) == want, (col, r)
    # calls chained through the carry and the previous frame give the columns of the whole, and coarser columns are folds of finer ones
    for cut in (1, 2, 3, 4, 10):
        a, left = ofr.overview(x[:cut], k, first_frame=first, flush=False)
        b, none = ofr.overview(x[cut:], k, first_frame=first + cut, prev=x[cut - 1], held=cut % k, carry=left)
        assert none is None and _same(np.concatenate([a, b]), recs)
    fine, _ = ofr.overview(x, 1, first_frame=first)
    assert _same(ofr.fold_columns(fine, 4), recs) and _same(api.overview_flux_fold(fine, 4), recs)
