"""The band lane's host helpers (csrc/band_columns.hip) against tests/band_ref.py and the oracle's crossover and colour rule, and the
definition itself against the unsegmented fp64 recurrence and the oracle's fp32 network.  No GPU."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from oracle import pyoracle
from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import band_ref as br  # noqa: E402

E = api.SGZ_EINVAL
_cache = {}


def rate_filter(rate):
    if rate not in _cache:
        _cache[rate] = api.band_filter_for_rate(rate)
    return _cache[rate]


def tiny():
    return api.band_filter(br.TINY.c, br.TINY.W, br.TINY.L)


def coefs(f):
    return np.array([[f.c[s][i] for i in range(5)] for s in range(4)], np.float64)


# ---- the filter of a rate and the tap table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate, W", [(44100, 1024), (48000, 1024), (192000, 4096)])
def test_the_filter_of_a_rate_is_the_live_scopes(rate, W):
    f = rate_filter(rate)
    assert (f.W, f.L) == (W, W // 16)
    want = np.zeros(20, np.float32)
    pyoracle.lib().sgzo_lr_design(300.0, 3000.0, float(rate), want.ctypes.data_as(C.c_void_p))
    got = coefs(f)
    assert np.array_equal(got.astype(np.float32).reshape(-1), want)
    assert np.array_equal(got.astype(np.float32).astype(np.float64), got), "every coefficient is a float, widened"


def test_the_memory_of_a_rate():
    for rate, low, high, W in ((8000, 300, 3000, 256), (384000, 300, 3000, 8192), (48000, 20, 200, 16384), (48000, 2000, 20000, 256), (96000, 300, 3000, 2048),
                               (3276800, 300, 3000, 65536)):
        f = api.band_filter_for_rate(rate, low, high)
        assert (f.W, f.L) == (W, W // 16), (rate, low, high)
        t = br.taps(f)
        assert t is not None and np.abs(t[:, -1]).max() == 0, "the impulse response is below 2^-31 at W"


@pytest.mark.parametrize("which", ["tiny", 44100, 48000, 96000])
def test_the_tap_table_entry_for_entry(which):
    f = tiny() if which == "tiny" else rate_filter(which)
    st, got = api.band_taps(f)
    want = br.taps(f)
    assert st == api.SGZ_OK and want is not None
    assert got.shape == want.shape == (16, f.W) and np.array_equal(got.astype(np.int64), want)
    assert int(np.abs(want).sum(axis=1).max()) << 26 < 1 << 62 and int(np.abs(want).max()) < 2 ** 31


def test_why_the_scale_is_30():
    """with the Oscilloscope's own filter at 22050 Hz one state component of the impulse response passes 0.5: no int32 at 2^32"""
    t = br.taps(api.band_filter_for_rate(22050))
    assert 0.5 < float(np.abs(t).max()) / 2 ** 30 < 0.6


def _refused(f):
    taps = np.full((16, 70000), 0x5A5A5A5A, np.int32)
    st = api.lib().sgz_band_taps(C.byref(f), taps.ctypes.data_as(C.c_void_p))
    assert st in (E, api.SGZ_OK) and (br.taps(f) is None) == (st == E)
    assert st == api.SGZ_OK or (taps == 0x5A5A5A5A).all(), "a refusal wrote the table"
    return st == E


def test_the_largest_table_is_decided_as_the_restatement_decides():
    assert not _refused(api.band_filter(br.TINY.c, 65536, 4096))
    assert not _refused(api.band_filter_for_rate(3276800, 300, 3000))
    slow = [list(r) for r in br.TINY.c]
    slow[0] = [0.0, 0.9, 0.0, -0.99999, 0.0]                        # a pole at 0.99999: 65536 taps near 0.9 * 2^30 each pass the sum's bound
    assert _refused(api.band_filter(slow, 65536, 4096))


def test_refused_filters():
    c = [list(r) for r in br.TINY.c]
    assert not _refused(tiny())
    for W, L in ((96, 16), (64, 24), (64, 8), (64, 128), (131072, 16), (0, 0), (64, 0)):
        assert _refused(api.band_filter(c, W, L)), (W, L)
    # a tap outside int32: z0 of lp1a after the first step is c1 - c3 c0 = 2.5 -> 2.5 * 2^30
    assert _refused(api.band_filter([[0.0, 2.5, 0.0, 0.0, 0.0]] + c[1:], 64, 16))
    # every tap inside int32, the sum of their magnitudes is not: a pole at 0.999 in lp1a and lp1b keeps lp1b's state near 0.0025 k 0.999^k
    slow = api.band_filter([[0.0, 0.05, 0.0, -0.999, 0.0]] + c[1:], 1024, 64)
    full = br.taps(br.Filter(coefs(slow), 1024, 1024))
    assert full is None and (0.0025 * np.arange(1024) * 0.999 ** np.arange(1024)).max() < 1      # (below 1 everywhere: it is the sum that refuses)
    t = br.taps(br.Filter(coefs(slow), 16, 16))
    assert t is not None and int(np.abs(t).max()) < 2 ** 31         # (the first 16 taps alone are accepted)
    assert _refused(slow)
    assert _refused(api.band_filter([[np.nan, 0.0, 0.0, 0.0, 0.0]] + c[1:], 64, 16))
    assert api.lib().sgz_band_taps(None, None) == E


def test_refused_designs():
    call = api.lib().sgz_band_filter_for_rate
    f = api.BandFilter()
    f.W = 0x5A5A
    for rate, low, high in ((48000.0, 0.0, 3000.0), (48000.0, -1.0, 3000.0), (48000.0, 300.0, 300.0), (48000.0, 300.0, 200.0), (48000.0, 300.0, 24000.0),
                            (48000.0, 300.0, 30000.0), (48000.0, 1.0, 3000.0), (0.0, 300.0, 3000.0), (-48000.0, 300.0, 3000.0), (np.nan, 300.0, 3000.0),
                            (np.inf, 300.0, 3000.0), (48000.0, np.nan, 3000.0), (48000.0, 300.0, np.nan)):
        assert call(rate, low, high, C.byref(f)) == E, (rate, low, high)
    assert f.W == 0x5A5A, "a refusal wrote the filter"
    assert call(48000.0, 300.0, 3000.0, None) == E
    assert call(48000.0, 4.4, 3000.0, C.byref(f)) == api.SGZ_OK and f.W == 65536        # 6 rate / low_hz = 65454.5: the largest W still fits


# ---- fold and readout --------------------------------------------------------------------------------------------------------------------------
def random_records(n, channels, seed, big=False):
    rng = np.random.default_rng(seed)
    r = np.zeros((n, channels), br.DTYPE)
    r["sumsq"][..., 0] = rng.integers(0, 2 ** 64, size=(n, channels, 3), dtype=np.uint64)
    r["sumsq"][..., 1] = rng.integers(0, 2 ** 20 if big else 4, size=(n, channels, 3), dtype=np.uint64)
    r["count"] = rng.integers(1, 5000, size=(n, channels))
    return r


def test_fold_equals_the_sums():
    r = random_records(37, 3, 1, big=True)
    for x0, x1 in ((0, 37), (3, 30), (36, 37)):
        for cols in (1, 2, 5, 36, 37, 100):
            got = api.band_fold(r, cols, x0, x1)
            want = br.fold(r, br.view_bounds(x0, x1, cols))
            assert got.tobytes() == want.tobytes(), (x0, x1, cols)
    # nested boundaries: a fold of a fold is the fold
    r = random_records(32, 2, 2, big=True)
    assert api.band_fold(api.band_fold(r, 8), 4).tobytes() == api.band_fold(r, 4).tobytes() == br.fold(r, [0, 8, 16, 24, 32]).tobytes()
    # the low words carry into the high ones, band by band
    r = np.zeros((2, 1), br.DTYPE)
    r["sumsq"][:, 0, 1, 0] = 2 ** 64 - 1
    got = api.band_fold(r, 1)
    assert got["sumsq"][0, 0].tolist() == [[0, 0], [2 ** 64 - 2, 1], [0, 0]]


def test_fold_refusals_write_nothing_and_the_count_limit():
    r = random_records(4, 1, 3)
    r["count"] = 2 ** 31
    out = np.full((4, 1), 0x5A, np.uint8).repeat(64, axis=1).view(br.DTYPE)
    before = out.tobytes()
    call = api.lib().sgz_band_fold
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                # noqa: E731
    assert call(ptr(r), 4, 1, 0, 4, 2, ptr(out)) == E            # 2^32 samples in a folded column
    assert out.tobytes() == before
    r["count"][1] = 2 ** 31 - 1                                  # 2^32 - 1 in the first folded column: the most a count holds
    r["count"][3] = 0
    assert call(ptr(r), 4, 1, 0, 4, 2, ptr(out)) == api.SGZ_OK and out["count"][:2, 0].tolist() == [2 ** 32 - 1, 2 ** 31]
    out[:] = np.frombuffer(before, br.DTYPE).reshape(out.shape)
    assert call(None, 4, 1, 0, 4, 2, ptr(out)) == E and call(ptr(r), 4, 0, 0, 4, 2, ptr(out)) == E and call(ptr(r), 4, 1, 0, 4, 2, None) == E
    assert call(ptr(r), 4, 1, 3, 3, 2, ptr(out)) == E and call(ptr(r), 4, 1, 0, 5, 2, ptr(out)) == E and call(ptr(r), 4, 1, 0, 4, 0, ptr(out)) == E
    assert out.tobytes() == before


def test_readout_against_fractions():
    for seed, channels in ((1, 1), (2, 2), (3, 5)):
        r = random_records(50, channels, seed, big=True)
        for a, n in ((0, 1), (3, 4), (10, 30), (0, 50)):
            for ch in range(channels):
                ms, db = api.band_readout(r[a:a + n], ch)
                want = br.mean_squares(r[a:a + n], ch)
                for b in range(3):
                    assert abs(Fraction(float(ms[b])) - want[b]) <= want[b] * Fraction(1, 10 ** 15), (seed, a, n, ch, b)
                    assert abs(db[b] - 10.0 * np.log10(float(want[b]))) < 1e-10
    z = np.zeros((10, 2), br.DTYPE)
    ms, db = api.band_readout(z, 1)
    assert ms.tolist() == [0.0] * 3 and np.isneginf(db).all()
    z["count"] = 4800
    ms, db = api.band_readout(z, 0)
    assert ms.tolist() == [0.0] * 3 and np.isneginf(db).all()
    call = api.lib().sgz_band_readout
    assert call(None, 1, 1, 0, None, None) == E and call(z.ctypes.data_as(C.c_void_p), 0, 2, 0, None, None) == E
    assert call(z.ctypes.data_as(C.c_void_p), 10, 2, 2, None, None) == E and call(z.ctypes.data_as(C.c_void_p), 10, 0, 0, None, None) == E
    assert call(z.ctypes.data_as(C.c_void_p), 10, 2, 1, None, None) == api.SGZ_OK                  # either result may be NULL


# ---- the colours ---------------------------------------------------------------------------------------------------------------------------------
RATE, M = 48000, 1024


def tone_records():
    """records [5 columns][2 channels] with the 48 kHz filter: a silent column (the first: behind a tone the filters still ring), a low tone, a
    mid tone, a high tone, a mixture; the second channel is the first at a tenth of the level"""
    t = np.arange(M) / RATE
    low, mid, high = (np.sin(2.0 * np.pi * hz * t) for hz in (80.0, 1000.0, 9000.0))
    x = np.concatenate([np.zeros(M), 0.5 * low, 0.5 * mid, 0.5 * high, 0.3 * low + 0.2 * mid + 0.25 * high]).astype(np.float32)
    r, _ = br.records_of(np.stack([x, (0.1 * x).astype(np.float32)]), rate_filter(RATE), M)
    return r


def test_colours_are_the_live_scopes_rule_byte_for_byte():
    r = tone_records()
    assert r.shape == (5, 2) and not r["sumsq"][0].any() and (r["count"] == M).all()
    colours = np.array([[1.0, 0.1, 0.0], [0.05, 0.9, 0.2], [0.0, 0.3, 1.0]], np.float32)         # band -> rgb
    keys = (np.array([200, 30, 90, 255], np.uint8), np.array([10, 250, 128, 77], np.uint8))
    accumulate = pyoracle.lib().sgzo_colour_accumulate
    seen = set()
    for ch in (0, 1):
        for blend in (0.0, 0.3, 1.0):
            got = api.band_colours(r, ch, colours, keys[ch], blend)
            assert got.shape == (5, 4) and got.dtype == np.uint8
            t = float(np.float32(1) - np.float32(blend))                                        # what enable_colours hands to the rule
            for col in range(5):
                state = np.array([float(v) for v in br.mean_squares(r[col:col + 1], ch)], np.float64).astype(np.float32)
                want = np.zeros(4, np.uint8)
                accumulate(state.ctypes.data_as(C.c_void_p), colours.ctypes.data_as(C.c_void_p), keys[ch].ctypes.data_as(C.c_void_p), C.c_float(t),
                           want.ctypes.data_as(C.c_void_p))
                assert got[col].tolist() == want.tolist(), (ch, blend, col)
                seen.add(tuple(got[col].tolist()))
    # the tones land where their band's colour is: with the key blended out, the strongest byte is red, green, blue
    pure = api.band_colours(r, 0, colours, keys[0], 1.0)
    assert [int(np.argmax(pure[i, :3])) for i in (1, 2, 3)] == [0, 1, 2] and pure[0].tolist() == [0, 0, 0, 255]
    assert api.band_colours(r, 0, colours, keys[0], 0.0)[2].tolist() == keys[0].tolist()          # blend 0: the key alone
    assert len(seen) > 12
    call = api.lib().sgz_band_colours
    p = lambda a: a.ctypes.data_as(C.c_void_p)                  # noqa: E731
    out = np.full((5, 4), 0x5A, np.uint8)
    assert call(None, 5, 2, 0, p(colours), p(keys[0]), 0.5, p(out)) == E and call(p(r), 5, 2, 0, None, p(keys[0]), 0.5, p(out)) == E
    assert call(p(r), 5, 2, 0, p(colours), None, 0.5, p(out)) == E and call(p(r), 5, 2, 0, p(colours), p(keys[0]), 0.5, None) == E
    assert call(p(r), 5, 2, 2, p(colours), p(keys[0]), 0.5, p(out)) == E and call(p(r), 5, 0, 0, p(colours), p(keys[0]), 0.5, p(out)) == E
    assert (out == 0x5A).all()


# ---- the segmentation against the unsegmented recurrence, reference against reference --------------------------------------------------------
# Measured here (these signals, this seed, 16384 samples): |q - rint(z_unsegmented)| <= 1 everywhere, z itself differs by at most 0.712 units of
# 2^-23 (44100 Hz, 1 kHz sine); the band energy of a 1024-sample column differs by at most 4.48e-5 of the column's total (48000 Hz, noise at
# 1e-4 rms, where rounding q to an integer dominates; 7.32e-5 with another draw of that noise), 3.85e-5 and 2.76e-5 for that noise at 44100
# and 8000 Hz, and 1.71e-7 or less on every other signal.  The bounds are the issue's: 4 units and 2e-4.
SIGNALS = ("noise at 0.2 rms", "noise at 1e-4 rms", "60 Hz sine", "1 kHz sine")
N_SEG = 16384


def signal(name, rate, seed=7):
    rng = np.random.default_rng(seed)
    t = np.arange(N_SEG) / rate
    x = {"noise at 0.2 rms": lambda: 0.2 * rng.standard_normal(N_SEG), "noise at 1e-4 rms": lambda: 1e-4 * rng.standard_normal(N_SEG),
         "60 Hz sine": lambda: 0.5 * np.sin(2.0 * np.pi * 60.0 * t), "1 kHz sine": lambda: 0.5 * np.sin(2.0 * np.pi * 1000.0 * t)}[name]()
    return x.astype(np.float32)


@pytest.mark.parametrize("rate", [48000, 44100, 8000])
def test_the_segmented_definition_stays_at_the_recurrence(rate):
    f = rate_filter(rate)
    for name in SIGNALS:
        v, _ = br.quantise(signal(name, rate))
        q = br.q_of(v, f)
        u = br.unsegmented_z(v, f)
        dq = float(np.abs(q - np.rint(u)).max())
        eq = (q.astype(np.float64) ** 2).reshape(3, -1, 1024).sum(axis=2)
        eu = (u ** 2).reshape(3, -1, 1024).sum(axis=2)
        rel = float((np.abs(eq - eu) / eu.sum(axis=0)).max())
        print(f"band segmentation at {rate} Hz, {name}: q differs by at most {dq:.0f} units of 2^-23, a column's band energy by {rel:.3e} of its total")
        assert dq <= 4
        assert rel <= 2e-4


# ---- the definition against the oracle's fp32 network -------------------------------------------------------------------------------------------
# Measured here (48000 Hz; 0.3 at 100 Hz + 0.2 at 1 kHz + 0.1 at 8 kHz; 8 columns of 1024): the column energy of the low band differs from the
# oracle's fp32 recurrence by at most 2.37e-5 of itself, the mid band's by 9.85e-7, the high band's by 9.09e-8 -- the fp32 recurrence's own
# rounding, largest where the poles sit closest to 1.  The bounds are four times that.
MEASURED_FP32 = (2.37e-5, 9.85e-7, 9.09e-8)


def test_band_energies_against_the_oracles_fp32_network():
    f = rate_filter(RATE)
    n = 8 * M
    t = np.arange(n) / RATE
    x = (0.3 * np.sin(2.0 * np.pi * 100.0 * t) + 0.2 * np.sin(2.0 * np.pi * 1000.0 * t) + 0.1 * np.sin(2.0 * np.pi * 8000.0 * t)).astype(np.float32)
    bands = pyoracle.lr_bands(x, float(RATE))
    r, _ = br.records_of(x[None, :], f, M)
    want = (bands.astype(np.float64) ** 2).reshape(-1, M, 3).sum(axis=1)                            # [columns][band]
    for b in range(3):
        got = np.array([float(v[0][b]) for v in br.total(r)]) / 2.0 ** 46
        rel = float((np.abs(got - want[:, b]) / want[:, b]).max())
        print(f"band {b}: column energy differs from the fp32 network's by at most {rel:.3e} of itself")
        assert rel <= 4.0 * MEASURED_FP32[b], (b, rel)
    # and the readout says the same: the three tones sit 3.5 dB apart in level and land in their bands
    ms, db = api.band_readout(r, 0)
    np.testing.assert_allclose(ms, [0.3 ** 2 / 2, 0.2 ** 2 / 2, 0.1 ** 2 / 2], rtol=0.05)
    np.testing.assert_allclose(db, 10.0 * np.log10(ms), atol=1e-12)


# ---- the exports, the header, the refusals made before the device is touched, the code objects -------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sgz_stage_band_columns", "sgz_band_columns_limits", "sgz_band_filter_for_rate", "sgz_band_taps", "sgz_band_fold", "sgz_band_readout",
         "sgz_band_colours", "sgz_pcm_stream_set_band", "sgz_pcm_stream_band_for", "sgz_pcm_stream_band_state", "sgz_pcm_stream_flush_band"]


def test_exports_and_the_header():
    import re
    L = api.lib()
    assert [n for n in NAMES if not hasattr(L, n)] == [] and [n for n in NAMES if n not in api.EXPORTS] == []
    assert L.sgz_abi_version() == 5 and api.BAND_DTYPE == br.DTYPE and api.BAND_DTYPE.itemsize == 64 and C.sizeof(api.BandFilter) == 168
    text = open(os.path.join(ROOT, "include", "sgz.h")).read()
    assert re.search(r"#define\s+SGZ_ABI_VERSION\s+5\b", text)
    history = text[:text.index("#define SGZ_ABI_VERSION")]
    assert "(5, later: the band lane" in history
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text) and n in history, n
    lane = text[text.index("/* The band lane"):]
    assert "exact, no tolerance" in lane[:1500] and text.index("/* The stereo-field lane") < text.index("/* The band lane")
    for line in ("y = c0*x + z0;   z0 = (c1*x - c3*y) + z1;   z1 = c2*x - c4*y",
                 "low = lp1b(lp1a(x));   rest = hp1b(hp1a(x));   mid = lp2b(lp2a(rest));   high = hp2b(hp2a(rest))",
                 "C[c][k] = (int32) rint(2^30 h[c][k])", "/* 168 bytes */", "/* 64 bytes */"):
        assert line in lane, line


def test_refusals_before_the_device_is_touched():
    """every argument check of the stage call and of the stream's calls that needs no device: made on fake, never dereferenced addresses"""
    L = api.lib()
    good, carry, out = 0x10000, 0x20000, 0x30000
    f = C.byref(tiny())
    call = L.sgz_stage_band_columns
    #          planar stride ch  n  f first m held flush cont slices carry out stream
    assert call(None, 128, 1, 100, f, 0, 8, 0, 1, 0, 0, carry, out, None) == E                  # a null d_planar
    assert call(good, 128, 1, 100, None, 0, 8, 0, 1, 0, 0, carry, out, None) == E               # a null filter
    assert call(good, 128, 1, 100, C.byref(api.band_filter(br.TINY.c, 64, 48)), 0, 8, 0, 1, 0, 0, carry, out, None) == E
    assert call(good, 128, 1, 100, C.byref(api.band_filter(br.TINY.c, 32768, 64)), 0, 8, 0, 1, 0, 0, carry, out, None) == E      # W > 16384 on the device
    assert call(good, 128, 0, 100, f, 0, 8, 0, 1, 0, 0, carry, out, None) == E                  # channels 0
    assert call(good, 128, 65, 100, f, 0, 8, 0, 1, 0, 0, carry, out, None) == E                 # channels above 64
    assert call(good, 128, 1, 100, f, 0, 0, 0, 1, 0, 0, carry, out, None) == E                  # m == 0
    assert call(good, 128, 1, 100, f, 0, 8, 8, 1, 1, 0, carry, out, None) == E                  # held >= m
    assert call(good, 128, 1, 100, f, 0, 8, 3, 1, 0, 0, carry, out, None) == E                  # held > 0 in a stream that begins here
    assert call(good, 99, 1, 100, f, 0, 8, 0, 1, 0, 0, carry, out, None) == E                   # channel_stride < nsamples
    assert call(good, 2 ** 41, 1, 2 ** 40 + 1, f, 0, 8, 0, 1, 0, 0, carry, out, None) == E      # nsamples above 2^40
    assert call(good, 128, 1, 100, f, 2 ** 63, 8, 0, 1, 0, 0, carry, out, None) == E            # first_index above 2^62
    assert call(good, 128, 1, 100, f, 0, 8, 0, 1, 0, 65, carry, out, None) == E                 # slices > 64
    assert call(good + 2, 128, 1, 100, f, 0, 8, 0, 1, 0, 0, carry, out, None) == E              # d_planar not aligned to 4
    assert call(good, 128, 1, 100, f, 0, 8, 3, 1, 1, 0, carry + 8, out, None) == E              # d_carry not aligned to 16
    assert call(good, 128, 1, 100, f, 0, 8, 0, 1, 0, 0, carry, out + 8, None) == E              # nor d_records
    assert call(good, 128, 1, 100, f, 0, 8, 0, 1, 0, 0, None, out, None) == E                   # the carry is written: samples arrive
    assert call(good, 128, 1, 0, f, 0, 8, 0, 1, 1, 0, None, out, None) == E                     # the carry is read: continued
    assert call(good, 128, 1, 100, f, 0, 8, 0, 1, 0, 0, carry, None, None) == E                 # columns close
    assert call(good, 128, 1, 0, f, 0, 8, 3, 1, 1, 0, carry, None, None) == E                   # the flushed carry is a column
    assert b"sgz_stage_band_columns" in L.sgz_last_error()
    assert call(good, 128, 1, 0, f, 0, 8, 0, 1, 0, 0, None, None, None) == api.SGZ_OK           # nothing arrives, nothing is flushed: nothing launched
    assert call(good, 128, 1, 0, f, 0, 8, 3, 0, 1, 0, carry, out, None) == api.SGZ_OK
    assert L.sgz_pcm_stream_set_band(None, f, 64, None, 0) == E and L.sgz_pcm_stream_flush_band(None) == E
    assert L.sgz_pcm_stream_band_state(None, None, None) == E and L.sgz_pcm_stream_band_for(None, 100, 0) == 0
    assert L.sgz_band_columns_limits(f, 2, None, None, None) == api.SGZ_OK                      # any result may be NULL


def test_band_kernels_need_no_scratch_and_do_not_contract():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_report as cr
    lib = os.path.join(ROOT, "signalizer_amd", "libsgz.so")
    if not (os.path.exists(lib) and os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("library or llvm tools not present")
    # (the history and sum kernels are column_lanes.hpp's templates, instantiated on this lane's kernel arguments)
    mine = "<(anonymous namespace)::BandParams"
    names = ("bandRunKernel", "historyKernel" + mine, "sumTileKernel" + mine, "sumSliceKernel" + mine, "sumEmitKernel" + mine)
    rows = [r for r in cr.kernels(lib) if any(k in r["demangled"] for k in names)]
    assert len(rows) == 5, [r["demangled"] for r in rows]
    bad = [(r["demangled"], r.get("vgpr_spill_count"), r.get("sgpr_spill_count"), r.get("private_segment_fixed_size")) for r in rows
           if r.get("vgpr_spill_count", 0) or r.get("sgpr_spill_count", 0) or r.get("private_segment_fixed_size", 0)]
    assert not bad, bad
    # the run's recurrence is one IEEE operation per *, + and -: the kernel multiplies and adds in fp64 and holds no fused multiply-add
    import subprocess
    import tempfile
    objdump = f"{cr.LLVM}/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not present")
    found = 0
    for elf in cr.code_objects(lib):
        if b"bandRunKernel" not in elf:
            continue
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(elf)
            f.flush()
            text = subprocess.run([objdump, "-d", f.name], check=True, capture_output=True, text=True).stdout
        body = text[text.index("bandRunKernel"):]
        body = body[:body.index("\n\n")] if "\n\n" in body else body
        assert "v_mul_f64" in body and "v_add_f64" in body and "v_mad_i64_i32" in body and "v_fma_f64" not in body
        found += 1
    assert found == 1
