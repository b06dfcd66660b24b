"""The level lane (sgz.h, "The level lane"): what needs no GPU -- the exports, the header, tests/level_ref.py against a brute-force loop and
corners by hand, the fold of finer records into coarser ones (sgz_level_fold), the readout (sgz_level_readout) against exact rationals, the
refusals made before the device is touched, and the new kernels' code objects.  Records are compared as bytes."""
import math
import os
import re
import struct
import sys
from fractions import Fraction

import numpy as np
import pytest

from signalizer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import level_ref as lr  # noqa: E402
import wave_ref as wr  # noqa: E402

NAMES = ["sgz_stage_level_columns", "sgz_level_columns_limits", "sgz_pcm_stream_set_level", "sgz_pcm_stream_level_for",
         "sgz_pcm_stream_level_state", "sgz_pcm_stream_flush_level", "sgz_level_fold", "sgz_level_readout"]
E = api.SGZ_EINVAL


def _same(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a, lr.DTYPE).tobytes() == np.ascontiguousarray(b, lr.DTYPE).tobytes()


def test_exports_exist():
    L = api.lib()
    assert [n for n in NAMES if not hasattr(L, n)] == []
    assert [n for n in NAMES if n not in api.EXPORTS] == []
    assert L.sgz_abi_version() == 5
    assert api.LEVEL_DTYPE == lr.DTYPE and api.LEVEL_DTYPE.itemsize == 80


def test_header_names_them_and_keeps_version_5():
    text = open(os.path.join(ROOT, "include", "sgz.h")).read()
    assert re.search(r"#define\s+SGZ_ABI_VERSION\s+5\b", text)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n                    # declared
    history = text[:text.index("#define SGZ_ABI_VERSION")]
    assert [n for n in NAMES if n not in history] == []                # and listed under the version-5 entry
    lane = text[text.index("/* The level lane"):]
    assert "has no counterpart" in lane[:700] and "sgz_level_record" in lane and text.index("/* The waveform lane") < text.index("/* The level lane")
    for field in ("uint64_t sumsq[2][2]", "uint64_t cross[2]", "int64_t  sum[2]", "uint32_t count[2]", "uint32_t overs[2]"):
        assert field in lane, field


def test_limits_are_the_documented_ones():
    switch, tile = api.level_columns_limits()
    assert 1 <= switch <= min(tile, 1024) and tile % 4 == 0, (switch, tile)       # 1024: what 64-bit accumulators take (2^52 a term)
    text = open(os.path.join(ROOT, "include", "sgz.h")).read()
    lane = text[text.index("/* The level lane"):]
    assert f"({switch};" in lane and f"{tile} / m" in lane


def _q(x):
    """the quantiser on one Python float that holds an fp32 value: None for a NaN.  round() is ties-to-even on exact rationals"""
    if x != x:
        return None
    if math.isinf(x):
        return lr.CLAMP if x > 0 else -lr.CLAMP
    return max(-lr.CLAMP, min(lr.CLAMP, round(Fraction(x) * lr.FULL)))


def _brute(x, m, flush):
    """the definition, sample by sample, on Python integers"""
    pairs, S = x.shape[0] // 2, x.shape[1]
    columns = S // m + (1 if flush and S % m else 0)
    out = np.zeros((columns, pairs), lr.DTYPE)
    for c in range(columns):
        for p in range(pairs):
            sq, cross, sums, count, overs = [0, 0], 0, [0, 0], [0, 0], [0, 0]
            for i in range(c * m, min((c + 1) * m, S)):
                v = [_q(float(x[2 * p, i])), _q(float(x[2 * p + 1, i]))]
                for ch in range(2):
                    if v[ch] is not None:
                        sq[ch] += v[ch] * v[ch]
                        sums[ch] += v[ch]
                        count[ch] += 1
                        overs[ch] += abs(v[ch]) >= lr.FULL
                if v[0] is not None and v[1] is not None:
                    cross += v[0] * v[1]
            out[c, p] = lr.pack(sq, cross, sums, count, overs)
    return out


def test_level_ref_against_a_brute_force_loop():
    rng = np.random.default_rng(11)
    cases = 0
    for trial in range(300):
        S = int(rng.integers(0, 65))
        m = int(rng.choice([1, 2, 3, 7, int(rng.integers(1, 70))]))
        pairs = int(rng.integers(1, 3))
        x = wr.content(["random", "constant", "ramp"][trial % 3], 2 * pairs, S, m, seed=trial)
        if trial % 5 == 0 and S:
            with np.errstate(all="ignore"):                             # some of it above full scale and above the clamp
                x = (x.astype(np.float64) * 7.0).clip(-3e38, 3e38).astype(np.float32)
        if S:                                                           # more specials than content() sprinkles: a third of the samples
            b = x.view(np.uint32)
            pick = rng.random(x.shape) < 0.33
            b[pick] = wr.SPECIALS[rng.integers(0, len(wr.SPECIALS), size=int(pick.sum()))]
        for flush in (True, False):
            got, left = lr.records_of(x, m, flush)
            assert left == (0 if flush else S % m)
            assert _same(got, _brute(x, m, flush)), (trial, S, m, pairs, flush)
            cases += 1
    assert cases == 600


def _one(l, r):
    """the record of one sample frame, as integers"""
    x = np.array([[l], [r]], np.float32)
    return lr.unpack(lr.records_of(x, 1)[0][0, 0])


def test_corners_by_hand():
    u = 2.0 ** -23
    # ties to even at x 2^23 = +-0.5, +-1.5, +-2.5
    for x, v in ((0.5 * u, 0), (-0.5 * u, 0), (1.5 * u, 2), (-1.5 * u, -2), (2.5 * u, 2), (-2.5 * u, -2)):
        got = _one(x, x)
        assert got["sum"] == [v, v] and got["sq"] == [v * v, v * v] and got["cross"] == v * v and got["count"] == [1, 1], (x, got)
    # the clamp: the last value below it, the clamp itself, above it, the infinities
    # (8 - 2^-23 is no fp32 value: as one it IS 8.0; the last one below 8.0 is 8 - 2^-21)
    assert float(np.float32(8.0 - u)) == 8.0
    top = 8.0 - 4 * u
    assert float(np.float32(top)) == top
    for x, v in ((top, 2**26 - 4), (-top, -(2**26 - 4)), (8.0 - u, 2**26), (-(8.0 - u), -2**26), (8.0, 2**26), (-8.0, -2**26), (8.5, 2**26), (-1e30, -2**26), (math.inf, 2**26), (-math.inf, -2**26)):
        got = _one(x, -x)
        assert got["sum"] == [v, -v] and got["sq"] == [v * v, v * v] and got["cross"] == -v * v and got["overs"] == [1, 1], (x, got)
    # denormals quantise to 0 and count
    for bits in (0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF):
        x = struct.unpack("<f", struct.pack("<I", bits))[0]
        got = _one(x, 1.0)
        assert got["sum"] == [0, 2**23] and got["sq"] == [0, 2**46] and got["cross"] == 0 and got["count"] == [1, 1] and got["overs"] == [0, 1]
    # overs: |x| = 1 - 2^-24 is the last fp32 value below 1.0 and already an over, 1 - 2^-22 is not, 1.0 is
    below = 1.0 - 2.0 ** -24
    assert float(np.float32(below)) == below
    got = _one(below, -below)                                        # (1 - 2^-24) 2^23 = 2^23 - 0.5: a tie, to the even 2^23
    assert got["sum"] == [2**23, -(2**23)] and got["overs"] == [1, 1]
    got = _one(1.0 - 2.0 ** -22, 1.0)
    assert got["sum"] == [2**23 - 2, 2**23] and got["overs"] == [0, 1]
    # a NaN on one side of a pair only: that side takes no part, the cross term neither
    nan = struct.unpack("<f", struct.pack("<I", 0x7F800001))[0]
    x = np.array([[0.5, nan, 0.25], [0.5, 0.5, nan]], np.float32)
    got = lr.unpack(lr.records_of(x, 3)[0][0, 0])
    assert got["count"] == [2, 2] and got["sum"] == [2**22 + 2**21, 2**23] and got["cross"] == 2**44 and got["sq"] == [2**44 + 2**42, 2**45]
    # a column of NaNs alone is the all-zero record
    rec = lr.records_of(np.full((2, 4), np.nan, np.float32), 4)[0]
    assert rec.tobytes() == bytes(80)
    # the library's brute restatement agrees on these too
    assert _same(lr.records_of(x, 3)[0], _brute(x, 3, True))


def test_the_quantiser_in_fp32_and_in_fp64_give_the_same_integers():
    rng = np.random.default_rng(4)
    bits = rng.integers(0, 2**32, size=400000, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32)
    ok = ~lr.is_nan(x)
    with np.errstate(over="ignore", invalid="ignore"):
        f32 = np.clip(np.rint(x[ok] * np.float32(2.0**23)), np.float32(-2.0**26), np.float32(2.0**26)).astype(np.int64)
    v, has = lr.quantise(x)
    assert np.array_equal(has, ok) and np.array_equal(v[ok], f32) and not v[~ok].any()


def test_a_coarser_column_is_the_fold_of_the_finer_ones():
    rng = np.random.default_rng(5)
    for trial in range(40):
        S = int(rng.integers(1, 400))
        m = int(rng.integers(1, 9))
        r = int(rng.integers(2, 6))                                     # the coarser column: r finer ones
        x = lr.saturated(4, S, trial) if trial % 4 == 0 else wr.content("random", 4, S, m, seed=100 + trial)
        fine, _ = lr.records_of(x, m)
        coarse, _ = lr.records_of(x, m * r)
        n = fine.shape[0]
        bounds = list(range(0, n, r)) + [n]
        assert _same(lr.fold(fine, bounds), coarse), (trial, S, m, r)
        # the library's fold where its boundary rule gives these boundaries: n a multiple of r
        if n % r == 0:
            assert lr.view_bounds(0, n, n // r) == bounds
            assert _same(api.level_fold(fine, n // r), coarse), (trial, S, m, r)
        # nested: a fold of a fold is the direct fold
        twice, _ = lr.records_of(x, m * r * 2)
        n2 = coarse.shape[0]
        assert _same(lr.fold(coarse, list(range(0, n2, 2)) + [n2]), twice), (trial, S, m, r)
        if n % (2 * r) == 0:
            assert _same(api.level_fold(api.level_fold(fine, n // r), n2 // 2), twice), (trial, S, m, r)


def test_level_fold_against_brute_force_boundaries():
    rng = np.random.default_rng(6)
    x = lr.saturated(4, 64 * 40, 9)
    x[:, ::3] = wr.content("random", 4, 64 * 40, 7, seed=3)[:, ::3]
    records, _ = lr.records_of(x, 40)                                  # 64 columns, two pairs
    huge = records.copy()
    huge["sumsq"][:, :, :, 1] = np.uint64(0x7FFFFFFFFFFFFFFF)          # high words that carry on
    huge["cross"][:, :, 1] ^= np.uint64(0x4000000000000000)
    assert records.shape == (64, 2)
    for src in (records, huge):
        for n in range(1, 65):
            for out_columns in sorted({1, 2, 3, n // 2 + 1, n, n + 5, int(rng.integers(1, n + 1))}):
                x0 = int(rng.integers(0, n))
                x1 = int(rng.integers(x0 + 1, n + 1))
                for a, b in ((0, n), (x0, x1)):
                    w, cols = b - a, min(out_columns, b - a)
                    bounds = [a + (k * w + cols - 1) // cols for k in range(cols + 1)]
                    assert bounds == lr.view_bounds(a, b, out_columns) and bounds[0] == a and bounds[-1] == b
                    got = api.level_fold(src[:n], out_columns, a, b)
                    assert _same(got, lr.fold(src[:n], bounds)), (n, out_columns, a, b)


def test_level_fold_refusals():
    L = api.lib()
    rec = np.zeros((4, 1), lr.DTYPE)
    out = np.full((4, 1), 0xAB, np.uint8).repeat(80, axis=1).view(lr.DTYPE)
    before = out.tobytes()
    p, q = rec.ctypes.data, out.ctypes.data
    assert L.sgz_level_fold(None, 4, 1, 0, 4, 2, q) == E and L.sgz_level_fold(p, 4, 1, 0, 4, 2, None) == E
    assert L.sgz_level_fold(p, 4, 0, 0, 4, 2, q) == E                  # pairs == 0
    assert L.sgz_level_fold(p, 4, 1, 2, 2, 2, q) == E                  # x0 >= x1
    assert L.sgz_level_fold(p, 4, 1, 0, 5, 2, q) == E                  # x1 > n
    assert L.sgz_level_fold(p, 4, 1, 0, 4, 0, q) == E                  # out_columns == 0
    rec["count"][:, 0, 1] = 2**31                                      # two of them: a count of 2^32
    assert L.sgz_level_fold(p, 4, 1, 0, 4, 3, q) == E and b"2^32" in L.sgz_last_error()
    assert out.tobytes() == before
    assert L.sgz_level_fold(p, 4, 1, 0, 4, 4, q) == api.SGZ_OK and out.tobytes() == rec.tobytes()       # one to one: nothing folds
    rec["count"][:, 0, 1] = (2**32 - 1) // 4                           # the largest that fits
    assert L.sgz_level_fold(p, 4, 1, 0, 4, 1, q) == api.SGZ_OK and int(out["count"][0, 0, 1]) == 4 * ((2**32 - 1) // 4)


def _exact(u):
    """the readout of a record's integers as exact rationals / correctly rounded floats (math.sqrt and the division of big integers are exact
    to the last bit; log10 takes the integer itself)"""
    out = dict(rms=[], rms_db=[], dc=[])
    for c in range(2):
        n, sq = u["count"][c], u["sq"][c]
        if n == 0:
            out["rms"].append(math.nan); out["rms_db"].append(math.nan); out["dc"].append(math.nan)
            continue
        ms = Fraction(sq, n << 46)
        out["rms"].append(math.sqrt(ms))
        out["rms_db"].append(-math.inf if sq == 0 else 10.0 * (math.log10(ms.numerator) - math.log10(ms.denominator)))
        out["dc"].append(float(Fraction(u["sum"][c], n << 23)))
    prod = u["sq"][0] * u["sq"][1]
    out["correlation"] = 0.0 if prod == 0 else float(Fraction(u["cross"]) / Fraction(math.isqrt(prod << 200), 1 << 100))
    return out


def _close(got, want, rel):
    if want != want:
        return got != got
    if want == 0 or math.isinf(want):
        return got == want
    return abs(got - want) <= rel * abs(want)


def test_readout_against_exact_rationals():
    """The bars are derived, not measured: rms, dc and correlation go through about ten fp64 roundings of 1.1e-16 each (the conversions of the
    words, the products, a division, a square root) -- 1e-12 relative leaves three decimal orders; rms_db adds libm's log10, good to under
    1 ulp of a value below 20 in magnitude (3.6e-15), times 10 -- 1e-11 dB absolute."""
    rng = np.random.default_rng(8)
    cases = []
    for trial in range(60):                                            # records of real content, short and long columns
        S = int(rng.integers(1, 5000))
        with np.errstate(all="ignore"):
            x = lr.saturated(2, S, trial) if trial % 3 == 0 else wr.content("random", 2, S, 7, seed=trial) * np.float32(10.0 ** rng.uniform(-6, 1))
        cases.append(lr.unpack(lr.records_of(x, S)[0][0, 0]))
    cases.append(dict(sq=[25, 1], cross=-5, sum=[-5, 1], count=[1, 1], overs=[0, 0]))                    # hi 2^64 + lo of -5 would cancel to 0
    cases.append(dict(sq=[3 << 70, (1 << 83) + 12345], cross=-((1 << 76) + 99), sum=[-(1 << 57), 12345], count=[2**32 - 1, 2**31], overs=[7, 0]))
    cases.append(dict(sq=[(1 << 127) + 5, 1 << 100], cross=(1 << 113) - 1, sum=[1, -1], count=[1000, 1000], overs=[0, 0]))  # folded: above a column's bounds
    cases.append(dict(sq=[0, 0], cross=0, sum=[0, 0], count=[0, 0], overs=[0, 0]))                       # count 0
    cases.append(dict(sq=[0, 0], cross=0, sum=[0, 0], count=[512, 512], overs=[0, 0]))                   # silence
    cases.append(dict(sq=[1 << 46, 0], cross=0, sum=[1 << 23, 0], count=[1, 0], overs=[1, 0]))           # one side without samples
    assert any(u["cross"] < 0 for u in cases) and any(u["sq"][0] >> 64 for u in cases)
    for u in cases:
        got = api.level_readout(lr.pack(u["sq"], u["cross"], u["sum"], u["count"], u["overs"]))
        want = _exact(u)
        for c in range(2):
            assert _close(got["rms"][c], want["rms"][c], 1e-12), (u, got, want)
            assert _close(got["dc"][c], want["dc"][c], 1e-12), (u, got, want)
            w = want["rms_db"][c]
            assert (got["rms_db"][c] != got["rms_db"][c]) if w != w else (got["rms_db"][c] == w if math.isinf(w) else abs(got["rms_db"][c] - w) <= 1e-11), (u, got, want)
        assert _close(got["correlation"], want["correlation"], 1e-12), (u, got, want)
    got = api.level_readout(lr.pack([25, 1], -5, [-5, 1], [1, 1], [0, 0]))
    assert got["correlation"] == -1.0 and got["dc"] == (-5 / 2**23, 1 / 2**23)
    silent = api.level_readout(lr.pack([0, 0], 0, [0, 0], [512, 512], [0, 0]))
    assert silent["rms"] == (0.0, 0.0) and silent["rms_db"] == (-math.inf, -math.inf) and silent["correlation"] == 0.0
    assert api.lib().sgz_level_readout(None, None) == E


def test_refusals_before_the_device_is_touched():
    """every argument check of the stage call and of the stream's calls that needs no device: made on fake, never dereferenced addresses"""
    L = api.lib()
    good, carry, level = 0x10000, 0x20000, 0x30000
    call = L.sgz_stage_level_columns
    assert call(None, 128, 1, 100, 8, 0, 1, 0, carry, level, None) == E                    # a null d_planar
    assert call(good, 128, 0, 100, 8, 0, 1, 0, carry, level, None) == E                    # pairs 0
    assert call(good, 128, 33, 100, 8, 0, 1, 0, carry, level, None) == E                   # pairs above 32
    assert call(good, 128, 1, 100, 0, 0, 1, 0, carry, level, None) == E                    # m == 0
    assert call(good, 128, 1, 100, 8, 8, 1, 0, carry, level, None) == E                    # held >= m
    assert call(good, 99, 1, 100, 8, 0, 1, 0, carry, level, None) == E                     # channel_stride < nsamples
    assert call(good, 128, 1, 100, 8, 0, 1, 65, carry, level, None) == E                   # slices > 64
    assert call(good + 2, 128, 1, 100, 8, 0, 1, 0, carry, level, None) == E                # d_planar not aligned to 4
    assert call(good, 128, 1, 100, 8, 3, 1, 0, carry + 8, level, None) == E                # d_carry not aligned to 16
    assert call(good, 128, 1, 100, 8, 0, 1, 0, carry, level + 8, None) == E                # nor d_level
    assert call(good, 128, 1, 100, 8, 3, 1, 0, None, level, None) == E                     # the carry is read: held > 0
    assert call(good, 128, 1, 100, 8, 0, 0, 0, None, level, None) == E                     # the carry is written: 100 % 8 samples stay open
    assert call(good, 128, 1, 100, 8, 0, 1, 0, carry, None, None) == E                     # columns close
    assert call(good, 128, 1, 0, 8, 3, 1, 0, carry, None, None) == E                       # the flushed carry is a column
    assert b"sgz_stage_level_columns" in L.sgz_last_error()
    assert call(good, 128, 1, 0, 8, 0, 1, 0, None, None, None) == api.SGZ_OK               # nothing arrives, nothing is flushed: nothing launched
    assert call(good, 128, 1, 0, 8, 3, 0, 0, carry, level, None) == api.SGZ_OK
    # the stream's calls on a null stream
    assert L.sgz_pcm_stream_set_level(None, 8, None, 0) == E and L.sgz_pcm_stream_flush_level(None) == E
    assert L.sgz_pcm_stream_level_state(None, None, None) == E and L.sgz_pcm_stream_level_for(None, 100, 0) == 0
    L.sgz_level_columns_limits(None, None)                                                 # either result may be NULL


def test_level_kernels_need_no_scratch():
    import codeobj_report as cr
    lib = os.path.join(ROOT, "signalizer_amd", "libsgz.so")
    if not (os.path.exists(lib) and os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("library or llvm tools not present")
    rows = [r for r in cr.kernels(lib) if any(k in r["demangled"] for k in ("levelTileKernel", "levelSliceKernel", "levelEmitKernel"))]
    assert len(rows) == 3, [r["demangled"] for r in rows]
    bad = [(r["demangled"], r.get("vgpr_spill_count"), r.get("sgpr_spill_count"), r.get("private_segment_fixed_size")) for r in rows
           if r.get("vgpr_spill_count", 0) or r.get("sgpr_spill_count", 0) or r.get("private_segment_fixed_size", 0)]
    assert not bad, bad
