"""The true-peak lane (sgz.h, "The true-peak lane"): what needs no GPU -- the exports, the tap table, the struct sizes, tests/truepeak_ref.py
against a brute-force loop on Python integers, what the meter reads on sines (a property of the definition), the fold of finer records into
coarser ones (sgz_truepeak_fold), the readout (sgz_truepeak_readout), the refusals made before the device is touched, and the new kernels'
code objects.  Records are compared as bytes."""
import ctypes as C
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
import truepeak_ref as tr  # noqa: E402

NAMES = ["sgz_stage_truepeak_columns", "sgz_truepeak_columns_limits", "sgz_truepeak_taps", "sgz_truepeak_fold", "sgz_truepeak_readout",
         "sgz_pcm_stream_set_truepeak", "sgz_pcm_stream_truepeak_for", "sgz_pcm_stream_truepeak_state", "sgz_pcm_stream_flush_truepeak"]
E = api.SGZ_EINVAL
# the issue's table, as literals
LITERAL = [[0, 0, 0, 0, 0, 0, 1048576, 0, 0, 0, 0, 0],
           [-1780, 12162, -29613, 59093, -116769, 306657, 941356, -175616, 82260, -42310, 19798, -6258],
           [-5454, 22259, -50264, 98518, -200334, 659945, 659945, -200334, 98518, -50264, 22259, -5454],
           [-6258, 19798, -42310, 82260, -175616, 941356, 306657, -116769, 59093, -29613, 12162, -1780]]
SPECIALS = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF,
                     0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x42C80000, 0xC2C80000], np.uint32)   # NaNs, +-inf, +-0, denormals, +-FLT_MAX, +-100


def _same(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a, tr.DTYPE).tobytes() == np.ascontiguousarray(b, tr.DTYPE).tobytes()


def test_exports_exist():
    L = api.lib()
    assert [n for n in NAMES if not hasattr(L, n)] == []
    assert [n for n in NAMES if n not in api.EXPORTS] == []
    assert L.sgz_abi_version() == 5
    assert api.TRUEPEAK_DTYPE == tr.DTYPE and api.TRUEPEAK_CARRY_DTYPE == tr.CARRY_DTYPE


def test_header_names_them_and_keeps_version_5():
    text = open(os.path.join(ROOT, "include", "sgz.h")).read()
    assert re.search(r"#define\s+SGZ_ABI_VERSION\s+5\b", text)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n
    history = text[:text.index("#define SGZ_ABI_VERSION")]
    assert [n for n in NAMES if n not in history] == []
    lane = text[text.index("/* The true-peak lane"):]
    assert "has no counterpart" in lane[:700] and "BS.1770" in lane[:900] and text.index("/* The level lane") < text.index("/* The true-peak lane")
    for row in LITERAL[1:3]:
        assert "  ".join(str(v) for v in row) in lane, row


def test_taps():
    taps = api.truepeak_taps()
    assert taps.dtype == np.int32 and taps.shape == (4, 12)
    assert np.array_equal(taps, tr.C) and taps.tolist() == LITERAL
    assert all(taps[3][j] == taps[1][11 - j] for j in range(12)) and np.array_equal(taps[2], taps[2][::-1])
    sums = np.abs(taps.astype(np.int64)).sum(axis=1).tolist()
    assert sums == [1048576, 1793672, 2073548, 1793672]
    assert max(sums) * 2**26 < 2**47 < 2**53


def test_struct_sizes():
    class Record(C.Structure):
        _fields_ = [("peak", C.c_uint64), ("count", C.c_uint32), ("overs", C.c_uint32)]

    class Carry(C.Structure):
        _fields_ = [("open", Record), ("hist", C.c_int32 * 11), ("reserved", C.c_uint32)]
    assert C.sizeof(Record) == 16 == tr.DTYPE.itemsize and C.sizeof(Carry) == 64 == tr.CARRY_DTYPE.itemsize
    assert Carry.hist.offset == 16 == tr.CARRY_DTYPE.fields["hist"][1] and Carry.reserved.offset == 60 == tr.CARRY_DTYPE.fields["reserved"][1]


def test_limits_are_the_documented_ones():
    switch, tile = api.truepeak_columns_limits()
    assert 1 <= switch <= tile and tile % 4 == 0, (switch, tile)
    text = open(os.path.join(ROOT, "include", "sgz.h")).read()
    lane = text[text.index("/* The true-peak lane"):]
    assert f"({switch};" in lane and f"{tile} / m" in lane


def _q(x):
    """the quantiser on one Python float that holds an fp32 value: (v, counted)"""
    if x != x:
        return 0, False
    if math.isinf(x):
        return (tr.CLAMP if x > 0 else -tr.CLAMP), True
    return max(-tr.CLAMP, min(tr.CLAMP, round(Fraction(x) * tr.FULL))), True


def _brute(x, m, flush, table=LITERAL):
    """the definition, sample by sample, on Python integers and the literal table"""
    channels, S = x.shape
    columns = S // m + (1 if flush and S % m else 0)
    out = np.zeros((columns, channels), tr.DTYPE)
    for d in range(channels):
        q = [_q(float(v)) for v in x[d]]
        v = [a for a, _ in q]
        for c in range(columns):
            peak = count = overs = 0
            for i in range(c * m, min((c + 1) * m, S)):
                ys = [abs(sum(table[ph][j] * v[i - j] for j in range(12) if i - j >= 0)) for ph in range(4)]
                peak = max(peak, max(ys))
                count += q[i][1]
                overs += max(ys) >= 2**43
            out[c, d] = (peak, count, overs)
    return out


def _content(rng, channels, S, trial):
    kind = trial % 4
    if kind == 0:
        x = rng.standard_normal((channels, S)).astype(np.float32)
    elif kind == 1:
        x = np.full((channels, S), 0.75, np.float32)
    elif kind == 2:
        x = np.linspace(-1.5, 1.5, max(S, 1), dtype=np.float32)[None, :S].repeat(channels, axis=0).copy()
    else:
        x = tr.saturated(channels, S, trial)
    if trial % 5 == 0:
        x = (x * np.float32(7.0)).astype(np.float32)
    return x


def test_truepeak_ref_against_a_brute_force_loop():
    rng = np.random.default_rng(11)
    cases = 0
    for trial in range(200):
        S = int(rng.integers(0, 65))
        m = int(rng.choice([1, 2, 3, 7, 11, 12, int(rng.integers(1, 70))]))
        channels = int(rng.integers(1, 4))
        x = _content(rng, channels, S, trial)
        if S and trial % 2:                                             # NaN, +-inf, +-100, denormals: a third of the samples
            b = x.view(np.uint32)
            pick = rng.random(x.shape) < 0.33
            b[pick] = SPECIALS[rng.integers(0, len(SPECIALS), size=int(pick.sum()))]
        for flush in (True, False):
            got, left = tr.records_of(x, m, flush)
            assert left == (0 if flush else S % m)
            assert _same(got, _brute(x, m, flush)), (trial, S, m, channels, flush)
            cases += 1
    assert cases == 400


def test_an_impulse_reads_the_table():
    for a in (1.0, -0.5, 2.0 ** -23):
        v = int(abs(a) * 2**23)
        x = np.zeros((1, 40), np.float32)
        x[0, 3] = a
        got, _ = tr.records_of(x, 1)
        for k in range(40):
            want = max(abs(LITERAL[q][k - 3]) for q in range(4)) * v if 0 <= k - 3 < 12 else 0
            assert int(got["peak"][k, 0]) == want and int(got["count"][k, 0]) == 1, (a, k)
        assert int(got["overs"].sum()) == (1 if v >= 2**23 else 0)                        # only the sample itself (phase 0, six later) reaches 2^43
    # a NaN is silence and is not counted; an all-NaN column is the zero record but for nothing
    x = np.full((1, 8), np.nan, np.float32)
    assert tr.records_of(x, 8)[0].tobytes() == bytes(16)
    x[0, 2] = 0.5
    r = tr.records_of(x, 8)[0][0, 0]
    assert int(r["count"]) == 1 and int(r["peak"]) == max(abs(LITERAL[q][j]) for q in range(4) for j in range(6)) * 2**22
    # saturation: the bound is reached
    x = tr.saturated(1, 12, 0)
    assert int(tr.records_of(x, 12)[0]["peak"][0, 0]) == 2**26 * 2073548


def _reading(x):
    """max |y| / 2^43 over the samples behind the filter's start-up"""
    v, _ = tr.quantise(x)
    return float(tr.outputs(v)[24:].max()) / 2.0**43


def test_the_meter_reads_a_sine_within_three_per_cent():
    n = np.arange(4096, dtype=np.float64)
    lo, hi = 10.0, 0.0
    for f in (0.01, 0.05, 0.125, 0.2, 0.25, 0.3, 0.375, 0.42, 0.45):
        for k in range(64):
            x = (0.5 * np.sin(2.0 * np.pi * f * n + np.pi * k / 64.0)).astype(np.float32)
            r = _reading(x) / 0.5
            lo, hi = min(lo, r), max(hi, r)
            assert 0.97 <= r <= 1.03, (f, k, r)
    print("sine readings: %.4f .. %.4f" % (lo, hi))


def test_the_fs4_sine_at_45_degrees_reads_its_true_peak():
    n = np.arange(4096, dtype=np.float64)
    x = (0.9 * np.sin(2.0 * np.pi * 0.25 * n + np.pi / 4.0)).astype(np.float32)
    sample_peak = float(np.abs(x).max())
    peak = _reading(x)
    assert abs(sample_peak - 0.6364) < 1e-4
    assert 0.97 * 0.9 <= peak <= 1.03 * 0.9 and peak > 1.3 * sample_peak, (peak, sample_peak)
    assert abs(peak - 0.8973) < 5e-4, peak


def test_a_coarser_column_is_the_fold_of_the_finer_ones():
    rng = np.random.default_rng(5)
    for trial in range(40):
        S = int(rng.integers(1, 400))
        m = int(rng.integers(1, 9))
        r = int(rng.integers(2, 6))
        x = _content(rng, 3, S, trial)
        fine, _ = tr.records_of(x, m)
        coarse, _ = tr.records_of(x, m * r)
        n = fine.shape[0]
        bounds = list(range(0, n, r)) + [n]
        assert _same(tr.fold(fine, bounds), coarse), (trial, S, m, r)
        if n % r == 0:
            assert tr.view_bounds(0, n, n // r) == bounds
            assert _same(api.truepeak_fold(fine, n // r), coarse), (trial, S, m, r)
        twice, _ = tr.records_of(x, m * r * 2)
        n2 = coarse.shape[0]
        assert _same(tr.fold(coarse, list(range(0, n2, 2)) + [n2]), twice), (trial, S, m, r)
        if n % (2 * r) == 0:
            assert _same(api.truepeak_fold(api.truepeak_fold(fine, n // r), n2 // 2), twice), (trial, S, m, r)


def test_truepeak_fold_against_brute_force_boundaries():
    rng = np.random.default_rng(6)
    records, _ = tr.records_of((rng.standard_normal((2, 64 * 40)) * 0.7).astype(np.float32), 40)
    assert records.shape == (64, 2)
    for n in range(1, 65):
        for out_columns in sorted({1, 2, 3, n // 2 + 1, n, n + 5, int(rng.integers(1, n + 1))}):
            x0 = int(rng.integers(0, n))
            x1 = int(rng.integers(x0 + 1, n + 1))
            for a, b in ((0, n), (x0, x1)):
                w, cols = b - a, min(out_columns, b - a)
                bounds = [a + (k * w + cols - 1) // cols for k in range(cols + 1)]
                assert bounds == tr.view_bounds(a, b, out_columns) and bounds[0] == a and bounds[-1] == b
                assert _same(api.truepeak_fold(records[:n], out_columns, a, b), tr.fold(records[:n], bounds)), (n, out_columns, a, b)


def test_truepeak_fold_refusals():
    L = api.lib()
    rec = np.zeros((4, 1), tr.DTYPE)
    out = np.full((4, 16), 0xAB, np.uint8).view(tr.DTYPE)
    before = out.tobytes()
    p, q = rec.ctypes.data, out.ctypes.data
    assert L.sgz_truepeak_fold(None, 4, 1, 0, 4, 2, q) == E and L.sgz_truepeak_fold(p, 4, 1, 0, 4, 2, None) == E
    assert L.sgz_truepeak_fold(p, 4, 0, 0, 4, 2, q) == E               # channels == 0
    assert L.sgz_truepeak_fold(p, 4, 1, 2, 2, 2, q) == E               # x0 >= x1
    assert L.sgz_truepeak_fold(p, 4, 1, 0, 5, 2, q) == E               # x1 > n
    assert L.sgz_truepeak_fold(p, 4, 1, 0, 4, 0, q) == E               # out_columns == 0
    for field in ("count", "overs"):
        rec[:] = 0
        rec[field][:, 0] = 2**31                                       # two of them: 2^32
        assert L.sgz_truepeak_fold(p, 4, 1, 0, 4, 3, q) == E and b"2^32" in L.sgz_last_error()
        assert out.tobytes() == before
        assert L.sgz_truepeak_fold(p, 4, 1, 0, 4, 4, q) == api.SGZ_OK and out.tobytes() == rec.tobytes()
        out[:] = np.frombuffer(before, tr.DTYPE).reshape(out.shape)
        rec[field][:, 0] = (2**32 - 1) // 4                            # the largest that fits
        assert L.sgz_truepeak_fold(p, 4, 1, 0, 4, 1, q) == api.SGZ_OK and int(out[field][0, 0]) == 4 * ((2**32 - 1) // 4)
        out[:] = np.frombuffer(before, tr.DTYPE).reshape(out.shape)


def test_readout():
    """peak / 2^43 is exact (a power of two); dBTP goes through libm's log10 on both sides: the bar is 4 ulp of a value below 400 in
    magnitude, 2e-13 dB -- log10 is good to under 1 ulp and the factor 20 rounds once"""
    rng = np.random.default_rng(8)
    one = np.zeros((), tr.DTYPE)
    assert api.truepeak_readout(one) == (0.0, -math.inf)
    one["peak"] = 2**43
    assert api.truepeak_readout(one) == (1.0, 0.0)
    for peak in [1, 2**26 * 2073548, 2**47 - 1] + [int(v) for v in rng.integers(1, 2**47, size=200)]:
        one["peak"] = peak
        p, d = api.truepeak_readout(one)
        assert p == peak / 2.0**43 and abs(d - 20.0 * math.log10(peak / 2.0**43)) <= 2e-13, (peak, p, d)
    L = api.lib()
    assert L.sgz_truepeak_readout(None, None, None) == E
    assert L.sgz_truepeak_readout(one.ctypes.data if hasattr(one, "ctypes") else None, None, None) == api.SGZ_OK      # either result may be NULL


def test_refusals_before_the_device_is_touched():
    """every argument check of the stage call and of the stream's calls that needs no device: made on fake, never dereferenced addresses"""
    L = api.lib()
    good, carry, peaks = 0x10000, 0x20000, 0x30000
    call = L.sgz_stage_truepeak_columns
    #          planar stride ch  n   m  held flush cont slices carry peaks stream
    assert call(None, 128, 1, 100, 8, 0, 1, 0, 0, carry, peaks, None) == E                  # a null d_planar
    assert call(good, 128, 0, 100, 8, 0, 1, 0, 0, carry, peaks, None) == E                  # channels 0
    assert call(good, 128, 65, 100, 8, 0, 1, 0, 0, carry, peaks, None) == E                 # channels above 64
    assert call(good, 128, 1, 100, 0, 0, 1, 0, 0, carry, peaks, None) == E                  # m == 0
    assert call(good, 128, 1, 100, 8, 8, 1, 1, 0, carry, peaks, None) == E                  # held >= m
    assert call(good, 128, 1, 100, 8, 3, 1, 0, 0, carry, peaks, None) == E                  # held > 0 in a stream that begins here
    assert call(good, 99, 1, 100, 8, 0, 1, 0, 0, carry, peaks, None) == E                   # channel_stride < nsamples
    assert call(good, 128, 1, 100, 8, 0, 1, 0, 65, carry, peaks, None) == E                 # slices > 64
    assert call(good + 2, 128, 1, 100, 8, 0, 1, 0, 0, carry, peaks, None) == E              # d_planar not aligned to 4
    assert call(good, 128, 1, 100, 8, 3, 1, 1, 0, carry + 8, peaks, None) == E              # d_carry not aligned to 16
    assert call(good, 128, 1, 100, 8, 0, 1, 0, 0, carry, peaks + 8, None) == E              # nor d_peaks
    assert call(good, 128, 1, 100, 8, 0, 1, 0, 0, None, peaks, None) == E                   # the carry is written: samples arrive
    assert call(good, 128, 1, 0, 8, 0, 1, 1, 0, None, peaks, None) == E                     # the carry is read: continued
    assert call(good, 128, 1, 100, 8, 0, 1, 0, 0, carry, None, None) == E                   # columns close
    assert call(good, 128, 1, 0, 8, 3, 1, 1, 0, carry, None, None) == E                     # the flushed carry is a column
    assert b"sgz_stage_truepeak_columns" in L.sgz_last_error()
    assert call(good, 128, 1, 0, 8, 0, 1, 0, 0, None, None, None) == api.SGZ_OK             # nothing arrives, nothing is flushed: nothing launched
    assert call(good, 128, 1, 0, 8, 3, 0, 1, 0, carry, peaks, None) == api.SGZ_OK
    # the stream's calls on a null stream
    assert L.sgz_pcm_stream_set_truepeak(None, 8, None, 0) == E and L.sgz_pcm_stream_flush_truepeak(None) == E
    assert L.sgz_pcm_stream_truepeak_state(None, None, None) == E and L.sgz_pcm_stream_truepeak_for(None, 100, 0) == 0
    L.sgz_truepeak_columns_limits(None, None)                                               # either result may be NULL
    L.sgz_truepeak_taps(None)


def test_truepeak_kernels_need_no_scratch():
    import codeobj_report as cr
    lib = os.path.join(ROOT, "signalizer_amd", "libsgz.so")
    if not (os.path.exists(lib) and os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("library or llvm tools not present")
    rows = [r for r in cr.kernels(lib) if any(k in r["demangled"] for k in ("truePeakTileKernel", "truePeakSliceKernel", "truePeakEmitKernel"))]
    assert len(rows) == 3, [r["demangled"] for r in rows]
    bad = [(r["demangled"], r.get("vgpr_spill_count"), r.get("sgpr_spill_count"), r.get("private_segment_fixed_size")) for r in rows
           if r.get("vgpr_spill_count", 0) or r.get("sgpr_spill_count", 0) or r.get("private_segment_fixed_size", 0)]
    assert not bad, bad
