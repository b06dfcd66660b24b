"""The loudness lane's host helpers (csrc/loudness_columns.hip) against tests/loudness_ref.py, and the definition itself against known answers
and against the unsegmented fp64 recurrence.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness_ref as lr  # noqa: E402

E = api.SGZ_EINVAL
_cache = {}


def rate_filter(rate):
    if rate not in _cache:
        _cache[rate] = api.loudness_filter_for_rate(rate)
    return _cache[rate]


def tiny():
    return api.loudness_filter(lr.TINY.b, lr.TINY.a, lr.TINY.W, lr.TINY.L)


# ---- the filter of a rate and the tap table ---------------------------------------------------------------------------------------------------
def test_the_printed_table_at_48_kHz():
    f = rate_filter(48000)
    assert [list(r) for r in f.b] == [[1.53512485958697, -2.69169618940638, 1.19839281085285], [1.0, -2.0, 1.0]]
    assert [list(r) for r in f.a] == [[-1.69065929318241, 0.73248077421585], [-1.99004745483398, 0.99007225036621]]
    assert (f.W, f.L) == (4096, 256)


@pytest.mark.parametrize("rate, W", [(8000, 1024), (44100, 4096), (48000, 4096), (96000, 8192), (192000, 16384)])
def test_the_filter_of_a_rate(rate, W):
    f = rate_filter(rate)
    assert (f.W, f.L) == (W, W // 16)
    # the re-derivation lands on the printed table at 48 kHz to the table's own digits, and every rate's high-pass has b = 1, -2, 1
    assert list(f.b[1]) == [1.0, -2.0, 1.0]
    if rate != 48000:
        # an independent derivation: the same prototype through the bilinear transform, in numpy
        K = np.tan(np.pi * 1681.974450955533 / rate)
        Vh = 10.0 ** (3.999843853973347 / 20.0)
        Vb = Vh ** 0.4996667741545416
        Q = 0.7071752369554196
        a0 = 1.0 + K / Q + K * K
        want = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
        np.testing.assert_allclose(list(f.b[0]) + list(f.a[0]), want, rtol=1e-13)
        K, Q = np.tan(np.pi * 38.13547087602444 / rate), 0.5003270373238773
        a0 = 1.0 + K / Q + K * K
        np.testing.assert_allclose(list(f.a[1]), [2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], rtol=1e-13)


def test_the_rederivation_meets_the_printed_table():
    """at 48000 the helper returns literals; the formulas give them back to the digits printed"""
    g = api.loudness_filter_for_rate(48000.0 * (1 + 2.0 ** -40))
    p = rate_filter(48000)
    np.testing.assert_allclose([list(r) for r in g.b], [list(r) for r in p.b], atol=2e-11)
    np.testing.assert_allclose([list(r) for r in g.a], [list(r) for r in p.a], atol=2e-11)


@pytest.mark.parametrize("which", ["tiny", 8000, 48000])
def test_the_tap_table_entry_for_entry(which):
    f = tiny() if which == "tiny" else rate_filter(which)
    st, got = api.loudness_taps(f)
    want = lr.taps(f)
    assert st == api.SGZ_OK and want is not None
    assert got.shape == want.shape and np.array_equal(got.astype(np.int64), want)
    bound = int(np.abs(want).sum(axis=1).max()) << 26
    assert bound < 1 << 62
    if which == 8000:                                           # the figures the definition was checked with
        assert abs(np.log2(float(np.abs(want).max())) - 30.44) < 0.01 and abs(np.log2(float(bound)) - 58.35) < 0.01


def _refused(f):
    taps = np.full((4, 70000), 0x5A5A5A5A, np.int32)
    st = api.lib().sgz_loudness_taps(C.byref(f), taps.ctypes.data_as(C.c_void_p))
    assert st in (E, api.SGZ_OK) and (lr.taps(f) is None) == (st == E)
    assert st == api.SGZ_OK or (taps == 0x5A5A5A5A).all(), "a refusal wrote the table"
    return st == E


def test_refused_filters():
    b, a = lr.TINY.b, lr.TINY.a
    assert not _refused(tiny())
    for W, L in ((96, 16), (64, 24), (64, 8), (64, 128), (131072, 16), (0, 0), (64, 0)):
        assert _refused(api.loudness_filter(b, a, W, L)), (W, L)
    # a tap outside int32: s1 after the first step is b01 - a00 b00 = 0.6 -> 0.6 * 2^32
    assert _refused(api.loudness_filter([[0.0, 0.6, 0.0], [1.0, 0.0, 0.0]], [[0.0, 0.0], [0.0, 0.0]], 64, 16))
    # every tap inside int32, the sum of their magnitudes is not: a pole at 0.999 keeps s1 near 0.4 for a thousand steps
    slow = api.loudness_filter([[0.0, 0.4, 0.0], [1.0, 0.0, 0.0]], [[-0.999, 0.0], [0.0, 0.0]], 1024, 64)
    t = lr.taps(lr.Filter(slow.b, slow.a, 16, 16))
    assert t is not None and int(np.abs(t).max()) < 2 ** 31         # (the first 16 taps alone are accepted)
    assert _refused(slow)
    assert _refused(api.loudness_filter([[np.nan, 0.0, 0.0], [1.0, 0.0, 0.0]], [[0.0, 0.0], [0.0, 0.0]], 64, 16))
    assert api.lib().sgz_loudness_taps(None, None) == E
    assert api.lib().sgz_loudness_filter_for_rate(100.0, C.byref(api.LoudnessFilter())) == E
    assert api.lib().sgz_loudness_filter_for_rate(48000.0, None) == E


# ---- fold, readout, integrated ---------------------------------------------------------------------------------------------------------------
def random_records(n, channels, seed, big=False):
    rng = np.random.default_rng(seed)
    r = np.zeros((n, channels), lr.DTYPE)
    r["sumsq"][..., 0] = rng.integers(0, 2 ** 64, size=(n, channels), dtype=np.uint64)
    r["sumsq"][..., 1] = rng.integers(0, 2 ** 20 if big else 4, size=(n, channels), dtype=np.uint64)
    r["count"] = rng.integers(1, 5000, size=(n, channels))
    return r


def test_fold_equals_the_sums():
    r = random_records(37, 3, 1, big=True)
    for x0, x1 in ((0, 37), (3, 30), (36, 37)):
        for cols in (1, 2, 5, 36, 37, 100):
            got = api.loudness_fold(r, cols, x0, x1)
            want = lr.fold(r, lr.view_bounds(x0, x1, cols))
            assert got.tobytes() == want.tobytes(), (x0, x1, cols)
    # nested boundaries: a fold of a fold is the fold
    r = random_records(32, 2, 2, big=True)
    assert api.loudness_fold(api.loudness_fold(r, 8), 4).tobytes() == api.loudness_fold(r, 4).tobytes() == lr.fold(r, [0, 8, 16, 24, 32]).tobytes()
    # the low words carry into the high ones
    r = np.zeros((2, 1), lr.DTYPE)
    r["sumsq"][:, 0, 0] = 2 ** 64 - 1
    got = api.loudness_fold(r, 1)
    assert (int(got["sumsq"][0, 0, 0]), int(got["sumsq"][0, 0, 1])) == (2 ** 64 - 2, 1)


def test_fold_refusals_write_nothing():
    r = random_records(4, 1, 3)
    r["count"] = 2 ** 31
    out = np.full((4, 1), 0x5A, np.uint8).repeat(32, axis=1).view(lr.DTYPE)
    before = out.tobytes()
    call = api.lib().sgz_loudness_fold
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                # noqa: E731
    assert call(ptr(r), 4, 1, 0, 4, 2, ptr(out)) == E            # 2^32 samples in a folded column
    assert call(ptr(r), 4, 1, 0, 4, 4, ptr(out)) == api.SGZ_OK   # one column each: fine
    out[:] = np.frombuffer(before, lr.DTYPE).reshape(out.shape)
    assert call(None, 4, 1, 0, 4, 2, ptr(out)) == E and call(ptr(r), 4, 0, 0, 4, 2, ptr(out)) == E
    assert call(ptr(r), 4, 1, 3, 3, 2, ptr(out)) == E and call(ptr(r), 4, 1, 0, 5, 2, ptr(out)) == E and call(ptr(r), 4, 1, 0, 4, 0, ptr(out)) == E
    assert out.tobytes() == before


def test_readout_and_integrated_against_numpy():
    for seed, channels, weights in ((1, 1, None), (2, 2, None), (3, 5, [1.0, 1.0, 1.0, 1.41, 1.41])):
        r = random_records(50, channels, seed)
        for a, n in ((0, 1), (3, 4), (10, 30), (0, 50)):
            l, z = api.loudness_readout(r[a:a + n], weights)
            want = lr.mean_square(r[a:a + n], weights)
            assert abs(z - want) <= 1e-13 * want and abs(l - lr.lufs(want)) < 1e-10
        assert abs(api.loudness_integrated(r, weights) - lr.integrated(r, weights)) < 1e-10
    # records of very different levels: both gates cut
    r = random_records(60, 2, 4)
    r["sumsq"][:20, :, 1] = 0
    r["sumsq"][:20, :, 0] = 1000                                 # far below -70
    r["sumsq"][20:30, :, 1] = 0
    r["sumsq"][20:30, :, 0] = 2 ** 62                            # 12 dB and more below the rest
    want = lr.integrated(r)
    assert np.isfinite(want) and abs(api.loudness_integrated(r) - want) < 1e-10
    assert want > lr.lufs(np.mean([lr.mean_square(r[i:i + 4]) for i in range(57)])) + 1.0      # (the gates moved it)
    # nothing to read
    z = np.zeros((10, 2), lr.DTYPE)
    assert api.loudness_readout(z) == (-np.inf, 0.0) and api.loudness_integrated(z) == -np.inf and api.loudness_integrated(r[:3]) == -np.inf
    z["count"] = 4800
    assert api.loudness_readout(z)[0] == -np.inf and api.loudness_integrated(z) == -np.inf
    assert api.lib().sgz_loudness_readout(None, 1, 1, None, None, None) == E
    assert api.lib().sgz_loudness_readout(z.ctypes.data_as(C.c_void_p), 0, 2, None, None, None) == E
    assert api.lib().sgz_loudness_integrated(z.ctypes.data_as(C.c_void_p), 10, 2, None, None) == E


# ---- known answers, through the reference's records and the C helpers ---------------------------------------------------------------------
RATE, M = 48000, 4800            # 100 ms columns
TOL = 0.1                        # LU: the meters' own tolerance in EBU Tech 3341


def sine_records(freq, segments, channels):
    """records [columns][channels] of a sine at `freq` whose level follows `segments` = [(seconds, dBFS), ..]; every channel the same"""
    amp = np.concatenate([np.full(int(round(s * RATE)), 10.0 ** (db / 20.0)) for s, db in segments])
    x = (amp * np.sin(2.0 * np.pi * freq * np.arange(len(amp)) / RATE)).astype(np.float32)
    one, _ = lr.records_of(x[None, :], rate_filter(RATE), M)
    return np.repeat(one, channels, axis=1)


def test_a_full_scale_997_Hz_sine_reads_minus_3_01():
    r = sine_records(997.0, [(2.0, 0.0)], 1)
    assert abs(api.loudness_readout(r[10:14])[0] - (-3.01)) < TOL           # BS.1770's own calibration
    assert abs(api.loudness_readout(r[10:14])[0] - (-3.01)) < 0.02          # (and in fact much closer)


def test_a_stereo_1_kHz_sine_at_minus_23():
    r = sine_records(1000.0, [(20.0, -23.0)], 2)
    assert r.shape == (200, 2)
    assert abs(api.loudness_readout(r[100:104])[0] + 23.0) < TOL            # momentary
    assert abs(api.loudness_readout(r[100:130])[0] + 23.0) < TOL            # short-term
    assert abs(api.loudness_integrated(r) + 23.0) < TOL


def test_the_gates_drop_the_quiet_ends():
    r = sine_records(1000.0, [(10.0, -36.0), (60.0, -23.0), (10.0, -36.0)], 2)
    assert abs(api.loudness_integrated(r) + 23.0) < TOL
    assert api.loudness_readout(r)[0] < -23.4                               # (ungated, the ends pull it down)


# ---- the segmentation against the unsegmented recurrence --------------------------------------------------------------------------------------
# Measured on the first run (this signal, this seed): the largest difference of a 100 ms block's energy between the definition and the plain
# fp64 recurrence is MEASURED_DB[rate] dB.  The bound is ten times that: room for another seed, not for another algorithm.
MEASURED_DB = {8000: 9.219e-07, 48000: 8.673e-06}
MEASURED_Z = {8000: 2.740e-08, 48000: 1.398e-07}         # the largest difference in z, as a fraction of full scale


def segmentation_error(rate, seconds=3.0, seed=7):
    f = rate_filter(rate)
    n = int(rate * seconds)
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    x = 0.5 * np.sin(2.0 * np.pi * 440.0 * t) + 0.1 * rng.standard_normal(n) + 0.2
    x[n // 3:2 * n // 3] *= 1e-3                                            # a -60 dB stretch in the middle
    v, _ = lr.quantise(x.astype(np.float32))
    z = lr.q_of(v, f, want_z=True)
    u = lr.unsegmented_z(v, f)
    block = rate // 10
    blocks = n // block
    ez = (z[:blocks * block] ** 2).reshape(blocks, block).sum(axis=1)
    eu = (u[:blocks * block] ** 2).reshape(blocks, block).sum(axis=1)
    return float(np.abs(10.0 * np.log10(ez / eu)).max()), float(np.abs(z - u).max() / 2.0 ** 23)


@pytest.mark.parametrize("rate", [8000, 48000])
def test_the_segmented_definition_stays_at_the_recurrence(rate):
    db, dz = segmentation_error(rate)
    print(f"loudness segmentation at {rate} Hz: block energy differs by at most {db:.3e} dB, z by {dz:.3e} of full scale")
    assert db < 10.0 * MEASURED_DB[rate] and dz < 10.0 * MEASURED_Z[rate]


# ---- the exports, the header, the refusals made before the device is touched, the code objects -------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sgz_stage_loudness_columns", "sgz_loudness_columns_limits", "sgz_loudness_filter_for_rate", "sgz_loudness_taps", "sgz_loudness_fold",
         "sgz_loudness_readout", "sgz_loudness_integrated", "sgz_pcm_stream_set_loudness", "sgz_pcm_stream_loudness_for",
         "sgz_pcm_stream_loudness_state", "sgz_pcm_stream_flush_loudness"]


def test_exports_and_the_header():
    import re
    L = api.lib()
    assert [n for n in NAMES if not hasattr(L, n)] == [] and [n for n in NAMES if n not in api.EXPORTS] == []
    assert L.sgz_abi_version() == 5 and api.LOUDNESS_DTYPE == lr.DTYPE and C.sizeof(api.LoudnessFilter) == 88
    text = open(os.path.join(ROOT, "include", "sgz.h")).read()
    assert re.search(r"#define\s+SGZ_ABI_VERSION\s+5\b", text)
    history = text[:text.index("#define SGZ_ABI_VERSION")]
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text) and n in history, n
    lane = text[text.index("/* The loudness lane"):]
    assert "exact, no tolerance" in lane[:1200] and text.index("/* The true-peak lane") < text.index("/* The loudness lane")
    for line in ("y = b00*x + s1;   s1 = (b01*x - a00*y) + s2;   s2 = b02*x - a01*y;", "z = b10*y + t1;   t1 = (b11*y - a10*z) + t2;   t2 = b12*y - a11*z;"):
        assert line in lane


def test_refusals_before_the_device_is_touched():
    """every argument check of the stage call and of the stream's calls that needs no device: made on fake, never dereferenced addresses"""
    L = api.lib()
    good, carry, out = 0x10000, 0x20000, 0x30000
    f = C.byref(tiny())
    call = L.sgz_stage_loudness_columns
    #          planar stride ch  n  f first m held flush cont slices carry out stream
    assert call(None, 128, 1, 100, f, 0, 8, 0, 1, 0, 0, carry, out, None) == E                  # a null d_planar
    assert call(good, 128, 1, 100, None, 0, 8, 0, 1, 0, 0, carry, out, None) == E               # a null filter
    assert call(good, 128, 1, 100, C.byref(api.loudness_filter(lr.TINY.b, lr.TINY.a, 64, 48)), 0, 8, 0, 1, 0, 0, carry, out, None) == E
    assert call(good, 128, 1, 100, C.byref(api.loudness_filter(lr.TINY.b, lr.TINY.a, 32768, 64)), 0, 8, 0, 1, 0, 0, carry, out, None) == E
    assert call(good, 128, 0, 100, f, 0, 8, 0, 1, 0, 0, carry, out, None) == E                  # channels 0
    assert call(good, 128, 65, 100, f, 0, 8, 0, 1, 0, 0, carry, out, None) == E                 # channels above 64
    assert call(good, 128, 1, 100, f, 0, 0, 0, 1, 0, 0, carry, out, None) == E                  # m == 0
    assert call(good, 128, 1, 100, f, 0, 8, 8, 1, 1, 0, carry, out, None) == E                  # held >= m
    assert call(good, 128, 1, 100, f, 0, 8, 3, 1, 0, 0, carry, out, None) == E                  # held > 0 in a stream that begins here
    assert call(good, 99, 1, 100, f, 0, 8, 0, 1, 0, 0, carry, out, None) == E                   # channel_stride < nsamples
    assert call(good, 128, 1, 100, f, 2 ** 63, 8, 0, 1, 0, 0, carry, out, None) == E            # first_index above 2^62
    assert call(good, 128, 1, 100, f, 0, 8, 0, 1, 0, 65, carry, out, None) == E                 # slices > 64
    assert call(good + 2, 128, 1, 100, f, 0, 8, 0, 1, 0, 0, carry, out, None) == E              # d_planar not aligned to 4
    assert call(good, 128, 1, 100, f, 0, 8, 3, 1, 1, 0, carry + 8, out, None) == E              # d_carry not aligned to 16
    assert call(good, 128, 1, 100, f, 0, 8, 0, 1, 0, 0, carry, out + 8, None) == E              # nor d_records
    assert call(good, 128, 1, 100, f, 0, 8, 0, 1, 0, 0, None, out, None) == E                   # the carry is written: samples arrive
    assert call(good, 128, 1, 0, f, 0, 8, 0, 1, 1, 0, None, out, None) == E                     # the carry is read: continued
    assert call(good, 128, 1, 100, f, 0, 8, 0, 1, 0, 0, carry, None, None) == E                 # columns close
    assert call(good, 128, 1, 0, f, 0, 8, 3, 1, 1, 0, carry, None, None) == E                   # the flushed carry is a column
    assert b"sgz_stage_loudness_columns" in L.sgz_last_error()
    assert call(good, 128, 1, 0, f, 0, 8, 0, 1, 0, 0, None, None, None) == api.SGZ_OK           # nothing arrives, nothing is flushed: nothing launched
    assert call(good, 128, 1, 0, f, 0, 8, 3, 0, 1, 0, carry, out, None) == api.SGZ_OK
    assert L.sgz_pcm_stream_set_loudness(None, f, 8, None, 0) == E and L.sgz_pcm_stream_flush_loudness(None) == E
    assert L.sgz_pcm_stream_loudness_state(None, None, None) == E and L.sgz_pcm_stream_loudness_for(None, 100, 0) == 0
    assert L.sgz_loudness_columns_limits(f, 2, None, None, None) == api.SGZ_OK                  # any result may be NULL


def test_loudness_kernels_need_no_scratch_and_do_not_contract():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_report as cr
    lib = os.path.join(ROOT, "signalizer_amd", "libsgz.so")
    if not (os.path.exists(lib) and os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("library or llvm tools not present")
    # (the history and sum kernels are column_lanes.hpp's templates, instantiated on this lane's kernel arguments)
    mine = "<(anonymous namespace)::LoudnessParams"
    names = ("loudnessRunKernel", "historyKernel" + mine, "sumTileKernel" + mine, "sumSliceKernel" + mine, "sumEmitKernel" + mine)
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
        if b"loudnessRunKernel" not in elf:
            continue
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(elf)
            f.flush()
            text = subprocess.run([objdump, "-d", f.name], check=True, capture_output=True, text=True).stdout
        body = text[text.index("loudnessRunKernel"):]
        body = body[:body.index("\n\n")] if "\n\n" in body else body
        assert "v_mul_f64" in body and "v_add_f64" in body and "v_mad_i64_i32" in body and "v_fma_f64" not in body
        found += 1
    assert found == 1
