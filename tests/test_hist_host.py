"""The histogram lane (sgz.h, "The histogram lane"): what needs no GPU -- the exports, the header, the bucket edges, tests/hist_ref.py against
brute-force Python loops, the fold of finer records into coarser ones (sgz_hist_fold), the percentile (sgz_hist_percentile), the readout
(sgz_hist_readout), the refusals made before the device is touched, and the new kernels' code objects.  Records are compared as bytes."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

from signalizer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hist_ref as hr  # noqa: E402

NAMES = ["sgz_stage_hist_columns", "sgz_hist_columns_limits", "sgz_hist_edges", "sgz_hist_fold", "sgz_hist_percentile", "sgz_hist_readout",
         "sgz_pcm_stream_set_hist", "sgz_pcm_stream_hist_for", "sgz_pcm_stream_hist_state", "sgz_pcm_stream_flush_hist"]
E = api.SGZ_EINVAL


def _same(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a, hr.DTYPE).tobytes() == np.ascontiguousarray(b, hr.DTYPE).tobytes()


def _header():
    return open(os.path.join(ROOT, "include", "sgz.h")).read()


def _error():
    return api.lib().sgz_last_error().decode()


def test_exports_exist():
    L = api.lib()
    assert [n for n in NAMES if not hasattr(L, n)] == []
    assert [n for n in NAMES if n not in api.EXPORTS] == []
    assert L.sgz_abi_version() == 5
    assert api.HIST_DTYPE == hr.DTYPE and api.HIST_DTYPE.itemsize == 448 and api.HIST_BUCKETS == hr.BUCKETS == 106
    for name in ("HistReading", "stage_hist_columns", "hist_columns_limits", "hist_edges", "hist_fold", "hist_percentile", "hist_readout"):
        assert hasattr(api, name), name
    for name in ("set_hist", "hist_for", "hist_state", "flush_hist"):
        assert hasattr(api.PcmStream, name), name


def test_header_names_them_and_keeps_version_5():
    text = _header()
    assert re.search(r"#define\s+SGZ_ABI_VERSION\s+5\b", text) and re.search(r"#define\s+SGZ_HIST_BUCKETS\s+106\b", text)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n                    # declared
    history = text[:text.index("#define SGZ_ABI_VERSION")]
    assert "(5, later: the histogram lane -- " in history
    assert [n for n in NAMES + ["sgz_hist_record", "sgz_hist_reading", "SGZ_HIST_BUCKETS"] if n not in history] == []
    lane = text[text.index("/* The histogram lane"):]
    assert "has no" in lane[:900] and "sgz_hist_record" in lane and "448 bytes" in lane
    assert text.index("/* The band lane") < text.index("/* The histogram lane") < text.index("/* The track lane")
    struct = lane[lane.index("typedef struct sgz_hist_record"):lane.index("} sgz_hist_record;")]
    fields = re.findall(r"uint32_t\s+(\w+)", struct)
    assert fields == ["bucket", "count", "skipped", "negative", "peak", "bits_or", "bits_and"] and "bucket[SGZ_HIST_BUCKETS]" in struct


def test_limits_are_the_documented_ones():
    switch, tile = api.hist_columns_limits()
    assert 1 <= switch <= tile and tile % 4 == 0, (switch, tile)
    lane = _header()
    lane = lane[lane.index("/* The histogram lane"):]
    assert f"({switch};" in lane and f"{tile} / m" in lane
    api.lib().sgz_hist_columns_limits(None, None)                      # either result may be NULL


def test_edges_against_the_closed_form():
    lo, hi = api.hist_edges()
    rlo, rhi = hr.edges()
    assert np.array_equal(lo.astype(np.int64), rlo) and np.array_equal(hi.astype(np.int64), rhi)
    assert (int(lo[0]), int(hi[0])) == (0, 0)
    assert [b for b in range(106) if lo[b] > hi[b]] == [2, 3, 4, 6, 8] == list(hr.EMPTY)
    nxt = 1                                                             # the reachable buckets tile 1 .. 2^26 without gaps, in order
    for b in hr.reachable()[1:]:
        assert int(lo[b]) == nxt and int(hi[b]) >= int(lo[b]), b
        nxt = int(hi[b]) + 1
    assert nxt == 2**26 + 1
    assert int(lo[93]) == 2**23 and (int(lo[105]), int(hi[105])) == (2**26, 2**26)
    # an octave in four linear parts, 1.2 to 1.9 dB wide (from the third octave on, where the parts hold integers of their own)
    for b in range(13, 105):
        width = 20 * math.log10((int(hi[b]) + 1) / int(lo[b]))
        assert 1.15 <= width <= 1.95, (b, width)
    api.lib().sgz_hist_edges(None, None)                               # either array may be NULL


def test_bucket_of_against_a_brute_force_loop():
    lo, hi = hr.edges()
    probe = set(range(1 << 16))
    for b in hr.reachable():
        for a in (int(lo[b]), int(hi[b])):
            probe |= {a - 1, a, a + 1}
    probe = sorted(a for a in probe if 0 <= a <= 2**26)
    got = hr.bucket_of(np.array(probe, np.int64))
    by_edges = np.searchsorted(np.array([int(hi[b]) for b in hr.reachable()]), np.array(probe))      # the first reachable bucket with hi >= a
    reach = np.array(hr.reachable())
    for a, g, r in zip(probe, got.tolist(), reach[by_edges].tolist()):
        assert g == hr.bucket_of_int(a) == r, (a, g, r)
        assert int(lo[g]) <= a <= int(hi[g]), a
    # the float form the kernel must not take: it misfiles all 8 of the 8 upper edges above 2^24
    wrong = 0
    for b in range(97, 105):
        a = int(hi[b])
        assert a > 2**24
        f = int(np.float32(a))                                          # rounds to the next bucket's lower edge
        wrong += hr.bucket_of_int(f) != b
    assert wrong == 8


def _loop_columns(x, m, flush):
    """the definition sample by sample in Python integers"""
    channels, S = x.shape
    ncols = S // m + (1 if S % m and flush else 0)
    out = np.zeros((ncols, channels), hr.DTYPE)
    for d in range(channels):
        for c in range(ncols):
            r = {k: 0 for k in ("count", "skipped", "negative", "peak", "bits_or")}
            r["bits_and"] = 0xFFFFFFFF
            buckets = [0] * 106
            for i in range(c * m, min((c + 1) * m, S)):
                f = float(x[d, i])
                if math.isnan(f):
                    r["skipped"] += 1
                    continue
                y = f * 2.0**23
                v = int(min(max(np.rint(y) if math.isfinite(y) else math.copysign(2.0**26, y), -(2.0**26)), 2.0**26))
                a = abs(v)
                buckets[hr.bucket_of_int(a)] += 1
                r["count"] += 1
                r["negative"] += v < 0
                r["peak"] = max(r["peak"], a)
                r["bits_or"] |= v & 0xFFFFFFFF
                r["bits_and"] &= v & 0xFFFFFFFF
            out[c, d]["bucket"] = buckets
            for k, val in r.items():
                out[c, d][k] = val
    return out


def test_columns_against_a_per_sample_loop():
    x = np.stack([hr.corners(700), hr.edge_values(700), hr.silence(700), hr.s16(700)])
    for m, flush in ((1, True), (7, True), (7, False), (64, True), (699, False), (700, True), (1000, True)):
        got, open_ = hr.columns(x, m, flush=flush)
        assert _same(got, _loop_columns(x, m, flush)), (m, flush)
        assert (open_ is None) == (flush or 700 % m == 0)
        assert (got["bucket"].sum(axis=-1) == got["count"]).all()
    # a call behind held samples equals the whole
    whole, _ = hr.columns(x, 64)
    for held in (1, 63):
        _, carry = hr.columns(x[:, :held], 64, flush=False)
        got, none = hr.columns(x[:, held:], 64, held=held, carry=carry)
        assert none is None and _same(got, whole)
    # a column of NaNs alone is the identity with `skipped`
    rec = hr.columns(np.full((1, 5), np.nan, np.float32), 5)[0][0, 0]
    want = hr.identity()
    want["skipped"] = 5
    assert rec.tobytes() == want.tobytes() and int(want["bits_and"]) == 0xFFFFFFFF


def test_a_coarser_column_is_the_fold_of_the_finer_ones():
    rng = np.random.default_rng(5)
    for trial in range(10):
        S = int(rng.integers(1, 400))
        m = int(rng.integers(1, 9))
        r = int(rng.integers(2, 6))
        x = np.stack([hr.noise(S, seed=trial), hr.noise(S, seed=100 + trial) * np.float32(200.0)])         # the second channel clips
        x[rng.integers(0, 2), rng.integers(0, S)] = np.nan
        x[:, rng.integers(0, S)] = 0.0
        fine, _ = hr.columns(x, m)
        coarse, _ = hr.columns(x, m * r)
        n = fine.shape[0]
        bounds = list(range(0, n, r)) + [n]
        assert _same(hr.fold(fine, bounds), coarse), (trial, S, m, r)
        if n % r == 0:                                                  # the library's fold where its boundary rule gives these boundaries
            assert hr.view_bounds(0, n, n // r) == bounds
            assert _same(api.hist_fold(fine, n // r), coarse), (trial, S, m, r)


def test_hist_fold_against_brute_force_boundaries():
    rng = np.random.default_rng(6)
    x = np.stack([hr.corners(24 * 40), hr.s16(24 * 40)])
    x[0, 80:120] = np.nan                                               # a column of NaNs alone: bits_and of an empty column is all ones
    records, _ = hr.columns(x, 40)                                      # 24 columns, two channels
    assert records.shape == (24, 2) and int(records[2, 0]["bits_and"]) == 0xFFFFFFFF and int(records[2, 0]["count"]) == 0
    for n in (1, 2, 3, 7, 16, 24):
        for out_columns in sorted({1, 2, 3, n // 2 + 1, n, n + 5}):
            x0 = int(rng.integers(0, n))
            x1 = int(rng.integers(x0 + 1, n + 1))
            for a, b in ((0, n), (x0, x1)):
                w, cols = b - a, min(out_columns, b - a)
                bounds = [a + (k * w + cols - 1) // cols for k in range(cols + 1)]
                assert bounds == hr.view_bounds(a, b, out_columns) and bounds[0] == a and bounds[-1] == b
                assert _same(api.hist_fold(records[:n], out_columns, a, b), hr.fold(records[:n], bounds)), (n, out_columns, a, b)
    # the identity folds to itself and changes nothing it is folded with
    ident = np.array([[hr.identity()], [hr.identity()]], hr.DTYPE).reshape(2, 1)
    assert _same(api.hist_fold(ident, 1), ident[:1])
    pair = np.array([records[5, 1], hr.identity()], hr.DTYPE).reshape(2, 1)
    assert _same(api.hist_fold(pair, 1), pair[:1])
    # the folds by hand: or, and, max
    two = np.zeros((2, 1), hr.DTYPE)
    two["bits_or"][:, 0], two["bits_and"][:, 0], two["peak"][:, 0] = (0x0F00, 0x00F1), (0xFF00, 0x0FF0), (7, 5)
    got = api.hist_fold(two, 1)[0, 0]
    assert (int(got["bits_or"]), int(got["bits_and"]), int(got["peak"])) == (0x0FF1, 0x0F00, 7)


def test_hist_fold_refusals_write_nothing():
    L = api.lib()
    rec = np.zeros((4, 1), hr.DTYPE)
    out = np.full((4, 448), 0xAB, np.uint8).view(hr.DTYPE)
    before = out.tobytes()
    p, q = rec.ctypes.data, out.ctypes.data
    assert L.sgz_hist_fold(None, 4, 1, 0, 4, 2, q) == E and _error() == "sgz_hist_fold: null argument"
    assert L.sgz_hist_fold(p, 4, 1, 0, 4, 2, None) == E
    assert L.sgz_hist_fold(p, 4, 0, 0, 4, 2, q) == E and _error() == "sgz_hist_fold: channels >= 1"
    assert L.sgz_hist_fold(p, 4, 1, 2, 2, 2, q) == E                   # x0 >= x1
    assert L.sgz_hist_fold(p, 4, 1, 0, 5, 2, q) == E                   # x1 > n
    assert L.sgz_hist_fold(p, 4, 1, 0, 4, 0, q) == E                   # out_columns == 0
    for field in ("count", "skipped"):
        rec[:] = np.zeros((), hr.DTYPE)
        rec[field][:, 0] = 2**31                                        # two of them: 2^32
        assert L.sgz_hist_fold(p, 4, 1, 0, 4, 3, q) == E, field
        assert _error() == "sgz_hist_fold: a folded column counts more than 2^32 - 1 samples"
        assert out.tobytes() == before
        assert L.sgz_hist_fold(p, 4, 1, 0, 4, 4, q) == api.SGZ_OK      # one to one: nothing folds but the identity
        assert np.array_equal(out[field], rec[field])
        out[:] = np.frombuffer(before, hr.DTYPE).reshape(out.shape)
    rec[:] = np.zeros((), hr.DTYPE)
    rec["count"][:, 0] = (2**32 - 1) // 4                               # the largest that fits
    rec["bucket"][:, 0, 50] = (2**32 - 1) // 4
    assert L.sgz_hist_fold(p, 4, 1, 0, 4, 1, q) == api.SGZ_OK and int(out["count"].reshape(-1)[0]) == 4 * ((2**32 - 1) // 4)
    assert int(out["bucket"].reshape(-1, 106)[0, 50]) == 4 * ((2**32 - 1) // 4)


def _record(buckets, **fields):
    r = hr.identity()
    for b, n in buckets.items():
        r["bucket"][b] = n
    r["count"] = sum(buckets.values())
    for k, v in fields.items():
        r[k] = v
    return r


def test_percentile():
    lo, hi = hr.edges()
    rec = _record({0: 10, 50: 30, 93: 59, 105: 1})                      # 100 samples
    for q, bucket in ((0.0, 0), (0.1, 0), (0.1 + 2.0**-50, 50), (0.4, 50), (0.4 + 2.0**-50, 93), (0.5, 93), (0.99, 93), (0.99 + 2.0**-50, 105), (1.0, 105)):
        got = api.hist_percentile(rec, q)
        assert got == hr.percentile(rec, q) and got[0] == bucket, (q, got)
        assert got[1] == int(lo[bucket]) / 2.0**23 and got[2] == int(hi[bucket]) / 2.0**23
    assert api.hist_percentile(rec, 0.5)[1] == 1.0 and api.hist_percentile(rec, 1.0)[1:] == (8.0, 8.0)
    assert api.hist_percentile(rec, 0.0)[1:] == (0.0, 0.0)             # bucket 0 gives 0, 0
    one = _record({41: 7})                                              # a single-bucket record: every q
    for q in (0.0, 1e-300, 0.5, 1.0):
        assert api.hist_percentile(one, q)[0] == 41
    rng = np.random.default_rng(3)
    for trial in range(20):
        x = hr.noise(int(rng.integers(1, 3000)), seed=trial) * np.float32(10.0 ** rng.uniform(-4, 1.5))
        r = hr.columns(x[None, :], x.size)[0][0, 0]
        for q in (0.0, 0.1, 0.5, 0.95, 1.0, float(rng.uniform(0, 1)), int(rng.integers(0, x.size + 1)) / x.size):
            assert api.hist_percentile(r, q) == hr.percentile(r, q), (trial, q)
    # the refusals
    L = api.lib()
    b, l, h = C.c_uint32(77), C.c_double(-1), C.c_double(-1)
    p = np.ascontiguousarray(rec, hr.DTYPE).reshape(1)
    ok = (p.ctypes.data, 0.5, C.byref(b), C.byref(l), C.byref(h))
    for i in (0, 2, 3, 4):
        args = list(ok)
        args[i] = None
        assert L.sgz_hist_percentile(*args) == E and _error() == "sgz_hist_percentile: null argument"
    for q in (-1e-9, 1.0 + 1e-9, math.nan, math.inf):
        assert L.sgz_hist_percentile(p.ctypes.data, q, C.byref(b), C.byref(l), C.byref(h)) == E and _error() == "sgz_hist_percentile: 0 <= q <= 1"
    empty = np.ascontiguousarray(hr.identity(), hr.DTYPE).reshape(1)
    assert L.sgz_hist_percentile(empty.ctypes.data, 0.5, C.byref(b), C.byref(l), C.byref(h)) == E
    assert _error() == "sgz_hist_percentile: a record without samples has no percentile"
    assert (b.value, l.value, h.value) == (77, -1.0, -1.0)              # nothing was written


def _close(a, b):
    """1e-12 relative, or the same NaN / infinity: a quotient and one log10 of fp64 values"""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= 1e-12 * max(1.0, abs(a), abs(b))


def test_readout_against_numpy():
    rng = np.random.default_rng(8)
    recs = []
    for trial in range(20):
        S = int(rng.integers(1, 3000))
        x = hr.noise(S, seed=trial) * np.float32(10.0 ** rng.uniform(-5, 2))
        if trial % 5 == 0:
            x[: S // 2] = 0.0
        recs.append(hr.columns(x[None, :], S)[0][0, 0])
    recs.append(hr.columns(hr.silence(100)[None, :], 100)[0][0, 0])
    recs.append(hr.identity())
    for rec in recs:
        want, got = hr.readout(rec), api.hist_readout(rec)
        for name in ("zero_share", "negative_share", "peak", "peak_db", "median_db"):
            assert _close(got[name], want[name]), (name, got, want)
        assert got["toggling"] == want["toggling"] and got["effective_bits"] == want["effective_bits"]
    # a 16-bit signal reads 16 bits
    r16 = hr.columns(hr.s16(4000)[None, :], 4000)[0][0, 0]
    assert api.hist_readout(r16)["effective_bits"] == 16 and int(r16["bits_or"]) & 0xFF == 0
    r24 = hr.columns((np.arange(-500, 500) * 2.0**-23).astype(np.float32)[None, :], 1000)[0][0, 0]
    assert api.hist_readout(r24)["effective_bits"] == 24
    # a stuck bit shows in `toggling`: bit 9 always set, every other bit of the low 16 takes both values
    v = (np.random.default_rng(1).integers(0, 1 << 16, 5000) | (1 << 9)).astype(np.float64) * 2.0**-23
    stuck = api.hist_readout(hr.columns(v.astype(np.float32)[None, :], 5000)[0][0, 0])
    assert stuck["toggling"] == 0xFFFF & ~(1 << 9) and stuck["negative_share"] == 0.0
    # only positive samples: no sign bit toggles
    pos = api.hist_readout(hr.columns(hr.positive(3000)[None, :], 3000)[0][0, 0])
    assert pos["negative_share"] == 0.0 and pos["toggling"] >> 27 == 0 and pos["zero_share"] == 0.0
    # digital silence
    sil = api.hist_readout(recs[-2])
    assert sil["zero_share"] == 1.0 and sil["peak"] == 0.0 and sil["peak_db"] == -math.inf and sil["median_db"] == -math.inf
    assert sil["effective_bits"] == 0 and sil["toggling"] == 0
    # count 0: the documented NaNs
    none = api.hist_readout(hr.identity())
    assert all(math.isnan(none[k]) for k in ("zero_share", "negative_share", "peak_db", "median_db")) and none["peak"] == 0.0
    assert none["toggling"] == 0 and none["effective_bits"] == 0
    assert api.lib().sgz_hist_readout(None, None) == E and _error() == "sgz_hist_readout: null argument"


def test_refusals_before_the_device_is_touched():
    """every argument check of the stage call and of the stream's calls that needs no device: made on fake, never dereferenced addresses"""
    L = api.lib()
    good, carry, hist = 0x10000, 0x20000, 0x30000
    call = L.sgz_stage_hist_columns
    who = "sgz_stage_hist_columns: "
    aligned = who + "d_planar aligned to 4 bytes, d_carry and d_hist to 16"
    for args, why in (((None, 128, 1, 100, 8, 0, 1, 0, carry, hist), "null d_planar"),
                      ((good, 128, 0, 100, 8, 0, 1, 0, carry, hist), "1 .. 64 channels"),
                      ((good, 128, 65, 100, 8, 0, 1, 0, carry, hist), "1 .. 64 channels"),
                      ((good, 128, 1, 100, 0, 0, 1, 0, carry, hist), "m >= 1 samples per column"),
                      ((good, 128, 1, 100, 8, 8, 1, 0, carry, hist), "held < m"),
                      ((good, 99, 1, 100, 8, 0, 1, 0, carry, hist), "channel_stride < nsamples"),
                      ((good, 128, 1, 100, 8, 0, 1, 65, carry, hist), "slices 0 (automatic) or 1 .. 64"),
                      ((good + 2, 128, 1, 100, 8, 0, 1, 0, carry, hist), aligned[len(who):]),
                      ((good, 128, 1, 100, 8, 3, 1, 0, carry + 8, hist), aligned[len(who):]),
                      ((good, 128, 1, 100, 8, 0, 1, 0, carry, hist + 8), aligned[len(who):]),
                      ((good, 128, 1, 100, 8, 3, 1, 0, None, hist), "d_carry is read (held > 0) or written (samples stay open)"),
                      ((good, 128, 1, 100, 8, 0, 0, 0, None, hist), "d_carry is read (held > 0) or written (samples stay open)"),
                      ((good, 128, 1, 100, 8, 0, 1, 0, carry, None), "d_hist is written (a column closes)"),
                      ((good, 128, 1, 0, 8, 3, 1, 0, carry, None), "d_hist is written (a column closes)")):
        assert call(*args, None) == E and _error() == who + why, (args, _error())
    assert call(good, 128, 64, 0, 8, 0, 1, 0, None, None, None) == api.SGZ_OK              # nothing arrives, nothing is flushed: nothing launched
    assert call(good, 128, 1, 0, 8, 3, 0, 0, carry, hist, None) == api.SGZ_OK
    # the stream's calls on a null stream
    assert L.sgz_pcm_stream_set_hist(None, 128, None, 0) == E and _error() == "null stream"
    assert L.sgz_pcm_stream_flush_hist(None) == E
    assert L.sgz_pcm_stream_hist_state(None, None, None) == E and L.sgz_pcm_stream_hist_for(None, 100, 0) == 0


def test_hist_kernels_are_in_the_code_object():
    import codeobj_report as cr
    lib = os.path.join(ROOT, "signalizer_amd", "libsgz.so")
    if not (os.path.exists(lib) and os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("library or llvm tools not present")
    rows = [r for r in cr.kernels(lib) if any(k in r["demangled"] for k in ("histTileKernel", "histSliceKernel", "histEmitKernel"))]
    assert len(rows) == 3, [r["demangled"] for r in rows]
    bad = [(r["demangled"], r.get("vgpr_spill_count"), r.get("sgpr_spill_count"), r.get("private_segment_fixed_size")) for r in rows
           if r.get("vgpr_spill_count", 0) or r.get("sgpr_spill_count", 0) or r.get("private_segment_fixed_size", 0)]
    assert not bad, bad
