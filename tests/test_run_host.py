"""The run lane (sgz.h, "The run lane"): what needs no GPU -- the exports, the header, the limits and defaults, tests/run_ref.py against a
brute-force Python loop, the fold of finer records into coarser ones (sgz_run_fold) against the per-sample definition on the coarser column,
the tie rule, the readout (sgz_run_readout), the refusals made before the device is touched, and the new kernels' code objects.  Records are
compared as bytes."""
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
import run_ref as rr  # noqa: E402

NAMES = ["sgz_stage_run_columns", "sgz_run_columns_limits", "sgz_run_params_default", "sgz_run_fold", "sgz_run_readout",
         "sgz_pcm_stream_set_run", "sgz_pcm_stream_run_for", "sgz_pcm_stream_run_state", "sgz_pcm_stream_flush_run"]
E = getattr(api, "SGZ_EINVAL", None)
PARAMS = [rr.DEFAULT, (3, 1), (1, 0), (2**26, 2**23)]


def _same(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a, rr.DTYPE).tobytes() == np.ascontiguousarray(b, rr.DTYPE).tobytes()


def _header():
    return open(os.path.join(ROOT, "include", "sgz.h")).read()


def _error():
    return api.lib().sgz_last_error().decode()


def test_exports_exist():
    L = api.lib()
    assert [n for n in NAMES if not hasattr(L, n)] == []
    assert [n for n in NAMES if n not in api.EXPORTS] == []
    assert L.sgz_abi_version() == 5
    assert api.RUN_DTYPE == rr.DTYPE and api.RUN_DTYPE.itemsize == 96
    assert api.RUN_CARRY_DTYPE == rr.CARRY_DTYPE and api.RUN_CARRY_DTYPE.itemsize == 112
    assert api.RUN_NAN == rr.NAN == -2**31 and (api.RUN_HOT, api.RUN_QUIET, api.RUN_FLAT) == (0, 1, 2)
    assert C.sizeof(api.RunParams) == 8 and C.sizeof(api.RunReading) == 80
    for name in ("RunReading", "run_params_default", "run_columns_limits", "stage_run_columns", "run_fold", "run_readout"):
        assert hasattr(api, name), name
    for name in ("set_run", "run_for", "run_state", "flush_run"):
        assert hasattr(api.PcmStream, name), name


def test_header_names_them_and_keeps_version_5():
    text = _header()
    assert re.search(r"#define\s+SGZ_ABI_VERSION\s+5\b", text)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n                    # declared
    history = text[:text.index("#define SGZ_ABI_VERSION")]
    assert "(5, later: the run lane -- " in history
    assert [n for n in NAMES + ["sgz_run_params", "sgz_run_record", "sgz_run_carry", "sgz_run_reading", "SGZ_RUN_NAN"] if n not in history] == []
    lane = text[text.index("/* The run lane"):]
    assert "has no" in lane[:900] and "96 bytes" in lane and "112-byte" in lane
    assert text.index("/* The histogram lane") < text.index("/* The run lane") < text.index("/* The track lane")
    for name, value in (("SGZ_RUN_HOT", "0"), ("SGZ_RUN_QUIET", "1"), ("SGZ_RUN_FLAT", "2")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), lane), name
    struct = lane[lane.index("typedef struct sgz_run_of"):lane.index("} sgz_run_of;")]
    assert re.findall(r"uint32_t\s+(\w+)", struct) == list(rr.FIELDS)
    struct = lane[lane.index("typedef struct sgz_run_record"):lane.index("} sgz_run_record;")]
    assert re.findall(r"(?:uint32_t|sgz_run_of)\s+(\w+)", struct) == ["len", "skipped", "crossings", "reserved0", "of", "reserved"]
    assert [f for f in rr.DTYPE.names] == ["len", "skipped", "crossings", "reserved0", "of", "reserved"] and rr.DTYPE.fields["of"][1] == 16


def test_limits_and_defaults_are_the_documented_ones():
    switch, tile = api.run_columns_limits()
    assert 1 <= switch <= tile and tile % 4 == 0, (switch, tile)
    lane = _header()
    lane = lane[lane.index("/* The run lane"):]
    assert f"({switch};" in lane and f"{tile} / m" in lane
    api.lib().sgz_run_columns_limits(None, None)                       # either result may be NULL
    p = api.run_params_default()
    assert (p.hot, p.quiet) == (2**23 - 2**8, 0) == rr.DEFAULT
    assert p.hot == int(np.float32(32767 / 32768) * 2**23)             # the positive full scale of 16-bit PCM
    api.lib().sgz_run_params_default(None)


def test_the_restatement_against_a_plain_python_loop():
    """run_ref.records (numpy over the definition) equals run_ref.loop_record (the definition in Python integers) column by column"""
    x = np.stack([rr.busy(700, seed=1), rr.clipped(700), np.zeros(700, np.float32), rr.busy(700, seed=2)])
    x[3, :5] = np.nan
    for m, params in ((1, rr.DEFAULT), (2, (3, 1)), (7, (3, 1)), (64, rr.DEFAULT), (700, (2, 0)), (1000, (3, 1))):
        got, _ = rr.records(x, m, params)
        for d in range(x.shape[0]):
            for c in range(got.shape[0]):
                a, b = c * m, min((c + 1) * m, 700)
                assert rr.as_dict(got[c, d]) == rr.loop_record(x[d, a:b], params, before=x[d, :a]), (m, d, c)
        assert (got["reserved0"] == 0).all() and (got["reserved"] == 0).all()
    # a stream behind a history equals the whole stream cut there
    whole, _ = rr.records(x, 64, (3, 1))
    for cut in (64, 128):
        got, _ = rr.records(x[:, cut:], 64, (3, 1), history=rr.history_after(x[:, :cut]))
        assert _same(got, whole[cut // 64:])
    # a column of no samples is the all-zero record
    assert rr.records(np.zeros((1, 0), np.float32), 4)[0].shape == (0, 1)
    assert rr.as_dict(np.zeros((), rr.DTYPE)) == rr.loop_record([], rr.DEFAULT)


def _pieces(rng, S):
    """a random cut of [0, S) into pieces, empty ones included"""
    cuts = sorted(int(c) for c in rng.integers(0, S + 1, int(rng.integers(0, 9))))
    return [0] + cuts + [S]


def test_the_fold_of_random_cuts_is_the_definition():
    """the fold, here run_ref's and the library's, of the records of ANY pieces of a column -- each piece's record taken from the definition
    with the stream in front of it -- is the column's record: random signals with NaNs, random cuts, empty pieces"""
    rng = np.random.default_rng(11)
    for trial in range(300):
        S = int(rng.integers(1, 200))
        x = rr.busy(S, seed=1000 + trial)[None, :]
        params = PARAMS[trial % len(PARAMS)]
        v, valid = rr.quantise(x)
        P, start, cross = rr.predicates(v[0], params)
        bounds = _pieces(rng, S)
        parts = np.zeros((len(bounds) - 1, 1), rr.DTYPE)
        for j, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
            parts[j, 0] = rr.column_record(P[:, a:b], start[:, a:b], cross[a:b], valid[0, a:b])
        want = rr.column_record(P, start, cross, valid[0])
        assert rr.fold(parts, [0, len(parts)])[0, 0].tobytes() == want.tobytes(), (trial, bounds)
        assert api.run_fold(parts, 1)[0, 0].tobytes() == want.tobytes(), (trial, bounds)


def test_run_fold_against_the_per_sample_loop_on_the_coarser_column():
    rng = np.random.default_rng(6)
    m, n = 10, 24
    x = np.stack([rr.busy(n * m, seed=3), rr.clipped(n * m, period=23.0)])
    x[0, 80:100] = np.nan                                               # two columns of NaNs alone
    x[1, 30:75] = 0.0                                                   # a hole across column boundaries
    params = (3, 1)
    fine, _ = rr.records(x, m, params)
    v, valid = rr.quantise(x)
    preds = [rr.predicates(v[d], params) for d in range(2)]

    def coarse(bounds):
        out = np.zeros((len(bounds) - 1, 2), rr.DTYPE)
        for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
            for d in range(2):
                P, start, cross = preds[d]
                out[i, d] = rr.column_record(P[:, a * m:b * m], start[:, a * m:b * m], cross[a * m:b * m], valid[d, a * m:b * m])
        return out

    for count in (1, 2, 3, 7, 16, 24):
        for out_columns in sorted({1, 2, 3, count // 2 + 1, count, count + 5}):         # above and below w
            x0 = int(rng.integers(0, count))
            x1 = int(rng.integers(x0 + 1, count + 1))
            for a, b in ((0, count), (x0, x1)):
                bounds = rr.view_bounds(a, b, out_columns)
                assert bounds[0] == a and bounds[-1] == b
                got = api.run_fold(fine[:count], out_columns, a, b)
                assert _same(got, coarse(bounds)), (count, out_columns, a, b)
                assert _same(got, rr.fold(fine[:count], bounds))
    # a one-sample check by hand on the tail of the loop above: column 8 and 9 of channel 0 are NaNs alone
    assert int(fine[8, 0]["skipped"]) == 10 and int(fine[8, 0]["len"]) == 10 and int(fine[8, 0]["of"][rr.FLAT]["count"]) == 0


def test_a_coarser_column_is_the_fold_of_the_finer_ones():
    rng = np.random.default_rng(5)
    for trial in range(10):
        S = int(rng.integers(1, 400))
        m = int(rng.integers(1, 9))
        r = int(rng.integers(2, 6))
        x = np.stack([rr.busy(S, seed=trial), rr.clipped(S, period=7.0 + trial)])
        params = PARAMS[trial % len(PARAMS)]
        fine, _ = rr.records(x, m, params)
        coarse, _ = rr.records(x, m * r, params)
        n = fine.shape[0]
        bounds = list(range(0, n, r)) + [n]
        assert _same(rr.fold(fine, bounds), coarse), (trial, S, m, r)
        if n % r == 0:                                                  # the library's fold where its boundary rule gives these boundaries
            assert rr.view_bounds(0, n, n // r) == bounds
            assert _same(api.run_fold(fine, n // r), coarse), (trial, S, m, r)


def _hot(pattern):
    """a float signal from a string: 'H' hot, '.' not"""
    return np.array([1.0 if c == "H" else 0.25 for c in pattern], np.float32)[None, :]


def test_ties_take_the_earlier_run():
    # two runs of equal length in one output column, in different source columns
    x = _hot("..HHH..." "...HHH.." "........")
    fine, _ = rr.records(x, 8)
    got = api.run_fold(fine, 1)[0, 0]["of"][rr.HOT]
    assert (int(got["longest"]), int(got["at"]), int(got["runs"]), int(got["count"])) == (3, 2, 2, 6)
    # ... and inside one source column (the kernel's or the reference's business: the fold only passes it on)
    x = _hot(".HH..HH." "........")
    fine, _ = rr.records(x, 8)
    assert (int(fine[0, 0]["of"][rr.HOT]["longest"]), int(fine[0, 0]["of"][rr.HOT]["at"])) == (2, 1)
    assert int(api.run_fold(fine, 1)[0, 0]["of"][rr.HOT]["at"]) == 1
    # a joined run that equals an earlier one gives the earlier
    x = _hot(".HHH..HH" "H......." "........")
    fine, _ = rr.records(x, 8)
    got = api.run_fold(fine, 1)[0, 0]["of"][rr.HOT]
    assert (int(got["longest"]), int(got["at"]), int(got["runs"])) == (3, 1, 2)
    # a joined run that equals a LATER one gives the joined one, and one that beats both wins
    x = _hot("......HH" "H..HHH.." "........")
    fine, _ = rr.records(x, 8)
    got = api.run_fold(fine, 1)[0, 0]["of"][rr.HOT]
    assert (int(got["longest"]), int(got["at"])) == (3, 6)
    x = _hot(".HHH..HH" "HH..HHH." "........")
    fine, _ = rr.records(x, 8)
    got = api.run_fold(fine, 1)[0, 0]["of"][rr.HOT]
    assert (int(got["longest"]), int(got["at"]), int(got["head"]), int(got["tail"])) == (4, 6, 0, 0)        # (the last column has no hot sample)
    # every sample hot: head == tail == longest == len, across three source columns
    x = _hot("H" * 24)
    got = api.run_fold(rr.records(x, 8)[0], 1)[0, 0]
    assert all(int(got["of"][rr.HOT][f]) == 24 for f in ("count", "longest", "head", "tail")) and int(got["of"][rr.HOT]["runs"]) == 1
    assert int(got["of"][rr.FLAT]["count"]) == 23 and int(got["of"][rr.FLAT]["at"]) == 1 and int(got["len"]) == 24
    # the fold is not commutative
    a, b = rr.records(_hot("...HH"), 5)[0][0, 0], rr.records(_hot("H...."), 5)[0][0, 0]
    assert rr.fold_pair(a, b).tobytes() != rr.fold_pair(b, a).tobytes()


def test_fold_refusals_write_nothing():
    L = api.lib()
    rec = np.zeros((4, 1), rr.DTYPE)
    out = np.full((4, 96), 0xAB, np.uint8).view(rr.DTYPE)
    before = out.tobytes()
    p, q = rec.ctypes.data, out.ctypes.data
    assert L.sgz_run_fold(None, 4, 1, 0, 4, 2, q) == E and _error() == "sgz_run_fold: null argument"
    assert L.sgz_run_fold(p, 4, 1, 0, 4, 2, None) == E
    assert L.sgz_run_fold(p, 4, 0, 0, 4, 2, q) == E and _error() == "sgz_run_fold: channels >= 1"
    assert L.sgz_run_fold(p, 4, 1, 2, 2, 2, q) == E                    # x0 >= x1
    assert L.sgz_run_fold(p, 4, 1, 0, 5, 2, q) == E                    # x1 > n
    assert L.sgz_run_fold(p, 4, 1, 0, 4, 0, q) == E                    # out_columns == 0
    rec["len"][:, 0] = 2**31                                            # two of them: 2^32
    assert L.sgz_run_fold(p, 4, 1, 0, 4, 3, q) == E
    assert _error() == "sgz_run_fold: a folded column counts more than 2^32 - 1 samples"
    assert out.tobytes() == before
    assert L.sgz_run_fold(p, 4, 1, 0, 4, 4, q) == api.SGZ_OK           # one to one: nothing folds but the identity
    assert np.array_equal(out["len"], rec["len"])
    rec["len"][:, 0] = (2**32 - 1) // 4                                 # the largest that fits, every sample quiet
    for f in ("count", "longest", "head", "tail"):
        rec["of"][f][:, 0, rr.QUIET] = (2**32 - 1) // 4
    assert L.sgz_run_fold(p, 4, 1, 0, 4, 1, q) == api.SGZ_OK
    got = out.reshape(-1)[0]
    assert int(got["len"]) == 4 * ((2**32 - 1) // 4) == int(got["of"][rr.QUIET]["longest"]) == int(got["of"][rr.QUIET]["head"])


def _close(a, b):
    """1e-12 relative, or the same NaN: a quotient or two of fp64 values"""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return abs(a - b) <= 1e-12 * max(1.0, abs(a), abs(b))


def test_readout_against_numpy():
    recs = [rr.records(rr.busy(3000, seed=s)[None, :], 3000, (3, 1))[0][0, 0] for s in range(6)]
    recs.append(rr.records(rr.clipped(4410)[None, :], 4410)[0][0, 0])
    recs.append(np.zeros((), rr.DTYPE))
    for rec in recs:
        for rate in (44100.0, 48000.0, 1.0):
            want, got = rr.readout(rec, rate), api.run_readout(rec, rate)
            for name in ("share", "longest_seconds", "at_seconds"):
                assert all(_close(g, w) for g, w in zip(got[name], want[name])), (name, got, want)
            assert _close(got["crossing_hz"], want["crossing_hz"])
    # a clipped sine of period 53 at 44100: 2 crossings a period
    clip = api.run_readout(recs[-2], 44100.0)
    assert abs(clip["crossing_hz"] - 44100.0 / 53.0) < 5.0 and clip["share"][rr.HOT] > 0.3 and clip["longest_seconds"][rr.HOT] > 5 / 44100.0
    none = api.run_readout(recs[-1], 44100.0)
    assert all(math.isnan(s) for s in none["share"]) and math.isnan(none["crossing_hz"]) and none["longest_seconds"] == (0.0, 0.0, 0.0)
    L = api.lib()
    r, rec = api.RunReading(), np.zeros(1, rr.DTYPE)
    assert L.sgz_run_readout(None, 44100.0, C.byref(r)) == E and _error() == "sgz_run_readout: null argument"
    assert L.sgz_run_readout(rec.ctypes.data, 44100.0, None) == E
    for rate in (0.0, -1.0, math.nan, math.inf):
        assert L.sgz_run_readout(rec.ctypes.data, rate, C.byref(r)) == E and _error() == "sgz_run_readout: rate > 0"


def test_refusals_before_the_device_is_touched():
    """every argument check of the stage call and of the stream's calls that needs no device: made on fake, never dereferenced addresses"""
    L = api.lib()
    good, carry, runs = 0x10000, 0x20000, 0x30000
    call = L.sgz_stage_run_columns
    who = "sgz_stage_run_columns: "
    ok = C.byref(api.run_params_default())
    aligned = "d_planar aligned to 4 bytes, d_carry and d_runs to 16"
    needed = "d_carry is read (continued) or written (nsamples > 0)"
    #          planar stride ch  n  params m held flush continued slices carry runs
    for args, why in (((None, 128, 1, 100, ok, 8, 0, 1, 0, 0, carry, runs), "null d_planar"),
                      ((None, 128, 1, 100, None, 8, 0, 1, 0, 0, carry, runs), "null d_planar"),
                      ((good, 128, 1, 100, None, 8, 0, 1, 0, 0, carry, runs), "null params"),
                      ((good, 128, 0, 100, ok, 8, 0, 1, 0, 0, carry, runs), "1 .. 64 channels"),
                      ((good, 128, 65, 100, ok, 8, 0, 1, 0, 0, carry, runs), "1 .. 64 channels"),
                      ((good, 128, 1, 100, ok, 0, 0, 1, 0, 0, carry, runs), "m >= 1 samples per column"),
                      ((good, 128, 1, 100, ok, 8, 8, 1, 1, 0, carry, runs), "held < m"),
                      ((good, 128, 1, 100, ok, 8, 3, 1, 0, 0, carry, runs), "held > 0 needs continued != 0 (a stream that begins here has no open column)"),
                      ((good, 99, 1, 100, ok, 8, 0, 1, 0, 0, carry, runs), "channel_stride < nsamples"),
                      ((good, 128, 1, 100, ok, 8, 0, 1, 0, 65, carry, runs), "slices 0 (automatic) or 1 .. 64"),
                      ((good + 2, 128, 1, 100, ok, 8, 0, 1, 0, 0, carry, runs), aligned),
                      ((good, 128, 1, 100, ok, 8, 3, 1, 1, 0, carry + 8, runs), aligned),
                      ((good, 128, 1, 100, ok, 8, 0, 1, 0, 0, carry, runs + 8), aligned),
                      ((good, 128, 1, 100, ok, 8, 0, 1, 0, 0, None, runs), needed),
                      ((good, 128, 1, 0, ok, 8, 3, 1, 1, 0, None, runs), needed),
                      ((good, 128, 1, 100, ok, 8, 0, 1, 0, 0, carry, None), "d_runs is written (a column closes)"),
                      ((good, 128, 1, 0, ok, 8, 3, 1, 1, 0, carry, None), "d_runs is written (a column closes)")):
        assert call(*args, None) == E and _error() == who + why, (args, _error())
    for hot, quiet in ((0, 0), (2**26 + 1, 0), (5, 5), (5, 6), (2**32 - 1, 0)):
        bad = api.RunParams(hot, quiet)
        assert call(good, 128, 1, 100, C.byref(bad), 8, 0, 1, 0, 0, carry, runs, None) == E
        assert _error() == who + "1 <= hot <= 2^26 and quiet < hot", (hot, quiet)
    for hot, quiet in ((1, 0), (2**26, 2**26 - 1)):                     # the widest valid ones, on a call that launches nothing
        fine = api.RunParams(hot, quiet)
        assert call(good, 128, 64, 0, C.byref(fine), 8, 0, 1, 0, 0, None, None, None) == api.SGZ_OK
    assert call(good, 128, 1, 0, ok, 8, 3, 0, 1, 0, carry, runs, None) == api.SGZ_OK       # nothing arrives, nothing is flushed: nothing launched
    # the stream's calls on a null stream
    assert L.sgz_pcm_stream_set_run(None, ok, 128, None, 0) == E and _error() == "null stream"
    assert L.sgz_pcm_stream_flush_run(None) == E
    assert L.sgz_pcm_stream_run_state(None, None, None) == E and L.sgz_pcm_stream_run_for(None, 100, 0) == 0


def test_run_kernels_are_in_the_code_object():
    import codeobj_report as cr
    lib = os.path.join(ROOT, "signalizer_amd", "libsgz.so")
    if not (os.path.exists(lib) and os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("library or llvm tools not present")
    rows = [r for r in cr.kernels(lib) if any(k in r["demangled"] for k in ("runTileKernel", "runSliceKernel", "runEmitKernel"))]
    assert len(rows) == 3, [r["demangled"] for r in rows]
    bad = [(r["demangled"], r.get("vgpr_spill_count"), r.get("sgpr_spill_count"), r.get("private_segment_fixed_size")) for r in rows
           if r.get("vgpr_spill_count", 0) or r.get("sgpr_spill_count", 0) or r.get("private_segment_fixed_size", 0)]
    assert not bad, bad
