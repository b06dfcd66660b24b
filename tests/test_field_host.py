"""The stereo-field lane (sgz.h, "The stereo-field lane"): what needs no GPU -- the exports, the header, the boundary table, tests/field_ref.py
against hand-made frames, boundary-hugging frames and an independent fp64 restatement, the fold of finer records into coarser ones
(sgz_field_fold), the readout (sgz_field_readout), the refusals made before the device is touched, and the new kernels' code objects.
Records are compared as bytes.

The boundary-hugging frames: the issue asks for M = 2^24 - j at every boundary with vL and vR below 2^24.  At the 16 boundaries steeper than
45 degrees that has no solution (X = M tan g_k passes 2^26 at the steepest); there the roles swap, |X| = 2^24 - j and the integers M either
side (field_ref.hugging).  Every boundary and every j is kept."""
import math
import os
import re
import struct
import sys

import numpy as np
import pytest

from signalizer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_ref as fr  # noqa: E402

NAMES = ["sgz_stage_field_columns", "sgz_field_columns_limits", "sgz_field_boundaries", "sgz_field_fold", "sgz_field_readout",
         "sgz_pcm_stream_set_field", "sgz_pcm_stream_field_for", "sgz_pcm_stream_field_state", "sgz_pcm_stream_flush_field"]
E = api.SGZ_EINVAL


def _same(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a, fr.DTYPE).tobytes() == np.ascontiguousarray(b, fr.DTYPE).tobytes()


def _header():
    return open(os.path.join(ROOT, "include", "sgz.h")).read()


def test_exports_exist():
    L = api.lib()
    assert [n for n in NAMES if not hasattr(L, n)] == []
    assert [n for n in NAMES if n not in api.EXPORTS] == []
    assert L.sgz_abi_version() == 5
    assert api.FIELD_DTYPE == fr.DTYPE and api.FIELD_DTYPE.itemsize == 528 and api.FIELD_SECTORS == fr.SECTORS == 32


def test_header_names_them_and_keeps_version_5():
    text = _header()
    assert re.search(r"#define\s+SGZ_ABI_VERSION\s+5\b", text) and re.search(r"#define\s+SGZ_FIELD_SECTORS\s+32\b", text)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n                    # declared
    history = text[:text.index("#define SGZ_ABI_VERSION")]
    assert [n for n in NAMES + ["sgz_field_record", "sgz_field_reading", "SGZ_FIELD_SECTORS"] if n not in history] == []
    lane = text[text.index("/* The stereo-field lane"):]
    assert "has no counterpart" in lane[:700] and "sgz_field_record" in lane
    assert text.index("/* The loudness lane") < text.index("/* The stereo-field lane") < text.index("/* The track lane")
    for field in ("uint64_t radius[SGZ_FIELD_SECTORS]", "uint32_t count[SGZ_FIELD_SECTORS]", "uint32_t peak[SGZ_FIELD_SECTORS]", "uint32_t silent",
                  "uint32_t skipped", "uint64_t reserved"):
        assert field in lane, field


def test_limits_are_the_documented_ones():
    switch, tile = api.field_columns_limits()
    assert 1 <= switch <= tile and tile % 4 == 0, (switch, tile)
    lane = _header()
    lane = lane[lane.index("/* The stereo-field lane"):]
    assert f"({switch};" in lane and f"{tile} / m" in lane
    api.lib().sgz_field_columns_limits(None, None)                     # either result may be NULL


def test_the_table():
    lib = api.field_boundaries().astype(np.int64)
    assert np.array_equal(lib, fr.BOUNDS)                              # numpy's
    lane = _header()
    lane = lane[lane.index("/* The stereo-field lane"):lane.index("#define SGZ_FIELD_SECTORS")]
    literal = {int(k): (int(c), int(s)) for k, c, s in re.findall(r"k\s*=\s*(\d+):\s*\((-?\d+),\s*(-?\d+)\)", lane)}
    assert sorted(literal) == list(range(32)) and [literal[k] for k in range(32)] == [tuple(int(v) for v in row) for row in lib]
    assert [literal[k] for k in (0, 1, 2, 15)] == [(52686014, -1072448455), (157550647, -1062120190), (260897982, -1041563127), (1072448455, -52686014)]
    C, S = [int(v) for v in lib[:, 0]], [int(v) for v in lib[:, 1]]
    for k in range(32):
        assert C[31 - k] == C[k] and S[31 - k] == -S[k] and 0 < C[k] <= 2**30 and abs(S[k]) <= 2**30
    for k in range(31):                                                # strictly increasing in angle: the integer cross product of neighbours
        assert C[k] * S[k + 1] - S[k] * C[k + 1] > 0, k
    assert S[0] < 0 < S[31] and C[0] > 0                              # and all of them inside the open half circle: no wrap between 31 and 0


def _one(l, r):
    """the record of one sample frame"""
    return fr.columns(np.array([[l], [r]], np.float32), 1)[0][0, 0]


def _only(rec, sector, radius):
    count = np.zeros(32, np.uint32)
    count[sector] = 1
    return (np.array_equal(rec["count"], count) and np.array_equal(rec["radius"], count.astype(np.uint64) * np.uint64(radius))
            and np.array_equal(rec["peak"], count * np.uint32(radius)) and rec["silent"] == 0 and rec["skipped"] == 0 and rec["reserved"] == 0)


def test_the_four_canonical_frames():
    for (l, r), sector, radius in (((1.0, 0.0), 8, 2**23), ((0.0, 1.0), 24, 2**23), ((0.5, 0.5), 16, 2**22), ((0.5, -0.5), 0, 2**22),
                                   ((-1.0, 0.0), 8, 2**23), ((0.0, -1.0), 24, 2**23), ((-0.5, -0.5), 16, 2**22), ((-0.5, 0.5), 0, 2**22)):
        assert _only(_one(l, r), sector, radius), (l, r)


def _bits(b):
    return struct.unpack("<f", struct.pack("<I", b))[0]


def test_corner_frames_by_hand():
    inf, nan = math.inf, _bits(0x7F800001)
    # the infinities saturate at 2^26: (+inf, +inf) is mono, (+inf, -inf) antiphase, (+inf, 0) left-only, all with radius 2^26
    assert _only(_one(inf, inf), 16, 2**26) and _only(_one(-inf, -inf), 16, 2**26)
    assert _only(_one(inf, -inf), 0, 2**26) and _only(_one(-inf, inf), 0, 2**26)
    assert _only(_one(inf, 0.0), 8, 2**26) and _only(_one(0.0, -inf), 24, 2**26)
    # |x| > 8 clamps: (100, 9) is (2^26, 2^26), mono; (100, 4) keeps its direction: atan2(-2^25, 3 2^25) = -18.43 deg = -3.28 sectors
    assert _only(_one(100.0, 9.0), 16, 2**26) and _only(_one(100.0, 4.0), 13, 2**26)
    # a NaN on either side: skipped, whatever the other side holds
    for l, r in ((nan, 0.5), (0.5, nan), (nan, nan), (nan, inf), (_bits(0xFFC00001), 0.0)):
        rec = _one(l, r)
        assert rec["skipped"] == 1 and rec["silent"] == 0 and not rec["count"].any() and not rec["radius"].any() and not rec["peak"].any()
    # -0 and denormals quantise to 0: silent
    for l, r in ((0.0, 0.0), (-0.0, 0.0), (-0.0, -0.0), (_bits(1), _bits(0x807FFFFF)), (0.5 * 2.0**-23, -0.5 * 2.0**-23)):
        rec = _one(l, r)
        assert rec["silent"] == 1 and rec["skipped"] == 0 and not rec["count"].any() and not rec["radius"].any(), (l, r)
    # a denormal beside a sample: the sample alone
    assert _only(_one(_bits(1), 2.0**-23), 24, 1) and _only(_one(-(2.0**-23), -0.0), 8, 1)
    # a column of NaNs alone has only `skipped` set
    rec = fr.columns(np.full((2, 5), np.nan, np.float32), 5)[0][0, 0]
    want = np.zeros((), fr.DTYPE)
    want["skipped"] = 5
    assert rec.tobytes() == want.tobytes()
    # a mixed column by hand
    x = np.array([[1.0, 0.0, nan, 0.25, 0.0], [0.0, 0.0, 1.0, 0.25, -0.5]], np.float32)
    rec = fr.columns(x, 5)[0][0, 0]
    assert rec["silent"] == 1 and rec["skipped"] == 1 and rec["count"].sum() == 3
    assert (rec["count"][8], rec["count"][16], rec["count"][24]) == (1, 1, 1) and (rec["radius"][8], rec["radius"][16], rec["radius"][24]) == (2**23, 2**21, 2**22)


def test_boundary_hugging_frames_land_either_side():
    cases = 0
    for k in range(32):
        for j in range(8):
            below, above = fr.hugging(k, j)
            for (vl, vr), want in ((below, k), (above, (k + 1) % 32)):
                assert max(abs(vl), abs(vr)) < 2**24
                b, r = fr.sectors(np.array([vl], np.int64), np.array([vr], np.int64))
                assert int(b[0]) == want and int(r[0]) == max(abs(vl), abs(vr)), (k, j, vl, vr)
                # ... and through the quantiser: v 2^-23 is an fp32 value
                rec = _one(vl * 2.0**-23, vr * 2.0**-23)
                assert _only(rec, want, max(abs(vl), abs(vr))), (k, j, vl, vr)
                cases += 1
    assert cases == 512


def test_field_ref_against_an_fp64_restatement():
    x = fr.correlated(2**20)
    v, has = fr.quantise(x)
    assert has.all()
    vl, vr = v[0], v[1]
    live = (vl != 0) | (vr != 0)
    b, _ = fr.sectors(vl[live], vr[live])
    M, X = (vl + vr)[live].astype(np.float64), (vr - vl)[live].astype(np.float64)
    flip = M < 0
    theta = np.arctan2(np.where(flip, -X, X), np.where(flip, -M, M))
    guess = np.floor((theta + np.pi / 2) / (np.pi / 32) + 0.5).astype(np.int64) % 32
    gamma = (np.arange(32) - 15.5) * np.pi / 32
    near = (np.abs(theta[:, None] - gamma[None, :]) <= 1e-6).any(axis=1)
    left_out = float(near.mean())
    disagree = int((guess[~near] != b[~near]).sum())
    print(f"left out {left_out:.2e} of {live.sum()} frames, disagreeing {disagree}")
    assert left_out <= 1e-3 and disagree == 0
    assert len(set(b.tolist())) == 32                                  # the noise reaches every sector


def test_a_coarser_column_is_the_fold_of_the_finer_ones():
    rng = np.random.default_rng(5)
    for trial in range(12):
        S = int(rng.integers(1, 400))
        m = int(rng.integers(1, 9))
        r = int(rng.integers(2, 6))
        x = np.concatenate([fr.correlated(S, seed=trial), fr.correlated(S, seed=100 + trial) * np.float32(20.0)])     # the second pair clips
        x[rng.integers(0, 4), rng.integers(0, S)] = np.nan
        x[:, rng.integers(0, S)] = 0.0
        fine, _ = fr.columns(x, m)
        coarse, _ = fr.columns(x, m * r)
        n = fine.shape[0]
        bounds = list(range(0, n, r)) + [n]
        assert _same(fr.fold(fine, bounds), coarse), (trial, S, m, r)
        if n % r == 0:                                                  # the library's fold where its boundary rule gives these boundaries
            assert fr.view_bounds(0, n, n // r) == bounds
            assert _same(api.field_fold(fine, n // r), coarse), (trial, S, m, r)


def test_field_fold_against_brute_force_boundaries():
    rng = np.random.default_rng(6)
    x = np.concatenate([fr.correlated(24 * 40, seed=1), fr.correlated(24 * 40, seed=2) * np.float32(30.0)])
    records, _ = fr.columns(x, 40)                                     # 24 columns, two pairs
    assert records.shape == (24, 2)
    for n in (1, 2, 3, 7, 16, 24):
        for out_columns in sorted({1, 2, 3, n // 2 + 1, n, n + 5}):
            x0 = int(rng.integers(0, n))
            x1 = int(rng.integers(x0 + 1, n + 1))
            for a, b in ((0, n), (x0, x1)):
                w, cols = b - a, min(out_columns, b - a)
                bounds = [a + (k * w + cols - 1) // cols for k in range(cols + 1)]
                assert bounds == fr.view_bounds(a, b, out_columns) and bounds[0] == a and bounds[-1] == b
                assert _same(api.field_fold(records[:n], out_columns, a, b), fr.fold(records[:n], bounds)), (n, out_columns, a, b)


def test_field_fold_refusals():
    L = api.lib()
    rec = np.zeros((4, 1), fr.DTYPE)
    out = np.full((4, 528), 0xAB, np.uint8).view(fr.DTYPE)
    before = out.tobytes()
    p, q = rec.ctypes.data, out.ctypes.data
    assert L.sgz_field_fold(None, 4, 1, 0, 4, 2, q) == E and L.sgz_field_fold(p, 4, 1, 0, 4, 2, None) == E
    assert L.sgz_field_fold(p, 4, 0, 0, 4, 2, q) == E                  # pairs == 0
    assert L.sgz_field_fold(p, 4, 1, 2, 2, 2, q) == E                  # x0 >= x1
    assert L.sgz_field_fold(p, 4, 1, 0, 5, 2, q) == E                  # x1 > n
    assert L.sgz_field_fold(p, 4, 1, 0, 4, 0, q) == E                  # out_columns == 0
    for field, at in (("count", 31), ("count", 0), ("silent", None), ("skipped", None)):
        rec[:] = np.zeros((), fr.DTYPE)
        if at is None:
            rec[field][:, 0] = 2**31
        else:
            rec[field][:, 0, at] = 2**31                               # two of them: 2^32
        assert L.sgz_field_fold(p, 4, 1, 0, 4, 3, q) == E and b"2^32" in L.sgz_last_error(), field
        assert out.tobytes() == before
        assert L.sgz_field_fold(p, 4, 1, 0, 4, 4, q) == api.SGZ_OK and out.tobytes() == rec.tobytes()    # one to one: nothing folds
        out[:] = np.frombuffer(before, fr.DTYPE).reshape(out.shape)
    rec[:] = np.zeros((), fr.DTYPE)
    rec["count"][:, 0, 5] = (2**32 - 1) // 4                           # the largest that fits
    assert L.sgz_field_fold(p, 4, 1, 0, 4, 1, q) == api.SGZ_OK and int(out["count"].reshape(-1, 32)[0, 5]) == 4 * ((2**32 - 1) // 4)


def test_readout_against_numpy():
    """1e-12 absolute: every figure is a quotient or an fp64 sum of 32 terms of magnitude <= 1 after normalisation -- some 40 roundings of
    1.1e-16; the direction is ill-conditioned only where the resultant vanishes, hence records with spread <= 0.99"""
    rng = np.random.default_rng(8)
    recs = []
    for trial in range(30):
        S = int(rng.integers(1, 3000))
        x = fr.correlated(S, seed=trial) * np.float32(10.0 ** rng.uniform(-5, 1.2))
        if trial % 3 == 0:
            x[1] = x[0] * np.float32(rng.uniform(-1, 1))               # a point source
        if trial % 5 == 0:
            x[:, : S // 2] = 0.0                                        # half silent
        recs.append(fr.columns(x, S)[0][0, 0])
    big = np.zeros((), fr.DTYPE)                                       # folded: above a column's bounds
    big["radius"][3], big["count"][3], big["peak"][3] = 2**63 + 12345, 2**32 - 1, 2**26
    big["radius"][29], big["count"][29], big["peak"][29] = 2**60, 2**31, 7
    big["silent"] = 2**32 - 1
    recs.append(big)
    checked = 0
    for rec in recs:
        want = fr.readout(rec)
        got = api.field_readout(rec)
        for name in ("share", "mean", "peak"):
            assert np.abs(got[name] - want[name]).max() <= 1e-12, name
        assert abs(got["silent_share"] - want["silent_share"]) <= 1e-12
        if want["spread"] <= 0.99:
            assert abs(got["direction"] - want["direction"]) <= 1e-12 and abs(got["spread"] - want["spread"]) <= 1e-12, (got, want)
            checked += 1
    assert checked >= 20
    # the canonical directions: left-only is -pi/4, right-only +pi/4, mono 0; a point source has no spread
    for (l, r), direction in (((1.0, 0.0), -math.pi / 4), ((0.0, 1.0), math.pi / 4), ((0.5, 0.5), 0.0)):
        got = api.field_readout(_one(l, r))
        assert abs(got["direction"] - direction) <= 1e-12 and abs(got["spread"]) <= 1e-12 and got["share"].sum() == 1.0
    # no radius summed: direction and spread are NaN, the shares 0
    empty = np.zeros((), fr.DTYPE)
    empty["silent"], empty["skipped"] = 7, 2
    got = api.field_readout(empty)
    assert math.isnan(got["direction"]) and math.isnan(got["spread"]) and not got["share"].any() and not got["mean"].any() and got["silent_share"] == 1.0
    got = api.field_readout(np.zeros((), fr.DTYPE))
    assert math.isnan(got["direction"]) and got["silent_share"] == 0.0
    assert api.lib().sgz_field_readout(None, None) == E


def test_refusals_before_the_device_is_touched():
    """every argument check of the stage call and of the stream's calls that needs no device: made on fake, never dereferenced addresses"""
    L = api.lib()
    good, carry, field = 0x10000, 0x20000, 0x30000
    call = L.sgz_stage_field_columns
    assert call(None, 128, 1, 100, 8, 0, 1, 0, carry, field, None) == E                    # a null d_planar
    assert call(good, 128, 0, 100, 8, 0, 1, 0, carry, field, None) == E                    # pairs 0
    assert call(good, 128, 33, 100, 8, 0, 1, 0, carry, field, None) == E                   # pairs above 32
    assert call(good, 128, 1, 100, 0, 0, 1, 0, carry, field, None) == E                    # m == 0
    assert call(good, 128, 1, 100, 8, 8, 1, 0, carry, field, None) == E                    # held >= m
    assert call(good, 99, 1, 100, 8, 0, 1, 0, carry, field, None) == E                     # channel_stride < nsamples
    assert call(good, 128, 1, 100, 8, 0, 1, 65, carry, field, None) == E                   # slices > 64
    assert call(good + 2, 128, 1, 100, 8, 0, 1, 0, carry, field, None) == E                # d_planar not aligned to 4
    assert call(good, 128, 1, 100, 8, 3, 1, 0, carry + 8, field, None) == E                # d_carry not aligned to 16
    assert call(good, 128, 1, 100, 8, 0, 1, 0, carry, field + 8, None) == E                # nor d_field
    assert call(good, 128, 1, 100, 8, 3, 1, 0, None, field, None) == E                     # the carry is read: held > 0
    assert call(good, 128, 1, 100, 8, 0, 0, 0, None, field, None) == E                     # the carry is written: 100 % 8 samples stay open
    assert call(good, 128, 1, 100, 8, 0, 1, 0, carry, None, None) == E                     # columns close
    assert call(good, 128, 1, 0, 8, 3, 1, 0, carry, None, None) == E                       # the flushed carry is a column
    assert b"sgz_stage_field_columns" in L.sgz_last_error()
    assert call(good, 128, 1, 0, 8, 0, 1, 0, None, None, None) == api.SGZ_OK               # nothing arrives, nothing is flushed: nothing launched
    assert call(good, 128, 1, 0, 8, 3, 0, 0, carry, field, None) == api.SGZ_OK
    # the stream's calls on a null stream
    assert L.sgz_pcm_stream_set_field(None, 64, None, 0) == E and L.sgz_pcm_stream_flush_field(None) == E
    assert L.sgz_pcm_stream_field_state(None, None, None) == E and L.sgz_pcm_stream_field_for(None, 100, 0) == 0


def test_field_kernels_need_no_scratch():
    import codeobj_report as cr
    lib = os.path.join(ROOT, "signalizer_amd", "libsgz.so")
    if not (os.path.exists(lib) and os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("library or llvm tools not present")
    rows = [r for r in cr.kernels(lib) if any(k in r["demangled"] for k in ("fieldTileKernel", "fieldSliceKernel", "fieldEmitKernel"))]
    assert len(rows) == 3, [r["demangled"] for r in rows]
    bad = [(r["demangled"], r.get("vgpr_spill_count"), r.get("sgpr_spill_count"), r.get("private_segment_fixed_size")) for r in rows
           if r.get("vgpr_spill_count", 0) or r.get("sgpr_spill_count", 0) or r.get("private_segment_fixed_size", 0)]
    assert not bad, bad
