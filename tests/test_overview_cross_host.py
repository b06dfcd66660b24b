"""The cross overview (sgz.h, "The cross overview"; csrc/overview_cross.hip) without a GPU: the exports, the record's layout, the two kernels
in the built gfx950 code object (no scratch, no spill), the refusals every call makes before it touches the device, and the host helpers:
  sgz_overview_cross_quantise  == the restatement (tests/overview_cross_ref.py) and == exact fractions.Fraction arithmetic, on the edge values;
  sgz_overview_cross_fold      over columns and over bands == folds in Python integers;
  sgz_overview_cross_readout   the six means within 2 ulp of exact rationals, coherence, phase and correlation within 8 ulp of an fp64
                               evaluation written differently; every NaN case;
  sgz_cross_edges_octave       == the restatement as integers, after the test has shown on its own fp64 values that no edge product lies
                               within 1e-9 (relative) of an integer;
  sgz_overview_cross_unit      == the oracle's invSize squared with (N/2)^2 in fp64."""
import cmath
import ctypes as C
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from signalizer_amd import api, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import overview_cross_ref as ocr  # noqa: E402

NAMES = ("sgz_plan_set_cross_edges", "sgz_stage_overview_cross", "sgz_spectrogram_overview_cross_device", "sgz_spectrogram_overview_cross_host",
         "sgz_overview_cross_quantise", "sgz_overview_cross_fold", "sgz_overview_cross_readout", "sgz_overview_cross_unit",
         "sgz_cross_edges_octave", "sgz_pcm_stream_set_cross_edges", "sgz_pcm_stream_feed_overview_cross", "sgz_spectrogram_overview_cross_pcm")
KERNELS = ("overviewCrossTileKernel", "overviewCrossEmitKernel")
E, U = api.SGZ_EINVAL, api.SGZ_EUNSUPPORTED
FLT_MAX = np.float32(3.4028234663852886e38)
TINY = np.array([1], np.uint32).view(np.float32)[0]                          # the smallest subnormal
N_LOG2 = 10                                                                  # the edge values are laid out for N = 1024: s = 2^42
UNIT = np.float32(2.0 ** -22)                                                # (x UNIT)(y UNIT) s = x y / 4: products of small integers tie


def _small(**over):
    return config.spectrum_config(**{**dict(window_size=64, hop=16, axis_points=33, channel_mode=config.CH_PHASE, bin_interp=config.INTERP_LINEAR), **over})


@pytest.fixture(scope="module")
def plan():
    return api.Plan(_small())                                                # host tables only: never uploaded here


@pytest.fixture(scope="module")
def buf():
    """a host block that stands for any non-NULL buffer: every call here is refused before a buffer is looked at"""
    b = np.zeros(8192, np.float64)
    return b, b.ctypes.data_as(C.c_void_p)


def _u32(values):
    a = np.ascontiguousarray(values, np.uint32)
    return a, a.ctypes.data_as(C.c_void_p)


def edge_bins():
    """(lr, li, rr, ri) float32 [n] each: the edge values of the definition"""
    root = np.float32(math.sqrt(2.0 ** 21))                                  # lr^2 s = 2^63: the clamp
    around = [root]
    for _ in range(3):
        around = [np.nextafter(around[0], np.float32(0))] + around + [np.nextafter(around[-1], np.float32(np.inf))]
    rows = [(0.0, 0.0, 0.0, 0.0), (-0.0, 0.0, -0.0, 0.0), (0.0, -0.0, 0.0, -0.0), (TINY, 0.0, TINY, 0.0), (TINY, -TINY, -TINY, TINY),
            (FLT_MAX, FLT_MAX, FLT_MAX, FLT_MAX), (FLT_MAX, 0.0, -FLT_MAX, 0.0), (0.0, FLT_MAX, -FLT_MAX, 0.0), (-FLT_MAX, FLT_MAX, FLT_MAX, FLT_MAX),
            (1.0, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, 1.0), (0.0, 1.0, 1.0, 0.0), (0.6, -0.8, -0.28, 0.96), (1e10, 0.0, 1e-10, 0.0)]
    for v in around:                                                         # values straddling the clamp, in every sum and both signs
        rows += [(v, 0.0, v, 0.0), (v, 0.0, -v, 0.0), (0.0, v, v, 0.0), (0.0, v, -v, 0.0), (0.0, v, 0.0, -v)]
    for x, y, z, w in ((1, 1, 1, 1), (1, 3, 3, 1), (1, 5, 5, 1), (3, 5, 5, 3), (3, 7, 1, 1), (2, 0, 3, 0), (2, 0, -3, 0), (0, 2, 3, 0), (0, 2, -3, 0),
                       (2, 0, 7, 0), (2, 0, 0, 5), (2, 0, 0, -5), (1, 1, 5, -3), (3, 0, 0.5, 0), (5, 0, -0.5, 0), (0, 1, 0.5, 0), (1, 0, 0, 1.5)):
        rows.append((x * UNIT, y * UNIT, z * UNIT, w * UNIT))                # ties: u = an integer + 1/2
    bad = (np.nan, np.inf, -np.inf)
    for at in range(4):                                                      # a non-finite float in each of the four positions
        for b in bad:
            row = [1.5, -2.5, 0.25, 4.0]
            row[at] = b
            rows.append(tuple(row))
    rows.append((np.nan, np.inf, -np.inf, np.nan))
    a = np.array(rows, np.float32)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy()


def exact_q(n, lr, li, rr, ri):
    """the definition in exact rationals: each product exact, each sum rounded once to fp64 (int / int division is correctly rounded), the
    scaling exact, the clamp, ties to even (round() of a Fraction)"""
    if not all(math.isfinite(v) for v in (lr, li, rr, ri)):
        return None
    Lr, Li, Rr, Ri = (Fraction(float(v)) for v in (lr, li, rr, ri))
    s = Fraction(2) ** (62 - 2 * n)
    out = []
    for x in (Lr * Lr + Li * Li, Rr * Rr + Ri * Ri, Lr * Rr + Li * Ri, Li * Rr - Lr * Ri):
        u = Fraction(float(x)) * s
        out.append(round(min(max(u, -ocr.Q_MOST), ocr.Q_MOST)))
    return out


def test_exports_exist():
    L = api.lib()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(L, name), name
    for name in ("set_cross_edges", "overview_cross_columns", "overview_cross", "overview_cross_unit"):
        assert callable(getattr(api.Plan, name))
    for name in ("set_cross_edges", "feed_overview_cross", "feed_overview_cross_into"):
        assert callable(getattr(api.PcmStream, name))
    for name in ("overview_cross_pcm", "overview_cross_fold", "overview_cross_readout", "overview_cross_quantise", "cross_edges_octave"):
        assert callable(getattr(api, name))
    with open(os.path.join(ROOT, "include", "sgz.h")) as f:
        header = f.read()
    assert all(name + "(" in header for name in NAMES) and "#define SGZ_ABI_VERSION 5" in header
    assert "(5, later: the cross overview" in header and "The cross overview:" in header
    assert "(5, later: the power overview" in header and "The power overview:" in header            # the earlier entries stay
    assert "-180 dB" in header and "+9 dB" in header
    assert L.sgz_abi_version() == 5


def test_the_record_layout_is_the_dtype():
    for d in (api.OVERVIEW_CROSS_DTYPE, ocr.DTYPE):
        assert d.itemsize == 80 and d.names == ("ll", "rr", "re", "im", "count", "skipped")
        assert [d.fields[n][1] for n in d.names] == [0, 16, 32, 48, 64, 72]
        assert all(d.fields[n][0] == np.dtype(("<u8", (2,))) for n in ocr.SUMS) and d.fields["count"][0] == d.fields["skipped"][0] == np.dtype("<u8")
    assert api.OVERVIEW_CROSS_READING_DTYPE.itemsize == 72
    assert api.OVERVIEW_CROSS_READING_DTYPE.names == ("ll", "rr", "mid", "side", "re", "im", "coherence", "phase", "correlation")
    # the library's own: one bin-frame of L = R = 1 at full scale reads 1, and survives a 1:1 fold
    r = np.zeros((1, 1, 1), api.OVERVIEW_CROSS_DTYPE)
    r[0, 0, 0] = ((1 << 60, 0), (1 << 60, 0), (1 << 60, 0), (0, 0), 1, 0)
    o = api.overview_cross_readout(r)[0, 0, 0]
    assert (o["ll"], o["rr"], o["mid"], o["side"], o["re"], o["im"], o["coherence"], o["phase"], o["correlation"]) == (1, 1, 1, 0, 1, 0, 1, 0, 1)
    assert api.overview_cross_fold(r, 1).tobytes() == r.tobytes()
    with open(os.path.join(ROOT, "include", "sgz.h")) as f:
        header = f.read()
    assert "static_assert(sizeof(sgz_overview_cross_record) == 80" in header and "offsetof(sgz_overview_cross_record, skipped) == 72" in header


def test_cross_kernels_in_the_code_object_without_scratch():
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
    tile = [r for r in rows if "overviewCrossTileKernel(" in r["demangled"]][0]
    assert tile.get("group_segment_fixed_size", 0) == 256 * 18 * 8                                   # 18 64-bit slots per rank of a tile


# ---- the quantiser ------------------------------------------------------------------------------------------------------------------------
def test_quantise_equals_the_restatement_and_exact_rationals():
    lr, li, rr, ri = edge_bins()
    q, skipped = api.overview_cross_quantise(N_LOG2, lr, li, rr, ri)
    want_q, want_skipped = ocr.quantise(N_LOG2, lr, li, rr, ri)
    assert q.dtype == np.int64 and np.array_equal(q, want_q) and np.array_equal(skipped, want_skipped)
    seen = set()
    for i in range(lr.size):
        exact = exact_q(N_LOG2, lr[i], li[i], rr[i], ri[i])
        if exact is None:
            assert skipped[i] and not q[i].any(), i
            seen.add("skipped")
            continue
        assert not skipped[i] and [int(v) for v in q[i]] == exact, (i, lr[i], li[i], rr[i], ri[i], q[i], exact)
        assert q[i, 0] >= 0 and q[i, 1] >= 0
        for v in exact:
            if abs(v) == ocr.Q_MOST:
                seen.add("clamp+" if v > 0 else "clamp-")
        Lr, Li, Rr, Ri = (Fraction(float(v)) for v in (lr[i], li[i], rr[i], ri[i]))
        for j, x in enumerate((Lr * Lr + Li * Li, Rr * Rr + Ri * Ri, Lr * Rr + Li * Ri, Li * Rr - Lr * Ri)):
            u = Fraction(float(x)) * Fraction(2) ** (62 - 2 * N_LOG2)
            if u.denominator == 2 and abs(u) < ocr.Q_MOST:
                seen.add("tie down" if abs(exact[j]) < abs(u) else "tie up")
                assert exact[j] % 2 == 0
    assert seen == {"skipped", "clamp+", "clamp-", "tie down", "tie up"}, seen
    assert int(skipped.sum()) == 13
    # just below the clamp the step is 2^10 and the values are not clamped
    assert any(0 < ocr.Q_MOST - int(v) <= 2 ** 41 for v in q[:, 0])
    # seeded values over nine decades, at two sizes
    rng = np.random.default_rng(5)
    for n in (6, 15):
        f = [(10.0 ** rng.uniform(-8, 1, 4000) * rng.choice([-1.0, 1.0], 4000)).astype(np.float32) for _ in range(4)]
        q, skipped = api.overview_cross_quantise(n, *f)
        want_q, _ = ocr.quantise(n, *f)
        assert np.array_equal(q, want_q) and not skipped.any()
        for i in range(0, 4000, 97):
            assert [int(v) for v in q[i]] == exact_q(n, *(a[i] for a in f))
    z = np.zeros(1, np.float32)
    q1, s1 = np.zeros(4, np.int64), np.zeros(1, np.uint8)
    for n in (0, 2, 31):
        assert api.lib().sgz_overview_cross_quantise(n, *(a.ctypes.data_as(C.c_void_p) for a in (z, z, z, z)), 1, q1.ctypes.data_as(C.c_void_p),
                                                     s1.ctypes.data_as(C.c_void_p)) == E


# ---- the folds ----------------------------------------------------------------------------------------------------------------------------
def random_records(rng, shape):
    r = np.zeros(shape, ocr.DTYPE)
    for name in ocr.SUMS:
        r[name] = rng.integers(0, 2 ** 64, (*shape, 2), dtype=np.uint64)
        r[name][..., 1] >>= np.uint64(8)                                      # |sums| below 2^120: no fold here wraps
    for name in ("re", "im"):
        neg = rng.random(shape) < 0.5
        r[name][..., 1] = np.where(neg, r[name][..., 1] | np.uint64(0xFF00000000000000), r[name][..., 1])
    r["count"] = rng.integers(0, 2 ** 40, shape, dtype=np.uint64)
    r["skipped"] = rng.integers(0, 2 ** 40, shape, dtype=np.uint64)
    return r


def py_fold(records):
    """records [m] -> one record, in Python integers"""
    out = np.zeros((), ocr.DTYPE)
    for name in ocr.SUMS:
        total = sum(int(lo) | (int(hi) << 64) for lo, hi in records[name].reshape(-1, 2)) % 2 ** 128
        out[name] = (total & ocr.MASK64, total >> 64)
    out["count"] = sum(int(v) for v in records["count"].reshape(-1))
    out["skipped"] = sum(int(v) for v in records["skipped"].reshape(-1))
    return out


def test_the_limb_chain_equals_python_integers():
    rng = np.random.default_rng(11)
    limbs = rng.integers(0, 2 ** 62, (500, 4), dtype=np.int64)
    limbs[:50] = 2 ** 63 - 1
    limbs[50:60] = 0
    assert np.array_equal(ocr.recombine(limbs), ocr.recombine_py(limbs))
    q = np.array([0, 1, -1, 2 ** 63 - 1, -2 ** 63, ocr.Q_MOST, -ocr.Q_MOST, 12345, -12345], np.int64)
    words = ocr.recombine_py(ocr.limbs_of(q))
    assert [int(lo) | (int(hi) << 64) for lo, hi in words] == [int(v) % 2 ** 128 for v in q]


def test_fold_over_columns_and_bands_equals_python_integer_folds():
    rng = np.random.default_rng(3)
    n, pairs = 13, 2
    edges = [1, 1, 4, 9, 9, 9, 15, 20, 31, 31]
    bands = len(edges) - 1
    r = random_records(rng, (n, pairs, bands))
    for x0, x1 in ((0, n), (2, 11), (5, 6)):
        m = x1 - x0
        for cols in (1, 2, 3, m, m + 3):
            got = api.overview_cross_fold(r, cols, x0, x1)
            want_cols = min(cols, m)
            assert got.shape == (want_cols, pairs, bands)
            assert ocr.same(got, ocr.view_of(r, x0, x1, cols))
            for c in range(want_cols):
                a, b = x0 + -(-c * m // want_cols), x0 + -(-(c + 1) * m // want_cols)
                for p in range(pairs):
                    for band in range(bands):
                        assert got[c, p, band].tobytes() == py_fold(r[a:b, p, band]).tobytes()
    # over bands: every coarse edge is a fine edge; empty fine bands hold no bin and take no part; an empty coarse band is zeros
    for coarse in ([1, 31], [1, 9, 31], [4, 9, 9, 20], [1, 1, 4, 9, 9, 9, 15, 20, 31, 31], [9, 9], [15, 31]):
        got = api.overview_cross_fold(r, 4, 1, 12, edges=edges, coarse_edges=coarse)
        assert got.shape == (4, pairs, len(coarse) - 1)
        cols = ocr.view_of(r, 1, 12, 4)
        assert ocr.same(got, ocr.bands_of(cols, edges, coarse))
        for c in range(len(coarse) - 1):
            js = [j for j in range(bands) if coarse[c] <= edges[j] < edges[j + 1] <= coarse[c + 1]]
            for col in range(4):
                a, b = 1 + -(-col * 11 // 4), 1 + -(-(col + 1) * 11 // 4)
                for p in range(pairs):
                    assert got[col, p, c].tobytes() == py_fold(r[a:b, p][:, js]).tobytes()
    assert [j for j in range(bands) if 9 <= edges[j] < edges[j + 1] <= 9] == []
    # the sums wrap modulo 2^128, as two's complement sums do
    w = np.zeros((2, 1, 1), ocr.DTYPE)
    w["re"][0, 0, 0] = (ocr.MASK64, ocr.MASK64)                               # -1
    w["re"][1, 0, 0] = (5, 0)
    assert [int(v) for v in api.overview_cross_fold(w, 1)["re"][0, 0, 0]] == [4, 0]


def test_fold_refusals(buf):
    L = api.lib()
    _, p = buf
    e, ep = _u32([1, 4, 9, 31])
    for coarse in ([1, 5, 31], [2, 31], [9, 4], [1, 32]):
        c, cp = _u32(coarse)
        assert L.sgz_overview_cross_fold(p, 4, 1, ep, 3, 0, 4, 2, cp, len(coarse) - 1, p) == E, coarse
    assert b"coarse" in api.lib().sgz_last_error()
    c, cp = _u32([1, 31])
    assert L.sgz_overview_cross_fold(p, 4, 1, None, 3, 0, 4, 2, cp, 1, p) == E                      # a band fold without the fine edges
    assert L.sgz_overview_cross_fold(p, 4, 1, ep, 3, 0, 4, 2, cp, 0, p) == E
    assert L.sgz_overview_cross_fold(None, 4, 1, ep, 3, 0, 4, 2, None, 0, p) == E
    assert L.sgz_overview_cross_fold(p, 4, 1, ep, 3, 0, 4, 2, None, 0, None) == E
    assert L.sgz_overview_cross_fold(p, 4, 0, ep, 3, 0, 4, 2, None, 0, p) == E
    assert L.sgz_overview_cross_fold(p, 4, 1, ep, 0, 0, 4, 2, None, 0, p) == E
    for x0, x1, cols in ((2, 2, 1), (3, 2, 1), (0, 5, 1), (0, 4, 0)):
        assert L.sgz_overview_cross_fold(p, 4, 1, ep, 3, x0, x1, cols, None, 0, p) == E
    # a count that passes 2^64 - 1: refused, nothing written
    r = np.zeros((2, 1, 1), ocr.DTYPE)
    r["count"] = 2 ** 63
    out = np.full((1, 1, 1), 0x55, np.uint8).view(np.uint8).repeat(80).view(ocr.DTYPE).reshape(1, 1, 1)
    before = out.tobytes()
    assert L.sgz_overview_cross_fold(r.ctypes.data_as(C.c_void_p), 2, 1, None, 1, 0, 2, 1, None, 0, out.ctypes.data_as(C.c_void_p)) == E
    assert out.tobytes() == before


# ---- the readout ----------------------------------------------------------------------------------------------------------------------------
def _within(got, want, ulps):
    if math.isnan(want):
        return math.isnan(got)
    return abs(got - want) <= ulps * math.ulp(want)


def test_readout_against_exact_rationals():
    rng = np.random.default_rng(9)
    r = random_records(rng, (400,))
    r["count"] = np.maximum(r["count"], 1)
    # physical records as well: |re|, |im| <= sqrt(ll rr), small sums, exact powers of two, zeros
    small = np.zeros(12, ocr.DTYPE)
    rows = [(4 << 60, 1 << 60, 2 << 60, 0, 4), (4 << 60, 1 << 60, -(2 << 60), 0, 4), (1 << 60, 1 << 60, 0, 1 << 60, 1), (1 << 60, 1 << 60, 0, -(1 << 60), 1),
            (3, 5, -2, 1, 7), (2 ** 100, 2 ** 90, -(2 ** 94), 2 ** 93, 2 ** 33), (1, 0, 0, 0, 1), (0, 1, 0, 0, 1), (0, 0, 0, 0, 5), (9, 9, 9, 0, 3),
            (9, 9, -9, 0, 3), (10 ** 30, 10 ** 30, 10 ** 30 - 1, 12345, 10 ** 6)]
    for i, (a, b, c, d, n) in enumerate(rows):
        for name, v in zip(ocr.SUMS, (a, b, c, d)):
            small[name][i] = ((v % 2 ** 128) & ocr.MASK64, (v % 2 ** 128) >> 64)
        small["count"][i] = n
    r = np.concatenate([r, small])
    got = api.overview_cross_readout(r)
    A, B, Cs, D = (ocr.sums(r, name) for name in ocr.SUMS)
    nans = 0
    for i in range(r.size):
        a, b, c, d, n = int(A[i]), int(B[i]), int(Cs[i]), int(D[i]), int(r["count"][i])
        g = got[i]
        means = {"ll": Fraction(a, n) / 2 ** 60, "rr": Fraction(b, n) / 2 ** 60, "re": Fraction(c, n) / 2 ** 60, "im": Fraction(d, n) / 2 ** 60,
                 "mid": Fraction(max(0, a + b + 2 * c), n) / 2 ** 62, "side": Fraction(max(0, a + b - 2 * c), n) / 2 ** 62}
        for name, exact in means.items():
            assert _within(float(g[name]), float(exact), 2), (i, name, g[name], float(exact))
        # written differently: correctly rounded conversions of the integers, a hypotenuse, separate roots, the phase of a complex number
        fa, fb, fc, fd = float(a), float(b), float(c), float(d)
        assert _within(float(g["phase"]), cmath.phase(complex(fc, fd)), 8), (i, g["phase"])
        if fa * fb == 0.0:
            assert math.isnan(g["coherence"]) and math.isnan(g["correlation"]), i
            nans += 1
            continue
        h = math.hypot(fc, fd) / (math.sqrt(fa) * math.sqrt(fb))
        assert _within(float(g["coherence"]), min(1.0, h * h), 8), (i, g["coherence"], h * h)
        assert _within(float(g["correlation"]), fc / math.sqrt(fa) / math.sqrt(fb), 8), (i, g["correlation"])
    assert nans == 3
    # known answers
    k = got[400:]
    assert (k["coherence"][0], k["correlation"][0], k["phase"][0], k["mid"][0], k["side"][0]) == (1.0, 1.0, 0.0, 9 / 16, 1 / 16)
    assert (k["correlation"][1], k["phase"][1], k["mid"][1]) == (-1.0, math.pi, 1 / 16)
    assert (k["phase"][2], k["phase"][3], k["correlation"][2]) == (math.pi / 2, -math.pi / 2, 0.0)
    assert k["coherence"][9] == 1.0 and k["side"][9] == 0.0 and k["mid"][10] == 0.0
    # count == 0: every plane is NaN, whatever the sums hold
    empty = random_records(rng, (5,))
    empty["count"] = 0
    for name in api.OVERVIEW_CROSS_READING_DTYPE.names:
        assert np.isnan(api.overview_cross_readout(empty)[name]).all(), name
    assert api.lib().sgz_overview_cross_readout(None, 1, None) == E


# ---- the band tables ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("triple", [(48000.0, 32768, 3), (96000.0, 65536, 12), (44100.0, 1024, 1)], ids=str)
def test_octave_edges_equal_the_restatement(triple):
    sample_rate, N, b = triple
    f_lo, f_hi = 20.0, min(20000.0, sample_rate / 2)
    want, centres, products = ocr.edges_octave(sample_rate, N, b, f_lo, f_hi)
    # no product is so close to an integer that the last bits of an exp2 could move its ceiling
    for p in products:
        assert abs(p - round(p)) > 1e-9 * p, p
    edges, got_centres = api.cross_edges_octave(sample_rate, N, b, f_lo, f_hi)
    assert edges.dtype == np.uint32 and [int(e) for e in edges] == want
    assert len(got_centres) == len(centres) == len(want) - 1
    assert all(abs(g - c) <= 2 * math.ulp(c) for g, c in zip(got_centres, centres))
    assert centres[0] >= f_lo and centres[-1] <= f_hi and any(c == 1000.0 for c in got_centres)
    assert all(1 <= e <= N // 2 - 1 for e in want) and all(x <= y for x, y in zip(want, want[1:]))
    if (sample_rate, N) == (44100.0, 1024):
        assert want[0] == 1 and want[-1] == N // 2 - 1                        # both clamps: 31.25 Hz / sqrt 2 is below bin 1, 16 kHz sqrt 2 above N/2 - 1


def test_octave_edges_refusals():
    L = api.lib()
    e = np.zeros(64, np.uint32)
    n = C.c_uint32(0)
    ep = e.ctypes.data_as(C.c_void_p)

    def call(sr=48000.0, N=1024, b=3, lo=20.0, hi=20000.0, edges=ep, cap=64, bands=C.byref(n)):
        return L.sgz_cross_edges_octave(sr, N, b, lo, hi, edges, cap, bands, None)

    assert call() == api.SGZ_OK and n.value == 29                         # 25 Hz .. 16 kHz
    for bad in (dict(b=0), dict(b=49), dict(N=1000), dict(N=4), dict(sr=0.0), dict(lo=0.0), dict(lo=300.0, hi=200.0), dict(edges=None), dict(bands=None),
                dict(cap=29), dict(lo=1001.0, hi=1100.0)):
        assert call(**bad) == E, bad
    assert call(cap=30) == api.SGZ_OK


def test_unit_is_the_oracles_inv_size_squared(oracle):
    for over in (dict(), dict(window_size=1024, hop=256, window_type=config.WIN_RECT), dict(window_size=4096, hop=512, window_type=config.WIN_BLACKMAN_HARRIS)):
        cfg = _small(**over)
        plan = api.Plan(cfg)
        W = cfg["window_size"]
        _, scale = oracle.window(cfg["window_type"], cfg["window_symmetry"], W, cfg["window_alpha"], cfg["window_beta"])
        inv_size = np.float32(scale / (W * 0.5))                             # oracle/spectrum.c: (float)(window_scale / (W * 0.5))
        half = np.float64(plan.N // 2)
        assert plan.overview_cross_unit() == float((np.float64(inv_size) * np.float64(inv_size)) * (half * half))
    assert api.Plan(_small(window_size=1024, hop=256, window_type=config.WIN_RECT)).overview_cross_unit() == 1.0     # a unit sine on a bin: |X| = N/2
    assert api.lib().sgz_overview_cross_unit(None, None) == E


# ---- refusals before the device -----------------------------------------------------------------------------------------------------------------
def test_plans_that_are_not_phase_fft_plans_are_unsupported(buf):
    L = api.lib()
    _, p = buf
    e, ep = _u32([1, 4, 9, 31])
    channels = (C.c_void_p * 2)(p, p)
    for over in (dict(channel_mode=config.CH_SEPARATE), dict(channel_mode=config.CH_LEFT), dict(channel_mode=config.CH_COMPLEX),
                 dict(channel_mode=config.CH_PHASE, algorithm=config.ALGO_RSNT), dict(channel_mode=config.CH_SEPARATE, algorithm=config.ALGO_RSNT)):
        cfg = config.spectrum_config(window_size=64, hop=16, axis_points=33, bin_interp=config.INTERP_LINEAR, **over)
        plan = api.Plan(cfg)
        assert L.sgz_plan_set_cross_edges(plan.h, ep, 3) == U, over
        assert L.sgz_stage_overview_cross(plan.h, p, 4, 2, 0, 1, 0, p, p, None) == U, over
        assert L.sgz_spectrogram_overview_cross_device(plan.h, p, 1024, 1024, 2, p, None) == U, over
        assert L.sgz_spectrogram_overview_cross_host(plan.h, channels, 2, 1024, 2, p, None) == U, over
        c = api._as_config(cfg)
        assert L.sgz_spectrogram_overview_cross_pcm(C.byref(c), p, api.PCM_S16, 2, None, 1024, ep, 3, 2, p, None) == U, over


def test_band_table_refusals_keep_the_plan_without_a_table(plan, buf):
    L = api.lib()
    _, p = buf
    N = plan.N
    assert N == 64
    for edges in ([0, 4, 31], [1, 4, 32], [1, 9, 4, 31], [5, 4], [31, 1]):
        e, ep = _u32(edges)
        assert L.sgz_plan_set_cross_edges(plan.h, ep, len(edges) - 1) == E, edges
    e, ep = _u32([1] * 5000)
    assert L.sgz_plan_set_cross_edges(plan.h, ep, 0) == E and L.sgz_plan_set_cross_edges(plan.h, ep, 4097) == E
    assert L.sgz_plan_set_cross_edges(plan.h, None, 3) == E and L.sgz_plan_set_cross_edges(None, ep, 3) == E
    # a plan without a table: every reducing call is refused
    channels = (C.c_void_p * 2)(p, p)
    assert L.sgz_stage_overview_cross(plan.h, p, 4, 2, 0, 1, 0, p, p, None) == E
    assert b"sgz_plan_set_cross_edges" in api.lib().sgz_last_error()
    assert L.sgz_spectrogram_overview_cross_device(plan.h, p, 1024, 1024, 2, p, None) == E
    assert L.sgz_spectrogram_overview_cross_host(plan.h, channels, 2, 1024, 2, p, None) == E
    for args in ((None, p, 4, 2, 0, 1, 0, p, p), (plan.h, None, 4, 2, 0, 1, 0, p, p), (plan.h, p, 4, 0, 0, 1, 0, p, p), (plan.h, p, 4, 2, 2, 1, 0, p, p),
                 (plan.h, p, 4, 2, 0, 1, 65, p, p)):
        assert L.sgz_stage_overview_cross(*args, None) == E, args
    assert L.sgz_spectrogram_overview_cross_device(plan.h, p, 1024, 1024, 0, p, None) == E
    assert L.sgz_spectrogram_overview_cross_host(plan.h, channels, 3, 1024, 2, p, None) == E
