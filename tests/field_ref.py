"""The stereo-field lane's definition (sgz.h, "The stereo-field lane") in numpy int64 and Python integers; it shares nothing with the library.

v = (int32) clamp(rint(x 2^23), -2^26, +2^26).  A frame with a NaN on either side is skipped, one with vL = vR = 0 is silent; every other frame
has M = vL + vR, X = vR - vL (both negated when M < 0), n = #{k : C_k X - S_k M >= 0} over the 32 integer boundary directions (C_k, S_k) =
(rint(cos g_k 2^30), rint(sin g_k 2^30)), g_k = (k - 15.5) pi / 32, sector n mod 32 and radius max(|vL|, |vR|).  A product is below 2^57 and
the difference of two below 2^58: int64 holds them.  One record per (column, pair): per sector the sum of the radii (int64 sums of at most 2^26
a frame: exact up to 2^37 frames), the frame count and the greatest radius; the silent and the skipped frames; a reserved word of 0."""
import math

import numpy as np

SECTORS = 32
DTYPE = np.dtype([("radius", "<u8", (SECTORS,)), ("count", "<u4", (SECTORS,)), ("peak", "<u4", (SECTORS,)), ("silent", "<u4"),
                  ("skipped", "<u4"), ("reserved", "<u8")])
FULL, CLAMP = 1 << 23, 1 << 26


def boundaries():
    """int64 [32][2]: (C_k, S_k).  cos and sin in fp64 are good to 1e-16 relative; no scaled value lies within 1e-3 of a tie (asserted)"""
    out = np.zeros((SECTORS, 2), np.int64)
    for k in range(SECTORS):
        g = (k - 15.5) * math.pi / 32
        for j, v in enumerate((math.cos(g) * 2.0**30, math.sin(g) * 2.0**30)):
            assert abs(abs(v - math.floor(v)) - 0.5) > 1e-3, (k, j, v)
            out[k, j] = round(v)
    return out


BOUNDS = boundaries()


def is_nan(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def quantise(x):
    """float32 [...] -> (v int64 with 0 for a NaN, has bool).  rint(float64(x) 2^23) clipped: the fp32 expression's integers (the product is
    exact in fp64, and below 2^-102 for a denormal)"""
    x = np.ascontiguousarray(x, np.float32)
    nan = is_nan(x)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.clip(np.rint(np.where(nan, np.float32(0), x).astype(np.float64) * float(FULL)), -float(CLAMP), float(CLAMP))
    return v.astype(np.int64), ~nan


def tests_of(vl, vr):
    """quantised frames int64 [S] -> bool [S][32]: C_k X - S_k M >= 0 (meaningless for silent frames)"""
    M, X = vl + vr, vr - vl
    flip = M < 0
    M, X = np.where(flip, -M, M), np.where(flip, -X, X)
    return BOUNDS[None, :, 0] * X[:, None] - BOUNDS[None, :, 1] * M[:, None] >= 0


def sectors(vl, vr):
    """quantised frames int64 [S] -> (sector int64 [S], radius int64 [S]); a silent frame has radius 0 (and a sector that means nothing)"""
    return tests_of(vl, vr).sum(axis=1).astype(np.int64) % SECTORS, np.maximum(np.abs(vl), np.abs(vr))


def columns(planar, m, flush=True):
    """planar float32 [2 pairs][S] -> (records DTYPE [columns][pairs], samples left open).  flush: a partial last column is emitted."""
    v, has = quantise(planar)
    pairs, S = v.shape[0] // 2, v.shape[1]
    rest = S % m
    ncols = S // m + (1 if rest and flush else 0)
    out = np.zeros((ncols, pairs), DTYPE)
    used = min(S, ncols * m)
    col = np.arange(used) // m
    for p in range(pairs):
        vl, vr = v[2 * p, :used], v[2 * p + 1, :used]
        skip = ~(has[2 * p, :used] & has[2 * p + 1, :used])
        silent = ~skip & (vl == 0) & (vr == 0)
        live = ~skip & ~silent
        b, r = sectors(vl[live], vr[live])
        cell = col[live] * SECTORS + b
        radius = np.zeros(ncols * SECTORS, np.int64)
        peak = np.zeros(ncols * SECTORS, np.int64)
        np.add.at(radius, cell, r)
        np.maximum.at(peak, cell, r)
        o = out[:, p]
        o["radius"] = radius.reshape(ncols, SECTORS).astype(np.uint64)
        o["count"] = np.bincount(cell, minlength=ncols * SECTORS).reshape(ncols, SECTORS)
        o["peak"] = peak.reshape(ncols, SECTORS)
        o["silent"] = np.bincount(col[silent], minlength=ncols)[:ncols]
        o["skipped"] = np.bincount(col[skip], minlength=ncols)[:ncols]
        out[:, p] = o
    return out, (0 if flush else rest)


def add(records):
    """the fold of records (any shape) in Python integers -> one record: add, add, max, add, add"""
    r = np.zeros((), DTYPE)
    recs = np.asarray(records, DTYPE).reshape(-1)
    for b in range(SECTORS):
        r["radius"][b] = sum(int(v) for v in recs["radius"][:, b])
        r["count"][b] = sum(int(v) for v in recs["count"][:, b])
        r["peak"][b] = max([int(v) for v in recs["peak"][:, b]], default=0)
    r["silent"] = sum(int(v) for v in recs["silent"])
    r["skipped"] = sum(int(v) for v in recs["skipped"])
    return r


def fold(records, bounds):
    """records [n][pairs] -> the coarser columns [len(bounds) - 1][pairs]: column b is the fold of finer columns bounds[b] <= j < bounds[b + 1]"""
    pairs = records.shape[1]
    out = np.zeros((len(bounds) - 1, pairs), DTYPE)
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        for p in range(pairs):
            out[i, p] = add(records[a:b, p])
    return out


def view_bounds(x0, x1, out_columns):
    """the boundaries of the overview view's rule: x0 + ceil(b w / cols), b = 0 .. cols"""
    w = x1 - x0
    cols = min(out_columns, w)
    return [x0 + -(-(b * w) // cols) for b in range(cols + 1)]


def readout(rec):
    """one record -> dict in fp64: share, mean, peak [32]; direction, spread (NaN where no radius was summed), silent_share"""
    count = rec["count"].astype(np.float64)
    w = rec["radius"].astype(np.float64)
    frames = count.sum()
    theta = (np.arange(SECTORS) - 16) * np.pi / 32
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(count > 0, w / (count * 2.0**23), 0.0)
    c2, s2, total = float((w * np.cos(2 * theta)).sum()), float((w * np.sin(2 * theta)).sum()), float(w.sum())
    silent = float(rec["silent"])
    return dict(share=count / frames if frames else np.zeros(SECTORS), mean=mean, peak=rec["peak"].astype(np.float64) / 2.0**23,
                direction=0.5 * math.atan2(s2, c2) if total else math.nan, spread=1.0 - math.hypot(s2, c2) / total if total else math.nan,
                silent_share=silent / (frames + silent) if frames + silent else 0.0)


def correlated(S, seed=7):
    """the suite's noise: PCG64(seed), L = 0.5 N(0, 1), R = 0.6 L + 0.3 N'(0, 1), float32 [2][S]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    left = 0.5 * rng.standard_normal(S)
    right = 0.6 * left + 0.3 * rng.standard_normal(S)
    return np.stack([left, right]).astype(np.float32)


def hugging(k, j):
    """the two frames (vL, vR) either side of boundary k at A = 2^24 - j.  Where the boundary is no steeper than 45 degrees (|S_k| <= C_k):
    M = A and the integers X either side of the rational M S_k / C_k.  Where it is steeper, that X would pass 2^26, the quantiser's range, so
    the roles swap: |X| = A with S_k's sign and the integers M either side of X C_k / S_k.  Either way max(|M|, |X|) = A, the free integer
    is the nearest one on its side with the other's parity (vL = (M - X) / 2 and vR = (M + X) / 2 are then integers below 2^24 in
    magnitude) -> ((vL, vR) below the boundary: the test fails, (vL, vR) on or above it: the test holds)"""
    C, S = int(BOUNDS[k, 0]), int(BOUNDS[k, 1])
    A = (1 << 24) - j
    if abs(S) <= C:
        t0, frame = (A * S) // C, lambda t: (A, t)
    else:
        X = A if S > 0 else -A
        t0, frame = (C * X) // S, lambda t: (t, X)
    below = above = None
    for d in range(4):
        for t in (t0 - d, t0 + 1 + d):
            M, X = frame(t)
            if (M - X) % 2:
                continue
            holds = C * X - S * M >= 0
            if holds and above is None:
                above = ((M - X) // 2, (M + X) // 2)
            if not holds and below is None:
                below = ((M - X) // 2, (M + X) // 2)
    assert below is not None and above is not None, (k, j)
    return below, above
