"""The flux overview's definition (sgz.h, "The flux overview") restated in Python integers and numpy.  It shares no code with the library: the
quantiser is numpy's fp64 product, minimum and rint (ties to even); every sum is a Python int; the fold is written out field by field."""
import numpy as np

DTYPE = np.dtype({"names": ["amp", "mom1", "mom2", "flux", "flux_max", "flux_at", "count", "nans"],
                  "formats": [("<u8", (2,)), ("<u8", (2,)), ("<u8", (2,)), ("<u8", (2,)), "<u8", "<u8", "<u4", "<u4"],
                  "offsets": [0, 16, 32, 48, 64, 72, 80, 84], "itemsize": 88})
NONE = 2 ** 64 - 1
MASK = 2 ** 64 - 1
SUMS = ("amp", "mom1", "mom2", "flux")


def quantise(x):
    """a(x) = rint(min(|x| 2^30, 2^34)) as uint64; 0 for a NaN"""
    x = np.asarray(x, np.float32)
    nan = np.isnan(x)
    d = np.abs(np.where(nan, np.float32(0), x).astype(np.float64)) * 2.0 ** 30
    return np.rint(np.minimum(d, 2.0 ** 34)).astype(np.uint64)


def _weighted(a, w):
    """sum_i w_i a_i over the last axis as Python ints, object array of the leading shape: a in three 12-bit limbs, so that every partial sum
    stays below 2^63 for w < 2^34 and fewer than 2^17 terms"""
    assert a.shape[-1] < 2 ** 17 and int(w.max(initial=0)) < 2 ** 34
    total = np.zeros(a.shape[:-1], object)
    for limb in range(3):
        part = ((a >> np.uint64(12 * limb)) & np.uint64(0xFFF)) * w
        total = total + (part.sum(-1, dtype=np.uint64).astype(object) << (12 * limb))
    return total


def frame_terms(mapped, prev=None):
    """mapped float32 [frames, rows, P]; prev float32 [rows, P] or None -> per frame and row A, M1, M2, F (object arrays of Python ints) and
    the NaN mark (bool), each [frames, rows]"""
    mapped = np.asarray(mapped, np.float32)
    frames, rows, P = mapped.shape
    a = quantise(mapped)
    i = np.arange(P, dtype=np.uint64)
    A = _weighted(a, np.ones(P, np.uint64))
    M1 = _weighted(a, i)
    M2 = _weighted(a, i * i)
    before = np.zeros_like(a)
    before[1:] = a[:-1]
    if prev is not None and frames:
        before[0] = quantise(np.asarray(prev, np.float32).reshape(rows, P))
    d = a.astype(np.int64) - before.astype(np.int64)
    F = np.maximum(d, 0).sum(-1, dtype=np.int64).astype(object)
    if prev is None and frames:
        F[0] = 0
    return A, M1, M2, F, np.isnan(mapped).any(-1)


def empty():
    return {"amp": 0, "mom1": 0, "mom2": 0, "flux": 0, "flux_max": 0, "flux_at": NONE, "count": 0, "nans": 0}


def fold(a, b):
    out = {name: a[name] + b[name] for name in SUMS + ("count", "nans")}
    best = min((-a["flux_max"], a["flux_at"]), (-b["flux_max"], b["flux_at"]))            # the greater maximum, then the smaller index
    out["flux_max"], out["flux_at"] = -best[0], best[1]
    return out


def of_frame(A, M1, M2, F, nan, index):
    return {"amp": int(A), "mom1": int(M1), "mom2": int(M2), "flux": int(F), "flux_max": int(F), "flux_at": int(index), "count": 1, "nans": int(bool(nan))}


def pack(recs):
    """nested lists of dicts -> DTYPE array of the same shape"""
    flat = []

    def walk(x):
        if isinstance(x, dict):
            flat.append(x)
            return ()
        shapes = [walk(y) for y in x]
        return (len(x),) + (shapes[0] if shapes else ())
    shape = walk(recs)
    out = np.zeros(len(flat), DTYPE)
    for j, r in enumerate(flat):
        for name in SUMS:
            assert 0 <= r[name] < 2 ** 128
            out[name][j] = (r[name] & MASK, r[name] >> 64)
        out["flux_max"][j], out["flux_at"][j], out["count"][j], out["nans"][j] = r["flux_max"], r["flux_at"], r["count"], r["nans"]
    return out.reshape(shape)


def unpack(rec):
    """one DTYPE element -> dict"""
    out = {name: int(rec[name][0]) | (int(rec[name][1]) << 64) for name in SUMS}
    out.update({name: int(rec[name]) for name in ("flux_max", "flux_at", "count", "nans")})
    return out


def overview(mapped, k, first_frame=0, prev=None, held=0, carry=None, flush=True, terms=None):
    """the columns of mapped float32 [frames, rows, P] behind `held` frames whose records are `carry` (a list of dicts, one per row):
    (DTYPE [closed columns, rows], the open column's list of dicts or None).  terms: frame_terms(mapped, prev) where the caller has them"""
    mapped = np.asarray(mapped, np.float32)
    frames, rows, _ = mapped.shape
    A, M1, M2, F, nan = terms if terms is not None else frame_terms(mapped, prev)
    cols = []
    cur = [dict(c) for c in carry] if held else [empty() for _ in range(rows)]
    n = held
    for f in range(frames):
        for r in range(rows):
            cur[r] = fold(cur[r], of_frame(A[f, r], M1[f, r], M2[f, r], F[f, r], nan[f, r], first_frame + f))
        n += 1
        if n == k:
            cols.append(cur)
            cur, n = [empty() for _ in range(rows)], 0
    left = None
    if n:
        if flush:
            cols.append(cur)
        else:
            left = cur
    return (pack(cols) if cols else np.zeros((0, rows), DTYPE)), left


def fold_columns(records, out_columns, x0=0, x1=None):
    """the boundary rule of sgz_overview_view_columns on DTYPE records [n, ...]: output column b is the fold of source columns
    ceil(b m / cols) <= j < ceil((b + 1) m / cols) of the range"""
    n = records.shape[0]
    x1 = n if x1 is None else x1
    m = x1 - x0
    cols = min(out_columns, m)
    flat = records.reshape(n, -1)
    out = []
    for b in range(cols):
        ja, jb = x0 + -(-(b * m) // cols), x0 + -(-((b + 1) * m) // cols)
        row = []
        for i in range(flat.shape[1]):
            acc = empty()
            for j in range(ja, jb):
                acc = fold(acc, unpack(flat[j, i]))
            row.append(acc)
        out.append(row)
    return pack(out).reshape((cols,) + records.shape[1:])


def wide(words):
    """a 128-bit sum as a double by the readout's rule: (double)hi * 2^64 + (double)lo"""
    w = np.asarray(words, np.uint64)
    return w[..., 1].astype(np.float64) * 2.0 ** 64 + w[..., 0].astype(np.float64)


def readout(records, pixels):
    """(mean amplitude, centroid, spread, mean flux, relative flux) in fp64 numpy, operation by operation as sgz.h orders them"""
    amp, m1, m2, fl = (wide(records[name]) for name in SUMS)
    count = records["count"].astype(np.float64)
    none = records["count"] == 0
    dark = none | ((records["amp"][..., 0] | records["amp"][..., 1]) == 0)
    with np.errstate(all="ignore"):
        mean_amp = np.where(none, np.nan, amp / (count * np.float64(pixels)) * 2.0 ** -30)
        c = np.where(dark, np.nan, m1 / amp)
        spread = np.where(dark, np.nan, np.sqrt(np.maximum(0.0, m2 / amp - c * c)))
        mean_flux = np.where(none, np.nan, fl / count * 2.0 ** -30)
        rel = np.where(dark, np.nan, fl / amp)
    return mean_amp, c, spread, mean_flux, rel


def hz(freqs, x):
    """fractional pixels into Hz by linear interpolation of the mapped frequencies (float32 [P]) in fp64"""
    f = np.asarray(freqs, np.float32).astype(np.float64)
    x = np.asarray(x, np.float64)
    P = f.size
    out = np.empty(x.shape, np.float64)
    for j, v in np.ndenumerate(x):
        if np.isnan(v):
            out[j] = v
        elif P == 1 or v <= 0:
            out[j] = f[0]
        elif v >= P - 1:
            out[j] = f[P - 1]
        else:
            i = int(np.floor(v))
            out[j] = f[i] + (v - i) * (f[i + 1] - f[i])
    return out
