"""The level lane's definition (sgz.h, "The level lane") in numpy and Python integers; it shares nothing with the library.

v = (int32) clamp(rint(x 2^23), -2^26, +2^26), a NaN takes no part.  One record per (column, pair) of samples c m <= i < min((c + 1) m, S) of
channels (2p, 2p + 1): sumsq (unsigned 128-bit as lo, hi), cross (128-bit two's complement as lo, hi; frames where neither side is a NaN),
sum, count, overs (|v| >= 2^23).  Sums of up to 1024 terms are taken in int64 (a term is at most 2^52), everything longer in Python integers."""
import numpy as np

DTYPE = np.dtype([("sumsq", "<u8", (2, 2)), ("cross", "<u8", (2,)), ("sum", "<i8", (2,)), ("count", "<u4", (2,)), ("overs", "<u4", (2,))])
FULL, CLAMP = 1 << 23, 1 << 26
BLOCK = 1024                               # terms an int64 takes: 1024 x 2^52 = 2^62
M64, M128 = (1 << 64) - 1, (1 << 128) - 1


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


def _words(value):
    """a Python integer -> (lo, hi) of its 128-bit two's complement"""
    value &= M128
    return value & M64, value >> 64


def pack(sq, cross, sums, count, overs):
    """Python integers -> one record"""
    r = np.zeros((), DTYPE)
    for c in range(2):
        r["sumsq"][c] = _words(sq[c])
        r["sum"][c] = sums[c]
        r["count"][c] = count[c]
        r["overs"][c] = overs[c]
    r["cross"] = _words(cross)
    return r


def unpack(r):
    """one record -> dict of Python integers (cross signed)"""
    cross = int(r["cross"][0]) | int(r["cross"][1]) << 64
    return dict(sq=[int(r["sumsq"][c][0]) | int(r["sumsq"][c][1]) << 64 for c in range(2)], cross=cross - (1 << 128) if cross >> 127 else cross,
                sum=[int(v) for v in r["sum"]], count=[int(v) for v in r["count"]], overs=[int(v) for v in r["overs"]])


def _total(a):
    """the exact sum of an int64 array whose elements are at most 2^52 in magnitude"""
    if a.size <= BLOCK:
        return int(a.sum())
    return sum(int(v) for v in np.add.reduceat(a, np.arange(0, a.size, BLOCK)))


def column_of(vl, hl, vr, hr):
    """the record of one column of one pair from quantised samples"""
    return pack([_total(vl * vl), _total(vr * vr)], _total(vl * vr), [_total(vl), _total(vr)], [int(hl.sum()), int(hr.sum())],
                [int((np.abs(vl) >= FULL).sum()), int((np.abs(vr) >= FULL).sum())])


def records_of(x, m, flush=True):
    """x float32 [2 pairs][S] -> (records DTYPE [columns][pairs], samples left open).  flush: a partial last column is emitted."""
    return records_of_integers(*quantise(x), m, flush)


def records_of_integers(v, has, m, flush=True):
    """the same from quantised samples: v int64 [2 pairs][S] (0 where has is False), has bool [2 pairs][S]"""
    pairs, S = v.shape[0] // 2, v.shape[1]
    full, rest = S // m, S % m
    columns = full + (1 if rest and flush else 0)
    out = np.zeros((columns, pairs), DTYPE)
    for p in range(pairs):
        vl, vr, hl, hr = v[2 * p], v[2 * p + 1], has[2 * p], has[2 * p + 1]
        if m <= BLOCK and full:                                    # every sum of a column fits an int64: all columns at once
            L, R = vl[:full * m].reshape(full, m), vr[:full * m].reshape(full, m)
            o = out[:full, p]
            for c, (a, h) in enumerate(((L, hl), (R, hr))):
                o["sumsq"][:, c, 0] = (a * a).sum(axis=1).astype(np.uint64)
                o["sum"][:, c] = a.sum(axis=1)
                o["count"][:, c] = h[:full * m].reshape(full, m).sum(axis=1)
                o["overs"][:, c] = (np.abs(a) >= FULL).sum(axis=1)
            cross = (L * R).sum(axis=1)
            o["cross"][:, 0] = cross.view(np.uint64)
            o["cross"][:, 1] = np.where(cross < 0, np.uint64(M64), np.uint64(0))
            out[:full, p] = o
            first = full
        else:
            first = 0
        for c in range(first, columns):
            a, b = c * m, min((c + 1) * m, S)
            out[c, p] = column_of(vl[a:b], hl[a:b], vr[a:b], hr[a:b])
    return out, (0 if flush else rest)


def add(records):
    """the field-wise sum of records (any shape) in Python integers -> one record"""
    sq, cross, sums, count, overs = [0, 0], 0, [0, 0], [0, 0], [0, 0]
    for r in np.asarray(records, DTYPE).reshape(-1):
        u = unpack(r)
        cross += u["cross"]
        for c in range(2):
            sq[c] += u["sq"][c]
            sums[c] += u["sum"][c]
            count[c] += u["count"][c]
            overs[c] += u["overs"][c]
    return pack(sq, cross, sums, count, overs)


def fold(records, bounds):
    """records [n][pairs] -> the coarser columns [len(bounds) - 1][pairs]: column b is the sum of finer columns bounds[b] <= j < bounds[b + 1]"""
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


def saturated(channels, S, seed):
    """float32 [channels][S]: nothing but +-inf and +-100, all of which quantise to +-2^26 -- a 1024-sample column's sum of squares is 2^62, a
    longer one's carries into the high word; the odd channel of a pair follows the even one's signs in the first half of the samples and
    opposes them in the second, so the cross term reaches both ends"""
    rng = np.random.default_rng(seed)
    values = np.array([np.inf, -np.inf, 100.0, -100.0], np.float32)
    x = values[rng.integers(0, 4, size=(channels, S))]
    for d in range(1, channels, 2):
        mag = values[rng.integers(0, 2, size=S) * 2]               # +inf or +100
        sign = np.sign(x[d - 1]) * np.where(np.arange(S) < S // 2, 1, -1)
        x[d] = (mag * sign).astype(np.float32)
    return x
