"""The percentile overview restated in numpy (sgz.h, "The percentile overview"): bucket, record, fold and quantile from the definition's
text.  It shares no code with the library: the bucket is computed in float64 from the inequalities (64 x is exact there as well), the fold is
np.add on uint64, the quantile is the cumulative-count rule in float64, whose operations round to nearest even as the definition asks."""
import numpy as np

BUCKETS, MAX_Q = 66, 8
DTYPE = np.dtype({"names": ["bucket", "nans", "reserved"], "formats": [("<u4", (BUCKETS,)), "<u4", "<u4"], "offsets": [0, 264, 268], "itemsize": 272})
WORDS = 68
NAN_BITS = np.uint32(0x7FC00000)


def bucket_of(x: np.ndarray) -> np.ndarray:
    """int64 buckets of float32 values; -1 for a NaN.  x < 0 -> 0 (-0 is not below 0), x >= 1 -> 65, else 1 + floor(64 x)"""
    x = np.asarray(x, np.float32)
    d = x.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        inner = 1 + np.floor(64.0 * np.where((d >= 0) & (d < 1), d, 0.0)).astype(np.int64)
        b = np.where(d < 0, 0, np.where(d >= 1, BUCKETS - 1, inner))
    return np.where(np.isnan(d), -1, b)


def empty(shape) -> np.ndarray:
    return np.zeros(shape, DTYPE)


def records_of(x: np.ndarray) -> np.ndarray:
    """one record per value of x (a column of one frame)"""
    b = bucket_of(x)
    r = empty(b.shape)
    flat, fb = r.reshape(-1), b.reshape(-1)
    ok = fb >= 0
    flat["bucket"][np.nonzero(ok)[0], fb[ok]] = 1
    flat["nans"][~ok] = 1
    return r


def fold(records: np.ndarray, axis: int = 0) -> np.ndarray:
    """every word adds; a word above 2^32 - 1 is an error"""
    records = np.asarray(records, DTYPE)
    out = empty(np.delete(records.shape, axis))
    for name in ("bucket", "nans"):
        total = records[name].astype(np.uint64).sum(axis=axis, dtype=np.uint64)
        if (total > 0xFFFFFFFF).any():
            raise OverflowError(name)
        out[name] = total
    return out


def columns_of(x: np.ndarray, k: int, held: int = 0, carry=None, flush: bool = True):
    """x [frames][...] behind `held` frames whose record is `carry` -> (records of the closed columns [columns][...], the open column's
    record or None, frames left open) -- the counting of sgz_overview_step"""
    frames = x.shape[0]
    per = records_of(x)
    t = held + frames
    closed = t // k + (1 if flush and t % k else 0)
    cols = []
    for c in range(closed):
        a, b = max(c * k - held, 0), min((c + 1) * k - held, frames)
        parts = [per[a:b]] if b > a else []
        if c == 0 and held:
            parts.append(np.asarray(carry, DTYPE)[None])
        cols.append(fold(np.concatenate(parts), 0) if parts else empty(x.shape[1:]))
    left = 0 if flush else t % k
    open_rec = None
    if left:
        a = max(closed * k - held, 0)
        parts = [per[a:]]
        if closed == 0 and held:
            parts.append(np.asarray(carry, DTYPE)[None])
        open_rec = fold(np.concatenate(parts), 0)
    out = np.stack(cols) if cols else empty((0, *x.shape[1:]))
    return out, open_rec, left


def view_of(records: np.ndarray, x0: int, x1: int, out_columns: int) -> np.ndarray:
    """the boundary rule of sgz_overview_view_columns: output column b folds source columns x0 + ceil(b m / cols) .. x0 + ceil((b + 1) m / cols)"""
    m = x1 - x0
    cols = min(out_columns, m)
    return np.stack([fold(records[x0 + -(-b * m // cols):x0 + -(-(b + 1) * m // cols)], 0) for b in range(cols)])


def quantile_bits(records: np.ndarray, q) -> np.ndarray:
    """uint32 bit patterns [nq][...] of the quantiles q of every record"""
    records = np.asarray(records, DTYPE)
    qs = np.atleast_1d(np.asarray(q, np.float64))
    flat = records.reshape(-1)
    out = np.empty((qs.size, flat.size), np.uint32)
    buckets = flat["bucket"].astype(np.int64)
    cum = np.cumsum(buckets, axis=1)
    count = cum[:, -1] if flat.size else np.zeros(0, np.int64)
    rows = np.arange(flat.size)
    some = count > 0
    for j, qj in enumerate(qs):
        r = np.clip(np.ceil(np.float64(qj) * count.astype(np.float64)), 1.0, np.maximum(count, 1).astype(np.float64)).astype(np.int64)
        b = (cum < r[:, None]).sum(axis=1)                                   # the least bucket whose cumulative count is >= r
        b = np.minimum(b, BUCKETS - 1)                                       # (count == 0: no such bucket; masked below)
        before = np.where(b > 0, cum[rows, np.maximum(b - 1, 0)], 0)
        inside = ((r - before).astype(np.float64) - 0.5) / np.maximum(buckets[rows, b], 1).astype(np.float64)
        v = ((b - 1).astype(np.float64) + inside) * np.float64(2.0 ** -6)
        v = np.where(b == 0, -2.0 ** -6, np.where(b == BUCKETS - 1, 1.0, v)).astype(np.float32)
        out[j] = np.where(some, v.view(np.uint32), NAN_BITS)
    return out.reshape(qs.size, *records.shape)


def same(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a, DTYPE), np.ascontiguousarray(b, DTYPE)
    return a.shape == b.shape and a.tobytes() == b.tobytes()
