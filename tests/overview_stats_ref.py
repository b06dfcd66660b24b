"""The mean overview's definition (include/sgz.h, "The mean overview") restated in numpy, for tests/test_overview_stats_host.py (which checks
this restatement against a brute-force Python loop and the host helpers against it) and the GPU tests (which hold the kernels to it):
  q      = rint((double)x 2^20), ties to even, clamped to +-(2^31 - 1); a NaN takes no part and is counted;
  record = (sum of q, count, nans, lo, hi) per (column, pair, pixel); lo / hi under the overview's total order (tests/overview_ref.py),
           0x7FC00000 when count == 0;
  fold   = field-wise: sums and counts add, lo the least of the los, hi the greatest of the his;
  mean   = (float)(((double)sum / (double)count) 2^-20), 0x7FC00000 when count == 0;
  pixel  = oracle.pyoracle.blend_column of the pairs' means.
Everything is compared as bytes or bit patterns."""
import numpy as np

import overview_ref as ov

DTYPE = np.dtype({"names": ["sum", "count", "nans", "lo", "hi"], "formats": ["<i8", "<u4", "<u4", "<f4", "<f4"], "offsets": [0, 8, 12, 16, 20],
                  "itemsize": 24})
Q_MOST = 2 ** 31 - 1
COUNT_MOST = 2 ** 32 - 1


def quantise(x: np.ndarray):
    """float32 -> (q int64, NaN mask); q of a NaN is 0"""
    x = np.ascontiguousarray(x, np.float32)
    nan = np.isnan(x)
    t = np.where(nan, 0.0, x.astype(np.float64)) * 2.0 ** 20                # exact: a power of two; +-inf stays +-inf
    q = np.where(t >= Q_MOST, float(Q_MOST), np.where(t <= -Q_MOST, float(-Q_MOST), np.rint(t)))
    return q.astype(np.int64), nan


def records_of(x: np.ndarray) -> np.ndarray:
    """the record of every single value: what a column of one frame holds"""
    x = np.ascontiguousarray(x, np.float32)
    q, nan = quantise(x)
    r = np.zeros(x.shape, DTYPE)
    r["sum"], r["count"], r["nans"] = q, ~nan, nan
    bits = np.where(nan, ov.QUIET_NAN, x.view(np.uint32)).astype(np.uint32)
    r["lo"] = bits.view(np.float32)
    r["hi"] = bits.view(np.float32)
    return r


def empty(shape) -> np.ndarray:
    r = np.zeros(shape, DTYPE)
    r["lo"] = r["hi"] = np.full(shape, ov.QUIET_NAN, np.uint32).view(np.float32)
    return r


def fold(records: np.ndarray, axis: int = 0) -> np.ndarray:
    """field-wise fold along `axis`; a count or nans above 2^32 - 1 raises OverflowError"""
    records = np.asarray(records, DTYPE)
    count = records["count"].astype(np.uint64).sum(axis=axis)
    nans = records["nans"].astype(np.uint64).sum(axis=axis)
    if (count > COUNT_MOST).any() or (nans > COUNT_MOST).any():
        raise OverflowError("a folded column counts more than 2^32 - 1 frames")
    out = np.zeros(count.shape, DTYPE)
    out["sum"] = records["sum"].sum(axis=axis, dtype=np.int64)
    out["count"], out["nans"] = count, nans
    shape = records.shape
    hi = ov.order_key(records["hi"]).reshape(shape).max(axis=axis, initial=0)
    lo = ((ov.order_key(records["lo"]).reshape(shape).astype(np.int64) - 1) & 0xFFFFFFFF).min(axis=axis, initial=0xFFFFFFFF)  # key - 1: a NaN's wraps to "none"
    out["hi"] = ov.key_value(hi).view(np.float32)
    out["lo"] = ov.key_value(((lo + 1) & 0xFFFFFFFF).astype(np.uint32)).view(np.float32)
    return out


def columns_of(x: np.ndarray, k: int, held: int = 0, carry=None, flush: bool = True):
    """x: float32 [frames][pairs][P], graph 0's first components.  -> (records [columns][pairs][P], the open column's records [pairs][P] or
    None, frames left open); `carry` (records [pairs][P]) stands for the `held` frames in front of x"""
    frames = x.shape[0]
    each = records_of(x)
    t = held + frames
    closed = t // k + (1 if flush and t % k else 0)

    def column(c):
        a, b = max(c * k - held, 0), min((c + 1) * k - held, frames)
        parts = each[a:max(a, b)]
        if c == 0 and held:
            parts = np.concatenate([np.asarray(carry, DTYPE).reshape(1, *x.shape[1:]), parts])
        return fold(parts, axis=0) if parts.shape[0] else empty(x.shape[1:])

    out = [column(c) for c in range(closed)]
    v = np.stack(out) if out else np.zeros((0, *x.shape[1:]), DTYPE)
    if not flush and t % k:
        return v, column(closed), t % k
    return v, None, 0


def view_of(records: np.ndarray, x0: int, x1: int, out_columns: int) -> np.ndarray:
    """the view of kept records [n][...]: column b = the fold of source columns x0 + ceil(b m / cols) .. x0 + ceil((b + 1) m / cols)"""
    m = x1 - x0
    cols = min(out_columns, m)
    return np.stack([fold(records[x0 + -(-b * m // cols):x0 + -(-(b + 1) * m // cols)], axis=0) for b in range(cols)])


def mean_bits(records: np.ndarray) -> np.ndarray:
    """uint32 bit patterns of the means"""
    records = np.asarray(records, DTYPE)
    count = records["count"]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = ((records["sum"].astype(np.float64) / count.astype(np.float64)) * 2.0 ** -20).astype(np.float32)
    return np.where(count == 0, ov.QUIET_NAN, mean.view(np.uint32)).astype(np.uint32)


def blend(po, params, records: np.ndarray) -> np.ndarray:
    """RGBA8 [columns][P][4] of records [columns][pairs][P]: the oracle's colour stage at the means"""
    return ov.blend(po, params, mean_bits(records))


def same(a: np.ndarray, b: np.ndarray) -> bool:
    """records equal byte for byte"""
    a, b = np.ascontiguousarray(a, DTYPE), np.ascontiguousarray(b, DTYPE)
    return a.shape == b.shape and a.tobytes() == b.tobytes()
