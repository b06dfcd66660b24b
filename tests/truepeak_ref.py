"""The true-peak lane's definition (sgz.h, "The true-peak lane") in numpy int64; it shares nothing with the library.

v = (int32) clamp(rint(x 2^23), -2^26, +2^26), a NaN is v = 0 and is not counted.  y[i][q] = sum_j c[q][j] v[i - j] with v[k] = 0 for k < 0 (or
the `history` in front of the stream), c[q][j] = rint(2^20 L(j - 6 + q / 4)), L(t) = sinc(t) sinc(t / 6) for |t| < 6 -- computed here from the
formula in fp64, not copied.  One record per (column, channel) of samples c m <= i < min((c + 1) m, S): peak = max |y[i][q]|, count = the
non-NaN samples, overs = the samples with |y[i][q]| >= 2^43 for some q.  |y| < 2^47: every sum is exact in int64."""
import numpy as np

DTYPE = np.dtype([("peak", "<u8"), ("count", "<u4"), ("overs", "<u4")])
CARRY_DTYPE = np.dtype([("open", DTYPE), ("hist", "<i4", (11,)), ("reserved", "<u4")])
FULL, CLAMP = 1 << 23, 1 << 26
TAPS, PHASES, SCALE = 12, 4, 1 << 20
FULL_SCALE = FULL * SCALE                  # 2^43


def lanczos(t):
    t = np.asarray(t, np.float64)
    return np.where(np.abs(t) < 6.0, np.sinc(t) * np.sinc(t / 6.0), 0.0)


def table():
    """int64 [4][12]: c[q][j] = rint(2^20 L(j - 6 + q / 4))"""
    q = np.arange(PHASES, dtype=np.float64)[:, None]
    j = np.arange(TAPS, dtype=np.float64)[None, :]
    return np.rint(float(SCALE) * lanczos(j - 6.0 + q / 4.0)).astype(np.int64)


C = table()


def is_nan(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def quantise(x):
    """float32 [...] -> (v int64 with 0 for a NaN, has bool)"""
    x = np.ascontiguousarray(x, np.float32)
    nan = is_nan(x)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.clip(np.rint(np.where(nan, np.float32(0), x).astype(np.float64) * float(FULL)), -float(CLAMP), float(CLAMP))
    return v.astype(np.int64), ~nan


def outputs(v, history=None):
    """v int64 [S] -> |y| int64 [S][4]: np.convolve per phase on the stream behind its history (11 samples, oldest first; default zeros)"""
    h = np.zeros(TAPS - 1, np.int64) if history is None else np.asarray(history, np.int64)
    z = np.concatenate([h, np.asarray(v, np.int64)])
    y = np.stack([np.convolve(z, C[q])[TAPS - 1:TAPS - 1 + len(v)] for q in range(PHASES)], axis=1) if len(v) else np.zeros((0, PHASES), np.int64)
    return np.abs(y)


def records_of_integers(v, has, m, flush=True, history=None):
    """v int64 [channels][S] (0 where has is False), has bool [channels][S] -> (records DTYPE [columns][channels], samples left open).
    history: int [channels][11] in front of the stream, or None"""
    channels, S = v.shape
    full, rest = S // m, S % m
    columns = full + (1 if rest and flush else 0)
    out = np.zeros((columns, channels), DTYPE)
    for d in range(channels):
        p = outputs(v[d], None if history is None else history[d]).max(axis=1) if S else np.zeros(0, np.int64)
        edges = np.arange(columns) * m
        if columns:
            out["peak"][:, d] = np.maximum.reduceat(p, edges).astype(np.uint64) if S else 0
            out["count"][:, d] = np.add.reduceat(has[d].astype(np.int64), edges)
            out["overs"][:, d] = np.add.reduceat((p >= FULL_SCALE).astype(np.int64), edges)
        if not flush and rest and columns:                          # reduceat's last segment ran to the end: cut the open samples off
            a, b = (columns - 1) * m, columns * m
            out["peak"][-1, d] = p[a:b].max()
            out["count"][-1, d] = has[d, a:b].sum()
            out["overs"][-1, d] = (p[a:b] >= FULL_SCALE).sum()
    return out, (0 if flush else rest)


def records_of(x, m, flush=True, history=None):
    """x float32 [channels][S] -> (records, samples left open)"""
    return records_of_integers(*quantise(x), m, flush, history)


def history_after(x, history=None):
    """the last 11 quantised samples of (history, x): int32 [channels][11]"""
    v, _ = quantise(x)
    h = np.zeros((v.shape[0], TAPS - 1), np.int64) if history is None else np.asarray(history, np.int64)
    return np.concatenate([h, v], axis=1)[:, -(TAPS - 1):].astype(np.int32)


def fold(records, bounds):
    """records [n][channels] -> the coarser columns [len(bounds) - 1][channels]: max of peak, sums of count and overs"""
    out = np.zeros((len(bounds) - 1, records.shape[1]), DTYPE)
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        out["peak"][i] = records["peak"][a:b].max(axis=0)
        out["count"][i] = records["count"][a:b].astype(np.uint64).sum(axis=0)
        out["overs"][i] = records["overs"][a:b].astype(np.uint64).sum(axis=0)
    return out


def view_bounds(x0, x1, out_columns):
    """the boundaries of the overview view's rule: x0 + ceil(b w / cols), b = 0 .. cols"""
    w = x1 - x0
    cols = min(out_columns, w)
    return [x0 + -(-(b * w) // cols) for b in range(cols + 1)]


def saturated(channels, S, seed):
    """float32 [channels][S]: nothing but +-inf and +-100, all of which quantise to +-2^26; the first 12 samples of channel 0 take the signs of
    phase 2's taps, so |y| reaches the bound 2^26 * 2073548 at sample 11"""
    rng = np.random.default_rng(seed)
    values = np.array([np.inf, -np.inf, 100.0, -100.0], np.float32)
    x = values[rng.integers(0, 4, size=(channels, S))]
    n = min(S, TAPS)
    if n == TAPS:
        x[0, :TAPS] = np.where(C[2][::-1] < 0, np.float32(-100.0), np.float32(np.inf))     # v[11 - j] has the sign of c[2][j]
    return x
