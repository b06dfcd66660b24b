"""The band lane's definition (sgz.h, "The band lane") in numpy; it shares nothing with the library.

v = (int32) clamp(rint(x 2^23), -2^26, +2^26), a NaN is v = 0 and is not counted.  Segment j covers samples j L <= i < (j + 1) L; its start state
is (double)(int64) sum_k C[c][k] v[j L - 1 - k] * 2^-30 with C[c][k] = rint(2^30 h[c][k]), h the 16 state components of the crossover tree's
impulse response; the sums are np.int64 (exact below 2^63).  From there the eight transposed-direct-form-II sections run in fp64, a Python
loop of L steps vectorised over the segments -- numpy does not contract.  q_b = clip(rint(z_b), +-(2^31 - 1)) for low, mid, high; one record
per (column, channel): three 128-bit sums of q_b^2 and the count of non-NaN samples.  A filter is anything with c[4][5], W and L
(api.BandFilter is one)."""
import numpy as np

DTYPE = np.dtype([("sumsq", "<u8", (3, 2)), ("count", "<u4"), ("reserved", "<u4", (3,))])
FULL, CLAMP = 1 << 23, 1 << 26
QMAX = (1 << 31) - 1
MASK64 = (1 << 64) - 1
SCALE = 30
COMPS = 16
REC_WORDS = 16


class Filter:
    def __init__(self, c, W, L):
        self.c, self.W, self.L = [[float(v) for v in r] for r in c], int(W), int(L)


def coef(f):
    return [[float(f.c[s][i]) for i in range(5)] for s in range(4)]


def hist_len(f):
    return int(f.W) + int(f.L) - 1


def carry_bytes(f):
    """per channel: the open column's record, W + L - 1 history words, a zero word"""
    return 64 + 4 * (int(f.W) + int(f.L))


def section(c, st, i, x):
    """one section on arrays (or scalars): st[i], st[i + 1] are replaced; returns y.  One operation per *, + and -."""
    y = c[0] * x + st[i]
    n0 = (c[1] * x - c[3] * y) + st[i + 1]
    n1 = c[2] * x - c[4] * y
    st[i], st[i + 1] = n0, n1
    return y


def step(c, st, x):
    """one step of the tree; st: 16 components (lp1a, lp1b, hp1a, hp1b, lp2a, lp2b, hp2a, hp2b); returns (low, mid, high)"""
    low = section(c[0], st, 2, section(c[0], st, 0, x))
    rest = section(c[1], st, 6, section(c[1], st, 4, x))
    mid = section(c[2], st, 10, section(c[2], st, 8, rest))
    high = section(c[3], st, 14, section(c[3], st, 12, rest))
    return low, mid, high


def is_pow2(v):
    return v > 0 and v & (v - 1) == 0


def taps(f):
    """int64 [16][W], or None where the definition refuses the filter"""
    W, L = int(f.W), int(f.L)
    if not (is_pow2(W) and is_pow2(L) and 16 <= L <= W <= 65536):
        return None
    c = coef(f)
    st = [0.0] * COMPS                                                  # (Python floats: IEEE doubles, one rounding per operation)
    h = np.zeros((COMPS, W), np.float64)
    for k in range(W):
        step(c, st, 1.0 if k == 0 else 0.0)
        h[:, k] = st
    with np.errstate(all="ignore"):
        t = np.rint(h * float(1 << SCALE))
    if not np.isfinite(t).all() or (t < -2147483648.0).any() or (t > 2147483647.0).any():
        return None
    t = t.astype(np.int64)
    if int(np.abs(t).sum(axis=1).max()) << 26 >= 1 << 62:
        return None
    return t


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


_tables = {}


def _table(f):
    key = (tuple(map(tuple, coef(f))), int(f.W), int(f.L))
    if key not in _tables:
        _tables[key] = taps(f)
    return _tables[key]


def q_of(v, f, first_index=0, history=None, want_z=False):
    """v int64 [S] -> q int64 [3][S] (or z float64 [3][S]).  history: the quantised samples in front of v (any length, zeros in front of
    those); first_index: the absolute index of v[0], which places the segment grid"""
    W, L, H = int(f.W), int(f.L), hist_len(f)
    C = _table(f)
    assert C is not None
    v = np.asarray(v, np.int64)
    S = len(v)
    if S == 0:
        return np.zeros((3, 0), np.float64 if want_z else np.int64)
    h = np.zeros(H, np.int64)
    if history is not None and len(history):
        hh = np.asarray(history, np.int64)[-H:]
        h[H - len(hh):] = hh
    p = first_index % L
    nseg = -(-(S + p) // L)
    ext = np.concatenate([h, v, np.zeros(L, np.int64)])                 # ext[H + r] = sample r of the call
    starts = H - p + L * np.arange(nseg)                                # ext index of every segment's first sample
    windows = np.lib.stride_tricks.sliding_window_view(ext, W)          # windows[e] = ext[e : e + W]
    state = np.zeros((COMPS, nseg), np.float64)
    Crev = np.ascontiguousarray(C[:, ::-1].T)                           # [W][16]: the window's oldest sample meets the last tap
    block = max(1, (1 << 22) // W)
    for a0 in range(0, nseg, block):
        w = windows[starts[a0:a0 + block] - W]                          # samples j L - W .. j L - 1
        state[:, a0:a0 + block] = ((w @ Crev).astype(np.float64) * 2.0 ** -SCALE).T
    c = coef(f)
    st = [state[i].copy() for i in range(COMPS)]
    z = np.zeros((3, nseg, L), np.float64)
    with np.errstate(all="ignore"):
        for s in range(L):
            z[0, :, s], z[1, :, s], z[2, :, s] = step(c, st, ext[starts + s].astype(np.float64))
    z = z.reshape(3, -1)[:, p:p + S]
    if want_z:
        return z
    return np.clip(np.rint(z), -float(QMAX), float(QMAX)).astype(np.int64)


def unsegmented_z(v, f):
    """the plain fp64 recurrence over the whole stream from rest: what the definition approximates; float64 [3][S]"""
    c = coef(f)
    st = [0.0] * COMPS
    out = np.zeros((3, len(v)), np.float64)
    for i, x in enumerate(np.asarray(v, np.float64).tolist()):
        out[0, i], out[1, i], out[2, i] = step(c, st, x)
    return out


def _records(q, has, m, flush):
    """q int64 [3][S], has bool [S] -> (three lists of python-int sums per column, counts per column)"""
    S = q.shape[1]
    full, rest = S // m, S % m
    columns = full + (1 if rest and flush else 0)
    if not columns:
        return [[], [], []], []
    used = S if flush else full * m
    edges = np.arange(columns) * m
    sums = []
    for b in range(3):
        sq = (q[b, :used] * q[b, :used]).astype(np.uint64)               # (q^2 < 2^62)
        lo = np.add.reduceat(sq & np.uint64(0xFFFFFFFF), edges)
        hi = np.add.reduceat(sq >> np.uint64(32), edges)
        sums.append([(int(h) << 32) + int(l) for l, h in zip(lo, hi)])
    counts = np.add.reduceat(has[:used].astype(np.int64), edges)
    return sums, [int(c) for c in counts]


def pack(sums, counts, out, d):
    for c, k in enumerate(counts):
        for b in range(3):
            out["sumsq"][c, d, b, 0] = sums[b][c] & MASK64
            out["sumsq"][c, d, b, 1] = sums[b][c] >> 64
        out["count"][c, d] = k


def records_of_integers(v, has, f, m, flush=True, history=None, first_index=0):
    """v int64 [channels][S], has bool [channels][S] -> (records DTYPE [columns][channels], samples left open).  history: int [channels][any] in
    front of the stream, or None"""
    channels, S = v.shape
    full, rest = S // m, S % m
    columns = full + (1 if rest and flush else 0)
    out = np.zeros((columns, channels), DTYPE)
    for d in range(channels):
        q = q_of(v[d], f, first_index, None if history is None else history[d])
        pack(*_records(q, has[d], m, flush), out, d)
    return out, (0 if flush else rest)


def records_of(x, f, m, flush=True, history=None, first_index=0):
    """x float32 [channels][S] -> (records, samples left open)"""
    return records_of_integers(*quantise(x), f, m, flush, history, first_index)


def history_after(x, f, history=None):
    """the last W + L - 1 quantised samples of (zeros, history, x): int32 [channels][W + L - 1]"""
    v, _ = quantise(x)
    H = hist_len(f)
    h = np.zeros((v.shape[0], H), np.int64)
    if history is not None:
        h = np.concatenate([h, np.asarray(history, np.int64)], axis=1)
    return np.concatenate([h, v], axis=1)[:, -H:].astype(np.int32)


def carry_of(f, open_records, history):
    """the carry as the stage call lays it out: uint32 words [channels][16 + W + L] -- the open record, the history, a zero word"""
    channels = len(history)
    words = np.zeros((channels, carry_bytes(f) // 4), np.uint32)
    words[:, :REC_WORDS] = np.ascontiguousarray(open_records, DTYPE).reshape(channels).view(np.uint32).reshape(channels, REC_WORDS)
    words[:, REC_WORDS:REC_WORDS + hist_len(f)] = np.asarray(history, np.int64).astype(np.int32).view(np.uint32).reshape(channels, -1)
    return words


def total(records):
    """python ints [n][channels][3]: the 128-bit sums"""
    return [[[(int(r["sumsq"][b][1]) << 64) | int(r["sumsq"][b][0]) for b in range(3)] for r in row] for row in records]


def fold(records, bounds):
    """records [n][channels] -> the coarser columns [len(bounds) - 1][channels]: field-wise sums"""
    out = np.zeros((len(bounds) - 1, records.shape[1]), DTYPE)
    t = total(records)
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        for d in range(records.shape[1]):
            for k in range(3):
                s = sum(t[j][d][k] for j in range(a, b))
                out["sumsq"][i, d, k, 0], out["sumsq"][i, d, k, 1] = s & MASK64, s >> 64
        out["count"][i] = records["count"][a:b].astype(np.uint64).sum(axis=0)
    return out


def view_bounds(x0, x1, out_columns):
    """the boundaries of the overview view's rule: x0 + ceil(b w / cols), b = 0 .. cols"""
    w = x1 - x0
    cols = min(out_columns, w)
    return [x0 + -(-(b * w) // cols) for b in range(cols + 1)]


def mean_squares(records, channel):
    """records [ncols][channels] of one channel read together -> fractions.Fraction [3] (0 without samples)"""
    from fractions import Fraction
    t = total(records)
    count = int(records["count"][:, channel].astype(np.uint64).sum())
    return [Fraction(sum(row[channel][b] for row in t), count << 46) if count else Fraction(0) for b in range(3)]


# a tiny stable crossover for W = 64, L = 16: every pole has radius 0.4 or 0.5, so the state after 64 steps is far below 2^-30 of an impulse;
# every state component of the impulse response stays below 2, as a tap at 2^30 in int32 needs
TINY = Filter(c=[[0.25, 0.5, 0.25, -0.4, 0.16], [0.5, -1.0, 0.5, -0.4, 0.16], [0.3, 0.6, 0.3, 0.3, 0.25], [0.6, -0.9, 0.35, 0.3, 0.25]], W=64, L=16)
