"""The loudness lane's definition (sgz.h, "The loudness lane") in numpy; it shares nothing with the library.

v = (int32) clamp(rint(x 2^23), -2^26, +2^26), a NaN is v = 0 and is not counted.  Segment j covers samples j L <= i < (j + 1) L; its start state
is (double)(int64) sum_k C[c][k] v[j L - 1 - k] * 2^-32 with C[c][k] = rint(2^32 h[c][k]), h the four state components of the impulse response;
the sums are np.int64 (exact below 2^63).  From there the transposed-direct-form-II step runs in fp64, a Python loop of L steps vectorised over
the segments -- numpy does not contract.  q = clip(rint(z), +-(2^31 - 1)); one record per (column, channel): the 128-bit sum of q^2 and the
count of non-NaN samples.  A filter is anything with b[2][3], a[2][2], W and L (api.LoudnessFilter is one)."""
import numpy as np

DTYPE = np.dtype([("sumsq", "<u8", (2,)), ("count", "<u4"), ("reserved", "<u4", (3,))])
FULL, CLAMP = 1 << 23, 1 << 26
QMAX = (1 << 31) - 1
MASK64 = (1 << 64) - 1


class Filter:
    def __init__(self, b, a, W, L):
        self.b, self.a, self.W, self.L = [[float(v) for v in r] for r in b], [[float(v) for v in r] for r in a], int(W), int(L)


def coef(f):
    return ([[float(f.b[s][i]) for i in range(3)] for s in range(2)], [[float(f.a[s][i]) for i in range(2)] for s in range(2)])


def hist_len(f):
    return int(f.W) + int(f.L) - 1


def carry_bytes(f):
    """per channel: the open column's record, W + L - 1 history words, a zero word"""
    return 32 + 4 * (int(f.W) + int(f.L))


def step(b, a, st, x):
    """one step of both biquads on arrays (or scalars); st = [s1, s2, t1, t2] is replaced; returns z.  One operation per *, + and -."""
    s1, s2, t1, t2 = st
    y = b[0][0] * x + s1
    n1 = (b[0][1] * x - a[0][0] * y) + s2
    n2 = b[0][2] * x - a[0][1] * y
    z = b[1][0] * y + t1
    m1 = (b[1][1] * y - a[1][0] * z) + t2
    m2 = b[1][2] * y - a[1][1] * z
    st[0], st[1], st[2], st[3] = n1, n2, m1, m2
    return z


def is_pow2(v):
    return v > 0 and v & (v - 1) == 0


def taps(f):
    """int64 [4][W], or None where the definition refuses the filter"""
    W, L = int(f.W), int(f.L)
    if not (is_pow2(W) and is_pow2(L) and 16 <= L <= W <= 65536):
        return None
    b, a = coef(f)
    st = [0.0, 0.0, 0.0, 0.0]
    h = np.zeros((4, W), np.float64)
    with np.errstate(all="ignore"):
        for k in range(W):
            step(b, a, st, np.float64(1.0 if k == 0 else 0.0))
            h[:, k] = st
        t = np.rint(h * 4294967296.0)
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
    key = (tuple(map(tuple, coef(f)[0])), tuple(map(tuple, coef(f)[1])), int(f.W), int(f.L))
    if key not in _tables:
        _tables[key] = taps(f)
    return _tables[key]


def q_of(v, f, first_index=0, history=None, want_z=False):
    """v int64 [S] -> q int64 [S] (or z float64 [S]).  history: the quantised samples in front of v (any length, zeros in front of those);
    first_index: the absolute index of v[0], which places the segment grid"""
    W, L, H = int(f.W), int(f.L), hist_len(f)
    C = _table(f)
    assert C is not None
    v = np.asarray(v, np.int64)
    S = len(v)
    if S == 0:
        return np.zeros(0, np.float64 if want_z else np.int64)
    h = np.zeros(H, np.int64)
    if history is not None and len(history):
        hh = np.asarray(history, np.int64)[-H:]
        h[H - len(hh):] = hh
    p = first_index % L
    nseg = -(-(S + p) // L)
    ext = np.concatenate([h, v, np.zeros(L, np.int64)])                 # ext[H + r] = sample r of the call
    starts = H - p + L * np.arange(nseg)                                # ext index of every segment's first sample
    windows = np.lib.stride_tricks.sliding_window_view(ext, W)          # windows[e] = ext[e : e + W]
    state = np.zeros((4, nseg), np.float64)
    Crev = np.ascontiguousarray(C[:, ::-1].T)                           # [W][4]: the window's oldest sample meets the last tap
    for a0 in range(0, nseg, 512):
        w = windows[starts[a0:a0 + 512] - W]                            # samples j L - W .. j L - 1
        state[:, a0:a0 + 512] = ((w @ Crev).astype(np.float64) * 2.0 ** -32).T
    b, a = coef(f)
    st = [state[0].copy(), state[1].copy(), state[2].copy(), state[3].copy()]
    z = np.zeros((nseg, L), np.float64)
    with np.errstate(all="ignore"):
        for s in range(L):
            z[:, s] = step(b, a, st, ext[starts + s].astype(np.float64))
    z = z.reshape(-1)[p:p + S]
    if want_z:
        return z
    return np.clip(np.rint(z), -float(QMAX), float(QMAX)).astype(np.int64)


def unsegmented_z(v, f):
    """the plain fp64 recurrence over the whole stream from rest: what the definition approximates"""
    b, a = coef(f)
    st = [0.0, 0.0, 0.0, 0.0]
    out = np.zeros(len(v), np.float64)
    for i, x in enumerate(np.asarray(v, np.float64).tolist()):
        out[i] = step(b, a, st, x)
    return out


def _records(q, has, m, flush):
    """q int64 [S], has bool [S] -> (sumsq python ints per column, counts per column)"""
    S = len(q)
    full, rest = S // m, S % m
    columns = full + (1 if rest and flush else 0)
    if not columns:
        return [], []
    used = S if flush else full * m
    sq = (q[:used] * q[:used]).astype(np.uint64)                          # (q^2 < 2^62)
    edges = np.arange(columns) * m
    lo = np.add.reduceat(sq & np.uint64(0xFFFFFFFF), edges)
    hi = np.add.reduceat(sq >> np.uint64(32), edges)
    counts = np.add.reduceat(has[:used].astype(np.int64), edges)
    return [(int(h) << 32) + int(l) for l, h in zip(lo, hi)], [int(c) for c in counts]


def pack(sums, counts, out, d):
    for c, (s, k) in enumerate(zip(sums, counts)):
        out["sumsq"][c, d, 0] = s & MASK64
        out["sumsq"][c, d, 1] = s >> 64
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
    """the carry as the stage call lays it out: uint32 words [channels][8 + W + L] -- the open record, the history, a zero word"""
    channels = len(history)
    words = np.zeros((channels, carry_bytes(f) // 4), np.uint32)
    words[:, :8] = np.ascontiguousarray(open_records, DTYPE).reshape(channels).view(np.uint32).reshape(channels, 8)
    words[:, 8:8 + hist_len(f)] = np.asarray(history, np.int64).astype(np.int32).view(np.uint32).reshape(channels, -1)
    return words


def total(records):
    """python ints [n][channels]: the 128-bit sums"""
    return [[(int(r["sumsq"][1]) << 64) | int(r["sumsq"][0]) for r in row] for row in records]


def fold(records, bounds):
    """records [n][channels] -> the coarser columns [len(bounds) - 1][channels]: field-wise sums"""
    out = np.zeros((len(bounds) - 1, records.shape[1]), DTYPE)
    t = total(records)
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        for d in range(records.shape[1]):
            s = sum(t[j][d] for j in range(a, b))
            out["sumsq"][i, d, 0], out["sumsq"][i, d, 1] = s & MASK64, s >> 64
        out["count"][i] = records["count"][a:b].astype(np.uint64).sum(axis=0)
    return out


def view_bounds(x0, x1, out_columns):
    """the boundaries of the overview view's rule: x0 + ceil(b w / cols), b = 0 .. cols"""
    w = x1 - x0
    cols = min(out_columns, w)
    return [x0 + -(-(b * w) // cols) for b in range(cols + 1)]


def mean_square(records, weights=None):
    """records [ncols][channels] read together -> sum_c G_c ms_c"""
    t = total(records)
    z = 0.0
    for d in range(records.shape[1]):
        count = int(records["count"][:, d].astype(np.uint64).sum())
        if count:
            z += (1.0 if weights is None else float(weights[d])) * (float(sum(row[d] for row in t)) / count / 2.0 ** 46)
    return z


def lufs(z):
    return -0.691 + 10.0 * np.log10(z) if z > 0.0 else -np.inf


def integrated(records, weights=None):
    n = records.shape[0]
    if n < 4:
        return -np.inf
    z = np.array([mean_square(records[i:i + 4], weights) for i in range(n - 3)])
    l = np.array([lufs(v) for v in z])
    keep = l > -70.0
    if not keep.any():
        return -np.inf
    gate = lufs(z[keep].mean()) - 10.0
    keep &= l > gate
    return lufs(z[keep].mean()) if keep.any() else -np.inf


# a tiny stable filter for W = 64, L = 16: poles of radius 0.5 and 0.6, so the state after 64 steps is below 2^-32 of an impulse; every state
# component of the impulse response stays below 0.5, as a tap at 2^32 in int32 needs
TINY = Filter(b=[[0.25, -0.1, 0.05], [0.5, -0.3, 0.1]], a=[[-0.5, 0.25], [-0.6, 0.36]], W=64, L=16)
