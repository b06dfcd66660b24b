"""The run lane's definition (sgz.h, "The run lane") restated; it shares nothing with the library.

Per channel: v = (int32) clamp(rint(x 2^23), -2^26, +2^26), a NaN is invalid.  P_hot(i) = valid(i) and |v[i]| >= hot, P_quiet(i) = valid(i)
and |v[i]| <= quiet, P_flat(i) = i >= 1 and valid(i) and valid(i - 1) and v[i] = v[i - 1]; cross(i) = i >= 1 and both valid and the signs
differ (zero counts as non-negative); start_k(i) = P_k(i) and not (i >= 1 and P_k(i - 1)).  One record per (column, channel) of samples
c m <= i < min((c + 1) m, S): len, skipped, crossings, and per predicate count, runs (the starts), longest / at (the longest stretch inside the
column and the least offset where one begins), head / tail (the stretches at either end).

`records` works from the DEFINITION, sample by sample: the predicates of every sample first, then every column from its samples' predicates
alone -- never from another column's record.  `loop_record` is the same in plain Python integers, for small inputs.  The FOLD (`fold_pair`,
`fold`) is written separately and is what the tests hold against the definition."""
import math

import numpy as np

OF_DTYPE = np.dtype([("count", "<u4"), ("runs", "<u4"), ("longest", "<u4"), ("at", "<u4"), ("head", "<u4"), ("tail", "<u4")])
DTYPE = np.dtype([("len", "<u4"), ("skipped", "<u4"), ("crossings", "<u4"), ("reserved0", "<u4"), ("of", OF_DTYPE, (3,)), ("reserved", "<u4", (2,))])
CARRY_DTYPE = np.dtype([("open", DTYPE), ("prev", "<i4", (2,)), ("reserved", "<u4", (2,))])
HOT, QUIET, FLAT = 0, 1, 2
NAN = -2**31
FULL, CLAMP = 1 << 23, 1 << 26
DEFAULT = (FULL - (1 << 8), 0)                  # (hot, quiet)
FIELDS = ("count", "runs", "longest", "at", "head", "tail")


def is_nan(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def quantise(x):
    """float32 [...] -> (v int64, NAN where the sample is a NaN; valid bool)"""
    x = np.ascontiguousarray(x, np.float32)
    nan = is_nan(x)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.clip(np.rint(np.where(nan, np.float32(0), x).astype(np.float64) * float(FULL)), -float(CLAMP), float(CLAMP)).astype(np.int64)
    return np.where(nan, NAN, v), ~nan


def predicates(v, params=DEFAULT, history=None):
    """v int64 [S] of one channel (NAN: invalid), history (v[-1], v[-2]) or None (none: marks) -> P bool [3][S], start bool [3][S], cross bool [S]"""
    hot, quiet = params
    h = (NAN, NAN) if history is None else (int(history[0]), int(history[1]))
    z = np.concatenate([np.array([h[1], h[0]], np.int64), np.asarray(v, np.int64)])        # z[j] = v[j - 2]
    ok = z != NAN
    a = np.abs(np.where(ok, z, 0))
    before = np.concatenate([[False], ok[:-1]])                                            # valid(i - 1); nothing lies before z[0]
    zb = np.concatenate([[0], z[:-1]])
    P = np.stack([ok & (a >= hot), ok & (a <= quiet), ok & before & (z == zb)])
    Pb = np.concatenate([np.zeros((3, 1), bool), P[:, :-1]], axis=1)                       # P_k(i - 1)
    start = P & ~Pb
    cross = ok & before & ((z < 0) != (zb < 0))
    return P[:, 2:], start[:, 2:], cross[2:]


def _stretches(p):
    """bool [n] -> (starts, lengths) of its maximal stretches of True"""
    d = np.diff(np.concatenate([[0], p.astype(np.int8), [0]]))
    s, e = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return s, e - s


def column_record(P, start, cross, valid):
    """the record of one column from its own samples' predicates (arrays over the column's samples alone)"""
    r = np.zeros((), DTYPE)
    n = int(valid.size)
    r["len"], r["skipped"], r["crossings"] = n, int((~valid).sum()), int(cross.sum())
    for k in range(3):
        if not P[k].any():
            continue
        s, l = _stretches(P[k])
        o = r["of"][k]
        o["count"], o["runs"] = int(P[k].sum()), int(start[k].sum())
        if l.size:
            best = int(l.max())
            o["longest"], o["at"] = best, int(s[np.flatnonzero(l == best)[0]])
            o["head"] = int(l[0]) if s[0] == 0 else 0
            o["tail"] = int(l[-1]) if s[-1] + l[-1] == n else 0
    return r


def records(x, m, params=DEFAULT, flush=True, history=None):
    """x float32 [channels][S] -> (records DTYPE [columns][channels], the open column's records DTYPE [channels] or None).  history: int
    [channels][2], (v[-1], v[-2]) in front of the stream, or None"""
    x = np.atleast_2d(np.ascontiguousarray(x, np.float32))
    channels, S = x.shape
    full, rest = S // m, S % m
    columns = full + (1 if rest and flush else 0)
    out = np.zeros((columns, channels), DTYPE)
    open_ = np.zeros(channels, DTYPE) if rest and not flush else None
    v, valid = quantise(x)
    for d in range(channels):
        P, start, cross = predicates(v[d], params, None if history is None else history[d])
        for c in range(columns):
            a, b = c * m, min((c + 1) * m, S)
            out[c, d] = column_record(P[:, a:b], start[:, a:b], cross[a:b], valid[d, a:b])
        if open_ is not None:
            a = full * m
            open_[d] = column_record(P[:, a:], start[:, a:], cross[a:], valid[d, a:])
    return out, open_


def history_after(x, history=None):
    """(v[S - 1], v[S - 2]) of (history, x): int32 [channels][2]"""
    v, _ = quantise(np.atleast_2d(x))
    h = np.full((v.shape[0], 2), NAN, np.int64) if history is None else np.asarray(history, np.int64)
    z = np.concatenate([h[:, ::-1], v], axis=1)
    return z[:, :-3:-1].astype(np.int32)


def carry_after(x, m, params=DEFAULT, history=None, flushed=False):
    """the sgz_run_carry [channels] behind a call that took x from a stream's (or a flush's) beginning: the open column (zeros where none is
    open or the call flushed), the history, zeros"""
    x = np.atleast_2d(np.ascontiguousarray(x, np.float32))
    c = np.zeros(x.shape[0], CARRY_DTYPE)
    _, open_ = records(x, m, params, flush=flushed, history=history)
    if open_ is not None:
        c["open"] = open_
    c["prev"] = history_after(x, history)
    return c


def loop_record(xs, params=DEFAULT, before=()):
    """the definition in plain Python for one column: xs -- its float samples, before -- the stream's samples in front of it (any number).
    Returns a dict of the record's fields, of[k] as dicts"""
    hot, quiet = params

    def q(f):
        f = float(np.float32(f))
        if math.isnan(f):
            return None
        y = f * 2.0**23
        return int(min(max(np.rint(y) if math.isfinite(y) else math.copysign(2.0**26, y), -(2.0**26)), 2.0**26))

    z = [q(f) for f in before] + [q(f) for f in xs]
    off = len(before)

    def P(k, i):
        if i < 0 or z[i] is None:
            return False
        if k == HOT:
            return abs(z[i]) >= hot
        if k == QUIET:
            return abs(z[i]) <= quiet
        return i >= 1 and z[i - 1] is not None and z[i] == z[i - 1]

    n = len(xs)
    rec = dict(len=n, skipped=sum(z[off + j] is None for j in range(n)), crossings=0, of=[])
    for j in range(n):
        i = off + j
        if i >= 1 and z[i] is not None and z[i - 1] is not None and (z[i] < 0) != (z[i - 1] < 0):
            rec["crossings"] += 1
    for k in range(3):
        p = [P(k, off + j) for j in range(n)]
        o = dict(count=sum(p), runs=sum(p[j] and not P(k, off + j - 1) for j in range(n)), longest=0, at=0, head=0, tail=0)
        while o["head"] < n and p[o["head"]]:
            o["head"] += 1
        while o["tail"] < n and p[n - 1 - o["tail"]]:
            o["tail"] += 1
        for s in range(n):                              # the greatest r with p[s : s + r] all true, the least s that attains it
            r = 0
            while s + r < n and p[s + r]:
                r += 1
            if r > o["longest"]:
                o["longest"], o["at"] = r, s
        rec["of"].append(o)
    return rec


def as_dict(r):
    """a DTYPE record -> loop_record's form"""
    return dict(len=int(r["len"]), skipped=int(r["skipped"]), crossings=int(r["crossings"]),
                of=[{f: int(r["of"][k][f]) for f in FIELDS} for k in range(3)])


# ---- the fold, written on its own ------------------------------------------------------------------------------------------------------------
def fold_pair(A, B):
    """A followed by B, both DTYPE records -> a DTYPE record"""
    r = np.zeros((), DTYPE)
    la, lb = int(A["len"]), int(B["len"])
    for f in ("len", "skipped", "crossings"):
        r[f] = int(A[f]) + int(B[f])
    for k in range(3):
        a, b = {f: int(A["of"][k][f]) for f in FIELDS}, {f: int(B["of"][k][f]) for f in FIELDS}
        o = r["of"][k]
        o["count"], o["runs"] = a["count"] + b["count"], a["runs"] + b["runs"]
        o["head"] = la + b["head"] if a["head"] == la else a["head"]
        o["tail"] = lb + a["tail"] if b["tail"] == lb else b["tail"]
        cands = [(a["longest"], a["at"]), (a["tail"] + b["head"], la - a["tail"]), (b["longest"], la + b["at"])]
        best = max(l for l, _ in cands)
        o["longest"] = best
        o["at"] = min(p for l, p in cands if l == best) if best else 0
    return r


def fold(recs, bounds):
    """records [n][channels] -> the coarser columns [len(bounds) - 1][channels], source columns folded in their order"""
    out = np.zeros((len(bounds) - 1, recs.shape[1]), DTYPE)
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        for d in range(recs.shape[1]):
            r = np.zeros((), DTYPE)
            for j in range(a, b):
                r = fold_pair(r, recs[j, d])
            out[i, d] = r
    return out


def view_bounds(x0, x1, out_columns):
    """the boundaries of the overview view's rule: x0 + ceil(b w / cols), b = 0 .. cols"""
    w = x1 - x0
    cols = min(out_columns, w)
    return [x0 + -(-(b * w) // cols) for b in range(cols + 1)]


def readout(r, rate):
    n = float(r["len"])
    nan = float("nan")
    return dict(share=tuple(float(r["of"][k]["count"]) / n if n else nan for k in range(3)),
                longest_seconds=tuple(float(r["of"][k]["longest"]) / rate for k in range(3)),
                at_seconds=tuple(float(r["of"][k]["at"]) / rate for k in range(3)),
                crossing_hz=float(r["crossings"]) * rate / (2.0 * n) if n else nan)


# ---- signals ---------------------------------------------------------------------------------------------------------------------------------
def noise(S, seed=0, scale=0.25):
    return (np.random.default_rng(seed).standard_normal(S) * scale).astype(np.float32)


def s16(S, seed=1):
    """a music-like 16-bit signal: two sines and a little noise, rounded to 16 bits"""
    t = np.arange(S, dtype=np.float64)
    y = 0.5 * np.sin(2 * np.pi * t / 97.3) + 0.3 * np.sin(2 * np.pi * t / 11.7) + 0.02 * np.random.default_rng(seed).standard_normal(S)
    return (np.clip(np.rint(y * 32768.0), -32768, 32767) / 32768.0).astype(np.float32)


def clipped(S, period=53.0, gain=1.6):
    """a hard-clipped 16-bit sine: runs on both rails"""
    y = gain * np.sin(2 * np.pi * np.arange(S, dtype=np.float64) / period)
    return (np.clip(np.rint(y * 32768.0), -32768, 32767) / 32768.0).astype(np.float32)


def busy(S, seed=0):
    """a little of everything, so that every field moves: noise in a few levels (equal neighbours are common), clipped stretches, holes of
    zeros, NaNs, infinities, values that clamp, -0.0 and denormals"""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-3, 4, S) / 8388608.0).astype(np.float32)                # |v| <= 3: flat runs and sign changes everywhere
    for _ in range(max(1, S // 40)):
        a = int(rng.integers(0, S))
        n = int(rng.integers(1, 80))
        kind = int(rng.integers(0, 6))
        x[a:a + n] = (1.0, -1.0, 0.0, np.nan, np.inf, -20.0)[kind]
    for _ in range(max(1, S // 100)):
        x[int(rng.integers(0, S))] = (np.nan, -0.0, 1e-42, -1e-42, 0.99997, -np.inf)[int(rng.integers(0, 6))]
    return x
