"""The histogram lane's definition (sgz.h, "The histogram lane") in numpy int64 and Python integers; it shares nothing with the library.

v = (int32) clamp(rint(x 2^23), -2^26, +2^26); a NaN is skipped.  a = |v|; a = 0 is bucket 0, otherwise e = a.bit_length() - 1, s = the two bits
below the leading one (for e < 2: what there is of them, shifted up) and the bucket is 1 + 4 e + s.  One record per (column, channel): the 106
bucket counts, count, skipped, negative, peak = max a, bits_or / bits_and = OR / AND of v as a 32-bit two's complement word (0 / 0xffffffff
where nothing was counted).  The folds: add, add, add, add, max, or, and."""
import math

import numpy as np

BUCKETS = 106
DTYPE = np.dtype([("bucket", "<u4", (BUCKETS,)), ("count", "<u4"), ("skipped", "<u4"), ("negative", "<u4"), ("peak", "<u4"), ("bits_or", "<u4"),
                  ("bits_and", "<u4")])
FULL, CLAMP = 1 << 23, 1 << 26
EMPTY = (2, 3, 4, 6, 8)                                                  # the buckets that hold no integer
ALL_ONES = 0xFFFFFFFF


def identity():
    r = np.zeros((), DTYPE)
    r["bits_and"] = ALL_ONES
    return r


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


def bucket_of(a):
    """int64 [...] of 0 <= a <= 2^26 -> the bucket, by integer bit length (a binary search over the powers of two: no float takes part)"""
    a = np.asarray(a, np.int64)
    e = np.zeros(a.shape, np.int64)
    for k in range(1, 27):
        e += a >= (1 << k)                                                # floor(log2 a) for a >= 1
    s = np.where(e >= 2, (a >> np.maximum(e - 2, 0)) & 3, (a << np.maximum(2 - e, 0)) & 3)
    return np.where(a == 0, 0, 1 + 4 * e + s)


def bucket_of_int(a):
    """one Python integer, by int.bit_length"""
    if a == 0:
        return 0
    e = a.bit_length() - 1
    s = (a >> (e - 2)) & 3 if e >= 2 else (a << (2 - e)) & 3
    return 1 + 4 * e + s


def edges():
    """(lo, hi) int64 [106]: the closed form -- lo = ceil((4 + s) 2^(e-2)), hi = ceil((5 + s) 2^(e-2)) - 1, hi[105] = 2^26, bucket 0 = (0, 0)"""
    lo, hi = np.zeros(BUCKETS, np.int64), np.zeros(BUCKETS, np.int64)
    for b in range(1, BUCKETS):
        e, s = (b - 1) // 4, (b - 1) % 4
        lo[b] = math.ceil((4 + s) * 2.0 ** (e - 2))
        hi[b] = math.ceil((5 + s) * 2.0 ** (e - 2)) - 1
    hi[BUCKETS - 1] = CLAMP
    return lo, hi


def columns(x, m, held=0, flush=True, carry=None):
    """x float32 [channels][n]: a call's samples behind `held` earlier ones whose record per channel is `carry` (DTYPE [channels]) -> (records DTYPE
    [columns][channels] of the columns that close, the open column's records [channels] or None).  flush: a partial last column closes"""
    v, has = quantise(x)
    channels, n = v.shape
    total = held + n
    rest = total % m
    closed = total // m + (1 if rest and flush else 0)
    ncols = closed + (1 if rest and not flush else 0)
    out = np.zeros((ncols, channels), DTYPE)
    col = (held + np.arange(n)) // m
    for d in range(channels):
        o = out[:, d].copy()
        ok = has[d]
        vd, cd = v[d][ok], col[ok]
        a = np.abs(vd)
        o["bucket"] = np.bincount(cd * BUCKETS + bucket_of(a), minlength=ncols * BUCKETS).reshape(ncols, BUCKETS)
        o["count"] = np.bincount(cd, minlength=ncols)[:ncols]
        o["skipped"] = np.bincount(col[~ok], minlength=ncols)[:ncols]
        o["negative"] = np.bincount(cd[vd < 0], minlength=ncols)[:ncols]
        peak = np.zeros(ncols, np.int64)
        np.maximum.at(peak, cd, a)
        word = vd & ALL_ONES                                              # the 32-bit two's complement word
        bor, band = np.zeros(ncols, np.int64), np.full(ncols, ALL_ONES, np.int64)
        np.bitwise_or.at(bor, cd, word)
        np.bitwise_and.at(band, cd, word)
        o["peak"], o["bits_or"], o["bits_and"] = peak, bor, band
        out[:, d] = o
    if held and ncols:
        for d in range(channels):
            out[0, d] = add([carry[d], out[0, d]])
    if ncols > closed:
        return out[:closed], out[closed]
    return out[:closed], None


def add(records):
    """the fold of records (any shape) in Python integers -> one record, from the identity"""
    r = identity()
    recs = np.asarray(records, DTYPE).reshape(-1)
    for b in range(BUCKETS):
        r["bucket"][b] = sum(int(v) for v in recs["bucket"][:, b])
    for name in ("count", "skipped", "negative"):
        r[name] = sum(int(v) for v in recs[name])
    r["peak"] = max([int(v) for v in recs["peak"]], default=0)
    bor, band = 0, ALL_ONES
    for v, w in zip(recs["bits_or"], recs["bits_and"]):
        bor |= int(v)
        band &= int(w)
    r["bits_or"], r["bits_and"] = bor, band
    return r


def fold(records, bounds):
    """records [n][channels] -> the coarser columns [len(bounds) - 1][channels]: column b is the fold of finer columns bounds[b] <= j < bounds[b + 1]"""
    channels = records.shape[1]
    out = np.zeros((len(bounds) - 1, channels), DTYPE)
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        for d in range(channels):
            out[i, d] = add(records[a:b, d])
    return out


def view_bounds(x0, x1, out_columns):
    """the boundaries of the overview view's rule: x0 + ceil(b w / cols), b = 0 .. cols"""
    w = x1 - x0
    cols = min(out_columns, w)
    return [x0 + -(-(b * w) // cols) for b in range(cols + 1)]


def percentile(rec, q):
    """(bucket, lo, hi): r = the least integer >= q count (one fp64 multiply) clamped to [1, count]; the least b whose cumulative count reaches r"""
    count = int(rec["count"])
    r = min(max(int(math.ceil(float(q) * float(count))), 1), count)
    b = int(np.searchsorted(np.cumsum(rec["bucket"].astype(np.int64)), r))
    lo, hi = edges()
    return b, float(lo[b]) / 2.0**23, float(hi[b]) / 2.0**23


def readout(rec):
    """one record -> dict, in fp64"""
    count = int(rec["count"])
    peak = float(rec["peak"]) / 2.0**23
    bor, band = int(rec["bits_or"]), int(rec["bits_and"])
    with np.errstate(divide="ignore"):
        if count:
            median_db = 20.0 * float(np.log10(np.float64(percentile(rec, 0.5)[2])))
            peak_db = 20.0 * float(np.log10(np.float64(peak)))
        else:
            median_db = peak_db = math.nan
    ctz = (bor & -bor).bit_length() - 1
    return dict(zero_share=float(rec["bucket"][0]) / count if count else math.nan, negative_share=float(rec["negative"]) / count if count else math.nan,
                peak=peak, peak_db=peak_db, median_db=median_db, toggling=bor & ~band & ALL_ONES, effective_bits=max(0, 24 - ctz) if bor else 0)


# ---- the signal makers: float32 [S] each ------------------------------------------------------------------------------------------------------
def noise(S, seed=7):
    """0.1 N(0, 1): some 49 buckets, the fullest about a tenth of the samples"""
    return (0.1 * np.random.Generator(np.random.PCG64(seed)).standard_normal(S)).astype(np.float32)


def silence(S, seed=0):
    """+0.0 and -0.0: every sample in bucket 0"""
    x = np.zeros(S, np.float32)
    x[np.random.Generator(np.random.PCG64(seed)).integers(0, 2, S) == 1] = np.float32(-0.0)
    return x


def two_level(S, run=(1, 1)):
    """two buckets: run[0] samples of 0.25 then run[1] of -2^-10, over and over ((1, 1): in alternation; (48, 16): 48 and 16 of a wave)"""
    period = run[0] + run[1]
    return np.where(np.arange(S) % period < run[0], np.float32(0.25), np.float32(-(2.0**-10))).astype(np.float32)


def s16(S, seed=3):
    """multiples of 2^-15: a 16-bit file"""
    return (np.random.Generator(np.random.PCG64(seed)).integers(-32768, 32768, S).astype(np.float64) * 2.0**-15).astype(np.float32)


def positive(S, seed=4):
    return np.abs(noise(S, seed)) + np.float32(2.0**-20)


def reachable():
    return [b for b in range(BUCKETS) if b not in EMPTY]


def ramp(S):
    """every reachable bucket's lower edge, signs alternating, over and over: any S >= 101 of them is a column that holds every reachable bucket"""
    lo, _ = edges()
    vals = np.array([int(lo[b]) * (-1) ** i for i, b in enumerate(reachable())], np.float64) * 2.0**-23
    return np.resize(vals, S).astype(np.float32)


def edge_values(S):
    """every reachable bucket's lo and hi as +a 2^-23 and -a 2^-23, over and over.  Up to 2^24 every edge is an fp32 value and arrives as
    itself.  The eight upper edges above 2^24 are odd and no fp32 value: the cast to float32 rounds them to an even neighbour (a tie, to the
    even mantissa: the edge below or the next bucket's lower edge), which the quantiser of either side then sees alike"""
    lo, hi = edges()
    vals = []
    for b in reachable():
        for a in (int(lo[b]), int(hi[b])):
            vals += [a * 2.0**-23, -a * 2.0**-23]
    return np.resize(np.array(vals, np.float64), S).astype(np.float32)


def corners(S, seed=5):
    """noise with the corner values embedded: +-inf, NaNs alone and in a run, denormals, +-8, values either side of the clamp, full scale +- 1"""
    x = noise(S, seed)
    tiny = np.array([1, 0x807FFFFF], np.uint32).view(np.float32)
    nans = np.array([0x7FC00000, 0xFFC00001, 0x7F800001], np.uint32).view(np.float32)
    just_in, just_out = np.float32(8.0) - np.float32(2.0**-21), np.float32(8.0) + np.float32(2.0**-20)
    special = [np.inf, -np.inf, nans[0], nans[1], nans[2], tiny[0], tiny[1], 8.0, -8.0, just_in, -just_in, just_out, -just_out, 1.0, -1.0,
               1.0 + 2.0**-23, 1.0 - 2.0**-23, -1.0 - 2.0**-23, -1.0 + 2.0**-23, 0.0, -0.0, 100.0, -1e30, 0.5 * 2.0**-23, 1.5 * 2.0**-23]
    for i, v in enumerate(special * 3):
        if 17 * i + 3 < S:
            x[17 * i + 3] = v
        if S - 1 - 29 * i >= 0:
            x[S - 1 - 29 * i] = v
    if S > 3200:
        x[1500:3100] = nans[0]                                            # a run of NaNs longer than a column of up to 800 samples, and all of [2000, 3000)
    return x
