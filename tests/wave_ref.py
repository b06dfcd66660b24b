"""The waveform lane's definition (sgz.h, "The waveform lane") in numpy; it shares nothing with the library.

Wv[c][d] = (lo, hi) of samples c m <= i < min((c + 1) m, S) of channel d: the least and the greatest non-NaN sample under the total order
key(bits) = bits ^ (sign ? 0xFFFFFFFF : 0x80000000), compared as unsigned; a column of NaNs alone gives 0x7FC00000 twice.  Everything
here works on uint32 bit patterns."""
import numpy as np

QNAN = np.uint32(0x7FC00000)
NO_MIN = np.uint32(0xFFFFFFFF)          # the key of no value: the minimum's identity
NO_MAX = np.uint32(0)                   # a NaN pattern's key and nothing else's: the maximum's identity


def bits_of(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def is_nan(bits):
    return (bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def key_of(bits):
    """the order key of non-NaN bit patterns (meaningless for NaNs: mask them with is_nan)"""
    bits = np.asarray(bits, np.uint32)
    return bits ^ np.where(bits >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def bits_of_key(key):
    key = np.asarray(key, np.uint32)
    return key ^ np.where(key >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF)).astype(np.uint32)


def keys(bits):
    """(minimum keys, maximum keys) of samples: a NaN is each reduction's identity"""
    nan = is_nan(bits)
    k = key_of(bits)
    return np.where(nan, NO_MIN, k).astype(np.uint32), np.where(nan, NO_MAX, k).astype(np.uint32)


def pair_bits(kmin, kmax):
    """key pairs -> (lo, hi) bit patterns, [..., 2]"""
    lo = np.where(kmin == NO_MIN, QNAN, bits_of_key(kmin)).astype(np.uint32)
    hi = np.where(kmax == NO_MAX, QNAN, bits_of_key(kmax)).astype(np.uint32)
    return np.stack([lo, hi], axis=-1)


def columns_of(x, m, flush=True):
    """x float32 [channels][S] -> (Wv bits uint32 [columns][channels][2], samples left open).  flush: a partial last column is emitted."""
    b = bits_of(x)
    channels, S = b.shape
    kmin, kmax = keys(b)
    full = S // m
    lo = kmin[:, :full * m].reshape(channels, full, m).min(axis=2) if full else np.zeros((channels, 0), np.uint32)
    hi = kmax[:, :full * m].reshape(channels, full, m).max(axis=2) if full else np.zeros((channels, 0), np.uint32)
    rest = S - full * m
    if rest and flush:
        lo = np.concatenate([lo, kmin[:, full * m:].min(axis=1, keepdims=True)], axis=1)
        hi = np.concatenate([hi, kmax[:, full * m:].max(axis=1, keepdims=True)], axis=1)
    return np.ascontiguousarray(pair_bits(lo, hi).transpose(1, 0, 2)), (0 if flush else rest)


def fold(wv, bounds):
    """Wv bits [n][channels][2] -> the coarser columns [len(bounds) - 1][channels][2]: column b is the fold of finer columns
    bounds[b] <= j < bounds[b + 1] (never empty)"""
    out = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        lo, hi = wv[a:b, :, 0], wv[a:b, :, 1]
        kmin = np.where(is_nan(lo), NO_MIN, key_of(lo)).astype(np.uint32).min(axis=0)
        kmax = np.where(is_nan(hi), NO_MAX, key_of(hi)).astype(np.uint32).max(axis=0)
        out.append(pair_bits(kmin, kmax))
    return np.stack(out)


SPECIALS = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF,
                     0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF], np.uint32)      # NaNs (quiet, negative, signalling), +-inf, +-0, denormals, +-FLT_MAX


def content(kind, channels, S, m, seed):
    """float32 [channels][S] test content: 'random' (normal), 'constant', 'ramp', each with special values first, last and alone in a column of
    m samples, and whole columns of NaNs; 'plain': random without them"""
    rng = np.random.default_rng(seed)
    if kind == "constant":
        x = np.full((channels, S), 0.25, np.float32) * np.arange(1, channels + 1, dtype=np.float32)[:, None]
    elif kind == "ramp":
        x = (np.arange(S, dtype=np.float32)[None, :] - np.float32(S / 2)) * np.float32(1e-3) * np.arange(1, channels + 1, dtype=np.float32)[:, None]
    else:
        x = rng.standard_normal((channels, S)).astype(np.float32)
    b = np.ascontiguousarray(x).view(np.uint32)
    if kind == "plain" or S == 0:
        return x
    columns = -(-S // m)
    for d in range(channels):
        for c in rng.choice(columns, size=min(columns, 12), replace=False):
            a, e = c * m, min((c + 1) * m, S)
            how = int(rng.integers(0, 4))
            v = SPECIALS[int(rng.integers(0, len(SPECIALS)))]
            if how == 0:
                b[d, a] = v                                  # first in its column
            elif how == 1:
                b[d, e - 1] = v                              # last
            elif how == 2:
                b[d, a:e] = np.uint32(0x7FC00000)            # alone: the rest of the column are NaNs
                b[d, int(rng.integers(a, e))] = v
            else:
                b[d, a:e] = SPECIALS[int(rng.integers(0, 3))]        # a column of NaNs
    return x
