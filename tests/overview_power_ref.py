"""The power overview's definition (include/sgz.h, "The power overview") restated in numpy and Python ints, for
tests/test_overview_power_host.py (which checks this restatement against a brute-force loop and the host helpers against it) and the GPU
tests (which hold the kernels to it).  It shares no code with the library:
  q      = x^2 2^60 rounded to nearest, from the float's BITS in exact integer arithmetic (x = m 2^e, x^2 2^60 = m^2 2^(2e + 60); the
           exponent is even, so a tie cannot occur), clamped to 2^64 - 2^11; a NaN takes no part and is counted;
  record = (sum of q as a 128-bit integer in two words, count, nans, lo, hi) per (column, pair, side, pixel); lo / hi under the overview's
           total order (tests/overview_ref.py), 0x7FC00000 when count == 0;
  fold   = field-wise: sums (Python ints) and counts add, lo the least of the los, hi the greatest of the his;
  rms    = (float)(sqrt(((double)sum[1] 2^64 + (double)sum[0]) / (double)count) 2^-30) in numpy's fp64, 0x7FC00000 when count == 0.
Levels and pixels are not restated here: the tests hold them to the oracle's dB map and to the library's own K_B.
Everything is compared as bytes or bit patterns."""
import numpy as np

import overview_ref as ov

DTYPE = np.dtype({"names": ["sum", "count", "nans", "lo", "hi"], "formats": [("<u8", (2,)), "<u4", "<u4", "<f4", "<f4"],
                  "offsets": [0, 16, 20, 24, 28], "itemsize": 32})
Q_MOST = 2 ** 64 - 2 ** 11
COUNT_MOST = 2 ** 32 - 1
MASK64 = 2 ** 64 - 1


def q_of_bits(bits: int):
    """one float's bit pattern -> q as a Python int, or None for a NaN"""
    e, m = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    if e == 0xFF:
        return None if m else Q_MOST                                        # NaN / +-inf: the clamp
    if e == 0:
        e = 1                                                               # a denormal: no hidden bit, the least exponent
    else:
        m |= 0x800000
    shift = 2 * (e - 150) + 60                                              # x = m 2^(e - 150)
    sq = m * m
    if shift >= 0:
        u = sq << shift
    else:
        half = 1 << (-shift - 1)
        u, rest = sq >> -shift, sq & ((1 << -shift) - 1)
        if rest > half or (rest == half and u & 1):                         # (rest == half does not occur: see the docstring; kept for the rule)
            u += 1
    return min(u, Q_MOST)


def quantise(x: np.ndarray):
    """float32 [...] -> (q as an object array of Python ints, NaN mask); q of a NaN is 0"""
    x = np.ascontiguousarray(x, np.float32)
    qs = [q_of_bits(int(b)) for b in x.view(np.uint32).reshape(-1)]
    nan = np.array([q is None for q in qs], bool).reshape(x.shape)
    q = np.empty(len(qs), object)
    q[:] = [0 if v is None else v for v in qs]
    return q.reshape(x.shape), nan


def _sum_words(total) -> np.ndarray:
    """object array of Python ints < 2^128 -> uint64 [..., 2] (low word, high word)"""
    total = np.asarray(total, object)
    out = np.zeros((*total.shape, 2), np.uint64)
    flat = out.reshape(-1, 2)
    for i, v in enumerate(total.reshape(-1)):
        flat[i, 0], flat[i, 1] = v & MASK64, v >> 64
    return out


def sums(records: np.ndarray) -> np.ndarray:
    """the 128-bit sums of records as an object array of Python ints"""
    records = np.asarray(records, DTYPE)
    s = records["sum"]
    flat = [int(lo) | (int(hi) << 64) for lo, hi in s.reshape(-1, 2)]
    out = np.empty(len(flat), object)
    out[:] = flat
    return out.reshape(records.shape)


def _add_words(words: np.ndarray, axis: int) -> np.ndarray:
    """uint64 [..., 2] (low word, high word) summed along `axis` as 128-bit integers: four 32-bit limbs, each summed in uint64 (fewer than
    2^32 terms cannot overflow one), then the carries, all in integers; the test file checks it against Python ints"""
    m32 = np.uint64(0xFFFFFFFF)
    lo, hi = words[..., 0], words[..., 1]
    limbs = [(lo & m32).sum(axis=axis, dtype=np.uint64), (lo >> np.uint64(32)).sum(axis=axis, dtype=np.uint64),
             (hi & m32).sum(axis=axis, dtype=np.uint64), (hi >> np.uint64(32)).sum(axis=axis, dtype=np.uint64)]
    carry = np.zeros_like(limbs[0])
    digits = []
    for limb in limbs:
        # limb < 2^64 - 2^32 + 1 and carry < 2^33: split before adding, so nothing wraps
        low = (limb & m32) + (carry & m32)
        high = (limb >> np.uint64(32)) + (carry >> np.uint64(32)) + (low >> np.uint64(32))
        digits.append(low & m32)
        carry = high
    if np.any(carry):
        raise OverflowError("a folded sum passes 2^128")
    return np.stack([digits[0] | (digits[1] << np.uint64(32)), digits[2] | (digits[3] << np.uint64(32))], axis=-1)


def records_of(x: np.ndarray) -> np.ndarray:
    """the record of every single value: what a column of one frame holds"""
    x = np.ascontiguousarray(x, np.float32)
    q, nan = quantise(x)
    r = np.zeros(x.shape, DTYPE)
    r["sum"] = _sum_words(q)
    r["count"], r["nans"] = ~nan, nan
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
    out["sum"] = _add_words(records["sum"], axis)
    out["count"], out["nans"] = count, nans
    shape = records.shape
    hi = ov.order_key(records["hi"]).reshape(shape).max(axis=axis, initial=0)
    lo = ((ov.order_key(records["lo"]).reshape(shape).astype(np.int64) - 1) & 0xFFFFFFFF).min(axis=axis, initial=0xFFFFFFFF)  # key - 1: a NaN's wraps to "none"
    out["hi"] = ov.key_value(hi).view(np.float32)
    out["lo"] = ov.key_value(((lo + 1) & 0xFFFFFFFF).astype(np.uint32)).view(np.float32)
    return out


def columns_of(x: np.ndarray, k: int, held: int = 0, carry=None, flush: bool = True, each=None):
    """x: float32 [frames][pairs][sides][P], the mapped magnitudes.  -> (records [columns][pairs][sides][P], the open column's records
    [pairs][sides][P] or None, frames left open); `carry` (records [pairs][sides][P]) stands for the `held` frames in front of x; `each`:
    records_of(x), where the caller has them already"""
    frames = x.shape[0]
    each = records_of(x) if each is None else each
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


def mean_square_scaled(records: np.ndarray) -> np.ndarray:
    """ms of the definition as float64 (in units of 2^-60); NaN where count == 0"""
    records = np.asarray(records, DTYPE)
    s = records["sum"]
    S = s[..., 1].astype(np.float64) * 2.0 ** 64 + s[..., 0].astype(np.float64)     # uint64 -> double and the sum round to nearest even
    with np.errstate(divide="ignore", invalid="ignore"):
        return S / records["count"].astype(np.float64)


def rms_bits(records: np.ndarray) -> np.ndarray:
    """uint32 bit patterns of the rms values"""
    records = np.asarray(records, DTYPE)
    with np.errstate(invalid="ignore"):
        rms = (np.sqrt(mean_square_scaled(records)) * 2.0 ** -30).astype(np.float32)
    return np.where(records["count"] == 0, ov.QUIET_NAN, rms.view(np.uint32)).astype(np.uint32)


def same(a: np.ndarray, b: np.ndarray) -> bool:
    """records equal byte for byte"""
    a, b = np.ascontiguousarray(a, DTYPE), np.ascontiguousarray(b, DTYPE)
    return a.shape == b.shape and a.tobytes() == b.tobytes()
