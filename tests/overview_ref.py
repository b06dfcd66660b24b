"""The overview's definition (include/sgz.h, "The overview render") restated in numpy, for tests/test_overview_host.py (which checks this
restatement on hand-made groups) and tests/test_gpu_overview.py (which holds the kernels to it):
  V = the greatest value of a group under the total order "NaNs take no part; the others by bits ^ (sign ? 0xFFFFFFFF : 0x80000000) as
  unsigned" (IEEE order with -0 below +0); a group of NaNs alone gives the quiet NaN 0x7FC00000;
  pixel = oracle.pyoracle.blend_column of the pairs' V.
Everything is compared as bit patterns (uint32 views)."""
import numpy as np

QUIET_NAN = np.uint32(0x7FC00000)


def order_key(values: np.ndarray) -> np.ndarray:
    """float32 -> uint32 keys; 0 for a NaN (no non-NaN value has key 0: -inf's is 0x007FFFFF)"""
    bits = np.ascontiguousarray(values, np.float32).view(np.uint32)
    key = bits ^ np.where(bits >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)
    return np.where((bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0), key).astype(np.uint32)


def key_value(key: np.ndarray) -> np.ndarray:
    """uint32 keys -> the bits of the value (uint32); key 0 -> the quiet NaN"""
    key = np.asarray(key, np.uint32)
    bits = key ^ np.where(key >> 31 != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF)).astype(np.uint32)
    return np.where(key == 0, QUIET_NAN, bits).astype(np.uint32)


def greatest(values: np.ndarray, axis: int = 0) -> np.ndarray:
    """the greatest of `values` along `axis`, as uint32 bit patterns"""
    return key_value(order_key(values).max(axis=axis))


def columns_of(x: np.ndarray, k: int, held: int = 0, carry=None, flush: bool = True):
    """x: float32 [frames][pairs][P], graph 0's first components.  -> (V bits uint32 [columns][pairs][P], the open column's V bits [pairs][P]
    or None, frames left open); `carry` (float32 or uint32 bits [pairs][P]) stands for the `held` frames in front of x"""
    frames = x.shape[0]
    keys = order_key(x).reshape(x.shape)
    if held:
        c = np.asarray(carry)
        c = c.view(np.float32) if c.dtype == np.uint32 else c.astype(np.float32)
        keys = np.concatenate([np.broadcast_to(order_key(c).reshape(1, *x.shape[1:]), (held, *x.shape[1:])), keys])
    t = held + frames
    closed = t // k + (1 if flush and t % k else 0)
    out = [key_value(keys[c * k:min((c + 1) * k, t)].max(axis=0)) for c in range(closed)]
    v = np.stack(out) if out else np.zeros((0, *x.shape[1:]), np.uint32)
    if not flush and t % k:
        return v, key_value(keys[closed * k:].max(axis=0)), t % k
    return v, None, 0


def blend(po, params, v_bits: np.ndarray) -> np.ndarray:
    """RGBA8 [columns][P][4] of V bits [columns][pairs][P] through the oracle's colour stage"""
    v = np.ascontiguousarray(v_bits, np.uint32).view(np.float32)
    cols = []
    for c in range(v.shape[0]):
        z = np.zeros(v.shape[1:], np.complex64)
        z.real = v[c]
        assert np.array_equal(np.ascontiguousarray(z.real).view(np.uint32), v_bits[c])       # (the bits survive the complex container)
        cols.append(po.blend_column(params, z))
    return np.stack(cols) if cols else np.zeros((0, v.shape[2], 4), np.uint8)


def burst_signal(window_size: int, hop: int, frames: int, channels: int, sample_rate: float = 48000.0, seed: int = 0) -> np.ndarray:
    """float32 [channels][S], S = window_size + hop (frames - 1): silence with a burst of one hop's length every third hop, each at its
    own frequency and level (and each channel with its own), so that the frames of an overview column peak at different pixels"""
    S = window_size + hop * (frames - 1)
    rng = np.random.default_rng(seed)
    x = np.zeros((channels, S), np.float64)
    n = np.arange(hop)
    for ch in range(channels):
        for j, start in enumerate(range(0, S - hop + 1, 3 * hop)):
            f = sample_rate * (0.02 + 0.43 * rng.random())
            level = 10.0 ** (-2.5 * rng.random())
            x[ch, start:start + hop] = level * np.sin(2 * np.pi * f * (n + start) / sample_rate + ch + j)
    return x.astype(np.float32)
