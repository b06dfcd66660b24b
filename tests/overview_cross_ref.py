"""The cross overview's definition (include/sgz.h, "The cross overview") restated in numpy, for tests/test_overview_cross_host.py (which
checks this restatement against exact rational arithmetic and the host helpers against it) and the GPU tests (which hold the kernels to it).
It shares no code with the library:
  q      = per bin of a frame, from the floats lr, li, rr, ri: the fp64 products and sums in separate ufunc calls (nothing can be contracted),
           scaled by 2^(62 - 2n), clamped to +-(2^63 - 2^10), np.rint (ties to even), int64 -- which always fits, the clamp is below 2^63; a
           bin with a non-finite float takes no part and is counted in skipped;
  record = (ll, rr, re, im: 128-bit sums in two words each, re and im in two's complement; count; skipped) per (column, pair, band);
  sums   = 32-bit limbs added in int64 (fewer than 2^31 terms of less than 2^32 cannot overflow one), the limbs recombined modulo 2^128 --
           by a carry chain in numpy integers (recombine), which the host test holds to Python integers (recombine_py);
  fold   = every field adds, over frames, columns or adjacent bands.
The readout is restated in the host test, in exact rationals.  Everything is compared as bytes."""
import numpy as np

DTYPE = np.dtype({"names": ["ll", "rr", "re", "im", "count", "skipped"],
                  "formats": [("<u8", (2,)), ("<u8", (2,)), ("<u8", (2,)), ("<u8", (2,)), "<u8", "<u8"],
                  "offsets": [0, 16, 32, 48, 64, 72], "itemsize": 80})
SUMS = ("ll", "rr", "re", "im")
Q_MOST = 2 ** 63 - 2 ** 10
MASK64 = 2 ** 64 - 1
M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def log2_of(N: int) -> int:
    n = int(N).bit_length() - 1
    assert 1 << n == N and n >= 3, N
    return n


def quantise(n: int, lr, li, rr, ri):
    """float32 [...] each -> (q int64 [..., 4]: a, b, c, d of the definition, skipped bool [...]); the q of a skipped bin are 0"""
    f = [np.ascontiguousarray(a, np.float32) for a in (lr, li, rr, ri)]
    fin = np.isfinite(f[0]) & np.isfinite(f[1]) & np.isfinite(f[2]) & np.isfinite(f[3])
    Lr, Li, Rr, Ri = (np.where(fin, a, np.float32(0)).astype(np.float64) for a in f)
    s = np.float64(2.0) ** (62 - 2 * n)
    most = np.float64(Q_MOST)
    assert int(most) == Q_MOST
    values = (np.add(np.multiply(Lr, Lr), np.multiply(Li, Li)), np.add(np.multiply(Rr, Rr), np.multiply(Ri, Ri)),
              np.add(np.multiply(Lr, Rr), np.multiply(Li, Ri)), np.subtract(np.multiply(Li, Rr), np.multiply(Lr, Ri)))
    q = np.stack([np.rint(np.minimum(np.maximum(np.multiply(x, s), -most), most)).astype(np.int64) for x in values], axis=-1)
    return q, ~fin


def limbs_of(q: np.ndarray) -> np.ndarray:
    """int64 [...] -> int64 [..., 4]: the four 32-bit limbs of q as a 128-bit two's complement integer"""
    v = np.ascontiguousarray(q, np.int64).view(np.uint64)
    ext = np.where(q < 0, M32, np.uint64(0))
    return np.stack([v & M32, v >> S32, ext, ext], axis=-1).astype(np.int64)


def recombine(limbs: np.ndarray) -> np.ndarray:
    """limb sums, int64 [..., 4], each 0 <= limb < 2^63 -> uint64 [..., 2] (low word, high word) of sum(limb_i 2^(32 i)) modulo 2^128"""
    limbs = np.asarray(limbs).astype(np.uint64)
    carry = np.zeros(limbs.shape[:-1], np.uint64)
    digits = []
    for i in range(4):
        limb = limbs[..., i]
        low = (limb & M32) + (carry & M32)                                    # split before adding, so nothing wraps
        high = (limb >> S32) + (carry >> S32) + (low >> S32)
        digits.append(low & M32)
        carry = high
    return np.stack([digits[0] | (digits[1] << S32), digits[2] | (digits[3] << S32)], axis=-1)


def recombine_py(limbs) -> np.ndarray:
    """the same in Python integers"""
    limbs = np.asarray(limbs)
    out = np.zeros((*limbs.shape[:-1], 2), np.uint64)
    flat = out.reshape(-1, 2)
    for i, row in enumerate(limbs.reshape(-1, 4)):
        total = sum(int(v) << (32 * j) for j, v in enumerate(row)) % 2 ** 128
        flat[i, 0], flat[i, 1] = total & MASK64, total >> 64
    return out


def word_limbs(words: np.ndarray) -> np.ndarray:
    """uint64 [..., 2] -> int64 [..., 4]"""
    lo, hi = words[..., 0], words[..., 1]
    return np.stack([lo & M32, lo >> S32, hi & M32, hi >> S32], axis=-1).astype(np.int64)


def fold(records: np.ndarray, axis: int = 0) -> np.ndarray:
    """field-wise fold along `axis` (fewer than 2^31 records)"""
    records = np.asarray(records, DTYPE)
    axis = axis % records.ndim
    out = np.zeros(records.shape[:axis] + records.shape[axis + 1:], DTYPE)
    for name in SUMS:
        out[name] = recombine(word_limbs(records[name]).sum(axis=axis, dtype=np.int64))
    out["count"] = records["count"].sum(axis=axis, dtype=np.uint64)
    out["skipped"] = records["skipped"].sum(axis=axis, dtype=np.uint64)
    return out


def records_of(bins: np.ndarray, N: int, edges) -> np.ndarray:
    """bins: float32 [frames][pairs][N + 1][2] as sgz_stage_bins writes them on a Phase plan -> the records [frames][pairs][bands] of every
    single frame: what a column of one frame holds"""
    n = log2_of(N)
    bins = np.ascontiguousarray(bins, np.float32)
    assert bins.shape[2:] == (N + 1, 2), bins.shape
    edges = np.asarray(edges, np.int64)
    assert edges[0] >= 1 and edges[-1] <= N // 2 - 1 and (np.diff(edges) >= 0).all()
    L = bins[:, :, 1:N // 2 - 1]                                              # bins 1 .. N/2 - 2
    R = bins[:, :, N - 1:N // 2 + 1:-1]                                       # N - k for the same k
    assert L.shape == R.shape == (*bins.shape[:2], N // 2 - 2, 2)
    q, skipped = quantise(n, L[..., 0], L[..., 1], R[..., 0], R[..., 1])

    def band_sums(x):                                                         # [frames][pairs][bins][...] -> [frames][pairs][bands][...], int64
        cs = np.concatenate([np.zeros_like(x[:, :, :1]), np.cumsum(x, axis=2, dtype=np.int64)], axis=2)
        return cs[:, :, edges[1:] - 1] - cs[:, :, edges[:-1] - 1]

    limbs = band_sums(limbs_of(q))                                            # [frames][pairs][bands][4][4]
    out = np.zeros(limbs.shape[:3], DTYPE)
    for i, name in enumerate(SUMS):
        out[name] = recombine(limbs[..., i, :])
    out["count"] = band_sums((~skipped).astype(np.int64))
    out["skipped"] = band_sums(skipped.astype(np.int64))
    return out


def columns_of(each: np.ndarray, k: int, held: int = 0, carry=None, flush: bool = True):
    """each: records_of(...) [frames][pairs][bands].  -> (records [columns][pairs][bands], the open column's records [pairs][bands] or None,
    frames left open); `carry` (records [pairs][bands]) stands for the `held` frames in front"""
    frames = each.shape[0]
    t = held + frames
    closed = t // k + (1 if flush and t % k else 0)

    def column(c):
        a, b = max(c * k - held, 0), min((c + 1) * k - held, frames)
        parts = each[a:max(a, b)]
        if c == 0 and held:
            parts = np.concatenate([np.asarray(carry, DTYPE).reshape(1, *each.shape[1:]), parts])
        return fold(parts, axis=0)

    out = [column(c) for c in range(closed)]
    v = np.stack(out) if out else np.zeros((0, *each.shape[1:]), DTYPE)
    if not flush and t % k:
        return v, column(closed), t % k
    return v, None, 0


def view_of(records: np.ndarray, x0: int, x1: int, out_columns: int) -> np.ndarray:
    """the fold over columns: column b = the fold of source columns x0 + ceil(b m / cols) .. x0 + ceil((b + 1) m / cols)"""
    m = x1 - x0
    cols = min(out_columns, m)
    return np.stack([fold(records[x0 + -(-b * m // cols):x0 + -(-(b + 1) * m // cols)], axis=0) for b in range(cols)])


def bands_of(records: np.ndarray, edges, coarse) -> np.ndarray:
    """the fold over bands of records [...][bands]: coarse band c is the fold of the non-empty fine bands inside [coarse[c], coarse[c + 1])"""
    edges, coarse = [int(e) for e in edges], [int(e) for e in coarse]
    assert all(c in edges for c in coarse)
    out = np.zeros((*records.shape[:-1], len(coarse) - 1), DTYPE)
    for c in range(len(coarse) - 1):
        js = [j for j in range(len(edges) - 1) if coarse[c] <= edges[j] < edges[j + 1] <= coarse[c + 1]]
        if js:
            out[..., c] = fold(records[..., js], axis=-1)
    return out


def sums(records: np.ndarray, name: str) -> np.ndarray:
    """a sum field as an object array of Python ints, the signed ones (re, im) as signed values"""
    w = np.asarray(records, DTYPE)[name]
    flat = [int(lo) | (int(hi) << 64) for lo, hi in w.reshape(-1, 2)]
    if name in ("re", "im"):
        flat = [v - 2 ** 128 if v >> 127 else v for v in flat]
    out = np.empty(len(flat), object)
    out[:] = flat
    return out.reshape(w.shape[:-1])


def same(a: np.ndarray, b: np.ndarray) -> bool:
    """records equal byte for byte"""
    a, b = np.ascontiguousarray(a, DTYPE), np.ascontiguousarray(b, DTYPE)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def edges_octave(sample_rate: float, N: int, b: int, f_lo: float, f_hi: float):
    """sgz_cross_edges_octave restated: (edges as Python ints, centres, the fp64 products whose ceilings the edges are)"""
    j0 = int(np.floor(b * np.log2(f_lo / 1000.0))) - 3
    j1 = int(np.ceil(b * np.log2(f_hi / 1000.0))) + 3
    centres = [1000.0 * 2.0 ** (j / b) for j in range(j0, j1 + 1)]
    centres = [f for f in centres if f_lo <= f <= f_hi]
    products = [f * 2.0 ** (-1.0 / (2 * b)) * N / sample_rate for f in centres] + [centres[-1] * 2.0 ** (1.0 / (2 * b)) * N / sample_rate]
    edges = [min(max(int(np.ceil(p)), 1), N // 2 - 1) for p in products]
    return edges, centres, products
