"""A plain numpy fp64 restatement of the csf[0 .. N] that sgz_stage_bins returns and the oracle's frame_bins computes, for every channel
mode (Source/Spectrum/TransformDSP.inl).  Nothing here calls into the oracle or the library (only config's constants are read): the
windows are evaluated from their definitions in fp64 as well.

A frame's W samples are windowed and zero-padded to N; numBins = N/2.
  Left / Right / Merge / Side (:61-147 the mixes, Merge and Side with their 0.5; :544-560 the map):  X = fft(s w, N) of one real signal,
    csf[0] = |X[0]| / 2, csf[k] = |X[k]| (k = 1 .. N/2 - 1),  csf[N/2] = X[N/2] / 2 and csf[N/2 + 1 .. N - 1] = X[k] left complex (KA15),
    csf[N] = 0 (never written by the reference).
  Separate (:854-869), Mid-Side (the same on ((l + r) / 2, (l - r) / 2), :148-181): one complex transform carries both channels,
    Z = fft((a + i b) w, N); the two-for-one split recovers
        L[k] = (Z[k] + conj Z[N - k]) / 2,   R[k] = (Z[k] - conj Z[N - k]) / (2 i)
    and the map keeps, per index:
        csf[k]      = |L[k]|              k = 1 .. N/2 - 2
        csf[N/2 - 1] = |L[N/2 - 1]| / 2   (quirk Q3: the reference halves the entry below N/2 as well, :864)
        csf[N/2]    = |Z[N/2]| / 2        (the one entry that needs both channels: L[N/2] + i R[N/2], never split, :863)
        csf[N - k]  = |R[k]|              k = 1 .. N/2 - 1
        csf[0]      = Re Z[0] / 2,  csf[N] = Im Z[0] / 2    (L[0] / 2 and R[0] / 2, signed, :861-862)
  Complex (:987-1002): Z = fft((l + i r) w, N), csf[0] = Z[0] / 2 left complex, csf[k] = |Z[k]| (k = 1 .. N - 1), csf[N] = 0.
  Phase (:643-652): the split of Separate with the values kept complex -- csf[k] = L[k], csf[N - k] = R[k], csf[N/2 - 1] halved (Q3),
    csf[N/2] = Z[N/2] / 2, csf[0] = Re Z[0] / 2, csf[N] = Im Z[0] / 2.

mode_bins returns the frame's scale beside csf: the largest |X| (mono modes) or |Z| (Complex) of the transform, the largest |csf| in the
split modes -- what the bars of the tests are relative to.  A derived channel (Side, the second channel of a split, a quiet channel)
is never scaled by its own maximum: its rounding comes from the whole frame's energy.
"""
import numpy as np

from signalizer_amd import config

# cosine-sum windows: coefficients a_j of w = sum_j (-1)^j a_j cos(j t), t = 2 pi x
_COS_SUMS = {
    config.WIN_RECT: (1.0,),
    config.WIN_HANN: (0.5, 0.5),
    config.WIN_HAMMING: (0.54, 0.46),
    config.WIN_FLATTOP: (0.21557895, 0.41663158, 0.277263158, 0.083578947, 0.006947368),
    config.WIN_BLACKMAN: (0.42, 0.5, 0.08),
    config.WIN_EXACT_BLACKMAN: (7938.0 / 18608.0, 9240.0 / 18608.0, 1430.0 / 18608.0),
    config.WIN_NUTTALL: (0.355768, 0.487396, 0.144232, 0.012604),
    config.WIN_BLACKMAN_NUTTALL: (0.3635819, 0.4891775, 0.1365995, 0.0106411),
    config.WIN_BLACKMAN_HARRIS: (0.35875, 0.48829, 0.14128, 0.01168),
}

MONO_MODES = (config.CH_LEFT, config.CH_RIGHT, config.CH_MERGE, config.CH_SIDE)


def window(window_type: int, symmetry: int, W: int, alpha: float = 0.0, beta: float = 0.0) -> np.ndarray:
    """fp64 window of W points at x = n / D, D = W (periodic) or W - 1 (symmetric)"""
    D = float(W) if symmetry == config.WIN_PERIODIC else float(max(W - 1, 1))
    x = np.arange(W, dtype=np.float64) / D
    u = 2.0 * x - 1.0
    if window_type in _COS_SUMS:
        w = np.zeros(W, np.float64)
        for j, a in enumerate(_COS_SUMS[window_type]):
            w += (-1.0) ** j * a * np.cos(2.0 * np.pi * j * x)
        return w
    if window_type == config.WIN_TRIANGULAR:
        return 1.0 - np.abs(u)
    if window_type == config.WIN_WELCH:
        return 1.0 - u * u
    if window_type == config.WIN_GAUSSIAN:
        s = alpha if alpha > 0 else 0.4
        return np.exp(-0.5 * (u / s) ** 2)
    if window_type == config.WIN_KAISER:
        return np.i0(beta * np.sqrt(np.maximum(1.0 - u * u, 0.0))) / np.i0(beta)
    raise ValueError(f"window type {window_type}")


def _split(Z: np.ndarray, N: int):
    """(L[1 .. N/2 - 1], R[1 .. N/2 - 1]) of the two-for-one split of Z [..., N]"""
    k = np.arange(1, N // 2)
    a, b = Z[..., k], np.conj(Z[..., N - k])
    return 0.5 * (a + b), -0.5j * (a - b)


def _transform(z: np.ndarray, w: np.ndarray, N: int) -> np.ndarray:
    return np.fft.fft(z * np.asarray(w, np.float64), N, axis=-1)


def separate_bins(l: np.ndarray, r: np.ndarray, w: np.ndarray, N: int) -> np.ndarray:
    """l, r: [..., W] samples of one or more frames, w: [W] window.  Returns csf [..., N + 1] in fp64."""
    Z = _transform(np.asarray(l, np.float64) + 1j * np.asarray(r, np.float64), w, N)
    M = N // 2
    k = np.arange(1, M)
    L, R = _split(Z, N)
    csf = np.zeros(Z.shape[:-1] + (N + 1,), np.float64)
    csf[..., k] = np.abs(L)
    csf[..., N - k] = np.abs(R)
    csf[..., M - 1] *= 0.5
    csf[..., M] = 0.5 * np.abs(Z[..., M])
    csf[..., 0] = 0.5 * Z[..., 0].real
    csf[..., N] = 0.5 * Z[..., 0].imag
    return csf


def phase_split(Z: np.ndarray, N: int) -> np.ndarray:
    """Phase mode's complex csf [..., N + 1] from a transform Z [..., N] of (l + i r) w (any precision; computed in fp64)"""
    Z = np.asarray(Z, np.complex128)
    M = N // 2
    k = np.arange(1, M)
    L, R = _split(Z, N)
    csf = np.zeros(Z.shape[:-1] + (N + 1,), np.complex128)
    csf[..., k] = L
    csf[..., N - k] = R
    csf[..., M - 1] *= 0.5
    csf[..., M] = 0.5 * Z[..., M]
    csf[..., 0] = 0.5 * Z[..., 0].real
    csf[..., N] = 0.5 * Z[..., 0].imag
    return csf


def mode_bins(mode: int, l: np.ndarray, r: np.ndarray, w: np.ndarray, N: int):
    """l, r: [..., W] samples of one or more frames, w: [W] window.  Returns (csf [..., N + 1] complex128, scale [...])."""
    l, r = np.asarray(l, np.float64), np.asarray(r, np.float64)
    M = N // 2
    if mode in MONO_MODES:
        s = {config.CH_LEFT: l, config.CH_RIGHT: r, config.CH_MERGE: 0.5 * (l + r), config.CH_SIDE: 0.5 * (l - r)}[mode]
        X = _transform(s, w, N)
        csf = np.zeros(X.shape[:-1] + (N + 1,), np.complex128)
        csf[..., :N] = X
        csf[..., :M] = np.abs(X[..., :M])
        csf[..., 0] *= 0.5
        csf[..., M] *= 0.5
        return csf, np.abs(X).max(axis=-1)
    if mode in (config.CH_SEPARATE, config.CH_MIDSIDE):
        a, b = (l, r) if mode == config.CH_SEPARATE else (0.5 * (l + r), 0.5 * (l - r))
        csf = separate_bins(a, b, w, N).astype(np.complex128)
        return csf, np.abs(csf).max(axis=-1)
    if mode == config.CH_COMPLEX:
        Z = _transform(l + 1j * r, w, N)
        csf = np.zeros(Z.shape[:-1] + (N + 1,), np.complex128)
        csf[..., :N] = np.abs(Z)
        csf[..., 0] = 0.5 * Z[..., 0]
        return csf, np.abs(Z).max(axis=-1)
    if mode == config.CH_PHASE:
        csf = phase_split(_transform(l + 1j * r, w, N), N)
        return csf, np.abs(csf).max(axis=-1)
    raise ValueError(f"channel mode {mode}")
