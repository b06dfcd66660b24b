"""A plain numpy restatement of everything the Spectrum chain does after the bins: the frequency and slope tables, the pixel map
(which bins a pixel shows, and how), the peak decay, the dB scale and the colour gradient.  It imports config's constants and
tests/fp64_bins.py and calls nothing in oracle/ or the library, so that it can hold both (tests/test_map_fp64_host.py the oracle,
tests/test_gpu_map_fp64.py every map form of the kernels): tests/parity_chain.py's links 2 and 3 are bit-exact *against the oracle*,
which only shows that two restatements by one reader of the reference agree.

Written from the reference's Source/Spectrum/TransformDSP.inl (mapToLinearSpace, FFT branch; mapAndTransformDFTFilters),
TransformConstant.h (remapFrequencies, generateSlopeMap) and SpectrumDSP.cpp (blendAndDispatchSpectrums), in set form: a pixel is
described by the set of bins it shows, not by the loop that visits them.

  frequencies   fp64.  Linear view: f(i) = c (left half + size i half / (P - 1)), half = sample rate / 2, c = 2 in Complex mode.  Log view:
                f(i) = m (half / m)^a, a = left + size i / (P - 1), m = min_log_freq; Complex folds at a = 0.5: a < 0.5 shows
                m (half / m)^(2a), above it half + (half - m (half / m)^(1 - 2 (a - 0.5))).  The reference evaluates in double and rounds once.
  slope         b f^a with a, b rounded to float32 first (the reference computes it in float32 from the float32 table).
  structure     exact float32 arithmetic on a GIVEN float32 table mf, as the reference does it: top = float32(sample rate) / 2,
                freqToBin = float32(numBins) / top, pos[x] = mf[x] freqToBin.  Pixel x is `narrow' when float32((mf[x + 1] - mf[x]) / top),
                widened to double, is <= 1 / numBins (Complex: 1 / (2 numBins)).  Outside Complex the pixels before the first that is not
                narrow interpolate, every pixel from it on shows a run of bins, and pixel P - 1 always shows a run.  Complex interpolates
                until a pixel is wider, shows runs until a pixel is *strictly* narrower, and so on; its pixel P - 1 stays in whichever
                phase it is met.  A run pixel with bin = floor(pos[x]) shows the bins old + 1 .. bin, old the bin of the run pixel
                before it, or {bin} alone when bin == old; the first pixel of a stretch of run pixels is its own `old'.  The second
                side of Separate / Mid-Side shows the mirrored entries N - k of the same run.
  values        fp64 on fp64_bins.mode_bins' complex csf[0 .. N] (the mono modes' upper half and Complex's csf[0] stay complex, as
                the reference leaves them: the interpolation filters reach them at low positions through the wrap).
                None: csf[clamp(floor(pos + 0.5), 0, hi)], hi = numBins (Complex: N); second side csf[N - index].
                Linear: csf[f] (1 - t) + csf[f + 1] t, f = floor(pos), t = pos - f.  Lanczos, a = 5: sum over i = f - 4 .. f + 5 of
                csf[i] L(pos - i), L(d) = sinc(d) sinc(d / 5).  Both index modulo N + 1; the second side filters at
                float32(float32(N) - pos).  A run pixel is the largest |csf| of its run.  Everything times
                invSize = window scale / (W / 2), window scale = W / sum(w); the plane holds the magnitude.
  decay, dB     state_k = max(state_k pole_k, magnitude), pole_k the float32 value; result = ln(slope state / lowFrac) /
                ln(highFrac / lowFrac), clip_db where the argument is not positive.  Two graphs, one state per side.
  colour        per pair: an intensity below 0 adds nothing; from 0.999 upward the last stop; otherwise the first stop c whose
                running sum of ratios reaches the intensity, mixed linearly with stop c - 1.  Pairs are screen-blended,
                c += (1 - c) colour.  Real values in 0 .. 255, not bytes.

Phase mode is out of scope: it shows the values of an arg-max bin, not a maximum, and has the lazily normalised boundary Q6
(oracle/spectrum.c); tests/test_gpu_phase.py and parity_chain.py's tie rule hold it.

`misread` selects one deliberately wrong reading (test_map_fp64_host.py shows that each misses the oracle by far more than the bars:
the standing evidence that the bars are sharp enough to matter); None everywhere else.
"""
from collections import namedtuple

import numpy as np

from signalizer_amd import config

import fp64_bins

MISREADINGS = ("run_from_old", "none_no_half", "mirror_plus_one", "break_lt_double", "decay_after_max", "mirror_run_shifted")
TWO_SIDED = (config.CH_SEPARATE, config.CH_MIDSIDE)
LANCZOS_A = 5

# interp [P] bool; pos [P] float32; lo, hi [P] int (the run lo .. hi of a run pixel, -1 elsewhere); breaks: the first pixel of every
# stretch of run pixels (one entry outside Complex: the break pixel); returns: the pixels at which Complex goes back to interpolating
Structure = namedtuple("Structure", "N num_bins complex two_sided interp pos lo hi breaks returns")


def _check_mode(mode):
    if mode == config.CH_PHASE:
        raise ValueError("Phase mode is out of scope (tests/test_gpu_phase.py)")


def transform_size(W: int) -> int:
    return max(32, 1 << (int(W) - 1).bit_length())


def frequencies(cfg: dict) -> np.ndarray:
    """fp64 [P]: the frequency every pixel shows"""
    _check_mode(cfg["channel_mode"])
    P = int(cfg["axis_points"])
    cplx = cfg["channel_mode"] == config.CH_COMPLEX
    half = float(np.float32(cfg["sample_rate"])) / 2.0
    left, size = float(cfg["view_left"]), float(cfg["view_right"]) - float(cfg["view_left"])
    t = np.arange(P, dtype=np.float64) / (P - 1)
    if cfg["view_scaling"] == config.VIEW_LINEAR:
        return (2.0 if cplx else 1.0) * half * (left + size * t)
    m = float(cfg["min_log_freq"])
    a = left + size * t
    if not cplx:
        return m * (half / m) ** a
    low = m * (half / m) ** np.minimum(2.0 * a, 1.0)
    high = half + (half - m * (half / m) ** np.clip(1.0 - 2.0 * (a - 0.5), 0.0, 1.0))
    return np.where(a < 0.5, low, high)


def slope(cfg: dict, mf: np.ndarray) -> np.ndarray:
    """fp64 [P]: b f^a on a given frequency table"""
    a, b = float(np.float32(cfg["slope_a"])), float(np.float32(cfg["slope_b"]))
    return b * np.asarray(mf, np.float64) ** a


def structure(cfg: dict, N: int, mf: np.ndarray, misread=None) -> Structure:
    mode = cfg["channel_mode"]
    _check_mode(mode)
    mf = np.asarray(mf)
    assert mf.dtype == np.float32, "the structure is float32 arithmetic on the float32 table"
    P = mf.size
    cplx = mode == config.CH_COMPLEX
    num_bins = N // 2
    top = np.float32(cfg["sample_rate"]) / np.float32(2)
    pos = mf * (np.float32(num_bins) / top)
    assert pos.dtype == np.float32
    width = ((mf[1:] - mf[:-1]) / top).astype(np.float64)              # of pixels 0 .. P - 2
    fft_width = 1.0 / (2 * num_bins if cplx else num_bins)
    if misread == "break_lt_double":
        wider = ~(width < 2.0 * fft_width)
    else:
        wider = width > fft_width
    narrower = width < fft_width
    interp = np.zeros(P, bool)
    breaks, returns = [], []
    if not cplx:
        first = np.flatnonzero(wider)
        brk = int(first[0]) if first.size else P - 1
        interp[:brk] = True
        breaks.append(brk)
    else:
        interpolating = True
        for x in range(P):
            if x != P - 1:
                if interpolating and wider[x]:
                    interpolating = False
                    breaks.append(x)
                elif not interpolating and narrower[x]:
                    interpolating = True
                    returns.append(x)
            interp[x] = interpolating
    bins = np.floor(pos.astype(np.float64)).astype(np.int64)
    lo = np.full(P, -1, np.int64)
    hi = np.full(P, -1, np.int64)
    run = np.flatnonzero(~interp)
    if run.size:
        starts = np.isin(run, breaks)                                    # the first pixel of a stretch is its own `old'
        old = np.where(starts, bins[run], np.concatenate([[0], bins[run][:-1]]))
        assert (bins[run] >= old).all(), "the frequency table must not decrease over run pixels"
        hi[run] = bins[run]
        lo[run] = np.where(bins[run] > old, old + 1, bins[run])
        if misread == "run_from_old":
            lo[run] = old
            hi[run] = np.where(bins[run] > old, bins[run] - 1, bins[run])
    return Structure(N, num_bins, cplx, mode in TWO_SIDED, interp, pos, lo, hi, breaks, returns)


def lanczos(d: np.ndarray, a: int = LANCZOS_A) -> np.ndarray:
    d = np.asarray(d, np.float64)
    return np.where(np.abs(d) < a, np.sinc(d) * np.sinc(d / a), 0.0)


def _filter(csf, pos, interpolation, hi, N, misread):
    """csf [F][N + 1] complex at positions pos [n] float32 -> (values [F][n] complex, sum |w| [n])"""
    p = pos.astype(np.float64)
    f = np.floor(p).astype(np.int64)
    if interpolation == config.INTERP_NONE:
        idx = np.clip(np.floor(p + (0.0 if misread == "none_no_half" else 0.5)).astype(np.int64), 0, hi)
        return idx, csf[:, idx], np.ones(p.size)
    if interpolation == config.INTERP_LINEAR:
        t = p - f
        return None, csf[:, f % (N + 1)] * (1.0 - t) + csf[:, (f + 1) % (N + 1)] * t, np.ones(p.size)
    taps = f[:, None] + np.arange(1 - LANCZOS_A, LANCZOS_A + 1)         # [n][2a]
    w = lanczos(p[:, None] - taps)
    return None, (csf[:, taps % (N + 1)] * w).sum(axis=-1), np.abs(w).sum(axis=-1)


def mapped(cfg: dict, st: Structure, csf: np.ndarray, inv_size: float, misread=None):
    """csf [F][N + 1] complex128 (fp64_bins.mode_bins) -> (planes [F][sides][P] fp64 magnitudes, sum |w| [sides][P])"""
    N, P = st.N, st.pos.size
    sides = 2 if st.two_sided else 1
    csf = np.asarray(csf, np.complex128)
    assert csf.ndim == 2 and csf.shape[1] == N + 1
    mag = np.abs(csf)
    planes = np.zeros((csf.shape[0], sides, P))
    sumw = np.ones((sides, P))
    ip = np.flatnonzero(st.interp)
    if ip.size:
        pos = st.pos[ip]
        idx, v, w = _filter(csf, pos, cfg["bin_interp"], N if st.complex else st.num_bins, N, misread)
        planes[:, 0, ip], sumw[0, ip] = np.abs(v), w
        if sides == 2:
            off = 1 if misread == "mirror_plus_one" else 0
            if idx is not None:
                v = csf[:, np.clip(N - idx + off, 0, N)]
            else:
                rpos = np.float32(N + off) - pos
                assert rpos.dtype == np.float32
                _, v, w = _filter(csf, rpos, cfg["bin_interp"], st.num_bins, N, misread)
            planes[:, 1, ip], sumw[1, ip] = np.abs(v), w
    shift = 1 if misread == "mirror_run_shifted" else 0
    for x in np.flatnonzero(~st.interp):
        lo, hi = int(st.lo[x]), int(st.hi[x])
        planes[:, 0, x] = mag[:, lo:hi + 1].max(axis=1)
        if sides == 2:
            planes[:, 1, x] = mag[:, max(N - hi + shift, 0):N - lo + shift + 1].max(axis=1)
    return planes * inv_size, sumw


def frame_planes(cfg: dict, st: Structure, l: np.ndarray, r: np.ndarray, misread=None):
    """l, r [F][W] samples of the frames of one pair -> (planes [F][sides][P], sum |w| [sides][P], scale [F], norm [F]): scale is
    invSize x the largest |fft((l + i r) w, N)| of the frame and norm invSize x ||l + i r||_2, what tests/parity_chain.py's bars are
    relative to (whatever the channel mode: the rounding of a derived channel comes from the whole frame's energy)"""
    W = int(cfg["window_size"])
    w = fp64_bins.window(cfg["window_type"], cfg["window_symmetry"], W, cfg["window_alpha"], cfg["window_beta"])
    inv_size = (W / w.sum()) / (W * 0.5)
    csf, _ = fp64_bins.mode_bins(cfg["channel_mode"], l, r, w, st.N)
    z = np.asarray(l, np.float64) + 1j * np.asarray(r, np.float64)
    scale = inv_size * np.abs(np.fft.fft(z * w, st.N, axis=-1)).max(axis=-1)
    norm = inv_size * np.sqrt((np.abs(z) ** 2).sum(axis=-1))
    planes, sumw = mapped(cfg, st, csf, inv_size, misread)
    return planes, sumw, scale, norm


def db_constants(cfg: dict):
    """(lowFrac, deltaYRecip = 1 / ln(highFrac / lowFrac))"""
    low, high = 10.0 ** (cfg["low_db"] / 20.0), 10.0 ** (cfg["high_db"] / 20.0)
    return low, 1.0 / np.log(high / low)


def decay_db(cfg: dict, planes: np.ndarray, slope_map: np.ndarray, state=None, misread=None):
    """planes [F][sides][P] -> (results [F][G][sides][P], states [F][G][sides][P]); state [G][sides][P]: carried in (zero when None)"""
    planes = np.asarray(planes, np.float64)
    F, sides, P = planes.shape
    poles = np.array([float(np.float32(v)) for v in cfg["pole"]])
    G = poles.size
    low, dyr = db_constants(cfg)
    s = np.zeros((G, sides, P)) if state is None else np.array(state, np.float64)
    states = np.zeros((F, G, sides, P))
    for f in range(F):
        if misread == "decay_after_max":
            s = np.maximum(s, planes[f][None]) * poles[:, None, None]
        else:
            s = np.maximum(s * poles[:, None, None], planes[f][None])
        states[f] = s
    arg = np.asarray(slope_map, np.float64) * states / low
    with np.errstate(divide="ignore", invalid="ignore"):
        results = np.where(arg > 0, np.log(np.where(arg > 0, arg, 1.0)) * dyr, float(cfg["clip_db"]))
    return results, states


def gradient(table: np.ndarray, ratios: np.ndarray, intensity: np.ndarray):
    """table [stops + 1][3], ratios [stops + 1] (ratios[0] = 0), intensity [P] -> (colour [P][3], shown [P] bool)"""
    table, ratios, v = np.asarray(table, np.float64), np.asarray(ratios, np.float64), np.asarray(intensity, np.float64)
    sums = np.cumsum(ratios)                                             # the running sum the stop search is on
    last = table.shape[0] - 1
    c = np.minimum(np.searchsorted(sums, v, side="left"), last)          # the first stop whose running sum reaches v
    c = np.maximum(c, 1)
    mix = (v - sums[c - 1]) / (sums[c] - sums[c - 1])
    col = table[c - 1] * (1.0 - mix)[:, None] + table[c] * mix[:, None]
    col = np.where(((v >= 0.999) | (v > sums[last]))[:, None], table[last], col)
    return col, v >= 0


def colour(tables, ratios: np.ndarray, intensities: np.ndarray) -> np.ndarray:
    """tables [C][stops + 1][3], intensities [C][P] (graph 0's first result of every pair) -> [P][3] real values in 0 .. 255"""
    intensities = np.asarray(intensities, np.float64)
    acc = np.zeros((intensities.shape[1], 3))
    for table, v in zip(tables, intensities):
        col, shown = gradient(table, ratios, v)
        acc = np.where(shown[:, None], acc + (1.0 - acc) * col, acc)
    return acc * 255.0


def gradient_slope(tables, ratios: np.ndarray) -> float:
    """the largest |d colour / d intensity| of a render: max over stops of |stop_c - stop_(c - 1)| / ratio_c, times the number of pairs"""
    ratios = np.asarray(ratios, np.float64)
    worst = 0.0
    for table in tables:
        t = np.asarray(table, np.float64)
        worst = max(worst, float((np.abs(t[1:] - t[:-1]).max(axis=1) / ratios[1:]).max()))
    return worst * len(tables)
