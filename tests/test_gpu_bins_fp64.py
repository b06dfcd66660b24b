"""sgz_stage_bins of every (K_A path, channel mode) pair the library can take, held to the fp64 restatement of tests/fp64_bins.py
(mode_bins), which shares no code with the oracle or the kernels.

tests/test_gpu_spectrum.py holds the bins to the oracle, and the oracle and the kernels were written from the same reading of
TransformDSP.inl; tests/test_oracle_math.py anchors the oracle to mode_bins in every mode, and this file anchors the kernels to it
directly: the 0.5 of the mixes, Mid-Side packed as mid + i side, Complex's halved DC, the mono modes' halved Nyquist, the sign of R[k]
in Phase, symmetric and zero-padded windows.

Each case asserts the path its plan takes (sgz_plan_path without the SGZ_PATH_SIDE_MAP bit, which only concerns the pixel map), so that
a change of a plan default fails here instead of quietly dropping coverage, and renders enough frames that every launch has more than
one workgroup per pair.  The output is allocated over NaN (test_gpu_full_size._poison_next, after the input is on the device, and the
output's address is checked against the poisoned block's): an entry the launch never writes is NaN, not a stale copy of a right answer.

What sgz_stage_bins reports (sgz.h): the csf the reference's map leaves complex is reported as its magnitude -- the mono modes'
csf[N/2 .. N - 1] and Complex's csf[0]; Phase reports the complex csf itself; csf[0] and csf[N] of Separate / Mid-Side are signed.
The channel-split kernel's mono form differs in two entries' worth: it writes csf[0 .. N/2] only (it never forms the upper half, its
pixels read conj X[k] from a few held entries), so there the upper half must still hold the poison, and its csf[N/2] is X[N/2] / 2
itself, signed, as the reference holds it -- compared as such.  Every other path's upper half is compared, csf[N] == 0 included.

Bar: every compared entry within BIN_TOL x the frame's scale (mode_bins: the largest |X| / |Z| / |csf| of the frame -- a derived or
quiet channel is never scaled by its own maximum), and csf[0], csf[N/2 - 1], csf[N/2], csf[N] (split modes) or csf[0], csf[N/2]
(mono modes, Complex) each on its own.
"""
import numpy as np
import pytest

from signalizer_amd import api, config, synth

pytestmark = pytest.mark.gpu

BIN_TOL = 4e-6                              # tests/test_gpu_spectrum.py BIN_TOL
GENERIC, FUSED, HALVES, SIDE_MAP, SPLIT = 0, 1, 2, 4, 8      # SGZ_PATH_* (sgz.h)

L, R, MERGE, SIDE, PHASE, SEP, MS, CPLX = (config.CH_LEFT, config.CH_RIGHT, config.CH_MERGE, config.CH_SIDE, config.CH_PHASE,
                                            config.CH_SEPARATE, config.CH_MIDSIDE, config.CH_COMPLEX)
MONO = (L, R, MERGE, SIDE)
OFF = {api.OPT_CHANNEL_SPLIT: 0}
FETCH = {api.OPT_FETCH_WINDOW: 1}
BH = dict(window_type=config.WIN_BLACKMAN_HARRIS)


def _c(N, mode, path, signal="synth", W=None, hop=None, frames=5, pairs=1, opts=None, **cfg):
    W = W or N
    return dict(N=N, W=W, hop=hop or max(W // 4, 1), mode=mode, path=path, signal=signal, frames=frames, pairs=pairs, opts=opts or {},
                cfg=cfg)


# name -> case.  Signals: synth (synth.gen), noise (white), quiet (every pair's second channel 80 dB down), same (L ~ R), edges
# (csf[0], csf[N/2 - 1], csf[N/2], csf[N] among the largest entries of the frame: offsets, a tone on bin N/2 - 1, a Nyquist tone)
CASES = {
    # generic path (spectrum_generic.hip): every size that is neither R^3 nor 2 R^3, the other paths switched off, and Phase at any size
    "gen32_separate": _c(32, SEP, GENERIC, W=20, hop=7, axis_points=16),
    "gen32_left": _c(32, L, GENERIC, "edges", W=32, hop=8, axis_points=16),
    "gen1024_right": _c(1024, R, GENERIC, "noise"),
    "gen1024_midside": _c(1024, MS, GENERIC, "same", W=1000, window_type=config.WIN_KAISER, window_beta=8.0,
                          window_symmetry=config.WIN_SYMMETRIC),
    "gen1024_phase": _c(1024, PHASE, GENERIC, "noise"),
    "gen2048_side": _c(2048, SIDE, GENERIC, "same"),
    "gen2048_complex": _c(2048, CPLX, GENERIC, "edges"),
    "gen2048_merge": _c(2048, MERGE, GENERIC, W=1500, window_type=config.WIN_GAUSSIAN, window_alpha=0.3),
    "gen16384_left": _c(16384, L, GENERIC, "edges", opts=OFF),
    "gen16384_right": _c(16384, R, GENERIC, opts=OFF),
    "gen16384_merge": _c(16384, MERGE, GENERIC, "noise", opts=OFF),
    "gen16384_side": _c(16384, SIDE, GENERIC, "same", opts=OFF),
    "gen16384_separate": _c(16384, SEP, GENERIC, "quiet", opts=OFF),
    "gen16384_separate_edges": _c(16384, SEP, GENERIC, "edges", opts=OFF),
    "gen16384_midside": _c(16384, MS, GENERIC, "same", opts=OFF),
    "gen16384_complex": _c(16384, CPLX, GENERIC),
    "gen16384_phase": _c(16384, PHASE, GENERIC, "quiet"),
    "gen4096_phase": _c(4096, PHASE, GENERIC, "edges"),                              # phaseFusedFft: Z from the in-register FFT
    "gen32768_phase": _c(32768, PHASE, GENERIC, pairs=3),                             # phaseFusedFft, three pairs
    "gen8192_phase": _c(8192, PHASE, GENERIC, "same", W=5000, window_type=config.WIN_FLATTOP),
    # fused path: N = R^3 in one workgroup (stft_body.hpp)
    "fused4096_left": _c(4096, L, FUSED),
    "fused4096_separate": _c(4096, SEP, FUSED, "quiet"),
    "fused4096_midside": _c(4096, MS, FUSED, "same", W=3000, window_type=config.WIN_NUTTALL, window_symmetry=config.WIN_SYMMETRIC),
    "fused4096_complex": _c(4096, CPLX, FUSED, "edges"),
    "fused4096_side_edges": _c(4096, SIDE, FUSED, "edges"),
    "fused32768_merge": _c(32768, MERGE, FUSED, opts=OFF),
    "fused32768_separate": _c(32768, SEP, FUSED, "edges", opts=OFF),
    "fused32768_midside": _c(32768, MS, FUSED, opts=OFF),
    "fused32768_complex": _c(32768, CPLX, FUSED, "noise"),
    "fused32768_left_oddhop": _c(32768, L, FUSED, hop=8191),                          # an odd hop keeps the plan off the channel split
    # halves path: N = 2 R^3 as two half-frame workgroups (stft_body.hpp HALF), W == N and zero-padded
    "halves8192_left": _c(8192, L, HALVES),
    "halves8192_right": _c(8192, R, HALVES, "edges", W=5000),
    "halves8192_merge": _c(8192, MERGE, HALVES, "noise", W=5000, window_type=config.WIN_WELCH),
    "halves8192_side": _c(8192, SIDE, HALVES, "same"),
    "halves8192_separate": _c(8192, SEP, HALVES, "edges"),
    "halves8192_midside": _c(8192, MS, HALVES, "quiet", W=5000),
    "halves8192_complex": _c(8192, CPLX, HALVES, "noise", W=5000, window_type=config.WIN_TRIANGULAR),
    "halves65536_merge": _c(65536, MERGE, HALVES, opts=OFF, frames=3),
    "halves65536_side": _c(65536, SIDE, HALVES, "same", W=40000, frames=3),
    "halves65536_left": _c(65536, L, HALVES, "edges", opts=OFF, frames=3),
    "halves65536_separate": _c(65536, SEP, HALVES, opts=OFF, frames=3),
    "halves65536_separate_pad": _c(65536, SEP, HALVES, "quiet", W=40000, frames=3, window_type=config.WIN_KAISER, window_beta=8.0),
    "halves65536_midside": _c(65536, MS, HALVES, "same", opts=OFF, frames=3),
    "halves65536_complex": _c(65536, CPLX, HALVES, "edges", frames=3),
    # channel-split path (spectrum_real.hip): mono form, in-kernel Hann (FETCH_WINDOW 0), the fetched Hann and a table window
    "split16384_left": _c(16384, L, GENERIC | SPLIT, "edges"),
    "split16384_right": _c(16384, R, GENERIC | SPLIT),
    "split16384_merge": _c(16384, MERGE, GENERIC | SPLIT, "noise"),
    "split16384_side": _c(16384, SIDE, GENERIC | SPLIT, "same"),
    "split16384_merge_fetch": _c(16384, MERGE, GENERIC | SPLIT, opts=FETCH),
    "split16384_right_bh": _c(16384, R, GENERIC | SPLIT, "edges", **BH),
    "split32768_left": _c(32768, L, FUSED | SPLIT),
    "split32768_right": _c(32768, R, FUSED | SPLIT, "noise"),
    "split32768_merge": _c(32768, MERGE, FUSED | SPLIT, "edges", pairs=3),
    "split32768_side": _c(32768, SIDE, FUSED | SPLIT, "same"),
    "split32768_left_fetch": _c(32768, L, FUSED | SPLIT, "edges", opts=FETCH),
    "split32768_side_bh": _c(32768, SIDE, FUSED | SPLIT, **BH),
    "split65536_left": _c(65536, L, HALVES | SPLIT, frames=3),
    "split65536_right": _c(65536, R, HALVES | SPLIT, "edges", frames=3),
    "split65536_merge": _c(65536, MERGE, HALVES | SPLIT, "same", frames=3),
    "split65536_side": _c(65536, SIDE, HALVES | SPLIT, "same", frames=3),
    "split65536_side_fetch": _c(65536, SIDE, HALVES | SPLIT, "edges", frames=3, opts=FETCH),
    "split65536_merge_bh": _c(65536, MERGE, HALVES | SPLIT, frames=3, **BH),
    # channel-split path, two workgroups per frame: Mid-Side ((l + r) / 2, (l - r) / 2) and Separate
    "split16384_midside": _c(16384, MS, GENERIC | SPLIT, "same"),
    "split32768_midside": _c(32768, MS, FUSED | SPLIT, "quiet"),
    "split32768_midside_fetch": _c(32768, MS, FUSED | SPLIT, "edges", opts=FETCH),
    "split65536_midside": _c(65536, MS, HALVES | SPLIT, "edges", frames=3, pairs=3),
    "split65536_midside_bh": _c(65536, MS, HALVES | SPLIT, "same", frames=3, **BH),
    "split16384_separate": _c(16384, SEP, GENERIC | SPLIT, "edges"),
    "split32768_separate": _c(32768, SEP, FUSED | SPLIT, "quiet"),
}


def _signal(case, S, seed):
    """[2 C][S] float32 input of a case"""
    C, N, mode, kind = case["pairs"], case["N"], case["mode"], case["signal"]
    sr = int(case["cfg"].get("sample_rate", 48000))
    if kind == "noise":
        return np.random.default_rng(seed).uniform(-1, 1, (2 * C, S)).astype(np.float32)
    g = synth.gen(seed, sr, S, 4 * C)
    x = g[:2 * C].copy()
    if kind == "quiet":
        x[1::2] = g[2 * C::2] * np.float32(1e-4)
    elif kind == "same":
        x[1::2] = x[0::2] + np.float32(1e-3) * g[2 * C::2]
    elif kind == "edges":
        n = np.arange(S)
        tone = np.cos(2 * np.pi * (N // 2 - 1) * n / N)
        nyq = 0.5 * np.cos(np.pi * n) + 0.25
        if mode in MONO:
            s = nyq + 0.3 * tone                                  # the signal the mono mode transforms
            l, r = {L: (s, tone), R: (tone, s), MERGE: (s, s), SIDE: (s, -s)}[mode]
        elif mode == CPLX:
            l, r = nyq, 0.3 * np.cos(np.pi * n) - 0.2
        else:
            l, r = tone + 0.5, nyq
        x[0::2] = (l + 0.01 * g[0:2 * C:2]).astype(np.float32)    # (a little of synth.gen: the pairs differ)
        x[1::2] = (r + 0.01 * g[1:2 * C:2]).astype(np.float32)
    return x


def _poison_next(gpu, shape):
    from test_gpu_full_size import _poison_next as poison
    return poison(gpu, shape)


def _compared(mode, ref, split_mono):
    """what sgz_stage_bins reports for the restated csf (sgz.h): signed csf[0] / csf[N] in Separate / Mid-Side, complex csf in Phase,
    the magnitude of every entry the map leaves complex in the mono modes and Complex -- but csf[N/2] = X[N/2] / 2 signed (real for a
    real signal) from the channel-split kernel's mono form"""
    if mode in (SEP, MS):
        return ref.real
    if mode == PHASE:
        return ref
    want = np.abs(ref)
    if split_mono:
        N = ref.shape[-1] - 1
        want[..., N // 2] = ref[..., N // 2].real
    return want


@pytest.mark.parametrize("name", list(CASES))
def test_bins_against_fp64(gpu, name):
    import torch
    from fp64_bins import mode_bins, window
    case = CASES[name]
    N, W, hop, mode, C, F = case["N"], case["W"], case["hop"], case["mode"], case["pairs"], case["frames"]
    cfg = config.spectrum_config(window_size=W, hop=hop, channel_mode=mode, num_pairs=C, **case["cfg"])
    plan = api.Plan(cfg)
    for o, v in case["opts"].items():
        plan.set_option(o, v)
    plan.upload()
    assert plan.N == N
    assert plan.path & ~SIDE_MAP == case["path"], (name, plan.path, case["path"])
    S = W + (F - 1) * hop
    x = _signal(case, S, seed=sum(map(ord, name)))
    assert plan.num_frames(S) == F
    w = window(cfg["window_type"], cfg["window_symmetry"], W, cfg["window_alpha"], cfg["window_beta"])
    shape = (F, C, N + 1, 2) if mode == PHASE else (F, C, N + 1)
    xg = torch.from_numpy(x).to(gpu)                           # (uploaded first: the output must be the next allocation)
    poisoned = _poison_next(gpu, shape)
    bins = plan.stage_bins(xg)
    assert bins.data_ptr() == poisoned, (name, "the output did not land on the NaN-filled block")
    got = bins.cpu().numpy()
    del bins, xg
    if mode == PHASE:
        got = got[..., 0] + 1j * got[..., 1].astype(np.float64)
    split_mono = mode in MONO and bool(case["path"] & SPLIT)
    upto = N // 2 + 1 if split_mono else N + 1                 # the channel-split mono form writes csf[0 .. N/2] (sgz.h)
    special = (0, N // 2 - 1, N // 2, N) if mode in (SEP, MS, PHASE) else (0, N // 2)
    starts = np.arange(F)[:, None] * hop + np.arange(W)
    worst, worst_at = 0.0, None
    worst_k = dict.fromkeys(special, 0.0)
    for c in range(C):
        ref, scale = mode_bins(mode, x[2 * c][starts], x[2 * c + 1][starts], w, N)
        g = got[:, c, :upto]
        assert np.isfinite(g).all(), (name, "non-finite bins (an entry the launch never wrote)", c,
                                      np.argwhere(~np.isfinite(g))[:5].tolist())
        rel = np.abs(g - _compared(mode, ref, split_mono)[:, :upto]) / scale[:, None]
        i = np.unravel_index(int(rel.argmax()), rel.shape)
        if rel[i] > worst:
            worst, worst_at = float(rel[i]), (int(i[0]), c, int(i[1]))
        for k in special:
            worst_k[k] = max(worst_k[k], float(rel[:, k].max()))
        if case["signal"] == "edges":                          # the special entries really are large here
            for k in special:
                assert (np.abs(ref[:, k]) > 0.05 * scale).all(), (name, k)
        if mode in MONO + (CPLX,) and upto == N + 1:
            assert (g[:, N] == 0).all(), (name, "csf[N] of a mono / Complex frame", g[:, N])
        if split_mono:                                          # left untouched (sgz.h): still the poison
            assert np.isnan(got[:, c, upto:]).all(), (name, "the channel-split mono form wrote csf[N/2 + 1 .. N]")
    msg = f"{name} (path {plan.path}, {F} frames x {C} pairs): worst err / scale {worst:.3g} at (frame, pair, bin) {worst_at}; " \
          f"entries {', '.join(f'csf[{k}] {v:.3g}' for k, v in worst_k.items())}"
    print(msg)
    assert worst <= BIN_TOL, msg
    for k in special:
        assert worst_k[k] <= BIN_TOL, (k, msg)
