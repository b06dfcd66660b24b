"""The cross overview's render on the GPU (sgz_spectrogram_overview_cross_device / _host: K_A's complex bins slab by slab, then the reduction).
  1  _host on synthetic stereo (N = 1024, hop 256, 2 pairs, 64 frames) == the restatement (tests/overview_cross_ref.py) applied to
     Plan.stage_bins of the same audio, byte for byte; the device form the same;
  2  the same bytes with SGZ_OPT_OVERVIEW_SLAB = 1, 3 and default: a frame's bins do not depend on what shares its launch;
  3  against tests/fp64_bins.py (phase_split, imported): each sum of each band within a bar derived from the bar test_gpu_bins_fp64 holds
     the kernels to.  Per bin delta = 4e-6 x the frame's scale; |d ll| <= sum over the band's bin-frames of (2 |L| delta + delta^2), likewise
     rr; for re and im the term is ((|L| + |R|) delta + delta^2); each scaled by s = 2^(62 - 2n), plus 0.5 per bin-frame for the rounding.
     The bar is computed from the fp64 values alone;
  4  known answer: L a sum of unit sines on exact bins under a rectangular full window, R = L delayed by d = 3 samples: the one-bin bands at
     those bins read coherence >= 1 - 1e-4 and phase = 2 pi k d / N (mod 2 pi) within delta (|L| + |R|) / |L conj R| rad; R = -L reads
     correlation <= -1 + 1e-4;
  5  the refusals: other channel modes, RSNT, no band table; fewer samples than a window."""
import math
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_cross_ref as ocr  # noqa: E402
from fp64_bins import _transform, phase_split, window  # noqa: E402

pytestmark = pytest.mark.gpu

N, HOP, PAIRS, FRAMES = 1024, 256, 2, 64
S = N + (FRAMES - 1) * HOP
BIN_TOL = 4e-6                                               # tests/test_gpu_bins_fp64.py BIN_TOL
SCALE = 2.0 ** (62 - 2 * 10)


def _cfg(**over):
    return config.spectrum_config(**{**dict(window_size=N, hop=HOP, axis_points=65, num_pairs=PAIRS, channel_mode=config.CH_PHASE,
                                            bin_interp=config.INTERP_LINEAR), **over})


def _audio():
    """float32 [4][S]: two stereo pairs of tones, a sweep and noise, the channels of a pair related but not equal"""
    rng = np.random.default_rng(42)
    t = np.arange(S) / 48000.0
    tone = 0.4 * np.sin(2 * np.pi * 997.0 * t) + 0.2 * np.sin(2 * np.pi * (200.0 + 4000.0 * t) * t)
    noise = rng.standard_normal((4, S)) * 0.05
    x = np.stack([tone + noise[0], 0.7 * np.roll(tone, 5) + noise[1], noise[2] + 0.3 * np.sin(2 * np.pi * 5000.0 * t), 0.5 * noise[2] + noise[3]])
    return np.ascontiguousarray(x, np.float32)


@pytest.fixture(scope="module")
def scene(gpu):
    import torch
    cfg = _cfg()
    plan = api.Plan(cfg).upload()
    x = _audio()
    assert plan.num_frames(S) == FRAMES and plan.N == N
    d_x = torch.from_numpy(x).to(gpu)
    bins = plan.stage_bins(d_x).cpu().numpy()
    tables = {"thirds": [int(e) for e in api.cross_edges_octave(48000.0, N, 3, 20.0, 20000.0)[0]], "bins": list(range(1, N // 2))}
    return dict(cfg=cfg, plan=plan, x=x, d_x=d_x, bins=bins, tables=tables)


@pytest.mark.parametrize("table", ["thirds", "bins"])
def test_host_render_equals_the_restatement_on_the_staged_bins(scene, table):
    plan, edges = scene["plan"], scene["tables"][table]
    plan.set_cross_edges(edges)
    each = ocr.records_of(scene["bins"], N, edges)
    assert not each["skipped"].any()
    for k in (1, 4, 5, 64, 100):
        want = ocr.columns_of(each, k)[0]
        got, timing = plan.overview_cross(scene["x"], k)
        assert timing["frames"] == FRAMES and ocr.same(got, want), (table, k)
        assert ocr.same(api.cross_from_device(plan.overview_cross(scene["d_x"], k)), want), (table, k)
    assert int(want["count"].sum()) == FRAMES * PAIRS * (edges[-1] - edges[0])


def test_the_slab_does_not_change_the_bytes(scene):
    plan, edges = scene["plan"], scene["tables"]["thirds"]
    plan.set_cross_edges(edges)
    each = ocr.records_of(scene["bins"], N, edges)
    try:
        for k in (4, 5):
            want = ocr.columns_of(each, k)[0]
            for slab in (1, 3, 0):
                plan.set_option(api.OPT_OVERVIEW_SLAB, slab)
                assert ocr.same(plan.overview_cross(scene["x"], k)[0], want), (k, slab)
                assert ocr.same(api.cross_from_device(plan.overview_cross(scene["d_x"], k)), want), (k, slab)
    finally:
        plan.set_option(api.OPT_OVERVIEW_SLAB, 0)


def _fp64_bins(cfg, x):
    """(L, R complex128 [frames][pairs][N/2 - 2] at the admitted bins, delta [frames][pairs]) from tests/fp64_bins.py"""
    w = window(cfg["window_type"], cfg["window_symmetry"], N, cfg["window_alpha"], cfg["window_beta"])
    starts = np.arange(FRAMES)[:, None] * HOP + np.arange(N)
    L, R, delta = [], [], []
    for c in range(x.shape[0] // 2):
        l, r = x[2 * c].astype(np.float64)[starts], x[2 * c + 1].astype(np.float64)[starts]
        csf = phase_split(_transform(l + 1j * r, w, N), N)
        L.append(csf[:, 1:N // 2 - 1])
        R.append(csf[:, N - 1:N // 2 + 1:-1])
        delta.append(BIN_TOL * np.abs(csf).max(axis=-1))
    return np.stack(L, 1), np.stack(R, 1), np.stack(delta, 1)


@pytest.mark.parametrize("table", ["thirds", "bins"])
def test_sums_against_the_fp64_bins(scene, table):
    """figures of one run (MI355X) are in the failure message's format: the worst |difference| / bar per field"""
    plan, cfg, edges = scene["plan"], scene["cfg"], scene["tables"][table]
    plan.set_cross_edges(edges)
    k = 4
    got = plan.overview_cross(scene["x"], k)[0]
    L, R, delta = _fp64_bins(cfg, scene["x"])
    d = delta[:, :, None]
    aL, aR = np.abs(L), np.abs(R)
    cross = L * np.conj(R)
    values = {"ll": aL * aL, "rr": aR * aR, "re": cross.real, "im": cross.imag}
    bars = {"ll": 2 * aL * d + d * d, "rr": 2 * aR * d + d * d, "re": (aL + aR) * d + d * d, "im": (aL + aR) * d + d * d}
    e = np.asarray(edges)
    columns = FRAMES // k

    def banded(v):                                            # [frames][pairs][bins] -> [columns][pairs][bands]: sums over a column's frames and a band's bins
        cs = np.concatenate([np.zeros_like(v[:, :, :1]), np.cumsum(v, axis=2)], axis=2)
        b = cs[:, :, e[1:] - 1] - cs[:, :, e[:-1] - 1]
        return b.reshape(columns, k, *b.shape[1:]).sum(axis=1)

    count = got["count"].astype(np.float64)
    assert np.array_equal(got["count"], np.broadcast_to((k * np.diff(e)).astype(np.uint64), got["count"].shape)) and not got["skipped"].any()
    worst = {}
    for name in ocr.SUMS:
        have = ocr.sums(got, name).astype(np.float64)
        want = banded(values[name]) * SCALE
        bar = banded(bars[name]) * SCALE + 0.5 * count
        ratio = np.abs(have - want) / np.maximum(bar, 1e-300)
        worst[name] = float(np.where(count > 0, ratio, 0.0).max())
    print("cross overview against fp64, worst |difference| / bar:", table, worst)
    assert all(v <= 1.0 for v in worst.values()), worst


def test_known_answer_delay_and_inversion(gpu):
    d = 3
    ks = (5, 40, 100, 300)
    cfg = _cfg(window_type=config.WIN_RECT)
    plan = api.Plan(cfg).upload()
    n = np.arange(S + d)
    tones = sum(np.sin(2 * np.pi * k * n / N + 0.3 * k) for k in ks)          # unit sines on exact bins: periodic in N
    Lx, Rx = tones[d:], tones[:-d]                                            # R[n] = L[n - d]: L leads
    x = np.ascontiguousarray(np.stack([Lx, Rx, Lx, -Lx]), np.float32)
    edges = sorted(e for k in ks for e in (k, k + 1))
    plan.set_cross_edges(edges)
    got, _ = plan.overview_cross(x, 4)
    r = api.overview_cross_readout(got)
    unit = plan.overview_cross_unit()
    assert unit == 1.0
    # the bar of the phase from fp64 values: |L| = |R| = N/2, the frame's scale the largest |csf| = N/2 (a unit sine under a rectangular window)
    Lmag = Rmag = N / 2
    delta = BIN_TOL * (N / 2)
    bar = delta * (Lmag + Rmag) / (Lmag * Rmag)
    for i, k in enumerate(ks):
        band = 2 * i
        assert (got["count"][:, :, band] == 4).all()
        assert (r["coherence"][:, 0, band] >= 1 - 1e-4).all(), (k, r["coherence"][:, 0, band])
        want = 2 * math.pi * k * d / N
        diff = np.angle(np.exp(1j * (r["phase"][:, 0, band] - want)))
        assert (np.abs(diff) <= bar).all(), (k, float(np.abs(diff).max()), bar)
        assert (np.abs(r["ll"][:, 0, band] * unit - 1.0) < 1e-4).all()        # a full-scale sine reads unit power
        assert (r["correlation"][:, 1, band] <= -1 + 1e-4).all(), (k, r["correlation"][:, 1, band])
        assert (r["side"][:, 1, band] * unit > 0.99).all() and (r["mid"][:, 1, band] * unit < 1e-6).all()
    assert r["phase"][0, 0, 0] > 0                                            # positive where L leads


def test_refusals_and_short_input(scene, gpu):
    import torch
    L = api.lib()
    x, d_x = scene["x"], scene["d_x"]
    out = torch.full((64, PAIRS, 40, 10), 0x5A5A5A5A, dtype=torch.int64, device=gpu)
    host = np.zeros((64, PAIRS, 40), api.OVERVIEW_CROSS_DTYPE)
    import ctypes as C
    ptrs = (C.c_void_p * 4)(*[x[i].ctypes.data for i in range(4)])
    for over in (dict(channel_mode=config.CH_SEPARATE), dict(channel_mode=config.CH_MIDSIDE), dict(algorithm=config.ALGO_RSNT),
                 dict(channel_mode=config.CH_SEPARATE, algorithm=config.ALGO_RSNT)):
        other = api.Plan(_cfg(**over)).upload()
        assert L.sgz_spectrogram_overview_cross_device(other.h, d_x.data_ptr(), d_x.stride(0), S, 4, out.data_ptr(), None) == api.SGZ_EUNSUPPORTED, over
        assert L.sgz_spectrogram_overview_cross_host(other.h, ptrs, 4, S, 4, host.ctypes.data, None) == api.SGZ_EUNSUPPORTED, over
    bare = api.Plan(_cfg()).upload()                                          # a Phase plan without a band table
    assert L.sgz_spectrogram_overview_cross_device(bare.h, d_x.data_ptr(), d_x.stride(0), S, 4, out.data_ptr(), None) == api.SGZ_EINVAL
    assert L.sgz_spectrogram_overview_cross_host(bare.h, ptrs, 4, S, 4, host.ctypes.data, None) == api.SGZ_EINVAL
    plan = scene["plan"]
    plan.set_cross_edges(scene["tables"]["thirds"])
    assert L.sgz_spectrogram_overview_cross_device(plan.h, d_x.data_ptr(), d_x.stride(0), S, 0, out.data_ptr(), None) == api.SGZ_EINVAL
    # fewer samples than a window: SGZ_SKIPPED_FRAME, nothing written
    assert plan.overview_cross(x[:, :N - 1].copy(), 4) is None
    assert L.sgz_spectrogram_overview_cross_device(plan.h, d_x.data_ptr(), d_x.stride(0), N - 1, 4, out.data_ptr(), None) == api.SGZ_SKIPPED_FRAME
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A5A5A).all()) and not host.view(np.uint8).any()
