"""The flux overview's render on the GPU (sgz_spectrogram_overview_flux_device / _host; csrc/api.hip runOverviewFluxSlabs): the records equal
the restatement (tests/overview_flux_ref.py) applied to Plan.stage_mapped of the same audio, byte for byte -- small plans in Left, Merge,
Separate and MidSide (N = 256, P = 97, hop 64, 40 frames) and one N = 32768 channel-split plan of a dozen frames, where the render must
complete the late pixels as sgz_stage_mapped does.  The bytes do not depend on the slab.  Phase and RSNT plans are refused with the device
untouched.  Two derived properties, no measured number in either: the frame of a column's strongest onset under unit clicks, and the centroid
of a bin-centred sine."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_ref as ov  # noqa: E402
import overview_flux_ref as ofr  # noqa: E402
from test_gpu_overview import Guarded, _stream  # noqa: E402

pytestmark = pytest.mark.gpu

RW = 22
SPLIT = 8                                                    # SGZ_PATH_* (sgz.h)
SMALL = dict(window_size=256, hop=64, axis_points=97)
CASES = {
    "left": dict(cfg=dict(SMALL, channel_mode=config.CH_LEFT), frames=40),
    "merge": dict(cfg=dict(SMALL, channel_mode=config.CH_MERGE), frames=40),
    "separate": dict(cfg=dict(SMALL, channel_mode=config.CH_SEPARATE), frames=40),
    "midside_two_pairs": dict(cfg=dict(SMALL, channel_mode=config.CH_MIDSIDE, num_pairs=2), frames=40),
    "n32768_split": dict(cfg=dict(window_size=32768, hop=8192), frames=12, path=SPLIT),
}
SLABS = (1, 5, 0)
_refs = {}


def _case(name, gpu):
    """(plan, planar, its device copy, Plan.stage_mapped of it as [F][rows][P], the restatement's frame terms) -- made once"""
    if name not in _refs:
        import torch
        case = CASES[name]
        cfg = config.spectrum_config(**case["cfg"])
        plan = api.Plan(cfg).upload()
        if "path" in case:
            assert plan.path & case["path"] == case["path"], (name, plan.path)
        x = ov.burst_signal(cfg["window_size"], cfg["hop"], case["frames"], 2 * cfg["num_pairs"], cfg["sample_rate"], seed=5)
        assert plan.num_frames(x.shape[1]) == case["frames"]
        d_x = torch.from_numpy(x).to(gpu)
        mapped = plan.stage_mapped(d_x).cpu().numpy().reshape(case["frames"], plan.C * plan.sides, plan.P)
        _refs[name] = (plan, x, d_x, mapped, ofr.frame_terms(mapped))
    return _refs[name]


def _same(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("name", list(CASES))
def test_flux_render_equals_stage_mapped_then_restatement(gpu, name):
    import torch
    plan, x, d_x, mapped, terms = _case(name, gpu)
    F = mapped.shape[0]
    assert not np.isnan(mapped).any() and (mapped > 0).any()
    for k in sorted({1, 4, 7, F, F + 3}):
        want = ofr.overview(mapped, k, terms=terms)[0].reshape(-1, plan.C, plan.sides)
        for slab in SLABS:
            plan.set_option(api.OPT_OVERVIEW_SLAB, slab)
            got = api.flux_from_device(plan.overview_flux(d_x, k))
            assert _same(got, want), (name, k, slab)
            h, timing = plan.overview_flux(x, k)
            assert _same(h, want) and timing["frames"] == F, (name, k, slab)
    plan.set_option(api.OPT_OVERVIEW_SLAB, 0)
    # stage_mapped is unchanged by the renders in between (they use the plan's scratch, never the caller's buffers)
    assert np.array_equal(plan.stage_mapped(d_x).cpu().numpy().view(np.uint32).reshape(mapped.shape), mapped.view(np.uint32))
    torch.cuda.synchronize()


def test_only_the_columns_are_written_and_a_short_input_is_skipped(gpu):
    import torch
    plan, x, d_x, mapped, terms = _case("separate", gpu)
    L = api.lib()
    k = 7
    want = ofr.overview(mapped, k, terms=terms)[0]
    columns, rows = want.shape
    out = Guarded(gpu, columns, rows * RW, torch.int32)
    assert L.sgz_spectrogram_overview_flux_device(plan.h, d_x.data_ptr(), d_x.stride(0), x.shape[1], k, out.ptr, _stream()) == api.SGZ_OK
    torch.cuda.synchronize()
    assert np.ascontiguousarray(out.payload()).tobytes() == want.tobytes()
    S = plan.cfg.window_size - 1
    xs = np.ascontiguousarray(x[:, :S])
    d_xs = torch.from_numpy(xs).to(gpu)
    out = Guarded(gpu, 1, rows * RW, torch.int32)
    st = L.sgz_spectrogram_overview_flux_device(plan.h, d_xs.data_ptr(), d_xs.stride(0), S, k, out.ptr, _stream())
    torch.cuda.synchronize()
    assert st == api.SGZ_SKIPPED_FRAME and out.untouched()
    assert plan.overview_flux(xs, k) is None and plan.overview_flux(d_xs, k) is None


@pytest.mark.parametrize("over", [dict(channel_mode=config.CH_PHASE), dict(algorithm=config.ALGO_RSNT)], ids=["phase", "rsnt"])
def test_phase_and_rsnt_are_refused(gpu, over):
    import torch
    cfg = config.spectrum_config(window_size=1024, hop=256, axis_points=128, **over)
    plan = api.Plan(cfg).upload()
    L = api.lib()
    x = ov.burst_signal(1024, 256, 9, 2, seed=1)
    d_x = torch.from_numpy(x).to(gpu)
    out = Guarded(gpu, 12, 2 * RW, torch.int32)
    st = L.sgz_spectrogram_overview_flux_device(plan.h, d_x.data_ptr(), d_x.stride(0), x.shape[1], 1, out.ptr, _stream())
    torch.cuda.synchronize()
    assert st == api.SGZ_EUNSUPPORTED and out.untouched()
    with pytest.raises(api.SgzError) as e:
        plan.overview_flux(x, 2)
    assert e.value.status == api.SGZ_EUNSUPPORTED
    # the plan renders as before
    assert plan.render(d_x).shape[0] == plan.num_frames(x.shape[1])
    torch.cuda.synchronize()


def test_click_timing(gpu):
    """silence with unit clicks under a rectangular window, one click per column: flux_at of each column is ceil((n - N + 1) / hop) clamped at
    0, the first frame whose window holds the click at sample n.  (Every click lies behind the first window: frame 0 has no predecessor, hence
    no onset, by the definition.)  A click stays in N / hop = 4 windows and k = 8, so no two clicks share a frame."""
    N, hop, k, columns = 256, 64, 8, 6
    cfg = config.spectrum_config(window_size=N, hop=hop, axis_points=97, channel_mode=config.CH_LEFT, window_type=config.WIN_RECT)
    plan = api.Plan(cfg).upload()
    frames = k * columns
    S = N + hop * (frames - 1)
    x = np.zeros((2, S), np.float32)
    first = [c * k + j for c, j in enumerate((1, 7, 4, 3, 4, 2))]                 # the frame each click enters at: one per column, anywhere in it
    clicks = [(f - 1) * hop + N + d for f, d in zip(first, (0, 63, 17, 1, 62, 30))]     # in frame f's window and not in frame f - 1's
    for n in clicks:
        x[0, n] = 1.0
    assert plan.num_frames(S) == frames
    recs, _ = plan.overview_flux(x, k)
    want = [max(0, -(-(n - N + 1) // hop)) for n in clicks]
    assert want == first
    assert [int(v) for v in recs["flux_at"][:, 0, 0]] == want
    assert (recs["flux_max"][:, 0, 0] > 0).all() and (recs["count"] == k).all() and not recs["nans"].any()


def test_the_centroid_of_a_bin_centred_sine(gpu):
    """rectangular window, interpolation None: every pixel shows the bin nearest to its mapped frequency, so the centroid lies within the run of
    pixels the plan's mapped frequencies assign to the sine's bin (the run is computed here from sgz_plan_get_mapped_frequencies)"""
    N, hop, P, sr = 256, 64, 197, 48000.0
    cfg = config.spectrum_config(window_size=N, hop=hop, axis_points=P, channel_mode=config.CH_LEFT, window_type=config.WIN_RECT,
                                 bin_interp=config.INTERP_NONE, sample_rate=sr)
    plan = api.Plan(cfg).upload()
    mf = plan.mapped_frequencies()
    to_bin = np.float32(np.float32(N // 2) / np.float32(sr / 2))
    bins = np.floor((mf * to_bin).astype(np.float64) + 0.5).astype(np.int64)
    brk = int(api.lib().sgz_plan_break_pixel(plan.h))
    frames = 9
    S = N + hop * (frames - 1)
    n = np.arange(S)
    for b in (3, 5, 8):
        run = np.flatnonzero(bins[:brk] == b)
        assert run.size >= 2 and (np.diff(run) == 1).all() and run[-1] < brk, (b, run, brk)
        x = np.zeros((2, S), np.float32)
        x[0] = np.sin(2 * np.pi * b * n / N + 0.3).astype(np.float32)
        recs, _ = plan.overview_flux(x, frames)
        _, centroid, spread, _, _ = api.overview_flux_readout(recs, P)
        assert run[0] <= centroid[0, 0, 0] <= run[-1], (b, run, centroid)
        assert spread[0, 0, 0] <= run.size, (b, run, spread)
        assert plan.overview_flux_hz(centroid)[0, 0, 0] >= mf[run[0]] and plan.overview_flux_hz(centroid)[0, 0, 0] <= mf[run[-1]]
