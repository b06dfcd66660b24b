"""The Nyquist workgroups of an image-only launch fetch each right-channel row once per workgroup (spectrum_real.hip nyquistUnit, "shared
rows"): where the hop is four whole rows of 2048 samples and a workgroup has more than one frame, a thread keeps its column pair's sixteen
raw rows as a window that slides by four rows per frame and requests only the four new ones.  Only the loads differ, so every Nyquist word
(compared as uint32) and every image byte must be what the two-channel launch (SGZ_OPT_IMAGE_ONLY_SPLIT = 0) gives.
Shapes are the smallest at which the sliding window can go wrong: a single frame (no reuse), two and three frames, four and five (a whole
window of rows turns over), workgroup sizes above the frame count, short last workgroups (frames % F != 0).  Two plans beside them: a hop
that is no whole number of rows (the form that requests every row of every frame) and a plan that fetches its window (the image-only form
stands aside).  Then the one-round shape's five frame counts (tests/test_gpu_image_only_priority.py), through plain renders and through
an sgz_render_queue of depth 2.  The signal is that file's: a strong (-1)^n component in the right channel, so that csf[N/2] wins the top
pixels of many frames; before each compared render a DIFFERENT signal goes through the same plan, so that a stale row or word shows."""
import functools

import numpy as np
import pytest

from signalizer_amd import api, config, synth

pytestmark = pytest.mark.gpu

N = 32768
HOP = 8192                       # four rows of 2048 samples: the shared-row form
ODD_HOP = 5000                   # no whole number of rows
FRAMES = (1, 2, 3, 4, 5, 7, 9)
OPTIONS = (1, 2, 3, 4, 5, 37)    # 1: the automatic size; n >= 2: n frames per Nyquist workgroup (capped at the frame count)
ROUND_CASES = ("below", "one_mate", "partial", "last", "past")


@functools.lru_cache(maxsize=None)
def _signal(seed: int, frames: int, hop: int = HOP) -> np.ndarray:
    x = synth.gen(seed, 48000, N + (frames - 1) * hop, 2).astype(np.float32)
    x[1] += np.float32(0.6) * np.where(np.arange(x.shape[1]) % 2 == 0, 1.0, -1.0).astype(np.float32)
    return x


@functools.lru_cache(maxsize=None)
def _plan(option: int, hop: int = HOP, fetch_window: bool = False):
    plan = api.Plan(config.spectrum_config(hop=hop))
    plan.set_option(api.OPT_IMAGE_ONLY_SPLIT, option)
    if fetch_window:
        plan.set_option(api.OPT_FETCH_WINDOW, 1)
    return plan.upload()


@functools.lru_cache(maxsize=None)
def _reference(frames: int, hop: int = HOP, fetch_window: bool = False):
    """image and Nyquist words of the two-channel launch, computed once per shape"""
    import torch
    x = torch.from_numpy(_signal(3, frames, hop)).to("cuda:0")
    plan = _plan(0, hop, fetch_window)
    rgba = plan.render(x).cpu().numpy()
    ny, ny_frames, low = plan.stage_nyquist(x, False)
    torch.cuda.synchronize()
    assert ny_frames == 0 and low == 0 and plan.N == N and plan.num_frames(x.shape[1]) == frames
    rgba.setflags(write=False)
    return rgba, ny.cpu().numpy().view(np.uint32)


def _compare(gpu, frames: int, option: int, hop: int = HOP, fetch_window: bool = False):
    """renders and Nyquist words of the plan with `option` against the two-channel launch; returns the launch's frames per Nyquist
    workgroup (0: the image-only form stood aside)"""
    import torch
    want_rgba, want_ny = _reference(frames, hop, fetch_window)
    x = torch.from_numpy(_signal(3, frames, hop)).to(gpu)
    other = torch.from_numpy(_signal(19, frames, hop)).to(gpu)
    plan = _plan(option, hop, fetch_window)
    stale = plan.render(other).cpu().numpy()                       # a different signal first, through the same plan and buffers
    assert (stale != want_rgba).any(axis=(1, 2)).sum() >= (frames + 1) // 2
    got = plan.render(x).cpu().numpy()
    plan.stage_nyquist(other, True)
    ny, ny_frames, low = plan.stage_nyquist(x, True)
    torch.cuda.synchronize()
    form = "the image-only form stood aside (ny_frames == 0)" if ny_frames == 0 else f"image-only form, {ny_frames} frames per Nyquist workgroup"
    assert low == 0, (form, low)
    assert got.shape == want_rgba.shape, form
    bad = np.nonzero((got != want_rgba).any(axis=(1, 2)))[0]
    assert bad.size == 0, (form, "image rows differ", bad.size, bad[:8].tolist())
    ny = ny.cpu().numpy().view(np.uint32)
    assert ny.size == want_ny.size, form
    bad = np.nonzero((ny != want_ny).reshape(frames, -1).any(axis=1))[0]
    assert bad.size == 0, (form, "Nyquist words differ", bad.size, bad[:8].tolist())
    return ny_frames


@pytest.mark.parametrize("option", OPTIONS)
@pytest.mark.parametrize("frames", FRAMES)
def test_shared_rows_same_words_and_bytes(gpu, frames, option):
    ny_frames = _compare(gpu, frames, option)
    assert ny_frames >= 1, "the image-only form stood aside (ny_frames == 0) on a plan that takes it"
    assert option == 1 or ny_frames == min(option, frames), (ny_frames, option, frames)     # forced sizes stay exactly F frames


@pytest.mark.parametrize("option", [1, 3, 5])
@pytest.mark.parametrize("frames", [5, 7])
def test_hop_of_no_whole_rows_requests_every_row(gpu, frames, option):
    """hop 5000: frame f + 1's rows are not rows of frame f; the role requests all sixteen rows of every frame, as it did"""
    ny_frames = _compare(gpu, frames, option, hop=ODD_HOP)
    assert ny_frames >= 1, "the image-only form stood aside (ny_frames == 0) on a plan that takes it"


@pytest.mark.parametrize("option", [1, 3])
def test_fetched_window_plan(gpu, option):
    """SGZ_OPT_FETCH_WINDOW: the Nyquist role evaluates its window, so a plan that fetches it keeps the two-channel launch"""
    ny_frames = _compare(gpu, 7, option, fetch_window=True)
    assert ny_frames == 0, f"a fetched-window plan took the image-only form ({ny_frames} frames per Nyquist workgroup)"


def _round_frames(case: str) -> int:
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return {"below": cus - 1, "one_mate": cus + 1, "partial": cus + 43, "last": 2 * cus - 1, "past": 2 * cus + 3}[case]


@pytest.mark.parametrize("case", ROUND_CASES)
def test_one_round_shape_renders(gpu, case):
    ny_frames = _compare(gpu, _round_frames(case), 1)
    assert ny_frames >= 1, "the image-only form stood aside (ny_frames == 0) on a plan that takes it"


@pytest.mark.parametrize("case", ROUND_CASES)
def test_one_round_shape_render_queue(gpu, case):
    """depth 2: each lane renders the other signal, then the compared one (submits go round-robin over the lanes)"""
    import torch
    frames = _round_frames(case)
    want_rgba, _ = _reference(frames)
    x = torch.from_numpy(_signal(3, frames)).to(gpu)
    other = torch.from_numpy(_signal(19, frames)).to(gpu)
    q = api.RenderQueue(config.spectrum_config(), 2).set_option(api.OPT_IMAGE_ONLY_SPLIT, 1)
    outs = [torch.zeros(want_rgba.shape, dtype=torch.uint8, device=gpu) for _ in range(4)]
    torch.cuda.synchronize()                     # the fills and uploads run on torch's stream
    for k, src in enumerate((other, other, x, x)):
        q.submit(src, outs[k])
    q.wait()
    for k in (2, 3):
        got = outs[k].cpu().numpy()
        bad = np.nonzero((got != want_rgba).any(axis=(1, 2)))[0]
        assert bad.size == 0, (k, bad.size, bad[:8].tolist())
    q.close()
