"""The wave priorities of a ONE-ROUND image-only launch (spectrum_real.hip "one-round shape"; kernels.hpp RealParams::prioFirst / prioMate /
prioNy / prioScope and their SGZ_PRIO_* defaults): the two channel workgroups of a doubled CU and the Nyquist role may run at different
priorities behind their first requests.  Like the rest of that schedule it is a speed assumption only: every byte of the image and
every Nyquist word must be what the two-channel launch (SGZ_OPT_IMAGE_ONLY_SPLIT = 0) gives, whatever the build's defaults are.
Frame counts around the shape window, from the device's CU count: no second workgroup on any CU, exactly one doubled CU, a partial
set whose XCDs get unequal shares, the window's last frame count (2 #CUs - 1 channel workgroups: the Nyquist workgroups no longer fit
the round and spill into a second generation) and a launch past the window.  Before each compared render a DIFFERENT signal goes through
the same plan, so that a skipped frame shows as a stale row.  The same frames through an sgz_render_queue of depth 2 (pipelined
launches, which take none of the rules)."""
import functools

import numpy as np
import pytest

from signalizer_amd import api, config, synth

pytestmark = pytest.mark.gpu

HOP = 8192
N = 32768
CASES = ("below", "one_mate", "partial", "last", "past")


def _frames(case: str) -> int:
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return {"below": cus - 1, "one_mate": cus + 1, "partial": cus + 43, "last": 2 * cus - 1, "past": 2 * cus + 3}[case]


@functools.lru_cache(maxsize=None)
def _signal(seed: int, frames: int) -> np.ndarray:
    """stereo signal with a strong (-1)^n component in the right channel: csf[N/2] wins the top pixels of many frames"""
    x = synth.gen(seed, 48000, N + (frames - 1) * HOP, 2).astype(np.float32)
    x[1] += np.float32(0.6) * np.where(np.arange(x.shape[1]) % 2 == 0, 1.0, -1.0).astype(np.float32)
    return x


def _plan(option: int):
    plan = api.Plan(config.spectrum_config())
    plan.set_option(api.OPT_IMAGE_ONLY_SPLIT, option)
    return plan.upload()


@functools.lru_cache(maxsize=None)
def _reference(case: str):
    """the two-channel launch's image and Nyquist words of the case's signal, computed once"""
    import torch
    frames = _frames(case)
    x = torch.from_numpy(_signal(3, frames)).to("cuda:0")
    plan = _plan(0)
    rgba = plan.render(x).cpu().numpy()
    ny, ny_frames, low = plan.stage_nyquist(x, False)
    torch.cuda.synchronize()
    assert ny_frames == 0 and low == 0 and plan.N == N and plan.num_frames(x.shape[1]) == frames
    rgba.setflags(write=False)
    return rgba, ny.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("option", [1, 2, 37])
@pytest.mark.parametrize("case", CASES)
def test_priorities_change_no_byte(gpu, case, option):
    import torch
    frames = _frames(case)
    want_rgba, want_ny = _reference(case)
    x = torch.from_numpy(_signal(3, frames)).to(gpu)
    other = torch.from_numpy(_signal(19, frames)).to(gpu)
    plan = _plan(option)
    # a different signal first, through the same plan and the same buffers
    stale = plan.render(other).cpu().numpy()
    assert (stale != want_rgba).any(axis=(1, 2)).sum() >= frames // 2
    got = plan.render(x).cpu().numpy()
    assert got.shape == want_rgba.shape
    bad = np.nonzero((got != want_rgba).any(axis=(1, 2)))[0]
    assert bad.size == 0, (bad.size, bad[:8].tolist())
    plan.stage_nyquist(other, True)
    ny, ny_frames, low = plan.stage_nyquist(x, True)
    torch.cuda.synchronize()
    assert low == 0 and ny_frames >= 1 and (option == 1 or ny_frames == min(option, frames)), (ny_frames, low)      # the image-only form was taken
    ny = ny.cpu().numpy().view(np.uint32)
    assert ny.size == want_ny.size
    bad = np.nonzero((ny != want_ny).reshape(frames, -1).any(axis=1))[0]
    assert bad.size == 0, (bad.size, bad[:8].tolist())


@pytest.mark.parametrize("option", [1, 2, 37])
@pytest.mark.parametrize("case", CASES)
def test_render_queue_lanes_same_bytes(gpu, case, option):
    """depth 2: each lane renders the other signal, then the compared one (submits go round-robin over the lanes)"""
    import torch
    frames = _frames(case)
    want_rgba, _ = _reference(case)
    x = torch.from_numpy(_signal(3, frames)).to(gpu)
    other = torch.from_numpy(_signal(19, frames)).to(gpu)
    q = api.RenderQueue(config.spectrum_config(), 2).set_option(api.OPT_IMAGE_ONLY_SPLIT, option)
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
