"""Image-only renders of a one-pair Separate plan at N = 32768 (sgz_spectrogram_render_device without lines or state) run the channel-split
K_A in its image-only form: side 0's channel workgroups, and Nyquist workgroups that leave the right channel's Nyquist bin -- the one
number of that channel the image reads, through csf[N/2] = |X_L[M] + i X_R[M]| / 2 -- summed in the transform's own order
(spectrum_real.hip nyquistUnit).  SGZ_OPT_IMAGE_ONLY_SPLIT = 0 keeps the two-channel launch.  The image must be byte-identical either way,
and renders that read more than the image must never take the new form."""
import numpy as np
import pytest

from signalizer_amd import api, config, synth

pytestmark = pytest.mark.gpu

HOP = 8192
N = 32768


def _samples(frames: int) -> int:
    return N + (frames - 1) * HOP


def _signal(seed: int, frames: int, alt_left: float = 0.0, alt_right: float = 0.0) -> np.ndarray:
    """stereo test signal; alt_*: amplitude of a (-1)^n component (energy at Nyquist) added to that channel"""
    x = synth.gen(seed, 48000, _samples(frames), 2).astype(np.float32)
    sign = np.where(np.arange(x.shape[1]) % 2 == 0, 1.0, -1.0).astype(np.float32)
    x[0] += alt_left * sign
    x[1] += alt_right * sign
    return x


def _plan(option: int, **over):
    plan = api.Plan(config.spectrum_config(**over))
    plan.set_option(api.OPT_IMAGE_ONLY_SPLIT, option)
    return plan.upload()


def _render(plan, x, gpu, lines=False, state=False):
    import torch
    xg = torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    F = plan.num_frames(x.shape[1])
    lines_t = torch.empty((F, plan.C, api.NUM_GRAPHS, plan.P, 2), dtype=torch.float32, device=gpu) if lines else None
    state_t = torch.zeros((plan.C, api.NUM_GRAPHS, plan.P, 2), dtype=torch.float32, device=gpu) if state else None
    rgba = plan.render(xg, lines=lines_t, state=state_t)
    torch.cuda.synchronize()
    out = {"rgba": rgba.cpu().numpy()}
    if lines:
        out["lines"] = lines_t.cpu().numpy()
    if state:
        out["state"] = state_t.cpu().numpy()
    return out


def _nyquist(plan, x, gpu, image_only: bool):
    """sgz_stage_nyquist: both channels' Nyquist bins as the chosen launch form leaves them, as raw words; frames per Nyquist workgroup
    of that launch (0: the two-channel form) and the plan's low-pixel count"""
    import torch
    ny, ny_frames, low = plan.stage_nyquist(torch.from_numpy(np.ascontiguousarray(x)).to(gpu), image_only)
    torch.cuda.synchronize()
    return ny.cpu().numpy().view(np.uint32), ny_frames, low


def _same(a: dict, b: dict):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape, k
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (k, int((a[k] != b[k]).sum()))


@pytest.mark.parametrize("frames", [4, 9, 100, 348])
@pytest.mark.parametrize("seed,alt_left,alt_right", [(3, 0.0, 0.6), (11, 0.5, 0.5), (29, 0.0, 0.0)])
def test_image_only_matches_two_channel_launch(gpu, frames, seed, alt_left, alt_right):
    """option on (automatic size) and off: the same RGBA8 bytes; the first two inputs put a strong (-1)^n component into the right
    channel (or both), so that csf[N/2] -- the right channel's Nyquist bin -- wins the top pixels of many frames"""
    x = _signal(seed, frames, alt_left, alt_right)
    on, off = _plan(1), _plan(0)
    assert on.path & 8 and on.N == N
    _same(_render(on, x, gpu), _render(off, x, gpu))
    # the words the image only sees through an 8-bit colour: both channels' Nyquist bins, bit for bit, and the new form was taken
    ny_on, f_on, low = _nyquist(on, x, gpu, True)
    ny_off, f_off, _ = _nyquist(on, x, gpu, False)
    assert low == 0 and f_on >= 1 and f_off == 0, (low, f_on, f_off)
    assert np.array_equal(ny_on, ny_off), int((ny_on != ny_off).sum())


@pytest.mark.parametrize("per_unit", [2, 3, 5, 8, 37, 4096])
def test_image_only_frames_per_nyquist_unit(gpu, per_unit):
    """forced sizes of the Nyquist workgroups (SGZ_OPT_IMAGE_ONLY_SPLIT = n): several frames per workgroup, a partial last one, one
    workgroup for all frames, and a size above the frame count (capped at it)"""
    frames = 37
    x = _signal(41, frames, 0.0, 0.7)
    plan = _plan(per_unit)
    _same(_render(plan, x, gpu), _render(_plan(0), x, gpu))
    ny_on, f_on, _ = _nyquist(plan, x, gpu, True)
    ny_off, _, _ = _nyquist(plan, x, gpu, False)
    assert f_on == min(per_unit, frames), f_on
    assert np.array_equal(ny_on, ny_off), int((ny_on != ny_off).sum())


def test_nyquist_words_with_nonfinite_and_tiny_input(gpu):
    """Nyquist bins bit for bit where rounding and special values are most fragile: denormal-scale samples, an inf and a NaN in one
    frame each of the right channel"""
    frames = 12
    x = _signal(17, frames, 0.0, 0.4)
    x[1, :HOP] *= np.float32(1e-38)
    x[1, 5 * HOP + 100] = np.inf
    x[1, 9 * HOP + 7] = np.nan
    plan = _plan(1)
    ny_on, f_on, _ = _nyquist(plan, x, gpu, True)
    ny_off, _, _ = _nyquist(plan, x, gpu, False)
    assert f_on >= 1
    assert np.array_equal(ny_on, ny_off), int((ny_on != ny_off).sum())


def test_right_channel_nyquist_reaches_the_image(gpu):
    """the input above does exercise the Nyquist workgroups: taking the (-1)^n component out of the right channel alone changes the image
    (the right channel reaches an image-only render through csf[N/2] and nothing else)"""
    frames = 24
    with_alt = _signal(3, frames, 0.0, 0.6)
    without = _signal(3, frames, 0.0, 0.0)
    plan = _plan(1)
    a = _render(plan, with_alt, gpu)["rgba"]
    b = _render(plan, without, gpu)["rgba"]
    changed_frames = int((a != b).any(axis=(1, 2)).sum())
    assert changed_frames >= frames // 2, changed_frames
    # ... and both agree with the two-channel launch
    _same({"rgba": a}, _render(_plan(0), with_alt, gpu))


@pytest.mark.parametrize("lines,state", [(True, False), (False, True), (True, True)])
def test_renders_with_lines_or_state_unchanged(gpu, lines, state):
    """renders that read lines or state keep both channels' transforms: image, lines and state identical with the option on and off"""
    frames = 40
    x = _signal(5, frames, 0.3, 0.6)
    _same(_render(_plan(1), x, gpu, lines=lines, state=state), _render(_plan(0), x, gpu, lines=lines, state=state))


def test_low_pixels_fall_back(gpu):
    """a linear view from 0 Hz has pixels whose tap windows reach over bin 0 into the other channel's bins (low pixels): such a plan keeps
    the two-channel launch, with the same bytes"""
    over = dict(view_scaling=config.VIEW_LINEAR, view_left=0.0, view_right=0.02, axis_points=777)
    frames = 30
    x = _signal(7, frames, 0.0, 0.6)
    plan = _plan(1, **over)
    _, ny_frames, low = _nyquist(plan, x, gpu, True)
    assert low > 0 and ny_frames == 0, (low, ny_frames)           # the view has low pixels, and the image-only form stands aside
    _same(_render(plan, x, gpu), _render(_plan(0, **over), x, gpu))


def test_image_only_full_cfg2_against_oracle(gpu, oracle):
    """the bench's shape (cfg2, 348 frames) with the option on, through the parity chain the full-size tests use"""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from parity_chain import check_render
    cfg = config.cfg2()
    S = int(config.CFG2_SECONDS * 48000)
    x = synth.gen(config.CFG2_SEED, 48000, S, 2)
    plan = api.Plan(cfg)
    plan.set_option(api.OPT_IMAGE_ONLY_SPLIT, 1)
    plan.upload()
    assert plan.num_frames(S) == 348 and plan.path & 8
    problems, stats = check_render(oracle, plan, cfg, x, gpu)
    assert not problems, (problems[:5], stats)
