"""The streamed load phase of the N = 32768 channel workgroups (spectrum_real.hip STREAM, fft_scalar.hpp ditPackedByArrival): the window
phases are requested in front of the samples, the sixteen rows in the bit-reversed order pass 1 consumes them, and the window and
pass 1 run in arrival order.  The order changes WHEN a thread touches an address, not which addresses, and the arithmetic is the same
butterflies on the same operands -- so the shapes that can go wrong are few: one frame, two and three, #CUs + 1 (the smallest launch
with a doubled CU, mates and priorities), a buffer whose last window ends on its last sample (NaN behind it), rows that are only
4-byte aligned (odd channel stride, base shifted by one sample), and a hop that is no whole number of rows.

Per shape:
  * the image-only render against the two-channel render: rgba and the Nyquist words bit for bit -- the Nyquist role sums Z[0] in the
    order the channel role's passes produce it, and the two roles must still window and fuse alike;
  * sgz_stage_bins against tests/fp64_bins.py at the bar of tests/test_gpu_bins_fp64.py (BIN_TOL x the frame's scale);
  * sgz_stage_map_from_bins on the transform's own bins against the transform's own pixels, bit for bit.
Instantiations: the two-channel form <4, true, 0> (bins, pixels, the reference render), the mono form <4, true, 1> (Left), the image-only
form with priorities / shared rows <4, true, 4, true> (hop of four rows, more than one frame per Nyquist workgroup or the one-round
shape) and the plain image-only form <4, true, 4> (one frame; a hop of no whole rows) all run the streamed order; the Mid-Side form
<4, true, 2> and a fetched window <4, false, 0> keep the request order of old (they hold more values in flight) and are checked to the
same bars, so that the selector is exercised on both sides."""
import functools

import numpy as np
import pytest

from signalizer_amd import api, config, synth

pytestmark = pytest.mark.gpu

N = 32768
HOP = 8192                       # four rows of 2048 samples
ODD_HOP = 5000                   # no whole number of rows
BIN_TOL = 4e-6                   # tests/test_gpu_bins_fp64.py BIN_TOL
PAD = 37                         # samples behind each channel's last one (S + PAD odd: rows 4-byte aligned only)

# name -> (frames or "cus+1", hop, layout): layout "tight" -- the buffer is exactly the signal; "tail" -- NaN behind every channel's last
# sample; "odd" -- odd channel stride and the base one sample into the allocation, NaN around the signal
SHAPES = {
    "one_frame": (1, HOP, "tight"),
    "two_frames": (2, HOP, "tight"),
    "three_frames": (3, HOP, "tight"),
    "cus_plus_one": ("cus+1", HOP, "tight"),
    "ends_on_last_sample": (5, HOP, "tail"),
    "rows_4_byte_aligned": (5, HOP, "odd"),
    "hop_no_whole_rows": (5, ODD_HOP, "tight"),
    "hop_no_whole_rows_unaligned": (3, ODD_HOP, "odd"),
}


def _frames(shape: str) -> int:
    import torch
    f = SHAPES[shape][0]
    return torch.cuda.get_device_properties(0).multi_processor_count + 1 if f == "cus+1" else f


@functools.lru_cache(maxsize=None)
def _signal(shape: str) -> np.ndarray:
    frames, hop = _frames(shape), SHAPES[shape][1]
    x = synth.gen(11 + len(shape), 48000, N + (frames - 1) * hop, 2).astype(np.float32)
    x[1] += np.float32(0.6) * np.where(np.arange(x.shape[1]) % 2 == 0, 1.0, -1.0).astype(np.float32)     # csf[N/2] wins top pixels
    x.setflags(write=False)
    return x


def _on_device(gpu, shape: str):
    """the signal in the shape's layout; the returned view has stride(1) == 1"""
    import torch
    x, layout = _signal(shape), SHAPES[shape][2]
    S = x.shape[1]
    if layout == "tight":
        return torch.from_numpy(x.copy()).to(gpu)
    lead = 1 if layout == "odd" else 0
    stride = S + PAD + lead
    stride += (stride % 2 == 0) if layout == "odd" else 0
    big = torch.full((2, stride), float("nan"), dtype=torch.float32, device=gpu)
    big[:, lead:lead + S] = torch.from_numpy(x.copy()).to(gpu)
    view = big[:, lead:lead + S]
    if layout == "odd":
        assert view.stride(0) % 2 == 1 and (view.data_ptr() // 4) % 2 == 1
    return view


@functools.lru_cache(maxsize=None)
def _plan(hop: int, mode: int = config.CH_SEPARATE, option: int = -1, fetch_window: bool = False):
    plan = api.Plan(config.spectrum_config(hop=hop, channel_mode=mode))
    if option >= 0:
        plan.set_option(api.OPT_IMAGE_ONLY_SPLIT, option)
    if fetch_window:
        plan.set_option(api.OPT_FETCH_WINDOW, 1)
    plan.upload()
    assert plan.N == N
    return plan


@functools.lru_cache(maxsize=None)
def _fp64(shape: str, mode: int, fetch_window: bool = False):
    """(csf, scale) of the fp64 restatement, computed once per shape and mode, 32 frames at a time"""
    from fp64_bins import mode_bins, window
    x, hop, frames = _signal(shape), SHAPES[shape][1], _frames(shape)
    cfg = config.spectrum_config(hop=hop, channel_mode=mode)
    w = window(cfg["window_type"], cfg["window_symmetry"], N, cfg["window_alpha"], cfg["window_beta"])
    refs, scales = [], []
    for f0 in range(0, frames, 32):
        starts = np.arange(f0, min(frames, f0 + 32))[:, None] * hop + np.arange(N)
        ref, scale = mode_bins(mode, x[0][starts], x[1][starts], w, N)
        refs.append(ref)
        scales.append(scale)
    ref, scale = np.concatenate(refs), np.concatenate(scales)
    ref.setflags(write=False)
    return ref, scale


def _check_bins(gpu, shape, mode, fetch_window=False):
    """the transform's bins against fp64 at the bar of tests/test_gpu_bins_fp64.py"""
    import torch
    plan = _plan(SHAPES[shape][1], mode, fetch_window=fetch_window)
    xg = _on_device(gpu, shape)
    got = plan.stage_bins(xg).cpu().numpy()[:, 0]
    torch.cuda.synchronize()
    ref, scale = _fp64(shape, mode, fetch_window)
    mono = mode in (config.CH_LEFT, config.CH_RIGHT, config.CH_MERGE, config.CH_SIDE)
    upto = N // 2 + 1 if mono else N + 1                           # the channel-split mono form writes csf[0 .. N/2] (sgz.h)
    want = ref.real if not mono else np.abs(ref)
    if mono:
        want[:, N // 2] = ref[:, N // 2].real                      # X[N/2] / 2, signed (tests/test_gpu_bins_fp64.py _compared)
    g = got[:, :upto]
    assert np.isfinite(g).all(), (shape, "non-finite bins", np.argwhere(~np.isfinite(g))[:5].tolist())
    rel = np.abs(g - want[:, :upto]) / scale[:, None]
    i = np.unravel_index(int(rel.argmax()), rel.shape)
    special = (0, N // 2) if mono else (0, N // 2 - 1, N // 2, N)
    msg = f"{shape} mode {mode}: worst err / scale {rel[i]:.3g} at (frame, bin) {tuple(int(v) for v in i)}; " + \
          ", ".join(f"csf[{k}] {rel[:, k].max():.3g}" for k in special)
    print(msg)
    assert rel[i] <= BIN_TOL, msg
    return plan, xg


def _check_map_given_own_bins(plan, xg, shape):
    """sgz_stage_map_from_bins on the transform's own bins == the transform's own pixels, bit for bit"""
    import torch
    bins = plan.stage_bins(xg)
    own = plan.stage_mapped(xg).cpu().numpy()
    again = plan.stage_map_from_bins(bins).cpu().numpy()
    torch.cuda.synchronize()
    assert np.isfinite(own).all(), (shape, "non-finite pixels")
    bad = np.argwhere(own.view(np.uint32) != again.view(np.uint32))
    assert bad.size == 0, (shape, "pixels of the transform differ from the map of its own bins", len(bad), bad[:8].tolist())


@functools.lru_cache(maxsize=None)
def _two_channel(shape: str):
    """image and Nyquist words of the two-channel launch on the tight layout, once per shape"""
    import torch
    plan = _plan(SHAPES[shape][1], option=0)
    x = torch.from_numpy(_signal(shape).copy()).to("cuda:0")
    rgba = plan.render(x).cpu().numpy()
    ny, ny_frames, low = plan.stage_nyquist(x, False)
    torch.cuda.synchronize()
    assert ny_frames == 0 and low == 0 and plan.num_frames(x.shape[1]) == _frames(shape)
    rgba.setflags(write=False)
    return rgba, ny.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_image_only_equals_two_channel(gpu, shape):
    """<4, true, 4, true> / <4, true, 4> against <4, true, 0>: every image byte and every Nyquist word"""
    import torch
    want_rgba, want_ny = _two_channel(shape)
    frames = _frames(shape)
    options = [1] + ([2, 3] if 2 <= frames <= 8 else [])            # automatic size; forced sizes (more than one frame: shared rows)
    xg = _on_device(gpu, shape)
    for option in options:
        plan = _plan(SHAPES[shape][1], option=option)
        got = plan.render(xg).cpu().numpy()
        ny, ny_frames, low = plan.stage_nyquist(xg, True)
        torch.cuda.synchronize()
        assert ny_frames >= 1 and low == 0, (shape, option, "the image-only form stood aside", ny_frames, low)
        bad = np.nonzero((got != want_rgba).any(axis=(1, 2)))[0]
        assert bad.size == 0, (shape, option, ny_frames, "image rows differ", bad.size, bad[:8].tolist())
        ny = ny.cpu().numpy().view(np.uint32)
        bad = np.nonzero((ny != want_ny).reshape(frames, -1).any(axis=1))[0]
        assert bad.size == 0, (shape, option, ny_frames, "Nyquist words differ", bad.size, bad[:8].tolist())
    # the two-channel launch itself on this layout
    plan = _plan(SHAPES[shape][1], option=0)
    got = plan.render(xg).cpu().numpy()
    assert np.array_equal(got, want_rgba), (shape, "two-channel render differs between layouts")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_two_channel_bins_and_map(gpu, shape):
    """<4, true, 0>: bins against fp64, pixels against the map of its own bins"""
    plan, xg = _check_bins(gpu, shape, config.CH_SEPARATE)
    _check_map_given_own_bins(plan, xg, shape)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_mono_bins(gpu, shape):
    """<4, true, 1> (Left): one workgroup per frame, the same streamed load"""
    _check_bins(gpu, shape, config.CH_LEFT)


@pytest.mark.parametrize("shape", ["three_frames", "rows_4_byte_aligned", "hop_no_whole_rows"])
def test_forms_that_keep_the_request_order(gpu, shape):
    """Mid-Side <4, true, 2> and a fetched window <4, false, 0>: not streamed, same bars"""
    _check_bins(gpu, shape, config.CH_MIDSIDE)
    plan, xg = _check_bins(gpu, shape, config.CH_SEPARATE, fetch_window=True)
    _check_map_given_own_bins(plan, xg, shape)
