"""The emission of the fused colour K_B (spectrum_post.hip decayColourFusedKernel<4 / 8 / 16>): sgz_stage_decay_colour on magnitudes made
here -- no transform runs -- against the CPU oracle's decay, dB and colour chain (oracle/pyoracle.py decay_colour) and against the
several-launch form of K_B (SGZ_OPT_FUSED_COLOUR = 0) on the same input, RGBA bytes bit for bit.

What the emission does per (frame, pixel) item and where it can go wrong:
  * the frame's zero-carry state is read from LDS, where the chunk scan left it  -> chunk edges, the partial last chunk (1, 7, 8, 9, 17 frames);
  * the carry of the chunk before is decayed t + 1 times and the larger of the two is shown  -> a single loud frame and silence: one
    carry survives to the end, every t of every chunk shows the decayed carry; a rising ramp: the local state always wins;
  * a thread's items are 960 apart  -> 240 / 241 frames (the first item of the second round at 4 pixels per workgroup), 348, 512 (the
    last count the fused kernel takes) and 513 (the other path, which must agree);
  * the gradient, whose interval differs from lane to lane  -> intensities below 0, exactly on every running sum, between every pair of
    stops, in [0.999, 1) and above 1 (test_inputs_reach_every_colour_case holds the input to that);
  * P = 1024 and P = 333 (no multiple of 4 or 32: the `pixel < P` guards, and a grid that is no multiple of 8: pixelGroup()'s other branch);
  * subnormal and +inf magnitudes, zeros (every pixel at lowerClip), a non-zero carry-in state, a plan with late pixels.
"""
import functools
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FRAMES = (1, 7, 8, 9, 17, 240, 241, 348, 512, 513)
PIXELS = (1024, 333)
KINDS = ("impulse", "ramp", "zeros", "stops", "extremes")
LOW_DB, HIGH_DB = -120.0, 0.0
POLES = (0.9, 0.99)


def _cfg(P):
    return config.spectrum_config(window_size=512, hop=128, axis_points=P, low_db=LOW_DB, high_db=HIGH_DB, pole=POLES)


@functools.lru_cache(maxsize=None)
def _plan(P, fused):
    """fused: 4, 8, 16 pixels per workgroup of the fused colour kernel, or 0: the scan / emit launches"""
    plan = api.Plan(_cfg(P))
    plan.set_option(api.OPT_FUSED_COLOUR, fused)
    return plan.upload()


def _ulps(x, k):
    """positive finite float32 x moved by k units in the last place"""
    return (np.asarray(x, np.float32).view(np.int32) + np.asarray(k, np.int32)).view(np.float32)


@functools.lru_cache(maxsize=None)
def _targets(P):
    """intensities the `stops` input aims at, ascending: below 0, then every running sum of the gradient and the middle of every interval, the
    0.999 edge, above 1 -- as magnitudes [targets][P] whose pixel p sits (p - P / 2) ulps from the fp64 estimate, so that a sweep of one frame
    crosses the exact float of every edge"""
    from oracle import pyoracle as po
    p = po.params_from_dict(_cfg(P))
    sums = np.cumsum(po.colour_ratios(_cfg(P)["ratios"])[1:].astype(np.float32), dtype=np.float32)
    edges = [-0.05, 0.5 * float(sums[0])]
    for c in range(len(sums) - 1):
        edges += [float(sums[c]), 0.5 * (float(sums[c]) + float(sums[c + 1]))]
    edges += [0.999, 0.9995, 1.5]
    lower, upper = 10.0 ** (LOW_DB / 20.0), 10.0 ** (HIGH_DB / 20.0)
    slope = po.slope_map(p, po.remap_frequencies(p)).astype(np.float64)
    base = np.stack([lower * np.exp(e * np.log(upper / lower)) / slope for e in edges]).astype(np.float32)
    return _ulps(base, np.arange(P, dtype=np.int32)[None, :] - P // 2), sums


@functools.lru_cache(maxsize=None)
def _input(kind, frames, P):
    """magnitudes [frames][1][2][P]; side 1 (not shown in the image) carries other values than side 0"""
    rng = np.random.default_rng(1000 * frames + P)
    m = np.zeros((frames, 1, 2, P), np.float32)
    if kind == "impulse":
        m[0, 0, 0] = rng.uniform(0.05, 2.0, P).astype(np.float32)
    elif kind == "ramp":
        start = rng.uniform(1e-7, 1e-5, P)
        m[:, 0, 0] = (start[None, :] * np.exp(np.arange(frames)[:, None] * (np.log(3e6) / max(frames - 1, 1)))).astype(np.float32)
    elif kind == "stops":
        t, _ = _targets(P)
        which = (np.arange(frames) * len(t)) // frames if frames >= len(t) else np.arange(frames) * (len(t) // max(frames, 1))
        first = np.array([np.argmax(which == w) for w in which])
        m[:, 0, 0] = _ulps(t[which], (np.arange(frames) - first)[:, None].astype(np.int32))      # ascending in time: the state is the magnitude
    elif kind == "extremes":
        pool = np.array([0.0, 1e-45, 3e-42, 1e-39, 1.1754944e-38, 1e-30, 1e-6, 0.3, 1.0, 1e30], np.float32)
        m[:, 0, 0] = pool[rng.integers(0, len(pool), (frames, P))]
        late = rng.integers(0, frames, P)
        cols = np.nonzero(rng.random(P) < 0.25)[0]
        m[late[cols], 0, 0, cols] = np.inf                                                      # +inf from some frame on, in a quarter of the pixels
    m[:, 0, 1] = m[::-1, 0, 0] * np.float32(0.5)
    return m


@functools.lru_cache(maxsize=None)
def _reference(kind, frames, P):
    """the oracle's image and dB lines of _input (computed once per input, shared by every launch form)"""
    from oracle import pyoracle as po
    rgba, lines = po.decay_colour(po.params_from_dict(_cfg(P)), _input(kind, frames, P), want_lines=True)
    rgba.setflags(write=False)
    return rgba, lines


@pytest.mark.gpu
@pytest.mark.parametrize("P", PIXELS)
@pytest.mark.parametrize("frames", FRAMES)
def test_emission_bit_exact(gpu, oracle, frames, P):
    import torch
    for kind in KINDS:
        want, _ = _reference(kind, frames, P)
        mag = torch.from_numpy(_input(kind, frames, P)).to(gpu)
        several, _ = _plan(P, 0).stage_decay_colour(mag)
        assert np.array_equal(several.cpu().numpy(), want), (kind, "scan / emit launches")
        for px in (4, 8, 16):
            got, _ = _plan(P, px).stage_decay_colour(mag)
            got = got.cpu().numpy()
            bad = np.nonzero((got != want).any(axis=2))
            assert not len(bad[0]), (kind, px, int(len(bad[0])), "first (frame, pixel)", int(bad[0][0]), int(bad[1][0]),
                                     got[bad[0][0], bad[1][0]], want[bad[0][0], bad[1][0]])
            assert torch.equal(torch.from_numpy(got).to(gpu), several), (kind, px)


def test_inputs_reach_every_colour_case(oracle):
    """the `stops` input as the oracle sees it: intensities below 0, EXACTLY on every running sum, inside every interval, in [0.999, 1) and
    above 1; zeros sit at the clip value; the impulse decays below 0 before the last frame (so the decayed carry is what is shown)"""
    for P in PIXELS:
        _, sums = _targets(P)
        for frames in (17, 348):
            _, lines = _reference("stops", frames, P)
            inten = lines[:, 0, 0, :].real.astype(np.float32)
            assert (inten < 0).any() and ((inten >= np.float32(0.999)) & (inten < 1)).any() and (inten > 1).any()
            for c in range(len(sums) - 1):
                assert (inten == sums[c]).any(), (P, frames, c, float(sums[c]))
            lo = np.concatenate([[np.float32(0)], sums[:-1]])
            for c in range(len(sums)):
                assert ((inten > lo[c]) & (inten < min(sums[c], np.float32(0.999)))).any(), (P, frames, c)
        _, lines = _reference("zeros", 9, P)
        assert (lines[:, 0, 0, :].real == np.float32(-384.0)).all()
        _, lines = _reference("impulse", 348, P)
        inten = lines[:, 0, 0, :].real
        assert (inten[1] > 0).all() and (inten[-1] < 0).all() and (np.diff(inten, axis=0) < 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("frames,P", [(9, 1024), (241, 333), (348, 1024)])
def test_carry_in_state_and_end_state(gpu, oracle, frames, P):
    """a non-zero carry-in: the state a first frame leaves (from zero, the state after one frame IS its magnitudes, in both graphs) handed to
    a render of the remaining frames gives the oracle's image of the whole input from its second frame on, and the end state is the
    recurrence s = max(fl(s * pole), m) in fp32.
    This is NOT the fused colour kernel: a call that hands a state over runs decayFullFusedKernel (the C ABI's one `state` pointer is
    carry-in and end state at once, and the colour kernel takes renders without one), so the image-only kernel never receives a carry-in
    through the API and the seed of chunk 0 in its scan is unreachable.  The case is here because a carry-in belongs to the emission's
    contract; it holds the kernel beside the changed one to the same inputs."""
    import torch
    for kind in ("impulse", "stops", "extremes"):
        m = _input(kind, frames + 1, P)
        want, _ = _reference(kind, frames + 1, P)
        state = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(m[0, 0].T[None, None], (1, 2, P, 2)))).to(gpu)
        got, _ = _plan(P, 4).stage_decay_colour(torch.from_numpy(m[1:]).to(gpu), state=state)
        assert np.array_equal(got.cpu().numpy(), want[1:]), kind
        s = np.zeros((2, 2, P), np.float32)                               # [graph][side][pixel]
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            for f in range(frames + 1):
                s = s * np.array(POLES, np.float32)[:, None, None]
                s = np.where(m[f, 0][None] > s, m[f, 0][None], s)
        assert np.array_equal(state.cpu().numpy()[0].view(np.uint32), np.ascontiguousarray(s.transpose(0, 2, 1)).view(np.uint32)), kind


@pytest.mark.gpu
def test_late_pixels_through_the_fused_kernel(gpu, oracle):
    """an image-only render at N = 32768 leaves the channel workgroups' late pixels (the top pixels, where csf[N/2] of BOTH channels can win)
    to the fused colour kernel, which completes them as it loads the magnitudes: its image is the oracle's colour chain on the completed
    magnitudes, for all three workgroup sizes.  The input carries a tone at the Nyquist frequency, so that csf[N/2] does win, and the
    test holds itself to that: the render's launch is the image-only channel-split one, and K_A's dominant launch alone leaves side 0
    of some pixels different from the completed magnitudes -- without the completion the image could not be the oracle's."""
    import ctypes as C
    import torch
    from signalizer_amd import synth
    po = oracle
    cfg = config.cfg2()
    frames = 9
    S = cfg["window_size"] + (frames - 1) * cfg["hop"]
    x = synth.gen(7, 48000, S, 2)
    x += (0.25 * (1 - 2 * (np.arange(S) & 1))).astype(np.float32)[None, :]
    xg = torch.from_numpy(x).to(gpu)
    stream = torch.cuda.current_stream().cuda_stream
    want = None
    for px in (4, 8, 16):
        plan = api.Plan(cfg)
        plan.set_option(api.OPT_FUSED_COLOUR, px)
        plan.upload()
        if want is None:
            complete = plan.stage_mapped(xg)
            alone = torch.empty_like(complete)
            api.check(api.lib().sgz_stage_mapped_dominant(plan.h, xg.data_ptr(), xg.stride(0), S, alone.data_ptr(), stream))
            ny = torch.empty((frames, plan.C, 2), dtype=torch.float32, device=gpu)
            ny_frames = C.c_uint32(0)
            api.check(api.lib().sgz_stage_nyquist(plan.h, xg.data_ptr(), xg.stride(0), S, 1, ny.data_ptr(), C.byref(ny_frames), None, stream))
            torch.cuda.synchronize()
            assert ny_frames.value >= 1, "not the image-only channel-split launch"
            late = (alone[:, 0, 0] != complete[:, 0, 0]).any(dim=0).nonzero().flatten().cpu().numpy()
            assert (late >= plan.P - 64).any(), late                         # late pixels exist, at the top of the axis
            want, _ = po.decay_colour(po.params_from_dict(cfg), complete.cpu().numpy())
            incomplete, _ = po.decay_colour(po.params_from_dict(cfg), alone.cpu().numpy())
            assert not np.array_equal(incomplete, want)                       # ... and they show in the image
        assert np.array_equal(plan.render(xg).cpu().numpy(), want), px


def test_fused_colour_kernels_use_no_scratch():
    """the three instantiations keep their working set in registers (the project's code-object report, tools/codeobj_report.py)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_report as cr
    lib = os.path.join(ROOT, "signalizer_amd", "libsgz.so")
    # no skip: build() has made the library before any test runs, and without the tools the check must not pass unseen
    assert os.path.exists(lib), lib
    assert os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy"), cr.LLVM
    rows = [r for r in cr.kernels(lib) if "decayColourFusedKernel" in r["demangled"]]
    assert len(rows) == 3, [r["demangled"] for r in rows]
    for r in rows:
        assert not r.get("private_segment_fixed_size", 0) and not r.get("vgpr_spill_count", 0) and not r.get("sgpr_spill_count", 0), r
        assert r["vgpr_count"] <= 128, r                                  # 1024 threads: four waves per SIMD
