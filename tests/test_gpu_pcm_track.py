"""The track lane inside the PCM stream on the GPU (sgz_pcm_stream_set_track, _track_for, _track_state; csrc/pcm.hip, the slab loop in
csrc/api.hip, csrc/tracker.hip).

Byte for byte (uint64 views of the records), no tolerance: the lane's records of all feeds == Plan.track_render (sgz_spectrogram_track_host) of
the numpy-converted planar floats on a separate plan, and == the host loop of sgz_track_peak_lines over a twin stream's feed(lines) -- for
every graph, mouse position, chunk_samples, SGZ_OPT_OVERVIEW_SLAB, kind of feed and way of cutting the stream into feeds; and everything
the feeds of an armed stream return == an unarmed twin's, byte for byte.  The caller's records lie in front of two sentinel records that
must stay untouched."""
import ctypes as C
import gc
import math
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_ref as ov  # noqa: E402
import wave_ref as wr  # noqa: E402
from test_gpu_pcm import BYTES, convert_ref, to_bytes  # noqa: E402  (the converter's numpy reference)
from test_gpu_pcm_overview import _feed_sizes  # noqa: E402  (the cuts: empty, one-sample and frameless feeds included)

pytestmark = pytest.mark.gpu

NAMES = ("sgz_pcm_stream_set_track", "sgz_pcm_stream_track_for", "sgz_pcm_stream_track_state")
SPLIT = 8                                                          # SGZ_PATH_* (sgz.h)
CASES = {
    # cfg, frames, format, source channels, channel map
    "w64_s16": (dict(window_size=64, hop=16, axis_points=63, pole=(0.3, 0.3)), 23, api.PCM_S16, 3, [2, 0]),
    "w256_f32_two_pairs": (dict(window_size=256, hop=64, axis_points=65, num_pairs=2, pole=(0.5, 0.5)), 23, api.PCM_F32, 4, [3, 0, 2, 1]),
    "n4096_odd_hop": (dict(window_size=4096, hop=333, axis_points=257, pole=(0.3, 0.3)), 13, api.PCM_S16, 2, None),
    "phase": (dict(window_size=256, hop=64, axis_points=100, channel_mode=config.CH_PHASE, pole=(0.3, 0.3)), 23, api.PCM_F32, 3, [1, 2]),
    "n32768_split": (dict(window_size=32768, hop=8192, pole=(0.3, 0.3)), 6, api.PCM_S16, 3, [2, 1]),
}
CHUNKS = (0, 1000, 4096)
SLABS = (0, 1, 3)
GRAPHS = (0, 1)
FRACTIONS = (-1.0, 0.0, 0.03, 0.5, 0.97, 2.0)
COMBOS = [(g, mf) for g in GRAPHS for mf in FRACTIONS]
PATTERNS = ("plain", "k1", "k5", "kF3", "mixed")
LP = len(api.LinePeak._fields_)
SENTINEL = 0x5A5AA5A5C3C33C3C
E = api.SGZ_EINVAL
_made, _wants = {}, {}


def _lib():
    L = api.lib()
    for name in NAMES:
        assert hasattr(L, name), f"libsgz.so does not export {name}"
    return L


def _case(name):
    """(cfg, format, source channels, map, PCM bytes, samples, frames, a plan of its own, the converted planar floats) -- once"""
    _lib()
    if name not in _made:
        over, frames, fmt, channels, cmap = CASES[name]
        cfg = config.spectrum_config(**over)
        x = ov.burst_signal(cfg["window_size"], cfg["hop"], frames, channels, cfg["sample_rate"], seed=13)
        inter = np.ascontiguousarray(x.T).reshape(-1)
        raw = to_bytes(np.clip(np.round(inter.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int64), fmt) if fmt == api.PCM_S16 else to_bytes(inter, fmt)
        n = x.shape[1]
        planar = np.ascontiguousarray(convert_ref(raw, fmt, channels)[cmap if cmap is not None else slice(None)])
        plan = api.Plan(cfg).upload()
        if name == "n32768_split":
            assert plan.path & SPLIT, plan.path
        assert plan.num_frames(n) == frames and planar.shape[0] == 2 * cfg["num_pairs"]
        for a in (raw, planar):
            a.setflags(write=False)
        _made[name] = (cfg, fmt, channels, cmap, raw, n, frames, plan, planar)
    return _made[name]


def _want(name, graph, mf):
    """Plan.track_render of the converted floats: uint64 [F][C][6]"""
    if (name, graph, mf) not in _wants:
        plan, planar = _case(name)[7], _case(name)[8]
        track, _, _ = plan.track_render(planar, graph, mf, want_rgba=False)
        _wants[name, graph, mf] = track.view(np.uint64).copy()
    return _wants[name, graph, mf]


def _records(frames, pairs):
    """the caller's buffer: `frames` records per pair and two sentinel records behind them; (uint64 view, float64 view of the same memory)"""
    bits = np.full((frames + 2, pairs, LP), SENTINEL, np.uint64)
    return bits, bits.view(np.float64)


def _feed(s, raw, fb, at, size, kind, k=0, flush=False, lines=True, image=True):
    """one feed of either kind -> what it returned, as bytes"""
    pcm = raw[at * fb:(at + size) * fb] if size else None
    if kind == "plain":
        rgba, got, _ = s.feed(pcm if size else raw[:0], nsamples=size, want_lines=lines)
        return ("plain", rgba.tobytes(), got.tobytes() if lines else b"")
    rgba, peaks, _ = s.feed_overview(pcm, k, flush=flush, nsamples=size, want_rgba=image, want_peaks=True)
    return ("overview", rgba.tobytes() if image else b"", peaks.tobytes())


def _plan_feeds(pattern, sizes, F):
    """(kind, k, with line results) per feed: plain feeds alternate between lines_out given and NULL; mixed: plain feeds, then overview feeds
    (the other order is refused while a column is open)"""
    k = {"k1": 1, "k5": 5, "kF3": F + 3, "mixed": 5}.get(pattern, 0)
    count = len(sizes)
    if pattern == "plain":
        return [("plain", 0, bool(i % 2)) for i in range(count)]
    if pattern == "mixed":
        return [("plain", 0, bool(i % 2)) if i < count // 2 else ("overview", k, False) for i in range(count)]
    return [("overview", k, False)] * count


def _run(s, raw, fb, sizes, pattern, F, W, hop, armed):
    """feeds the sizes in turn and flushes an open overview column with an empty feed; armed: checks track_for / track_state around every
    feed against sgz_stream_step chained.  -> everything the feeds returned"""
    returned, at, held, written = [], 0, 0, 0
    feeds = _plan_feeds(pattern, sizes, F)
    for size, (kind, k, lines) in zip(sizes, feeds):
        frames, held = api.stream_step(W, hop, held, size)
        assert s.track_for(size) == (frames if armed else 0)
        returned.append(_feed(s, raw, fb, at, size, kind, k, lines=lines))
        at += size
        written += frames
        assert s.track_state() == (written if armed else 0), (size, kind)
    if feeds[-1][0] == "overview":
        assert s.track_for(0) == 0
        returned.append(_feed(s, raw, fb, at, 0, "overview", feeds[-1][1], flush=True))
        assert s.track_state() == (written if armed else 0)
    assert written == F and s.open_frames() == 0
    return returned


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", list(CASES))
def test_lane_equals_the_track_render_and_leaves_the_feeds_alone(gpu, name, chunk):
    cfg, fmt, channels, cmap, raw, n, F, plan, planar = _case(name)
    W, hop, fb, Cn = cfg["window_size"], cfg["hop"], channels * BYTES[fmt], cfg["num_pairs"]
    salt = CHUNKS.index(chunk) + list(CASES).index(name)
    rng = np.random.default_rng(len(name) + chunk)
    armed = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
    twin = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
    seen = set()
    for i, (graph, mf) in enumerate(COMBOS):
        pattern, slab = PATTERNS[(i + salt) % len(PATTERNS)], SLABS[(i + salt // 2) % len(SLABS)]
        seen.add(pattern)
        sizes = _feed_sizes(rng, n, W, hop)
        assert 0 in sizes and 1 in sizes and any(0 < v < hop for v in sizes), sizes
        what = (name, chunk, graph, mf, pattern, slab, sizes)
        twin.reset()
        twin.set_option(api.OPT_OVERVIEW_SLAB, slab)
        unarmed = _run(twin, raw, fb, sizes, pattern, F, W, hop, False)
        bits, out = _records(F, Cn)
        armed.reset()
        armed.set_option(api.OPT_OVERVIEW_SLAB, slab)
        armed.set_track(graph, mf, out, F)
        got = _run(armed, raw, fb, sizes, pattern, F, W, hop, True)
        assert (bits[:F] == _want(name, graph, mf)).all(), what
        assert (bits[F:] == SENTINEL).all(), what
        assert got == unarmed, what
    assert seen == set(PATTERNS)
    # the whole file in one feed (the pieces of chunk_samples inside it): a plain feed without lines_out, and the track-only pass -- an
    # overview feed with more frames per column than the file has and the peaks only
    for graph, mf in ((0, 0.5), (1, 0.03)):
        for kind in ("plain", "overview"):
            bits, out = _records(F, Cn)
            armed.reset()
            armed.set_track(graph, mf, out, F)
            assert armed.track_for(n) == F
            got = _feed(armed, raw, fb, 0, n, kind, F + 3, flush=True, lines=False, image=False)
            twin.reset()
            assert got == _feed(twin, raw, fb, 0, n, kind, F + 3, flush=True, lines=False, image=False)
            assert armed.track_state() == F and (bits[:F] == _want(name, graph, mf)).all() and (bits[F:] == SENTINEL).all(), (name, chunk, graph, mf, kind)
    armed.close(); twin.close()


@pytest.mark.parametrize("name", list(CASES))
def test_lane_equals_the_host_loop_over_a_twins_lines(gpu, name):
    """the parent's way to a track from a stream: feed(..., lines_out), then sgz_track_peak_lines per (frame, pair)"""
    cfg, fmt, channels, cmap, raw, n, F, plan, planar = _case(name)
    W, hop, fb, Cn = cfg["window_size"], cfg["hop"], channels * BYTES[fmt], cfg["num_pairs"]
    L = api.lib()
    rng = np.random.default_rng(len(name))
    twin = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    lines, at = [], 0
    for size in _feed_sizes(rng, n, W, hop):
        lines.append(twin.feed(raw[at * fb:(at + size) * fb] if size else raw[:0], nsamples=size, want_lines=True)[1])
        at += size
    lines = np.ascontiguousarray(np.concatenate(lines))
    assert lines.shape == (F, Cn, api.NUM_GRAPHS, cfg["axis_points"], 2)
    armed = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    for graph, mf in COMBOS:
        loop = np.zeros((F, Cn, LP), np.uint64)
        for f in range(F):
            for p in range(Cn):
                one = api.LinePeak()
                api.check(L.sgz_track_peak_lines(plan.h, lines[f, p, graph].ctypes.data_as(C.c_void_p), mf, C.byref(one)))
                loop[f, p] = np.frombuffer(bytes(one), np.uint64)
        bits, out = _records(F, Cn)
        armed.reset()
        armed.set_track(graph, mf, out, F)
        _feed(armed, raw, fb, 0, n, "plain", lines=False)
        assert (bits[:F] == loop).all() and (loop == _want(name, graph, mf)).all(), (name, graph, mf)
    armed.close(); twin.close()


def test_with_the_waveform_lane_armed_as_well(gpu):
    name, m = "w256_f32_two_pairs", 100
    cfg, fmt, channels, cmap, raw, n, F, plan, planar = _case(name)
    W, hop, fb, Cn, D = cfg["window_size"], cfg["hop"], channels * BYTES[fmt], cfg["num_pairs"], planar.shape[0]
    wave_want = wr.columns_of(planar, m)[0]
    rng = np.random.default_rng(21)
    both = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    twin = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    for pattern in ("mixed", "plain", "k5"):
        sizes = _feed_sizes(rng, n, W, hop)
        twin.reset()
        unarmed = _run(twin, raw, fb, sizes, pattern, F, W, hop, False)
        bits, out = _records(F, Cn)
        wave = np.full((wave_want.shape[0] + 2, D, 2), np.float32(-77.0))
        both.reset()
        both.set_waveform(m, wave)
        both.set_track(1, 0.5, out, F)
        got = _run(both, raw, fb, sizes, pattern, F, W, hop, True)
        both.flush_waveform()
        assert got == unarmed, (pattern, sizes)
        assert (bits[:F] == _want(name, 1, 0.5)).all() and (bits[F:] == SENTINEL).all(), (pattern, sizes)
        assert np.array_equal(wave[:wave_want.shape[0]].view(np.uint32), wave_want) and (wave[wave_want.shape[0]:] == np.float32(-77.0)).all(), (pattern, sizes)
    both.close(); twin.close()


def test_draining_through_a_buffer_of_seven_frames(gpu):
    name, cap = "w64_s16", 7
    cfg, fmt, channels, cmap, raw, n, F, plan, planar = _case(name)
    hop, fb, Cn = cfg["hop"], channels * BYTES[fmt], cfg["num_pairs"]
    rng = np.random.default_rng(3)
    for kind in ("plain", "overview"):
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=64)
        small = [_records(cap, Cn), _records(cap, Cn)]
        which, kept, at, rearmed = 0, [], 0, 0
        s.set_track(0, 0.5, small[0][1], cap)
        while at < n:
            size = min(int(rng.integers(0, (cap - 1) * hop)), n - at)
            written = s.track_state()
            if written + s.track_for(size) > cap:                      # drain: keep what is there, re-arm with the other buffer
                kept.append(small[which][0][:written].copy())
                which ^= 1
                s.set_track(0, 0.5, small[which][1], cap)
                assert s.track_state() == 0
                rearmed += 1
            _feed(s, raw, fb, at, size, kind, 4)
            at += size
        kept.append(small[which][0][:s.track_state()].copy())
        assert rearmed >= 3 and (np.concatenate(kept) == _want(name, 0, 0.5)).all(), kind
        assert all((b[0][cap:] == SENTINEL).all() for b in small)
        s.close()


def test_counts_refusals_reset_and_disarm(gpu):
    name = "w256_f32_two_pairs"
    cfg, fmt, channels, cmap, raw, n, F, plan, planar = _case(name)
    W, hop, P, fb, Cn = cfg["window_size"], cfg["hop"], cfg["axis_points"], channels * BYTES[fmt], cfg["num_pairs"]
    L = _lib()
    want = _want(name, 1, 0.97)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    twin = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    assert s.track_for(n) == 0 and s.track_state() == 0                # disarmed
    first = W + 2 * hop                                                # three frames
    bits, out = _records(2, Cn)
    s.set_track(1, 0.97, out, 2)
    assert s.track_for(first) == 3 and s.track_for(W - 1) == 0 and s.frames_for(first) == 3
    big_rgba = np.zeros((F, P, 4), np.uint8)
    peaks = np.zeros((F, Cn, P), np.float32)
    # fewer frames left in the buffer than the feed completes: refused by both kinds, nothing consumed
    assert s.feed_into(raw, first, big_rgba, None, F)[0] == E and "track" in L.sgz_last_error().decode()
    assert s.feed_overview_into(raw, first, 5, False, big_rgba, peaks, F)[0] == E and "track" in L.sgz_last_error().decode()
    assert s.feed_overview_into(raw, first, 5, True, None, peaks, F)[0] == E
    assert (bits == SENTINEL).all() and not big_rgba.any() and not peaks.any()
    assert s.track_state() == 0 and s.frames_for(first) == 3 and s.open_frames() == 0
    # set_track's own refusals leave the lane as it was
    other = _records(F, Cn)
    for graph, mf, ptr, capacity in ((api.NUM_GRAPHS, 0.5, other[1].ctypes.data, F), (0xffffffff, 0.5, other[1].ctypes.data, F),
                                     (0, math.nan, other[1].ctypes.data, F), (0, math.inf, other[1].ctypes.data, F),
                                     (0, -math.inf, other[1].ctypes.data, F), (0, 0.5, None, 3)):
        assert L.sgz_pcm_stream_set_track(s.h, graph, mf, ptr, capacity) == E, (graph, mf, capacity)
    assert s.track_for(first) == 3 and s.feed_into(raw, first, big_rgba, None, F)[0] == E                  # still the buffer of two frames
    # ... and the feeds that fit are those of a stream that never saw the refusals, written where the lane was armed
    a = _feed(s, raw, fb, 0, first - hop, "plain")
    b = _feed(twin, raw, fb, 0, first - hop, "plain")
    assert a == b and s.track_state() == 2 and (bits[:2] == want[:2]).all() and (bits[2:] == SENTINEL).all() and (other[0] == SENTINEL).all()
    assert s.track_for(hop) == 1 and s.feed_into(raw[(first - hop) * fb:], hop, big_rgba, None, F)[0] == E         # full
    # reset restarts the cursor and keeps the lane armed; the same file again gives the same records
    s.reset(); twin.reset()
    assert s.track_state() == 0 and s.track_for(first) == 3
    bits, out = _records(F, Cn)
    s.set_track(1, 0.97, out, F)
    _feed(s, raw, fb, 0, n // 2, "plain")
    half = s.track_state()
    assert 0 < half < F and (bits[:half] == want[:half]).all() and (bits[half:] == SENTINEL).all()
    s.reset()
    assert s.track_state() == 0 and s.track_for(n) == F
    _feed(s, raw, fb, 0, n, "overview", 5, flush=True)
    assert s.track_state() == F and (bits[:F] == want).all() and (bits[F:] == SENTINEL).all()
    # set_track between feeds restarts the cursor in the middle of a stream and may change graph and position
    s.reset()
    _feed(s, raw, fb, 0, n // 2, "plain")
    bits2, out2 = _records(F - half, Cn)
    s.set_track(0, 0.03, out2, F - half)
    assert s.track_state() == 0
    _feed(s, raw, fb, n // 2, n - n // 2, "plain", lines=False)
    assert s.track_state() == F - half and (bits2[:F - half] == _want(name, 0, 0.03)[half:]).all() and (bits2[F - half:] == SENTINEL).all()
    # disarmed: nothing is written any more, the feeds are the twin's
    bits, out = _records(F, Cn)
    s.reset()
    s.set_track(0, 0.5, out, F)
    s.set_track(out=None)
    assert s.track_for(n) == 0 and s.track_state() == 0
    assert _feed(s, raw, fb, 0, n, "plain") == _feed(twin, raw, fb, 0, n, "plain")
    assert (bits == SENTINEL).all() and s.track_state() == 0
    s.close(); twin.close()


def test_pinned_and_pageable_destinations(gpu):
    import torch
    for name in ("w64_s16", "n4096_odd_hop"):
        cfg, fmt, channels, cmap, raw, n, F, plan, planar = _case(name)
        fb, Cn = channels * BYTES[fmt], cfg["num_pairs"]
        want = _want(name, 0, 0.5)
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
        pinned = torch.from_numpy(_records(F, Cn)[1].copy()).pin_memory()
        s.set_track(0, 0.5, pinned, F)
        _feed(s, raw, fb, 0, n // 3, "plain", lines=False)
        _feed(s, raw, fb, n // 3, n - n // 3, "overview", 5, flush=True)
        got = pinned.numpy().view(np.uint64)
        assert s.track_state() == F and (got[:F] == want).all() and (got[F:] == SENTINEL).all(), name
        s.reset()
        bits, out = _records(F, Cn)
        s.set_track(0, 0.5, out, F)                                    # the same stream, now through the pinned twins
        _feed(s, raw, fb, 0, n // 3, "overview", 5)
        _feed(s, raw, fb, n // 3, n - n // 3, "overview", 5, flush=True)
        assert s.track_state() == F and (bits[:F] == want).all() and (bits[F:] == SENTINEL).all(), name
        s.close()


def test_lane_is_the_same_beside_a_background_render(gpu):
    """another plan's renders in flight on a stream of their own while the feeds run (the pattern of tests/test_gpu_pcm.py)"""
    import torch
    cases = [(_case(name), _want(name, 0, 0.5)) for name in ("n32768_split", "w256_f32_two_pairs")]
    streams = [api.PcmStream(c[0], c[1], c[2], c[3], chunk_samples=4096) for c, _ in cases]
    lcfg = config.spectrum_config(window_size=4096, hop=1024, channel_mode=config.CH_COMPLEX)
    load = api.Plan(lcfg).upload()
    y = torch.from_numpy(ov.burst_signal(4096, 1024, 4000, 2, lcfg["sample_rate"], seed=5)).to(gpu)     # (a render of some 0.3 ms)
    side = torch.cuda.Stream(device=gpu)
    image = load.render(y, stream=side.cuda_stream)
    side.synchronize()
    first = image.clone()
    for it in range(8):                                                # (either kind of feed, four times each)
        for ((cfg, fmt, channels, cmap, raw, n, F, plan, planar), want), s in zip(cases, streams):
            for _ in range(8):
                load.render(y, rgba=image, stream=side.cuda_stream)
            bits, out = _records(F, cfg["num_pairs"])
            s.reset()
            s.set_track(0, 0.5, out, F)
            _feed(s, raw, channels * BYTES[fmt], 0, n, "overview" if it % 2 else "plain", 5, flush=True, lines=False)
            assert (bits[:F] == want).all() and (bits[F:] == SENTINEL).all(), (it, cfg["window_size"])
    side.synchronize()
    assert torch.equal(image, first)
    for s in streams:
        s.close()


def test_create_arm_feed_destroy_gives_the_memory_back(gpu):
    """200 create -> arm -> feed -> destroy cycles after 5 to settle the allocators (64 MiB of slack, as tests/test_gpu_pcm.py)"""
    import torch
    name = "w256_f32_two_pairs"
    cfg, fmt, channels, cmap, raw, n, F, plan, planar = _case(name)
    fb, Cn = channels * BYTES[fmt], cfg["num_pairs"]
    combos = ((0, 0.5), (1, 0.03), (0, 0.97))

    def cycle(i):
        graph, mf = combos[i % 3]
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=(500, 2000)[i % 2])
        bits, out = _records(F, Cn)
        s.set_track(graph, mf, out, F)
        _feed(s, raw, fb, 0, n // 2, "plain", lines=bool(i % 4 == 0))
        _feed(s, raw, fb, n // 2, n - n // 2, "plain" if i % 3 else "overview", 5, flush=True, lines=False)
        s.close()
        return bits[:F], _want(name, graph, mf)

    for i in range(5):
        cycle(i)
    gc.collect()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for i in range(200):
        got, want = cycle(i)
        assert (got == want).all(), i
    gc.collect()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    if "PYTEST_XDIST_WORKER" not in os.environ:                   # (the figure is the DEVICE's: under pytest -n the other workers' allocations move it)
        assert free0 - free1 < 64 << 20, f"device memory: {(free0 - free1) / 2**20:.1f} MiB fewer free after 200 cycles"
