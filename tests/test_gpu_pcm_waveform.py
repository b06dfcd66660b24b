"""The waveform lane inside the PCM stream on the GPU (sgz_pcm_stream_set_waveform, _waveform_for, _waveform_state, _flush_waveform;
csrc/pcm.hip, csrc/wave_columns.hip).

Bit for bit (uint32 views), no tolerance: the lane's columns after the flush == tests/wave_ref.py of the numpy-converted planar floats, for
every m, chunk_samples, kind of feed and way of cutting the stream into feeds; and the image, lines, overview image and peaks of an armed
stream == an unarmed twin's, byte for byte."""
import gc
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wave_ref as wr  # noqa: E402
from test_gpu_pcm import BYTES  # noqa: E402
from test_gpu_pcm_overview import _case, _feed_sizes  # noqa: E402  (the cases, converted with test_gpu_pcm's convert_ref / to_bytes; the cuts)

pytestmark = pytest.mark.gpu

NAMES = ("w64", "w256_two_pairs", "odd_hop")
CHUNKS = (0, 1000, 4096)
K = 3                                                                  # frames per overview column of the overview feeds
E = api.SGZ_EINVAL
_wants = {}


def _want(name, m):
    if (name, m) not in _wants:
        _wants[name, m] = wr.columns_of(_case(name)[8], m)[0]
    return _wants[name, m]


def _ms(n):
    return (1, 5, 16, 1000, 4097, n + 1)


def _feed(s, raw, fb, at, size, kind, flush=False):
    """one feed of either kind -> what it returned, as a tuple of byte arrays"""
    pcm = raw[at * fb:(at + size) * fb] if size else None
    if kind == "plain":
        rgba, lines, _ = s.feed(pcm if size else raw[:0], nsamples=size, want_lines=True)
        return ("plain", rgba, lines.view(np.uint32))
    rgba, peaks, _ = s.feed_overview(pcm, K, flush=flush, nsamples=size, want_peaks=True)
    return ("overview", rgba, peaks.view(np.uint32))


def _kinds(mode, count):
    if mode == "mixed":                                                # plain feeds, then overview feeds (the other order is refused while a column is open)
        return ["plain"] * (count // 2) + ["overview"] * (count - count // 2)
    return [mode] * count


def _run(s, raw, fb, sizes, mode, m=0, out=None):
    """feeds the sizes in turn; armed (m > 0): checks waveform_for / waveform_state around every feed against sgz_overview_step chained, then
    flushes the lane -> (everything the feeds returned, the lane's columns)"""
    returned, at, written, open_ = [], 0, 0, 0
    kinds = _kinds(mode, len(sizes))
    for size, kind in zip(sizes, kinds):
        if m:
            columns, left = api.overview_step(m, open_, size, False)
            assert s.waveform_for(size) == columns and s.waveform_for(size, True) == api.overview_step(m, open_, size, True)[0]
        returned.append(_feed(s, raw, fb, at, size, kind))
        at += size
        if m:
            written, open_ = written + columns, left
            assert s.waveform_state() == (written, open_), (size, kind)
    if kinds[-1] == "overview":
        returned.append(_feed(s, raw, fb, at, 0, "overview", flush=True))
    if not m:
        return returned, None
    s.flush_waveform()
    written += open_ > 0
    assert s.waveform_state() == (written, 0)
    s.flush_waveform()                                                 # nothing open: nothing happens
    assert s.waveform_state() == (written, 0)
    return returned, out[:written].view(np.uint32).copy()


def _same(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) for x, y in zip(a, b))


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", NAMES)
def test_lane_equals_the_definition_and_leaves_the_render_alone(gpu, name, chunk):
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case(name)
    W, hop, fb, D = cfg["window_size"], cfg["hop"], channels * BYTES[fmt], planar.shape[0]
    rng = np.random.default_rng(len(name) + chunk)
    armed = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
    twin = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
    runs = 0
    for mode in ("plain", "overview", "mixed"):
        sizes = _feed_sizes(rng, n, W, hop)
        assert 0 in sizes and 1 in sizes and any(0 < v < hop for v in sizes), sizes
        twin.reset()
        unarmed, _ = _run(twin, raw, fb, sizes, mode)
        if mode == "plain":
            assert np.array_equal(np.concatenate([r[1] for r in unarmed]), rgba)
        for m in _ms(n):
            want = _want(name, m)
            out = np.full((want.shape[0] + 2, D, 2), np.float32(-77.0))
            armed.reset()
            armed.set_waveform(m, out)
            got, wave = _run(armed, raw, fb, sizes, mode, m, out)
            what = (name, chunk, mode, m, sizes)
            assert np.array_equal(wave, want), what
            assert (out[want.shape[0]:] == np.float32(-77.0)).all(), what
            assert _same(got, unarmed), what
            runs += 1
        one = [n]                                                      # the whole file in one feed: the pieces of chunk_samples inside it
        armed.reset()
        out = np.zeros((_want(name, 16).shape[0], D, 2), np.float32)
        armed.set_waveform(16, out)
        _, wave = _run(armed, raw, fb, one, mode, 16, out)
        assert np.array_equal(wave, _want(name, 16)), (name, chunk, mode)
    assert runs == 18
    armed.set_waveform(0)
    armed.reset()
    disarmed, _ = _run(armed, raw, fb, sizes, "mixed")
    assert _same(disarmed, unarmed) and armed.waveform_state() == (0, 0) and armed.waveform_for(n) == 0
    armed.close(); twin.close()


def test_a_piece_without_a_frame_still_delivers_its_columns(gpu):
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case("w256_two_pairs")
    W, fb, D, m = cfg["window_size"], channels * BYTES[fmt], planar.shape[0], 5
    want = _want("w256_two_pairs", m)
    for chunk in (0, 16):                                              # one piece per feed; several frameless pieces inside a feed
        for kind in ("plain", "overview"):
            s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
            out = np.zeros((want.shape[0], D, 2), np.float32)
            s.set_waveform(m, out)
            at = 0
            for size in (49, 50, 51, 52, 53):                          # 255 samples: never a window
                assert s.frames_for(size) == 0
                got = _feed(s, raw, fb, at, size, kind)
                at += size
                assert got[1].shape[0] == 0
                assert s.waveform_state() == (at // m, at % m)
                assert np.array_equal(out[:at // m].view(np.uint32), want[:at // m]), (chunk, kind, at)       # delivered when the feed returns
                assert not out[at // m:].any()
            s.close()


def test_pinned_and_pageable_destinations(gpu):
    import torch
    for name in ("w64", "odd_hop"):
        cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case(name)
        fb, D = channels * BYTES[fmt], planar.shape[0]
        for m in (5, 1000):
            want = _want(name, m)
            s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
            pinned = torch.zeros((want.shape[0], D, 2), dtype=torch.float32).pin_memory()
            s.set_waveform(m, pinned)
            _run(s, raw, fb, [n // 3, n - n // 3], "plain", m, pinned.numpy())
            assert np.array_equal(pinned.numpy().view(np.uint32), want), (name, m)
            s.reset()
            pageable = np.zeros((want.shape[0], D, 2), np.float32)
            s.set_waveform(m, pageable)                                # the same stream, now through the pinned twins
            _run(s, raw, fb, [n // 3, n - n // 3], "overview", m, pageable)
            assert np.array_equal(pageable.view(np.uint32), want), (name, m)
            s.close()


def test_draining_through_a_small_buffer(gpu):
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case("odd_hop")
    fb, D, m, cap = channels * BYTES[fmt], planar.shape[0], 16, 7
    want = _want("odd_hop", m)
    rng = np.random.default_rng(3)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=64)
    small = [np.zeros((cap, D, 2), np.float32), np.zeros((cap, D, 2), np.float32)]
    which, kept, at, rearmed = 0, [], 0, 0
    s.set_waveform(m, small[0])
    while at < n:
        size = min(int(rng.integers(0, (cap - 1) * m)), n - at)
        written, open_ = s.waveform_state()
        if written + s.waveform_for(size) > cap:                       # drain: keep what is there, re-arm with the other buffer -- the open column stays
            kept.append(small[which][:written].copy())
            which ^= 1
            s.set_waveform(m, small[which])
            assert s.waveform_state() == (0, open_)
            rearmed += 1
        _feed(s, raw, fb, at, size, "plain")
        at += size
    written, open_ = s.waveform_state()
    if written == cap:                                                 # (the flush needs a column of its own)
        kept.append(small[which][:written].copy())
        which ^= 1
        s.set_waveform(m, small[which])
    s.flush_waveform()
    kept.append(small[which][:s.waveform_state()[0]].copy())
    assert rearmed >= 5 and np.array_equal(np.concatenate(kept).view(np.uint32), want)
    s.close()


def test_counts_state_and_refusals(gpu):
    name = "w256_two_pairs"
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case(name)
    W, hop, P, fb, D = cfg["window_size"], cfg["hop"], cfg["axis_points"], channels * BYTES[fmt], planar.shape[0]
    L = api.lib()
    m = 100
    want = _want(name, m)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    twin = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    assert s.waveform_for(n) == 0 and s.waveform_state() == (0, 0)     # disarmed
    assert L.sgz_pcm_stream_flush_waveform(s.h) == E
    assert L.sgz_pcm_stream_set_waveform(None, m, None, 0) == E and L.sgz_pcm_stream_set_waveform(s.h, m, None, 3) == E
    assert L.sgz_pcm_stream_waveform_state(None, None, None) == E
    first = 350                                                        # three columns and 50 samples open; W + hop <= 350: two frames
    small = np.zeros((2, D, 2), np.float32)
    s.set_waveform(m, small)
    assert s.waveform_for(first) == 3 and s.waveform_for(first, True) == 4 and s.frames_for(first) == 2
    big_rgba = np.zeros((F, P, 4), np.uint8)
    peaks = np.zeros((F, cfg["num_pairs"], P), np.float32)
    # a capacity below what the feed closes: refused by both kinds, nothing consumed
    assert s.feed_into(raw, first, big_rgba, None, F)[0] == E and "waveform" in L.sgz_last_error().decode()
    assert s.feed_overview_into(raw, first, K, False, big_rgba, peaks, F)[0] == E
    assert not small.any() and not big_rgba.any() and not peaks.any()
    assert s.waveform_state() == (0, 0) and s.frames_for(first) == 2 and s.open_frames() == 0
    # ... the next feed's outputs are those of a stream that never saw the refusals
    out = np.zeros((want.shape[0], D, 2), np.float32)
    s.set_waveform(m, out)
    a = _feed(s, raw, fb, 0, first, "plain")
    b = _feed(twin, raw, fb, 0, first, "plain")
    assert _same([a], [b]) and a[1].shape[0] == 2 and s.waveform_state() == (3, 50)
    assert np.array_equal(out[:3].view(np.uint32), want[:3])
    # another m while samples are open: refused, the lane as it was
    assert L.sgz_pcm_stream_set_waveform(s.h, m + 1, out.ctypes.data, out.shape[0]) == E
    assert s.waveform_state() == (3, 50) and s.waveform_for(50) == 1
    # the flush needs a column of its own
    s.set_waveform(m, small)
    _feed(s, raw, fb, first, 150, "plain")
    assert s.waveform_state() == (2, 0)
    _feed(s, raw, fb, first + 150, 30, "plain")
    assert s.waveform_state() == (2, 30) and L.sgz_pcm_stream_flush_waveform(s.h) == E and s.waveform_state() == (2, 30)
    assert np.array_equal(small.view(np.uint32), want[3:5])
    # reset drops the open column and restarts the cursor; the same file again gives the same columns
    s.reset()
    assert s.waveform_state() == (0, 0)
    s.set_waveform(m, out)
    out[:] = 0
    _, wave = _run(s, raw, fb, [n], "plain", m, out)
    assert np.array_equal(wave, want)
    # disarming drops the open column too: another m is taken afterwards
    s.reset()
    _feed(s, raw, fb, 0, 130, "plain")
    assert s.waveform_state() == (1, 30)
    s.set_waveform(0)
    assert s.waveform_state() == (0, 0) and s.waveform_for(1000) == 0
    s.set_waveform(7, out)
    assert s.waveform_state() == (0, 0) and s.waveform_for(15) == 2
    s.close(); twin.close()


def test_create_feed_destroy_gives_the_memory_back(gpu):
    """200 create -> armed feeds -> flush -> destroy cycles after 5 to settle the allocators (64 MiB of slack, as tests/test_gpu_pcm.py)"""
    import torch
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case("w256_two_pairs")
    fb, D = channels * BYTES[fmt], planar.shape[0]
    ms = (5, 16, 1000, 4097)

    def cycle(i):
        m = ms[i % 4]
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=(500, 2000)[i % 2])
        out = np.zeros((_want("w256_two_pairs", m).shape[0], D, 2), np.float32)
        s.set_waveform(m, out)
        _feed(s, raw, fb, 0, n // 2, "plain")
        _feed(s, raw, fb, n // 2, n - n // 2, "plain" if i % 3 else "overview")
        s.flush_waveform()
        s.close()
        return out.view(np.uint32)

    for i in range(5):
        cycle(i)
    gc.collect()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for i in range(200):
        assert np.array_equal(cycle(i), _want("w256_two_pairs", ms[i % 4])), i
    gc.collect()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    if "PYTEST_XDIST_WORKER" not in os.environ:                   # (the figure is the DEVICE's: under pytest -n the other workers' allocations move it)
        assert free0 - free1 < 64 << 20, f"device memory: {(free0 - free1) / 2**20:.1f} MiB fewer free after 200 cycles"
