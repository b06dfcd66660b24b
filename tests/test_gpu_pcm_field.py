"""The stereo-field lane inside the PCM stream on the GPU (sgz_pcm_stream_set_field, _field_for, _field_state, _flush_field; csrc/pcm.hip,
csrc/field_columns.hip), on the cases of tests/test_gpu_pcm_level.py.

Byte for byte, no tolerance: the lane's records after the flush == tests/field_ref.py of the numpy-converted planar floats, for every m,
chunk_samples, kind of feed and way of cutting the stream into feeds; everything the feeds return == an unarmed twin's, and every other
lane's records == those of a twin without this lane."""
import gc
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_ref as fr  # noqa: E402
from test_gpu_pcm import BYTES  # noqa: E402
from test_gpu_pcm_level import CHUNKS, FRAMES, HOP, K, N, NAMES, W, _case, _feed, _kinds, _same  # noqa: E402
from test_gpu_pcm_loudness import filt  # noqa: E402
from test_gpu_pcm_overview import _feed_sizes  # noqa: E402  (the cuts)

pytestmark = pytest.mark.gpu

MS = (64, 100, 333)
E = api.SGZ_EINVAL
_wants = {}
assert 1000 in CHUNKS


def _want(name, m):
    if (name, m) not in _wants:
        _wants[name, m] = fr.columns(_case(name)[5], m)[0]
    return _wants[name, m]


def _same_records(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a, fr.DTYPE).tobytes() == np.ascontiguousarray(b, fr.DTYPE).tobytes()


def _sentinel(columns, pairs):
    return np.full((columns, pairs, 528), 0xA5, np.uint8).view(fr.DTYPE).reshape(columns, pairs)


def _error():
    return api.lib().sgz_last_error().decode()


def _run(s, raw, fb, sizes, mode, m=0, out=None):
    """feeds the sizes in turn; armed (m > 0): checks field_for / field_state around every feed against sgz_overview_step chained, then
    flushes the lane -> (everything the feeds returned, the lane's records)"""
    returned, at, written, open_ = [], 0, 0, 0
    kinds = _kinds(mode, len(sizes))
    for size, kind in zip(sizes, kinds):
        if m:
            columns, left = api.overview_step(m, open_, size, False)
            assert s.field_for(size) == columns and s.field_for(size, True) == api.overview_step(m, open_, size, True)[0]
        returned.append(_feed(s, raw, fb, at, size, kind))
        at += size
        if m:
            written, open_ = written + columns, left
            assert s.field_state() == (written, open_), (size, kind)
    if kinds[-1] == "overview":
        returned.append(_feed(s, raw, fb, at, 0, "overview", flush=True))
    if not m:
        return returned, None
    s.flush_field()
    written += open_ > 0
    assert s.field_state() == (written, 0)
    s.flush_field()                                                    # nothing open: nothing happens
    assert s.field_state() == (written, 0)
    return returned, out[:written].copy()


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", NAMES)
def test_lane_equals_the_definition_and_leaves_the_render_alone(gpu, name, chunk):
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb, pairs = channels * BYTES[fmt], planar.shape[0] // 2
    rng = np.random.default_rng(len(name) + chunk)
    armed = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
    twin = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
    for mode in ("plain", "overview", "mixed"):                        # both kinds of feed, and one after the other
        sizes = _feed_sizes(rng, N, W, HOP)
        twin.reset()
        unarmed, _ = _run(twin, raw, fb, sizes, mode)
        for m in MS:
            want = _want(name, m)
            out = _sentinel(want.shape[0] + 2, pairs)
            armed.reset()
            armed.set_field(m, out)
            got, field = _run(armed, raw, fb, sizes, mode, m, out)
            what = (name, chunk, mode, m, sizes)
            assert _same_records(field, want), what
            assert out[want.shape[0]:].tobytes() == _sentinel(2, pairs).tobytes(), what
            assert _same(got, unarmed), what
        armed.reset()                                                  # the whole file in one feed: the pieces of chunk_samples inside it
        out = np.zeros(_want(name, 100).shape, fr.DTYPE)
        armed.set_field(100, out)
        _, field = _run(armed, raw, fb, [N], mode, 100, out)
        assert _same_records(field, _want(name, 100)), (name, chunk, mode)
    armed.set_field(0)
    armed.reset()
    disarmed, _ = _run(armed, raw, fb, sizes, "mixed")
    assert _same(disarmed, unarmed) and armed.field_state() == (0, 0) and armed.field_for(N) == 0
    armed.close(); twin.close()


def test_all_six_lanes_armed_together(gpu):
    """against an unarmed twin (what the feeds return) and a twin with the five other lanes (their records): byte for byte"""
    name = "f32_two_pairs"
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb, D, pairs = channels * BYTES[fmt], planar.shape[0], planar.shape[0] // 2
    ms = {"waveform": 7, "level": 16, "truepeak": 33, "loudness": 50}
    rows = {"waveform": (D, 8), "level": (pairs, 80), "truepeak": (D, 16), "loudness": (D, 32)}
    rng = np.random.default_rng(23)
    fm = 100
    for mode in ("plain", "mixed"):
        sizes = _feed_sizes(rng, N, W, HOP)
        results = []
        for lanes in ("none", "five", "six"):
            s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
            bufs = {lane: np.full((N // m + 1,) + rows[lane], 0xA5, np.uint8) for lane, m in ms.items()}
            track = np.full((FRAMES, pairs, 48), 0xA5, np.uint8)
            out = _sentinel(_want(name, fm).shape[0], pairs)
            if lanes != "none":
                for lane, m in ms.items():
                    if lane == "loudness":
                        s.set_loudness(filt(8000), m, bufs[lane])
                    else:
                        getattr(s, "set_" + lane)(m, bufs[lane])
                s.set_track(0, 0.5, track, FRAMES)
            if lanes == "six":
                s.set_field(fm, out)
            got, field = _run(s, raw, fb, sizes, mode, fm if lanes == "six" else 0, out)
            if lanes != "none":
                for lane in ms:
                    getattr(s, "flush_" + lane)()
                assert s.track_state() == FRAMES
            results.append((got, [bufs[lane].copy() for lane in ms] + [track.copy()]))
            if lanes == "six":
                assert _same_records(field, _want(name, fm)), mode
            s.close()
        none, five, six = results
        assert _same(none[0], five[0]) and _same(none[0], six[0]), mode
        assert all(a.tobytes() == b.tobytes() for a, b in zip(five[1], six[1])), mode
        assert not any((b == 0xA5).all() for b in six[1])


def test_a_piece_without_a_frame_still_delivers_its_records(gpu):
    name = "f32_two_pairs"
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb, pairs, m = channels * BYTES[fmt], planar.shape[0] // 2, 64
    want = _want(name, m)
    for chunk in (0, 100):                                             # one piece per feed; several frameless pieces inside a feed
        for kind in ("plain", "overview"):
            s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
            out = np.zeros(want.shape, fr.DTYPE)
            s.set_field(m, out)
            at = 0
            for size in (199, 200, 201, 202, 203):                     # 1005 samples: never a window
                assert s.frames_for(size) == 0
                got = _feed(s, raw, fb, at, size, kind)
                at += size
                assert got[1].shape[0] == 0
                assert s.field_state() == (at // m, at % m)
                assert _same_records(out[:at // m], want[:at // m]), (chunk, kind, at)       # delivered when the feed returns
                assert out[at // m:].tobytes() == bytes(528 * pairs * (want.shape[0] - at // m))
            s.close()


def test_pinned_and_pageable_destinations(gpu):
    import torch
    for name in ("s16_3ch", "f32_two_pairs"):
        cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
        fb, pairs = channels * BYTES[fmt], planar.shape[0] // 2
        for m in (64, 333):
            want = _want(name, m)
            s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
            pinned = torch.zeros((want.shape[0], pairs, 528), dtype=torch.uint8).pin_memory()
            view = pinned.numpy().view(fr.DTYPE).reshape(want.shape)
            s.set_field(m, pinned)
            _run(s, raw, fb, [N // 3, N - N // 3], "plain", m, view)
            assert _same_records(view, want), (name, m)
            s.reset()
            pageable = np.zeros(want.shape, fr.DTYPE)
            s.set_field(m, pageable)                                   # the same stream, now through the pinned twins
            _run(s, raw, fb, [N // 3, N - N // 3], "overview", m, pageable)
            assert _same_records(pageable, want), (name, m)
            s.close()


def test_draining_through_a_small_buffer(gpu):
    name = "s24"
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb, pairs, m, cap = channels * BYTES[fmt], planar.shape[0] // 2, 64, 7
    want = _want(name, m)
    rng = np.random.default_rng(3)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    small = [np.zeros((cap, pairs), fr.DTYPE), np.zeros((cap, pairs), fr.DTYPE)]
    which, kept, at, rearmed = 0, [], 0, 0
    s.set_field(m, small[0])
    while at < N:
        size = min(int(rng.integers(0, (cap - 1) * m)), N - at)
        written, open_ = s.field_state()
        if written + s.field_for(size) > cap:                          # drain: keep what is there, re-arm with the other buffer -- the open column stays
            kept.append(small[which][:written].copy())
            which ^= 1
            s.set_field(m, small[which])                               # the same m
            assert s.field_state() == (0, open_)
            rearmed += 1
        _feed(s, raw, fb, at, size, "plain")
        at += size
    written, open_ = s.field_state()
    if written == cap:                                                 # (the flush needs a column of its own)
        kept.append(small[which][:written].copy())
        which ^= 1
        s.set_field(m, small[which])
    s.flush_field()
    kept.append(small[which][:s.field_state()[0]].copy())
    assert rearmed >= 5 and _same_records(np.concatenate(kept), want)
    s.close()


def test_counts_state_refusals_and_reset(gpu):
    name = "f32_two_pairs"
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    P, fb, pairs = cfg["axis_points"], channels * BYTES[fmt], planar.shape[0] // 2
    L = api.lib()
    m = 400
    want = _want(name, m)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    twin = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    assert s.field_for(N) == 0 and s.field_state() == (0, 0)           # disarmed
    assert L.sgz_pcm_stream_flush_field(s.h) == E
    assert _error() == "sgz_pcm_stream_flush_field: the lane is off (sgz_pcm_stream_set_field)"
    assert L.sgz_pcm_stream_set_field(None, m, None, 0) == E and L.sgz_pcm_stream_set_field(s.h, m, None, 3) == E
    assert L.sgz_pcm_stream_field_state(None, None, None) == E
    odd = np.zeros(3 * pairs * 528 + 8, np.uint8)
    assert L.sgz_pcm_stream_set_field(s.h, m, odd.ctypes.data + 1 + (-odd.ctypes.data) % 8, 3) == E        # not aligned to 8 bytes
    # 0 < m < 64: refused, the lane stays off
    out = np.zeros(want.shape, fr.DTYPE)
    for short in (1, 63):
        assert L.sgz_pcm_stream_set_field(s.h, short, out.ctypes.data, out.shape[0]) == E
        assert _error() == "sgz_pcm_stream_set_field: m >= 64 samples per column (a 528-byte record per pair for fewer would read back more than the samples)"
        assert s.field_for(N) == 0
    s.set_field(64, out)
    assert s.field_for(N) == N // 64
    first = 1400                                                       # three columns and 200 samples open; W + hop <= 1400: two frames
    small = np.zeros((2, pairs), fr.DTYPE)
    s.set_field(m, small)
    assert s.field_for(first) == 3 and s.field_for(first, True) == 4 and s.frames_for(first) == 2
    big_rgba = np.zeros((FRAMES, P, 4), np.uint8)
    peaks = np.zeros((FRAMES, pairs, P), np.float32)
    # a capacity below what the feed closes: refused by both kinds before anything is consumed
    message = "sgz_pcm_stream: the feed closes more stereo-field columns than the buffer has left (sgz_pcm_stream_field_for; re-arm with sgz_pcm_stream_set_field)"
    assert s.feed_into(raw, first, big_rgba, None, FRAMES)[0] == E and _error() == message
    assert s.feed_overview_into(raw, first, K, False, big_rgba, peaks, FRAMES)[0] == E and _error() == message
    assert small.tobytes() == bytes(small.nbytes) and not big_rgba.any() and not peaks.any()
    assert s.field_state() == (0, 0) and s.frames_for(first) == 2 and s.open_frames() == 0
    # ... the next feed's outputs are those of a stream that never saw the refusals
    s.set_field(m, out)
    a = _feed(s, raw, fb, 0, first, "plain")
    b = _feed(twin, raw, fb, 0, first, "plain")
    assert _same([a], [b]) and a[1].shape[0] == 2 and s.field_state() == (3, 200)
    assert _same_records(out[:3], want[:3])
    # another m while samples are open: refused, the lane as it was
    assert L.sgz_pcm_stream_set_field(s.h, m + 1, out.ctypes.data, out.shape[0]) == E
    assert _error() == "sgz_pcm_stream_set_field: m differs from the open column's -- flush it (sgz_pcm_stream_flush_field), disarm or reset first"
    assert s.field_state() == (3, 200) and s.field_for(200) == 1
    # the level lane's m is its own: armed beside an open stereo-field column with another m
    level = np.zeros((4, pairs), api.LEVEL_DTYPE)
    s.set_level(m + 1, level)
    assert s.field_state() == (3, 200) and s.level_state() == (0, 0)
    s.set_level(0)
    # the flush needs a column of its own
    s.set_field(m, small)
    _feed(s, raw, fb, first, 600, "plain")
    assert s.field_state() == (2, 0)
    _feed(s, raw, fb, first + 600, 30, "plain")
    assert s.field_state() == (2, 30) and L.sgz_pcm_stream_flush_field(s.h) == E and s.field_state() == (2, 30)
    assert _error() == "sgz_pcm_stream_flush_field: no column left in the buffer (re-arm with sgz_pcm_stream_set_field)"
    assert _same_records(small, want[3:5])
    # reset drops the open column and restarts the cursor; the same file again gives the same records
    s.reset()
    assert s.field_state() == (0, 0)
    s.set_field(m, out)
    out[:] = np.zeros((), fr.DTYPE)
    _, field = _run(s, raw, fb, [N], "plain", m, out)
    assert _same_records(field, want)
    # disarming drops the open column too: another m is taken afterwards
    s.reset()
    _feed(s, raw, fb, 0, 430, "plain")
    assert s.field_state() == (1, 30)
    s.set_field(0)
    assert s.field_state() == (0, 0) and s.field_for(1000) == 0
    s.set_field(70, out)
    assert s.field_state() == (0, 0) and s.field_for(150) == 2
    s.close(); twin.close()


def test_create_feed_destroy_gives_the_memory_back(gpu):
    """200 create -> armed feeds -> flush -> destroy cycles after 5 to settle the allocators (64 MiB of slack, as tests/test_gpu_pcm.py)"""
    import torch
    name = "s16_3ch"
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb = channels * BYTES[fmt]

    def cycle(i):
        m = MS[i % 3]
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=(500, 2000)[i % 2])
        out = np.zeros(_want(name, m).shape, fr.DTYPE)
        s.set_field(m, out)
        _feed(s, raw, fb, 0, N // 2, "plain")
        _feed(s, raw, fb, N // 2, N - N // 2, "plain" if i % 3 else "overview")
        s.flush_field()
        s.close()
        return out

    for i in range(5):
        cycle(i)
    gc.collect()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for i in range(200):
        assert _same_records(cycle(i), _want(name, MS[i % 3])), i
    gc.collect()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    if "PYTEST_XDIST_WORKER" not in os.environ:                   # (the figure is the DEVICE's: under pytest -n the other workers' allocations move it)
        assert free0 - free1 < 64 << 20, f"device memory: {(free0 - free1) / 2**20:.1f} MiB fewer free after 200 cycles"
