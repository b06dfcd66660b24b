"""The loudness lane inside the PCM stream on the GPU (sgz_pcm_stream_set_loudness, _loudness_for, _loudness_state, _flush_loudness;
csrc/pcm.hip, csrc/loudness_columns.hip).

Byte for byte, no tolerance: the lane's records after the flush == tests/loudness_ref.py of the numpy-converted planar floats, for every m,
chunk_samples (3 L + 1, W - 1, the default), kind of feed and way of cutting the stream into feeds; == the stage call on the whole buffer;
and everything the feeds return == an unarmed twin's.  The cases and the feeds are those of tests/test_gpu_pcm_level.py."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness_ref as lr  # noqa: E402
import wave_ref as wr  # noqa: E402
from test_gpu_pcm import BYTES  # noqa: E402
from test_gpu_pcm_level import FRAMES, HOP, K, N, W, _case, _feed, _kinds, _same  # noqa: E402  (cases, feeds, the feeds' comparison)
from test_gpu_pcm_overview import _feed_sizes  # noqa: E402  (random cuts)

pytestmark = pytest.mark.gpu

E = api.SGZ_EINVAL
NAMES = ("s16_3ch", "f32_two_pairs")                                 # 16-bit and float PCM
_wants, _filters = {}, {}


def filt(which):
    if which not in _filters:
        _filters[which] = api.loudness_filter(lr.TINY.b, lr.TINY.a, lr.TINY.W, lr.TINY.L) if which == "tiny" else api.loudness_filter_for_rate(which)
    return _filters[which]


def _want(name, which, m):
    if (name, which, m) not in _wants:
        _wants[name, which, m] = lr.records_of(_case(name)[5], filt(which), m)[0]
    return _wants[name, which, m]


def _same_records(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a, lr.DTYPE).tobytes() == np.ascontiguousarray(b, lr.DTYPE).tobytes()


def _sentinel(columns, channels):
    return np.full((columns, channels, 32), 0xA5, np.uint8).view(lr.DTYPE).reshape(columns, channels)


def _cut_sets(f, rng):
    """the stage call's cut points as feed sizes: two and three cuts around L and W, and a random set with empty and tiny feeds"""
    Wf, L = f.W, f.L
    sets = [[L - 1, L + 1], [L, Wf + 1], [Wf - 1, Wf], [1, Wf, Wf + L + 7]]
    out = [[b - a for a, b in zip([0] + cuts, cuts + [N])] for cuts in sets]
    return out + [_feed_sizes(rng, N, W, HOP)]


def _run(s, raw, fb, sizes, mode, m=0, out=None, at=0, flush=True):
    """feeds the sizes in turn; armed (m > 0): checks loudness_for / loudness_state around every feed against sgz_overview_step chained, then
    flushes the lane -> (everything the feeds returned, the lane's records)"""
    returned = []
    written, open_ = s.loudness_state() if m else (0, 0)
    kinds = _kinds(mode, len(sizes))
    for size, kind in zip(sizes, kinds):
        if m:
            columns, left = api.overview_step(m, open_, size, False)
            assert s.loudness_for(size) == columns and s.loudness_for(size, True) == api.overview_step(m, open_, size, True)[0]
        returned.append(_feed(s, raw, fb, at, size, kind))
        at += size
        if m:
            written, open_ = written + columns, left
            assert s.loudness_state() == (written, open_), (size, kind)
    if kinds[-1] == "overview":
        returned.append(_feed(s, raw, fb, at, 0, "overview", flush=True))
    if not m:
        return returned, None
    if flush:
        s.flush_loudness()
        written += open_ > 0
        assert s.loudness_state() == (written, 0)
        s.flush_loudness()                                              # nothing open: nothing happens
        assert s.loudness_state() == (written, 0)
    return returned, out[:written].copy()


@pytest.mark.parametrize("chunk", ["3L+1", "W-1", 0])
@pytest.mark.parametrize("which", ["tiny", 8000])
@pytest.mark.parametrize("name", NAMES)
def test_lane_equals_the_definition_and_leaves_the_render_alone(gpu, name, which, chunk):
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    f = filt(which)
    chunk = {"3L+1": 3 * f.L + 1, "W-1": f.W - 1}.get(chunk, chunk)
    fb, D = channels * BYTES[fmt], planar.shape[0]
    rng = np.random.default_rng(len(name) + chunk)
    armed = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
    twin = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
    ms = (7, f.L + 1, 1000, 4097)
    for i, sizes in enumerate(_cut_sets(f, rng)):
        mode = ("plain", "overview", "mixed")[i % 3]
        twin.reset()
        unarmed, _ = _run(twin, raw, fb, sizes, mode)
        for m in (ms[i % 4], ms[(i + 1) % 4]):
            want = _want(name, which, m)
            out = _sentinel(want.shape[0] + 2, D)
            armed.reset()
            armed.set_loudness(f, m, out)
            got, records = _run(armed, raw, fb, sizes, mode, m, out)
            what = (name, which, chunk, mode, m, sizes)
            assert _same_records(records, want), what
            assert out[want.shape[0]:].tobytes() == _sentinel(2, D).tobytes(), what
            assert _same(got, unarmed), what
    armed.set_loudness(None, 0)
    armed.reset()
    disarmed, _ = _run(armed, raw, fb, sizes, mode)
    assert _same(disarmed, unarmed) and armed.loudness_state() == (0, 0) and armed.loudness_for(N) == 0
    armed.close(); twin.close()


@pytest.mark.parametrize("name", NAMES)
def test_lane_equals_the_stage_call_on_the_whole_buffer(gpu, name):
    import torch
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb, D = channels * BYTES[fmt], planar.shape[0]
    f, m = filt(8000), 480
    want = _want(name, 8000, m)
    dev = torch.from_numpy(planar).cuda()
    carry = torch.zeros(lr.carry_bytes(f) * D // 4, dtype=torch.int32, device="cuda")
    staged = torch.zeros((want.shape[0], D, 8), dtype=torch.int32, device="cuda")
    assert api.stage_loudness_columns(dev, N, D, N, f, 0, m, carry=carry, records=staged) == api.SGZ_OK
    torch.cuda.synchronize()
    staged = staged.cpu().numpy().view(lr.DTYPE).reshape(want.shape)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    out = np.zeros(want.shape, lr.DTYPE)
    s.set_loudness(f, m, out)
    _, records = _run(s, raw, fb, [N // 3, N - N // 3], "plain", m, out)
    assert _same_records(records, staged) and _same_records(records, want)
    s.close()


def test_pinned_and_pageable_destinations(gpu):
    import torch
    name = "s16_3ch"
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb, D, f = channels * BYTES[fmt], planar.shape[0], filt(8000)
    for m in (5, 1000):
        want = _want(name, 8000, m)
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
        pinned = torch.zeros((want.shape[0], D, 32), dtype=torch.uint8).pin_memory()
        view = pinned.numpy().view(lr.DTYPE).reshape(want.shape)
        s.set_loudness(f, m, pinned)
        _run(s, raw, fb, [N // 3, N - N // 3], "plain", m, view)
        assert _same_records(view, want), m
        s.reset()
        pageable = np.zeros(want.shape, lr.DTYPE)
        s.set_loudness(f, m, pageable)                                 # the same stream, now through the pinned twins
        _run(s, raw, fb, [N // 3, N - N // 3], "overview", m, pageable)
        assert _same_records(pageable, want), m
        s.close()


def test_draining_through_a_small_buffer_keeps_the_history(gpu):
    cfg, fmt, channels, cmap, raw, planar, ints = _case("s24")
    fb, D, m, cap = channels * BYTES[fmt], planar.shape[0], 16, 7
    f = filt("tiny")
    want = _want("s24", "tiny", m)
    rng = np.random.default_rng(3)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=64)
    small = [np.zeros((cap, D), lr.DTYPE), np.zeros((cap, D), lr.DTYPE)]
    which, kept, at, rearmed = 0, [], 0, 0
    s.set_loudness(f, m, small[0])
    while at < N:
        size = min(int(rng.integers(0, (cap - 1) * m)), N - at)
        written, open_ = s.loudness_state()
        if written + s.loudness_for(size) > cap:                       # drain: re-arm with the other buffer -- the open column and the history stay
            kept.append(small[which][:written].copy())
            which ^= 1
            s.set_loudness(f, m, small[which])
            assert s.loudness_state() == (0, open_)
            rearmed += 1
        _feed(s, raw, fb, at, size, "plain")
        at += size
    written, open_ = s.loudness_state()
    if written == cap:                                                 # (the flush needs a column of its own)
        kept.append(small[which][:written].copy())
        which ^= 1
        s.set_loudness(f, m, small[which])
    s.flush_loudness()
    kept.append(small[which][:s.loudness_state()[0]].copy())
    assert rearmed >= 5 and _same_records(np.concatenate(kept), want)  # (a zeroed history or index at any re-arm would change the columns behind it)
    s.close()


def test_a_flush_in_mid_stream_keeps_the_history_and_the_grid(gpu):
    for name, which in (("s16_3ch", 8000), ("f32_two_pairs", "tiny")):
        cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
        f = filt(which)
        fb, D, m, cut = channels * BYTES[fmt], planar.shape[0], 16, 1003            # 1003 = 62 * 16 + 11: inside a segment of either filter
        v, has = lr.quantise(planar)
        head = lr.records_of(planar[:, :cut], f, m)[0]                              # the partial column closes as it stands
        tail = lr.records_of_integers(v[:, cut:], has[:, cut:], f, m, True, v[:, :cut], cut)[0]      # columns count from the flush on; the grid does not
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=500)
        out = np.zeros((head.shape[0] + tail.shape[0], D), lr.DTYPE)
        s.set_loudness(f, m, out)
        _run(s, raw, fb, [cut], "plain", m, out)
        assert s.loudness_state() == (head.shape[0], 0)
        _run(s, raw, fb, [700, N - cut - 700], "plain", m, out, at=cut)
        assert _same_records(out, np.concatenate([head, tail])), name
        fresh = lr.records_of(planar[:, cut:], f, m)[0]
        assert not _same_records(tail[:1], fresh[:1])                               # (the history matters to the first column behind the flush)
        s.close()


def test_counts_state_reset_and_refusals(gpu):
    name = "f32_two_pairs"
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    P, fb, D, pairs = cfg["axis_points"], channels * BYTES[fmt], planar.shape[0], planar.shape[0] // 2
    L = api.lib()
    import ctypes as C
    f, g = filt(8000), filt("tiny")
    m = 400
    want = _want(name, 8000, m)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    twin = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    assert s.loudness_for(N) == 0 and s.loudness_state() == (0, 0)     # disarmed
    assert L.sgz_pcm_stream_flush_loudness(s.h) == E
    assert L.sgz_pcm_stream_set_loudness(None, C.byref(f), m, None, 0) == E and L.sgz_pcm_stream_set_loudness(s.h, C.byref(f), m, None, 3) == E
    assert L.sgz_pcm_stream_set_loudness(s.h, None, m, None, 0) == E                                           # armed without a filter
    bad = api.loudness_filter([[0.0, 0.6, 0.0], [1.0, 0.0, 0.0]], [[0.0, 0.0], [0.0, 0.0]], 64, 16)
    assert L.sgz_pcm_stream_set_loudness(s.h, C.byref(bad), m, None, 0) == E and s.loudness_for(N) == 0       # a refused table arms nothing
    assert L.sgz_pcm_stream_set_loudness(s.h, C.byref(api.loudness_filter(lr.TINY.b, lr.TINY.a, 64, 24)), m, None, 0) == E
    assert L.sgz_pcm_stream_loudness_state(None, None, None) == E
    odd = np.zeros(3 * D * 32 + 8, np.uint8)
    assert L.sgz_pcm_stream_set_loudness(s.h, C.byref(f), m, odd.ctypes.data + 1 + (-odd.ctypes.data) % 8, 3) == E       # not aligned to 8 bytes
    first = 1400                                                       # three columns and 200 samples open; W + hop <= 1400: two frames
    small = np.zeros((2, D), lr.DTYPE)
    s.set_loudness(f, m, small)
    assert s.loudness_for(first) == 3 and s.loudness_for(first, True) == 4 and s.frames_for(first) == 2
    big_rgba = np.zeros((FRAMES, P, 4), np.uint8)
    peaks = np.zeros((FRAMES, pairs, P), np.float32)
    # a capacity below what the feed closes: refused by both kinds, nothing consumed
    assert s.feed_into(raw, first, big_rgba, None, FRAMES)[0] == E and "loudness" in L.sgz_last_error().decode()
    assert s.feed_overview_into(raw, first, K, False, big_rgba, peaks, FRAMES)[0] == E
    assert small.tobytes() == bytes(small.nbytes) and not big_rgba.any() and not peaks.any()
    assert s.loudness_state() == (0, 0) and s.frames_for(first) == 2 and s.open_frames() == 0
    # ... the next feed's outputs are those of a stream that never saw the refusals
    out = np.zeros(want.shape, lr.DTYPE)
    s.set_loudness(f, m, out)
    a = _feed(s, raw, fb, 0, first, "plain")
    b = _feed(twin, raw, fb, 0, first, "plain")
    assert _same([a], [b]) and a[1].shape[0] == 2 and s.loudness_state() == (3, 200)
    assert _same_records(out[:3], want[:3])
    # another m or another filter while samples are open: refused, the lane as it was
    assert L.sgz_pcm_stream_set_loudness(s.h, C.byref(f), m + 1, out.ctypes.data, out.shape[0]) == E
    assert L.sgz_pcm_stream_set_loudness(s.h, C.byref(g), m, out.ctypes.data, out.shape[0]) == E
    assert s.loudness_state() == (3, 200) and s.loudness_for(200) == 1
    # the flush needs a column of its own
    s.set_loudness(f, m, small)
    _feed(s, raw, fb, first, 600, "plain")
    assert s.loudness_state() == (2, 0)
    _feed(s, raw, fb, first + 600, 30, "plain")
    assert s.loudness_state() == (2, 30) and L.sgz_pcm_stream_flush_loudness(s.h) == E and s.loudness_state() == (2, 30)
    assert _same_records(small, want[3:5])
    # reset drops the open column, zeroes the history and the index and restarts the cursor: the same file again gives a fresh stream's records
    s.reset()
    assert s.loudness_state() == (0, 0)
    s.set_loudness(f, m, out)
    out[:] = np.zeros((), lr.DTYPE)
    _, records = _run(s, raw, fb, [N], "plain", m, out)
    assert _same_records(records, want)
    # ... and so does a reset in mid-stream, at an index that is no multiple of L
    r = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    short = np.zeros((10, D), lr.DTYPE)
    r.set_loudness(g, 4, short)
    _feed(r, raw, fb, 3000, 30, "plain")
    r.reset()
    assert r.loudness_state() == (0, 0)
    _feed(r, raw, fb, 0, 8, "plain")
    assert r.loudness_state() == (2, 0) and _same_records(short[:2], _want(name, "tiny", 4)[:2])
    assert not _same_records(_want(name, "tiny", 4)[:1], lr.records_of(planar[:, :4], g, 4, True, lr.quantise(planar[:, 3000:3030])[0], 30)[0])
    r.close()
    # disarming drops the open column, the history and the index too: another m and another filter are taken afterwards, from rest
    s.reset()
    _feed(s, raw, fb, 0, 430, "plain")
    assert s.loudness_state() == (1, 30)
    s.set_loudness(None, 0)
    assert s.loudness_state() == (0, 0) and s.loudness_for(1000) == 0
    s.set_loudness(g, 7, out)
    assert s.loudness_state() == (0, 0) and s.loudness_for(15) == 2
    _feed(s, raw, fb, 430, 14, "plain")
    assert _same_records(out[:2], lr.records_of(planar[:, 430:444], g, 7)[0])
    s.close(); twin.close()


@pytest.mark.parametrize("name", NAMES)
def test_all_lanes_armed_together(gpu, name):
    """every lane armed against a twin with all but the loudness lane, and against streams with one lane each: what the feeds return and every
    other lane's output are the twin's byte for byte, and each lane's records are those of the lane armed alone"""
    import level_ref as lv
    import truepeak_ref as tr
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb, D, pairs = channels * BYTES[fmt], planar.shape[0], planar.shape[0] // 2
    rng = np.random.default_rng(17)
    f = filt(8000)
    wm, lm, tm, dm = 7, 16, 33, 50
    for mode in ("plain", "mixed"):
        sizes = _feed_sizes(rng, N, W, HOP)

        def run(lanes):
            s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
            wave = np.zeros((N // wm + 1, D, 2), np.float32)
            track = np.zeros((FRAMES, pairs, 6), np.float64)
            level = np.zeros((-(-N // lm), pairs), lv.DTYPE)
            peak = np.zeros((-(-N // tm), D), tr.DTYPE)
            loud = np.zeros(_want(name, 8000, dm).shape, lr.DTYPE)
            if "wave" in lanes:
                s.set_waveform(wm, wave)
            if "track" in lanes:
                s.set_track(0, 0.5, track, FRAMES)
            if "level" in lanes:
                s.set_level(lm, level)
            if "peak" in lanes:
                s.set_truepeak(tm, peak)
            if "loud" in lanes:
                s.set_loudness(f, dm, loud)
            got, _ = _run(s, raw, fb, sizes, mode, dm if "loud" in lanes else 0, loud)
            for lane, flush in (("wave", s.flush_waveform), ("level", s.flush_level), ("peak", s.flush_truepeak)):
                if lane in lanes:
                    flush()
            s.close()
            return got, wave.view(np.uint32), track.view(np.uint64), level.tobytes(), peak.tobytes(), loud.tobytes()

        every = run(("wave", "track", "level", "peak", "loud"))
        twin = run(("wave", "track", "level", "peak"))
        assert _same(every[0], twin[0]) and all(np.array_equal(every[i], twin[i]) for i in (1, 2)) and every[3:5] == twin[3:5], (name, mode)
        assert every[5] == _want(name, 8000, dm).tobytes()
        assert np.array_equal(every[1], wr.columns_of(planar, wm)[0]) and every[3] == lv.records_of(planar, lm)[0].tobytes()
        assert every[4] == tr.records_of(planar, tm)[0].tobytes()
        for i, lane in ((1, "wave"), (2, "track"), (3, "level"), (4, "peak"), (5, "loud")):
            alone = run((lane,))
            assert _same(alone[0], every[0]), (name, mode, lane)
            assert np.array_equal(alone[i], every[i]) if i < 3 else alone[i] == every[i], (name, mode, lane)
