"""The band lane inside the PCM stream on the GPU (sgz_pcm_stream_set_band, _band_for, _band_state, _flush_band; csrc/pcm.hip,
csrc/band_columns.hip).

Byte for byte, no tolerance: the lane's records after the flush == tests/band_ref.py of the numpy-converted planar floats of the whole file,
for S16, S24 and F32 with a channel subset, every way of cutting the stream into feeds (1 sample, a prime, the whole file, random) and into
pieces (the default, 2^12 samples, a prime), and both kinds of feed; and everything the feeds return == an unarmed twin's.  The cases and
the feeds are those of tests/test_gpu_pcm_level.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import band_ref as br  # noqa: E402
import wave_ref as wr  # noqa: E402
from test_gpu_pcm import BYTES  # noqa: E402
from test_gpu_pcm_level import FRAMES, HOP, K, N, W, _case, _feed, _kinds, _same  # noqa: E402  (cases, feeds, the feeds' comparison)
from test_gpu_pcm_overview import _feed_sizes  # noqa: E402  (random cuts)

pytestmark = pytest.mark.gpu

E = api.SGZ_EINVAL
NAMES = ("s16_3ch", "s24", "f32_two_pairs")                          # 16-bit, 24-bit, and float PCM with a channel subset of five
_wants, _filters = {}, {}


def filt(which):
    if which not in _filters:
        _filters[which] = api.band_filter(br.TINY.c, br.TINY.W, br.TINY.L) if which == "tiny" else api.band_filter_for_rate(which)
    return _filters[which]


def _want(name, which, m):
    if (name, which, m) not in _wants:
        _wants[name, which, m] = br.records_of(_case(name)[5], filt(which), m)[0]
    return _wants[name, which, m]


def _same_records(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a, br.DTYPE).tobytes() == np.ascontiguousarray(b, br.DTYPE).tobytes()


def _sentinel(columns, channels):
    return np.full((columns, channels, 64), 0xA5, np.uint8).view(br.DTYPE).reshape(columns, channels)


def _cut_sets(rng):
    """feed sizes: one sample and the rest, a prime, the whole file, a random set with empty and tiny feeds"""
    prime = [997] * (N // 997) + [N % 997]
    return [[1, N - 1], prime, [N], _feed_sizes(rng, N, W, HOP)]


def _run(s, raw, fb, sizes, mode, m=0, out=None, at=0, flush=True):
    """feeds the sizes in turn; armed (m > 0): checks band_for / band_state around every feed against sgz_overview_step chained, then flushes
    the lane -> (everything the feeds returned, the lane's records)"""
    returned = []
    written, open_ = s.band_state() if m else (0, 0)
    kinds = _kinds(mode, len(sizes))
    for size, kind in zip(sizes, kinds):
        if m:
            columns, left = api.overview_step(m, open_, size, False)
            assert s.band_for(size) == columns and s.band_for(size, True) == api.overview_step(m, open_, size, True)[0]
        returned.append(_feed(s, raw, fb, at, size, kind))
        at += size
        if m:
            written, open_ = written + columns, left
            assert s.band_state() == (written, open_), (size, kind)
    if kinds[-1] == "overview":
        returned.append(_feed(s, raw, fb, at, 0, "overview", flush=True))
    if not m:
        return returned, None
    if flush:
        s.flush_band()
        written += open_ > 0
        assert s.band_state() == (written, 0)
        s.flush_band()                                                  # nothing open: nothing happens
        assert s.band_state() == (written, 0)
    return returned, out[:written].copy()


@pytest.mark.parametrize("chunk", [0, 4096, 997])
@pytest.mark.parametrize("name", NAMES)
def test_lane_equals_the_definition_and_leaves_the_render_alone(gpu, name, chunk):
    """chunk 0: the whole file is one piece; 4096: pieces of 2^12 samples, with the overview's slab set through sgz_pcm_stream_set_option;
    997: a prime"""
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb, D = channels * BYTES[fmt], planar.shape[0]
    rng = np.random.default_rng(len(name) + chunk)
    armed = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
    twin = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
    if chunk == 4096:
        armed.set_option(api.OPT_OVERVIEW_SLAB, 2)
        twin.set_option(api.OPT_OVERVIEW_SLAB, 2)
    cases = (("tiny", 64), (8000, 100), ("tiny", 1000), (8000, 4097))
    for i, sizes in enumerate(_cut_sets(rng)):
        mode = ("plain", "overview", "mixed")[(i + chunk) % 3]
        twin.reset()
        unarmed, _ = _run(twin, raw, fb, sizes, mode)
        for which, m in (cases[i % 4], cases[(i + 1) % 4]):
            f = filt(which)
            want = _want(name, which, m)
            out = _sentinel(want.shape[0] + 2, D)
            armed.set_band(None, 0)
            armed.reset()
            armed.set_band(f, m, out)
            got, records = _run(armed, raw, fb, sizes, mode, m, out)
            what = (name, which, chunk, mode, m, sizes)
            assert _same_records(records, want), what
            assert out[want.shape[0]:].tobytes() == _sentinel(2, D).tobytes(), what
            assert _same(got, unarmed), what
    armed.set_band(None, 0)
    armed.reset()
    disarmed, _ = _run(armed, raw, fb, sizes, mode)
    assert _same(disarmed, unarmed) and armed.band_state() == (0, 0) and armed.band_for(N) == 0
    armed.close(); twin.close()


def test_lane_equals_the_stage_call_on_the_whole_buffer(gpu):
    import torch
    name = "f32_two_pairs"
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb, D = channels * BYTES[fmt], planar.shape[0]
    f, m = filt(8000), 480
    want = _want(name, 8000, m)
    dev = torch.from_numpy(planar).cuda()
    carry = torch.zeros(br.carry_bytes(f) * D // 4, dtype=torch.int32, device="cuda")
    staged = torch.zeros((want.shape[0], D, 16), dtype=torch.int32, device="cuda")
    assert api.stage_band_columns(dev, N, D, N, f, 0, m, carry=carry, records=staged) == api.SGZ_OK
    torch.cuda.synchronize()
    staged = staged.cpu().numpy().view(br.DTYPE).reshape(want.shape)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    out = np.zeros(want.shape, br.DTYPE)
    s.set_band(f, m, out)
    _, records = _run(s, raw, fb, [N // 3, N - N // 3], "plain", m, out)
    assert _same_records(records, staged) and _same_records(records, want)
    s.close()


def test_pinned_and_pageable_destinations(gpu):
    import torch
    name = "s16_3ch"
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb, D, f = channels * BYTES[fmt], planar.shape[0], filt(8000)
    for m in (64, 1000):
        want = _want(name, 8000, m)
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
        pinned = torch.zeros((want.shape[0], D, 64), dtype=torch.uint8).pin_memory()
        view = pinned.numpy().view(br.DTYPE).reshape(want.shape)
        s.set_band(f, m, pinned)
        _run(s, raw, fb, [N // 3, N - N // 3], "plain", m, view)
        assert _same_records(view, want), m
        s.reset()
        pageable = np.zeros(want.shape, br.DTYPE)
        s.set_band(f, m, pageable)                                     # the same stream, now through the pinned twins
        _run(s, raw, fb, [N // 3, N - N // 3], "overview", m, pageable)
        assert _same_records(pageable, want), m
        s.close()


def test_draining_through_a_small_buffer_keeps_the_history(gpu):
    """re-arming with another buffer while samples are open keeps the open column, the history and the index"""
    cfg, fmt, channels, cmap, raw, planar, ints = _case("s24")
    fb, D, m, cap = channels * BYTES[fmt], planar.shape[0], 70, 7
    f = filt("tiny")
    want = _want("s24", "tiny", m)
    rng = np.random.default_rng(3)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=256)
    small = [np.zeros((cap, D), br.DTYPE), np.zeros((cap, D), br.DTYPE)]
    which, kept, at, rearmed = 0, [], 0, 0
    s.set_band(f, m, small[0])
    while at < N:
        size = min(int(rng.integers(0, (cap - 1) * m)), N - at)
        written, open_ = s.band_state()
        if written + s.band_for(size) > cap:                           # drain: re-arm with the other buffer -- the open column and the history stay
            kept.append(small[which][:written].copy())
            which ^= 1
            s.set_band(f, m, small[which])
            assert s.band_state() == (0, open_)
            rearmed += 1
        _feed(s, raw, fb, at, size, "plain")
        at += size
    written, open_ = s.band_state()
    if written == cap:                                                 # (the flush needs a column of its own)
        kept.append(small[which][:written].copy())
        which ^= 1
        s.set_band(f, m, small[which])
    s.flush_band()
    kept.append(small[which][:s.band_state()[0]].copy())
    assert rearmed >= 5 and _same_records(np.concatenate(kept), want)  # (a zeroed history or index at any re-arm would change the columns behind it)
    s.close()


def test_a_flush_in_mid_stream_keeps_the_history_and_the_grid(gpu):
    for name, which in (("s16_3ch", 8000), ("f32_two_pairs", "tiny")):
        cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
        f = filt(which)
        fb, D, m, cut = channels * BYTES[fmt], planar.shape[0], 64, 1003            # 1003 = 62 * 16 + 11: inside a segment of either filter
        v, has = br.quantise(planar)
        head = br.records_of(planar[:, :cut], f, m)[0]                              # the partial column closes as it stands
        tail = br.records_of_integers(v[:, cut:], has[:, cut:], f, m, True, v[:, :cut], cut)[0]      # columns count from the flush on; the grid does not
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=500)
        out = np.zeros((head.shape[0] + tail.shape[0], D), br.DTYPE)
        s.set_band(f, m, out)
        _run(s, raw, fb, [cut], "plain", m, out)
        assert s.band_state() == (head.shape[0], 0)
        _run(s, raw, fb, [700, N - cut - 700], "plain", m, out, at=cut)
        assert _same_records(out, np.concatenate([head, tail])), name
        fresh = br.records_of(planar[:, cut:], f, m)[0]
        assert not _same_records(tail[:1], fresh[:1])                               # (the history matters to the first column behind the flush)
        s.close()


def test_counts_state_reset_and_refusals(gpu):
    name = "f32_two_pairs"
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    P, fb, D, pairs = cfg["axis_points"], channels * BYTES[fmt], planar.shape[0], planar.shape[0] // 2
    L = api.lib()
    f, g = filt(8000), filt("tiny")
    m = 400
    want = _want(name, 8000, m)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    twin = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    assert s.band_for(N) == 0 and s.band_state() == (0, 0)             # disarmed
    assert L.sgz_pcm_stream_flush_band(s.h) == E
    assert L.sgz_pcm_stream_set_band(None, C.byref(f), m, None, 0) == E and L.sgz_pcm_stream_set_band(s.h, C.byref(f), m, None, 3) == E
    assert L.sgz_pcm_stream_set_band(s.h, None, m, None, 0) == E                                               # armed without a filter
    for few in (1, 7, 63):                                                                                     # fewer samples than a record's bytes
        assert L.sgz_pcm_stream_set_band(s.h, C.byref(f), few, None, 0) == E and s.band_for(N) == 0
    assert L.sgz_pcm_stream_set_band(s.h, C.byref(f), 64, None, 0) == api.SGZ_OK and s.band_for(N) == N // 64
    s.set_band(None, 0)
    bad = api.band_filter([[0.0, 2.5, 0.0, 0.0, 0.0]] + [list(r) for r in br.TINY.c[1:]], 64, 16)
    assert L.sgz_pcm_stream_set_band(s.h, C.byref(bad), m, None, 0) == E and s.band_for(N) == 0               # a refused table arms nothing
    assert L.sgz_pcm_stream_set_band(s.h, C.byref(api.band_filter(br.TINY.c, 64, 24)), m, None, 0) == E
    assert L.sgz_pcm_stream_set_band(s.h, C.byref(api.band_filter(br.TINY.c, 32768, 64)), m, None, 0) == E    # W above what the device takes
    assert L.sgz_pcm_stream_band_state(None, None, None) == E
    odd = np.zeros(3 * D * 64 + 8, np.uint8)
    assert L.sgz_pcm_stream_set_band(s.h, C.byref(f), m, odd.ctypes.data + 1 + (-odd.ctypes.data) % 8, 3) == E          # not aligned to 8 bytes
    first = 1400                                                       # three columns and 200 samples open; W + hop <= 1400: two frames
    small = np.zeros((2, D), br.DTYPE)
    s.set_band(f, m, small)
    assert s.band_for(first) == 3 and s.band_for(first, True) == 4 and s.frames_for(first) == 2
    big_rgba = np.zeros((FRAMES, P, 4), np.uint8)
    peaks = np.zeros((FRAMES, pairs, P), np.float32)
    # a capacity below what the feed closes: refused by both kinds, nothing consumed
    assert s.feed_into(raw, first, big_rgba, None, FRAMES)[0] == E and "band" in L.sgz_last_error().decode()
    assert s.feed_overview_into(raw, first, K, False, big_rgba, peaks, FRAMES)[0] == E
    assert small.tobytes() == bytes(small.nbytes) and not big_rgba.any() and not peaks.any()
    assert s.band_state() == (0, 0) and s.frames_for(first) == 2 and s.open_frames() == 0
    # ... the next feed's outputs are those of a stream that never saw the refusals
    out = np.zeros(want.shape, br.DTYPE)
    s.set_band(f, m, out)
    a = _feed(s, raw, fb, 0, first, "plain")
    b = _feed(twin, raw, fb, 0, first, "plain")
    assert _same([a], [b]) and a[1].shape[0] == 2 and s.band_state() == (3, 200)
    assert _same_records(out[:3], want[:3])
    # another m or another filter while samples are open: refused, the lane as it was
    assert L.sgz_pcm_stream_set_band(s.h, C.byref(f), m + 1, out.ctypes.data, out.shape[0]) == E
    assert L.sgz_pcm_stream_set_band(s.h, C.byref(g), m, out.ctypes.data, out.shape[0]) == E
    assert s.band_state() == (3, 200) and s.band_for(200) == 1
    # the flush needs a column of its own
    s.set_band(f, m, small)
    _feed(s, raw, fb, first, 600, "plain")
    assert s.band_state() == (2, 0)
    _feed(s, raw, fb, first + 600, 30, "plain")
    assert s.band_state() == (2, 30) and L.sgz_pcm_stream_flush_band(s.h) == E and s.band_state() == (2, 30)
    assert _same_records(small, want[3:5])
    # reset drops the open column, zeroes the history and the index and restarts the cursor: the same file again gives a fresh stream's records
    s.reset()
    assert s.band_state() == (0, 0)
    s.set_band(f, m, out)
    out[:] = np.zeros((), br.DTYPE)
    _, records = _run(s, raw, fb, [N], "plain", m, out)
    assert _same_records(records, want)
    # ... and so does a reset in mid-stream, at an index that is no multiple of L
    r = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    short = np.zeros((10, D), br.DTYPE)
    r.set_band(g, 64, short)
    _feed(r, raw, fb, 3000, 30, "plain")
    r.reset()
    assert r.band_state() == (0, 0)
    _feed(r, raw, fb, 0, 128, "plain")
    assert r.band_state() == (2, 0) and _same_records(short[:2], _want(name, "tiny", 64)[:2])
    assert not _same_records(_want(name, "tiny", 64)[:1], br.records_of(planar[:, :64], g, 64, True, br.quantise(planar[:, 3000:3030])[0], 30)[0])
    r.close()
    # disarming drops the open column, the history and the index too: another m and another filter are taken afterwards, from rest
    s.reset()
    _feed(s, raw, fb, 0, 430, "plain")
    assert s.band_state() == (1, 30)
    s.set_band(None, 0)
    assert s.band_state() == (0, 0) and s.band_for(1000) == 0
    s.set_band(g, 70, out)
    assert s.band_state() == (0, 0) and s.band_for(150) == 2
    _feed(s, raw, fb, 430, 140, "plain")
    assert _same_records(out[:2], br.records_of(planar[:, 430:570], g, 70)[0])
    s.close(); twin.close()


@pytest.mark.parametrize("name", ("s16_3ch", "f32_two_pairs"))
def test_all_lanes_armed_together(gpu, name):
    """the six column lanes and the track lane armed together: what the feeds return is an unarmed stream's, and each lane's output is that
    of the lane armed alone"""
    import field_ref as fr
    import level_ref as lv
    import loudness_ref as ld
    import truepeak_ref as tr
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb, D, pairs = channels * BYTES[fmt], planar.shape[0], planar.shape[0] // 2
    rng = np.random.default_rng(17)
    f, kf = filt(8000), api.loudness_filter_for_rate(8000)
    wm, lm, tm, dm, fm, bm = 7, 16, 33, 50, 64, 100
    order = ("wave", "track", "level", "peak", "loud", "field", "band")
    for mode in ("plain", "mixed"):
        sizes = _feed_sizes(rng, N, W, HOP)

        def run(lanes):
            s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
            wave = np.zeros((N // wm + 1, D, 2), np.float32)
            track = np.zeros((FRAMES, pairs, 6), np.float64)
            level = np.zeros((-(-N // lm), pairs), lv.DTYPE)
            peak = np.zeros((-(-N // tm), D), tr.DTYPE)
            loud = np.zeros((-(-N // dm), D), ld.DTYPE)
            field = np.zeros((-(-N // fm), pairs), fr.DTYPE)
            band = np.zeros(_want(name, 8000, bm).shape, br.DTYPE)
            if "wave" in lanes:
                s.set_waveform(wm, wave)
            if "track" in lanes:
                s.set_track(0, 0.5, track, FRAMES)
            if "level" in lanes:
                s.set_level(lm, level)
            if "peak" in lanes:
                s.set_truepeak(tm, peak)
            if "loud" in lanes:
                s.set_loudness(kf, dm, loud)
            if "field" in lanes:
                s.set_field(fm, field)
            if "band" in lanes:
                s.set_band(f, bm, band)
            got, _ = _run(s, raw, fb, sizes, mode, bm if "band" in lanes else 0, band)
            for lane, flush in (("wave", s.flush_waveform), ("level", s.flush_level), ("peak", s.flush_truepeak), ("loud", s.flush_loudness),
                                ("field", s.flush_field)):
                if lane in lanes:
                    flush()
            s.close()
            return got, wave.tobytes(), track.tobytes(), level.tobytes(), peak.tobytes(), loud.tobytes(), field.tobytes(), band.tobytes()

        every = run(order)
        unarmed = run(())
        assert _same(every[0], unarmed[0]), (name, mode)
        assert every[7] == _want(name, 8000, bm).tobytes()
        assert every[1] == wr.columns_of(planar, wm)[0].tobytes() and every[3] == lv.records_of(planar, lm)[0].tobytes()
        assert every[4] == tr.records_of(planar, tm)[0].tobytes() and every[5] == ld.records_of(planar, kf, dm)[0].tobytes()
        assert every[6] == fr.columns(planar, fm)[0].tobytes()
        for i, lane in enumerate(order, start=1):
            alone = run((lane,))
            assert _same(alone[0], every[0]), (name, mode, lane)
            assert alone[i] == every[i], (name, mode, lane)
