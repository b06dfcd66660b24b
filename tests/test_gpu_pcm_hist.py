"""The histogram lane inside the PCM stream on the GPU (sgz_pcm_stream_set_hist, _hist_for, _hist_state, _flush_hist; csrc/pcm.hip,
csrc/hist_columns.hip).

Byte for byte, no tolerance: the lane's records after the flush == sgz_stage_hist_columns on the whole file's converted floats ==
tests/hist_ref.py of them, for every m, chunk_samples, kind of feed and way of cutting the stream into feeds; everything the feeds return ==
an unarmed twin's; and armed beside the other six column lanes and the track lane, every other output is that of a stream without it.  The
cases and the feeds are those of tests/test_gpu_pcm_level.py."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hist_ref as hr  # noqa: E402
from test_gpu_pcm import BYTES  # noqa: E402
from test_gpu_pcm_level import FRAMES, HOP, K, N, W, _case, _feed, _kinds, _same  # noqa: E402  (cases, feeds, the feeds' comparison)
from test_gpu_pcm_overview import _feed_sizes  # noqa: E402  (random cuts)

pytestmark = pytest.mark.gpu

E = api.SGZ_EINVAL
NAMES = ("s16_3ch", "s24", "f32_two_pairs")
CHUNKS = (0, 1000, 4096)
MS = (128, 1000, 4097, N + 1)
_wants = {}


def _want(name, m):
    if (name, m) not in _wants:
        _wants[name, m] = hr.columns(_case(name)[5], m)[0]
    return _wants[name, m]


def _same_records(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a, hr.DTYPE).tobytes() == np.ascontiguousarray(b, hr.DTYPE).tobytes()


def _sentinel(columns, channels):
    return np.full((columns, channels, 448), 0xA5, np.uint8).view(hr.DTYPE).reshape(columns, channels)


def _run(s, raw, fb, sizes, mode, m=0, out=None):
    """feeds the sizes in turn; armed (m > 0): checks hist_for / hist_state around every feed against sgz_overview_step chained, then flushes
    the lane -> (everything the feeds returned, the lane's records)"""
    returned, at, written, open_ = [], 0, 0, 0
    kinds = _kinds(mode, len(sizes))
    for size, kind in zip(sizes, kinds):
        if m:
            columns, left = api.overview_step(m, open_, size, False)
            assert s.hist_for(size) == columns and s.hist_for(size, True) == api.overview_step(m, open_, size, True)[0]
        returned.append(_feed(s, raw, fb, at, size, kind))
        at += size
        if m:
            written, open_ = written + columns, left
            assert s.hist_state() == (written, open_), (size, kind)
    if kinds[-1] == "overview":
        returned.append(_feed(s, raw, fb, at, 0, "overview", flush=True))
    if not m:
        return returned, None
    s.flush_hist()
    written += open_ > 0
    assert s.hist_state() == (written, 0)
    s.flush_hist()                                                     # nothing open: nothing happens
    assert s.hist_state() == (written, 0)
    return returned, out[:written].copy()


def _staged(planar, m):
    """sgz_stage_hist_columns on the whole file in one call"""
    import torch
    D, n = planar.shape
    cols = -(-n // m)
    dev = torch.from_numpy(np.ascontiguousarray(planar)).cuda()
    out = torch.zeros((cols, D, 112), dtype=torch.int32, device="cuda")
    assert api.stage_hist_columns(dev, n, D, n, m, 0, True, 0, None, out) == api.SGZ_OK
    torch.cuda.synchronize()
    return out.cpu().numpy().view(hr.DTYPE).reshape(cols, D)


@pytest.mark.parametrize("name", NAMES)
def test_the_cases_are_what_they_say(gpu, name):
    """the host half: 16-bit PCM reads 16 effective bits, 24-bit PCM 24, and the stage call on the whole file is the definition"""
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    for m in MS:
        assert _same_records(_staged(planar, m), _want(name, m)), (name, m)
    rec = hr.add(_want(name, 1000)[:, 0])
    bits = api.hist_readout(rec)["effective_bits"]
    assert bits == {"s16_3ch": 16, "s24": 24}.get(name, bits)
    if ints is not None:                                               # the quantiser is the identity on integer PCM: the OR and the AND of the raw words
        word = ints[0] & 0xFFFFFFFF
        assert int(rec["bits_or"]) == int(np.bitwise_or.reduce(word)) and int(rec["bits_and"]) == int(np.bitwise_and.reduce(word))
        assert int(rec["peak"]) == int(np.abs(ints[0]).max()) and int(rec["negative"]) == int((ints[0] < 0).sum())


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", NAMES)
def test_lane_equals_the_definition_and_leaves_the_render_alone(gpu, name, chunk):
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb, D = channels * BYTES[fmt], planar.shape[0]
    rng = np.random.default_rng(len(name) + chunk)
    armed = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
    twin = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
    runs = 0
    for mode in ("plain", "overview", "mixed"):
        sizes = _feed_sizes(rng, N, W, HOP)
        assert 0 in sizes and 1 in sizes and any(0 < v < HOP for v in sizes), sizes
        twin.reset()
        unarmed, _ = _run(twin, raw, fb, sizes, mode)
        for m in MS:
            want = _want(name, m)
            out = _sentinel(want.shape[0] + 2, D)
            armed.reset()
            armed.set_hist(m, out)
            got, hist = _run(armed, raw, fb, sizes, mode, m, out)
            what = (name, chunk, mode, m, sizes)
            assert _same_records(hist, want), what
            assert (hist["bucket"].sum(axis=-1, dtype=np.uint64) == hist["count"]).all(), what
            assert out[want.shape[0]:].tobytes() == _sentinel(2, D).tobytes(), what
            assert _same(got, unarmed), what
            runs += 1
        one = [N]                                                      # the whole file in one feed: the pieces of chunk_samples inside it
        armed.reset()
        out = np.zeros(_want(name, 128).shape, hr.DTYPE)
        armed.set_hist(128, out)
        _, hist = _run(armed, raw, fb, one, mode, 128, out)
        assert _same_records(hist, _want(name, 128)), (name, chunk, mode)
    assert runs == 12
    armed.set_hist(0)
    armed.reset()
    disarmed, _ = _run(armed, raw, fb, sizes, "mixed")
    assert _same(disarmed, unarmed) and armed.hist_state() == (0, 0) and armed.hist_for(N) == 0
    armed.close(); twin.close()


def test_pinned_and_pageable_destinations(gpu):
    import torch
    for name in ("s16_3ch", "f32_two_pairs"):
        cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
        fb, D = channels * BYTES[fmt], planar.shape[0]
        for m in (128, 1000):
            want = _want(name, m)
            s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
            pinned = torch.zeros((want.shape[0], D, 448), dtype=torch.uint8).pin_memory()
            view = pinned.numpy().view(hr.DTYPE).reshape(want.shape)
            s.set_hist(m, pinned)
            _run(s, raw, fb, [N // 3, N - N // 3], "plain", m, view)
            assert _same_records(view, want), (name, m)
            s.reset()
            pageable = np.zeros(want.shape, hr.DTYPE)
            s.set_hist(m, pageable)                                    # the same stream, now through the pinned twins
            _run(s, raw, fb, [N // 3, N - N // 3], "overview", m, pageable)
            assert _same_records(pageable, want), (name, m)
            s.close()


def test_draining_through_a_small_buffer(gpu):
    cfg, fmt, channels, cmap, raw, planar, ints = _case("s24")
    fb, D, m, cap = channels * BYTES[fmt], planar.shape[0], 128, 5
    want = _want("s24", m)
    rng = np.random.default_rng(3)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=200)
    small = [np.zeros((cap, D), hr.DTYPE), np.zeros((cap, D), hr.DTYPE)]
    which, kept, at, rearmed = 0, [], 0, 0
    s.set_hist(m, small[0])
    while at < N:
        size = min(int(rng.integers(0, (cap - 1) * m)), N - at)
        written, open_ = s.hist_state()
        if written + s.hist_for(size) > cap:                           # drain: keep what is there, re-arm with the other buffer -- the open column stays
            kept.append(small[which][:written].copy())
            which ^= 1
            s.set_hist(m, small[which])
            assert s.hist_state() == (0, open_)
            rearmed += 1
        _feed(s, raw, fb, at, size, "plain")
        at += size
    written, open_ = s.hist_state()
    if written == cap:                                                 # (the flush needs a column of its own)
        kept.append(small[which][:written].copy())
        which ^= 1
        s.set_hist(m, small[which])
    s.flush_hist()
    kept.append(small[which][:s.hist_state()[0]].copy())
    assert rearmed >= 5 and _same_records(np.concatenate(kept), want)
    s.close()


def test_counts_state_and_refusals(gpu):
    name = "f32_two_pairs"
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    P, fb, D, pairs = cfg["axis_points"], channels * BYTES[fmt], planar.shape[0], planar.shape[0] // 2
    L = api.lib()
    m = 400
    want = _want(name, m)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    twin = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    assert s.hist_for(N) == 0 and s.hist_state() == (0, 0)             # disarmed
    assert L.sgz_pcm_stream_flush_hist(s.h) == E
    assert L.sgz_last_error().decode() == "sgz_pcm_stream_flush_hist: the lane is off (sgz_pcm_stream_set_hist)"
    assert L.sgz_pcm_stream_set_hist(None, m, None, 0) == E and L.sgz_pcm_stream_set_hist(s.h, m, None, 3) == E
    assert L.sgz_pcm_stream_hist_state(None, None, None) == E
    for few in (1, 64, 127):                                           # 0 < m < 128 is refused and arms nothing
        assert L.sgz_pcm_stream_set_hist(s.h, few, None, 0) == E and s.hist_for(N) == 0
        assert L.sgz_last_error().decode().startswith("sgz_pcm_stream_set_hist: m >= 128 samples per column")
    assert L.sgz_pcm_stream_set_hist(s.h, 128, None, 0) == api.SGZ_OK and s.hist_for(N) == N // 128
    s.set_hist(0)
    odd = np.zeros(3 * D * 448 + 8, np.uint8)
    assert L.sgz_pcm_stream_set_hist(s.h, m, odd.ctypes.data + 1 + (-odd.ctypes.data) % 4, 3) == E         # not aligned to 4 bytes
    first = 1400                                                       # three columns and 200 samples open; W + hop <= 1400: two frames
    small = np.zeros((2, D), hr.DTYPE)
    s.set_hist(m, small)
    assert s.hist_for(first) == 3 and s.hist_for(first, True) == 4 and s.frames_for(first) == 2
    big_rgba = np.zeros((FRAMES, P, 4), np.uint8)
    peaks = np.zeros((FRAMES, pairs, P), np.float32)
    # a capacity below what the feed closes: refused by both kinds, nothing consumed, and the message names the lane
    assert s.feed_into(raw, first, big_rgba, None, FRAMES)[0] == E
    assert L.sgz_last_error().decode() == ("sgz_pcm_stream: the feed closes more histogram columns than the buffer has left (sgz_pcm_stream_hist_for; "
                                           "re-arm with sgz_pcm_stream_set_hist)")
    assert s.feed_overview_into(raw, first, K, False, big_rgba, peaks, FRAMES)[0] == E
    assert small.tobytes() == bytes(small.nbytes) and not big_rgba.any() and not peaks.any()
    assert s.hist_state() == (0, 0) and s.frames_for(first) == 2 and s.open_frames() == 0
    # ... the next feed's outputs are those of a stream that never saw the refusals
    out = np.zeros(want.shape, hr.DTYPE)
    s.set_hist(m, out)
    a = _feed(s, raw, fb, 0, first, "plain")
    b = _feed(twin, raw, fb, 0, first, "plain")
    assert _same([a], [b]) and a[1].shape[0] == 2 and s.hist_state() == (3, 200)
    assert _same_records(out[:3], want[:3])
    # another m while samples are open: refused, the lane as it was
    assert L.sgz_pcm_stream_set_hist(s.h, m + 1, out.ctypes.data, out.shape[0]) == E
    assert s.hist_state() == (3, 200) and s.hist_for(200) == 1
    # the flush needs a column of its own
    s.set_hist(m, small)
    _feed(s, raw, fb, first, 600, "plain")
    assert s.hist_state() == (2, 0)
    _feed(s, raw, fb, first + 600, 30, "plain")
    assert s.hist_state() == (2, 30) and L.sgz_pcm_stream_flush_hist(s.h) == E and s.hist_state() == (2, 30)
    assert _same_records(small, want[3:5])
    # reset drops the open column and restarts the cursor; the same file again gives the same records
    s.reset()
    assert s.hist_state() == (0, 0)
    s.set_hist(m, out)
    out[:] = np.zeros((), hr.DTYPE)
    _, hist = _run(s, raw, fb, [N], "plain", m, out)
    assert _same_records(hist, want)
    # disarming drops the open column too: another m is taken afterwards
    s.reset()
    _feed(s, raw, fb, 0, 430, "plain")
    assert s.hist_state() == (1, 30)
    s.set_hist(0)
    assert s.hist_state() == (0, 0) and s.hist_for(1000) == 0
    s.set_hist(150, out)
    assert s.hist_state() == (0, 0) and s.hist_for(300) == 2
    s.close(); twin.close()


@pytest.mark.parametrize("name", ("s16_3ch", "f32_two_pairs"))
def test_beside_the_other_six_lanes_and_the_track(gpu, name):
    """the histogram lane armed beside the six other column lanes and the track lane: what the feeds return and every other lane's output is
    byte for byte that of a stream without it; its own records are the definition's"""
    import band_ref as br
    import field_ref as fr
    import level_ref as lv
    import loudness_ref as ld
    import truepeak_ref as tr
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb, D, pairs = channels * BYTES[fmt], planar.shape[0], planar.shape[0] // 2
    rng = np.random.default_rng(23)
    f, kf = api.band_filter_for_rate(8000), api.loudness_filter_for_rate(8000)
    wm, lm, tm, dm, fm, bm, hm = 7, 16, 33, 50, 64, 100, 130
    for mode in ("plain", "mixed"):
        sizes = _feed_sizes(rng, N, W, HOP)

        def run(with_hist):
            s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
            wave = np.zeros((N // wm + 1, D, 2), np.float32)
            track = np.zeros((FRAMES, pairs, 6), np.float64)
            level = np.zeros((-(-N // lm), pairs), lv.DTYPE)
            peak = np.zeros((-(-N // tm), D), tr.DTYPE)
            loud = np.zeros((-(-N // dm), D), ld.DTYPE)
            field = np.zeros((-(-N // fm), pairs), fr.DTYPE)
            band = np.zeros((-(-N // bm), D), br.DTYPE)
            hist = np.zeros(_want(name, hm).shape, hr.DTYPE)
            s.set_waveform(wm, wave)
            s.set_track(0, 0.5, track, FRAMES)
            s.set_level(lm, level)
            s.set_truepeak(tm, peak)
            s.set_loudness(kf, dm, loud)
            s.set_field(fm, field)
            s.set_band(f, bm, band)
            if with_hist:
                s.set_hist(hm, hist)
            got, records = _run(s, raw, fb, sizes, mode, hm if with_hist else 0, hist)
            for flush in (s.flush_waveform, s.flush_level, s.flush_truepeak, s.flush_loudness, s.flush_field, s.flush_band):
                flush()
            s.close()
            return got, [v.tobytes() for v in (wave, track, level, peak, loud, field, band)], records

        with_, without = run(True), run(False)
        assert _same(with_[0], without[0]), (name, mode)
        assert with_[1] == without[1], (name, mode, [a == b for a, b in zip(with_[1], without[1])])
        assert with_[1][2] == lv.records_of(planar, lm)[0].tobytes() and with_[1][5] == fr.columns(planar, fm)[0].tobytes()
        assert _same_records(with_[2], _want(name, hm)), (name, mode)
