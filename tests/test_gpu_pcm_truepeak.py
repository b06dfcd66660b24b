"""The true-peak lane inside the PCM stream on the GPU (sgz_pcm_stream_set_truepeak, _truepeak_for, _truepeak_state, _flush_truepeak;
csrc/pcm.hip, csrc/truepeak_columns.hip).

Byte for byte, no tolerance: the lane's records after the flush == tests/truepeak_ref.py of the numpy-converted planar floats, for every m,
chunk_samples, kind of feed and way of cutting the stream into feeds; for the integer formats also == the filter on the raw PCM's integers
(at a scale of 2^23 the quantiser is the identity on S16 and S24); and everything the feeds return == an unarmed twin's.  The cases, the cuts
and the feeds are those of tests/test_gpu_pcm_level.py."""
import gc
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import truepeak_ref as tr  # noqa: E402
import wave_ref as wr  # noqa: E402
from test_gpu_pcm import BYTES  # noqa: E402
from test_gpu_pcm_level import CHUNKS, FRAMES, HOP, K, N, NAMES, W, _case, _feed, _kinds, _same  # noqa: E402  (cases, feeds, the feeds' comparison)
from test_gpu_pcm_overview import _feed_sizes  # noqa: E402  (the cuts)

pytestmark = pytest.mark.gpu

E = api.SGZ_EINVAL
_wants = {}


def _want(name, m):
    if (name, m) not in _wants:
        _wants[name, m] = tr.records_of(_case(name)[5], m)[0]
    return _wants[name, m]


def _ms():
    return (1, 5, 16, 1000, 4097, N + 1)


def _same_records(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a, tr.DTYPE).tobytes() == np.ascontiguousarray(b, tr.DTYPE).tobytes()


def _run(s, raw, fb, sizes, mode, m=0, out=None, at=0, flush=True):
    """feeds the sizes in turn; armed (m > 0): checks truepeak_for / truepeak_state around every feed against sgz_overview_step chained, then
    flushes the lane -> (everything the feeds returned, the lane's records)"""
    returned = []
    written, open_ = s.truepeak_state() if m else (0, 0)
    kinds = _kinds(mode, len(sizes))
    for size, kind in zip(sizes, kinds):
        if m:
            columns, left = api.overview_step(m, open_, size, False)
            assert s.truepeak_for(size) == columns and s.truepeak_for(size, True) == api.overview_step(m, open_, size, True)[0]
        returned.append(_feed(s, raw, fb, at, size, kind))
        at += size
        if m:
            written, open_ = written + columns, left
            assert s.truepeak_state() == (written, open_), (size, kind)
    if kinds[-1] == "overview":
        returned.append(_feed(s, raw, fb, at, 0, "overview", flush=True))
    if not m:
        return returned, None
    if flush:
        s.flush_truepeak()
        written += open_ > 0
        assert s.truepeak_state() == (written, 0)
        s.flush_truepeak()                                              # nothing open: nothing happens
        assert s.truepeak_state() == (written, 0)
    return returned, out[:written].copy()


def _sentinel(columns, channels):
    return np.full((columns, channels, 16), 0xA5, np.uint8).view(tr.DTYPE).reshape(columns, channels)


@pytest.mark.parametrize("name", NAMES)
def test_integer_pcm_is_its_own_quantisation(gpu, name):
    """the host half of the exactness claim: truepeak_ref of the converted floats == the filter on the raw PCM's integers"""
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    v, has = tr.quantise(planar)
    if ints is None:
        assert not has.all() and (np.abs(v) > tr.FULL).any()
        return
    assert has.all() and np.array_equal(v, ints)
    for m in _ms():
        assert _same_records(tr.records_of_integers(ints, np.ones(ints.shape, bool), m)[0], _want(name, m)), (name, m)


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
        for m in _ms():
            want = _want(name, m)
            if ints is not None:                                       # the records against integer arithmetic on the raw PCM
                want_int = tr.records_of_integers(ints, np.ones(ints.shape, bool), m)[0]
            out = _sentinel(want.shape[0] + 2, D)
            armed.reset()
            armed.set_truepeak(m, out)
            got, records = _run(armed, raw, fb, sizes, mode, m, out)
            what = (name, chunk, mode, m, sizes)
            assert _same_records(records, want), what
            assert ints is None or _same_records(records, want_int), what
            assert out[want.shape[0]:].tobytes() == _sentinel(2, D).tobytes(), what
            assert _same(got, unarmed), what
            runs += 1
        armed.reset()                                                  # the whole file in one feed: the pieces of chunk_samples inside it
        out = np.zeros(_want(name, 16).shape, tr.DTYPE)
        armed.set_truepeak(16, out)
        _, records = _run(armed, raw, fb, [N], mode, 16, out)
        assert _same_records(records, _want(name, 16)), (name, chunk, mode)
    assert runs == 18
    armed.set_truepeak(0)
    armed.reset()
    disarmed, _ = _run(armed, raw, fb, sizes, "mixed")
    assert _same(disarmed, unarmed) and armed.truepeak_state() == (0, 0) and armed.truepeak_for(N) == 0
    armed.close(); twin.close()


@pytest.mark.parametrize("name", NAMES)
def test_beside_the_waveform_level_and_track_lanes(gpu, name):
    """all four lanes armed against a twin with the other three alone: what the feeds return and the other lanes' outputs are the twin's byte
    for byte; the true-peak lane's m is its own"""
    import level_ref as lr
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb, D, pairs = channels * BYTES[fmt], planar.shape[0], planar.shape[0] // 2
    rng = np.random.default_rng(17)
    wm, lm, tm = 7, 16, 33
    for mode in ("plain", "mixed"):
        sizes = _feed_sizes(rng, N, W, HOP)
        results = []
        for with_lane in (False, True):
            s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
            wave = np.zeros((N // wm + 1, D, 2), np.float32)
            track = np.zeros((FRAMES, pairs, 6), np.float64)
            level = np.zeros((-(-N // lm), pairs), lr.DTYPE)
            s.set_waveform(wm, wave)
            s.set_track(0, 0.5, track, FRAMES)
            s.set_level(lm, level)
            out = np.zeros(_want(name, tm).shape, tr.DTYPE)
            if with_lane:
                s.set_truepeak(tm, out)
            got, records = _run(s, raw, fb, sizes, mode, tm if with_lane else 0, out)
            s.flush_waveform(); s.flush_level()
            assert s.waveform_state() == (N // wm + 1, 0) and s.track_state() == FRAMES and s.level_state() == (-(-N // lm), 0)
            results.append((got, wave.view(np.uint32).copy(), track.view(np.uint64).copy(), level.tobytes()))
            if with_lane:
                assert _same_records(records, _want(name, tm)), (name, mode)
            s.close()
        a, b = results
        assert _same(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3], (name, mode)
        assert np.array_equal(a[1], wr.columns_of(planar, wm)[0]) and a[3] == lr.records_of(planar, lm)[0].tobytes()


def test_a_piece_without_a_frame_still_delivers_its_records(gpu):
    cfg, fmt, channels, cmap, raw, planar, ints = _case("f32_two_pairs")
    fb, D, m = channels * BYTES[fmt], planar.shape[0], 5
    want = _want("f32_two_pairs", m)
    for chunk in (0, 16):                                              # one piece per feed; several frameless pieces inside a feed
        for kind in ("plain", "overview"):
            s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
            out = np.zeros(want.shape, tr.DTYPE)
            s.set_truepeak(m, out)
            at = 0
            for size in (199, 200, 201, 202, 203):                     # 1005 samples: never a window
                assert s.frames_for(size) == 0
                got = _feed(s, raw, fb, at, size, kind)
                at += size
                assert got[1].shape[0] == 0
                assert s.truepeak_state() == (at // m, at % m)
                assert _same_records(out[:at // m], want[:at // m]), (chunk, kind, at)       # delivered when the feed returns
                assert out[at // m:].tobytes() == bytes(16 * D * (want.shape[0] - at // m))
            s.close()


def test_pinned_and_pageable_destinations(gpu):
    import torch
    for name in ("s16_3ch", "f32_two_pairs"):
        cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
        fb, D = channels * BYTES[fmt], planar.shape[0]
        for m in (5, 1000):
            want = _want(name, m)
            s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
            pinned = torch.zeros((want.shape[0], D, 16), dtype=torch.uint8).pin_memory()
            view = pinned.numpy().view(tr.DTYPE).reshape(want.shape)
            s.set_truepeak(m, pinned)
            _run(s, raw, fb, [N // 3, N - N // 3], "plain", m, view)
            assert _same_records(view, want), (name, m)
            s.reset()
            pageable = np.zeros(want.shape, tr.DTYPE)
            s.set_truepeak(m, pageable)                                # the same stream, now through the pinned twins
            _run(s, raw, fb, [N // 3, N - N // 3], "overview", m, pageable)
            assert _same_records(pageable, want), (name, m)
            s.close()


def test_draining_through_a_small_buffer_keeps_the_history(gpu):
    cfg, fmt, channels, cmap, raw, planar, ints = _case("s24")
    fb, D, m, cap = channels * BYTES[fmt], planar.shape[0], 16, 7
    want = _want("s24", m)
    rng = np.random.default_rng(3)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=64)
    small = [np.zeros((cap, D), tr.DTYPE), np.zeros((cap, D), tr.DTYPE)]
    which, kept, at, rearmed = 0, [], 0, 0
    s.set_truepeak(m, small[0])
    while at < N:
        size = min(int(rng.integers(0, (cap - 1) * m)), N - at)
        written, open_ = s.truepeak_state()
        if written + s.truepeak_for(size) > cap:                       # drain: re-arm with the other buffer -- the open column and the history stay
            kept.append(small[which][:written].copy())
            which ^= 1
            s.set_truepeak(m, small[which])
            assert s.truepeak_state() == (0, open_)
            rearmed += 1
        _feed(s, raw, fb, at, size, "plain")
        at += size
    written, open_ = s.truepeak_state()
    if written == cap:                                                 # (the flush needs a column of its own)
        kept.append(small[which][:written].copy())
        which ^= 1
        s.set_truepeak(m, small[which])
    s.flush_truepeak()
    kept.append(small[which][:s.truepeak_state()[0]].copy())
    assert rearmed >= 5 and _same_records(np.concatenate(kept), want)  # (a zeroed history at any re-arm would change the column behind it)
    s.close()


def test_a_flush_in_mid_stream_keeps_the_history_and_starts_a_new_column(gpu):
    for name in ("s16_3ch", "f32_two_pairs"):
        cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
        fb, D, m, cut = channels * BYTES[fmt], planar.shape[0], 16, 1003            # 1003 = 62 * 16 + 11
        v, has = tr.quantise(planar)
        head = tr.records_of(planar[:, :cut], m)[0]                                 # the partial column closes as it stands
        tail = tr.records_of_integers(v[:, cut:], has[:, cut:], m, True, v[:, cut - 11:cut])[0]    # columns count from the flush on, behind the history
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=500)
        out = np.zeros((head.shape[0] + tail.shape[0], D), tr.DTYPE)
        s.set_truepeak(m, out)
        _run(s, raw, fb, [cut], "plain", m, out)
        assert s.truepeak_state() == (head.shape[0], 0)
        _run(s, raw, fb, [700, N - cut - 700], "plain", m, out, at=cut)
        assert _same_records(out, np.concatenate([head, tail])), name
        fresh = tr.records_of(planar[:, cut:], m)[0]
        assert not _same_records(tail[:1], fresh[:1])                               # (the history matters to the first column behind the flush)
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
    assert s.truepeak_for(N) == 0 and s.truepeak_state() == (0, 0)     # disarmed
    assert L.sgz_pcm_stream_flush_truepeak(s.h) == E
    assert L.sgz_pcm_stream_set_truepeak(None, m, None, 0) == E and L.sgz_pcm_stream_set_truepeak(s.h, m, None, 3) == E
    assert L.sgz_pcm_stream_truepeak_state(None, None, None) == E
    odd = np.zeros(3 * D * 16 + 8, np.uint8)
    assert L.sgz_pcm_stream_set_truepeak(s.h, m, odd.ctypes.data + 1 + (-odd.ctypes.data) % 8, 3) == E       # not aligned to 8 bytes
    first = 1400                                                       # three columns and 200 samples open; W + hop <= 1400: two frames
    small = np.zeros((2, D), tr.DTYPE)
    s.set_truepeak(m, small)
    assert s.truepeak_for(first) == 3 and s.truepeak_for(first, True) == 4 and s.frames_for(first) == 2
    big_rgba = np.zeros((FRAMES, P, 4), np.uint8)
    peaks = np.zeros((FRAMES, pairs, P), np.float32)
    # a capacity below what the feed closes: refused by both kinds, nothing consumed
    assert s.feed_into(raw, first, big_rgba, None, FRAMES)[0] == E and "true-peak" in L.sgz_last_error().decode()
    assert s.feed_overview_into(raw, first, K, False, big_rgba, peaks, FRAMES)[0] == E
    assert small.tobytes() == bytes(small.nbytes) and not big_rgba.any() and not peaks.any()
    assert s.truepeak_state() == (0, 0) and s.frames_for(first) == 2 and s.open_frames() == 0
    # ... the next feed's outputs are those of a stream that never saw the refusals
    out = np.zeros(want.shape, tr.DTYPE)
    s.set_truepeak(m, out)
    a = _feed(s, raw, fb, 0, first, "plain")
    b = _feed(twin, raw, fb, 0, first, "plain")
    assert _same([a], [b]) and a[1].shape[0] == 2 and s.truepeak_state() == (3, 200)
    assert _same_records(out[:3], want[:3])
    # another m while samples are open: refused, the lane as it was
    assert L.sgz_pcm_stream_set_truepeak(s.h, m + 1, out.ctypes.data, out.shape[0]) == E
    assert s.truepeak_state() == (3, 200) and s.truepeak_for(200) == 1
    # the other lanes' m is their own: armed beside an open true-peak column with another m
    wave = np.zeros((4, D, 2), np.float32)
    s.set_waveform(m + 1, wave)
    assert s.truepeak_state() == (3, 200) and s.waveform_state() == (0, 0)
    s.set_waveform(0)
    # the flush needs a column of its own
    s.set_truepeak(m, small)
    _feed(s, raw, fb, first, 600, "plain")
    assert s.truepeak_state() == (2, 0)
    _feed(s, raw, fb, first + 600, 30, "plain")
    assert s.truepeak_state() == (2, 30) and L.sgz_pcm_stream_flush_truepeak(s.h) == E and s.truepeak_state() == (2, 30)
    assert _same_records(small, want[3:5])
    # reset drops the open column, zeroes the history and restarts the cursor: the same file again gives a fresh stream's records
    s.reset()
    assert s.truepeak_state() == (0, 0)
    s.set_truepeak(m, out)
    out[:] = np.zeros((), tr.DTYPE)
    _, records = _run(s, raw, fb, [N], "plain", m, out)
    assert _same_records(records, want)
    # ... and so does a reset in mid-stream: the first record behind it is a fresh stream's, not one behind the old samples
    # (columns of 4 samples: shorter than the filter, so the history decides the first of them)
    r = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    short = np.zeros((10, D), tr.DTYPE)
    r.set_truepeak(4, short)
    _feed(r, raw, fb, 3000, 30, "plain")
    r.reset()
    assert r.truepeak_state() == (0, 0)
    _feed(r, raw, fb, 0, 8, "plain")
    assert r.truepeak_state() == (2, 0) and _same_records(short[:2], _want(name, 4)[:2])
    assert not _same_records(_want(name, 4)[:1], tr.records_of(planar[:, :4], 4, True, tr.history_after(planar[:, 3000:3030]))[0])
    r.close()
    # disarming drops the open column and the history too: another m is taken afterwards, from a zero history
    s.reset()
    _feed(s, raw, fb, 0, 430, "plain")
    assert s.truepeak_state() == (1, 30)
    s.set_truepeak(0)
    assert s.truepeak_state() == (0, 0) and s.truepeak_for(1000) == 0
    s.set_truepeak(7, out)
    assert s.truepeak_state() == (0, 0) and s.truepeak_for(15) == 2
    _feed(s, raw, fb, 430, 14, "plain")
    assert _same_records(out[:2], tr.records_of(planar[:, 430:444], 7)[0])
    s.close(); twin.close()


def test_create_feed_destroy_gives_the_memory_back(gpu):
    """200 create -> armed feeds -> flush -> destroy cycles after 5 to settle the allocators (64 MiB of slack, as tests/test_gpu_pcm.py)"""
    import torch
    name = "s16_3ch"
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb = channels * BYTES[fmt]
    ms = (5, 16, 1000, 4097)

    def cycle(i):
        m = ms[i % 4]
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=(500, 2000)[i % 2])
        out = np.zeros(_want(name, m).shape, tr.DTYPE)
        s.set_truepeak(m, out)
        _feed(s, raw, fb, 0, N // 2, "plain")
        _feed(s, raw, fb, N // 2, N - N // 2, "plain" if i % 3 else "overview")
        s.flush_truepeak()
        s.close()
        return out

    for i in range(5):
        cycle(i)
    gc.collect()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for i in range(200):
        assert _same_records(cycle(i), _want(name, ms[i % 4])), i
    gc.collect()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    if "PYTEST_XDIST_WORKER" not in os.environ:                   # (the figure is the DEVICE's: under pytest -n the other workers' allocations move it)
        assert free0 - free1 < 64 << 20, f"device memory: {(free0 - free1) / 2**20:.1f} MiB fewer free after 200 cycles"
