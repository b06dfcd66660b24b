"""The level lane inside the PCM stream on the GPU (sgz_pcm_stream_set_level, _level_for, _level_state, _flush_level; csrc/pcm.hip,
csrc/level_columns.hip).

Byte for byte, no tolerance: the lane's records after the flush == tests/level_ref.py of the numpy-converted planar floats, for every m,
chunk_samples, kind of feed and way of cutting the stream into feeds; for the integer formats also == integer arithmetic on the raw PCM (the
exactness claim: at a scale of 2^23 the quantiser is the identity on S16 and S24); and everything the feeds return == an unarmed twin's."""
import gc
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import level_ref as lr  # noqa: E402
import wave_ref as wr  # noqa: E402
from test_gpu_pcm import BYTES, convert_ref, to_bytes  # noqa: E402  (the converter's numpy reference)
from test_gpu_pcm_overview import _feed_sizes  # noqa: E402  (the cuts)

pytestmark = pytest.mark.gpu

# every case at hop 333: format, source channels, channel map, pairs
CASES = {
    "s16_3ch": (api.PCM_S16, 3, [2, 0], 1),
    "s24": (api.PCM_S24, 2, None, 1),
    "f32_two_pairs": (api.PCM_F32, 5, [4, 0, 2, 1], 2),
}
NAMES = tuple(CASES)
CHUNKS = (0, 1000, 4096)
W, HOP, FRAMES = 1024, 333, 14
N = W + (FRAMES - 1) * HOP + 7                                         # 5360 samples: m = 4097 closes a column
K = 3                                                                  # frames per overview column of the overview feeds
E = api.SGZ_EINVAL
_made, _wants = {}, {}


def _case(name):
    """(cfg, format, source channels, map, PCM bytes, planar floats [2 pairs][N], the mapped raw integers [2 pairs][N] or None) -- once"""
    if name not in _made:
        fmt, channels, cmap, pairs = CASES[name]
        cfg = config.spectrum_config(window_size=W, hop=HOP, axis_points=100, num_pairs=pairs, pole=(0.3, 0.3))
        rng = np.random.default_rng(len(name))
        t = np.arange(N)[:, None]
        x = 0.4 * np.sin(2 * np.pi * t * (0.01 + 0.013 * np.arange(channels))[None, :]) + 0.2 * rng.standard_normal((N, channels)) + 0.05    # (a DC offset)
        ints = None
        if fmt == api.PCM_F32:
            v = x.astype(np.float32)
            v[100:140] *= np.float32(3.0)                              # overs, and past them
            v[200, 0], v[201, 4], v[202, 2] = np.nan, np.inf, -np.inf  # a NaN on one side of a pair, the infinities
            v[300:303, 1] = np.array([1e-40, -1e-45, 1.0], np.float32)  # denormals, full scale
            raw = to_bytes(v.reshape(-1), fmt)
        else:
            bits = 16 if fmt == api.PCM_S16 else 24
            top = 1 << (bits - 1)
            q = np.clip(np.round(x * top), -top, top - 1).astype(np.int64)
            q[50, :], q[51, :] = -top, top - 1                         # the type's extremes: -1.0 is an over
            raw = to_bytes(q.reshape(-1), fmt)
            ints = np.ascontiguousarray(q.T[cmap if cmap is not None else list(range(channels))]) << (24 - bits)
        planar = np.ascontiguousarray(convert_ref(raw, fmt, channels)[cmap if cmap is not None else list(range(channels))])
        _made[name] = (cfg, fmt, channels, cmap, raw, planar, ints)
    return _made[name]


def _want(name, m):
    if (name, m) not in _wants:
        _wants[name, m] = lr.records_of(_case(name)[5], m)[0]
    return _wants[name, m]


def _ms():
    return (1, 5, 16, 1000, 4097, N + 1)


def _same_records(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a, lr.DTYPE).tobytes() == np.ascontiguousarray(b, lr.DTYPE).tobytes()


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
    """feeds the sizes in turn; armed (m > 0): checks level_for / level_state around every feed against sgz_overview_step chained, then
    flushes the lane -> (everything the feeds returned, the lane's records)"""
    returned, at, written, open_ = [], 0, 0, 0
    kinds = _kinds(mode, len(sizes))
    for size, kind in zip(sizes, kinds):
        if m:
            columns, left = api.overview_step(m, open_, size, False)
            assert s.level_for(size) == columns and s.level_for(size, True) == api.overview_step(m, open_, size, True)[0]
        returned.append(_feed(s, raw, fb, at, size, kind))
        at += size
        if m:
            written, open_ = written + columns, left
            assert s.level_state() == (written, open_), (size, kind)
    if kinds[-1] == "overview":
        returned.append(_feed(s, raw, fb, at, 0, "overview", flush=True))
    if not m:
        return returned, None
    s.flush_level()
    written += open_ > 0
    assert s.level_state() == (written, 0)
    s.flush_level()                                                    # nothing open: nothing happens
    assert s.level_state() == (written, 0)
    return returned, out[:written].copy()


def _same(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) for x, y in zip(a, b))


def _sentinel(columns, pairs):
    return np.full((columns, pairs, 80), 0xA5, np.uint8).view(lr.DTYPE).reshape(columns, pairs)


@pytest.mark.parametrize("name", NAMES)
def test_integer_pcm_is_its_own_quantisation(gpu, name):
    """the exactness claim's host half: level_ref of the converted floats == integer arithmetic on the raw PCM (S16: sample << 8, S24: the
    sample itself); the GPU half is the test below, which holds the lane to the former"""
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    if ints is None:
        v, has = lr.quantise(planar)
        assert not has.all() and (np.abs(v) > lr.FULL).any()           # the float case carries what integers cannot: NaNs, values above full scale
        return
    v, has = lr.quantise(planar)
    assert has.all() and np.array_equal(v, ints) and (np.abs(ints) == lr.FULL).any()
    for m in _ms():
        assert _same_records(lr.records_of_integers(ints, np.ones(ints.shape, bool), m)[0], _want(name, m)), (name, m)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", NAMES)
def test_lane_equals_the_definition_and_leaves_the_render_alone(gpu, name, chunk):
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb, pairs = channels * BYTES[fmt], planar.shape[0] // 2
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
                want_int = lr.records_of_integers(ints, np.ones(ints.shape, bool), m)[0]
            out = _sentinel(want.shape[0] + 2, pairs)
            armed.reset()
            armed.set_level(m, out)
            got, level = _run(armed, raw, fb, sizes, mode, m, out)
            what = (name, chunk, mode, m, sizes)
            assert _same_records(level, want), what
            assert ints is None or _same_records(level, want_int), what
            assert out[want.shape[0]:].tobytes() == _sentinel(2, pairs).tobytes(), what
            assert _same(got, unarmed), what
            runs += 1
        one = [N]                                                      # the whole file in one feed: the pieces of chunk_samples inside it
        armed.reset()
        out = np.zeros(_want(name, 16).shape, lr.DTYPE)
        armed.set_level(16, out)
        _, level = _run(armed, raw, fb, one, mode, 16, out)
        assert _same_records(level, _want(name, 16)), (name, chunk, mode)
    assert runs == 18
    armed.set_level(0)
    armed.reset()
    disarmed, _ = _run(armed, raw, fb, sizes, "mixed")
    assert _same(disarmed, unarmed) and armed.level_state() == (0, 0) and armed.level_for(N) == 0
    armed.close(); twin.close()


@pytest.mark.parametrize("name", NAMES)
def test_beside_the_waveform_and_track_lanes(gpu, name):
    """all three lanes armed against a twin with the waveform and track lanes alone: what the feeds return, the waveform's columns and the
    track's records are the twin's byte for byte; the level lane's m is its own"""
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    fb, D, pairs = channels * BYTES[fmt], planar.shape[0], planar.shape[0] // 2
    rng = np.random.default_rng(17)
    wm, lm = 7, 16
    for mode in ("plain", "mixed"):
        sizes = _feed_sizes(rng, N, W, HOP)
        results = []
        for with_level in (False, True):
            s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
            wave = np.zeros((N // wm + 1, D, 2), np.float32)
            track = np.zeros((FRAMES, pairs, 6), np.float64)
            s.set_waveform(wm, wave)
            s.set_track(0, 0.5, track, FRAMES)
            out = np.zeros(_want(name, lm).shape, lr.DTYPE)
            if with_level:
                s.set_level(lm, out)
            got, level = _run(s, raw, fb, sizes, mode, lm if with_level else 0, out)
            s.flush_waveform()
            assert s.waveform_state() == (N // wm + 1, 0) and s.track_state() == FRAMES
            results.append((got, wave.view(np.uint32).copy(), track.view(np.uint64).copy()))
            if with_level:
                assert _same_records(level, _want(name, lm)), (name, mode)
            s.close()
        a, b = results
        assert _same(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (name, mode)
        assert np.array_equal(a[1], wr.columns_of(planar, wm)[0])


def test_a_piece_without_a_frame_still_delivers_its_records(gpu):
    cfg, fmt, channels, cmap, raw, planar, ints = _case("f32_two_pairs")
    fb, pairs, m = channels * BYTES[fmt], planar.shape[0] // 2, 5
    want = _want("f32_two_pairs", m)
    for chunk in (0, 16):                                              # one piece per feed; several frameless pieces inside a feed
        for kind in ("plain", "overview"):
            s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
            out = np.zeros(want.shape, lr.DTYPE)
            s.set_level(m, out)
            at = 0
            for size in (199, 200, 201, 202, 203):                     # 1005 samples: never a window
                assert s.frames_for(size) == 0
                got = _feed(s, raw, fb, at, size, kind)
                at += size
                assert got[1].shape[0] == 0
                assert s.level_state() == (at // m, at % m)
                assert _same_records(out[:at // m], want[:at // m]), (chunk, kind, at)       # delivered when the feed returns
                assert out[at // m:].tobytes() == bytes(80 * pairs * (want.shape[0] - at // m))
            s.close()


def test_pinned_and_pageable_destinations(gpu):
    import torch
    for name in ("s16_3ch", "f32_two_pairs"):
        cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
        fb, pairs = channels * BYTES[fmt], planar.shape[0] // 2
        for m in (5, 1000):
            want = _want(name, m)
            s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
            pinned = torch.zeros((want.shape[0], pairs, 80), dtype=torch.uint8).pin_memory()
            view = pinned.numpy().view(lr.DTYPE).reshape(want.shape)
            s.set_level(m, pinned)
            _run(s, raw, fb, [N // 3, N - N // 3], "plain", m, view)
            assert _same_records(view, want), (name, m)
            s.reset()
            pageable = np.zeros(want.shape, lr.DTYPE)
            s.set_level(m, pageable)                                   # the same stream, now through the pinned twins
            _run(s, raw, fb, [N // 3, N - N // 3], "overview", m, pageable)
            assert _same_records(pageable, want), (name, m)
            s.close()


def test_draining_through_a_small_buffer(gpu):
    cfg, fmt, channels, cmap, raw, planar, ints = _case("s24")
    fb, pairs, m, cap = channels * BYTES[fmt], planar.shape[0] // 2, 16, 7
    want = _want("s24", m)
    rng = np.random.default_rng(3)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=64)
    small = [np.zeros((cap, pairs), lr.DTYPE), np.zeros((cap, pairs), lr.DTYPE)]
    which, kept, at, rearmed = 0, [], 0, 0
    s.set_level(m, small[0])
    while at < N:
        size = min(int(rng.integers(0, (cap - 1) * m)), N - at)
        written, open_ = s.level_state()
        if written + s.level_for(size) > cap:                          # drain: keep what is there, re-arm with the other buffer -- the open column stays
            kept.append(small[which][:written].copy())
            which ^= 1
            s.set_level(m, small[which])
            assert s.level_state() == (0, open_)
            rearmed += 1
        _feed(s, raw, fb, at, size, "plain")
        at += size
    written, open_ = s.level_state()
    if written == cap:                                                 # (the flush needs a column of its own)
        kept.append(small[which][:written].copy())
        which ^= 1
        s.set_level(m, small[which])
    s.flush_level()
    kept.append(small[which][:s.level_state()[0]].copy())
    assert rearmed >= 5 and _same_records(np.concatenate(kept), want)
    s.close()


def test_counts_state_and_refusals(gpu):
    name = "f32_two_pairs"
    cfg, fmt, channels, cmap, raw, planar, ints = _case(name)
    P, fb, pairs = cfg["axis_points"], channels * BYTES[fmt], planar.shape[0] // 2
    L = api.lib()
    m = 400
    want = _want(name, m)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    twin = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    assert s.level_for(N) == 0 and s.level_state() == (0, 0)           # disarmed
    assert L.sgz_pcm_stream_flush_level(s.h) == E
    assert L.sgz_pcm_stream_set_level(None, m, None, 0) == E and L.sgz_pcm_stream_set_level(s.h, m, None, 3) == E
    assert L.sgz_pcm_stream_level_state(None, None, None) == E
    odd = np.zeros(3 * pairs * 80 + 8, np.uint8)
    assert L.sgz_pcm_stream_set_level(s.h, m, odd.ctypes.data + 1 + (-odd.ctypes.data) % 8, 3) == E        # not aligned to 8 bytes
    first = 1400                                                       # three columns and 200 samples open; W + hop <= 1400: two frames
    small = np.zeros((2, pairs), lr.DTYPE)
    s.set_level(m, small)
    assert s.level_for(first) == 3 and s.level_for(first, True) == 4 and s.frames_for(first) == 2
    big_rgba = np.zeros((FRAMES, P, 4), np.uint8)
    peaks = np.zeros((FRAMES, pairs, P), np.float32)
    # a capacity below what the feed closes: refused by both kinds, nothing consumed
    assert s.feed_into(raw, first, big_rgba, None, FRAMES)[0] == E and "level" in L.sgz_last_error().decode()
    assert s.feed_overview_into(raw, first, K, False, big_rgba, peaks, FRAMES)[0] == E
    assert small.tobytes() == bytes(small.nbytes) and not big_rgba.any() and not peaks.any()
    assert s.level_state() == (0, 0) and s.frames_for(first) == 2 and s.open_frames() == 0
    # ... the next feed's outputs are those of a stream that never saw the refusals
    out = np.zeros(want.shape, lr.DTYPE)
    s.set_level(m, out)
    a = _feed(s, raw, fb, 0, first, "plain")
    b = _feed(twin, raw, fb, 0, first, "plain")
    assert _same([a], [b]) and a[1].shape[0] == 2 and s.level_state() == (3, 200)
    assert _same_records(out[:3], want[:3])
    # another m while samples are open: refused, the lane as it was
    assert L.sgz_pcm_stream_set_level(s.h, m + 1, out.ctypes.data, out.shape[0]) == E
    assert s.level_state() == (3, 200) and s.level_for(200) == 1
    # the waveform lane's m is its own: armed beside an open level column with another m
    wave = np.zeros((4, 2 * pairs, 2), np.float32)
    s.set_waveform(m + 1, wave)
    assert s.level_state() == (3, 200) and s.waveform_state() == (0, 0)
    s.set_waveform(0)
    # the flush needs a column of its own
    s.set_level(m, small)
    _feed(s, raw, fb, first, 600, "plain")
    assert s.level_state() == (2, 0)
    _feed(s, raw, fb, first + 600, 30, "plain")
    assert s.level_state() == (2, 30) and L.sgz_pcm_stream_flush_level(s.h) == E and s.level_state() == (2, 30)
    assert _same_records(small, want[3:5])
    # reset drops the open column and restarts the cursor; the same file again gives the same records
    s.reset()
    assert s.level_state() == (0, 0)
    s.set_level(m, out)
    out[:] = np.zeros((), lr.DTYPE)
    _, level = _run(s, raw, fb, [N], "plain", m, out)
    assert _same_records(level, want)
    # disarming drops the open column too: another m is taken afterwards
    s.reset()
    _feed(s, raw, fb, 0, 430, "plain")
    assert s.level_state() == (1, 30)
    s.set_level(0)
    assert s.level_state() == (0, 0) and s.level_for(1000) == 0
    s.set_level(7, out)
    assert s.level_state() == (0, 0) and s.level_for(15) == 2
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
        out = np.zeros(_want(name, m).shape, lr.DTYPE)
        s.set_level(m, out)
        _feed(s, raw, fb, 0, N // 2, "plain")
        _feed(s, raw, fb, N // 2, N - N // 2, "plain" if i % 3 else "overview")
        s.flush_level()
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
