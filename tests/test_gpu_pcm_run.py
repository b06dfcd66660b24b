"""The run lane inside the PCM stream on the GPU (sgz_pcm_stream_set_run, _run_for, _run_state, _flush_run; csrc/pcm.hip,
csrc/run_columns.hip).

Byte for byte, no tolerance: the lane's records after the flush == tests/run_ref.py -- the per-sample definition -- of the numpy-converted
planar floats, for every m, chunk_samples, kind of feed and way of cutting the stream into feeds, pieces smaller than a column and feeds of
one sample among them; and everything the feeds return == an unarmed twin's.  Two files: "clip", 16-bit PCM made for the lane -- a hard-
clipped sine with a hole of digital silence that crosses piece and feed boundaries beside a channel of very few levels -- and
tests/test_gpu_pcm_level.py's float case with its NaN, infinities and denormals."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import run_ref as rr  # noqa: E402
from test_gpu_pcm import BYTES, convert_ref, to_bytes  # noqa: E402  (the converter's numpy reference)
from test_gpu_pcm_level import FRAMES, HOP, K, N, W, _feed, _kinds, _same  # noqa: E402  (feeds, the feeds' comparison)
from test_gpu_pcm_level import _case as _level_case  # noqa: E402
from test_gpu_pcm_overview import _feed_sizes  # noqa: E402  (the cuts)

pytestmark = pytest.mark.gpu

E = api.SGZ_EINVAL
NAMES = ("clip", "f32_two_pairs")
HOLE = (1490, 2610)                     # digital silence in "clip": across the boundaries of many pieces and feeds
_made, _wants = {}, {}


def _case(name):
    """(cfg, format, source channels, map, PCM bytes, planar floats [channels][N], the thresholds) -- once"""
    if name not in _made:
        if name == "clip":
            cfg = config.spectrum_config(window_size=W, hop=HOP, axis_points=100, num_pairs=1, pole=(0.3, 0.3))
            t = np.arange(N, dtype=np.float64)
            q = np.zeros((N, 2), np.int64)
            q[:, 0] = np.clip(np.rint(1.7 * 32768.0 * np.sin(2 * np.pi * t / 61.0)), -32768, 32767)
            q[HOLE[0]:HOLE[1], 0] = 0
            q[:, 1] = np.random.default_rng(2).integers(-2, 3, N)                           # five levels: equal neighbours, zeros, sign changes
            q[3990:4010, 1] = 7                                                         # a flat run across a piece boundary
            raw = to_bytes(q.reshape(-1), api.PCM_S16)
            _made[name] = (cfg, api.PCM_S16, 2, None, raw, np.ascontiguousarray(convert_ref(raw, api.PCM_S16, 2)), rr.DEFAULT)
        else:
            cfg, fmt, channels, cmap, raw, planar, _ = _level_case(name)
            _made[name] = (cfg, fmt, channels, cmap, raw, planar, (1 << 22, 1 << 15))
    return _made[name]


def _want(name, m):
    if (name, m) not in _wants:
        _wants[name, m] = rr.records(_case(name)[5], m, _case(name)[6])[0]
    return _wants[name, m]


def _params(name):
    return api.RunParams(*_case(name)[6])


def _same_records(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a, rr.DTYPE).tobytes() == np.ascontiguousarray(b, rr.DTYPE).tobytes()


def _run(s, raw, fb, sizes, mode, m=0, out=None, at=0, flush=True):
    """feeds the sizes in turn; armed (m > 0): checks run_for / run_state around every feed against sgz_overview_step chained, then flushes
    the lane -> (everything the feeds returned, the lane's records)"""
    returned = []
    written, open_ = s.run_state() if m else (0, 0)
    kinds = _kinds(mode, len(sizes))
    for size, kind in zip(sizes, kinds):
        if m:
            columns, left = api.overview_step(m, open_, size, False)
            assert s.run_for(size) == columns and s.run_for(size, True) == api.overview_step(m, open_, size, True)[0]
        returned.append(_feed(s, raw, fb, at, size, kind))
        at += size
        if m:
            written, open_ = written + columns, left
            assert s.run_state() == (written, open_), (size, kind)
    if kinds[-1] == "overview":
        returned.append(_feed(s, raw, fb, at, 0, "overview", flush=True))
    if not m:
        return returned, None
    if flush:
        s.flush_run()
        written += open_ > 0
        assert s.run_state() == (written, 0)
        s.flush_run()                                                   # nothing open: nothing happens
        assert s.run_state() == (written, 0)
    return returned, out[:written].copy()


def _sentinel(columns, channels):
    return np.full((columns, channels, 96), 0xA5, np.uint8).view(rr.DTYPE).reshape(columns, channels)


def test_the_clip_file_is_what_it_says():
    """(no GPU) the definition on "clip": clipped runs on both rails, one hole of silence, and the five-level channel's flat runs"""
    planar, params = _case("clip")[5], _case("clip")[6]
    whole = rr.records(planar, N, params)[0][0]
    hot, quiet, flat = (whole[0]["of"][k] for k in (rr.HOT, rr.QUIET, rr.FLAT))
    assert int(hot["runs"]) >= 2 * (N - (HOLE[1] - HOLE[0])) // 61 - 4 and int(hot["longest"]) >= 15
    assert (int(quiet["longest"]), int(quiet["at"])) == (HOLE[1] - HOLE[0], HOLE[0])
    assert (int(flat["longest"]), int(flat["at"])) == (HOLE[1] - HOLE[0] - 1, HOLE[0] + 1)
    other = whole[1]["of"][rr.FLAT]
    assert int(other["runs"]) > N // 10 and (int(other["longest"]), int(other["at"])) == (19, 3991) and int(whole[1]["crossings"]) > N // 10


@pytest.mark.parametrize("chunk", (0, 1000, 16))
@pytest.mark.parametrize("name", NAMES)
def test_lane_equals_the_definition_and_leaves_the_render_alone(gpu, name, chunk):
    cfg, fmt, channels, cmap, raw, planar, _ = _case(name)
    fb, D = channels * BYTES[fmt], planar.shape[0]
    rng = np.random.default_rng(len(name) + chunk)
    armed = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
    twin = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
    # (pieces of 16 samples: smaller than every column; they make a feed slow, so fewer of them)
    plan = (("plain", (32, 100)),) if chunk == 16 else (("plain", (32, 1000, N + 1)), ("overview", (100, 4097)), ("mixed", (33, 1025)))
    for mode, ms in plan:
        sizes = _feed_sizes(rng, N, W, HOP)
        assert 0 in sizes and 1 in sizes and any(0 < v < HOP for v in sizes), sizes
        twin.reset()
        unarmed, _ = _run(twin, raw, fb, sizes, mode)
        for m in ms:
            want = _want(name, m)
            out = _sentinel(want.shape[0] + 2, D)
            armed.reset()
            armed.set_run(_params(name), m, out)
            got, records = _run(armed, raw, fb, sizes, mode, m, out)
            what = (name, chunk, mode, m, sizes)
            assert _same_records(records, want), what
            assert out[want.shape[0]:].tobytes() == _sentinel(2, D).tobytes(), what
            assert _same(got, unarmed), what
        armed.reset()                                                  # the whole file in one feed: the pieces of chunk_samples inside it
        out = np.zeros(_want(name, 64).shape, rr.DTYPE)
        armed.set_run(_params(name), 64, out)
        _, records = _run(armed, raw, fb, [N], mode, 64, out)
        assert _same_records(records, _want(name, 64)), (name, chunk, mode)
    armed.set_run(None, 0)
    armed.reset()
    disarmed, _ = _run(armed, raw, fb, sizes, mode)
    assert _same(disarmed, unarmed) and armed.run_state() == (0, 0) and armed.run_for(N) == 0
    armed.close(); twin.close()


def test_feeds_of_one_sample_and_runs_across_feed_and_piece_boundaries(gpu):
    cfg, fmt, channels, cmap, raw, planar, params = _case("clip")
    fb, D, m = channels * BYTES[fmt], planar.shape[0], 40
    want = _want("clip", m)
    # the hole begins inside a feed, crosses ten feeds of one sample and a piece boundary (2505) inside a long feed, and ends inside a feed of 2;
    # channel 1's flat run at 3990 .. 4009 begins inside a long feed and crosses feeds of one and two samples
    sizes = [HOLE[0] + 5] + [1] * 10 + [1100, HOLE[1] - (HOLE[0] + 15 + 1100) - 1, 2] + [3995 - HOLE[1] - 1] + [1, 2, 1, 2, 1, 1]
    sizes.append(N - sum(sizes))
    assert min(sizes) > 0 and sum(sizes) == N
    for kind in ("plain", "overview"):
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
        out = np.zeros(want.shape, rr.DTYPE)
        s.set_run(_params("clip"), m, out)
        _, records = _run(s, raw, fb, sizes, kind, m, out)
        assert _same_records(records, want), kind
        s.close()
    # what the records say of the hole: whole columns of silence between a tail and a head, one run begun
    first, last = -(-HOLE[0] // m), HOLE[1] // m
    q = want["of"][:, 0, rr.QUIET]
    assert (q["head"][first:last] == m).all() and (q["tail"][first:last] == m).all() and int(q["runs"][first - 1:last].sum()) == 1
    assert int(q["tail"][first - 1]) == first * m - HOLE[0] and int(q["head"][last]) == HOLE[1] - last * m


def test_beside_the_level_lane_with_another_m(gpu):
    import level_ref as lr
    for name in NAMES:
        cfg, fmt, channels, cmap, raw, planar, _ = _case(name)
        fb, D, pairs = channels * BYTES[fmt], planar.shape[0], planar.shape[0] // 2
        rng = np.random.default_rng(17)
        lm, rm = 16, 33
        for mode in ("plain", "mixed"):
            sizes = _feed_sizes(rng, N, W, HOP)
            results = []
            for with_lane in (False, True):
                s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
                level = np.zeros((-(-N // lm), pairs), lr.DTYPE)
                s.set_level(lm, level)
                out = np.zeros(_want(name, rm).shape, rr.DTYPE)
                if with_lane:
                    s.set_run(_params(name), rm, out)
                got, records = _run(s, raw, fb, sizes, mode, rm if with_lane else 0, out)
                s.flush_level()
                assert s.level_state() == (-(-N // lm), 0)
                results.append((got, level.tobytes()))
                if with_lane:
                    assert _same_records(records, _want(name, rm)), (name, mode)
                s.close()
            a, b = results
            assert _same(a[0], b[0]) and a[1] == b[1] == lr.records_of(planar, lm)[0].tobytes(), (name, mode)


def test_draining_through_a_small_buffer_keeps_the_open_column_and_the_history(gpu):
    cfg, fmt, channels, cmap, raw, planar, _ = _case("clip")
    fb, D, m, cap = channels * BYTES[fmt], planar.shape[0], 32, 7
    want = _want("clip", m)
    rng = np.random.default_rng(3)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=64)
    small = [np.zeros((cap, D), rr.DTYPE), np.zeros((cap, D), rr.DTYPE)]
    which, kept, at, rearmed = 0, [], 0, 0
    s.set_run(_params("clip"), m, small[0])
    while at < N:
        size = min(int(rng.integers(0, (cap - 1) * m)), N - at)
        written, open_ = s.run_state()
        if written + s.run_for(size) > cap:                             # drain: re-arm with the other buffer -- the open column and the history stay
            kept.append(small[which][:written].copy())
            which ^= 1
            s.set_run(_params("clip"), m, small[which])
            assert s.run_state() == (0, open_)
            rearmed += 1
        _feed(s, raw, fb, at, size, "plain")
        at += size
    written, open_ = s.run_state()
    if written == cap:                                                  # (the flush needs a column of its own)
        kept.append(small[which][:written].copy())
        which ^= 1
        s.set_run(_params("clip"), m, small[which])
    s.flush_run()
    kept.append(small[which][:s.run_state()[0]].copy())
    assert rearmed >= 5 and _same_records(np.concatenate(kept), want)   # (marks for a history at any re-arm would begin a run behind it)
    s.close()


def test_a_flush_in_mid_stream_keeps_the_history_and_starts_a_new_column(gpu):
    cfg, fmt, channels, cmap, raw, planar, params = _case("clip")
    fb, D, m, cut = channels * BYTES[fmt], planar.shape[0], 64, 2003               # inside the hole: 2003 = 31 * 64 + 19
    head = rr.records(planar[:, :cut], m, params)[0]                               # the partial column closes as it stands
    tail = rr.records(planar[:, cut:], m, params, True, rr.history_after(planar[:, :cut]))[0]     # columns count from the flush on, behind the history
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=500)
    out = np.zeros((head.shape[0] + tail.shape[0], D), rr.DTYPE)
    s.set_run(_params("clip"), m, out)
    _run(s, raw, fb, [cut], "plain", m, out)
    assert s.run_state() == (head.shape[0], 0)
    _run(s, raw, fb, [700, N - cut - 700], "plain", m, out, at=cut)
    assert _same_records(out, np.concatenate([head, tail]))
    fresh = rr.records(planar[:, cut:], m, params)[0]
    assert not _same_records(tail[:1], fresh[:1])                                   # (the history matters to the first column behind the flush:
    assert int(tail[0, 0]["of"][rr.QUIET]["runs"]) == 0 and int(fresh[0, 0]["of"][rr.QUIET]["runs"]) == 1      # no run of silence begins there)
    s.close()


def test_counts_state_and_refusals(gpu):
    name = "f32_two_pairs"
    cfg, fmt, channels, cmap, raw, planar, params = _case(name)
    P, fb, D, pairs = cfg["axis_points"], channels * BYTES[fmt], planar.shape[0], planar.shape[0] // 2
    L = api.lib()
    m = 400
    want = _want(name, m)
    ok = _params(name)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    twin = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    assert s.run_for(N) == 0 and s.run_state() == (0, 0)               # disarmed
    assert L.sgz_pcm_stream_flush_run(s.h) == E
    assert L.sgz_pcm_stream_set_run(None, ok, m, None, 0) == E and L.sgz_pcm_stream_set_run(s.h, ok, m, None, 3) == E
    assert L.sgz_pcm_stream_run_state(None, None, None) == E
    odd = np.zeros(3 * D * 96 + 8, np.uint8)
    assert L.sgz_pcm_stream_set_run(s.h, ok, m, odd.ctypes.data + 1 + (-odd.ctypes.data) % 4, 3) == E        # not aligned to 4 bytes
    small = np.zeros((2, D), rr.DTYPE)
    for bad_m in (1, 31):                                               # 0 < m < 32
        assert L.sgz_pcm_stream_set_run(s.h, ok, bad_m, small.ctypes.data, 2) == E and "m >= 32" in L.sgz_last_error().decode()
    assert L.sgz_pcm_stream_set_run(s.h, None, m, small.ctypes.data, 2) == E and "null params" in L.sgz_last_error().decode()
    for hot, quiet in ((0, 0), (2**26 + 1, 0), (9, 9)):
        assert L.sgz_pcm_stream_set_run(s.h, api.RunParams(hot, quiet), m, small.ctypes.data, 2) == E
    assert s.run_for(N) == 0 and s.run_state() == (0, 0)               # (a refusal arms nothing)
    s.set_run(None, 0)                                                  # disarming needs no params
    first = 1400                                                        # three columns and 200 samples open; W + hop <= 1400: two frames
    s.set_run(ok, m, small)
    assert s.run_for(first) == 3 and s.run_for(first, True) == 4 and s.frames_for(first) == 2
    big_rgba = np.zeros((FRAMES, P, 4), np.uint8)
    peaks = np.zeros((FRAMES, pairs, P), np.float32)
    # a capacity below what the feed closes: refused by both kinds, nothing consumed
    assert s.feed_into(raw, first, big_rgba, None, FRAMES)[0] == E and "more run columns" in L.sgz_last_error().decode()
    assert s.feed_overview_into(raw, first, K, False, big_rgba, peaks, FRAMES)[0] == E
    assert small.tobytes() == bytes(small.nbytes) and not big_rgba.any() and not peaks.any()
    assert s.run_state() == (0, 0) and s.frames_for(first) == 2 and s.open_frames() == 0
    # ... the next feed's outputs are those of a stream that never saw the refusals
    out = np.zeros(want.shape, rr.DTYPE)
    s.set_run(ok, m, out)
    a = _feed(s, raw, fb, 0, first, "plain")
    b = _feed(twin, raw, fb, 0, first, "plain")
    assert _same([a], [b]) and a[1].shape[0] == 2 and s.run_state() == (3, 200)
    assert _same_records(out[:3], want[:3])
    # another m or other params while samples are open: refused, the lane as it was
    assert L.sgz_pcm_stream_set_run(s.h, ok, m + 1, out.ctypes.data, out.shape[0]) == E
    assert L.sgz_pcm_stream_set_run(s.h, api.RunParams(ok.hot - 1, ok.quiet), m, out.ctypes.data, out.shape[0]) == E
    assert s.run_state() == (3, 200) and s.run_for(200) == 1
    # the other lanes' m is their own: armed beside an open run column with another m
    wave = np.zeros((4, D, 2), np.float32)
    s.set_waveform(m + 1, wave)
    assert s.run_state() == (3, 200) and s.waveform_state() == (0, 0)
    s.set_waveform(0)
    # the flush needs a column of its own
    s.set_run(ok, m, small)
    _feed(s, raw, fb, first, 600, "plain")
    assert s.run_state() == (2, 0)
    _feed(s, raw, fb, first + 600, 30, "plain")
    assert s.run_state() == (2, 30) and L.sgz_pcm_stream_flush_run(s.h) == E and s.run_state() == (2, 30)
    assert _same_records(small, want[3:5])
    # reset drops the open column, sets the history to marks and restarts the cursor: the same file again gives a fresh stream's records
    s.reset()
    assert s.run_state() == (0, 0)
    s.set_run(ok, m, out)
    out[:] = np.zeros((), rr.DTYPE)
    _, records = _run(s, raw, fb, [N], "plain", m, out)
    assert _same_records(records, want)
    s.close(); twin.close()
    # ... and so does a reset in mid-stream: inside the hole of "clip" the first record behind it is a fresh stream's -- a run begins --, not
    # one behind the old samples; disarming drops the open column and the history too, and another m is taken afterwards
    cfg, fmt, channels, cmap, raw, planar, params = _case("clip")
    fb, D = channels * BYTES[fmt], planar.shape[0]
    r = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    short = np.zeros((10, D), rr.DTYPE)
    r.set_run(_params("clip"), 32, short)
    _feed(r, raw, fb, 1600, 40, "plain")
    assert r.run_state() == (1, 8)
    r.reset()
    assert r.run_state() == (0, 0)
    _feed(r, raw, fb, 1700, 64, "plain")
    fresh = rr.records(planar[:, 1700:1764], 32, params)[0]
    assert r.run_state() == (2, 0) and _same_records(short[:2], fresh) and int(fresh[0, 0]["of"][rr.QUIET]["runs"]) == 1
    _feed(r, raw, fb, 1764, 10, "plain")
    r.set_run(None, 0)
    assert r.run_state() == (0, 0) and r.run_for(1000) == 0
    r.set_run(_params("clip"), 35, short)
    assert r.run_state() == (0, 0) and r.run_for(70) == 2
    _feed(r, raw, fb, 1774, 70, "plain")
    assert _same_records(short[:2], rr.records(planar[:, 1774:1844], 35, params)[0])
    r.close()
