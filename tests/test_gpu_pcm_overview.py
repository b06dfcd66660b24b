"""The overview inside the PCM stream on the GPU (sgz_pcm_stream_feed_overview, sgz_pcm_stream_columns_for, sgz_pcm_stream_open_frames,
sgz_spectrogram_overview_pcm; csrc/pcm.hip, the slab loop in csrc/api.hip).

Byte for byte, image and peaks (uint32 views), no tolerance: the columns of all overview feeds of a stream, of which only the last
flushes, concatenated == Plan.overview (sgz_spectrogram_overview_host) of the numpy-converted planar floats -- for every k, chunk_samples,
SGZ_OPT_OVERVIEW_SLAB and way of cutting the stream into feeds.  With intermediate flushes: the column counts are sgz_overview_step's
chained over the feeds and the columns are tests/overview_ref.py's restatement of every segment between two flushes, on the line results
of sgz_spectrogram_render_host."""
import gc
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_ref as ov  # noqa: E402
from test_gpu_pcm import BYTES, convert_ref, to_bytes  # noqa: E402  (the converter's numpy reference)

pytestmark = pytest.mark.gpu

SPLIT = 8                                                          # SGZ_PATH_* (sgz.h)
CASES = {
    # cfg, frames, format, source channels, channel map (a subset of the source's channels, out of order)
    "w64": (dict(window_size=64, hop=16, axis_points=33, pole=(0.3, 0.3)), 23, api.PCM_S16, 3, [2, 0]),
    "w256_two_pairs": (dict(window_size=256, hop=64, axis_points=100, num_pairs=2, pole=(0.5, 0.5)), 23, api.PCM_F32, 5, [4, 0, 2, 1]),
    "n4096_two_pairs": (dict(window_size=4096, hop=1024, num_pairs=2, pole=(0.5, 0.5)), 23, api.PCM_S16, 5, [3, 1, 0, 4]),
    "phase": (dict(window_size=256, hop=64, axis_points=100, channel_mode=config.CH_PHASE, pole=(0.3, 0.3)), 23, api.PCM_F32, 3, [1, 2]),
    "n32768_split": (dict(window_size=32768, hop=8192, pole=(0.3, 0.3)), 6, api.PCM_S16, 3, [2, 1]),
    "odd_hop": (dict(window_size=1024, hop=333, axis_points=100, pole=(0.3, 0.3)), 10, api.PCM_F32, 3, [0, 2]),
}
CHUNKS = (0, 1000, 4096, 100000)
SLABS = (0, 1, 3)
_made = {}


def _case(name):
    """(cfg, format, source channels, map, PCM bytes, samples, frames, plan, planar floats, graph 0's first components [F][C][P]) -- once"""
    if name not in _made:
        over, frames, fmt, channels, cmap = CASES[name]
        cfg = config.spectrum_config(**over)
        x = ov.burst_signal(cfg["window_size"], cfg["hop"], frames, channels, cfg["sample_rate"], seed=7)        # [channels][S], every channel its own
        inter = np.ascontiguousarray(x.T).reshape(-1)
        raw = to_bytes(np.clip(np.round(inter.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int64), fmt) if fmt == api.PCM_S16 else to_bytes(inter, fmt)
        n = x.shape[1]
        planar = np.ascontiguousarray(convert_ref(raw, fmt, channels)[cmap])
        plan = api.Plan(cfg).upload()
        if name == "n32768_split":
            assert plan.path & SPLIT, plan.path
        assert plan.num_frames(n) == frames
        rgba, lines, _ = api.render_spectrogram_host(plan, planar, want_lines=True)
        main = np.ascontiguousarray(lines[:, :, 0, :, 0])
        for a in (raw, planar, rgba, main):
            a.setflags(write=False)
        _made[name] = (cfg, fmt, channels, cmap, raw, n, frames, plan, planar, rgba, main)
    return _made[name]


_wants = {}


def _want(name, k):
    """Plan.overview of the converted floats at k: (image, peaks bits)"""
    if (name, k) not in _wants:
        plan, planar = _case(name)[7], _case(name)[8]
        image, peaks, _ = plan.overview(planar, k, want_peaks=True)
        _wants[name, k] = (image, peaks.view(np.uint32))
    return _wants[name, k]


def _feed_sizes(rng, n, W, hop):
    """a cut of n samples into feeds: empty and one-sample feeds, feeds shorter than the hop and than the held tail, longer ones"""
    sizes, at = [], 0
    forced = [1, 0, hop - 1, W, 1, 0, max(1, W - hop - 1), 5]
    while at < n:
        kind = int(rng.integers(0, 6))
        size = [0, 1, int(rng.integers(1, hop)), int(rng.integers(1, W - hop + 1)), int(rng.integers(0, 3 * W + 1)), int(rng.integers(0, 3 * W + 1))][kind]
        size = min(forced.pop(0) if forced else size, n - at)
        sizes.append(size)
        at += size
    return sizes


def _run(s, raw, fb, sizes, k, last_flushes, W, hop):
    """feeds the sizes in turn (the last one flushing, or an empty flushing feed behind them); checks columns_for and open_frames around every
    feed against sgz_stream_step / sgz_overview_step chained; -> (image, peaks bits) of all feeds"""
    images, peaks, at, held, open_frames = [], [], 0, 0, 0
    feeds = [(size, last_flushes and i == len(sizes) - 1) for i, size in enumerate(sizes)] + ([] if last_flushes else [(0, True)])
    for size, flush in feeds:
        frames, held = api.stream_step(W, hop, held, size)
        columns, open_frames = api.overview_step(k, open_frames, frames, flush)
        assert s.columns_for(size, k, flush) == columns
        image, v, t = s.feed_overview(raw[at * fb:(at + size) * fb] if size else None, k, flush=flush, nsamples=size, want_peaks=True)
        assert image.shape[0] == v.shape[0] == columns == t["frames"] and s.open_frames() == open_frames, (size, flush, columns, open_frames)
        images.append(image)
        peaks.append(v.view(np.uint32))
        at += size
    return np.concatenate(images), np.concatenate(peaks)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", list(CASES))
def test_streamed_overview_equals_the_overview_of_the_converted_floats(gpu, name, chunk):
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case(name)
    W, hop, fb = cfg["window_size"], cfg["hop"], channels * BYTES[fmt]
    rng = np.random.default_rng(len(name) + chunk)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
    runs = 0
    for k in sorted({1, 2, 5, 7, F, F + 3}):
        image, peaks = _want(name, k)
        for slab in SLABS:
            s.set_option(api.OPT_OVERVIEW_SLAB, slab)
            for mode in ("one feed", "random feeds", "random feeds, then an empty flushing feed"):
                s.reset()
                sizes = [n] if mode == "one feed" else _feed_sizes(rng, n, W, hop)
                if mode != "one feed":
                    assert 0 in sizes and 1 in sizes and any(0 < v < hop for v in sizes), sizes
                got_image, got_peaks = _run(s, raw, fb, sizes, k, mode != "random feeds, then an empty flushing feed", W, hop)
                what = (name, chunk, k, slab, mode, sizes)
                assert np.array_equal(got_peaks, peaks), what
                assert np.array_equal(got_image, image), what
                assert s.open_frames() == 0
                runs += 1
    assert runs == 6 * 3 * 3
    s.close()


def test_k1_streamed_is_the_feeds_image(gpu):
    for name in ("w64", "n4096_two_pairs"):
        cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case(name)
        a = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=3000)
        b = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=3000)
        want, _, _ = a.feed(raw)
        got, peaks, t = b.feed_overview(raw, 1, want_peaks=True)
        assert np.array_equal(got, want) and np.array_equal(want, rgba) and np.array_equal(peaks.view(np.uint32), main.view(np.uint32)), name
        assert b.open_frames() == 0 and t["frames"] == F
        a.close(); b.close()


@pytest.mark.parametrize("name", ["w64", "w256_two_pairs", "odd_hop"])
def test_intermediate_flushes_close_the_open_column(gpu, oracle, name):
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case(name)
    params = oracle.params_from_dict(cfg)
    W, hop, fb = cfg["window_size"], cfg["hop"], channels * BYTES[fmt]
    for seed, chunk in ((4, 0), (6, 1000), (8, W + hop - 1)):
        rng = np.random.default_rng(seed)
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
        sizes = _feed_sizes(rng, n, W, hop)
        at = held = open_frames = done = 0
        k = int(rng.choice([2, 3, 5]))
        segment = 0                                                  # the first frame of the segment: the frames since the last flush
        flushed = early = 0                                          # flushes that returned columns; those that closed a column early
        for i, size in enumerate(sizes + [0, 0]):
            flush = bool(rng.integers(0, 3) == 0) or i >= len(sizes)                        # (the last two feeds: a flush, and a flush with nothing open)
            frames, held = api.stream_step(W, hop, held, size)
            columns, left = api.overview_step(k, open_frames, frames, flush)
            assert s.columns_for(size, k, flush) == columns
            image, v, t = s.feed_overview(raw[at * fb:(at + size) * fb] if size else None, k, flush=flush, nsamples=size, want_peaks=True)
            assert image.shape[0] == v.shape[0] == columns and s.open_frames() == left, (name, seed, i, size, flush)
            # the restatement: the columns of frames [segment, done + frames) at k, of which the first (done - segment) // k were returned already
            upto = done + frames
            want_v, _, _ = ov.columns_of(main[segment:upto], k, flush=flush)
            want_v = want_v[(done - segment) // k:]
            assert np.array_equal(v.view(np.uint32), want_v), (name, seed, i, size, flush, k)
            assert np.array_equal(image, ov.blend(oracle, params, want_v)), (name, seed, i, size, flush, k)
            early += flush and i < len(sizes) and (open_frames + frames) % k != 0
            at, done, open_frames = at + size, upto, left
            if flush:
                flushed += columns > 0
                segment = done
                k = int(rng.choice([1, 2, 3, 5, 7]))                 # nothing is open: the next column may have another k
        assert done == F and flushed >= 2 and early >= 2 and s.open_frames() == 0, (name, seed, flushed, early)
        empty, _, _ = s.feed_overview(None, k, flush=True)
        assert empty.shape[0] == 0
        s.close()


def test_refusals_leave_the_stream_unchanged(gpu):
    name = "w256_two_pairs"
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case(name)
    W, hop, P, Cn, fb = cfg["window_size"], cfg["hop"], cfg["axis_points"], cfg["num_pairs"], channels * BYTES[fmt]
    k = 5
    image, peaks = _want(name, k)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    first = W + 11 * hop + 17                                        # 12 frames: two columns and two frames open
    need = s.columns_for(first, k, False)
    assert need == 2 and s.columns_for(first, k, True) == 3
    small = np.zeros((need, P, 4), np.uint8)
    small_v = np.zeros((need, Cn, P), np.float32)
    E = api.SGZ_EINVAL
    # a capacity below the need: refused, the need reported, nothing consumed
    st, c, _ = s.feed_overview_into(raw, first, k, False, small, small_v, need - 1)
    assert st == E and c == need and not small.any() and not small_v.any() and s.columns_for(first, k, False) == need and s.open_frames() == 0
    st, c, _ = s.feed_overview_into(raw, first, k, True, small, small_v, need)             # (flushing needs one more)
    assert st == E and c == need + 1 and s.open_frames() == 0
    assert s.feed_overview_into(raw, first, 0, False, small, small_v, need)[0] == E        # k == 0
    assert s.feed_overview_into(raw, first, k, False, None, None, need)[0] == E            # both outputs NULL
    assert s.feed_overview_into(None, first, k, False, small, small_v, need)[0] == E       # a null pcm
    assert s.columns_for(first, k, False) == need and s.columns_for(first, 0, False) == 0 and s.frames_for(first) == 12
    a, va, _ = s.feed_overview(raw[:first * fb], k, want_peaks=True)
    assert a.shape[0] == 2 and s.open_frames() == 2
    # an open column: another k is refused, and so is the plain feed; the stream goes on as if they had not been tried
    rest = n - first
    assert s.columns_for(rest, k + 1, True) == 0
    big = np.zeros((F, P, 4), np.uint8)
    big_v = np.zeros((F, Cn, P), np.float32)
    assert s.feed_overview_into(raw[first * fb:], rest, k + 1, True, big, big_v, F)[0] == E
    assert s.feed_overview_into(raw[first * fb:], rest, 1, True, big, big_v, F)[0] == E
    st, f, _ = s.feed_into(raw[first * fb:], rest, big, None, F)
    assert st == E and "flush" in api.lib().sgz_last_error().decode() and not big.any() and not big_v.any()
    assert s.open_frames() == 2 and s.frames_for(rest) == F - 12
    b, vb, _ = s.feed_overview(raw[first * fb:], k, flush=True, want_peaks=True)
    assert np.array_equal(np.concatenate([a, b]), image) and np.array_equal(np.concatenate([va, vb]).view(np.uint32), peaks)
    # after the flush the plain feed is taken again, and any k
    assert s.open_frames() == 0 and s.feed_into(None, 0, big, None, F)[0] == api.SGZ_OK
    # reset drops the open column and the held samples: the same file again gives the same columns
    s.reset()
    s.feed_overview(raw[:first * fb], k)
    assert s.open_frames() == 2
    s.reset()
    assert s.open_frames() == 0 and s.frames_for(W - 1) == 0 and s.columns_for(W, 7, False) == 0 and s.columns_for(W, 7, True) == 1
    c, vc, _ = s.feed_overview(raw, 7, flush=True, want_peaks=True)
    assert np.array_equal(c, _want(name, 7)[0]) and np.array_equal(vc.view(np.uint32), _want(name, 7)[1])
    # a stream shorter than a window: no column, and the flush returns none
    s.reset()
    for size, flush in ((0, False), (1, False), (hop - 1, True), (W - hop - 1, False), (0, True)):
        a, va, t = s.feed_overview(raw[:size * fb] if size else None, k, flush=flush, nsamples=size, want_peaks=True)
        assert a.shape[0] == 0 and va.shape[0] == 0 and t["frames"] == 0 and s.open_frames() == 0
    s.close()
    # RSNT is refused at create, as before
    with pytest.raises(api.SgzError) as e:
        api.PcmStream(dict(cfg, algorithm=config.ALGO_RSNT), fmt, channels, cmap)
    assert e.value.status == api.SGZ_EUNSUPPORTED


def test_pinned_outputs_and_the_one_shot_call(gpu):
    import torch
    for name in ("w256_two_pairs", "n32768_split"):
        cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case(name)
        W, fb = cfg["window_size"], channels * BYTES[fmt]
        for k in (2, 7):
            image, peaks = _want(name, k)
            pcm = torch.from_numpy(raw.copy()).pin_memory()
            out = torch.zeros(image.shape, dtype=torch.uint8).pin_memory()
            out_v = torch.zeros(peaks.shape, dtype=torch.float32).pin_memory()
            s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=5000)
            st, c, t = s.feed_overview_into(pcm, n, k, True, out, out_v, image.shape[0])
            assert st == api.SGZ_OK and c == image.shape[0] == t.frames and t.chunks == -(-n // 5000)
            assert np.array_equal(out.numpy(), image) and np.array_equal(out_v.numpy().view(np.uint32), peaks), (name, k)
            # one output alone, pinned or pageable: the other is not touched
            s.reset()
            out.zero_()
            st, c, _ = s.feed_overview_into(pcm, n, k, True, out, None, image.shape[0])
            assert st == api.SGZ_OK and np.array_equal(out.numpy(), image)
            s.reset()
            none, v, _ = s.feed_overview(raw, k, flush=True, want_rgba=False, want_peaks=True)
            assert none is None and np.array_equal(v.view(np.uint32), peaks)
            s.close()
            st, a, v, t = api.overview_pcm(cfg, raw, fmt, channels, k, cmap, want_peaks=True)
            assert st == api.SGZ_OK and t["chunks"] == 1 and t["frames"] == image.shape[0]
            assert np.array_equal(a, image) and np.array_equal(v.view(np.uint32), peaks), (name, k)
        st, a, v, _ = api.overview_pcm(cfg, raw[:(W - 1) * fb], fmt, channels, 2, cmap, want_peaks=True)
        assert st == api.SGZ_SKIPPED_FRAME and a.shape[0] == 0 and v.shape[0] == 0


def test_overview_feed_beside_a_background_render(gpu):
    from test_gpu_concurrency import BackgroundLoad
    names = ("n32768_split", "w256_two_pairs")
    streams = {name: api.PcmStream(_case(name)[0], *_case(name)[1:4], chunk_samples=20000) for name in names}
    want = {name: _want(name, 5) for name in names}
    with BackgroundLoad(gpu) as load:
        beside = 0
        for _ in range(400):                                         # (the load's threads build their plans first: go on until three rounds ran beside it)
            busy = load.renders > 0
            for name in names:
                s = streams[name]
                s.reset()
                image, v, _ = s.feed_overview(_case(name)[4], 5, flush=True, want_peaks=True)
                assert np.array_equal(image, want[name][0]) and np.array_equal(v.view(np.uint32), want[name][1]), name
            beside += busy
            if beside >= 3 or load.errors:
                break
        assert beside >= 3, (beside, load.errors)
    for s in streams.values():
        s.close()


def test_create_feed_destroy_gives_the_memory_back(gpu):
    """100 create -> overview feeds -> destroy cycles after 5 to settle the allocators (64 MiB of slack, as tests/test_gpu_pcm.py)"""
    import torch
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case("w256_two_pairs")
    fb = channels * BYTES[fmt]

    def cycle(i):
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=2000)
        k = 1 + i % 7
        a, va, _ = s.feed_overview(raw[:(n // 2) * fb], k, want_peaks=True)
        b, vb, _ = s.feed_overview(raw[(n // 2) * fb:], k, flush=True, want_peaks=bool(i % 2))
        s.close()
        return np.concatenate([a, b])

    for i in range(5):
        cycle(i)
    gc.collect()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for i in range(100):
        assert np.array_equal(cycle(i), _want("w256_two_pairs", 1 + i % 7)[0])
    gc.collect()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    if "PYTEST_XDIST_WORKER" not in os.environ:                   # (the figure is the DEVICE's: under pytest -n the other workers' allocations move it)
        assert free0 - free1 < 64 << 20, f"device memory: {(free0 - free1) / 2**20:.1f} MiB fewer free after 100 cycles"
