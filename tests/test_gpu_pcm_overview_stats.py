"""The mean overview inside the PCM stream on the GPU (sgz_pcm_stream_feed_overview_stats, sgz_spectrogram_overview_stats_pcm; csrc/pcm.hip, the
slab loop in csrc/api.hip).

Byte for byte -- image, records and means --, no tolerance: the columns of all stats feeds of a stream, of which only the last flushes,
concatenated == Plan.overview_stats (sgz_spectrogram_overview_stats_host) of the numpy-converted planar floats, for 16-bit and fp32 PCM, every
way of cutting the stream into feeds (the whole file and one-sample feeds included), two chunk_samples and two SGZ_OPT_OVERVIEW_SLAB; that
reference in turn == tests/overview_stats_ref.py on sgz_spectrogram_render_host's line results.  A column is of one kind: the kind-mixing
refusals consume nothing; a plain feed after a flush is that of a stream that never ran a stats feed; armed waveform and track lanes return what
they return under a peak-hold feed.  The cases and the feed cutter are those of tests/test_gpu_pcm_overview.py, imported from there."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_stats_ref as osr  # noqa: E402
from test_gpu_pcm import BYTES  # noqa: E402
from test_gpu_pcm_overview import _case, _feed_sizes  # noqa: E402

pytestmark = pytest.mark.gpu

_wants = {}


def _want(name, k):
    """Plan.overview_stats of the converted floats at k: (image, records, mean bits) -- held to the restatement once"""
    if (name, k) not in _wants:
        from oracle import pyoracle as po
        cfg, plan, planar, main = _case(name)[0], _case(name)[7], _case(name)[8], _case(name)[10]
        image, stats, means, _ = plan.overview_stats(planar, k, want_stats=True, want_means=True)
        want = osr.columns_of(main, k)[0]
        assert osr.same(stats, want) and np.array_equal(means.view(np.uint32), osr.mean_bits(want))
        assert np.array_equal(image, osr.blend(po, po.params_from_dict(cfg), want))
        _wants[name, k] = (image, stats, means.view(np.uint32))
    return _wants[name, k]


def _run(s, raw, fb, sizes, k, last_flushes, W, hop):
    """feeds the sizes in turn (the last one flushing, or an empty flushing feed behind them); checks columns_for and open_frames around every
    feed against sgz_stream_step / sgz_overview_step chained; -> (image, records, mean bits) of all feeds"""
    images, stats, means, at, held, open_frames = [], [], [], 0, 0, 0
    feeds = [(size, last_flushes and i == len(sizes) - 1) for i, size in enumerate(sizes)] + ([] if last_flushes else [(0, True)])
    for size, flush in feeds:
        frames, held = api.stream_step(W, hop, held, size)
        columns, open_frames = api.overview_step(k, open_frames, frames, flush)
        assert s.columns_for(size, k, flush) == columns
        image, r, m, t = s.feed_overview_stats(raw[at * fb:(at + size) * fb] if size else None, k, flush=flush, nsamples=size, want_means=True)
        assert image.shape[0] == r.shape[0] == m.shape[0] == columns == t["frames"] and s.open_frames() == open_frames, (size, flush, columns)
        images.append(image); stats.append(r); means.append(m.view(np.uint32))
        at += size
    return np.concatenate(images), np.concatenate(stats), np.concatenate(means)


@pytest.mark.parametrize("chunk", [1000, 0])
@pytest.mark.parametrize("name", ["w64", "w256_two_pairs", "odd_hop"])           # 16-bit, fp32 with two pairs, fp32 with a hop that divides nothing
def test_streamed_stats_equal_the_stats_of_the_converted_floats(gpu, name, chunk):
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case(name)
    W, hop, fb = cfg["window_size"], cfg["hop"], channels * BYTES[fmt]
    rng = np.random.default_rng(len(name) + chunk + 1)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
    for k in sorted({1, 2, 5, F, F + 3}):
        image, stats, means = _want(name, k)
        for slab in (0, 3):
            s.set_option(api.OPT_OVERVIEW_SLAB, slab)
            modes = ["one feed", "random feeds", "random feeds, then an empty flushing feed"] + (["one-sample feeds"] if k == 5 and slab == 3 and name == "w64" else [])
            for mode in modes:
                s.reset()
                sizes = [n] if mode == "one feed" else [1] * n if mode == "one-sample feeds" else _feed_sizes(rng, n, W, hop)
                got = _run(s, raw, fb, sizes, k, mode != "random feeds, then an empty flushing feed", W, hop)
                what = (name, chunk, k, slab, mode, sizes if len(sizes) < 100 else len(sizes))
                assert osr.same(got[1], stats), what
                assert np.array_equal(got[2], means) and np.array_equal(got[0], image), what
                assert s.open_frames() == 0
    s.close()


def test_the_kinds_do_not_mix_and_a_later_feed_is_unchanged(gpu):
    name = "w256_two_pairs"
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case(name)
    W, hop, P, Cn, fb = cfg["window_size"], cfg["hop"], cfg["axis_points"], cfg["num_pairs"], channels * BYTES[fmt]
    k = 5
    image, stats, means = _want(name, k)
    peak_image, peak_v, _ = plan.overview(planar, k, want_peaks=True)
    E = api.SGZ_EINVAL
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    first = W + 11 * hop + 17                                        # 12 frames: two columns and two frames open
    rest = n - first
    big = np.zeros((F, P, 4), np.uint8)
    big_r = np.zeros((F, Cn, P), api.OVERVIEW_STAT_DTYPE)
    big_v = np.zeros((F, Cn, P), np.float32)
    # refusals of the call itself: nothing consumed
    assert s.feed_overview_stats_into(raw, first, 0, False, big, big_r, big_v, F)[0] == E                  # k == 0
    assert s.feed_overview_stats_into(raw, first, k, False, None, None, None, F)[0] == E                   # all outputs NULL
    assert s.feed_overview_stats_into(None, first, k, False, big, big_r, big_v, F)[0] == E                 # a null pcm
    st, c, _ = s.feed_overview_stats_into(raw, first, k, False, big, big_r, big_v, 1)                      # a capacity below the need
    assert st == E and c == 2 and s.open_frames() == 0 and s.frames_for(first) == 12
    # a stats column open: a peak-hold feed is refused, says why and consumes nothing; so are the plain feed and another k
    a = s.feed_overview_stats(raw[:first * fb], k, want_means=True)
    assert a[0].shape[0] == 2 and s.open_frames() == 2 and s.columns_for(rest, k, True) == stats.shape[0] - 2
    st, c, _ = s.feed_overview_into(raw[first * fb:], rest, k, True, big, big_v, F)
    assert st == E and "mean overview" in api.lib().sgz_last_error().decode()
    assert s.feed_overview_into(None, 0, k, True, big, big_v, F)[0] == E                                   # ... not even its flush
    assert s.feed_into(raw[first * fb:], rest, big, None, F)[0] == E
    assert s.feed_overview_stats_into(raw[first * fb:], rest, k + 1, True, big, big_r, big_v, F)[0] == E
    assert not big.any() and not big_v.any() and not big_r.view(np.uint8).any()
    assert s.open_frames() == 2 and s.frames_for(rest) == F - 12
    b = s.feed_overview_stats(raw[first * fb:], k, flush=True, want_means=True)
    assert np.array_equal(np.concatenate([a[0], b[0]]), image) and osr.same(np.concatenate([a[1], b[1]]), stats)
    assert np.array_equal(np.concatenate([a[2], b[2]]).view(np.uint32), means) and s.open_frames() == 0
    # the reverse: a peak-hold column open, a stats feed is refused and consumes nothing
    s.reset()
    pa, va, _ = s.feed_overview(raw[:first * fb], k, want_peaks=True)
    assert s.open_frames() == 2
    st, c, _ = s.feed_overview_stats_into(raw[first * fb:], rest, k, True, big, big_r, big_v, F)
    assert st == E and "peak-hold" in api.lib().sgz_last_error().decode() and not big.any() and not big_r.view(np.uint8).any() and s.open_frames() == 2
    assert s.feed_overview_stats_into(None, 0, k, True, big, big_r, big_v, F)[0] == E
    pb, vb, _ = s.feed_overview(raw[first * fb:], k, flush=True, want_peaks=True)
    assert np.array_equal(np.concatenate([pa, pb]), peak_image) and np.array_equal(np.concatenate([va, vb]).view(np.uint32), peak_v.view(np.uint32))
    # reset drops an open stats column: either kind and any k is taken afterwards
    s.reset()
    s.feed_overview_stats(raw[:first * fb], k)
    assert s.open_frames() == 2
    s.reset()
    assert s.open_frames() == 0 and s.columns_for(W, 7, True) == 1
    pc, vc, _ = s.feed_overview(raw, k, flush=True, want_peaks=True)
    assert np.array_equal(pc, peak_image) and np.array_equal(vc.view(np.uint32), peak_v.view(np.uint32))
    # the image and lines of a plain feed behind flushed stats feeds are those of a stream that never ran one (the decay state went through both)
    half = (n // 2) * fb
    s.reset()
    fresh = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    s.feed_overview_stats(raw[:half], 3, flush=True)
    fresh.feed(raw[:half])
    got_image, got_lines, _ = s.feed(raw[half:], want_lines=True)
    want_image, want_lines, _ = fresh.feed(raw[half:], want_lines=True)
    assert got_image.shape[0] > 0 and np.array_equal(got_image, want_image) and np.array_equal(got_lines.view(np.uint32), want_lines.view(np.uint32))
    s.close(); fresh.close()


@pytest.mark.parametrize("name", ["w64", "w256_two_pairs"])
def test_armed_lanes_return_what_they_return_under_a_peak_hold_feed(gpu, name):
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case(name)
    W, hop, fb = cfg["window_size"], cfg["hop"], channels * BYTES[fmt]
    k, m = 3, 100
    image, stats, means = _want(name, k)
    nch = 2 * cfg["num_pairs"]
    results = []
    for kind in ("peak hold", "stats"):
        rng = np.random.default_rng(5)
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1500)
        s.set_option(api.OPT_OVERVIEW_SLAB, 4)
        wave = np.zeros((n // m + 2, nch, 2), np.float32)
        track = np.zeros((F, cfg["num_pairs"], 6), np.float64)
        s.set_waveform(m, wave)
        s.set_track(0, 0.4, track)
        sizes = _feed_sizes(rng, n, W, hop)
        at, cols = 0, []
        for i, size in enumerate(sizes):
            piece, flush = (raw[at * fb:(at + size) * fb] if size else None), i == len(sizes) - 1
            out = s.feed_overview(piece, k, flush=flush, nsamples=size) if kind == "peak hold" else s.feed_overview_stats(piece, k, flush=flush, nsamples=size)
            cols.append(out[1] if kind == "stats" else None)
            at += size
        s.flush_waveform()
        written, _ = s.waveform_state()
        assert s.track_state() == F and written == -(-n // m)
        if kind == "stats":
            assert osr.same(np.concatenate(cols), stats)
        results.append((wave[:written].copy(), track.copy()))
        s.close()
    assert np.array_equal(results[0][0].view(np.uint32), results[1][0].view(np.uint32))
    assert np.array_equal(results[0][1].view(np.uint64), results[1][1].view(np.uint64)) and results[0][1].any()


def test_pinned_outputs_and_the_one_shot_call(gpu):
    import torch
    name = "w256_two_pairs"
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case(name)
    W, fb = cfg["window_size"], channels * BYTES[fmt]
    for k in (2, 7):
        image, stats, means = _want(name, k)
        cols = image.shape[0]
        pcm = torch.from_numpy(raw.copy()).pin_memory()
        out = torch.zeros(image.shape, dtype=torch.uint8).pin_memory()
        out_r = torch.zeros((*stats.shape, 3), dtype=torch.int64).pin_memory()
        out_m = torch.zeros(means.shape, dtype=torch.float32).pin_memory()
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=5000)
        st, c, t = s.feed_overview_stats_into(pcm, n, k, True, out, out_r, out_m, cols)
        assert st == api.SGZ_OK and c == cols == t.frames and t.chunks == -(-n // 5000)
        assert np.array_equal(out.numpy(), image) and np.array_equal(out_m.numpy().view(np.uint32), means), k
        assert osr.same(out_r.numpy().view(api.OVERVIEW_STAT_DTYPE).reshape(stats.shape), stats), k
        # one output alone: the others are not touched
        s.reset()
        out.zero_(); out_r.zero_()
        st, c, _ = s.feed_overview_stats_into(pcm, n, k, True, None, None, out_m, cols)
        assert st == api.SGZ_OK and np.array_equal(out_m.numpy().view(np.uint32), means) and not out.any() and not out_r.any()
        s.close()
        st, a, r, v, t = api.overview_stats_pcm(cfg, raw, fmt, channels, k, cmap, want_means=True)
        assert st == api.SGZ_OK and t["chunks"] == 1 and t["frames"] == cols
        assert np.array_equal(a, image) and osr.same(r, stats) and np.array_equal(v.view(np.uint32), means), k
    st, a, r, v, _ = api.overview_stats_pcm(cfg, raw[:(W - 1) * fb], fmt, channels, 2, cmap, want_means=True)
    assert st == api.SGZ_SKIPPED_FRAME and a.shape[0] == 0 and r.shape[0] == 0 and v.shape[0] == 0
