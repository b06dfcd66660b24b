"""The percentile overview inside the PCM stream on the GPU (sgz_pcm_stream_feed_overview_pct, sgz_spectrogram_overview_pct_pcm; csrc/pcm.hip,
the slab loop in csrc/api.hip).

Byte for byte -- image, records and value planes --, no tolerance: the columns of all percentile feeds of a stream, of which only the last
flushes, concatenated == Plan.overview_pct (sgz_spectrogram_overview_pct_host) of the numpy-converted planar floats, for 16-bit and fp32 PCM
(the fp32 case maps a subset of the source channels), arbitrary cuts of the stream into feeds, two chunk_samples and two
SGZ_OPT_OVERVIEW_SLAB; that reference in turn == tests/overview_pct_ref.py on sgz_spectrogram_render_host's line results.  The one-shot call
gives the same bytes.  A column is of one kind: the new refusals are held word for word and consume nothing; armed waveform and track
lanes return what they return under a peak-hold feed.  The cases and the feed cutter are those of tests/test_gpu_pcm_overview.py."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_pct_ref as opr  # noqa: E402
import overview_ref as ov  # noqa: E402
from test_gpu_pcm import BYTES  # noqa: E402
from test_gpu_pcm_overview import _case, _feed_sizes  # noqa: E402

pytestmark = pytest.mark.gpu

Q = [0.5, 0.1, 1.0]
_wants = {}


def _want(name, k):
    """Plan.overview_pct of the converted floats at k: (image, records, value bits [nq][columns][pairs][P]) -- held to the restatement once"""
    if (name, k) not in _wants:
        from oracle import pyoracle as po
        cfg, plan, planar, main = _case(name)[0], _case(name)[7], _case(name)[8], _case(name)[10]
        image, records, values, _ = plan.overview_pct(planar, k, Q, want_records=True, want_values=True)
        want = opr.columns_of(main, k)[0]
        bits = opr.quantile_bits(want, Q)
        assert opr.same(records, want) and np.array_equal(values.view(np.uint32), bits)
        assert np.array_equal(image, ov.blend(po, po.params_from_dict(cfg), bits[0]))
        _wants[name, k] = (image, records, bits)
    return _wants[name, k]


def _run(s, raw, fb, sizes, k, last_flushes, W, hop):
    """feeds the sizes in turn (the last one flushing, or an empty flushing feed behind them) -> (image, records, value bits) of all feeds"""
    images, records, values, at, held, open_frames = [], [], [], 0, 0, 0
    feeds = [(size, last_flushes and i == len(sizes) - 1) for i, size in enumerate(sizes)] + ([] if last_flushes else [(0, True)])
    for size, flush in feeds:
        frames, held = api.stream_step(W, hop, held, size)
        columns, open_frames = api.overview_step(k, open_frames, frames, flush)
        assert s.columns_for(size, k, flush) == columns
        image, r, v, t = s.feed_overview_pct(raw[at * fb:(at + size) * fb] if size else None, k, Q, flush=flush, nsamples=size, want_values=True)
        assert image.shape[0] == r.shape[0] == v.shape[1] == columns == t["frames"] and v.shape[0] == len(Q) and s.open_frames() == open_frames
        images.append(image); records.append(r); values.append(v.view(np.uint32))
        at += size
    return np.concatenate(images), np.concatenate(records), np.concatenate(values, axis=1)


@pytest.mark.parametrize("chunk", [1000, 0])
@pytest.mark.parametrize("name", ["w64", "w256_two_pairs"])                      # 16-bit; fp32 with two pairs from a subset of the channels
def test_streamed_pct_equals_the_pct_of_the_converted_floats(gpu, name, chunk):
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case(name)
    W, hop, fb = cfg["window_size"], cfg["hop"], channels * BYTES[fmt]
    rng = np.random.default_rng(len(name) + chunk + 2)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=chunk)
    for k in sorted({1, 5, F + 3}):
        image, records, bits = _want(name, k)
        for slab in (0, 3):
            s.set_option(api.OPT_OVERVIEW_SLAB, slab)
            for mode in ("one feed", "random feeds", "random feeds, then an empty flushing feed"):
                s.reset()
                sizes = [n] if mode == "one feed" else _feed_sizes(rng, n, W, hop)
                got = _run(s, raw, fb, sizes, k, mode != "random feeds, then an empty flushing feed", W, hop)
                what = (name, chunk, k, slab, mode, sizes)
                assert opr.same(got[1], records), what
                assert np.array_equal(got[2], bits) and np.array_equal(got[0], image), what
                assert s.open_frames() == 0
    s.close()


def test_the_one_shot_call_and_a_capacity_above_the_need(gpu):
    name = "w256_two_pairs"
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case(name)
    W, P, Cn, fb = cfg["window_size"], cfg["axis_points"], cfg["num_pairs"], channels * BYTES[fmt]
    for k in (2, 7):
        image, records, bits = _want(name, k)
        cols = image.shape[0]
        st, a, r, v, t = api.overview_pct_pcm(cfg, raw, fmt, channels, k, Q, cmap, want_values=True)
        assert st == api.SGZ_OK and t["chunks"] == 1 and t["frames"] == cols
        assert np.array_equal(a, image) and opr.same(r, records) and np.array_equal(v.view(np.uint32), bits), k
        # value plane j starts at j * capacity_columns * pairs * P: a capacity above the need leaves the rest of every plane alone
        cap = cols + 3
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=5000)
        big_v = np.full((len(Q), cap, Cn, P), 0x5A5AA5A5, np.uint32)
        st, c, _ = s.feed_overview_pct_into(raw, n, k, True, Q, None, None, big_v, cap)
        assert st == api.SGZ_OK and c == cols
        assert np.array_equal(big_v[:, :cols], bits) and (big_v[:, cols:] == 0x5A5AA5A5).all(), k
        s.close()
    st, a, r, v, _ = api.overview_pct_pcm(cfg, raw[:(W - 1) * fb], fmt, channels, 2, Q, cmap, want_values=True)
    assert st == api.SGZ_SKIPPED_FRAME and a.shape[0] == 0 and r.shape[0] == 0 and v.shape[1] == 0


def test_the_open_column_refusals_word_for_word(gpu):
    name = "w256_two_pairs"
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case(name)
    W, hop, P, Cn, fb = cfg["window_size"], cfg["hop"], cfg["axis_points"], cfg["num_pairs"], channels * BYTES[fmt]
    k = 5
    image, records, bits = _want(name, k)
    E = api.SGZ_EINVAL
    tail = " -- flush it (sgz_pcm_stream_feed_overview_pct) or reset the stream first"
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
    first = W + 11 * hop + 17                                        # 12 frames: two columns and two frames open
    rest = n - first
    big = np.zeros((F, P, 4), np.uint8)
    big_r = np.zeros((F, Cn, P), api.OVERVIEW_PCT_DTYPE)
    big_s = np.zeros((F, Cn, P), api.OVERVIEW_STAT_DTYPE)
    big_v = np.zeros((len(Q), F, Cn, P), np.float32)

    def err():
        return api.lib().sgz_last_error().decode()
    # refusals of the call itself: nothing consumed
    assert s.feed_overview_pct_into(raw, first, 0, False, Q, big, big_r, big_v, F)[0] == E                 # k == 0
    assert s.feed_overview_pct_into(raw, first, k, False, Q, None, None, None, F)[0] == E                  # all outputs NULL
    assert s.feed_overview_pct_into(None, first, k, False, Q, big, big_r, big_v, F)[0] == E                # a null pcm
    assert s.feed_overview_pct_into(raw, first, k, False, [0.5, 1.5], big, big_r, big_v, F)[0] == E        # a quantile outside [0, 1]
    st, c, _ = s.feed_overview_pct_into(raw, first, k, False, Q, big, big_r, big_v, 1)                     # a capacity below the need
    assert st == E and c == 2 and s.open_frames() == 0 and s.frames_for(first) == 12
    # a percentile column open: every other kind's feed is refused in the established wording and consumes nothing
    a = s.feed_overview_pct(raw[:first * fb], k, Q, want_values=True)
    assert a[0].shape[0] == 2 and s.open_frames() == 2 and s.columns_for(rest, k, True) == records.shape[0] - 2
    piece = raw[first * fb:]
    assert s.feed_overview_into(piece, rest, k, True, big, big_v[0], F)[0] == E
    assert err() == "sgz_pcm_stream_feed_overview: the open column is a percentile overview's" + tail
    assert s.feed_overview_stats_into(piece, rest, k, True, big, big_s, big_v[0], F)[0] == E
    assert err() == "sgz_pcm_stream_feed_overview_stats: the open column is a percentile overview's" + tail
    assert s.feed_overview_into(None, 0, k, True, big, big_v[0], F)[0] == E                                # ... not even its flush
    assert s.feed_into(piece, rest, big, None, F)[0] == E and "a percentile overview's column is open" + tail in err()
    assert s.feed_overview_pct_into(piece, rest, k + 1, True, Q, big, big_r, big_v, F)[0] == E
    assert err() == "sgz_pcm_stream_feed_overview_pct: k differs from the open column's -- flush or reset first"
    assert not big.any() and not big_v.any() and not big_r.view(np.uint8).any() and not big_s.view(np.uint8).any()
    assert s.open_frames() == 2 and s.frames_for(rest) == F - 12
    b = s.feed_overview_pct(piece, k, Q, flush=True, want_values=True)
    assert np.array_equal(np.concatenate([a[0], b[0]]), image) and opr.same(np.concatenate([a[1], b[1]]), records)
    assert np.array_equal(np.concatenate([a[2], b[2]], axis=1).view(np.uint32), bits) and s.open_frames() == 0
    # the reverse: a mean overview's column open, a percentile feed is refused and consumes nothing
    s.reset()
    s.feed_overview_stats(raw[:first * fb], k)
    assert s.open_frames() == 2
    assert s.feed_overview_pct_into(piece, rest, k, True, Q, big, big_r, big_v, F)[0] == E
    assert err() == "sgz_pcm_stream_feed_overview_pct: the open column is a mean overview's -- flush it (sgz_pcm_stream_feed_overview_stats) or reset the stream first"
    assert not big.any() and not big_r.view(np.uint8).any() and s.open_frames() == 2
    # reset drops an open percentile column: any kind and any k is taken afterwards
    s.reset()
    s.feed_overview_pct(raw[:first * fb], k, Q)
    assert s.open_frames() == 2
    s.reset()
    assert s.open_frames() == 0
    got = s.feed_overview_pct(raw, 7, Q, flush=True, want_values=True)
    assert opr.same(got[1], _want(name, 7)[1]) and np.array_equal(got[2].view(np.uint32), _want(name, 7)[2])
    s.close()


@pytest.mark.parametrize("name", ["w64", "w256_two_pairs"])
def test_armed_lanes_return_what_they_return_under_a_peak_hold_feed(gpu, name):
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case(name)
    W, hop, fb = cfg["window_size"], cfg["hop"], channels * BYTES[fmt]
    k, m = 3, 100
    image, records, bits = _want(name, k)
    nch = 2 * cfg["num_pairs"]
    results = []
    for kind in ("peak hold", "pct"):
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
            out = s.feed_overview(piece, k, flush=flush, nsamples=size) if kind == "peak hold" else s.feed_overview_pct(piece, k, Q, flush=flush, nsamples=size)
            cols.append(out[1] if kind == "pct" else None)
            at += size
        s.flush_waveform()
        written, _ = s.waveform_state()
        assert s.track_state() == F and written == -(-n // m)
        if kind == "pct":
            assert opr.same(np.concatenate(cols), records)
        results.append((wave[:written].copy(), track.copy()))
        s.close()
    assert np.array_equal(results[0][0].view(np.uint32), results[1][0].view(np.uint32))
    assert np.array_equal(results[0][1].view(np.uint64), results[1][1].view(np.uint64)) and results[0][1].any()
