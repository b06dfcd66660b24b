"""The cross overview inside the PCM stream on the GPU (sgz_pcm_stream_set_cross_edges, sgz_pcm_stream_feed_overview_cross,
sgz_spectrogram_overview_cross_pcm; csrc/pcm.hip, the slab loop in csrc/api.hip): 16-bit and fp32 interleaved PCM, 2 source channels and 4
with a channel map, Phase mode, window 64, hop 16, 2000 sample frames.

Byte for byte, no tolerance: the columns of all cross feeds of a stream, of which only the last flushes, concatenated ==
Plan.overview_cross (sgz_spectrogram_overview_cross_host) of the numpy-converted planar floats, for every way of cutting the stream into
feeds of a seeded list (pieces shorter than a hop among them), small chunk_samples, slab 3 and a flush with no new samples; that reference
in turn == the restatement (tests/overview_cross_ref.py) on Plan.stage_bins.  The four kinds of open column refuse one another with their
texts and consume nothing; edges set with a cross column open, the track lane armed and a stream of another mode are refused; a plain feed
and a power feed on a reset stream behave as before."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_ref as ov  # noqa: E402
import overview_cross_ref as ocr  # noqa: E402
from test_gpu_pcm import BYTES, convert_ref, to_bytes  # noqa: E402
from test_gpu_pcm_overview import _feed_sizes  # noqa: E402

pytestmark = pytest.mark.gpu

FRAMES = 122                                                 # 64 + 16 * 121 = 2000 sample frames
N = 64
EDGES = [1, 2, 3, 5, 8, 8, 13, 21, 31]
CASES = {"s16x2": (api.PCM_S16, 2, None, 1), "f32x2": (api.PCM_F32, 2, None, 1), "s16x4": (api.PCM_S16, 4, [2, 0], 1),
         "f32x4": (api.PCM_F32, 4, [3, 1, 0, 2], 2)}
_made, _wants = {}, {}


def _cfg(pairs, **over):
    return config.spectrum_config(**{**dict(window_size=N, hop=16, axis_points=33, num_pairs=pairs, channel_mode=config.CH_PHASE,
                                            bin_interp=config.INTERP_LINEAR), **over})


def _case(name, gpu):
    """(cfg, format, source channels, map, PCM bytes, samples, plan, the converted and mapped planar floats) -- once per case"""
    if name not in _made:
        fmt, src, cmap, pairs = CASES[name]
        cfg = _cfg(pairs)
        x = ov.burst_signal(cfg["window_size"], cfg["hop"], FRAMES, src, cfg["sample_rate"], seed=3 + fmt + src)
        x[1] = 0.5 * x[0] + 0.5 * x[1]                       # related channels: a coherence that is neither 0 nor 1
        inter = np.ascontiguousarray(x.T).reshape(-1)
        raw = to_bytes(np.clip(np.round(inter.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int64), fmt) if fmt == api.PCM_S16 else to_bytes(inter, fmt)
        planar = np.ascontiguousarray(convert_ref(raw, fmt, src))
        planar = np.ascontiguousarray(planar[cmap]) if cmap is not None else planar
        plan = api.Plan(cfg).upload()
        plan.set_cross_edges(EDGES)
        assert x.shape[1] == 2000 and plan.num_frames(2000) == FRAMES and planar.shape == (2 * pairs, 2000)
        for a in (raw, planar):
            a.setflags(write=False)
        _made[name] = (cfg, fmt, src, cmap, raw, 2000, plan, planar)
    return _made[name]


def _want(name, k, gpu):
    """Plan.overview_cross of the converted floats at k -- held to the restatement on stage_bins once"""
    if (name, k) not in _wants:
        import torch
        cfg, fmt, src, cmap, raw, n, plan, planar = _case(name, gpu)
        cross, _ = plan.overview_cross(planar, k)
        bins = plan.stage_bins(torch.from_numpy(planar.copy()).to(gpu)).cpu().numpy()
        assert ocr.same(cross, ocr.columns_of(ocr.records_of(bins, N, EDGES), k)[0])
        assert int(cross["count"].sum()) == FRAMES * cross.shape[1] * (EDGES[-1] - EDGES[0])
        _wants[name, k] = cross
    return _wants[name, k]


def _run(s, raw, fb, sizes, k, last_flushes, W, hop):
    """feeds the sizes in turn (the last one flushing, or an empty flushing feed behind them); checks columns_for and open_frames around every
    feed against sgz_stream_step / sgz_overview_step chained; -> the records of all feeds"""
    cross, at, held, open_frames = [], 0, 0, 0
    feeds = [(size, last_flushes and i == len(sizes) - 1) for i, size in enumerate(sizes)] + ([] if last_flushes else [(0, True)])
    for size, flush in feeds:
        frames, held = api.stream_step(W, hop, held, size)
        columns, open_frames = api.overview_step(k, open_frames, frames, flush)
        assert s.columns_for(size, k, flush) == columns
        r, t = s.feed_overview_cross(raw[at * fb:(at + size) * fb] if size else None, k, flush=flush, nsamples=size)
        assert r.shape[0] == columns == t["frames"] and s.open_frames() == open_frames, (size, flush, columns)
        cross.append(r)
        at += size
    return np.concatenate(cross)


@pytest.mark.parametrize("name", list(CASES))
def test_streamed_cross_equals_the_cross_of_the_converted_floats(gpu, name):
    cfg, fmt, src, cmap, raw, n, plan, planar = _case(name, gpu)
    W, hop, fb = cfg["window_size"], cfg["hop"], src * BYTES[fmt]
    rng = np.random.default_rng(11 + fmt + src)
    for chunk in (100, 0):                                   # pieces of 100 samples: about six frames each; and the default
        s = api.PcmStream(cfg, fmt, src, cmap, chunk_samples=chunk)
        s.set_cross_edges(EDGES)
        for k in (1, 4, 7, FRAMES + 3):
            want = _want(name, k, gpu)
            for slab in (0, 3):
                s.set_option(api.OPT_OVERVIEW_SLAB, slab)
                for mode in ("one feed", "seeded feeds", "seeded feeds, then an empty flushing feed"):
                    s.reset()
                    sizes = [n] if mode == "one feed" else _feed_sizes(rng, n, W, hop)
                    got = _run(s, raw, fb, sizes, k, mode != "seeded feeds, then an empty flushing feed", W, hop)
                    assert ocr.same(got, want), (name, chunk, k, slab, mode, sizes)
                    assert s.open_frames() == 0
        s.close()
    # the one-shot call equals the stream; fewer samples than a window: skipped
    for k in (2, 7):
        st, r, t = api.overview_cross_pcm(cfg, raw, fmt, src, EDGES, k, channel_map=cmap)
        assert st == api.SGZ_OK and t["frames"] == r.shape[0] and ocr.same(r, _want(name, k, gpu)), k
    st, r, _ = api.overview_cross_pcm(cfg, raw[:(W - 1) * fb], fmt, src, EDGES, 2, channel_map=cmap)
    assert st == api.SGZ_SKIPPED_FRAME and r.shape[0] == 0
    # the readout of the whole file's fold: related channels, a coherence strictly inside (0, 1) somewhere
    whole = api.overview_cross_readout(api.overview_cross_fold(_want(name, 1, gpu), 1))
    assert np.isnan(whole["ll"][0, :, 4]).all()              # the empty band
    coherence = whole["coherence"][0][:, [0, 1, 2, 3, 5, 6, 7]]
    assert ((coherence >= 0) & (coherence <= 1)).all()


def test_the_four_kinds_refuse_one_another(gpu):
    name = "f32x2"
    cfg, fmt, src, cmap, raw, n, plan, planar = _case(name, gpu)
    W, hop, P, fb = cfg["window_size"], cfg["hop"], cfg["axis_points"], src * BYTES[fmt]
    k = 5
    want = _want(name, k, gpu)
    B = len(EDGES) - 1
    E, L = api.SGZ_EINVAL, api.lib()
    s = api.PcmStream(cfg, fmt, src, cmap, chunk_samples=300)
    first = W + 11 * hop + 7                                         # 12 frames: two columns and two frames open
    rest = n - first
    F = FRAMES
    big = np.zeros((F, P, 4), np.uint8)
    big_c = np.zeros((F, 1, B), api.OVERVIEW_CROSS_DTYPE)
    big_r = np.zeros((F, 1, P), api.OVERVIEW_STAT_DTYPE)
    big_v = np.zeros((F, 1, 2, P), np.float32)

    def err():
        return L.sgz_last_error().decode()

    def untouched():
        return not big.any() and not big_v.any() and not big_c.view(np.uint8).any() and not big_r.view(np.uint8).any()

    # a stream without a band table; then the call's own refusals: nothing consumed
    assert s.feed_overview_cross_into(raw, first, k, False, big_c, F)[0] == E and "sgz_pcm_stream_set_cross_edges" in err()
    s.set_cross_edges(EDGES)
    assert s.feed_overview_cross_into(raw, first, 0, False, big_c, F)[0] == E                             # k == 0
    assert s.feed_overview_cross_into(raw, first, k, False, None, F)[0] == E                              # columns close and no output
    assert s.feed_overview_cross_into(None, first, k, False, big_c, F)[0] == E                            # a null pcm
    st, c, _ = s.feed_overview_cross_into(raw, first, k, False, big_c, 1)                                 # a capacity below the need
    assert st == E and c == 2 and s.open_frames() == 0 and s.frames_for(first) == 12 and untouched()
    # a cross column open: the three other kinds and the plain feed are refused, name the flush call and consume nothing; so are another
    # k and new edges
    a, _ = s.feed_overview_cross(raw[:first * fb], k)
    assert a.shape[0] == 2 and s.open_frames() == 2 and s.columns_for(rest, k, True) == want.shape[0] - 2
    call = "flush it (sgz_pcm_stream_feed_overview_cross)"
    assert s.feed_overview_into(raw[first * fb:], rest, k, True, big, big_v, F)[0] == E and "cross overview's" in err() and call in err()
    assert s.feed_overview_into(None, 0, k, True, big, big_v, F)[0] == E                                   # ... not even its flush
    assert s.feed_overview_stats_into(raw[first * fb:], rest, k, True, big, big_r, big_v, F)[0] == E and "cross overview's" in err() and call in err()
    assert s.feed_overview_power_into(raw[first * fb:], rest, k, True, big, None, big_v, F)[0] == api.SGZ_EUNSUPPORTED     # (a Phase stream)
    assert s.feed_into(raw[first * fb:], rest, big, None, F)[0] == E and "a cross overview's column is open" in err() and call in err()
    assert s.feed_overview_cross_into(raw[first * fb:], rest, k + 1, True, big_c, F)[0] == E
    edges = np.array([1, 31], np.uint32)
    assert L.sgz_pcm_stream_set_cross_edges(s.h, edges.ctypes.data, 1) == E and "column is open" in err()
    assert untouched() and s.open_frames() == 2 and s.frames_for(rest) == F - 12
    b, _ = s.feed_overview_cross(raw[first * fb:], k, flush=True)
    assert ocr.same(np.concatenate([a, b]), want) and s.open_frames() == 0
    # a peak-hold column open, then a mean overview's: a cross feed is refused, names their flush calls and consumes nothing
    for kind, call in (("peak-hold", "sgz_pcm_stream_feed_overview)"), ("mean overview", "sgz_pcm_stream_feed_overview_stats)")):
        s.reset()
        if kind == "peak-hold":
            s.feed_overview(raw[:first * fb], k)
        else:
            s.feed_overview_stats(raw[:first * fb], k)
        assert s.open_frames() == 2
        st, c, _ = s.feed_overview_cross_into(raw[first * fb:], rest, k, True, big_c, F)
        assert st == E and kind in err() and call in err() and untouched() and s.open_frames() == 2 and s.frames_for(rest) == F - 12
        assert s.feed_overview_cross_into(None, 0, k, True, big_c, F)[0] == E
    # reset drops an open cross column: any kind, any k and new edges are taken afterwards; a plain feed behaves as before
    s.reset()
    s.feed_overview_cross(raw[:first * fb], k)
    assert s.open_frames() == 2
    s.reset()
    assert s.open_frames() == 0 and s.columns_for(W, 7, True) == 1
    s.set_cross_edges([1, 31])
    s.set_cross_edges(EDGES)
    image, _, _ = s.feed(raw)
    fresh = api.PcmStream(cfg, fmt, src, cmap, chunk_samples=300)
    assert image.shape[0] == F and np.array_equal(image, fresh.feed(raw)[0])
    fresh.close()
    # the track lane armed: refused, nothing consumed; disarmed, the feed is taken
    s.reset()
    track = np.zeros((F, 1, 6), np.float64)
    s.set_track(0, 0.4, track)
    st, c, _ = s.feed_overview_cross_into(raw, n, k, True, big_c, F)
    assert st == E and "track lane" in err() and untouched() and s.frames_for(n) == F and not track.any()
    s.set_track(0, 0.4, None)
    got, _ = s.feed_overview_cross(raw, k, flush=True)
    assert ocr.same(got, want)
    s.close()


def test_a_plain_feed_and_a_power_feed_on_a_reset_stream_behave_as_before(gpu):
    """a Separate stream that has refused the cross calls: its plain feed and its power feed give the bytes of a stream that never saw them"""
    cfg = config.spectrum_config(window_size=N, hop=16, axis_points=33)
    x = ov.burst_signal(N, 16, FRAMES, 2, cfg["sample_rate"], seed=9)
    raw = to_bytes(np.ascontiguousarray(x.T).reshape(-1), api.PCM_F32)
    results = []
    for touched in (False, True):
        s = api.PcmStream(cfg, api.PCM_F32, 2, None, chunk_samples=300)
        if touched:
            edges = np.array(EDGES, np.uint32)
            big_c = np.zeros((FRAMES, 1, len(EDGES) - 1), api.OVERVIEW_CROSS_DTYPE)
            assert api.lib().sgz_pcm_stream_set_cross_edges(s.h, edges.ctypes.data, len(EDGES) - 1) == api.SGZ_EUNSUPPORTED
            assert s.feed_overview_cross_into(raw, 2000, 4, True, big_c, FRAMES)[0] == api.SGZ_EUNSUPPORTED
            assert not big_c.view(np.uint8).any() and s.frames_for(2000) == FRAMES and s.open_frames() == 0
            s.reset()
        image, lines, _ = s.feed(raw, want_lines=True)
        s.reset()
        rgba, power, levels, _ = s.feed_overview_power(raw, 4, flush=True, want_levels=True)
        results.append((image, lines, rgba, power, levels))
        s.close()
    for a, b in zip(*results):
        assert a.shape[0] > 0 and a.tobytes() == b.tobytes()
    with pytest.raises(api.SgzError) as refused:
        api.overview_cross_pcm(cfg, raw, api.PCM_F32, 2, EDGES, 4)
    assert refused.value.status == api.SGZ_EUNSUPPORTED


def test_pinned_output(gpu):
    import torch
    name = "s16x4"
    cfg, fmt, src, cmap, raw, n, plan, planar = _case(name, gpu)
    k = 3
    want = _want(name, k, gpu)
    cols = want.shape[0]
    pcm = torch.from_numpy(raw.copy()).pin_memory()
    out = torch.zeros((*want.shape, 10), dtype=torch.int64).pin_memory()
    s = api.PcmStream(cfg, fmt, src, cmap, chunk_samples=500)
    s.set_cross_edges(EDGES)
    st, c, t = s.feed_overview_cross_into(pcm, n, k, True, out, cols)
    assert st == api.SGZ_OK and c == cols == t.frames and t.chunks == -(-n // 500)
    assert ocr.same(out.numpy().view(api.OVERVIEW_CROSS_DTYPE).reshape(want.shape), want)
    s.close()
