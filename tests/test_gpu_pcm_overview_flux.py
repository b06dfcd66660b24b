"""The flux overview inside the PCM stream on the GPU (sgz_pcm_stream_feed_overview_flux, sgz_spectrogram_overview_flux_pcm; csrc/pcm.hip, the
slab loop in csrc/api.hip): 16-bit and fp32 stereo, window 64, hop 16, P 33, 2000 sample frames.

Byte for byte, no tolerance: the columns of all flux feeds of a stream, of which only the last flushes, concatenated == Plan.overview_flux
(sgz_spectrogram_overview_flux_host) of the numpy-converted planar floats -- for one feed, feeds of one sample, feeds that end in the middle
of a frame and of a column, seeded feeds, small chunk_samples, slab 3 and a flush with no new samples; that reference in turn == the
restatement (tests/overview_flux_ref.py) on Plan.stage_mapped.  A plain feed between two flux feeds resets the predecessor as sgz.h says and
the frames go on counting.  The five kinds of open column refuse one another with their message and consume nothing; the track lane armed is
refused; an armed waveform lane returns its usual bytes; columns_for / open_frames / reset serve the kind; the one-shot call equals the
stream."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_ref as ov  # noqa: E402
import overview_flux_ref as ofr  # noqa: E402
from test_gpu_pcm import BYTES, convert_ref, to_bytes  # noqa: E402
from test_gpu_pcm_overview import _feed_sizes  # noqa: E402

pytestmark = pytest.mark.gpu

FRAMES = 122                                                 # 64 + 16 * 121 = 2000 sample frames
CFG = dict(window_size=64, hop=16, axis_points=33)
FORMATS = {"s16": api.PCM_S16, "f32": api.PCM_F32}
_made, _wants = {}, {}


def _same(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _case(name, gpu):
    """(cfg, format, PCM bytes, samples, plan, planar floats, stage_mapped of them [F][rows][P]) -- once per format"""
    if name not in _made:
        import torch
        fmt = FORMATS[name]
        cfg = config.spectrum_config(**CFG)
        x = ov.burst_signal(cfg["window_size"], cfg["hop"], FRAMES, 2, cfg["sample_rate"], seed=3 + fmt)
        inter = np.ascontiguousarray(x.T).reshape(-1)
        raw = to_bytes(np.clip(np.round(inter.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int64), fmt) if fmt == api.PCM_S16 else to_bytes(inter, fmt)
        planar = np.ascontiguousarray(convert_ref(raw, fmt, 2))
        plan = api.Plan(cfg).upload()
        assert x.shape[1] == 2000 and plan.num_frames(2000) == FRAMES
        mapped = plan.stage_mapped(torch.from_numpy(planar.copy()).to(gpu)).cpu().numpy().reshape(FRAMES, 2, 33)
        for a in (raw, planar, mapped):
            a.setflags(write=False)
        _made[name] = (cfg, fmt, raw, 2000, plan, planar, mapped)
    return _made[name]


def _want(name, k, gpu):
    """Plan.overview_flux of the converted floats at k -- held to the restatement on stage_mapped once"""
    if (name, k) not in _wants:
        cfg, fmt, raw, n, plan, planar, mapped = _case(name, gpu)
        flux, _ = plan.overview_flux(planar, k)
        assert _same(flux, ofr.overview(mapped, k)[0].reshape(-1, 1, 2))
        _wants[name, k] = flux
    return _wants[name, k]


def _run(s, raw, fb, sizes, k, last_flushes, W, hop):
    """feeds the sizes in turn (the last one flushing, or an empty flushing feed behind them); checks columns_for and open_frames around every
    feed against sgz_stream_step / sgz_overview_step chained; -> the records of all feeds"""
    flux, at, held, open_frames = [], 0, 0, 0
    feeds = [(size, last_flushes and i == len(sizes) - 1) for i, size in enumerate(sizes)] + ([] if last_flushes else [(0, True)])
    for size, flush in feeds:
        frames, held = api.stream_step(W, hop, held, size)
        columns, open_frames = api.overview_step(k, open_frames, frames, flush)
        assert s.columns_for(size, k, flush) == columns
        r, t = s.feed_overview_flux(raw[at * fb:(at + size) * fb] if size else None, k, flush=flush, nsamples=size)
        assert r.shape[0] == columns == t["frames"] and s.open_frames() == open_frames, (size, flush, columns)
        flux.append(r)
        at += size
    return np.concatenate(flux)


def _cuts(n, W, hop, k):
    """ways of cutting n samples: one piece; one sample first; an end in the middle of a frame; an end in the middle of a column; ones"""
    mid_frame = W + 9 * hop + hop // 2
    mid_column = W + (min(k + k // 2 + 1, 60) - 1) * hop + 3          # that many frames: no whole number of columns for k > 1
    yield "one piece", [n]
    yield "one sample first", [1, n - 1]
    yield "mid-frame", [mid_frame, n - mid_frame]
    yield "mid-column", [mid_column, 7, n - mid_column - 7]
    yield "single samples, then the rest", [1] * (W + 2 * hop + 3) + [n - (W + 2 * hop + 3)]


@pytest.mark.parametrize("name", list(FORMATS))
def test_streamed_flux_equals_the_flux_of_the_converted_floats(gpu, name):
    cfg, fmt, raw, n, plan, planar, mapped = _case(name, gpu)
    W, hop, fb = cfg["window_size"], cfg["hop"], 2 * BYTES[fmt]
    rng = np.random.default_rng(11 + fmt)
    for chunk in (100, 0):                                   # pieces of 100 samples: about six frames each; and the default
        s = api.PcmStream(cfg, fmt, 2, None, chunk_samples=chunk)
        for k in (1, 4, 7, FRAMES + 3):
            flux = _want(name, k, gpu)
            for slab in (0, 3):
                s.set_option(api.OPT_OVERVIEW_SLAB, slab)
                modes = list(_cuts(n, W, hop, k)) + [("seeded feeds", _feed_sizes(rng, n, W, hop)), ("seeded feeds, then an empty flushing feed", _feed_sizes(rng, n, W, hop))]
                for mode, sizes in modes:
                    if mode.startswith("single") and (slab or chunk):
                        continue
                    s.reset()
                    got = _run(s, raw, fb, sizes, k, mode != "seeded feeds, then an empty flushing feed", W, hop)
                    assert _same(got, flux), (name, chunk, k, slab, mode, sizes[:8])
                    assert s.open_frames() == 0
        s.close()


def test_a_plain_feed_between_two_flux_feeds_resets_the_predecessor(gpu):
    """flux feed A, plain feed B, flux feed C: C's first frame has no predecessor (F = 0) and its frames are counted behind A's and B's; then
    reset: the frames count from 0 again and there is no predecessor"""
    name = "f32"
    cfg, fmt, raw, n, plan, planar, mapped = _case(name, gpu)
    W, hop, fb = cfg["window_size"], cfg["hop"], 2 * BYTES[fmt]
    k = 4
    s = api.PcmStream(cfg, fmt, 2, None, chunk_samples=300)
    na, nb = W + 19 * hop + 5, 30 * hop + 3
    fa = s.frames_for(na)
    a, _ = s.feed_overview_flux(raw[:na * fb], k, flush=True)
    assert fa == 20 and _same(a, ofr.overview(mapped[:fa], k)[0].reshape(-1, 1, 2))
    fb_ = s.frames_for(nb)
    s.feed(raw[na * fb:(na + nb) * fb])
    c, _ = s.feed_overview_flux(raw[(na + nb) * fb:], k, flush=True)
    fc = FRAMES - fa - fb_
    assert fb_ > 0 and fc > 10
    assert _same(c, ofr.overview(mapped[fa + fb_:], k, first_frame=fa + fb_)[0].reshape(-1, 1, 2))          # no predecessor: prev=None
    assert not _same(c, ofr.overview(mapped[fa + fb_:], k, first_frame=fa + fb_, prev=mapped[fa + fb_ - 1])[0].reshape(-1, 1, 2))
    # two flux feeds in a row keep the predecessor; an empty plain feed (no frame consumed) does not break the chain
    s.reset()
    a, _ = s.feed_overview_flux(raw[:na * fb], k, flush=True)
    assert s.feed_into(None, 0, np.zeros((1, 33, 4), np.uint8), None, 1)[0] == api.SGZ_OK
    b, _ = s.feed_overview_flux(raw[na * fb:], k, flush=True)
    assert _same(np.concatenate([a, b]), ofr.overview(mapped, k)[0].reshape(-1, 1, 2))
    # reset: frames from 0, no predecessor
    s.reset()
    d, _ = s.feed_overview_flux(raw[:na * fb], k, flush=True)
    assert _same(d, ofr.overview(mapped[:fa], k)[0].reshape(-1, 1, 2))
    s.close()


def test_the_kinds_refuse_one_another(gpu):
    name = "f32"
    cfg, fmt, raw, n, plan, planar, mapped = _case(name, gpu)
    W, hop, P, fb = cfg["window_size"], cfg["hop"], cfg["axis_points"], 2 * BYTES[fmt]
    k = 5
    flux = _want(name, k, gpu)
    E, L = api.SGZ_EINVAL, api.lib()
    s = api.PcmStream(cfg, fmt, 2, None, chunk_samples=300)
    first = W + 11 * hop + 7                                         # 12 frames: two columns and two frames open
    rest = n - first
    F = FRAMES
    big = np.zeros((F, P, 4), np.uint8)
    big_f = np.zeros((F, 1, 2), api.OVERVIEW_FLUX_DTYPE)
    big_p = np.zeros((F, 1, 2, P), api.OVERVIEW_POWER_DTYPE)
    big_r = np.zeros((F, 1, P), api.OVERVIEW_STAT_DTYPE)
    big_v = np.zeros((F, 1, 2, P), np.float32)

    def err():
        return L.sgz_last_error().decode()

    def untouched():
        return not any(a.view(np.uint8).any() for a in (big, big_f, big_p, big_r, big_v))

    # refusals of the call itself: nothing consumed
    assert s.feed_overview_flux_into(raw, first, 0, False, big_f, F)[0] == E                               # k == 0
    assert s.feed_overview_flux_into(raw, first, k, False, None, F)[0] == E                                # columns close and there is no output
    assert s.feed_overview_flux_into(None, first, k, False, big_f, F)[0] == E                              # a null pcm
    st, c, _ = s.feed_overview_flux_into(raw, first, k, False, big_f, 1)                                   # a capacity below the need
    assert st == E and c == 2 and s.open_frames() == 0 and s.frames_for(first) == 12 and untouched()
    # a flux column open: the other kinds and the plain feed are refused, name the flush call and consume nothing; so is another k
    a, _ = s.feed_overview_flux(raw[:first * fb], k)
    assert a.shape[0] == 2 and s.open_frames() == 2 and s.columns_for(rest, k, True) == flux.shape[0] - 2 and s.columns_for(rest, k + 1, True) == 0
    tail = "a flux overview's -- flush it (sgz_pcm_stream_feed_overview_flux) or reset the stream first"
    assert s.feed_overview_into(raw[first * fb:], rest, k, True, big, big_v, F)[0] == E and err() == "sgz_pcm_stream_feed_overview: the open column is " + tail
    assert s.feed_overview_into(None, 0, k, True, big, big_v, F)[0] == E                                   # ... not even its flush
    assert s.feed_overview_stats_into(raw[first * fb:], rest, k, True, big, big_r, big_v, F)[0] == E and err() == "sgz_pcm_stream_feed_overview_stats: the open column is " + tail
    assert s.feed_overview_power_into(raw[first * fb:], rest, k, True, big, big_p, big_v, F)[0] == E and err() == "sgz_pcm_stream_feed_overview_power: the open column is " + tail
    assert s.feed_into(raw[first * fb:], rest, big, None, F)[0] == E
    assert err() == "sgz_pcm_stream_feed: a flux overview's column is open -- flush it (sgz_pcm_stream_feed_overview_flux) or reset the stream first"
    assert s.feed_overview_flux_into(raw[first * fb:], rest, k + 1, True, big_f, F)[0] == E and "k differs" in err()
    assert untouched() and s.open_frames() == 2 and s.frames_for(rest) == F - 12
    b, _ = s.feed_overview_flux(raw[first * fb:], k, flush=True)
    assert _same(np.concatenate([a, b]), flux) and s.open_frames() == 0
    # a column of another kind open: a flux feed is refused, names its flush call and consumes nothing
    for kind, call, feed in (("peak-hold", "sgz_pcm_stream_feed_overview", lambda: s.feed_overview(raw[:first * fb], k)),
                             ("mean", "sgz_pcm_stream_feed_overview_stats", lambda: s.feed_overview_stats(raw[:first * fb], k)),
                             ("power", "sgz_pcm_stream_feed_overview_power", lambda: s.feed_overview_power(raw[:first * fb], k))):
        s.reset()
        feed()
        assert s.open_frames() == 2
        st, c, _ = s.feed_overview_flux_into(raw[first * fb:], rest, k, True, big_f, F)
        assert st == E and err() == f"sgz_pcm_stream_feed_overview_flux: the open column is a {kind} overview's -- flush it ({call}) or reset the stream first"
        assert untouched() and s.open_frames() == 2 and s.frames_for(rest) == F - 12
        assert s.feed_overview_flux_into(None, 0, k, True, big_f, F)[0] == E
    # reset drops an open flux column: any kind and any k is taken afterwards
    s.reset()
    s.feed_overview_flux(raw[:first * fb], k)
    assert s.open_frames() == 2
    s.reset()
    assert s.open_frames() == 0 and s.columns_for(W, 7, True) == 1
    pc, vc, _ = s.feed_overview(raw, k, flush=True, want_peaks=True)
    want_pc, want_vc, _ = plan.overview(planar, k, want_peaks=True)
    assert np.array_equal(pc, want_pc) and np.array_equal(vc.view(np.uint32), want_vc.view(np.uint32))
    # the track lane armed: refused, nothing consumed; disarmed, the feed is taken
    s.reset()
    track = np.zeros((F, 1, 6), np.float64)
    s.set_track(0, 0.4, track)
    st, c, _ = s.feed_overview_flux_into(raw, n, k, True, big_f, F)
    assert st == E and "track lane" in err() and untouched() and s.frames_for(n) == F and not track.any()
    s.set_track(0, 0.4, None)
    got, _ = s.feed_overview_flux(raw, k, flush=True)
    assert _same(got, flux)
    s.close()


@pytest.mark.parametrize("name", list(FORMATS))
def test_an_armed_waveform_lane_returns_its_usual_bytes(gpu, name):
    cfg, fmt, raw, n, plan, planar, mapped = _case(name, gpu)
    W, hop, fb = cfg["window_size"], cfg["hop"], 2 * BYTES[fmt]
    k, m = 3, 100
    flux = _want(name, k, gpu)
    results = []
    for kind in ("peak hold", "flux"):
        rng = np.random.default_rng(5)
        s = api.PcmStream(cfg, fmt, 2, None, chunk_samples=150)
        s.set_option(api.OPT_OVERVIEW_SLAB, 4)
        wave = np.zeros((n // m + 2, 2, 2), np.float32)
        s.set_waveform(m, wave)
        sizes = _feed_sizes(rng, n, W, hop)
        at, cols = 0, []
        for i, size in enumerate(sizes):
            piece, flush = (raw[at * fb:(at + size) * fb] if size else None), i == len(sizes) - 1
            out = s.feed_overview(piece, k, flush=flush, nsamples=size) if kind == "peak hold" else s.feed_overview_flux(piece, k, flush=flush, nsamples=size)
            cols.append(out[0] if kind == "flux" else None)
            at += size
        s.flush_waveform()
        written, _ = s.waveform_state()
        assert written == -(-n // m)
        if kind == "flux":
            assert _same(np.concatenate(cols), flux)
        results.append(wave[:written].copy())
        s.close()
    assert np.array_equal(results[0].view(np.uint32), results[1].view(np.uint32)) and results[0].any()


def test_pinned_output_and_the_one_shot_call(gpu):
    import torch
    name = "s16"
    cfg, fmt, raw, n, plan, planar, mapped = _case(name, gpu)
    W, fb = cfg["window_size"], 2 * BYTES[fmt]
    for k in (2, 7):
        flux = _want(name, k, gpu)
        cols = flux.shape[0]
        pcm = torch.from_numpy(raw.copy()).pin_memory()
        out = torch.zeros((*flux.shape, 11), dtype=torch.int64).pin_memory()
        s = api.PcmStream(cfg, fmt, 2, None, chunk_samples=500)
        st, c, t = s.feed_overview_flux_into(pcm, n, k, True, out, cols)
        assert st == api.SGZ_OK and c == cols == t.frames and t.chunks == -(-n // 500)
        assert _same(out.numpy().view(api.OVERVIEW_FLUX_DTYPE).reshape(flux.shape), flux), k
        s.close()
        st, r, t = api.overview_flux_pcm(cfg, raw, fmt, 2, k)
        assert st == api.SGZ_OK and t["chunks"] == 1 and t["frames"] == cols and _same(r, flux), k
    st, r, _ = api.overview_flux_pcm(cfg, raw[:(W - 1) * fb], fmt, 2, 2)
    assert st == api.SGZ_SKIPPED_FRAME and r.shape[0] == 0


def test_a_phase_stream_is_refused(gpu):
    """(an RSNT stream cannot be made at all; the one-shot call refuses both, tests/test_overview_flux_host.py)"""
    cfg = config.spectrum_config(window_size=1024, hop=256, axis_points=128, channel_mode=config.CH_PHASE)
    s = api.PcmStream(cfg, api.PCM_S16, 2, None, chunk_samples=4000)
    raw = np.zeros(4000 * 4, np.uint8)
    big = np.zeros((20, 1, 1), api.OVERVIEW_FLUX_DTYPE)
    frames = s.frames_for(4000)
    st, c, _ = s.feed_overview_flux_into(raw, 4000, 2, True, big, 20)
    assert st == api.SGZ_EUNSUPPORTED and not big.view(np.uint8).any() and s.frames_for(4000) == frames == 12
    image, _, _ = s.feed(raw)                                # nothing was consumed: the plain feed yields every frame of the 4000 samples
    assert image.shape[0] == frames
    s.close()
