"""The power overview inside the PCM stream on the GPU (sgz_pcm_stream_feed_overview_power, sgz_spectrogram_overview_power_pcm; csrc/pcm.hip, the
slab loop in csrc/api.hip): 16-bit and fp32 stereo, window 64, hop 16, P 33, 2000 sample frames.

Byte for byte -- image, records and levels --, no tolerance: the columns of all power feeds of a stream, of which only the last flushes,
concatenated == Plan.overview_power (sgz_spectrogram_overview_power_host) of the numpy-converted planar floats, for every way of cutting the
stream into feeds of a seeded list, small chunk_samples, slab 3 and a flush with no new samples; that reference in turn == the restatement
(tests/overview_power_ref.py) on Plan.stage_mapped.  The three kinds of open column refuse one another and consume nothing; the track lane
armed is refused; an armed waveform lane returns its usual bytes; the decay state of a following plain feed is that of a stream that never saw
the power feed; the one-shot call equals the stream."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_ref as ov  # noqa: E402
import overview_power_ref as opr  # noqa: E402
from test_gpu_pcm import BYTES, convert_ref, to_bytes  # noqa: E402
from test_gpu_pcm_overview import _feed_sizes  # noqa: E402

pytestmark = pytest.mark.gpu

FRAMES = 122                                                 # 64 + 16 * 121 = 2000 sample frames
CFG = dict(window_size=64, hop=16, axis_points=33)
FORMATS = {"s16": api.PCM_S16, "f32": api.PCM_F32}
_made, _wants = {}, {}


def _case(name, gpu):
    """(cfg, format, PCM bytes, samples, plan, planar floats) -- once per format"""
    if name not in _made:
        fmt = FORMATS[name]
        cfg = config.spectrum_config(**CFG)
        x = ov.burst_signal(cfg["window_size"], cfg["hop"], FRAMES, 2, cfg["sample_rate"], seed=3 + fmt)
        inter = np.ascontiguousarray(x.T).reshape(-1)
        raw = to_bytes(np.clip(np.round(inter.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int64), fmt) if fmt == api.PCM_S16 else to_bytes(inter, fmt)
        planar = np.ascontiguousarray(convert_ref(raw, fmt, 2))
        plan = api.Plan(cfg).upload()
        assert x.shape[1] == 2000 and plan.num_frames(2000) == FRAMES
        for a in (raw, planar):
            a.setflags(write=False)
        _made[name] = (cfg, fmt, raw, 2000, plan, planar)
    return _made[name]


def _want(name, k, gpu):
    """Plan.overview_power of the converted floats at k: (image, records, level bits) -- held to the restatement on stage_mapped once"""
    if (name, k) not in _wants:
        import torch
        cfg, fmt, raw, n, plan, planar = _case(name, gpu)
        image, power, levels, _ = plan.overview_power(planar, k, want_power=True, want_levels=True)
        mapped = plan.stage_mapped(torch.from_numpy(planar.copy()).to(gpu)).cpu().numpy()
        assert opr.same(power, opr.columns_of(mapped, k)[0])
        assert np.array_equal(levels.view(np.uint32), plan.overview_power_levels(power).view(np.uint32))
        _wants[name, k] = (image, power, levels.view(np.uint32))
    return _wants[name, k]


def _run(s, raw, fb, sizes, k, last_flushes, W, hop):
    """feeds the sizes in turn (the last one flushing, or an empty flushing feed behind them); checks columns_for and open_frames around every
    feed against sgz_stream_step / sgz_overview_step chained; -> (image, records, level bits) of all feeds"""
    images, power, levels, at, held, open_frames = [], [], [], 0, 0, 0
    feeds = [(size, last_flushes and i == len(sizes) - 1) for i, size in enumerate(sizes)] + ([] if last_flushes else [(0, True)])
    for size, flush in feeds:
        frames, held = api.stream_step(W, hop, held, size)
        columns, open_frames = api.overview_step(k, open_frames, frames, flush)
        assert s.columns_for(size, k, flush) == columns
        image, r, lv, t = s.feed_overview_power(raw[at * fb:(at + size) * fb] if size else None, k, flush=flush, nsamples=size, want_levels=True)
        assert image.shape[0] == r.shape[0] == lv.shape[0] == columns == t["frames"] and s.open_frames() == open_frames, (size, flush, columns)
        images.append(image); power.append(r); levels.append(lv.view(np.uint32))
        at += size
    return np.concatenate(images), np.concatenate(power), np.concatenate(levels)


@pytest.mark.parametrize("name", list(FORMATS))
def test_streamed_power_equals_the_power_of_the_converted_floats(gpu, name):
    cfg, fmt, raw, n, plan, planar = _case(name, gpu)
    W, hop, fb = cfg["window_size"], cfg["hop"], 2 * BYTES[fmt]
    rng = np.random.default_rng(11 + fmt)
    for chunk in (100, 0):                                   # pieces of 100 samples: about six frames each; and the default
        s = api.PcmStream(cfg, fmt, 2, None, chunk_samples=chunk)
        for k in (1, 4, 7, FRAMES + 3):
            image, power, levels = _want(name, k, gpu)
            for slab in (0, 3):
                s.set_option(api.OPT_OVERVIEW_SLAB, slab)
                for mode in ("one feed", "seeded feeds", "seeded feeds, then an empty flushing feed"):
                    s.reset()
                    sizes = [n] if mode == "one feed" else _feed_sizes(rng, n, W, hop)
                    got = _run(s, raw, fb, sizes, k, mode != "seeded feeds, then an empty flushing feed", W, hop)
                    what = (name, chunk, k, slab, mode, sizes)
                    assert opr.same(got[1], power), what
                    assert np.array_equal(got[2], levels) and np.array_equal(got[0], image), what
                    assert s.open_frames() == 0
        s.close()


def test_the_three_kinds_refuse_one_another_and_the_decay_state_is_left_alone(gpu):
    name = "f32"
    cfg, fmt, raw, n, plan, planar = _case(name, gpu)
    W, hop, P, fb = cfg["window_size"], cfg["hop"], cfg["axis_points"], 2 * BYTES[fmt]
    k = 5
    image, power, levels = _want(name, k, gpu)
    E, L = api.SGZ_EINVAL, api.lib()
    s = api.PcmStream(cfg, fmt, 2, None, chunk_samples=300)
    first = W + 11 * hop + 7                                         # 12 frames: two columns and two frames open
    rest = n - first
    F = FRAMES
    big = np.zeros((F, P, 4), np.uint8)
    big_p = np.zeros((F, 1, 2, P), api.OVERVIEW_POWER_DTYPE)
    big_r = np.zeros((F, 1, P), api.OVERVIEW_STAT_DTYPE)
    big_v = np.zeros((F, 1, 2, P), np.float32)

    def err():
        return L.sgz_last_error().decode()

    def untouched():
        return not big.any() and not big_v.any() and not big_p.view(np.uint8).any() and not big_r.view(np.uint8).any()

    # refusals of the call itself: nothing consumed
    assert s.feed_overview_power_into(raw, first, 0, False, big, big_p, big_v, F)[0] == E                  # k == 0
    assert s.feed_overview_power_into(raw, first, k, False, None, None, None, F)[0] == E                   # all outputs NULL
    assert s.feed_overview_power_into(None, first, k, False, big, big_p, big_v, F)[0] == E                 # a null pcm
    st, c, _ = s.feed_overview_power_into(raw, first, k, False, big, big_p, big_v, 1)                      # a capacity below the need
    assert st == E and c == 2 and s.open_frames() == 0 and s.frames_for(first) == 12 and untouched()
    # a power column open: the two other kinds and the plain feed are refused, name the flush call and consume nothing; so is another k
    a = s.feed_overview_power(raw[:first * fb], k, want_levels=True)
    assert a[0].shape[0] == 2 and s.open_frames() == 2 and s.columns_for(rest, k, True) == power.shape[0] - 2
    assert s.feed_overview_into(raw[first * fb:], rest, k, True, big, big_v, F)[0] == E and "sgz_pcm_stream_feed_overview_power" in err()
    assert s.feed_overview_into(None, 0, k, True, big, big_v, F)[0] == E                                   # ... not even its flush
    assert s.feed_overview_stats_into(raw[first * fb:], rest, k, True, big, big_r, big_v, F)[0] == E and "sgz_pcm_stream_feed_overview_power" in err()
    assert s.feed_into(raw[first * fb:], rest, big, None, F)[0] == E and "sgz_pcm_stream_feed_overview_power" in err()
    assert s.feed_overview_power_into(raw[first * fb:], rest, k + 1, True, big, big_p, big_v, F)[0] == E
    assert untouched() and s.open_frames() == 2 and s.frames_for(rest) == F - 12
    b = s.feed_overview_power(raw[first * fb:], k, flush=True, want_levels=True)
    assert np.array_equal(np.concatenate([a[0], b[0]]), image) and opr.same(np.concatenate([a[1], b[1]]), power)
    assert np.array_equal(np.concatenate([a[2], b[2]]).view(np.uint32), levels) and s.open_frames() == 0
    # a peak-hold column open, then a mean overview's: a power feed is refused, names their flush calls and consumes nothing
    for kind, call in (("peak-hold", "sgz_pcm_stream_feed_overview)"), ("mean overview", "sgz_pcm_stream_feed_overview_stats)")):
        s.reset()
        if kind == "peak-hold":
            s.feed_overview(raw[:first * fb], k)
        else:
            s.feed_overview_stats(raw[:first * fb], k)
        assert s.open_frames() == 2
        st, c, _ = s.feed_overview_power_into(raw[first * fb:], rest, k, True, big, big_p, big_v, F)
        assert st == E and kind in err() and call in err() and untouched() and s.open_frames() == 2 and s.frames_for(rest) == F - 12
        assert s.feed_overview_power_into(None, 0, k, True, big, big_p, big_v, F)[0] == E
    # reset drops an open power column: any kind and any k is taken afterwards
    s.reset()
    s.feed_overview_power(raw[:first * fb], k)
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
    st, c, _ = s.feed_overview_power_into(raw, n, k, True, big, big_p, big_v, F)
    assert st == E and "track lane" in err() and untouched() and s.frames_for(n) == F and not track.any()
    s.set_track(0, 0.4, None)
    got = s.feed_overview_power(raw, k, flush=True, want_levels=True)
    assert np.array_equal(got[0], image) and opr.same(got[1], power)
    s.close()


def test_a_power_feed_neither_reads_nor_advances_the_decay_state(gpu):
    """plain feed A, power feed B, plain feed C: C's image and line results are the render of its frames from the decay state A left -- the
    reference carries that state over B's frames through the plan's own render with a state buffer"""
    import torch
    name = "s16"
    cfg, fmt, raw, n, plan, planar = _case(name, gpu)
    W, hop, P, fb = cfg["window_size"], cfg["hop"], cfg["axis_points"], 2 * BYTES[fmt]
    d_x = torch.from_numpy(planar.copy()).to(gpu)
    for na, nb in ((W + 20 * hop + 5, 30 * hop + 3), (0, 41 * hop)):                 # a state from A; and a power feed first, state at rest
        s = api.PcmStream(cfg, fmt, 2, None, chunk_samples=300)
        fa = s.frames_for(na)
        if na:
            s.feed(raw[:na * fb])
        fb_ = s.frames_for(nb)
        _, power, _, _ = s.feed_overview_power(raw[na * fb:(na + nb) * fb], 4, flush=True)
        assert power.shape[0] == -(-fb_ // 4) and fb_ > 0
        got_image, got_lines, _ = s.feed(raw[(na + nb) * fb:], want_lines=True)
        fc = got_image.shape[0]
        assert fa + fb_ + fc == FRAMES and fc > 10
        state = torch.zeros((1, api.NUM_GRAPHS, P, 2), dtype=torch.float32, device=gpu)
        if fa:
            plan.render(d_x[:, :W + (fa - 1) * hop], state=state)
        lines = torch.empty((fc, 1, api.NUM_GRAPHS, P, 2), dtype=torch.float32, device=gpu)
        want_image = plan.render(d_x[:, (fa + fb_) * hop:], lines=lines, state=state).cpu().numpy()
        assert np.array_equal(got_image, want_image), (na, nb)
        assert np.array_equal(got_lines.view(np.uint32), lines.cpu().numpy().view(np.uint32)), (na, nb)
        s.close()


@pytest.mark.parametrize("name", list(FORMATS))
def test_an_armed_waveform_lane_returns_its_usual_bytes(gpu, name):
    cfg, fmt, raw, n, plan, planar = _case(name, gpu)
    W, hop, fb = cfg["window_size"], cfg["hop"], 2 * BYTES[fmt]
    k, m = 3, 100
    image, power, levels = _want(name, k, gpu)
    results = []
    for kind in ("peak hold", "power"):
        rng = np.random.default_rng(5)
        s = api.PcmStream(cfg, fmt, 2, None, chunk_samples=150)
        s.set_option(api.OPT_OVERVIEW_SLAB, 4)
        wave = np.zeros((n // m + 2, 2, 2), np.float32)
        s.set_waveform(m, wave)
        sizes = _feed_sizes(rng, n, W, hop)
        at, cols = 0, []
        for i, size in enumerate(sizes):
            piece, flush = (raw[at * fb:(at + size) * fb] if size else None), i == len(sizes) - 1
            out = s.feed_overview(piece, k, flush=flush, nsamples=size) if kind == "peak hold" else s.feed_overview_power(piece, k, flush=flush, nsamples=size)
            cols.append(out[1] if kind == "power" else None)
            at += size
        s.flush_waveform()
        written, _ = s.waveform_state()
        assert written == -(-n // m)
        if kind == "power":
            assert opr.same(np.concatenate(cols), power)
        results.append(wave[:written].copy())
        s.close()
    assert np.array_equal(results[0].view(np.uint32), results[1].view(np.uint32)) and results[0].any()


def test_pinned_outputs_and_the_one_shot_call(gpu):
    import torch
    name = "f32"
    cfg, fmt, raw, n, plan, planar = _case(name, gpu)
    W, fb = cfg["window_size"], 2 * BYTES[fmt]
    for k in (2, 7):
        image, power, levels = _want(name, k, gpu)
        cols = image.shape[0]
        pcm = torch.from_numpy(raw.copy()).pin_memory()
        out = torch.zeros(image.shape, dtype=torch.uint8).pin_memory()
        out_r = torch.zeros((*power.shape, 4), dtype=torch.int64).pin_memory()
        out_l = torch.zeros(levels.shape, dtype=torch.float32).pin_memory()
        s = api.PcmStream(cfg, fmt, 2, None, chunk_samples=500)
        st, c, t = s.feed_overview_power_into(pcm, n, k, True, out, out_r, out_l, cols)
        assert st == api.SGZ_OK and c == cols == t.frames and t.chunks == -(-n // 500)
        assert np.array_equal(out.numpy(), image) and np.array_equal(out_l.numpy().view(np.uint32), levels), k
        assert opr.same(out_r.numpy().view(api.OVERVIEW_POWER_DTYPE).reshape(power.shape), power), k
        # one output alone: the others are not touched
        s.reset()
        out.zero_(); out_r.zero_()
        st, c, _ = s.feed_overview_power_into(pcm, n, k, True, None, None, out_l, cols)
        assert st == api.SGZ_OK and np.array_equal(out_l.numpy().view(np.uint32), levels) and not out.any() and not out_r.any()
        s.close()
        st, a, r, v, t = api.overview_power_pcm(cfg, raw, fmt, 2, k, want_levels=True)
        assert st == api.SGZ_OK and t["chunks"] == 1 and t["frames"] == cols
        assert np.array_equal(a, image) and opr.same(r, power) and np.array_equal(v.view(np.uint32), levels), k
    st, a, r, v, _ = api.overview_power_pcm(cfg, raw[:(W - 1) * fb], fmt, 2, 2, want_levels=True)
    assert st == api.SGZ_SKIPPED_FRAME and a.shape[0] == 0 and r.shape[0] == 0 and v.shape[0] == 0


def test_a_phase_stream_is_refused(gpu):
    """(an RSNT stream cannot be made at all; the one-shot call refuses both, tests/test_overview_power_host.py)"""
    cfg = config.spectrum_config(window_size=1024, hop=256, axis_points=128, channel_mode=config.CH_PHASE)
    s = api.PcmStream(cfg, api.PCM_S16, 2, None, chunk_samples=4000)
    raw = np.zeros(4000 * 4, np.uint8)
    big = np.zeros((20, 128, 4), np.uint8)
    frames = s.frames_for(4000)
    st, c, _ = s.feed_overview_power_into(raw, 4000, 2, True, big, None, None, 20)
    assert st == api.SGZ_EUNSUPPORTED and not big.any() and s.frames_for(4000) == frames == 12
    image, _, _ = s.feed(raw)                                # nothing was consumed: the plain feed yields every frame of the 4000 samples
    assert image.shape[0] == frames
    s.close()
