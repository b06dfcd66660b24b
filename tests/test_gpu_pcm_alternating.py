"""Both kinds of feed in turn on one PCM stream with both lanes armed and every destination pageable (csrc/pcm.hip: one piece loop, and
one table of pending host copies per slot that both kinds share).

Byte for byte, no tolerance: the plain feeds' rows == the same rows of sgz_spectrogram_render_host of the converted floats (image and line
results); every overview segment == tests/overview_ref.py's restatement on those line results; the waveform columns == tests/wave_ref.py
over the whole file; the track records == Plan.track_render; the sentinels behind both lanes' buffers stay; and every feed's timing counts
the frames / columns of sgz_stream_step / sgz_overview_step and ceil(size / chunk) pieces -- one for the empty flushing feed."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_ref as ov  # noqa: E402
import wave_ref as wr  # noqa: E402
from test_gpu_pcm import BYTES  # noqa: E402
from test_gpu_pcm_overview import _case  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK, M, GRAPH, FRACTION = 100, 7, 1, 0.03
LP = len(api.LinePeak._fields_)
SENTINEL = 0x5A5AA5A5C3C33C3C
# (kind, samples, k, flush, lines / image wanted): 2, 3, 1, 1 and 1 pieces, so each kind of feed finds the other's copies in both slots
FEEDS = (("plain", 150, 0, False, True), ("overview", 210, 5, False, True), ("overview", 0, 5, True, True), ("plain", 30, 0, False, False),
         ("overview", 26, 3, True, False))


def test_alternating_feeds_with_everything_armed_and_pageable(gpu, oracle):
    cfg, fmt, channels, cmap, raw, n, F, plan, planar, rgba, main = _case("w64")
    params = oracle.params_from_dict(cfg)
    W, hop, fb, Cn, D = cfg["window_size"], cfg["hop"], channels * BYTES[fmt], cfg["num_pairs"], planar.shape[0]
    assert sum(f[1] for f in FEEDS) == n
    _, lines, _ = api.render_spectrogram_host(plan, planar, want_lines=True)
    wave_want = wr.columns_of(planar, M)[0]
    track_want = plan.track_render(planar, GRAPH, FRACTION, want_rgba=False)[0].view(np.uint64)
    wave = np.full((wave_want.shape[0] + 2, D, 2), np.float32(-77.0))
    bits = np.full((F + 2, Cn, LP), SENTINEL, np.uint64)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=CHUNK)
    s.set_waveform(M, wave)
    s.set_track(GRAPH, FRACTION, bits.view(np.float64), F)
    at = held = done = open_frames = segment = 0
    for kind, size, k, flush, full in FEEDS:
        frames, held = api.stream_step(W, hop, held, size)
        upto = done + frames
        pcm = raw[at * fb:(at + size) * fb]
        what = (kind, size, k, flush)
        if kind == "plain":
            image, got_lines, t = s.feed(pcm, nsamples=size, want_lines=full)
            assert np.array_equal(image, rgba[done:upto]), what
            assert got_lines is None if not full else np.array_equal(got_lines.view(np.uint32), lines[done:upto].view(np.uint32)), what
            units, segment = frames, upto
        else:
            units, left = api.overview_step(k, open_frames, frames, flush)
            image, v, t = s.feed_overview(pcm if size else None, k, flush=flush, nsamples=size, want_rgba=full, want_peaks=True)
            want_v = ov.columns_of(main[segment:upto], k, flush=flush)[0][(done - segment) // k:]
            assert v.shape[0] == units and np.array_equal(v.view(np.uint32), want_v), what
            assert image is None if not full else np.array_equal(image, ov.blend(oracle, params, want_v)), what
            assert s.open_frames() == left, what
            open_frames = left
            if flush:
                segment = upto
        print(what, "frames", t["frames"], "chunks", t["chunks"])
        assert t["frames"] == units and t["chunks"] == max(1, -(-size // CHUNK)), (what, t)
        at, done = at + size, upto
        assert s.track_state() == done, what
    assert at == n and done == F and s.open_frames() == 0
    s.flush_waveform()
    assert s.waveform_state() == (wave_want.shape[0], 0)
    assert np.array_equal(wave[:wave_want.shape[0]].view(np.uint32), wave_want) and (wave[wave_want.shape[0]:] == np.float32(-77.0)).all()
    assert (bits[:F] == track_want).all() and (bits[F:] == SENTINEL).all()
    s.close()
