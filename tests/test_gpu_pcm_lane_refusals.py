"""All five lanes of the PCM stream armed together, and a feed that one or two of them cannot take (csrc/pcm.hip: the stream walks its lanes
in loops; this is what such a loop can get wrong and no single-lane test sees).

f32_two_pairs of tests/test_gpu_pcm_level.py on a stream at chunk_samples = 1000, the m of test_all_lanes_armed_together (7, 16, 33, 50),
every buffer pageable and filled with a sentinel.  Byte for byte, no tolerance:
  (a) one lane at a time re-armed one unit short of a feed of 1400 samples: both kinds of feed return SGZ_EINVAL and name that lane, every
      lane's state and the stream's are what they were, every buffer -- image, lines and peaks included -- is untouched;
  (b) two lanes short, every pair: the message names the earlier one in the order waveform, level, true-peak, loudness, track;
  (c) with room again, the same feed gives what a twin that never saw a refusal gives, in every buffer;
  (d) each flush adds one column to its own lane and leaves the others alone; reset() empties every lane and leaves all armed.
7 and 50 divide 1400: behind that feed the waveform and loudness lanes have no column open, and their flushes add nothing (checked as such).
13 more samples open a column in all four lanes, and then each flush adds exactly one.  The refusals' messages are compared whole, a flush's
two as well (no column left; the lane off): every lane composes them from its own word."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_pcm import BYTES  # noqa: E402
from test_gpu_pcm_level import FRAMES, K, _case  # noqa: E402
from test_gpu_pcm_loudness import filt  # noqa: E402

pytestmark = pytest.mark.gpu

E = api.SGZ_EINVAL
FIRST, MORE = 1400, 13
LANES = ("waveform", "level", "truepeak", "loudness", "track")         # the order a feed refuses them in
WORDS = {"waveform": "waveform", "level": "level", "truepeak": "true-peak", "loudness": "loudness", "track": "track"}
M = {"waveform": 7, "level": 16, "truepeak": 33, "loudness": 50}
FEED_MESSAGE = {lane: f"sgz_pcm_stream: the feed closes more {WORDS[lane]} columns than the buffer has left (sgz_pcm_stream_{lane}_for; re-arm with "
                      f"sgz_pcm_stream_set_{lane})" for lane in M}
FEED_MESSAGE["track"] = ("sgz_pcm_stream: the feed completes more frames than the track buffer has left (sgz_pcm_stream_track_for; re-arm with "
                         "sgz_pcm_stream_set_track)")


class _Armed:
    """a stream with every lane armed: sentinel buffers of [capacity][rows][bytes of a record], a few units more than FIRST + MORE samples need"""

    def __init__(self):
        cfg, fmt, channels, cmap, raw, planar, _ = _case("f32_two_pairs")
        self.raw, self.fb, D = raw, channels * BYTES[fmt], planar.shape[0]
        self.P, self.pairs = cfg["axis_points"], D // 2
        self.s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=1000)
        self.rows = {"waveform": (D, 8), "level": (self.pairs, 80), "truepeak": (D, 16), "loudness": (D, 32), "track": (self.pairs, 48)}
        self.need = {lane: FIRST // m for lane, m in M.items()}         # units a feed of FIRST samples yields from rest
        self.need["track"] = self.s.frames_for(FIRST)
        self.out = {}
        for lane in LANES:
            self.arm(lane, self.need[lane] + 4)
        self.rgba = np.full((FRAMES, self.P, 4), 0xA5, np.uint8)
        self.lines = np.full((FRAMES, self.pairs, api.NUM_GRAPHS, self.P, 2, 4), 0xA5, np.uint8)
        self.peaks = np.full((FRAMES, self.pairs, self.P, 4), 0xA5, np.uint8)

    def arm(self, lane, capacity):
        buf = np.full((capacity,) + self.rows[lane], 0xA5, np.uint8)
        if lane == "track":
            self.s.set_track(0, 0.5, buf, capacity)
        elif lane == "loudness":
            self.s.set_loudness(filt(8000), M[lane], buf, capacity)
        else:
            getattr(self.s, "set_" + lane)(M[lane], buf, capacity)
        self.out[lane] = buf

    def state(self):
        s = self.s
        return ([getattr(s, lane + "_state")() for lane in LANES], [getattr(s, lane + "_for")(FIRST) for lane in LANES], s.frames_for(FIRST), s.open_frames())

    def buffers(self):
        return [self.out[lane] for lane in LANES] + [self.rgba, self.lines, self.peaks]

    def untouched(self):
        return all(bool((b == 0xA5).all()) for b in self.buffers())

    def refused(self, kind):
        """one feed of FIRST samples that must be refused -> the message"""
        if kind == "plain":
            st = self.s.feed_into(self.raw, FIRST, self.rgba, self.lines, FRAMES)[0]
        else:
            st = self.s.feed_overview_into(self.raw, FIRST, K, False, self.rgba, self.peaks, FRAMES)[0]
        assert st == E, kind
        return api.lib().sgz_last_error().decode()

    def feed(self, at, size):
        st, frames, _ = self.s.feed_into(self.raw[at * self.fb:(at + size) * self.fb], size, self.rgba, self.lines, FRAMES)
        assert st == api.SGZ_OK
        return frames


def test_a_short_lane_refuses_the_feed_and_nothing_else_moves(gpu):
    a, twin = _Armed(), _Armed()
    s = a.s
    rest = a.state()
    assert rest[0] == [(0, 0)] * 4 + [0] and rest[1] == [a.need[lane] for lane in LANES] and all(rest[1]) and rest[2:] == (2, 0)
    # (a) each lane in turn one unit short
    for lane in LANES:
        a.arm(lane, a.need[lane] - 1)
        for kind in ("plain", "overview"):
            assert a.refused(kind) == FEED_MESSAGE[lane], (lane, kind)
            assert a.state() == rest and a.untouched(), (lane, kind)
        a.arm(lane, a.need[lane] + 4)
    # (b) two lanes short: the earlier one is named
    for i, first in enumerate(LANES):
        for second in LANES[i + 1:]:
            a.arm(first, a.need[first] - 1)
            a.arm(second, a.need[second] - 1)
            for kind in ("plain", "overview"):
                msg = a.refused(kind)
                assert WORDS[first] in msg and WORDS[second] not in msg, (first, second, kind, msg)
            assert a.state() == rest and a.untouched(), (first, second)
            a.arm(first, a.need[first] + 4)
            a.arm(second, a.need[second] + 4)
    # (c) with room again: the twin's outputs, byte for byte
    assert a.feed(0, FIRST) == twin.feed(0, FIRST) == 2
    assert a.state() == twin.state()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.buffers(), twin.buffers()))
    assert not a.untouched()
    twin.s.close()
    # (d) a flush adds one column to its own lane, none where nothing is open, and leaves the other lanes alone
    columns = [lane for lane in LANES if lane != "track"]

    def flush_each(opened):
        for lane in columns:
            before = a.state()[0]
            getattr(s, "flush_" + lane)()
            want = list(before)
            written, open_ = before[LANES.index(lane)]
            assert (open_ > 0) == opened[lane], lane
            want[LANES.index(lane)] = (written + (open_ > 0), 0)
            assert a.state()[0] == want, lane

    assert a.state()[0] == [(FIRST // M[lane], FIRST % M[lane]) for lane in columns] + [2]
    flush_each({"waveform": False, "level": True, "truepeak": True, "loudness": False})
    a.feed(FIRST, MORE)
    flush_each(dict.fromkeys(columns, True))
    # reset: every lane empty, every lane still armed
    s.reset()
    assert a.state()[0] == [(0, 0)] * 4 + [0]
    assert all(getattr(s, lane + "_for")(FIRST) > 0 for lane in LANES)
    # a flush refuses in its lane's own words: no column left behind the cursor, then the lane off; neither moves anything
    L = api.lib()
    for lane in columns:
        a.arm(lane, MORE // M[lane])
    a.feed(0, MORE)
    full = a.state()
    assert full[0] == [(MORE // M[lane], MORE % M[lane]) for lane in columns] + [0]
    for lane in columns:
        assert getattr(L, "sgz_pcm_stream_flush_" + lane)(s.h) == E
        assert L.sgz_last_error().decode() == f"sgz_pcm_stream_flush_{lane}: no column left in the buffer (re-arm with sgz_pcm_stream_set_{lane})"
        assert a.state() == full, lane
    for lane in columns:
        s.set_loudness(None, 0) if lane == "loudness" else getattr(s, "set_" + lane)(0)
        assert getattr(L, "sgz_pcm_stream_flush_" + lane)(s.h) == E
        assert L.sgz_last_error().decode() == f"sgz_pcm_stream_flush_{lane}: the lane is off (sgz_pcm_stream_set_{lane})"
    s.close()
