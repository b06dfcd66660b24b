"""What the track lane costs (sgz_pcm_stream_set_track; sgz_stage_track_peaks_values), on cfg2's 60 s at hop 200 (stereo, 2 880 000 samples,
N = W = 32768: 14 237 frames) as interleaved S16, one kept sgz_pcm_stream per way, all in one process.
    python tools/bench_track_lane.py [--reps 7] [--hop 200] [--out gpu_out/track_lane.json]
  (a) what the library offered before for a track from a stream: feed(..., lines_out) and the host loop of sgz_track_peak_lines over every
      (frame, pair) -- feed and loop apart and together (the loop goes through ctypes, one call per record, as any Python caller's would)
  (b) the armed feed without lines_out: the image and the records come back, the line results stay on the device
  (c) the track-only pass: an overview feed with k = the frame count and the peaks only -- one column of peaks beside the records
  (d) feed without lines_out, the lane armed against disarmed, alternating: what arming costs a feed that wanted the image alone (armed, it
      renders in the with-lines form)
  (e) sgz_stage_track_peaks_values alone on 1780 x 1 and 100 000 x 1 records of P = 1024 (a view's columns; a whole file's), between events
(b)'s and (c)'s records are checked against (a)'s byte for byte before anything is timed.  Wall times are the host's clock around the
calls, medians of --reps after one warm-up.  Every figure comes from a run on the GPU; the tool refuses to run without one."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from signalizer_amd import api, config, synth

GRAPH, MOUSE = 0, 0.37
LP = len(api.LinePeak._fields_)


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def med(f, reps):
    f()
    ts = [timed(f) for _ in range(reps)]
    return round(statistics.median(ts), 3), [round(min(ts), 3), round(max(ts), 3)]


def host_loop(plan, lines, track):
    L, out = api.lib(), api.LinePeak()
    F, Cn = lines.shape[:2]
    for f in range(F):
        for p in range(Cn):
            L.sgz_track_peak_lines(plan.h, lines[f, p, GRAPH].ctypes.data_as(C.c_void_p), MOUSE, C.byref(out))
            track[f, p] = np.frombuffer(out, np.float64)
    return track


def events(f, warm=3, reps=20):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = []
    for k in range(warm + reps):
        ev[0].record()
        f()
        ev[1].record()
        ev[1].synchronize()
        if k >= warm:
            ts.append(ev[0].elapsed_time(ev[1]))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--hop", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = config.cfg2()
    cfg["hop"] = a.hop
    S = int(config.CFG2_SECONDS * 48000)
    sig = synth.gen(config.CFG2_SEED, 48000, S, 2)
    s16 = np.ascontiguousarray(np.clip(np.round(sig.T * 32768.0), -32768, 32767).astype(np.int16))
    del sig
    F, P, Cn = int(api.lib().sgz_num_frames(S, cfg["window_size"], cfg["hop"])), cfg["axis_points"], cfg["num_pairs"]
    plan = api.Plan(cfg)                                                    # host tables: the host loop's
    res = {"device": torch.cuda.get_device_name(0), "samples": S, "hop": a.hop, "frames": F, "reps": a.reps,
           "record_bytes": LP * 8, "lines_bytes_per_record": api.NUM_GRAPHS * P * 8}
    rgba = np.zeros((F, P, 4), np.uint8)

    # (a)
    lines = np.zeros((F, Cn, api.NUM_GRAPHS, P, 2), np.float32)
    want = np.zeros((F, Cn, LP), np.float64)
    kept = api.PcmStream(cfg, api.PCM_S16, 2)

    def a_feed():
        kept.reset()
        st, f, _ = kept.feed_into(s16, S, rgba, lines, F, timing=False)
        assert st == 0 and f == F

    a_feed()
    host_loop(plan, lines, want)
    image = rgba.copy()
    res["a_feed_with_lines_ms"], res["a_feed_with_lines_min_max_ms"] = med(a_feed, a.reps)
    res["a_host_loop_ms"], _ = med(lambda: host_loop(plan, lines, np.zeros_like(want)), a.reps)
    res["a_together_ms"], res["a_together_min_max_ms"] = med(lambda: (a_feed(), host_loop(plan, lines, np.zeros_like(want))), a.reps)
    res["a_lines_bytes"] = int(lines.nbytes)
    kept.close()
    del lines

    # (b), checked first
    track = np.zeros((F, Cn, LP), np.float64)
    lane = api.PcmStream(cfg, api.PCM_S16, 2)

    def b_feed(armed=True):
        lane.reset()
        lane.set_track(GRAPH, MOUSE, track if armed else None)
        st, f, _ = lane.feed_into(s16, S, rgba, None, F, timing=False)
        assert st == 0 and f == F

    rgba[:] = 0
    b_feed()
    res["b_equals_a"] = bool(np.array_equal(track.view(np.uint64), want.view(np.uint64)) and np.array_equal(rgba, image))
    assert res["b_equals_a"], "(b)'s records or image differ from (a)'s"

    # (c), checked first
    only = api.PcmStream(cfg, api.PCM_S16, 2)
    peaks = np.zeros((1, Cn, P), np.float32)

    def c_feed():
        only.reset()
        only.set_track(GRAPH, MOUSE, track)
        st, c, _ = only.feed_overview_into(s16, S, F, True, None, peaks, 1, timing=False)
        assert st == 0 and c == 1

    track[:] = 0
    c_feed()
    res["c_equals_a"] = bool(np.array_equal(track.view(np.uint64), want.view(np.uint64)))
    assert res["c_equals_a"], "(c)'s records differ from (a)'s"

    res["b_armed_feed_ms"], res["b_armed_feed_min_max_ms"] = med(b_feed, a.reps)
    res["c_track_only_ms"], res["c_track_only_min_max_ms"] = med(c_feed, a.reps)
    res["b_over_a"] = round(res["b_armed_feed_ms"] / res["a_together_ms"], 4)
    res["c_over_a"] = round(res["c_track_only_ms"] / res["a_together_ms"], 4)
    res["track_bytes"] = int(track.nbytes)
    only.close()

    # (d)
    b_feed(True), b_feed(False)
    ts = {True: [], False: []}
    for _ in range(a.reps):
        for armed in (True, False):
            ts[armed].append(timed(lambda: b_feed(armed)))
            assert np.array_equal(rgba, image)
    res["d_armed_ms"], res["d_disarmed_ms"] = round(statistics.median(ts[True]), 3), round(statistics.median(ts[False]), 3)
    res["d_armed_min_max_ms"] = [round(min(ts[True]), 3), round(max(ts[True]), 3)]
    res["d_disarmed_min_max_ms"] = [round(min(ts[False]), 3), round(max(ts[False]), 3)]
    res["d_armed_over_disarmed"] = round(res["d_armed_ms"] / res["d_disarmed_ms"], 4)
    lane.close()

    # (e)
    stage = api.Plan(config.spectrum_config(window_size=4096, hop=1024, axis_points=1024)).upload()
    res["e_stage_values"] = {}
    for records in (1780, 100000):
        values = torch.rand((records, 1, 1024), dtype=torch.float32, device="cuda")
        out = torch.empty((records, 1, LP), dtype=torch.float64, device="cuda")
        ms = events(lambda: stage.track_peaks_values(values, MOUSE, out=out))
        res["e_stage_values"][str(records)] = {"ms": round(ms, 4), "bytes_of_values": records * 1024 * 4}
        del values, out
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
