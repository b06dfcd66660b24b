"""What a peak track of a whole render costs, on cfg2's buffer (stereo, 2 880 000 samples, N = W = 32768, hop 8192: 348 frames) and on a
buffer eight times as long.
    python tools/bench_track.py [--reps 7] [--out gpu_out/track.json]
  (a) what the library offered before for the same numbers: sgz_spectrogram_render_host with lines_out on a kept plan, then the host loop
      of sgz_track_peak_lines over every (frame, pair) -- render and loop apart and together (the loop goes through ctypes, one call per
      record, as any Python caller's would)
  (b) sgz_spectrogram_track_host on the same plan, with and without the image; its stage times (sgz_timing) beside (a)'s
Wall times are the host's clock around the call, median of --reps after one warm-up.  (b)'s track is checked against (a)'s, byte for byte.
    python tools/bench_track.py --kernels        # a few launches of the two batched tracker kernels and nothing else: the run to put
                                                 # under a kernel trace for their own times"""
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


def med(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


def host_loop(plan, lines):
    L, out = api.lib(), api.LinePeak()
    F, Cn = lines.shape[:2]
    track = np.zeros((F, Cn, 6), np.float64)
    for f in range(F):
        for p in range(Cn):
            L.sgz_track_peak_lines(plan.h, lines[f, p, GRAPH].ctypes.data_as(C.c_void_p), MOUSE, C.byref(out))
            track[f, p] = np.frombuffer(out, np.float64)
    return track


def measure(plan, x, reps):
    res = {"samples": x.shape[1], "frames": plan.num_frames(x.shape[1])}
    _, lines, t = api.render_spectrogram_host(plan, x, want_lines=True)
    want = host_loop(plan, lines)
    res["a_render_host_with_lines_ms"] = med(lambda: api.render_spectrogram_host(plan, x, want_lines=True), reps)
    res["a_render_host_stages"] = t
    res["a_host_loop_ms"] = med(lambda: host_loop(plan, lines), reps)
    res["a_together_ms"] = med(lambda: host_loop(plan, api.render_spectrogram_host(plan, x, want_lines=True)[1]), reps)
    res["a_lines_bytes"] = int(lines.nbytes)
    track, _, t = plan.track_render(x, GRAPH, MOUSE)
    res["b_equals_a"] = bool(np.array_equal(track.view(np.uint64), want.view(np.uint64)))
    res["b_track_host_with_image_ms"] = med(lambda: plan.track_render(x, GRAPH, MOUSE), reps)
    res["b_with_image_stages"] = t
    res["b_track_host_track_only_ms"] = med(lambda: plan.track_render(x, GRAPH, MOUSE, want_rgba=False), reps)
    res["b_track_only_stages"] = plan.track_render(x, GRAPH, MOUSE, want_rgba=False)[2]
    res["b_track_bytes"] = int(track.nbytes)
    return res


def kernels_only():
    """the two batched kernels alone, on cfg2's shapes: 348 records of line results / of bins, a render's and silent ones (the longest walks)"""
    cfg = config.cfg2()
    plan = api.Plan(cfg).upload()
    x = torch.from_numpy(synth.gen(config.CFG2_SEED, 48000, int(config.CFG2_SECONDS * 48000), 2)).cuda()
    F = plan.num_frames(x.shape[1])
    lines = torch.empty((F, 1, api.NUM_GRAPHS, plan.P, 2), dtype=torch.float32, device="cuda")
    plan.render(x, lines=lines)
    bins = plan.stage_bins(x)
    for _ in range(5):
        plan.track_peaks_lines(lines, GRAPH, MOUSE)
        plan.track_peaks(bins, MOUSE)
    silent_lines, silent_bins = torch.zeros_like(lines), torch.zeros_like(bins)
    for _ in range(5):
        plan.track_peaks_lines(silent_lines, GRAPH, 0.9)
        plan.track_peaks(silent_bins, 0.9)
    torch.cuda.synchronize()
    print(json.dumps({"records": F, "launches_each": 10}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if a.kernels:
        return kernels_only()
    cfg = config.cfg2()
    S = int(config.CFG2_SECONDS * 48000)
    x = synth.gen(config.CFG2_SEED, 48000, S, 2)
    plan = api.Plan(cfg).upload()
    res = {"cfg2_60s": measure(plan, x, a.reps), "cfg2_480s": measure(plan, np.ascontiguousarray(np.tile(x, (1, 8))), a.reps)}
    plan.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
