#!/usr/bin/env python3
"""The mean overview beside the peak-hold overview, its yardstick, on one device in one run:
  stage   sgz_stage_overview_stats against sgz_stage_overview on the same resident line results -- cfg2's shape: 348 frames, P = 1024, one
          pair -- at k = 1, 16 and 348, image + records + means against image + peaks.  Windows of 200 calls between two events, the two
          calls alternating window by window, medians of 7 windows, microseconds per call.
  feed    sgz_pcm_stream_feed_overview_stats against sgz_pcm_stream_feed_overview on kept streams: cfg2's 60 s as interleaved stereo S16
          (348 frames), k = 16, image + records + means against image + peaks; wall medians of 7, alternating.
The reads of the two stage calls are identical; the stats call stores 28 bytes per (column, pair, pixel) where the peak hold stores 4, and
divides once per (column, pair, pixel).  No bar is set: one JSON line per result, the ratio with it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from signalizer_amd import api, config, synth  # noqa: E402

REPS = 7
CALLS = 200
FRAMES = 348


def run_stage():
    import torch
    gpu = torch.device("cuda:0")
    plan = api.Plan(config.cfg2()).upload()
    P = plan.P
    rng = np.random.default_rng(2)
    lines = torch.from_numpy(rng.random((FRAMES, 1, api.NUM_GRAPHS, P, 2), dtype=np.float32)).to(gpu)
    L, s = api.lib(), torch.cuda.current_stream().cuda_stream
    for k in (1, 16, FRAMES):
        columns = -(-FRAMES // k)
        rgba = torch.empty((columns, P, 4), dtype=torch.uint8, device=gpu)
        peaks = torch.empty((columns, 1, P), dtype=torch.float32, device=gpu)
        stats = torch.empty((columns, 1, P, 3), dtype=torch.int64, device=gpu)
        means = torch.empty((columns, 1, P), dtype=torch.float32, device=gpu)

        def peak_hold():
            return L.sgz_stage_overview(plan.h, lines.data_ptr(), FRAMES, k, 0, 1, 0, None, rgba.data_ptr(), peaks.data_ptr(), s)

        def mean_range():
            return L.sgz_stage_overview_stats(plan.h, lines.data_ptr(), FRAMES, k, 0, 1, 0, None, rgba.data_ptr(), stats.data_ptr(), means.data_ptr(), s)

        times = {"peak_hold": [], "stats": []}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for rep in range(REPS + 2):                                # (two windows of each to warm up)
            for name, fn in (("peak_hold", peak_hold), ("stats", mean_range)):
                ev[0].record()
                for _ in range(CALLS):
                    assert fn() == api.SGZ_OK
                ev[1].record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[name].append(ev[0].elapsed_time(ev[1]) * 1e3 / CALLS)
        same_hi = bool(torch.equal((stats[..., 2] >> 32).to(torch.int32), peaks.view(torch.int32)))                     # hi: the high half of word 2
        p_us, s_us = float(np.median(times["peak_hold"])), float(np.median(times["stats"]))
        print(json.dumps({"run": "stage", "k": k, "frames": FRAMES, "columns": columns, "P": P, "peak_hold_us": round(p_us, 2), "stats_us": round(s_us, 2),
                          "stats_over_peak_hold": round(s_us / p_us, 3), "all_peak_hold_us": [round(t, 2) for t in times["peak_hold"]],
                          "all_stats_us": [round(t, 2) for t in times["stats"]], "read_bytes": FRAMES * P * 8,
                          "peak_hold_store_bytes": columns * P * 8, "stats_store_bytes": columns * P * 32, "hi_equals_peaks": same_hi}), flush=True)


def run_feed(seconds):
    cfg = config.cfg2()
    S = int(cfg["sample_rate"] * seconds)
    x = synth.gen(config.CFG2_SEED, int(cfg["sample_rate"]), S, 2)
    pcm = np.clip(np.round(x.T.astype(np.float64) * 32768.0), -32768, 32767).astype("<i2").reshape(-1)      # interleaved
    k = 16
    streams = {"peak_hold": api.PcmStream(cfg, api.PCM_S16, 2), "stats": api.PcmStream(cfg, api.PCM_S16, 2)}

    def peak_hold():
        streams["peak_hold"].reset()
        return streams["peak_hold"].feed_overview(pcm, k, flush=True, want_peaks=True)

    def mean_range():
        streams["stats"].reset()
        return streams["stats"].feed_overview_stats(pcm, k, flush=True, want_means=True)

    times = {"peak_hold": [], "stats": []}
    for rep in range(REPS + 2):
        for name, fn in (("peak_hold", peak_hold), ("stats", mean_range)):
            t0 = time.perf_counter()
            out = fn()
            if rep >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
    columns = out[0].shape[0]
    p_ms, s_ms = float(np.median(times["peak_hold"])), float(np.median(times["stats"]))
    print(json.dumps({"run": "feed", "k": k, "seconds": seconds, "columns": columns, "peak_hold_ms": round(p_ms, 3), "stats_ms": round(s_ms, 3),
                      "stats_over_peak_hold": round(s_ms / p_ms, 3), "all_peak_hold_ms": [round(t, 3) for t in times["peak_hold"]],
                      "all_stats_ms": [round(t, 3) for t in times["stats"]]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=config.CFG2_SECONDS)
    ap.add_argument("--stage-only", action="store_true")
    args = ap.parse_args()
    run_stage()
    if not args.stage_only:
        run_feed(args.seconds)


if __name__ == "__main__":
    main()
