#!/usr/bin/env python3
"""The power overview's render beside the mean overview's, on one device in one process:
  sgz_spectrogram_overview_power_device against sgz_spectrogram_overview_stats_device on the same resident audio, image + records + the
  value plane (levels / means) each, k = 4 -- cfg2's 60 s (348 frames) and a file of about ten minutes.  Device events around windows of
  CALLS calls, the two calls alternating window by window after two warm-up windows of each, the median and the spread (least .. greatest)
  of REPS windows, milliseconds per call.
The power render runs K_A and its reduction, which reads 4 bytes a value; the stats render runs K_A, K_B with line results and a reduction that
reads them.  No bar is set: one JSON line per length, the ratio with it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from signalizer_amd import api, config, synth  # noqa: E402

REPS = 7
K = 4


def run(seconds, calls):
    import torch
    gpu = torch.device("cuda:0")
    cfg = config.cfg2()
    plan = api.Plan(cfg).upload()
    S = int(cfg["sample_rate"] * seconds)
    tile = synth.gen(config.CFG2_SEED, int(cfg["sample_rate"]), min(S, int(cfg["sample_rate"] * config.CFG2_SECONDS)), 2)
    x = torch.from_numpy(np.ascontiguousarray(np.tile(tile, (1, -(-S // tile.shape[1])))[:, :S])).to(gpu)
    frames = plan.num_frames(S)
    columns = -(-frames // K)
    P, sides = plan.P, plan.sides
    L, s = api.lib(), torch.cuda.current_stream().cuda_stream
    rgba = torch.empty((columns, P, 4), dtype=torch.uint8, device=gpu)
    stats = torch.empty((columns, 1, P, 3), dtype=torch.int64, device=gpu)
    means = torch.empty((columns, 1, P), dtype=torch.float32, device=gpu)
    power = torch.empty((columns, 1, sides, P, 4), dtype=torch.int64, device=gpu)
    levels = torch.empty((columns, 1, sides, P), dtype=torch.float32, device=gpu)

    def mean_range():
        return L.sgz_spectrogram_overview_stats_device(plan.h, x.data_ptr(), x.stride(0), S, K, rgba.data_ptr(), stats.data_ptr(), means.data_ptr(), None, s)

    def mean_square():
        return L.sgz_spectrogram_overview_power_device(plan.h, x.data_ptr(), x.stride(0), S, K, rgba.data_ptr(), power.data_ptr(), levels.data_ptr(), s)

    times = {"stats": [], "power": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for rep in range(REPS + 2):                                    # (two windows of each to warm up)
        for name, fn in (("stats", mean_range), ("power", mean_square)):
            ev[0].record()
            for _ in range(calls):
                assert fn() == api.SGZ_OK
            ev[1].record()
            torch.cuda.synchronize()
            if rep >= 2:
                times[name].append(ev[0].elapsed_time(ev[1]) / calls)
    s_ms, p_ms = float(np.median(times["stats"])), float(np.median(times["power"]))
    print(json.dumps({"seconds": seconds, "frames": frames, "k": K, "columns": columns, "P": P, "calls_per_window": calls,
                      "stats_ms": round(s_ms, 4), "power_ms": round(p_ms, 4), "power_over_stats": round(p_ms / s_ms, 3),
                      "stats_spread_ms": [round(min(times["stats"]), 4), round(max(times["stats"]), 4)],
                      "power_spread_ms": [round(min(times["power"]), 4), round(max(times["power"]), 4)],
                      "all_stats_ms": [round(t, 4) for t in times["stats"]], "all_power_ms": [round(t, 4) for t in times["power"]]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, nargs="*", default=[config.CFG2_SECONDS, 600.0])
    args = ap.parse_args()
    for seconds in args.seconds:
        run(seconds, 50 if seconds <= 120 else 10)


if __name__ == "__main__":
    main()
