#!/usr/bin/env python3
"""The cross overview's reduction beside the bins stage that feeds it, on one device in one process:
  sgz_stage_overview_cross (its two launches alone, on resident complex bins) against sgz_stage_bins for the same frames -- existing code, the
  yardstick -- at cfg2's shape in Phase mode: stereo, N = 32768, 348 frames, k = 4.  One JSON line per band table: 1/3-octave and 1024 equal
  bands.  Device events around windows of CALLS calls, the two calls alternating window by window after two warm-up windows of each, the
  median and the spread (least .. greatest) of REPS windows, milliseconds per call.
The reduction reads every bin of every frame once, 8 (N + 1) bytes per (frame, pair): those bytes / its time are reported as a fraction of
the achievable copy rate of the device (6.29 TB/s, a float4 copy).  From the byte count the reduction should cost less than the bins stage.
No bar is set."""
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
COPY_RATE = 6.29e12                                            # bytes per second, measured float4 copy


def run(table, calls):
    import torch
    gpu = torch.device("cuda:0")
    cfg = config.cfg2()
    cfg["channel_mode"] = config.CH_PHASE
    plan = api.Plan(cfg).upload()
    N = plan.N
    S = int(cfg["sample_rate"] * config.CFG2_SECONDS)
    x = torch.from_numpy(np.ascontiguousarray(synth.gen(config.CFG2_SEED, int(cfg["sample_rate"]), S, 2))).to(gpu)
    frames = plan.num_frames(S)
    if table == "thirds":
        edges = api.cross_edges_octave(cfg["sample_rate"], N, 3, 20.0, 20000.0)[0]
    else:
        edges = np.unique(np.round(np.linspace(1, N // 2 - 1, 1025)).astype(np.uint32))
    plan.set_cross_edges(edges)
    bands = len(edges) - 1
    columns = -(-frames // K)
    L, s = api.lib(), torch.cuda.current_stream().cuda_stream
    bins = plan.stage_bins(x)
    out = torch.empty((columns, 1, bands, 10), dtype=torch.int64, device=gpu)
    carry = torch.empty((1, bands, 10), dtype=torch.int64, device=gpu)

    def stage_bins():
        return L.sgz_stage_bins(plan.h, x.data_ptr(), x.stride(0), S, bins.data_ptr(), s)

    def reduction():
        return L.sgz_stage_overview_cross(plan.h, bins.data_ptr(), frames, K, 0, 1, 0, carry.data_ptr(), out.data_ptr(), s)

    times = {"bins": [], "cross": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for rep in range(REPS + 2):                                    # (two windows of each to warm up)
        for name, fn in (("bins", stage_bins), ("cross", reduction)):
            ev[0].record()
            for _ in range(calls):
                assert fn() == api.SGZ_OK
            ev[1].record()
            torch.cuda.synchronize()
            if rep >= 2:
                times[name].append(ev[0].elapsed_time(ev[1]) / calls)
    b_ms, c_ms = float(np.median(times["bins"])), float(np.median(times["cross"]))
    read = frames * 8 * (N + 1)
    print(json.dumps({"table": table, "bands": bands, "N": N, "frames": frames, "k": K, "columns": columns, "calls_per_window": calls,
                      "stage_bins_ms": round(b_ms, 4), "cross_ms": round(c_ms, 4), "cross_over_bins": round(c_ms / b_ms, 3),
                      "bytes_read": read, "fraction_of_copy_rate": round(read / (c_ms * 1e-3) / COPY_RATE, 3),
                      "stage_bins_spread_ms": [round(min(times["bins"]), 4), round(max(times["bins"]), 4)],
                      "cross_spread_ms": [round(min(times["cross"]), 4), round(max(times["cross"]), 4)],
                      "all_stage_bins_ms": [round(t, 4) for t in times["bins"]], "all_cross_ms": [round(t, 4) for t in times["cross"]]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", nargs="*", default=["thirds", "equal1024"])
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    for table in args.tables:
        run(table, args.calls)


if __name__ == "__main__":
    main()
