#!/usr/bin/env python3
"""The percentile overview's reduction beside the mean overview's, on one device in one process:
  sgz_stage_overview_pct against sgz_stage_overview_stats on the same resident line results [frames][1][2][1024] float2 (random values on the
  dB axis, a few NaNs), records + the value plane each (nq = 1, the median) -- cfg2's shape (348 frames, k = 4) and a long launch (40 000
  frames) as one column and as 1000 columns.  Then the streamed feed of cfg2's 60 s, 16-bit stereo, through sgz_pcm_stream_feed_overview_stats
  and _pct (k = 4, records + value plane to pageable memory).
Device events around windows of CALLS calls (the feeds: wall time of a whole file), the two calls alternating window by window after two
warm-up windows of each, the median and the spread (least .. greatest) of REPS windows, milliseconds per call.
A percentile record is 272 bytes, a stats record 24: at k = 4, where the records are most of the traffic, 272 / 24 = 11.3 is the expected floor
of the ratio.  No bar is set: one JSON line per shape, the ratio with it."""
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
Q = np.array([0.5], np.float64)


def _line(name, extra, times):
    a, b = float(np.median(times["stats"])), float(np.median(times["pct"]))
    print(json.dumps({"what": name, **extra, "stats_ms": round(a, 4), "pct_ms": round(b, 4), "pct_over_stats": round(b / a, 3),
                      "stats_spread_ms": [round(min(times["stats"]), 4), round(max(times["stats"]), 4)],
                      "pct_spread_ms": [round(min(times["pct"]), 4), round(max(times["pct"]), 4)]}), flush=True)


def stage(plan, frames, k, calls):
    import torch
    gpu = torch.device("cuda:0")
    P = plan.P
    gen = torch.Generator(device=gpu).manual_seed(frames + k)
    lines = torch.rand((frames, 1, api.NUM_GRAPHS, P, 2), dtype=torch.float32, device=gpu, generator=gen) * 1.2 - 0.1
    lines[::97, :, :, ::13] = float("nan")
    columns = -(-frames // k)
    L, s = api.lib(), torch.cuda.current_stream().cuda_stream
    stats = torch.empty((columns, 1, P, 3), dtype=torch.int64, device=gpu)
    pct = torch.empty((columns, 1, P, 34), dtype=torch.int64, device=gpu)
    values = torch.empty((columns, 1, P), dtype=torch.float32, device=gpu)
    qp = Q.ctypes.data

    def mean_range():
        return L.sgz_stage_overview_stats(plan.h, lines.data_ptr(), frames, k, 0, 1, 0, None, None, stats.data_ptr(), values.data_ptr(), s)

    def percentile():
        return L.sgz_stage_overview_pct(plan.h, lines.data_ptr(), frames, k, 0, 1, 0, qp, 1, None, None, pct.data_ptr(), values.data_ptr(), s)

    times = {"stats": [], "pct": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for rep in range(REPS + 2):                                    # (two windows of each to warm up)
        for name, fn in (("stats", mean_range), ("pct", percentile)):
            ev[0].record()
            for _ in range(calls):
                assert fn() == api.SGZ_OK
            ev[1].record()
            torch.cuda.synchronize()
            if rep >= 2:
                times[name].append(ev[0].elapsed_time(ev[1]) / calls)
    line_mb = frames * P * 8 / 1e6                                 # graph 0's rows, 8 bytes a value (the .y half rides along)
    _line("stage", {"frames": frames, "k": k, "columns": columns, "P": P, "calls_per_window": calls, "line_rows_MB": round(line_mb, 2),
                    "stats_records_MB": round(columns * P * 24 / 1e6, 3), "pct_records_MB": round(columns * P * 272 / 1e6, 3)}, times)


def feed(seconds):
    cfg = config.cfg2()
    S = int(cfg["sample_rate"] * seconds)
    x = synth.gen(config.CFG2_SEED, int(cfg["sample_rate"]), S, 2)
    raw = np.ascontiguousarray((np.clip(x.T, -1, 1) * 32767.0).astype(np.int16))
    k = 4
    times = {"stats": [], "pct": []}
    streams = {"stats": api.PcmStream(cfg, api.PCM_S16, 2), "pct": api.PcmStream(cfg, api.PCM_S16, 2)}
    for rep in range(REPS + 2):
        for name, st in streams.items():
            st.reset()
            t0 = time.perf_counter()
            if name == "stats":
                out = st.feed_overview_stats(raw, k, flush=True, want_rgba=True, want_stats=True, want_means=True)
            else:
                out = st.feed_overview_pct(raw, k, Q, flush=True, want_rgba=True, want_records=True, want_values=True)
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= 2:
                times[name].append(dt)
    columns = out[0].shape[0]
    for st in streams.values():
        st.close()
    _line("feed", {"seconds": seconds, "k": k, "columns": columns, "P": cfg["axis_points"]}, times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-feed", action="store_true")
    args = ap.parse_args()
    plan = api.Plan(config.cfg2()).upload()
    stage(plan, 348, 4, 200)
    stage(plan, 40000, 40000, 20)
    stage(plan, 40000, 40, 20)
    if not args.skip_feed:
        feed(config.CFG2_SECONDS)


if __name__ == "__main__":
    main()
