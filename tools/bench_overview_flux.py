#!/usr/bin/env python3
"""The flux overview's reduction beside its nearest sibling and the stage that feeds both, on one device in one process:
  sgz_stage_overview_flux (on resident mapped magnitudes; without d_prev, and with it) against sgz_stage_overview_power (records only: the
  same bytes read, existing code, the yardstick) and sgz_stage_mapped for the same frames, at cfg2's shape: stereo, N = 32768, P = 1024,
  348 frames, k = 4.  Then a long input of --long frames of seeded magnitudes (above the 256 MiB the Infinity Cache holds), where the launch
  overhead no longer dominates: flux and power again, and the bytes either must read -- 4 P sides bytes per (frame, pair) -- over the flux
  time as a fraction of the achievable copy rate of the device (6.29 TB/s, a float4 copy).
Device events around windows of CALLS calls, the calls alternating window by window after two warm-up windows of each, the median and the
spread (least .. greatest) of REPS windows, milliseconds per call.  One JSON line per shape.  No bar is set."""
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


def windows(fns, calls):
    import torch
    times = {name: [] for name in fns}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for rep in range(REPS + 2):                                    # (two windows of each to warm up)
        for name, fn in fns.items():
            ev[0].record()
            for _ in range(calls):
                assert fn() == api.SGZ_OK
            ev[1].record()
            torch.cuda.synchronize()
            if rep >= 2:
                times[name].append(ev[0].elapsed_time(ev[1]) / calls)
    return times


def report(shape, frames, calls, times, plan):
    out = {"shape": shape, "frames": frames, "k": K, "P": plan.P, "rows": plan.C * plan.sides, "calls_per_window": calls}
    for name, t in times.items():
        out[name + "_ms"] = round(float(np.median(t)), 4)
        out[name + "_spread_ms"] = [round(min(t), 4), round(max(t), 4)]
    read = frames * plan.C * plan.sides * plan.P * 4
    out["bytes_read"] = read
    out["flux_over_power"] = round(out["flux_ms"] / out["power_ms"], 3)
    out["flux_fraction_of_copy_rate"] = round(read / (out["flux_ms"] * 1e-3) / COPY_RATE, 3)
    out["power_fraction_of_copy_rate"] = round(read / (out["power_ms"] * 1e-3) / COPY_RATE, 3)
    print(json.dumps(out), flush=True)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--long", type=int, default=40000)
    args = ap.parse_args()
    gpu = torch.device("cuda:0")
    cfg = config.cfg2()
    plan = api.Plan(cfg).upload()
    S = int(cfg["sample_rate"] * config.CFG2_SECONDS)
    x = torch.from_numpy(np.ascontiguousarray(synth.gen(config.CFG2_SEED, int(cfg["sample_rate"]), S, 2))).to(gpu)
    L, s = api.lib(), torch.cuda.current_stream().cuda_stream
    rows, P = plan.C * plan.sides, plan.P
    carry_f = torch.empty((rows, 11), dtype=torch.int64, device=gpu)
    carry_p = torch.empty((rows, P, 4), dtype=torch.int64, device=gpu)
    prev = torch.zeros((rows, P), dtype=torch.float32, device=gpu)

    def fns(mapped, frames, with_stage):
        columns = -(-frames // K)
        out_f = torch.empty((columns, rows, 11), dtype=torch.int64, device=gpu)
        out_p = torch.empty((columns, rows, P, 4), dtype=torch.int64, device=gpu)
        d = {"flux": lambda: L.sgz_stage_overview_flux(plan.h, mapped.data_ptr(), frames, K, 0, 1, 0, 0, None, carry_f.data_ptr(), out_f.data_ptr(), s),
             "flux_with_prev": lambda: L.sgz_stage_overview_flux(plan.h, mapped.data_ptr(), frames, K, 0, 1, 0, 0, prev.data_ptr(), carry_f.data_ptr(),
                                                                 out_f.data_ptr(), s),
             "power": lambda: L.sgz_stage_overview_power(plan.h, mapped.data_ptr(), frames, K, 0, 1, 0, carry_p.data_ptr(), None, out_p.data_ptr(), None, s)}
        if with_stage:
            d["stage_mapped"] = lambda: L.sgz_stage_mapped(plan.h, x.data_ptr(), x.stride(0), S, mapped.data_ptr(), s)
        return d, (out_f, out_p)

    mapped = plan.stage_mapped(x)
    frames = mapped.shape[0]
    d, keep = fns(mapped, frames, True)
    report("cfg2", frames, args.calls, windows(d, args.calls), plan)
    del mapped, keep
    gen = torch.Generator(device=gpu).manual_seed(1)
    long_mapped = torch.exp2(torch.rand((args.long, plan.C, plan.sides, P), generator=gen, device=gpu) * 40 - 35)
    d, keep = fns(long_mapped, args.long, False)
    report("long", args.long, max(1, args.calls // 10), windows(d, max(1, args.calls // 10)), plan)


if __name__ == "__main__":
    main()
