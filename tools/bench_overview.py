#!/usr/bin/env python3
"""The overview render against the parent's two ways to the same picture: cfg2's 60 s buffer at the reference's default hop of 200 samples
(14 237 frames), k = 8 and k = 64 frames per column, medians of 7 wall times on one device in one run:
  (a) sgz_spectrogram_render_host, image only, on a kept plan            -- a picture, one column per frame
  (b) the same with lines_out + the numpy reduction (tests/overview_ref.py) -- this picture's peaks, the parent's way
  (c) sgz_spectrogram_overview_host
Exit status 1 if (c) is not below (a) by more than 5 % at both k.
  --sweep     the stage call alone on 16 columns of P = 1024 (k = frames / 16), slices 0 (automatic), 1, 2, 4 .. 64: event-timed medians
  --kernels   a few overview renders and nothing else, for a kernel trace of a run of its own
One JSON line per result."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from signalizer_amd import api, config, synth  # noqa: E402

REPS = 7
HOP = 200


def median_ms(fn, reps=REPS, warmup=2):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), times


def buffer_and_plan(seconds):
    cfg = config.spectrum_config(hop=HOP)
    S = int(cfg["sample_rate"] * seconds)
    x = synth.gen(config.CFG2_SEED, int(cfg["sample_rate"]), S, 2)
    return cfg, x, api.Plan(cfg).upload()


def run_render(seconds):
    import overview_ref as ov
    cfg, x, plan = buffer_and_plan(seconds)
    F, P = plan.num_frames(x.shape[1]), plan.P
    a_ms, _ = median_ms(lambda: api.render_spectrogram_host(plan, x))
    print(json.dumps({"run": "a", "what": "render_host, image only", "frames": F, "ms": round(a_ms, 3), "read_back_bytes": F * P * 4}), flush=True)
    ok = True
    for k in (8, 64):
        columns = -(-F // k)

        def parent():
            _, lines, _ = api.render_spectrogram_host(plan, x, want_lines=True)
            return ov.columns_of(np.ascontiguousarray(lines[:, :, 0, :, 0]), k)[0]

        b_ms, _ = median_ms(parent, reps=3, warmup=1)
        c_ms, c_all = median_ms(lambda: plan.overview(x, k))
        image, peaks, timing = plan.overview(x, k, want_peaks=True)
        same = bool(np.array_equal(peaks.view(np.uint32), parent()))
        ok = ok and c_ms < 0.95 * a_ms and same
        print(json.dumps({"run": "b", "k": k, "what": "render_host with lines_out + numpy reduction", "ms": round(b_ms, 3),
                          "read_back_bytes": F * P * 4 + F * plan.C * api.NUM_GRAPHS * P * 8}), flush=True)
        print(json.dumps({"run": "c", "k": k, "what": "overview_host", "columns": columns, "ms": round(c_ms, 3), "all_ms": [round(t, 3) for t in c_all],
                          "read_back_bytes": columns * P * 4, "stage_ms": {n: round(timing[n], 3) for n in ("h2d_ms", "kernel_ms", "d2h_ms")},
                          "c_over_a": round(c_ms / a_ms, 4), "peaks_equal_parent": same}), flush=True)
    return ok


def run_sweep():
    import torch
    gpu = torch.device("cuda:0")
    plan = api.Plan(config.spectrum_config(hop=HOP)).upload()
    P, columns = plan.P, 16
    for k in (64, 890):
        frames = columns * k
        lines = torch.rand((frames, 1, api.NUM_GRAPHS, P, 2), dtype=torch.float32, device=gpu)
        want = None
        for slices in (0, 1, 2, 4, 8, 16, 32, 64):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            times = []
            for rep in range(REPS + 2):
                ev[0].record()
                rgba, _, _ = plan.overview_columns(lines, k, slices=slices)
                ev[1].record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times.append(ev[0].elapsed_time(ev[1]) * 1e3)
            got = rgba.cpu().numpy()
            want = got if want is None else want
            print(json.dumps({"run": "sweep", "columns": columns, "k": k, "frames": frames, "slices": slices, "us": round(float(np.median(times)), 2),
                              "bytes": frames * P * 8 + columns * P * 4, "same_image": bool(np.array_equal(got, want))}), flush=True)


def run_kernels(seconds):
    cfg, x, plan = buffer_and_plan(seconds)
    for k in (8, 64, 8, 64):
        plan.overview(x, k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=config.CFG2_SECONDS)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    if args.kernels:
        run_kernels(args.seconds)
    elif args.sweep:
        run_sweep()
    elif not run_render(args.seconds):
        sys.exit(1)


if __name__ == "__main__":
    main()
