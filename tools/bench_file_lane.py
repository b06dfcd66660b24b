#!/usr/bin/env python3
"""The file lane: cfg2's 60 s buffer at the reference's default hop of 200 samples (14 237 frames) as interleaved stereo S16, medians of 7
wall times on one device in one run, event times beside them.
  (a) the streamed overview, sgz_pcm_stream_feed_overview on a kept stream at k = 8 and k = 64, against the way to that picture without
      it: sgz_pcm_stream_feed (image only, every column read back) + a numpy reduction of those columns (a maximum over every k columns:
      the work of that size; the picture itself needs the line results) -- entry points this change leaves as they were -- and beside
      sgz_spectrogram_overview_host from planar floats;
  (b) a redraw: sgz_stage_overview_view from device-resident k = 8 peaks (1780 columns) to 223 columns + its read-back, and
      sgz_overview_view_host from host peaks, against the only way to another zoom without them: sgz_spectrogram_overview_host at k = 64.
Exit status 1 unless the streamed overview is more than 5 % below its parent at both k and both redraws more than 5 % below theirs.
  --sweep     the stage call alone, 100 000 -> 16 columns of P = 1024 (and 1780 -> 223), slices 0 (automatic), 1, 2, 4 .. 64: event-timed
  --kernels   a few views and nothing else, for a kernel trace of a run of its own
One JSON line per result."""
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
HOP = 200


def median_ms(fn, reps=REPS, warmup=2):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), [round(t, 3) for t in times]


def buffer(seconds):
    cfg = config.spectrum_config(hop=HOP)
    S = int(cfg["sample_rate"] * seconds)
    x = synth.gen(config.CFG2_SEED, int(cfg["sample_rate"]), S, 2)
    pcm = np.clip(np.round(x.T.astype(np.float64) * 32768.0), -32768, 32767).astype("<i2").reshape(-1)      # interleaved
    planar = np.ascontiguousarray((pcm.astype(np.float32) * np.float32(2.0 ** -15)).reshape(-1, 2).T)
    return cfg, pcm, planar


def run_lane(seconds):
    import torch
    cfg, pcm, planar = buffer(seconds)
    plan = api.Plan(cfg).upload()
    F, P = plan.num_frames(planar.shape[1]), plan.P
    stream = api.PcmStream(cfg, api.PCM_S16, 2)
    ok = True
    rgba = np.zeros((F, P, 4), np.uint8)

    for k in (8, 64):
        columns = -(-F // k)

        def parent():
            stream.reset()
            st, f, _ = stream.feed_into(pcm, planar.shape[1], rgba, None, F, timing=False)
            assert st == api.SGZ_OK and f == F
            pad = np.zeros((columns * k - F, P, 4), np.uint8)
            return np.concatenate([rgba, pad]).reshape(columns, k, P, 4).max(axis=1)

        def streamed():
            stream.reset()
            return stream.feed_overview(pcm, k, flush=True)

        p_ms, p_all = median_ms(parent)
        s_ms, s_all = median_ms(streamed)
        h_ms, _ = median_ms(lambda: plan.overview(planar, k))
        image, _, timing = streamed()
        same = bool(np.array_equal(image, plan.overview(planar, k)[0]))
        ok = ok and s_ms < 0.95 * p_ms and same
        print(json.dumps({"run": "a", "k": k, "columns": columns, "parent_feed_plus_numpy_ms": round(p_ms, 3), "parent_all_ms": p_all,
                          "streamed_overview_ms": round(s_ms, 3), "streamed_all_ms": s_all, "overview_host_from_planar_ms": round(h_ms, 3),
                          "streamed_over_parent": round(s_ms / p_ms, 4), "equals_overview_host": same,
                          "stage_ms": {n: round(timing[n], 3) for n in ("h2d_ms", "convert_ms", "render_ms", "d2h_ms")}, "chunks": timing["chunks"]}), flush=True)

    # (b) a redraw from kept k = 8 peaks
    _, peaks, _ = plan.overview(planar, 8, want_rgba=False, want_peaks=True)
    n, out = peaks.shape[0], -(-F // 64)
    d_peaks = torch.from_numpy(peaks).to("cuda:0")
    direct, _, _ = plan.overview(planar, 64)

    def view_device():
        image, _ = plan.overview_view(d_peaks, out)
        return image.cpu().numpy()

    r_ms, r_all = median_ms(lambda: plan.overview(planar, 64))
    d_ms, d_all = median_ms(view_device)
    v_ms, v_all = median_ms(lambda: plan.overview_view(peaks, out))
    _, _, timing = plan.overview_view(peaks, out)
    # (1780 is no multiple of 8: the timed view's boundaries ceil(b 1780 / 223) are not the direct render's; the 222 whole columns are)
    whole = n // 8
    same = bool(np.array_equal(plan.overview_view(d_peaks, whole, x1=8 * whole)[0].cpu().numpy(), direct[:whole])) and \
        bool(np.array_equal(plan.overview_view(peaks, whole, x1=8 * whole)[0], direct[:whole]))
    ok = ok and d_ms < 0.95 * r_ms and v_ms < 0.95 * r_ms and same
    print(json.dumps({"run": "b", "source_columns": n, "columns": out, "parent_overview_host_k64_ms": round(r_ms, 3), "parent_all_ms": r_all,
                      "view_device_plus_read_back_ms": round(d_ms, 3), "view_device_all_ms": d_all, "view_host_ms": round(v_ms, 3), "view_host_all_ms": v_all,
                      "view_host_stage_ms": {k: round(timing[k], 3) for k in ("h2d_ms", "kernel_ms", "d2h_ms")},
                      "whole_columns_equal_overview_host_k64": same}), flush=True)
    return ok


def run_sweep():
    import torch
    gpu = torch.device("cuda:0")
    plan = api.Plan(config.spectrum_config(hop=HOP)).upload()
    P = plan.P
    for n, out in ((1780, 223), (100000, 16)):
        peaks = torch.rand((n, 1, P), dtype=torch.float32, device=gpu)
        want = None
        for slices in (0, 1, 2, 4, 8, 16, 32, 64):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            times = []
            for rep in range(REPS + 2):
                ev[0].record()
                rgba, _ = plan.overview_view(peaks, out, slices=slices)
                ev[1].record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times.append(ev[0].elapsed_time(ev[1]) * 1e3)
            got = rgba.cpu().numpy()
            want = got if want is None else want
            print(json.dumps({"run": "sweep", "source_columns": n, "columns": out, "slices": slices, "us": round(float(np.median(times)), 2),
                              "bytes_read": n * P * 4, "bytes_written": out * P * 4, "same_image": bool(np.array_equal(got, want))}), flush=True)


def run_kernels():
    import torch
    plan = api.Plan(config.spectrum_config(hop=HOP)).upload()
    for n, out in ((1780, 223), (100000, 16)) * 3:
        plan.overview_view(torch.rand((n, 1, plan.P), dtype=torch.float32, device="cuda:0"), out)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=config.CFG2_SECONDS)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    if args.kernels:
        run_kernels()
    elif args.sweep:
        run_sweep()
    elif not run_lane(args.seconds):
        sys.exit(1)


if __name__ == "__main__":
    main()
