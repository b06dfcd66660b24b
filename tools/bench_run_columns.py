"""What the run lane costs (sgz_stage_run_columns; sgz_pcm_stream_set_run).
    python tools/bench_run_columns.py [--reps 15] [--out gpu_out/run_columns.json] [--parent-tree DIR]
  (a) the stage call, cold: 64 Mi samples of two channels (512 MiB: past the 256 MiB Infinity Cache) at m = 128 and 1000 (the tile form)
      and at 4096 and 2^20 (the sliced form) -- 20 launches after 3 warm-ups between events, median, as bytes READ per second -- on four
      signals: `noise` (no runs to speak of), `s16` (16-bit music-like: tones and noise in multiples of 2^-15), `silence` (every sample
      quiet and flat: the all-ones short-cut) and `clipped` (a hard-clipped 16-bit sine: runs of some twenty samples on both rails, the
      case that walks the longest-run loop).  From the same run, on the same buffer: sgz_stage_level_columns at the same m (it reads the
      same bytes as one pair and is this code base's yardstick) and a device-to-device copy by 16-byte accesses
  (b) the stream: one feed of a kept sgz_pcm_stream of cfg2's 60 s of stereo S16, the lane armed at m = 1024 with the default thresholds,
      against the disarmed feed -- alternating, --reps rounds after a warm-up round, wall medians.  The records must be byte-equal to
      tests/run_ref.py on the converted PCM; the tool exits non-zero otherwise
  (c) with --parent-tree, a built checkout of the parent commit: fresh child processes, alternating this tree and the parent's, --rounds
      times each: the disarmed feed of (b) (this file's --feed-child on the tree's own package and library), and the tree's own bench.py
      (--gpus 1 --steps 20 --warmup 5)
Every figure comes from a run on the GPU; the tool refuses to run without one."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("SGZ_BENCH_TREE", HERE)                           # ((c)'s children: the package and library of another checkout)
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(TREE, "tests"))
import numpy as np
import torch

from signalizer_amd import api, config, synth

M = 1024
SIGNALS = ("noise", "s16", "silence", "clipped")


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


def fill(x, signal):
    """x float32 [2][n] on the device, in place"""
    n = x.shape[1]
    if signal == "noise":
        x.normal_(0.0, 0.1)
    elif signal == "silence":
        x.zero_()
    else:
        for d in range(2):                                              # (row by row: no second buffer of the size)
            t = torch.arange(n, dtype=torch.float32, device=x.device)
            if signal == "s16":
                x[d].normal_(0.0, 0.02).add_(0.3 * torch.sin(t * (0.0131 + 0.004 * d))).add_(0.1 * torch.sin(t * 0.00071))
            else:
                x[d].copy_(1.6 * torch.sin((t % 10007.0) * (0.0597 + 0.004 * d)))     # (the argument kept small: fp32 sin of 64 Mi is noise)
            del t
            x[d].mul_(32768.0).round_().clamp_(-32768.0, 32767.0).mul_(2.0 ** -15)


def stream_case():
    cfg = config.cfg2()
    S = int(config.CFG2_SECONDS * 48000)
    sig = synth.gen(config.CFG2_SEED, 48000, S, 2)
    s16 = np.ascontiguousarray(np.clip(np.round(sig.T * 32768.0), -32768, 32767).astype(np.int16))
    F, P = int(api.lib().sgz_num_frames(S, cfg["window_size"], cfg["hop"])), cfg["axis_points"]
    return cfg, S, s16, F, P


def disarmed_feed_ms(reps):
    """the feed of (b) on a stream that never arms a lane: wall milliseconds per rep (what (c)'s children print)"""
    cfg, S, s16, F, P = stream_case()
    out = np.zeros((F, P, 4), np.uint8)
    stream = api.PcmStream(cfg, api.PCM_S16, 2)
    ts = []
    for k in range(reps + 1):                                           # (the first is the warm-up)
        stream.reset()
        t0 = time.perf_counter()
        st, f, _ = stream.feed_into(s16, S, out, None, F, timing=False)
        assert st == 0 and f == F
        if k:
            ts.append((time.perf_counter() - t0) * 1e3)
    stream.close()
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3, help="(c): children per library")
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples", type=int, default=64 << 20, help="samples per channel of the cold buffer")
    ap.add_argument("--skip-stream", action="store_true", help="(a) alone")
    ap.add_argument("--skip-cold", action="store_true", help="without (a)")
    ap.add_argument("--parent-tree", default=None, help="(c): a built checkout of the parent commit")
    ap.add_argument("--feed-child", action="store_true", help="(internal) print the disarmed feed's milliseconds and exit")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if a.feed_child:
        print(json.dumps(disarmed_feed_ms(a.reps)))
        return
    dev = torch.device("cuda:0")
    switch, tile = api.run_columns_limits()
    level_switch, _ = api.level_columns_limits()
    params = api.run_params_default()
    res = {"device": torch.cuda.get_device_name(0), "switch_over": switch, "tile_samples": tile, "level_switch_over": level_switch,
           "hot": params.hot, "quiet": params.quiet}

    # (a)
    if not a.skip_cold:
        n = a.samples
        read = 2 * n * 4
        x = torch.empty((2, n), dtype=torch.float32, device=dev)
        fill(x, "noise")
        y = torch.empty_like(x)
        ms = events(lambda: y.copy_(x))
        res["a_copy"] = {"ms": round(ms, 4), "bytes_read": read, "read_tb_per_s": round(read / ms / 1e9, 3)}
        del y
        res["a_cold"] = {}
        carry = torch.zeros(2 * 112, dtype=torch.uint8, device=dev)
        level_carry = torch.zeros(80, dtype=torch.uint8, device=dev)
        for signal in SIGNALS:
            fill(x, signal)
            rows = {}
            for m in (128, 1000, 4096, 1 << 20):
                columns = -(-n // m)
                runs = torch.empty((columns, 2, 96), dtype=torch.uint8, device=dev)
                level = torch.empty((columns, 1, 80), dtype=torch.uint8, device=dev)

                def call():
                    st = api.stage_run_columns(x, n, 2, n, params, m, 0, True, False, 0, carry, runs)
                    assert st == 0, st

                def level_call():
                    st = api.stage_level_columns(x, n, 1, n, m, 0, True, 0, level_carry, level)
                    assert st == 0, st
                ms, level_ms = events(call), events(level_call)
                words = runs.view(torch.int32).view(columns * 2, 24)
                rows[str(m)] = {"form": "tile" if m <= switch else "sliced", "ms": round(ms, 4), "bytes_read": read, "bytes_written": runs.numel(),
                                "read_tb_per_s": round(read / ms / 1e9, 3), "of_copy": round(res["a_copy"]["ms"] / ms, 3),
                                "longest_hot": int(words[:, 6].max().item()), "longest_quiet": int(words[:, 12].max().item()),
                                "longest_flat": int(words[:, 18].max().item()),
                                "level_ms": round(level_ms, 4), "level_read_tb_per_s": round(read / level_ms / 1e9, 3), "of_level": round(level_ms / ms, 3)}
                del runs, level, words
            res["a_cold"][signal] = rows
        del x

    # (b)
    equal = True
    if not a.skip_stream:
        import run_ref as rr
        cfg, S, s16, F, P = stream_case()
        out = np.zeros((F, P, 4), np.uint8)
        run_out = np.zeros((-(-S // M), 2), api.RUN_DTYPE)
        stream = api.PcmStream(cfg, api.PCM_S16, 2)

        def feed(way):
            stream.reset()
            stream.set_run(params if way == "armed" else None, M if way == "armed" else 0, run_out if way == "armed" else None)
            t0 = time.perf_counter()
            st, f, _ = stream.feed_into(s16, S, out, None, F, timing=False)
            assert st == 0 and f == F
            if way == "armed":
                stream.flush_run()                                     # (the armed way pays for its flush)
            return (time.perf_counter() - t0) * 1e3

        ways = ("armed", "disarmed")
        for way in ways:                                               # the warm-up round
            feed(way)
        planar = np.ascontiguousarray(s16.reshape(S, 2).T).astype(np.float32) * np.float32(2.0 ** -15)
        equal = run_out.tobytes() == rr.records(planar, M, (params.hot, params.quiet))[0].tobytes()
        image = out.copy()
        ts = {way: [] for way in ways}
        for _ in range(a.reps):
            for way in ways:
                ts[way].append(feed(way))
                assert np.array_equal(out, image)
        stream.close()
        med = {way: statistics.median(ts[way]) for way in ways}
        res["b_stream"] = {"samples": S, "m": M, "reps": a.reps, "records_equal": bool(equal),
                           "armed_ms": round(med["armed"], 3), "disarmed_ms": round(med["disarmed"], 3),
                           "min_max_ms": {way: [round(min(ts[way]), 3), round(max(ts[way]), 3)] for way in ways},
                           "armed_over_disarmed": round(med["armed"] / med["disarmed"], 4)}

    # (c)
    if a.parent_tree:
        libs = {"this": HERE, "parent": os.path.abspath(a.parent_tree)}
        feeds, lines = {k: [] for k in libs}, {k: [] for k in libs}
        for _ in range(a.rounds):
            for which, path in libs.items():
                env = dict(os.environ, SGZ_BENCH_TREE=path)
                child = subprocess.run([sys.executable, os.path.abspath(__file__), "--feed-child", "--reps", str(a.reps)], env=env, capture_output=True,
                                       text=True, timeout=300, check=True)
                feeds[which].append(statistics.median(json.loads(child.stdout.strip().splitlines()[-1])))
                child = subprocess.run([sys.executable, os.path.join(path, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=path,
                                       capture_output=True, text=True, timeout=300, check=True)
                line = json.loads(child.stdout.strip().splitlines()[-1])
                lines[which].append({k: line[k] for k in ("value", "unit", "ms_per_step")})
        res["c_parent"] = {"rounds": a.rounds, "disarmed_feed_ms": {k: [round(v, 3) for v in feeds[k]] for k in libs}, "bench_lines": lines}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")
    assert equal, "the lane's records differ from tests/run_ref.py on the converted PCM"


if __name__ == "__main__":
    main()
