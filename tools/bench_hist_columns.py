"""What the histogram lane costs (sgz_stage_hist_columns; sgz_pcm_stream_set_hist).
    python tools/bench_hist_columns.py [--reps 15] [--out gpu_out/hist_columns.json]
  (a) the stage call, cold: 64 Mi samples of two channels (512 MiB: past the 256 MiB Infinity Cache) at m = 128 and 1000 (the tile form)
      and at 4096 and 2^20 (the sliced form) -- 20 launches after 3 warm-ups between events, median, as bytes READ per second -- on four
      signals: `noise` (some 49 buckets), `s16` (16-bit music-like: tones and noise in multiples of 2^-15), `silence` (every sample in
      bucket 0: the case that serialises a histogram of LDS adds and that the pre-fold takes out) and `two_level` (two buckets in
      alternation: half of every wave on one table word).  From the same run, on the same buffer: sgz_stage_level_columns and
      sgz_stage_field_columns at the same m (they read the same bytes as one pair and are this code base's yardsticks) and a
      device-to-device copy by 16-byte accesses
  (b) the stream: one feed of a kept sgz_pcm_stream of cfg2's 60 s of stereo S16, the lane armed at m = 1024, against the disarmed feed
      and against the only way to the same records without the lane: the disarmed feed plus tests/hist_ref.py in numpy on the host --
      alternating, --reps rounds after a warm-up round, wall medians.  The records must be byte-equal; the tool exits non-zero otherwise
Every figure comes from a run on the GPU; the tool refuses to run without one."""
import argparse
import json
import os
import statistics
import sys
import time

TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(TREE, "tests"))
import numpy as np
import torch

import hist_ref as hr
from signalizer_amd import api, config, synth

M = 1024
SIGNALS = ("noise", "s16", "silence", "two_level")


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
    elif signal == "s16":
        for d in range(2):                                              # (row by row: no second buffer of the size)
            t = torch.arange(n, dtype=torch.float32, device=x.device)
            x[d].normal_(0.0, 0.02).add_(0.3 * torch.sin(t * (0.0131 + 0.004 * d))).add_(0.1 * torch.sin(t * 0.00071))
            del t
            x[d].mul_(32768.0).round_().clamp_(-32768.0, 32767.0).mul_(2.0 ** -15)
    elif signal == "silence":
        x.zero_()
    else:
        x.fill_(-(2.0 ** -10))
        x[:, 0::2] = 0.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples", type=int, default=64 << 20, help="samples per channel of the cold buffer")
    ap.add_argument("--skip-stream", action="store_true", help="(a) alone")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    switch, tile = api.hist_columns_limits()
    level_switch, _ = api.level_columns_limits()
    field_switch, _ = api.field_columns_limits()
    res = {"device": torch.cuda.get_device_name(0), "switch_over": switch, "tile_samples": tile, "level_switch_over": level_switch,
           "field_switch_over": field_switch}

    # (a)
    n = a.samples
    read = 2 * n * 4
    x = torch.empty((2, n), dtype=torch.float32, device=dev)
    fill(x, "noise")
    y = torch.empty_like(x)
    ms = events(lambda: y.copy_(x))
    res["a_copy"] = {"ms": round(ms, 4), "bytes_read": read, "read_tb_per_s": round(read / ms / 1e9, 3)}
    del y
    res["a_cold"] = {}
    carry = torch.zeros(2 * 448, dtype=torch.uint8, device=dev)
    level_carry = torch.zeros(80, dtype=torch.uint8, device=dev)
    field_carry = torch.zeros(528, dtype=torch.uint8, device=dev)
    for signal in SIGNALS:
        fill(x, signal)
        rows = {}
        for m in (128, 1000, 4096, 1 << 20):
            columns = -(-n // m)
            hist = torch.empty((columns, 2, 448), dtype=torch.uint8, device=dev)
            level = torch.empty((columns, 1, 80), dtype=torch.uint8, device=dev)
            field = torch.empty((columns, 1, 528), dtype=torch.uint8, device=dev)

            def call():
                st = api.stage_hist_columns(x, n, 2, n, m, 0, True, 0, carry, hist)
                assert st == 0, st

            def level_call():
                st = api.stage_level_columns(x, n, 1, n, m, 0, True, 0, level_carry, level)
                assert st == 0, st

            def field_call():
                st = api.stage_field_columns(x, n, 1, n, m, 0, True, 0, field_carry, field)
                assert st == 0, st
            ms, level_ms, field_ms = events(call), events(level_call), events(field_call)
            used = int((hist.view(torch.int32).view(columns * 2, 112)[:, :106].sum(dim=0) != 0).sum().item())       # buckets with a sample
            rows[str(m)] = {"form": "tile" if m <= switch else "sliced", "ms": round(ms, 4), "bytes_read": read, "bytes_written": hist.numel(),
                            "read_tb_per_s": round(read / ms / 1e9, 3), "of_copy": round(res["a_copy"]["ms"] / ms, 3), "buckets_used": used,
                            "level_ms": round(level_ms, 4), "level_read_tb_per_s": round(read / level_ms / 1e9, 3), "of_level": round(level_ms / ms, 3),
                            "field_ms": round(field_ms, 4), "field_read_tb_per_s": round(read / field_ms / 1e9, 3), "of_field": round(field_ms / ms, 3)}
            del hist, level, field
        res["a_cold"][signal] = rows
    del x

    # (b)
    equal = True
    if not a.skip_stream:
        cfg = config.cfg2()
        S = int(config.CFG2_SECONDS * 48000)
        sig = synth.gen(config.CFG2_SEED, 48000, S, 2)
        s16 = np.ascontiguousarray(np.clip(np.round(sig.T * 32768.0), -32768, 32767).astype(np.int16))
        F, P = int(api.lib().sgz_num_frames(S, cfg["window_size"], cfg["hop"])), cfg["axis_points"]
        out = np.zeros((F, P, 4), np.uint8)
        hist_out = np.zeros((-(-S // M), 2), api.HIST_DTYPE)
        stream = api.PcmStream(cfg, api.PCM_S16, 2)
        interleaved = s16.reshape(S, 2)

        def feed(way):
            stream.reset()
            stream.set_hist(M if way == "armed" else 0, hist_out if way == "armed" else None)
            t0 = time.perf_counter()
            st, f, _ = stream.feed_into(s16, S, out, None, F, timing=False)
            assert st == 0 and f == F
            records = None
            if way == "armed":
                stream.flush_hist()                                    # (the armed way pays for its flush)
            elif way == "numpy":
                planar = np.ascontiguousarray(interleaved.T).astype(np.float32) * np.float32(2.0 ** -15)
                records = hr.columns(planar, M)[0]
            return (time.perf_counter() - t0) * 1e3, records

        ways = ("armed", "disarmed", "numpy")
        records = None
        for way in ways:                                               # the warm-up round
            _, r = feed(way)
            records = r if r is not None else records
        equal = hist_out.tobytes() == np.ascontiguousarray(records, api.HIST_DTYPE).tobytes()
        image = out.copy()
        ts = {way: [] for way in ways}
        for _ in range(a.reps):
            for way in ways:
                ts[way].append(feed(way)[0])
                assert np.array_equal(out, image)
        stream.close()
        med = {way: statistics.median(ts[way]) for way in ways}
        res["b_stream"] = {"samples": S, "m": M, "reps": a.reps, "records_equal": bool(equal),
                           "armed_ms": round(med["armed"], 3), "disarmed_ms": round(med["disarmed"], 3), "disarmed_plus_numpy_ms": round(med["numpy"], 3),
                           "min_max_ms": {way: [round(min(ts[way]), 3), round(max(ts[way]), 3)] for way in ways},
                           "armed_over_disarmed": round(med["armed"] / med["disarmed"], 4), "armed_over_numpy_way": round(med["armed"] / med["numpy"], 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")
    assert equal, "the lane's records differ from tests/hist_ref.py on the converted PCM"


if __name__ == "__main__":
    main()
