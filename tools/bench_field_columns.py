"""What the stereo-field lane costs (sgz_stage_field_columns; sgz_pcm_stream_set_field).
    python tools/bench_field_columns.py [--reps 15] [--out gpu_out/field_columns.json]
  (a) the stage call, cold: 64 Mi stereo sample frames (512 MiB: past the 256 MiB Infinity Cache) at m = 64, at the switch-over (the tile
      form) and at 4096 and 2^20 (the sliced form) -- 20 launches after 3 warm-ups between events, median, as bytes READ per second -- on
      two signals: `diffuse` (independent noise left and right: every sector) and `mono` (left = right: every frame in sector 16, the
      case that serialises a histogram of LDS adds).  From the same run, on the same buffer: sgz_stage_level_columns at the same m (it
      reads the same bytes and is this code base's yardstick) and a device-to-device copy by 16-byte accesses
  (b) the stream: one feed of a kept sgz_pcm_stream of cfg2's 60 s of stereo S16, the lane armed at m = 1024, against the disarmed feed
      and against the only way to the same records without the lane: the disarmed feed plus tests/field_ref.py in numpy on the host --
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

import field_ref as fr
from signalizer_amd import api, config, synth

M = 1024


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples", type=int, default=64 << 20, help="sample frames of the cold buffer")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    switch, tile = api.field_columns_limits()
    level_switch, _ = api.level_columns_limits()
    res = {"device": torch.cuda.get_device_name(0), "switch_over": switch, "tile_samples": tile, "level_switch_over": level_switch}

    # (a)
    n = a.samples
    read = 2 * n * 4
    x = 0.25 * torch.randn((2, n), dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    ms = events(lambda: y.copy_(x))
    res["a_copy"] = {"ms": round(ms, 4), "bytes_read": read, "read_tb_per_s": round(read / ms / 1e9, 3)}
    del y
    res["a_cold"] = {}
    carry = torch.zeros(528, dtype=torch.uint8, device=dev)
    level_carry = torch.zeros(80, dtype=torch.uint8, device=dev)
    for signal in ("diffuse", "mono"):
        if signal == "mono":
            x[1].copy_(x[0])
        rows = {}
        for m in (64, switch, 4096, 1 << 20):
            columns = -(-n // m)
            field = torch.empty((columns, 1, 528), dtype=torch.uint8, device=dev)
            level = torch.empty((columns, 1, 80), dtype=torch.uint8, device=dev)

            def call():
                st = api.stage_field_columns(x, n, 1, n, m, 0, True, 0, carry, field)
                assert st == 0, st

            def level_call():
                st = api.stage_level_columns(x, n, 1, n, m, 0, True, 0, level_carry, level)
                assert st == 0, st
            ms, level_ms = events(call), events(level_call)
            used = int((field.view(torch.int32).view(columns, 132)[:, 64:96].sum(dim=0) != 0).sum().item())       # sectors with a frame
            rows[str(m)] = {"form": "tile" if m <= switch else "sliced", "ms": round(ms, 4), "bytes_read": read, "bytes_written": field.numel(),
                            "read_gb_per_s": round(read / ms / 1e6, 1), "of_copy": round(res["a_copy"]["ms"] / ms, 3), "sectors_used": used,
                            "level_form": "tile" if m <= level_switch else "sliced", "level_ms": round(level_ms, 4),
                            "level_read_gb_per_s": round(read / level_ms / 1e6, 1), "of_level": round(level_ms / ms, 3)}
            del field, level
        res["a_cold"][signal] = rows
    del x

    # (b)
    cfg = config.cfg2()
    S = int(config.CFG2_SECONDS * 48000)
    sig = synth.gen(config.CFG2_SEED, 48000, S, 2)
    s16 = np.ascontiguousarray(np.clip(np.round(sig.T * 32768.0), -32768, 32767).astype(np.int16))
    F, P = int(api.lib().sgz_num_frames(S, cfg["window_size"], cfg["hop"])), cfg["axis_points"]
    out = np.zeros((F, P, 4), np.uint8)
    field_out = np.zeros((-(-S // M), 1), api.FIELD_DTYPE)
    stream = api.PcmStream(cfg, api.PCM_S16, 2)
    interleaved = s16.reshape(S, 2)

    def feed(way):
        stream.reset()
        stream.set_field(M if way == "armed" else 0, field_out if way == "armed" else None)
        t0 = time.perf_counter()
        st, f, _ = stream.feed_into(s16, S, out, None, F, timing=False)
        assert st == 0 and f == F
        records = None
        if way == "armed":
            stream.flush_field()                                       # (the armed way pays for its flush)
        elif way == "numpy":
            planar = np.ascontiguousarray(interleaved.T).astype(np.float32) * np.float32(2.0 ** -15)
            records = fr.columns(planar, M)[0]
        return (time.perf_counter() - t0) * 1e3, records

    ways = ("armed", "disarmed", "numpy")
    records = None
    for way in ways:                                                   # the warm-up round
        _, r = feed(way)
        records = r if r is not None else records
    equal = field_out.tobytes() == np.ascontiguousarray(records, api.FIELD_DTYPE).tobytes()
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
    assert equal, "the lane's records differ from tests/field_ref.py on the converted PCM"


if __name__ == "__main__":
    main()
