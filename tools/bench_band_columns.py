"""What the band lane costs (sgz_stage_band_columns; sgz_pcm_stream_set_band).
    python tools/bench_band_columns.py [--reps 20] [--parent-tree /a/built/checkout/of/the/parent/commit] [--out gpu_out/band_columns.json]
  (a) the stage call, cold: 64 Mi stereo samples (512 MiB: past the 256 MiB Infinity Cache) with the 48 kHz crossover (300 / 3000 Hz, W = 1024,
      L = 64) at m = 64, 1024, 4096 and 2^20 -- 20 launches after 3 warm-ups between events, median, as bytes READ per second; from the same
      run on the same buffer the yardstick, sgz_stage_loudness_columns with its helper's filter (W = 4096, L = 256), and a device-to-device
      copy of the buffer.  No bar.
  (b) the stream: one feed of a kept sgz_pcm_stream of cfg2's 60 s of stereo S16, pageable memory, the lane armed at m = 1024, against the
      disarmed feed of the same process, alternating, --reps pairs after 3 warm-up pairs, wall medians; and once the disarmed feed plus
      tests/band_ref.py computing the same records with numpy from the PCM (the records must be byte-equal; the tool exits non-zero
      otherwise)
  (c) with --parent-tree: the same loop in fresh processes of this tree alternating with the disarmed feed in fresh processes of this tree
      that never arm the lane and of a built checkout of the parent commit (--tree)
--kernels M: nothing but three stage calls at that m on the cold buffer, for a counter run (rocprofv3 --pmc, nothing else traced).
Every figure comes from a run on the GPU; the tool refuses to run without one."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = HERE
if "--tree" in sys.argv[1:-1]:                                          # (a child of (c): the package of another checkout)
    TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, TREE)
sys.path.insert(1, os.path.join(HERE, "tests"))
import numpy as np
import torch

from signalizer_amd import api, config, synth

M = 1024
RATE = 48000


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


def cfg2_s16():
    cfg = config.cfg2()
    S = int(config.CFG2_SECONDS * RATE)
    sig = synth.gen(config.CFG2_SEED, RATE, S, 2)
    s16 = np.ascontiguousarray(np.clip(np.round(sig.T * 32768.0), -32768, 32767).astype(np.int16))
    F, P = int(api.lib().sgz_num_frames(S, cfg["window_size"], cfg["hop"])), cfg["axis_points"]
    return cfg, S, s16, F, P


def host_records(s16, f, m):
    """the lane's records of interleaved stereo S16 [S][2] by tests/band_ref.py on the PCM's integers (v = sample << 8)"""
    import band_ref as br
    v = np.ascontiguousarray(s16.T).astype(np.int64) << 8
    return br.records_of_integers(v, np.ones(v.shape, bool), f, m)[0]


def feed_medians(reps, never_armed=False):
    """wall medians of a kept stream's feed with the package that was imported (--tree): disarmed and, where the package has the lane, armed
    at m = 1024, alternating, nothing else between the feeds; the armed flush of the open column apart"""
    cfg, S, s16, F, P = cfg2_s16()
    out = np.zeros((F, P, 4), np.uint8)
    stream = api.PcmStream(cfg, api.PCM_S16, 2)
    has_lane = hasattr(stream, "set_band") and not never_armed
    f = api.band_filter_for_rate(RATE) if has_lane else None
    lane_out = np.zeros((-(-S // M), 2), api.BAND_DTYPE) if has_lane else None
    ts, flushes = {True: [], False: []}, []
    for k in range(reps + 3):
        for armed in ((True, False) if has_lane else (False,)):
            stream.reset()
            if has_lane:
                stream.set_band(f if armed else None, M if armed else 0, lane_out if armed else None)
            t0 = time.perf_counter()
            st, fr, _ = stream.feed_into(s16, S, out, None, F, timing=False)
            t1 = time.perf_counter()
            assert st == 0 and fr == F
            if armed:
                stream.flush_band()
                flushes.append((time.perf_counter() - t1) * 1e3)
            ts[armed].append((t1 - t0) * 1e3)
    stream.close()
    res = {"disarmed_ms": statistics.median(ts[False][3:]), "disarmed_min_max_ms": [min(ts[False][3:]), max(ts[False][3:])]}
    if has_lane:
        res.update(armed_ms=statistics.median(ts[True][3:]), armed_min_max_ms=[min(ts[True][3:]), max(ts[True][3:])], flush_ms=statistics.median(flushes[3:]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(HERE, "gpu_out", "band_columns.json"), help="where the JSON line goes ('' for nowhere)")
    ap.add_argument("--samples", type=int, default=64 << 20, help="samples per channel of the cold buffer")
    ap.add_argument("--kernels", type=int, default=0, help="only three stage calls at this m, for a counter run")
    ap.add_argument("--skip-host", action="store_true", help="leave the numpy comparison of (b) out")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit, for (c)'s process-alternating comparison")
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--never-armed", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if a.child:
        print(json.dumps(feed_medians(a.reps, a.never_armed)))
        return
    dev = torch.device("cuda:0")
    f = api.band_filter_for_rate(RATE)
    kf = api.loudness_filter_for_rate(RATE)
    switch, tile, carry_bytes = api.band_columns_limits(f, 2)
    res = {"device": torch.cuda.get_device_name(0), "W": f.W, "L": f.L, "switch_over": switch, "tile_samples": tile, "carry_bytes": carry_bytes,
           "loudness_W": kf.W, "loudness_L": kf.L}

    n = a.samples
    x = torch.randn((2, n), dtype=torch.float32, device=dev) * 0.3
    bd_carry = torch.zeros(carry_bytes, dtype=torch.uint8, device=dev)
    if a.kernels:
        records = torch.empty((-(-n // a.kernels), 2, 64), dtype=torch.uint8, device=dev)
        for _ in range(3):
            assert api.stage_band_columns(x, n, 2, n, f, 0, a.kernels, 0, True, False, 0, bd_carry, records) == 0
        torch.cuda.synchronize()
        return

    # (a)
    y = torch.empty_like(x)
    read = 2 * n * 4
    ms = events(lambda: y.copy_(x))
    res["a_copy"] = {"ms": round(ms, 4), "bytes_read": read, "read_tb_per_s": round(read / ms / 1e9, 3)}
    del y
    res["a_cold"] = {}
    ld_carry = torch.zeros(api.loudness_columns_limits(kf, 2)[2], dtype=torch.uint8, device=dev)
    for m in (64, 1024, 4096, 1 << 20):
        records = torch.empty((-(-n // m), 2, 64), dtype=torch.uint8, device=dev)
        loud = torch.empty((-(-n // m), 2, 32), dtype=torch.uint8, device=dev)

        def call():
            st = api.stage_band_columns(x, n, 2, n, f, 0, m, 0, True, False, 0, bd_carry, records)
            assert st == 0, st

        def loud_call():
            st = api.stage_loudness_columns(x, n, 2, n, kf, 0, m, 0, True, False, 0, ld_carry, loud)
            assert st == 0, st
        ms, loud_ms = events(call), events(loud_call)
        res["a_cold"][str(m)] = {"ms": round(ms, 4), "bytes_read": read, "read_tb_per_s": round(read / ms / 1e9, 3),
                                 "msamples_per_s": round(2 * n / ms / 1e3, 1), "of_copy": round(res["a_copy"]["ms"] / ms, 3),
                                 "loudness_ms": round(loud_ms, 4), "of_loudness_rate": round(loud_ms / ms, 3), "form": "tile" if m <= switch else "sliced"}
        del records, loud
    del x

    # (b)
    cfg, S, s16, F, P = cfg2_s16()
    own = feed_medians(a.reps)
    r3 = lambda v: [round(x, 3) for x in v] if isinstance(v, list) else round(v, 3)      # noqa: E731
    res["b_stream"] = {k: r3(v) for k, v in own.items()}
    res["b_stream"].update(samples=S, m=M, reps=a.reps, armed_over_disarmed=round(own["armed_ms"] / own["disarmed_ms"], 4))
    equal = True
    if not a.skip_host:
        out = np.zeros((F, P, 4), np.uint8)
        lane_out = np.zeros((-(-S // M), 2), api.BAND_DTYPE)
        stream = api.PcmStream(cfg, api.PCM_S16, 2)
        stream.set_band(f, M, lane_out)
        st, fr, _ = stream.feed_into(s16, S, out, None, F, timing=False)
        assert st == 0 and fr == F
        stream.flush_band()
        stream.close()
        t0 = time.perf_counter()
        records = host_records(np.ascontiguousarray(s16).reshape(S, 2), f, M)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        equal = lane_out.tobytes() == np.ascontiguousarray(records, api.BAND_DTYPE).tobytes()
        res["b_stream"].update(numpy_ms=round(numpy_ms, 1), disarmed_plus_numpy_ms=round(numpy_ms + own["disarmed_ms"], 1), records_equal=bool(equal))
    # (c)
    res["c_against_parent_build"] = "not measured"
    if a.parent_tree:
        runs = {"this": [], "this_never_armed": [], "parent": []}
        for _ in range(3):
            for which, tree in (("this", TREE), ("this_never_armed", TREE), ("parent", os.path.abspath(a.parent_tree))):
                got = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--tree", tree]
                                     + (["--never-armed"] if which == "this_never_armed" else []), capture_output=True, text=True, timeout=300, check=True)
                runs[which].append(json.loads(got.stdout.strip().splitlines()[-1]))
        this_d, this_a = [r["disarmed_ms"] for r in runs["this"]], [r["armed_ms"] for r in runs["this"]]
        parent = [r["disarmed_ms"] for r in runs["parent"]]
        never = [r["disarmed_ms"] for r in runs["this_never_armed"]]
        res["c_against_parent_build"] = {"parent_ms": r3(parent), "this_disarmed_ms": r3(this_d), "this_armed_ms": r3(this_a),
                                         "this_never_armed_ms": r3(never),
                                         "never_armed_over_parent": round(statistics.median(never) / statistics.median(parent), 4),
                                         "disarmed_over_parent": round(statistics.median(this_d) / statistics.median(parent), 4),
                                         "armed_over_parent": round(statistics.median(this_a) / statistics.median(parent), 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")
    assert equal, "the lane's records differ from numpy's on the PCM"


if __name__ == "__main__":
    main()
