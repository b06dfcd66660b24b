"""What the true-peak lane costs (sgz_stage_truepeak_columns; sgz_pcm_stream_set_truepeak).
    python tools/bench_truepeak_columns.py [--reps 31] [--parent-tree /a/built/checkout/of/the/parent/commit] [--out gpu_out/truepeak_columns.json]
  (a) the stage call, cold: 64 Mi stereo samples (512 MiB: past the 256 MiB Infinity Cache) at m = 64, 512, 4096 and 2^20 -- 20 launches
      after 3 warm-ups between events, median, as bytes READ per second; from the same run sgz_stage_level_columns and
      sgz_stage_wave_columns on the same buffer and the yardstick, a device-to-device copy of it.  No bar.
  (b) the stream: one feed of a kept sgz_pcm_stream of cfg2's 60 s of stereo S16, pageable memory, the lane armed at m = 512, against the
      only way to the same records without the lane: the disarmed feed plus tests/truepeak_ref.py computing them with numpy from the PCM --
      alternating, --reps pairs after a warm-up pair, wall medians.  The records must be byte-equal and armed < 0.95 x the other way (5 %:
      the box-to-box and run-to-run scatter README.md states); the tool exits non-zero otherwise
  (c) the overhead: armed and disarmed feeds alternating in a loop of their own (the flush of the last, open column is timed apart), and,
      with --parent-tree, the same loop in fresh processes of this tree alternating with the disarmed feed in fresh processes of a built
      checkout of the parent commit (--tree)
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

M = 512


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
    S = int(config.CFG2_SECONDS * 48000)
    sig = synth.gen(config.CFG2_SEED, 48000, S, 2)
    s16 = np.ascontiguousarray(np.clip(np.round(sig.T * 32768.0), -32768, 32767).astype(np.int16))
    F, P = int(api.lib().sgz_num_frames(S, cfg["window_size"], cfg["hop"])), cfg["axis_points"]
    return cfg, S, s16, F, P


def host_records(s16, m):
    """the lane's records of interleaved stereo S16 [S][2] by tests/truepeak_ref.py on the PCM's integers (v = sample << 8) -- what a host
    without the lane computes"""
    import truepeak_ref as tr
    v = np.ascontiguousarray(s16.T).astype(np.int64) << 8
    return tr.records_of_integers(v, np.ones(v.shape, bool), m)[0]


def feed_medians(reps):
    """wall medians of a kept stream's feed with the package that was imported (--tree): disarmed and, where the package has the lane, armed
    at m = 512, alternating, nothing else between the feeds; the armed flush of the open column apart"""
    cfg, S, s16, F, P = cfg2_s16()
    out = np.zeros((F, P, 4), np.uint8)
    stream = api.PcmStream(cfg, api.PCM_S16, 2)
    has_lane = hasattr(stream, "set_truepeak")
    lane_out = np.zeros((-(-S // M), 2), api.TRUEPEAK_DTYPE) if has_lane else None
    ts, flushes = {True: [], False: []}, []
    for k in range(reps + 2):
        for armed in ((True, False) if has_lane else (False,)):
            stream.reset()
            if has_lane:
                stream.set_truepeak(M if armed else 0, lane_out if armed else None)
            t0 = time.perf_counter()
            st, f, _ = stream.feed_into(s16, S, out, None, F, timing=False)
            t1 = time.perf_counter()
            assert st == 0 and f == F
            if armed:
                stream.flush_truepeak()
                flushes.append((time.perf_counter() - t1) * 1e3)
            ts[armed].append((t1 - t0) * 1e3)
    stream.close()
    res = {"disarmed_ms": statistics.median(ts[False][2:]), "disarmed_min_max_ms": [min(ts[False][2:]), max(ts[False][2:])]}
    if has_lane:
        res.update(armed_ms=statistics.median(ts[True][2:]), armed_min_max_ms=[min(ts[True][2:]), max(ts[True][2:])], flush_ms=statistics.median(flushes[2:]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--out", default=os.path.join(HERE, "gpu_out", "truepeak_columns.json"), help="where the JSON line goes ('' for nowhere)")
    ap.add_argument("--samples", type=int, default=64 << 20, help="samples per channel of the cold buffer")
    ap.add_argument("--kernels", type=int, default=0, help="only three stage calls at this m, for a counter run")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit, for (c)'s process-alternating comparison")
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if a.child:
        print(json.dumps(feed_medians(a.reps)))
        return
    dev = torch.device("cuda:0")
    switch, tile = api.truepeak_columns_limits()
    res = {"device": torch.cuda.get_device_name(0), "switch_over": switch, "tile_samples": tile}

    n = a.samples
    x = torch.randn((2, n), dtype=torch.float32, device=dev) * 0.3
    tp_carry = torch.zeros(2 * 64, dtype=torch.uint8, device=dev)
    if a.kernels:
        peaks = torch.empty((-(-n // a.kernels), 2, 16), dtype=torch.uint8, device=dev)
        for _ in range(3):
            assert api.stage_truepeak_columns(x, n, 2, n, a.kernels, 0, True, False, 0, tp_carry, peaks) == 0
        torch.cuda.synchronize()
        return

    # (a)
    y = torch.empty_like(x)
    read = 2 * n * 4
    ms = events(lambda: y.copy_(x))
    res["a_copy"] = {"ms": round(ms, 4), "bytes_read": read, "read_tb_per_s": round(read / ms / 1e9, 3)}
    del y
    res["a_cold"] = {}
    carry = torch.zeros(80, dtype=torch.uint8, device=dev)
    wave_carry = torch.zeros((2, 2), dtype=torch.float32, device=dev)
    for m in (64, 512, 4096, 1 << 20):
        peaks = torch.empty((-(-n // m), 2, 16), dtype=torch.uint8, device=dev)
        level = torch.empty((-(-n // m), 1, 80), dtype=torch.uint8, device=dev)
        wave = torch.empty((-(-n // m), 2, 2), dtype=torch.float32, device=dev)

        def call():
            st = api.stage_truepeak_columns(x, n, 2, n, m, 0, True, False, 0, tp_carry, peaks)
            assert st == 0, st

        def level_call():
            st = api.stage_level_columns(x, n, 1, n, m, 0, True, 0, carry, level)
            assert st == 0, st

        def wave_call():
            st = api.stage_wave_columns(x, n, 2, n, m, 0, True, 0, wave_carry, wave)
            assert st == 0, st
        ms, level_ms, wave_ms = events(call), events(level_call), events(wave_call)
        res["a_cold"][str(m)] = {"ms": round(ms, 4), "bytes_read": read, "bytes_written": peaks.numel(), "read_tb_per_s": round(read / ms / 1e9, 3),
                                 "of_copy": round(res["a_copy"]["ms"] / ms, 3), "level_ms": round(level_ms, 4),
                                 "level_read_tb_per_s": round(read / level_ms / 1e9, 3), "wave_ms": round(wave_ms, 4),
                                 "wave_read_tb_per_s": round(read / wave_ms / 1e9, 3), "form": "tile" if m <= switch else "sliced"}
        del peaks, level, wave
    del x

    # (b), (c)
    cfg, S, s16, F, P = cfg2_s16()
    out = np.zeros((F, P, 4), np.uint8)
    lane_out = np.zeros((-(-S // M), 2), api.TRUEPEAK_DTYPE)
    stream = api.PcmStream(cfg, api.PCM_S16, 2)
    flushes, host_ms = [], []
    interleaved = np.ascontiguousarray(s16).reshape(S, 2)

    def feed(armed):
        stream.reset()
        stream.set_truepeak(M if armed else 0, lane_out if armed else None)
        t0 = time.perf_counter()
        st, f, _ = stream.feed_into(s16, S, out, None, F, timing=False)
        t = (time.perf_counter() - t0) * 1e3
        assert st == 0 and f == F
        if armed:
            stream.flush_truepeak()
            flushes.append((time.perf_counter() - t0) * 1e3 - t)
            return t + flushes[-1], None                               # (the armed way pays for its flush)
        t1 = time.perf_counter()
        records = host_records(interleaved, M)
        host_ms.append((time.perf_counter() - t1) * 1e3)
        return t + host_ms[-1], records

    feed(True)
    _, records = feed(False)
    equal = lane_out.tobytes() == np.ascontiguousarray(records, api.TRUEPEAK_DTYPE).tobytes()
    image = out.copy()
    ts = {True: [], False: []}
    for _ in range(a.reps):
        for armed in (True, False):
            ts[armed].append(feed(armed)[0])
            assert np.array_equal(out, image)
    stream.close()
    armed_ms, other_ms = statistics.median(ts[True]), statistics.median(ts[False])
    flush_ms, numpy_ms = statistics.median(flushes), statistics.median(host_ms)
    res["b_stream"] = {"samples": S, "m": M, "reps": a.reps, "armed_ms": round(armed_ms, 3), "disarmed_plus_numpy_ms": round(other_ms, 3),
                       "numpy_ms": round(numpy_ms, 3), "flush_ms": round(flush_ms, 3), "armed_min_max_ms": [round(min(ts[True]), 3), round(max(ts[True]), 3)],
                       "disarmed_plus_numpy_min_max_ms": [round(min(ts[False]), 3), round(max(ts[False]), 3)],
                       "armed_over_other": round(armed_ms / other_ms, 4), "records_equal": bool(equal)}
    # (c): a loop of its own -- in (b) the armed feed follows numpy's pass over the PCM, the disarmed one follows a feed
    own = feed_medians(a.reps)
    r3 = lambda v: [round(x, 3) for x in v] if isinstance(v, list) else round(v, 3)      # noqa: E731
    res["c_overhead"] = {k: r3(v) for k, v in own.items()}
    res["c_overhead"]["armed_over_disarmed"] = round(own["armed_ms"] / own["disarmed_ms"], 4)
    res["c_overhead"]["against_parent_build"] = "not measured"
    if a.parent_tree:
        runs = {"this": [], "parent": []}
        for _ in range(3):
            for which, tree in (("this", TREE), ("parent", os.path.abspath(a.parent_tree))):
                got = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--tree", tree], capture_output=True,
                                     text=True, timeout=300, check=True)
                runs[which].append(json.loads(got.stdout.strip().splitlines()[-1]))
        this_d, this_a = [r["disarmed_ms"] for r in runs["this"]], [r["armed_ms"] for r in runs["this"]]
        parent = [r["disarmed_ms"] for r in runs["parent"]]
        res["c_overhead"]["against_parent_build"] = {"parent_ms": r3(parent), "this_disarmed_ms": r3(this_d), "this_armed_ms": r3(this_a),
                                                     "disarmed_over_parent": round(statistics.median(this_d) / statistics.median(parent), 4),
                                                     "armed_over_parent": round(statistics.median(this_a) / statistics.median(parent), 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")
    assert equal, "the lane's records differ from numpy's on the PCM"
    assert armed_ms < 0.95 * other_ms, f"armed {armed_ms:.3f} ms is not below 0.95 x {other_ms:.3f} ms"


if __name__ == "__main__":
    main()
