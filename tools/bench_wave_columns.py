"""What the waveform lane costs (sgz_stage_wave_columns; sgz_pcm_stream_set_waveform).
    python tools/bench_wave_columns.py [--reps 9] [--out gpu_out/wave_columns.json]
  (a) the stage call, cold: 64 Mi stereo samples (512 MiB: past the 256 MiB Infinity Cache) at m = 64, 512, 4096 and 2^20 -- 20 launches
      after 3 warm-ups between events, median, as bytes READ per second (the call writes next to nothing); and from the same run the
      yardstick: a device-to-device copy of the same buffer by 16-byte accesses (hipMemcpyAsync's copy kernel), as bytes read per second
  (b) the stage call, L2-warm: a piece-sized buffer (2^20 stereo samples) that the converter has just written -- converter and reduction
      back to back in one event interval, minus the converter alone, and the reduction alone on the buffer it has just read
  (c) the stream: one feed of a kept sgz_pcm_stream of cfg2's 60 s of stereo S16 (tools/bench_pcm_render.py (b)'s kept feed), the lane armed
      at m = 512 and disarmed, alternating, --reps pairs after a warm-up pair; wall clock of the host around the feed, medians and spread
      (the flush of the last, open column -- one launch, one column read back, a wait -- is timed apart)
Every figure comes from a run on the GPU; the tool refuses to run without one."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from signalizer_amd import api, config, synth


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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples", type=int, default=64 << 20, help="samples per channel of the cold buffer")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    switch, tile = api.wave_columns_limits()
    res = {"device": torch.cuda.get_device_name(0), "switch_over": switch, "tile_samples": tile}

    # (a)
    n = a.samples
    x = torch.randn((2, n), dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    read = 2 * n * 4
    ms = events(lambda: y.copy_(x))
    res["a_copy"] = {"ms": round(ms, 4), "bytes_read": read, "read_tb_per_s": round(read / ms / 1e9, 3)}
    del y
    res["a_cold"] = {}
    carry = torch.zeros((2, 2), dtype=torch.float32, device=dev)
    for m in (64, 512, 4096, 1 << 20):
        wave = torch.empty((-(-n // m), 2, 2), dtype=torch.float32, device=dev)

        def call():
            st = api.stage_wave_columns(x, n, 2, n, m, 0, True, 0, carry, wave)
            assert st == 0, st
        ms = events(call)
        res["a_cold"][str(m)] = {"ms": round(ms, 4), "bytes_read": read, "read_tb_per_s": round(read / ms / 1e9, 3),
                                 "of_copy": round(res["a_copy"]["ms"] / ms, 3), "form": "tile" if m <= switch else "sliced"}
        del wave
    del x

    # (b)
    n = 1 << 20
    src = torch.randint(0, 256, (n * 2 * 2,), dtype=torch.uint8, device=dev)
    planar = torch.empty((2, n), dtype=torch.float32, device=dev)
    conv = lambda: api.pcm_to_planar_device(src, api.PCM_S16, 2, n, planar)            # noqa: E731
    conv_ms = events(conv)
    res["b_warm"] = {"converter_ms": round(conv_ms, 4)}
    for m in (64, 512, 4096):
        wave = torch.empty((-(-n // m), 2, 2), dtype=torch.float32, device=dev)
        red = lambda: api.stage_wave_columns(planar, n, 2, n, m, 0, True, 0, carry, wave)          # noqa: E731
        both_ms = events(lambda: (conv(), red()))
        alone_ms = events(red)
        res["b_warm"][str(m)] = {"behind_converter_ms": round(both_ms - conv_ms, 4), "alone_ms": round(alone_ms, 4),
                                 "alone_read_tb_per_s": round(2 * n * 4 / alone_ms / 1e9, 3)}
        del wave

    # (c)
    cfg = config.cfg2()
    S = int(config.CFG2_SECONDS * 48000)
    sig = synth.gen(config.CFG2_SEED, 48000, S, 2)
    s16 = np.ascontiguousarray(np.clip(np.round(sig.T * 32768.0), -32768, 32767).astype(np.int16))
    F, P = int(api.lib().sgz_num_frames(S, cfg["window_size"], cfg["hop"])), cfg["axis_points"]
    out = np.zeros((F, P, 4), np.uint8)
    m = 512
    wave_out = np.zeros((-(-S // m), 2, 2), np.float32)
    stream = api.PcmStream(cfg, api.PCM_S16, 2)

    flushes = []

    def feed(armed):
        stream.reset()
        stream.set_waveform(m if armed else 0, wave_out if armed else None)
        t0 = time.perf_counter()
        st, f, _ = stream.feed_into(s16, S, out, None, F, timing=False)
        t = (time.perf_counter() - t0) * 1e3
        if armed:
            stream.flush_waveform()
            flushes.append((time.perf_counter() - t0) * 1e3 - t)
        assert st == 0 and f == F
        return t

    feed(True), feed(False)
    image = out.copy()
    ts = {True: [], False: []}
    for _ in range(a.reps):
        for armed in (True, False):
            ts[armed].append(feed(armed))
            assert np.array_equal(out, image)
    stream.close()
    planar_ref = np.ascontiguousarray(s16.T).astype(np.float32) * np.float32(2.0 ** -15)
    lo = planar_ref[:, :(S // m) * m].reshape(2, S // m, m).min(axis=2).T
    res["c_stream"] = {"samples": S, "m": m, "reps": a.reps,
                       "armed_ms": round(statistics.median(ts[True]), 3), "disarmed_ms": round(statistics.median(ts[False]), 3),
                       "armed_min_max_ms": [round(min(ts[True]), 3), round(max(ts[True]), 3)],
                       "disarmed_min_max_ms": [round(min(ts[False]), 3), round(max(ts[False]), 3)],
                       "flush_ms": round(statistics.median(flushes), 3),
                       "armed_over_disarmed": round(statistics.median(ts[True]) / statistics.median(ts[False]), 4),
                       "lo_equals_numpy": bool(np.array_equal(wave_out[:S // m, :, 0], lo))}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
