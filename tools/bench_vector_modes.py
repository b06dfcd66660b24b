"""The Vectorscope's two plot modes at cfg4's shape (8 channels, 96 kHz, 9600-sample window, fade on): ms per
sgz_vector_vertices_all (polar) and per sgz_vector_lissajous_vertices_all (Lissajous), every pair into caller-owned DEVICE buffers,
alternating the two call by call on one handle.
    python tools/bench_vector_modes.py [--reads 400] [--rounds 3]
"frame": one 60 Hz frame of audio (1600 samples, 400-sample blocks) pushed before every read, as a render loop sees it -- the polar read
then redoes its fade-ramp kernel; "repeat": reads with no push between (the polar ramp is reused).  Host clock around the call (it
waits for the GPU) and HIP events on the handle's stream around it; the push is outside both."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import HipEvents
from signalizer_amd import api, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    L = api.lib()
    W, NCH, SR = 9600, 8, 96000.0
    h = api.Vector(sample_rate=SR, num_channels=NCH, window_size=W, envelope_mode=1, lanes=8, fade_history=1, max_block=512,
                   envelope_window=0.3, stereo_window=0.05, colours=[(1.0, 0.5, 0.25), (0.2, 0.9, 0.4), (0.3, 0.3, 1.0), (0.7, 0.1, 0.6)])
    x = synth.gen(4, SR, 96000 * 4, NCH)
    d_xyz = torch.empty((NCH // 2, W, 3), dtype=torch.float32, device="cuda:0")
    d_rgb = torch.empty((NCH // 2, W, 3), dtype=torch.float32, device="cuda:0")
    px, pc = C.c_void_p(d_xyz.data_ptr()), C.c_void_p(d_rgb.data_ptr())
    stream = L.sgz_vector_stream(h.h)
    ev = HipEvents(2)
    calls = {"polar": L.sgz_vector_vertices_all, "lissajous": L.sgz_vector_lissajous_vertices_all}
    pos = [0]

    def push_frame():
        for _ in range(4):
            if pos[0] + 400 > x.shape[1]:
                pos[0] = 0
            blk = np.ascontiguousarray(x[:, pos[0]:pos[0] + 400])
            while h.push(blk) == api.SGZ_BUSY:
                pass
            pos[0] += 400
        h.flush()
        torch.cuda.synchronize()

    def read(name):
        cnt = C.c_uint32(W)
        ev.record(0, stream)
        t0 = time.perf_counter()
        api.check(calls[name](h.h, px, pc, C.byref(cnt)))
        t1 = time.perf_counter()
        ev.record(1, stream)
        return (t1 - t0) * 1e3, ev.elapsed_ms(0, 1)

    for _ in range(50):                                            # warm-up: both code paths, both shapes of the polar ramp work
        push_frame(); read("polar"); read("lissajous")
    out = {"shape": {"channels": NCH, "window": W, "sample_rate": SR, "destination": "device"}, "rounds": []}
    for rnd in range(args.rounds):
        res = {}
        for mode in ("frame", "repeat"):
            t = {"polar": ([], []), "lissajous": ([], [])}
            for i in range(args.reads):
                order = ("polar", "lissajous") if i % 2 == 0 else ("lissajous", "polar")
                for name in order:
                    if mode == "frame":
                        push_frame()
                    host, evms = read(name)
                    t[name][0].append(host); t[name][1].append(evms)
            res[mode] = {name: {"host_ms_median": float(np.median(a)), "host_ms_p10": float(np.percentile(a, 10)),
                                "host_ms_p90": float(np.percentile(a, 90)), "event_ms_median": float(np.median(b))}
                         for name, (a, b) in t.items()}
        out["rounds"].append(res)
        for mode, r in res.items():
            print(f"round {rnd} {mode:6s}  polar {r['polar']['host_ms_median']:.4f} ms (events {r['polar']['event_ms_median']:.4f})   "
                  f"lissajous {r['lissajous']['host_ms_median']:.4f} ms (events {r['lissajous']['event_ms_median']:.4f})", flush=True)
    print(json.dumps(out))
    h.close()


if __name__ == "__main__":
    main()
