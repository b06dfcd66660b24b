"""What a setting change costs on a live Spectrum: sgz_spectrum_update on a handle of cfg2's transform (N = W = 32768, Separate, P = 1024)
with the library's own 1024 x 2048 image bound, one class of fields at a time, the value alternating call by call.
    python tools/bench_update.py [--calls 30] [--out gpu_out/update.json]
  wall      host clock around each call (the call waits for its own work: the warm-up, the ring move, an image translation)
  busy      how long push is refused during a call: a producer thread pushes 32-sample blocks every 50 us (about 14x real time at
            48 kHz) and records the host time of every SGZ_BUSY; per call, the span from the first to the last refusal plus one push
            period (refusals outside every call are counted apart)
  stage     sgz_ring_resize_device alone, 32 channels, capacity 32768 -> 65536 and back, host clock around the call and a synchronize
For the kernel's own time run this under rocprofv3 --kernel-trace --stats (ringResizeKernel)."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from signalizer_amd import api, config, synth

# the classes of sgz.h's table: (name, the alternative value of the fields)
CLASSES = [
    ("db", dict(low_db=-90.0, high_db=6.0)),
    ("colours", dict(colours=[(0, 0, 0), (40, 0, 64), (0, 128, 255), (0, 255, 128), (255, 255, 0), (255, 0, 0)])),
    ("window", dict(window_type=config.WIN_BLACKMAN)),
    ("window_size", dict(window_size=16384)),
    ("hop", dict(hop=4096)),
    ("view", dict(view_left=0.1, view_right=0.9)),
    ("channel_mode", dict(channel_mode=config.CH_MERGE)),
    ("algorithm", dict(algorithm=config.ALGO_RSNT)),
]


def measure(L, cfg, over, calls, period=50e-6, block=32):
    c = api.config_from_dict(cfg)
    h = C.c_void_p()
    api.check(L.sgz_spectrum_create(C.byref(c), C.byref(h)))
    try:
        d_img, pitch = C.c_void_p(), C.c_size_t(0)
        api.check(L.sgz_spectrum_create_image(h, 2048, C.byref(d_img), C.byref(pitch), None))
        x = synth.gen(2, 48000, 32768 + 4 * cfg["hop"], 2)
        for pos in range(0, x.shape[1], cfg["hop"]):
            blk = np.ascontiguousarray(x[:, pos:pos + cfg["hop"]])
            ptrs = (C.c_void_p * 2)(blk[0].ctypes.data, blk[1].ctypes.data)
            api.check(L.sgz_spectrum_push(h, ptrs, 2, blk.shape[1]))
        L.sgz_spectrum_flush.argtypes = [C.c_void_p]
        api.check(L.sgz_spectrum_flush(h))
        cfgs = [dict(cfg, **over), cfg]
        for k in range(4):                                      # warm-up: both configurations' plans and scratch
            api.spectrum_update(h, cfgs[k % 2])
        blk = np.ascontiguousarray(synth.gen(3, 48000, block, 2))
        ptrs = (C.c_void_p * 2)(blk[0].ctypes.data, blk[1].ctypes.data)
        busy_t, stop = [], threading.Event()

        def producer():
            nxt = time.perf_counter()
            while not stop.is_set():
                if time.perf_counter() < nxt:
                    continue
                nxt += period
                st = L.sgz_spectrum_push(h, ptrs, 2, block)
                if st == api.SGZ_BUSY:
                    busy_t.append(time.perf_counter())
                else:
                    api.check(st)

        th = threading.Thread(target=producer)
        th.start()
        time.sleep(0.05)
        spans, wall = [], []
        try:
            for k in range(calls):
                time.sleep(0.01)
                t0 = time.perf_counter()
                api.spectrum_update(h, cfgs[k % 2])
                t1 = time.perf_counter()
                wall.append(t1 - t0)
                spans.append((t0, t1))
            time.sleep(0.02)
        finally:
            stop.set()
            th.join()
        outside = sum(1 for t in busy_t if not any(t0 <= t <= t1 + period for t0, t1 in spans))
        refused = []
        for t0, t1 in spans:
            ts = [t for t in busy_t if t0 <= t <= t1 + period]
            refused.append((ts[-1] - ts[0] + period) if ts else 0.0)
    finally:
        L.sgz_spectrum_destroy(h)
    return wall, refused, outside


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    L = api.lib()
    cfg = config.spectrum_config()
    ms = lambda v: round(float(np.median(v)) * 1e3, 3)          # noqa: E731
    res = dict(calls=a.calls, config="cfg2 (W = N = 32768, Separate, P = 1024), own 1024 x 2048 image", classes={})
    for name, over in CLASSES:
        wall, refused, outside = measure(L, cfg, over, a.calls)
        res["classes"][name] = dict(wall_ms_median=ms(wall), wall_ms_max=round(max(wall) * 1e3, 3), push_refused_ms_median=ms(refused),
                                    push_refused_ms_max=round(max(refused) * 1e3, 3), refusals_outside_calls=outside)
    small, large, ch = 32768, 65536, 32
    a_ring = torch.zeros((ch, 2 * small), dtype=torch.float32, device="cuda:0")
    b_ring = torch.zeros((ch, 2 * large), dtype=torch.float32, device="cuda:0")
    stage = {"32768->65536": [], "65536->32768": []}
    for k in range(a.calls + 4):
        for key, (src, sc, dst, dc) in (("32768->65536", (a_ring, small, b_ring, large)), ("65536->32768", (b_ring, large, a_ring, small))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            api.ring_resize_device(src, sc, dst, dc, ch, 10 ** 7 + k)
            torch.cuda.synchronize()
            if k >= 4:
                stage[key].append(time.perf_counter() - t0)
    res["stage_call_ms_median"] = {k: ms(v) for k, v in stage.items()}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    main()
