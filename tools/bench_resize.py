"""What a resize costs on a live Spectrum: sgz_spectrum_resize on a handle of cfg2's transform (N = W = 32768, Separate) alternating between
1024 and 1080 rows call by call, each call moving a 2048-column image into the other of two caller-owned device images (8.0 / 8.4 MiB), so
every call rebuilds the plans and the axis-sized buffers and resamples the image.
    python tools/bench_resize.py [--calls 50] [--out gpu_out/resize.json]
  wall      host clock around each call (the call waits for its own work, the translation included)
  busy      how long push is refused during a call: a producer thread pushes 32-sample blocks every 50 us (about 14x real time at
            48 kHz) and records the host time of every SGZ_BUSY; per call, the span from the first to the last refusal plus one push
            period.  The refusals come from the handle being held: the backlog never fills at this rate (checked: no BUSY outside calls)
  stage     sgz_image_resize_device alone, 1024 x 2048 into 1080 x 2048 and back, host clock around the call (it waits)
For the kernel's own time run this under rocprofv3 --kernel-trace --stats (imageResizeKernel)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    L = api.lib()
    cfg = config.spectrum_config()
    sizes, columns, hop = (1024, 1080), 2048, cfg["hop"]
    c = api.config_from_dict(cfg)
    h = C.c_void_p()
    api.check(L.sgz_spectrum_create(C.byref(c), C.byref(h)))
    imgs = [torch.zeros((P, columns), dtype=torch.int32, device="cuda:0") for P in sizes]
    pitch = columns * 4
    try:
        api.check(L.sgz_spectrum_bind_image(h, imgs[0].data_ptr(), columns, pitch))
        x = synth.gen(2, 48000, 32768 + 4 * hop, 2)
        for pos in range(0, x.shape[1], hop):
            blk = np.ascontiguousarray(x[:, pos:pos + hop])
            ptrs = (C.c_void_p * 2)(blk[0].ctypes.data, blk[1].ctypes.data)
            api.check(L.sgz_spectrum_push(h, ptrs, 2, hop))
        L.sgz_spectrum_flush.argtypes = [C.c_void_p]
        api.check(L.sgz_spectrum_flush(h))
        first, cnt = C.c_uint32(0), C.c_uint32(0)
        L.sgz_spectrum_flush_columns(h, C.byref(first), C.byref(cnt))
        for k in range(4):                                      # warm-up: the resampling's scratch, both sizes' plans
            api.spectrum_resize(h, sizes[(k + 1) % 2], imgs[(k + 1) % 2], columns, pitch)

        # the producer: 32-sample blocks every 50 us
        period, block = 50e-6, 32
        blk = np.ascontiguousarray(synth.gen(3, 48000, block, 2))
        ptrs = (C.c_void_p * 2)(blk[0].ctypes.data, blk[1].ctypes.data)
        busy_t, stop = [], threading.Event()
        pushes = [0]

        def producer():
            nxt = time.perf_counter()
            while not stop.is_set():
                now = time.perf_counter()
                if now < nxt:
                    continue
                nxt += period
                st = L.sgz_spectrum_push(h, ptrs, 2, block)
                pushes[0] += 1
                if st == api.SGZ_BUSY:
                    busy_t.append(time.perf_counter())
                else:
                    api.check(st)

        th = threading.Thread(target=producer)
        th.start()
        time.sleep(0.05)
        spans, wall = [], []
        try:
            for k in range(a.calls):
                time.sleep(0.01)
                t0 = time.perf_counter()
                api.spectrum_resize(h, sizes[(k + 1) % 2], imgs[(k + 1) % 2], columns, pitch)
                t1 = time.perf_counter()
                wall.append(t1 - t0)
                spans.append((t0, t1))
            time.sleep(0.02)
        finally:
            stop.set()
            th.join()
        refused = []
        outside = 0
        for t in busy_t:
            if not any(t0 <= t <= t1 + period for t0, t1 in spans):
                outside += 1
        for t0, t1 in spans:
            ts = [t for t in busy_t if t0 <= t <= t1 + period]
            refused.append((ts[-1] - ts[0] + period) if ts else 0.0)
    finally:
        L.sgz_spectrum_destroy(h)

    stage = []
    for k in range(a.calls + 4):
        src, dst = k % 2, (k + 1) % 2
        t0 = time.perf_counter()
        api.image_resize_device(imgs[src], columns, pitch, sizes[src], k % columns, imgs[dst], columns, pitch, sizes[dst])
        if k >= 4:
            stage.append(time.perf_counter() - t0)

    ms = lambda v: round(float(np.median(v)) * 1e3, 3)          # noqa: E731
    res = dict(calls=a.calls, image=f"{sizes[0]}<->{sizes[1]}x{columns} RGBA8", resize_wall_ms_median=ms(wall),
               resize_wall_ms_min=round(min(wall) * 1e3, 3), resize_wall_ms_max=round(max(wall) * 1e3, 3), push_refused_ms_median=ms(refused),
               push_refused_ms_max=round(max(refused) * 1e3, 3), pushes=pushes[0], refusals=len(busy_t), refusals_outside_calls=outside,
               stage_call_ms_median=ms(stage), stage_call_ms_min=round(min(stage) * 1e3, 3))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    main()
