"""What the render thread's colour-spectrum frame costs (spectrum_present.hip): sgz_spectrum_render_columns, sgz_image_unroll_device and
sgz_columns_to_image_device against what they replace or could at best be.
    python tools/bench_present.py [--out gpu_out/present.json]
  frame     10 ready columns of P = 1024 into a 2048-column image: sgz_spectrum_render_columns (one columnsToImageKernel launch) against
            sgz_spectrum_flush_columns (ten columnScatterKernel launches), on twin handles fed the same audio, alternating call by call.
            Both calls wait for their texels, so the figure is the host clock around the call (median of --calls)
  unroll    sgz_image_unroll_device on 1024 x 2048 texels (x = 777, so the source runs are 4 bytes off the destination's) against a
            hipMemcpy2DAsync device-to-device copy of the same image; device events around --reps launches back to back
  texture   sgz_columns_to_image_device on 348 x 1024 and 100 000 x 1024 columns, the same way; bytes per second = read + written
Every step runs in a child process of its own under a time limit and after a spin-up of the device; a step that fails ends the run."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"frame": 240, "unroll": 180, "texture": 240}      # seconds a step may take


def _spin_up(torch, seconds=0.5):
    a = torch.zeros(1 << 24, dtype=torch.float32, device="cuda:0")
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(50):
            a.add_(1.0)
        torch.cuda.synchronize()


def _event_ms(torch, launch, reps, windows=9):
    """median over `windows` of the device time of `reps` launches back to back, per launch"""
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            launch()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def step_frame(a):
    import numpy as np
    import torch

    from signalizer_amd import api, config, synth
    L = api.lib()
    L.sgz_spectrum_flush.argtypes = [C.c_void_p]
    P, columns, hop = 1024, 2048, 512
    cfg = config.spectrum_config(window_size=4096, hop=hop, axis_points=P)
    handles, images = [], []
    for _ in range(2):
        c = api.config_from_dict(cfg)
        h = C.c_void_p()
        api.check(L.sgz_spectrum_create(C.byref(c), C.byref(h)))
        img = torch.zeros((P, columns), dtype=torch.int32, device="cuda:0")
        api.check(L.sgz_spectrum_bind_image(h, C.c_void_p(img.data_ptr()), columns, 4 * columns))
        handles.append(h)
        images.append(img)
    x = synth.gen(5, 48000, hop * 10, 2)
    blocks = [np.ascontiguousarray(x[:, k * hop:(k + 1) * hop]) for k in range(10)]
    first, cnt = C.c_uint32(0), C.c_uint32(0)
    times = ([], [])
    try:
        _spin_up(torch)
        for it in range(a.calls + 5):
            for h in handles:
                for blk in blocks:
                    ptrs = (C.c_void_p * 2)(blk[0].ctypes.data, blk[1].ctypes.data)
                    while True:
                        st = L.sgz_spectrum_push(h, ptrs, 2, hop)
                        if st != api.SGZ_BUSY:
                            break
                    api.check(st)
                api.check(L.sgz_spectrum_flush(h))
            torch.cuda.synchronize()
            for which in ((0, 1) if it % 2 == 0 else (1, 0)):
                t0 = time.perf_counter()
                if which == 0:
                    st = L.sgz_spectrum_render_columns(handles[0], C.byref(first), C.byref(cnt), None)
                else:
                    st = L.sgz_spectrum_flush_columns(handles[1], C.byref(first), C.byref(cnt))
                dt = time.perf_counter() - t0
                assert st == api.SGZ_OK and cnt.value == 10, (which, st, cnt.value)
                if it >= 5:
                    times[which].append(dt)
        torch.cuda.synchronize()
        same = bool(torch.equal(images[0], images[1]))
    finally:
        for h in handles:
            L.sgz_spectrum_destroy(h)
    us = lambda v: round(float(np.median(v)) * 1e6, 2)          # noqa: E731
    return dict(calls=a.calls, columns_per_call=10, axis_points=P, render_columns_us_median=us(times[0]), render_columns_us_min=round(min(times[0]) * 1e6, 2),
                flush_columns_us_median=us(times[1]), flush_columns_us_min=round(min(times[1]) * 1e6, 2), images_equal=same)


def step_unroll(a):
    import torch

    from signalizer_amd import api
    P, columns, x = 1024, 2048, 777
    pitch = 4 * columns
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (P, columns), dtype=torch.int32, device="cuda:0")
    dst = torch.zeros_like(src)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream or None

    def unroll():
        api.image_unroll_device(src, columns, pitch, P, x, dst, pitch, stream)

    def copy():
        assert hip.hipMemcpy2DAsync(dst.data_ptr(), pitch, src.data_ptr(), pitch, pitch, P, 3, stream) == 0

    _spin_up(torch)
    res = {}
    for rnd in range(2):                                        # alternating, twice
        for name, fn in (("unroll", unroll), ("memcpy2d", copy)):
            med, lo, hi = _event_ms(torch, fn, a.reps)
            res.setdefault(name, []).append(med)
    unroll()
    torch.cuda.synchronize()
    ok = bool(torch.equal(dst, torch.roll(src, -x, dims=1)))
    nbytes = 2 * P * pitch
    out = dict(texels=f"{P}x{columns}", x=x, reps=a.reps, result_equals_roll=ok)
    for name, v in res.items():
        ms = min(v)
        out[f"{name}_us"] = round(ms * 1e3, 2)
        out[f"{name}_us_rounds"] = [round(t * 1e3, 2) for t in v]
        out[f"{name}_GBps"] = round(nbytes / (ms * 1e-3) / 1e9, 1)
    return out


def step_texture(a):
    import torch

    from signalizer_amd import api
    P = 1024
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream or None
    _spin_up(torch)
    out = {}
    for n in (348, 100000):
        cols = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, P), dtype=torch.int32, device="cuda:0")
        img = torch.zeros((P, n), dtype=torch.int32, device="cuda:0")
        other = torch.zeros_like(img)
        reps = a.reps if n < 10000 else max(2, a.reps // 10)

        def transpose():
            api.columns_to_image_device(cols, n, P, img, n, 4 * n, 0, stream)

        def copy():
            assert hip.hipMemcpy2DAsync(other.data_ptr(), 4 * n, img.data_ptr(), 4 * n, 4 * n, P, 3, stream) == 0

        t_ms = min(_event_ms(torch, transpose, reps)[0] for _ in range(2))
        c_ms = min(_event_ms(torch, copy, reps)[0] for _ in range(2))
        torch.cuda.synchronize()
        ok = bool(torch.equal(img, cols.t()))
        nbytes = 2 * 4 * n * P
        out[f"{n}x{P}"] = dict(columns_to_image_us=round(t_ms * 1e3, 2), columns_to_image_GBps=round(nbytes / (t_ms * 1e-3) / 1e9, 1),
                               memcpy2d_us=round(c_ms * 1e3, 2), memcpy2d_GBps=round(nbytes / (c_ms * 1e-3) / 1e9, 1), reps=reps,
                               result_equals_transpose=ok)
        del cols, img, other
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=list(STEPS), default=None, help="run one step in this process (what the parent starts)")
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "needs a GPU"
        print(json.dumps({a.step: globals()[f"step_{a.step}"](a)}))
        return 0
    res = {}
    for step, limit in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--calls", str(a.calls), "--reps", str(a.reps)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"step {step}: no result within {limit} s; stopping", file=sys.stderr)
            return 124
        if p.returncode != 0:                                   # nothing more is started on the device behind a failed step
            print(f"step {step}: exit status {p.returncode}; stopping", file=sys.stderr)
            return p.returncode or 1
        res.update(json.loads(p.stdout.decode().strip().splitlines()[-1]))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
