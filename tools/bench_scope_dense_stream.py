"""What the Oscilloscope's dense stream costs beside the Linear stream it reduces (scope_dense.hip against scope_vector.hip's
scopeWaveLinearKernel), on one stereo 192 kHz handle.
    python tools/bench_scope_dense_stream.py [--out gpu_out/scope_dense_stream.json] [--calls 60]
For n = 2^14, 2^17, 2^20 and 2^23 samples in the window, into DEVICE buffers and into pinned host buffers:
  linear   sgz_scope_vertices_all, two evaluators (Left, Right): n vertices of 16 bytes each
  dense    sgz_scope_dense_vertices_all, the same two evaluators, columns = 2048: 4096 vertices each
Both calls wait for their vertices, so the figure is the host clock around the call: the median (and the extremes) of --calls calls, the
two alternating call by call on the same frame after a spin-up of the device and warm-up calls of both.  Before it is timed the dense
strip is compared with the per-column minimum and maximum of the Linear strip it was taken from.
One JSON line per (n, destination); exit status 1 if the dense call is slower than the Linear one anywhere at n >= 2^17."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLUMNS = 2048
SIZES = (1 << 14, 1 << 17, 1 << 20, 1 << 23)


def _spin_up(torch, seconds=0.5):
    a = torch.zeros(1 << 24, dtype=torch.float32, device="cuda:0")
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(50):
            a.add_(1.0)
        torch.cuda.synchronize()


def _median_us(samples):
    s = sorted(samples)
    return 1e6 * s[len(s) // 2], 1e6 * s[0], 1e6 * s[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=60)
    a = ap.parse_args()
    import numpy as np
    import torch

    from signalizer_amd import api
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing measured")
    rows, slower = [], []
    view = api.ScopeView(0.0, 0.0, 1.0, 1.0, 2, 0)
    for n in SIZES:
        dev = api.Scope(sample_rate=192000.0, window_size=float(n), num_channels=2, trigger_mode=0, channel_mode=0, envelope_mode=0,
                        interpolation=2, max_block=131072, trigger_threshold=0.05, trigger_channel=1.0, envelope_window=0.3)
        rng = np.random.default_rng(n)
        x = (0.3 * rng.standard_normal((2, n + 5000))).astype(np.float32)
        for pos in range(0, x.shape[1], 131072):
            while dev.push(np.ascontiguousarray(x[:, pos:pos + 131072])) != api.SGZ_OK:
                pass
        dev.flush()
        assert api.lib().sgz_scope_vertex_count(dev.h, view) == n and dev.dense_vertex_count(COLUMNS) == 2 * COLUMNS
        for where in ("device", "pinned"):
            def mk(rows_, cols_, dt):
                t = torch.zeros((rows_, cols_), dtype=dt)
                return t.to("cuda:0") if where == "device" else t.pin_memory()
            lin = [(mk(n, 3, torch.float32), mk(n, 4, torch.uint8)) for _ in (0, 1)]
            den = [(mk(2 * COLUMNS, 3, torch.float32), mk(2 * COLUMNS, 4, torch.uint8)) for _ in (0, 1)]
            torch.cuda.synchronize()

            # both calls through the C ABI with their arguments built once: the clock is around the library call, not a Python wrapper
            ev = (C.c_uint32 * 2)(0, 1); ch = (C.c_uint32 * 2)(0, 0)
            lx = (C.c_void_p * 2)(*[o[0].data_ptr() for o in lin]); lc = (C.c_void_p * 2)(*[o[1].data_ptr() for o in lin])
            dx = (C.c_void_p * 2)(*[o[0].data_ptr() for o in den]); dc = (C.c_void_p * 2)(*[o[1].data_ptr() for o in den])
            lcnt, dcnt = (C.c_uint32 * 2)(), (C.c_uint32 * 2)()
            L, h, pview = api.lib(), dev.h, C.byref(view)

            def linear():
                lcnt[0] = lcnt[1] = n
                if L.sgz_scope_vertices_all(h, pview, 2, ev, ch, lx, lc, lcnt) != 0:
                    raise RuntimeError("sgz_scope_vertices_all")

            def dense():
                dcnt[0] = dcnt[1] = 2 * COLUMNS
                if L.sgz_scope_dense_vertices_all(h, COLUMNS, 2, ev, ch, dx, dc, dcnt) != 0:
                    raise RuntimeError("sgz_scope_dense_vertices_all")
            _spin_up(torch)
            for _ in range(5):
                linear(); dense()
            # the dense strip is the Linear strip's extremes, column by column (noise: no NaN, ties aside the values decide)
            for k in (0, 1):
                y = lin[k][0][:, 1].cpu().numpy()
                st = (np.arange(COLUMNS, dtype=np.int64) * n + COLUMNS - 1) // COLUMNS
                g = den[k][0].cpu().numpy()
                pair = np.stack([g[0::2, 1], g[1::2, 1]])
                assert np.array_equal(pair.min(axis=0), np.minimum.reduceat(y, st)) and np.array_equal(pair.max(axis=0), np.maximum.reduceat(y, st))
                assert np.array_equal(y[g[:, 0].astype(np.int64)], g[:, 1])
            t_lin, t_den = [], []
            for _ in range(a.calls):
                t0 = time.perf_counter(); linear(); t1 = time.perf_counter(); dense(); t2 = time.perf_counter()
                t_lin.append(t1 - t0); t_den.append(t2 - t1)
            lm, dm = _median_us(t_lin), _median_us(t_den)
            row = {"n": n, "columns": COLUMNS, "destination": where, "evaluators": 2, "calls": a.calls,
                   "linear_us": round(lm[0], 1), "linear_min_us": round(lm[1], 1), "linear_max_us": round(lm[2], 1),
                   "dense_us": round(dm[0], 1), "dense_min_us": round(dm[1], 1), "dense_max_us": round(dm[2], 1),
                   "linear_over_dense": round(lm[0] / dm[0], 2),
                   "linear_bytes": 2 * n * (4 + 16), "dense_bytes": 2 * (n * 4 + 2 * COLUMNS * 16)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            if n >= 1 << 17 and dm[0] > lm[0]:
                slower.append((n, where))
            del lin, den
        dev.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    if slower:
        sys.exit(f"the dense call is slower than the Linear one at {slower}")


if __name__ == "__main__":
    main()
