"""One video frame of the Spectrum line graph's vertices (renderTransformAsGraph, flood fill on), two ways, alternating call by call on
one LINE_GRAPH handle of cfg2's transform (N = W = 32768, Separate, P = 1024):
  (a) sgz_spectrum_render_lines into pageable host memory, then the vertices assembled in numpy -- what an adapter without the vertex
      stream has to do;
  (b) sgz_spectrum_render_line_vertices into a DEVICE buffer (a mapped VBO's stand-in), and into pinned host memory.
    python tools/bench_line_vertices.py [--calls 200] [--pairs 1 8]
Host clock around each call (every form waits for its result).  The ring holds one window of audio pushed before the timed calls; no
audio arrives between them, so every call transforms the same window and advances the filters once, as a paused frame loop would."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from signalizer_amd import api, config, synth


def assemble(res, out):
    """renderTransformAsGraph's vertices from the results [C][graphs][P][2] (two-sided mode, flood on) into out [vertices][3], in numpy"""
    C_, G, P, _ = res.shape
    ys = res[:, ::-1, :, ::-1].transpose(0, 1, 3, 2).reshape(C_, G * 2, P)          # k = 1, 0; right (.second) before left
    z = np.array([-0.5, 0.0] * G, np.float32)[None, :, None]
    x = np.arange(P, dtype=np.float32)[None, None, :]
    v = out.reshape(C_, 3 * G * 2 * P, 3)
    fill = v[:, :2 * G * 2 * P].reshape(C_, G * 2, P, 2, 3)
    fill[..., 0, 0] = x; fill[..., 0, 1] = ys; fill[..., 0, 2] = z
    fill[..., 1, 0] = x; fill[..., 1, 1] = 0.0; fill[..., 1, 2] = z
    strip = v[:, 2 * G * 2 * P:].reshape(C_, G * 2, P, 3)
    strip[..., 0] = x; strip[..., 1] = ys; strip[..., 2] = z
    return out


def run(pairs, calls):
    L = api.lib()
    cfg = config.spectrum_config(num_pairs=pairs, display_mode=config.DISPLAY_LINE_GRAPH)
    c = api.config_from_dict(cfg)
    h = C.c_void_p()
    api.check(L.sgz_spectrum_create(C.byref(c), C.byref(h)))
    W, P, mode = cfg["window_size"], cfg["axis_points"], cfg["channel_mode"]
    x = synth.gen(2, cfg["sample_rate"], W, 2 * pairs)
    for at in range(0, W, 8192):
        blk = np.ascontiguousarray(x[:, at:at + 8192])
        ptrs = (C.c_void_p * blk.shape[0])(*[blk[ch].ctypes.data for ch in range(blk.shape[0])])
        api.check(L.sgz_spectrum_push(h, ptrs, blk.shape[0], blk.shape[1]))
    api.check(L.sgz_spectrum_flush(h))
    n = api.line_graph_vertex_count(mode, pairs, P, True)
    res = np.zeros((pairs, 2, P, 2), np.float32)
    host = np.zeros((n, 3), np.float32)
    dev = torch.empty((n, 3), dtype=torch.float32, device="cuda:0")
    pinned = torch.empty((n, 3), dtype=torch.float32).pin_memory()

    def a():
        api.check(L.sgz_spectrum_render_lines(h, None, res.ctypes.data_as(C.c_void_p)))
        assemble(res, host)

    def b(buf):
        cnt = C.c_uint32(n)
        api.check(L.sgz_spectrum_render_line_vertices(h, None, 1, C.c_void_p(buf.data_ptr()), C.byref(cnt)))

    forms = {"a_render_lines_numpy": a, "b_vertices_device": lambda: b(dev), "b_vertices_pinned": lambda: b(pinned)}
    b(dev)                                                           # (a)'s assembly of the results (b) left = (b)'s stream
    for p in range(pairs):
        for k in range(2):
            api.check(L.sgz_spectrum_line_results(h, p, k, res[p, k].ctypes.data_as(C.c_void_p)))
    assert np.array_equal(assemble(res, host).view(np.uint32), dev.cpu().numpy().view(np.uint32))
    for _ in range(20):
        for f in forms.values():
            f()
    t = {k: [] for k in forms}
    names = list(forms)
    for i in range(calls):
        for name in names[i % len(names):] + names[:i % len(names)]:        # rotate the order call by call
            t0 = time.perf_counter()
            forms[name]()
            t[name].append((time.perf_counter() - t0) * 1e3)
    L.sgz_spectrum_destroy(h)
    return {"pairs": pairs, "vertices": n, "bytes": n * 12, "calls": calls,
            **{k: {"ms_median": float(np.median(v)), "ms_p10": float(np.percentile(v, 10)), "ms_p90": float(np.percentile(v, 90))} for k, v in t.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 8])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rows = []
    for pairs in args.pairs:
        r = run(pairs, args.calls)
        rows.append(r)
        print(f"pairs {pairs}: {r['vertices']} vertices  (a) render_lines + numpy {r['a_render_lines_numpy']['ms_median']:.4f} ms   "
              f"(b) device {r['b_vertices_device']['ms_median']:.4f} ms   pinned {r['b_vertices_pinned']['ms_median']:.4f} ms", flush=True)
    print(json.dumps({"shape": "cfg2 transform, Separate, P = 1024, flood fill on", "rows": rows}))


if __name__ == "__main__":
    main()
