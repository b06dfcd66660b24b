"""What the host-graph routing (sgz_scope_set_mix / sgz_vector_set_mix) costs the ingest launch, on bench.py's cfg3 (Oscilloscope) and
cfg4 (Vectorscope) shapes: the same frame loop (512-sample callbacks, then the render thread's peak filter and vertices) once with the
identity routing and once with twice as many sources summed pairwise, each under rocprofv3 --kernel-trace --stats in a process of its
own; eagerly submitted as bench.py runs it (how many callbacks share a launch then depends on timing), and with SGZ_RT_OPT_DEFER_SUBMIT
(one launch per rendered frame: the counts are exact).  Prints, per handle, submission and routing, the ingest kernel's calls and mean
time and the kernel launches per rendered frame.

  python tools/mix_ingest_cost.py [--frames 600] [--out DIR]      the eight profiled runs + the table (DIR: a new temporary directory)
  python tools/mix_ingest_cost.py run <scope|vector> <identity|mix> --frames N [--defer]   one frame loop (what rocprofv3 runs)"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INGEST = {"scope": "scopeIngestKernel", "vector": "vectorIngestKernel"}


def run(kind, routing, frames, defer):
    import ctypes as C

    import numpy as np
    import torch

    from signalizer_amd import api, synth
    assert torch.cuda.is_available(), "needs a GPU"
    L = api.lib()
    if kind == "scope":                                           # bench.py views_workload, cfg3
        sr, W, nch = 192000.0, 19200, 2
        h = api.Scope(sample_rate=sr, window_size=float(W), num_channels=nch, trigger_mode=4, channel_mode=0, envelope_mode=2,
                      interpolation=3, max_block=512, trigger_threshold=0.05, trigger_channel=1.0, envelope_window=0.3)
        view = api.ScopeView(float(W), 0.0, 1.0, 1.0, 8 * W + 1, 0)
        nv = L.sgz_scope_vertex_count(h.h, C.byref(view))
        outs = [(np.empty((nv, 3), np.float32), np.empty((nv, 4), np.uint8)) for _ in (0, 1)]
    else:                                                         # cfg4
        sr, W, nch = 96000.0, 9600, 8
        h = api.Vector(sample_rate=sr, num_channels=nch, window_size=W, envelope_mode=2, lanes=8, fade_history=1, max_block=512,
                       envelope_window=0.3, stereo_window=0.1)
        outs = (np.empty((nch // 2, W, 3), np.float32), np.empty((nch // 2, W, 3), np.float32))
    if defer:
        h.set_option(api.RT_OPT_DEFER_SUBMIT, 1)
    per_frame = int(sr / 60)
    sources = nch
    if routing == "mix":                                          # 2 x nch sources, destination d = source 2d + source 2d + 1
        sources = 2 * nch
        M = np.zeros((nch, sources), np.uint8)
        for d in range(nch):
            M[d, 2 * d] = M[d, 2 * d + 1] = 1
        h.set_mix(M)
    x = (synth.gen(31, int(sr), per_frame * 64, sources) * np.float32(0.5)).astype(np.float32)
    busy = 0
    for f in range(frames):
        a = (f % 64) * per_frame
        for pos in range(a, a + per_frame, 512):
            while h.push(x[:, pos:min(pos + 512, a + per_frame)]) == api.SGZ_BUSY:
                busy += 1
        if kind == "scope":
            h.peak_filter(1 / 60, 8)
            h.vertices_all(view, (0, 1), (0, 0), outs)
        else:
            h.peak_filter(1 / 60)
            h.vertices_all(out=outs)
    torch.cuda.synchronize()
    print(json.dumps({"kind": kind, "routing": routing, "defer": defer, "frames": frames, "sources": sources, "refused_pushes": busy}))


def profile(args):
    if args.out is None:
        args.out = tempfile.mkdtemp(prefix="mix_ingest_cost_")
    os.makedirs(args.out, exist_ok=True)
    print(f"profiles under {args.out}")
    rows = []
    for kind, submit, routing in [(k, s, r) for k in ("scope", "vector") for s in ("eager", "defer") for r in ("identity", "mix")]:
        d = os.path.join(args.out, f"{kind}_{submit}_{routing}")
        cmd = ["rocprofv3", "-f", "csv", "--kernel-trace", "--stats", "-d", d, "-o", "t", "--",
               sys.executable, os.path.abspath(__file__), "run", kind, routing, "--frames", str(args.frames)] + (["--defer"] if submit == "defer" else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            raise SystemExit(f"{kind} / {routing}: exit status {r.returncode}")
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        assert stats, f"no kernel stats under {d}"
        k = list(csv.DictReader(open(stats[0])))
        launches = sum(int(x["Calls"]) for x in k)
        ing = [x for x in k if INGEST[kind] in x["Name"]]
        calls = sum(int(x["Calls"]) for x in ing)
        total_ns = sum(float(x["TotalDurationNs"]) for x in ing)
        row = dict(kind=kind, submit=submit, routing=routing, frames=args.frames, ingest_calls=calls,
                   ingest_mean_us=round(total_ns / max(calls, 1) / 1e3, 2), ingest_us_per_frame=round(total_ns / args.frames / 1e3, 2),
                   launches=launches, launches_per_frame=round(launches / args.frames, 3),
                   kernels={x["Name"][:60]: int(x["Calls"]) for x in k})
        rows.append(row)
        print(json.dumps(row))
    with open(os.path.join(args.out, "summary.json"), "w") as f:
        json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", nargs="?", default="profile", choices=("profile", "run"))
    ap.add_argument("kind", nargs="?", choices=("scope", "vector"))
    ap.add_argument("routing", nargs="?", choices=("identity", "mix"))
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--defer", action="store_true")
    ap.add_argument("--out", default=None, help="where the profiles and summary.json go (default: a new temporary directory)")
    a = ap.parse_args()
    if a.cmd == "run":
        run(a.kind, a.routing, a.frames, a.defer)
    else:
        profile(a)


if __name__ == "__main__":
    main()
