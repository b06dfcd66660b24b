"""Sweep of the one-round image-only launch's start-up schedule (spectrum_real.hip "one-round shape") in ONE process of the debug build
(tools/mkdebug.sh; sgz_debug_set_schedule): Nyquist delay x mate delay (steps of ~1 k clocks) x mate-adjacent frame order, each setting
timed as tools/ka_image_time.py does (image-only K_A and the step, rotated input and one buffer), the whole grid `passes` times over
so that a setting's own pass-to-pass spread stands beside the differences.  The winners are then confirmed build against build
(tools/ab_image.sh): the debug build carries the stamp code.
usage: SGZ_LIB=tools/ab/lib_dbg.so image_sched_sweep.py [passes] [frames]      (image_sched_sweep.json goes under $SGZ_OUT, default the working directory)"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from signalizer_amd import api, config, synth
from ka_time import timeit

passes = int(sys.argv[1]) if len(sys.argv) > 1 else 3
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 348
NY, MATE, ADJ = (0, 1, 2, 4, 8), (0, 1, 2, 4, 6), (0, 1)
cfg = config.cfg2()
S = cfg["window_size"] + cfg["hop"] * (frames - 1)
x = torch.from_numpy(synth.gen(config.CFG2_SEED, 48000, S, 2)).cuda()
plan = api.Plan(cfg).upload()
L = api.lib()
stream = torch.cuda.current_stream().cuda_stream
F = plan.num_frames(S)
ny = torch.empty((F, plan.C, 2), dtype=torch.float32, device="cuda")
rgba = torch.empty((F, plan.P, 4), dtype=torch.uint8, device="cuda")
nbuf = max(1, -int(-288e6 // (x.numel() * 4)))
xs = [x] + [x.clone() for _ in range(nbuf - 1)]
res = {}
for p in range(passes):
    for proto, n in (("rotated", nbuf), ("one_buffer", 1)):
        turn = [0]

        def nextx():
            turn[0] = (turn[0] + 1) % n
            return xs[turn[0]]

        def ka():
            b = nextx()
            api.check(L.sgz_stage_nyquist(plan.h, b.data_ptr(), b.stride(0), S, 1, ny.data_ptr(), None, None, stream))

        def step():
            plan.render(nextx(), rgba=rgba)

        for a in ADJ:
            for m in MATE:
                for d in NY:
                    L.sgz_debug_set_schedule(d, m, a)
                    k, _ = timeit(ka, 40, spin_ms=15.0, batches=3)
                    s, _ = timeit(step, 40, spin_ms=15.0, batches=3)
                    res.setdefault((proto, a, m, d), []).append((k, s))
    print(f"pass {p + 1} of {passes} done", flush=True)
out = []
for proto in ("rotated", "one_buffer"):
    base = np.median([v[1] for v in res[(proto, 0, 0, 0)]])
    print(f"\n{proto}: step us (median of {passes} passes; +- = max - min over the passes), K_A + copy in brackets; (0, 0, 0) is the parent's schedule")
    for a in ADJ:
        print(f" mateAdjacent {a}:   " + "  ".join(f"ny {d:>2d} k      " for d in NY))
        for m in MATE:
            cells = []
            for d in NY:
                v = np.array(res[(proto, a, m, d)])
                cells.append(f"{np.median(v[:, 1]):5.2f}+-{np.ptp(v[:, 1]):4.2f}[{np.median(v[:, 0]):5.2f}]")
                out.append(dict(protocol=proto, mate_adjacent=a, mate_delay=m, ny_delay=d, step_us=[round(float(q), 3) for q in v[:, 1]],
                                ka_us=[round(float(q), 3) for q in v[:, 0]]))
            print(f"  mate {m} k:  " + "  ".join(cells))
outdir = os.environ.get("SGZ_OUT", ".")
os.makedirs(outdir, exist_ok=True)
with open(os.path.join(outdir, "image_sched_sweep.json"), "w") as fh:
    json.dump(dict(frames=F, passes=passes, settings=out), fh)
