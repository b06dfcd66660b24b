"""Sweep of the one-round image-only launch's start-up schedule (spectrum_real.hip "one-round shape") in ONE process of a build with the
knobs at run time (-DSGZ_SCHED_SWEEP: tools/mkdebug.sh, or the release flags plus that define; sgz_debug_set_schedule,
sgz_debug_set_priorities), each setting timed as tools/ka_image_time.py does (image-only K_A and the step, rotated input and one
buffer), the whole grid `passes` times over so that a setting's own pass-to-pass spread stands beside the differences.  The winners
are then confirmed build against build (tools/ab_image.sh): the debug build carries the stamp code.
  grid "delays" (round 7):  Nyquist delay x mate delay (steps of ~1 k clocks) x mate-adjacent frame order
  grid "prio":              wave priorities of the two channel workgroups of a doubled CU (first-on-CU, mate) x their scope (0 the
                            workgroup's life behind its first requests, 1 behind pass 1's butterflies to the recombination) x the
                            Nyquist role's priority x mate delay {0, 1 k, 2 k}, mates adjacent
  grid "scope":             the mate's priority 1 .. 3 x all four scopes (kernels.hpp RealParams::prioScope: start behind the requests
                            or behind pass 1's butterflies, end with the recombination or never), no delay, Nyquist priority 0
Every setting's image and Nyquist words are compared with the first one's before anything is timed.
usage: SGZ_LIB=tools/ab/lib_sweep.so image_sched_sweep.py [passes] [frames] [delays|prio|scope]
       (image_sched_sweep.json goes under $SGZ_OUT, default the working directory)"""
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
grid = sys.argv[3] if len(sys.argv) > 3 else "prio"
NY, MATE, ADJ = (0, 1, 2, 4, 8), (0, 1, 2, 4, 6), (0, 1)
PAIRS, PNY, PMATE = ((0, 0, 0), (1, 0, 0), (3, 0, 0), (0, 1, 0), (0, 3, 0), (1, 0, 1), (3, 0, 1), (0, 1, 1), (0, 3, 1)), (0, 3), (0, 1, 2)
# a setting: (nyDelay, mateDelay, mateAdjacent, prioFirst, prioMate, prioNy, prioScope); the first one is the reference
if grid == "delays":
    settings = [(0, 0, 0, 0, 0, 0, 0)] + [(d, m, a, 0, 0, 0, 0) for a in ADJ for m in MATE for d in NY if (d, m, a) != (0, 0, 0)]
elif grid == "scope":
    PAIRS, PNY, PMATE = ((0, 0, 0),) + tuple((0, s, sc) for s in (1, 2, 3) for sc in (0, 1, 2, 3)) + ((1, 0, 2), (1, 0, 3)), (0,), (0,)
    settings = [(0, 0, 1, f, s, 0, sc) for (f, s, sc) in PAIRS]
else:
    settings = [(0, m, 1, f, s, n, sc) for m in PMATE for n in PNY for (f, s, sc) in PAIRS]
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


def apply(s):
    L.sgz_debug_set_schedule(s[0], s[1], s[2])
    L.sgz_debug_set_priorities(s[3], s[4], s[5], s[6])


# no output byte may depend on a setting
want = None
for s in settings:
    apply(s)
    rgba.zero_()
    got = plan.render(x, rgba=rgba).clone()
    api.check(L.sgz_stage_nyquist(plan.h, x.data_ptr(), x.stride(0), S, 1, ny.data_ptr(), None, None, stream))
    got_ny = ny.clone().view(torch.int32)
    if want is None:
        want = (got, got_ny)
    assert torch.equal(got, want[0]) and torch.equal(got_ny, want[1]), f"setting {s}: the output differs from setting {settings[0]}'s"
print(f"{len(settings)} settings: image and Nyquist words identical", flush=True)
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

        for s in settings:
            apply(s)
            k, _ = timeit(ka, 40, spin_ms=15.0, batches=3)
            t, _ = timeit(step, 40, spin_ms=15.0, batches=3)
            res.setdefault((proto,) + s, []).append((k, t))
    print(f"pass {p + 1} of {passes} done", flush=True)


def cell(proto, s):
    v = np.array(res[(proto,) + s])
    return f"{np.median(v[:, 1]):5.2f}+-{np.ptp(v[:, 1]):4.2f}[{np.median(v[:, 0]):5.2f}]"


for proto in ("rotated", "one_buffer"):
    print(f"\n{proto}: step us (median of {passes} passes; +- = max - min over the passes), K_A + copy in brackets")
    if grid == "delays":
        print("(0, 0, 0) is round 6's schedule")
        for a in ADJ:
            print(f" mateAdjacent {a}:   " + "  ".join(f"ny {d:>2d} k      " for d in NY))
            for m in MATE:
                print(f"  mate {m} k:  " + "  ".join(cell(proto, (d, m, a, 0, 0, 0, 0)) for d in NY))
    else:
        print("columns: priority of (first-on-CU, mate) / scope; (0, 0) / 0 with mate delay 0 and Nyquist priority 0 is the build's schedule")
        for c0 in range(0, len(PAIRS), 9):
            cols = PAIRS[c0:c0 + 9]
            print("                      " + "  ".join(f"({f}, {s}) / {sc}        " for (f, s, sc) in cols))
            for m in PMATE:
                for n in PNY:
                    print(f"  mate {m} k, ny prio {n}: " + "  ".join(cell(proto, (0, m, 1, f, s, n, sc)) for (f, s, sc) in cols))
out = [dict(protocol=proto, ny_delay=s[0], mate_delay=s[1], mate_adjacent=s[2], prio_first=s[3], prio_mate=s[4], prio_ny=s[5], prio_scope=s[6],
            step_us=[round(float(q[1]), 3) for q in res[(proto,) + s]], ka_us=[round(float(q[0]), 3) for q in res[(proto,) + s]])
       for proto in ("rotated", "one_buffer") for s in settings]
outdir = os.environ.get("SGZ_OUT", ".")
os.makedirs(outdir, exist_ok=True)
with open(os.path.join(outdir, "image_sched_sweep.json"), "w") as fh:
    json.dump(dict(frames=F, passes=passes, grid=grid, settings=out), fh)
