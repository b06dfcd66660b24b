"""The schedule of one IMAGE-ONLY K_A launch (debug build, tools/mkdebug.sh): per workgroup the start / end wall clock (100 MHz), its CU
and its index in the launch, by class -- first channel workgroup on its CU, second channel workgroup on its CU (a "mate": index >= #CUs),
Nyquist workgroup -- and per class of CU (two channel workgroups / channel + Nyquist / one channel workgroup alone).  The input rotates
over copies of the audio past the Infinity Cache, as bench.py's does.
usage: SGZ_LIB=tools/ab/lib_dbg.so unit_trace_image.py [frames] [nyDelay mateDelay mateAdjacent] [name] [prioFirst prioMate prioNy prioScope]
       (delays in steps of ~1 k clocks, priorities 0 .. 3 and their scope as in kernels.hpp, -1: the build's default; name: <name>.npy /
       <name>.txt under $SGZ_OUT, default the working directory)"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from signalizer_amd import api, config, synth

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 348
sched = [int(a) for a in sys.argv[2:5]] if len(sys.argv) > 4 else [-1, -1, -1]
name = sys.argv[5] if len(sys.argv) > 5 else "unit_trace_image"
prio = [int(a) for a in sys.argv[6:10]] if len(sys.argv) > 9 else [-1, -1, -1, -1]
cfg = config.cfg2()
S = cfg["window_size"] + cfg["hop"] * (frames - 1)
x = torch.from_numpy(synth.gen(config.CFG2_SEED, 48000, S, 2)).cuda()
xs = [x] + [x.clone() for _ in range(max(0, -int(-288e6 // (x.numel() * 4)) - 1))]
plan = api.Plan(cfg).upload()
F = plan.num_frames(S)
cus = torch.cuda.get_device_properties(0).multi_processor_count
clk = torch.zeros(256 + 4 * 2 * F, dtype=torch.int64, device="cuda")
L = api.lib()
L.sgz_debug_set_ablate(0xffff << 16)
L.sgz_debug_set_schedule(*sched)
L.sgz_debug_set_priorities(*prio)
L.sgz_debug_phase_clocks_image.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
lines = []


def say(s):
    print(s)
    lines.append(s)


spans = []
for rep in range(2 * len(xs)):                                       # the last launch is the one kept; every launch reads a cold copy
    b = xs[rep % len(xs)]
    clk.zero_()
    api.check(L.sgz_debug_phase_clocks_image(plan.h, b.data_ptr(), b.stride(0), S, clk.data_ptr(), None))
    torch.cuda.synchronize()
    t = clk.cpu().numpy()[256:].reshape(2 * F, 4)
    used = t[:, 1] != 0
    spans.append((t[used, 1].max() - t[used, 0].min()) * 0.01)
t = t[used]
slot = np.nonzero(used)[0]
t0 = t[:, 0].min()
start, end = (t[:, 0] - t0) * 0.01, (t[:, 1] - t0) * 0.01            # us
hw, xcc, index = t[:, 2], t[:, 3] & 0xf, t[:, 3] >> 32
cu = (hw >> 8) & 0xf; sh = (hw >> 12) & 1; se = (hw >> 13) & 0x7
cuid = ((xcc * 8 + se) * 2 + sh) * 16 + cu
nyq = (slot & 1) == 1
mate = ~nyq & (index >= cus)
first = ~nyq & ~mate
frame = slot >> 1
say(f"frames {F}  workgroups {len(t)} ({int(first.sum())} first-on-CU channel, {int(mate.sum())} second-on-CU channel, {int(nyq.sum())} Nyquist)  "
    f"schedule (nyDelay, mateDelay, mateAdjacent) {sched}  priorities (first, mate, Nyquist, scope) {prio}  distinct CUs {len(set(cuid.tolist()))}")
say(f"launch span (first start -> last end), the {len(spans)} launches: median {np.median(spans):.2f} min {min(spans):.2f} max {max(spans):.2f} us; below: the last one, {end.max():.2f} us")
for label, m in (("first-on-CU channel", first), ("second-on-CU channel", mate), ("Nyquist", nyq)):
    if m.any():
        d = end[m] - start[m]
        say(f"{label:22s} n {int(m.sum()):3d}  start {start[m].min():5.2f} .. {start[m].max():5.2f}  end {end[m].min():5.2f} .. median {np.median(end[m]):5.2f} .. {end[m].max():5.2f}  "
            f"duration {d.min():5.2f} / {np.median(d):5.2f} / {d.max():5.2f} us")
last = int(np.argmax(end))
say(f"the launch's last workgroup: {'Nyquist' if nyq[last] else 'second-on-CU channel' if mate[last] else 'first-on-CU channel'} (index {int(index[last])}, CU {int(cuid[last])})")
# classes of CU
kinds = {}
shared_cu = 0
for c in set(cuid.tolist()):
    on = np.where(cuid == c)[0]
    k = (int((first | mate)[on].sum()), int(nyq[on].sum()))
    kinds.setdefault(k, []).append(end[on].max())
    if last in on:
        last_kind = k
    chans = on[~nyq[on]]
    if len(chans) == 2 and {int(index[chans[0]]) + cus, int(index[chans[0]]) - cus} & {int(index[chans[1]])}:
        shared_cu += 1
for k in sorted(kinds):
    e = np.array(kinds[k])
    say(f"CUs with {k[0]} channel + {k[1]} Nyquist workgroups: {len(e):3d}  last end on the CU: {e.min():5.2f} .. median {np.median(e):5.2f} .. {e.max():5.2f} us")
say(f"the launch's last workgroup runs on a CU with {last_kind[0]} channel + {last_kind[1]} Nyquist workgroups")
say(f"CUs whose two channel workgroups are b and b + {cus}: {shared_cu}")
doubled = [c for c in set(cuid.tolist()) if int((first | mate)[cuid == c].sum()) == 2]
if doubled:
    ef = np.array([end[(cuid == c) & first].max() for c in doubled if ((cuid == c) & first).any() and ((cuid == c) & mate).any()])
    em = np.array([end[(cuid == c) & mate].max() for c in doubled if ((cuid == c) & first).any() and ((cuid == c) & mate).any()])
    if len(ef):
        say(f"doubled CUs: first-on-CU workgroup ends {ef.min():5.2f} .. median {np.median(ef):5.2f} .. {ef.max():5.2f}, its mate {em.min():5.2f} .. median {np.median(em):5.2f} .. {em.max():5.2f}; "
            f"mate end - first end: {(em - ef).min():5.2f} .. median {np.median(em - ef):5.2f} .. {(em - ef).max():5.2f} us")
pairs = [(int(frame[a]), int(frame[b])) for a in np.where(first)[0] for b in np.where(mate & (cuid == cuid[a]))[0]]
if pairs:
    gap = np.array([abs(p - q) for p, q in pairs])
    say(f"frames of the two channel workgroups of a CU: |difference| min {gap.min()} median {int(np.median(gap))} max {gap.max()}")
hist, edges = np.histogram(end, bins=12)
say("end-time histogram: " + " ".join(f"{edges[i]:.1f}:{hist[i]}" for i in range(len(hist))))
out = os.environ.get("SGZ_OUT", ".")
os.makedirs(out, exist_ok=True)
np.save(os.path.join(out, name + ".npy"), np.stack([start, end, cuid.astype(np.float64), index.astype(np.float64), nyq.astype(np.float64), frame.astype(np.float64)], 1))
with open(os.path.join(out, name + ".txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
