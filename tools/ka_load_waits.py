#!/usr/bin/env python3
"""Where the channel role of stftRealKernel<4, ...> (N = 32768) waits for its requests, from a gfx950 listing of spectrum_real.hip:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fhip-fp32-correctly-rounded-divide-sqrt -fno-slp-vectorize -x hip --cuda-device-only -S \
          signalizer_amd/csrc/spectrum_real.hip -o real.s
    python tools/ka_load_waits.py real.s [more listings]
    python tools/ka_load_waits.py --source      (compiles the tree's spectrum_real.hip with the build's flags into a temporary listing)
Per instantiation: the requests (vector-memory loads) between the role's start and its first `s_barrier`, every `s_waitcnt vmcnt(n)`
among them, and the number of vector instructions (`v_` prefix) between consecutive events.  The load counter is waited for in order,
so a wait at vmcnt(n) behind the last request means "all but the last n requests have landed": a role that works under its samples'
arrival shows a LADDER of falling counts with vector work between the rungs, one that waits for everything first shows one low count.
The channel role's start: the function's entry, or in an image-only instantiation (MIX = 4) the target of the entry block's branch
past the Nyquist role (`if (blockIdx.x >= heavyUnits)`).  Straight listing order; the few blocks between the start and the barrier are
lane-predicated table requests, which every wave passes through.  No GPU needed."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = re.compile(r"^(_ZN3sgz14stftRealKernelILi4ELb([01])ELi(\d)ELb([01])EEEvNS_10RealParamsE):")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize", "-x", "hip",
         "--cuda-device-only", "-S"]


def listing_of_source(out):
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), "hipcc")
    subprocess.check_call([hipcc] + FLAGS + [os.path.join(ROOT, "signalizer_amd", "csrc", "spectrum_real.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    return out


def is_request(op):
    return op.startswith(("global_load", "flat_load", "buffer_load"))


def channel_roles(listing):
    """{instantiation: [events]}, events in listing order: ("load", op) | ("wait", n) | ("valu", count)"""
    lines = open(listing).read().splitlines()
    roles = {}
    for at, line in enumerate(lines):
        m = KERNEL.match(line)
        if not m:
            continue
        name = f"stftRealKernel<4, {'true' if m.group(2) == '1' else 'false'}, {m.group(3)}, {'true' if m.group(4) == '1' else 'false'}>"
        end = next(i for i in range(at, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = lines[at + 1:end]
        start = 0
        if m.group(3) == "4":                                   # image-only: the entry block branches past the Nyquist role
            target = next(l.split()[-1] for l in body if l.startswith("\t") and not l.strip().startswith((".", ";")) and l.split()[-1].startswith(".LBB"))   # the first jump's label
            start = body.index(target + ":")
        events, valu = [], 0
        for l in body[start:]:
            s = l.strip()
            if not l.startswith("\t") or not s or s.startswith((".", ";")):
                continue
            op = s.split()[0]
            if op == "s_barrier":
                break
            w = re.search(r"vmcnt\((\d+)\)", s) if op == "s_waitcnt" else None
            if is_request(op) or w:
                if valu:
                    events.append(("valu", valu))
                    valu = 0
                events.append(("wait", int(w.group(1))) if w else ("load", op))
            elif op.startswith("v_"):
                valu += 1
        if valu:
            events.append(("valu", valu))
        roles[name] = events
    return roles


def summary(events):
    """what the tests hold: the number of requests, the waits behind the LAST request with the vector instructions that follow each,
    the first wait of the role that has a vector instruction behind it (before the next event) and the requests issued before it"""
    last = max((i for i, e in enumerate(events) if e[0] == "load"), default=-1)
    requests = sum(1 for e in events if e[0] == "load")
    waits = [e[1] for e in events if e[0] == "wait"]
    ladder = []
    for i in range(last + 1, len(events)):
        if events[i][0] == "wait":
            ladder.append((events[i][1], events[i + 1][1] if i + 1 < len(events) and events[i + 1][0] == "valu" else 0))
    first = next(((e[1], sum(1 for x in events[:i] if x[0] == "load")) for i, e in enumerate(events)
                  if e[0] == "wait" and i + 1 < len(events) and events[i + 1][0] == "valu" and i > last), None)
    return {"requests": requests, "waits": waits, "ladder": ladder, "first_working_wait": first}


def report(listing, name=None):
    out = [f"{name or listing}"]
    for inst, events in channel_roles(listing).items():
        s = summary(events)
        out.append(f"  {inst}: {s['requests']} requests before the first barrier")
        text, run = [], 0
        for kind, v in events:
            if kind == "load":
                run += 1
                continue
            if run:
                text.append(f"{run} requests")
                run = 0
            text.append(f"vmcnt({v})" if kind == "wait" else f"{v} v_")
        if run:
            text.append(f"{run} requests")
        out.append("    in order: " + " | ".join(text))
        out.append("    behind the last request, wait -> vector instructions until the next wait: " +
                   " ".join(f"{n}->{v}" for n, v in s["ladder"]))
        out.append(f"    distinct counts behind the last request: {len(set(n for n, _ in s['ladder']))}; the first wait with vector work behind it: "
                   f"vmcnt({s['first_working_wait'][0] if s['first_working_wait'] else '-'})")
    return "\n".join(out)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args == ["--source"]:
        with tempfile.TemporaryDirectory() as d:
            print(report(listing_of_source(os.path.join(d, "real.s")), "signalizer_amd/csrc/spectrum_real.hip"))
    else:
        for a in args:
            print(report(a))
