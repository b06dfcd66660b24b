#!/usr/bin/env python3
"""Static instruction counts of decayColourFusedKernel<4>'s emission loop, from a gfx950 listing of spectrum_post.hip:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fhip-fp32-correctly-rounded-divide-sqrt -x hip --cuda-device-only -S \
          signalizer_amd/csrc/spectrum_post.hip -o post.s
    python tools/kb_emission_count.py post.s [more listings]
The emission loop is the outermost loop that holds the carry wait (the only `s_sleep` of the kernel): every block the listing marks as
"in Loop: Header=<that loop>", the header itself, and the loops nested in it.  No GPU needed."""
import re
import sys
from collections import Counter

KERNEL = "_ZN3sgz22decayColourFusedKernelILi4EEEvNS_11DecayParamsE"


def classify(op):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith(("s_load", "s_buffer_load")):
        return "SMEM"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    return "other"


def emission_loop(listing):
    text = open(listing).read()
    a = text.index(KERNEL + ":")
    body = text[a:text.index(".Lfunc_end", a)].splitlines()
    # blocks: label -> (the loop header it belongs to, instructions)
    blocks, cur = [], {"label": "entry", "header": None, "parent": None, "ins": []}
    for line in body:
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", line)
        n = re.match(r"^; %bb\.\d+:\s*(;.*)?$", line)
        if m or n:
            blocks.append(cur)
            note = (m.group(2) if m else n.group(1)) or ""
            cur = {"label": m.group(1) if m else "bb", "header": None, "parent": None, "ins": [], "is_header": "Loop Header" in note or "Inner Loop Header" in note}
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
            if h:
                cur["header"] = ".L" + h.group(1)
            h = re.search(r"Parent Loop (BB\d+_\d+)", note)
            if h:
                cur["parent"] = ".L" + h.group(1)
            continue
        s = line.strip()
        if line.startswith("\t") and s and not s.startswith((".", ";")):
            cur["ins"].append(s.split()[0])
    blocks.append(cur)
    sleeper = next(b for b in blocks if "s_sleep" in b["ins"])
    inner = sleeper["header"]
    outer = next((b["parent"] for b in blocks if b["label"] == inner and b["parent"]), inner)
    loops = {outer, inner}
    ins = [op for b in blocks if b["label"] in loops or b["header"] in loops for op in b["ins"]]
    return ins


if __name__ == "__main__":
    for listing in sys.argv[1:]:
        ins = emission_loop(listing)
        c = Counter(classify(op) for op in ins)
        f64 = sum(1 for op in ins if "_f64" in op)
        print(f"{listing}: {len(ins)} instructions  VALU {c['VALU']} (fp64 {f64})  SALU {c['SALU']}  branch {c['branch']}  LDS {c['LDS']}  VMEM {c['VMEM']}  SMEM {c['SMEM']}")
