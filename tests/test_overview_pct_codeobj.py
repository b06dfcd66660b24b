"""The percentile overview's kernels in the built gfx950 code object (csrc/overview_pct.hip): the three are there, none spills a register --
vector or scalar -- and none uses scratch memory; a lane's 68-word table is in LDS, one wave's worth a workgroup.  No GPU needed: the
metadata note is read with llvm-readelf, by the means of tests/test_host_codeobj.py (tools/codeobj_report.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("overviewPctColumnsKernel", "overviewPctSliceKernel", "overviewPctEmitKernel")


def test_the_three_kernels_keep_their_registers():
    import codeobj_report as cr
    lib = os.path.join(ROOT, "signalizer_amd", "libsgz.so")
    if not (os.path.exists(lib) and os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("library or llvm tools not present")
    rows = cr.kernels(lib)
    for name in KERNELS:
        mine = [r for r in rows if name + "(" in r["demangled"]]
        assert len(mine) == 1, (name, len(mine))
        r = mine[0]
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, r
        assert r["group_segment_fixed_size"] == 68 * 65 * 4, r                # the table: 68 words x 64 lanes at a row stride of 65
        assert r["vgpr_count"] <= 128, r                                      # (no fewer waves a SIMD than the table's LDS allows)
