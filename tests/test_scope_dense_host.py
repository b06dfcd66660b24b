"""The Oscilloscope's dense stream (sgz_scope_dense_*, csrc/scope_dense.hip) without a GPU: the exports, the count on a NULL handle,
the column bounds  ceil(b n / cols)  of the definition (include/sgz.h) against a brute-force assignment of samples to columns, and the
kernels in the built gfx950 code object: no scratch, no spill."""
import ctypes as C
import os
import sys

import pytest

from signalizer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("sgz_scope_dense_vertex_count", "sgz_scope_dense_vertices", "sgz_scope_dense_vertices_all", "sgz_scope_dense_vertices_device",
         "sgz_scope_dense_device")


def test_exports_exist():
    L = api.lib()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(L, name), name
    for name in ("dense_vertices", "dense_vertices_all", "dense_vertex_count"):
        assert callable(getattr(api.Scope, name))
    assert callable(api.scope_dense_device)
    with open(os.path.join(ROOT, "include", "sgz.h")) as f:
        header = f.read()
    assert all(name + "(" in header for name in NAMES) and "#define SGZ_ABI_VERSION 5" in header


def test_count_and_refusals_without_a_handle():
    L = api.lib()
    assert L.sgz_scope_dense_vertex_count.restype is C.c_size_t
    for columns in (0, 1, 2048, 0xffffffff):
        assert L.sgz_scope_dense_vertex_count(None, columns) == 0
    cnt = C.c_uint32(16)
    buf = (C.c_float * 48)()
    assert L.sgz_scope_dense_vertices(None, 8, 0, 0, buf, None, C.byref(cnt)) == api.SGZ_EINVAL and cnt.value == 16
    assert L.sgz_scope_dense_vertices_device(None, 8, 0, 0, buf, None, C.byref(cnt)) == api.SGZ_EINVAL
    assert L.sgz_scope_dense_vertices_all(None, 8, 0, None, None, None, None, None) == api.SGZ_EINVAL
    assert L.sgz_scope_dense_device(None, 100, 100, 1, 50, 8, None, None) == api.SGZ_EINVAL


def test_column_bounds_partition_the_strip():
    """column b = ceil(b n / cols) <= i < ceil((b + 1) n / cols), cols = min(columns, n): against the brute-force rule "sample i belongs to
    column floor(i cols / n)" -- for all n <= 64, columns <= 70 every column is non-empty, they tile [0, n) in order, and their lengths
    differ by at most one"""
    for n in range(1, 65):
        for columns in range(1, 71):
            cols = min(columns, n)
            st = [(b * n + cols - 1) // cols for b in range(cols + 1)]
            assert st[0] == 0 and st[-1] == n
            owner = [(i * cols) // n for i in range(n)]                 # brute force
            members = [[i for i in range(n) if owner[i] == b] for b in range(cols)]
            for b in range(cols):
                assert members[b] == list(range(st[b], st[b + 1])), (n, columns, b)
                assert len(members[b]) >= 1
            lengths = [len(m) for m in members]
            assert max(lengths) - min(lengths) <= 1 and max(lengths) == -(-n // cols)
            if columns >= n:
                assert lengths == [1] * n


def test_dense_kernels_in_the_code_object_without_scratch():
    import codeobj_report as cr
    lib = os.path.join(ROOT, "signalizer_amd", "libsgz.so")
    if not (os.path.exists(lib) and os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("library or llvm tools not present")
    rows = cr.kernels(lib)
    for kernel, forms in (("scopeDenseWaveKernel", 2), ("scopeDenseChunkKernel", 1), ("scopeDenseFoldKernel", 2)):
        mine = [r for r in rows if kernel in r["demangled"]]
        assert len(mine) == forms, [r["demangled"] for r in mine]
        for r in mine:
            assert not r.get("private_segment_fixed_size", 0) and not r.get("vgpr_spill_count", 0) and not r.get("sgpr_spill_count", 0), r
    # the Linear kernel it reduces shares ringPhys / evalSample with them (scope_ring.hpp) and is still there
    assert len([r for r in rows if "scopeWaveLinearKernel" in r["demangled"]]) == 1
