"""The Vectorscope's stereo meter readout and the Lissajous kernel without a GPU.

sgz_vector_meters_from_filters is drawStereoMeters' arithmetic (VectorscopeRendering.cpp:766-776) on the filter states: held bit for bit to
a plain fp32 restatement (numpy float32, atanf from libm) over a grid of filter values with every special case the division and the
isnormal fallback meet.  vectorLissajousKernel (drawRectPlot) is checked in the built gfx950 code object: no scratch, no spill."""
import ctypes as C
import ctypes.util
import itertools
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

F32 = np.float32
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.atanf.restype = C.c_float
_libm.atanf.argtypes = [C.c_float]

SUB = float(np.finfo(F32).tiny)                              # smallest normal float
GRID = [0.0, -0.0, 1.0, -1.0, 0.5, 2.0, -3.0, 1e-40, -1e-40, 1e-45, SUB, 1e-38, 1.5e-38, 3e38, -3e38, 1e30,
        float("inf"), float("-inf"), float("nan"), 0.25, 7.0, 1e-20]


def meters_ref(balance, phase):
    """drawStereoMeters: balance = atan(y / x) / (pi_f * 0.5f), 0.5f unless normal; stereo = phase * 0.5f + 0.5f (all float)"""
    half_pi = F32(np.pi) * F32(0.5)
    bal, ste = [], []
    with np.errstate(all="ignore"):
        for k in (0, 1):
            q = F32(balance[k][1]) / F32(balance[k][0])
            b = F32(_libm.atanf(float(q))) / half_pi
            if not (np.isfinite(b) and abs(b) >= F32(SUB)):
                b = F32(0.5)
            bal.append(b)
            ste.append(F32(phase[k]) * F32(0.5) + F32(0.5))
    return np.array(bal, F32), np.array(ste, F32)


def _filters(b00, b01, b10, b11, p0, p1):
    f = api.VectorFilters()
    f.balance[0][0], f.balance[0][1], f.balance[1][0], f.balance[1][1] = b00, b01, b10, b11
    f.phase[0], f.phase[1] = p0, p1
    return f


def _bits(a):
    return np.asarray(a, F32).view(np.uint32)


def test_meters_from_filters_is_the_restatement():
    rng = np.random.default_rng(9)
    cases = 0
    for x, y in itertools.product(GRID, GRID):
        # index 0 carries the grid pair, index 1 the swapped pair; phases walk the grid alongside
        p0, p1 = GRID[cases % len(GRID)], GRID[(cases * 7 + 3) % len(GRID)]
        f = _filters(x, y, y, x, p0, p1)
        m = api.vector_meters_from_filters(f)
        rb, rs = meters_ref([[f.balance[0][0], f.balance[0][1]], [f.balance[1][0], f.balance[1][1]]], [f.phase[0], f.phase[1]])
        assert np.array_equal(_bits(m.balance[:]), _bits(rb)), (x, y, m.balance[:], rb)
        assert np.array_equal(_bits(m.stereo[:]), _bits(rs)), (p0, p1, m.stereo[:], rs)
        cases += 1
    for _ in range(2000):                                     # what push produces: non-negative mean squares, phase in [-1, 1]
        v = rng.random(4).astype(F32) ** 3
        ph = (rng.random(2).astype(F32) * 2 - 1)
        f = _filters(*[float(t) for t in v], *[float(t) for t in ph])
        m = api.vector_meters_from_filters(f)
        rb, rs = meters_ref([[f.balance[0][0], f.balance[0][1]], [f.balance[1][0], f.balance[1][1]]], [f.phase[0], f.phase[1]])
        assert np.array_equal(_bits(m.balance[:]), _bits(rb)) and np.array_equal(_bits(m.stereo[:]), _bits(rs))
        cases += 1
    assert cases == len(GRID) ** 2 + 2000


def test_meters_special_values():
    """the fallback by name: 0 / 0 (NaN), a zero ratio (atan 0 = 0), a subnormal quotient, a ratio of -inf / inf -> 0.5f"""
    for x, y in [(0.0, 0.0), (1.0, 0.0), (1.0, -0.0), (1.0, 1e-40), (1.0, 1e-38), (float("inf"), 1.0), (float("nan"), 1.0)]:
        m = api.vector_meters_from_filters(_filters(x, y, x, y, 0.0, 0.0))
        assert m.balance[0] == np.float32(0.5) and m.balance[1] == np.float32(0.5), (x, y)
    m = api.vector_meters_from_filters(_filters(1.0, 1.0, 0.0, 1.0, -1.0, 1.0))
    assert m.balance[0] == np.float32(0.5) and m.balance[1] == np.float32(1.0)        # atan(1) / (pi / 2); atan(+inf) / (pi / 2)
    assert m.stereo[0] == 0.0 and m.stereo[1] == 1.0
    m = api.vector_meters_from_filters(_filters(1.0, -1.0, -1.0, 1.0, 0.0, 0.0))     # negative ratios: negative positions, as the reference
    assert m.balance[0] == np.float32(-0.5) and m.balance[1] == np.float32(-0.5)
    with pytest.raises(api.SgzError):
        api.check(api.lib().sgz_vector_meters_from_filters(None, None))


def test_lissajous_kernel_in_the_code_object_without_scratch():
    import codeobj_report as cr
    lib = os.path.join(ROOT, "signalizer_amd", "libsgz.so")
    if not (os.path.exists(lib) and os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("library or llvm tools not present")
    rows = [r for r in cr.kernels(lib) if "vectorLissajousKernel" in r["demangled"]]
    assert len(rows) == 1, [r["demangled"] for r in rows]
    r = rows[0]
    assert not r.get("private_segment_fixed_size", 0) and not r.get("vgpr_spill_count", 0) and not r.get("sgpr_spill_count", 0), r
