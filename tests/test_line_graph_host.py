"""The Spectrum line graph's draw list without a GPU (sgz_line_graph_draws, sgz_line_graph_vertex_count): renderTransformAsGraph's
order (SpectrumRendering.cpp:794-897) restated in plain Python -- per pair, flood fills then strips, k = 1 then 0, the right side (two-sided
modes only) before the left --, colours from api.rotate_hue plus JUCE's floatToUInt8, and the model coefficients.  lineGraphVertexKernel
is checked in the built gfx950 code object: no scratch, no LDS."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

F32 = np.float32
MODES = range(8)                                         # SGZ_CH_LEFT .. SGZ_CH_COMPLEX
TWO_SIDED = {4, 5, 6}                                    # Phase, Separate, MidSide
ONE = [(200, 40, 10, 255), (30, 220, 90, 128)]
TWO = [(10, 60, 250, 7), (250, 250, 0, 0)]


def float_to_uint8(a):
    """juce ColourHelpers::floatToUInt8 (juce_Colour.cpp:27-30) in fp32"""
    a = F32(a)
    return 0 if a <= 0 else 255 if a >= 1 else int(a * F32(255.996))


def draws_ref(mode, pairs, P, flood_alpha, primitive_size, rendering_scale):
    S = 2 if mode in TWO_SIDED else 1
    flood = F32(flood_alpha) != 0
    per_pair = 2 * S * P * (3 if flood else 1)
    fill_w = F32(rendering_scale)
    strip_w = max(F32(0.001), F32(float(rendering_scale) * float(F32(primitive_size))))
    out = []
    for p in range(pairs):
        first = p * per_pair
        for strip in ([False, True] if flood else [True]):
            for k in (1, 0):
                for side in ([1, 0] if S == 2 else [0]):
                    base = TWO[k] if side else ONE[k]
                    rgb = api.rotate_hue(base[:3], float(F32(p) / F32(pairs)))
                    alpha = base[3] if strip else float_to_uint8(flood_alpha)
                    n = P if strip else 2 * P
                    out.append((first, n, 3 if strip else 1, p, k, side, (*[int(c) for c in rgb], alpha), strip_w if strip else fill_w))
                    first += n
    return out


def _style(flood_alpha, primitive_size=1.5, rendering_scale=2.0):
    return api.line_graph_style(ONE, TWO, flood_alpha, primitive_size, rendering_scale)


@pytest.mark.parametrize("mode", MODES)
def test_draw_list_is_the_restatement(mode):
    for pairs, P, (fa, ps, rs) in itertools.product([1, 2, 5, 32], [2, 3, 300, 1024], [(0.0, 1.0, 1.0), (0.25, 1.5, 2.0), (1.0, 1e-4, 1.0)]):
        got, model = api.line_graph_draws(_style(fa, ps, rs), mode, pairs, P)
        want = draws_ref(mode, pairs, P, fa, ps, rs)
        assert len(got) == len(want), (mode, pairs, P, fa)
        for g, w in zip(got, want):
            assert (int(g["first"]), int(g["count"]), int(g["primitive"]), int(g["pair"]), int(g["graph"]), int(g["side"])) == w[:6], (g, w)
            assert tuple(int(c) for c in g["rgba"]) == w[6], (mode, pairs, P, g, w)
            assert F32(g["line_width"]).view(np.uint32) == F32(w[7]).view(np.uint32), (g, w)
        flood = fa != 0.0
        total = api.line_graph_vertex_count(mode, pairs, P, flood)
        assert total == int(got["count"].sum()) == pairs * 2 * (2 if mode in TWO_SIDED else 1) * P * (3 if flood else 1)
        assert int(got["first"][-1] + got["count"][-1]) == total
        # translate(-1, -1, 0) then scale(GLfloat(1.0 / ((P - 1) * 0.5)), 2, 1)
        assert model.view(np.uint32).tolist() == np.array([F32(1.0 / ((P - 1) * 0.5)), 2.0, -1.0, -1.0], F32).view(np.uint32).tolist()


def test_fill_alpha_is_floattouint8():
    """a fill draws withAlpha(alphaFloodFill): the byte floatToUInt8 makes of it, over a grid that includes its edges; strips keep the
    colour's own alpha"""
    grid = [1.0, 0.5, 1 / 255, 254.5 / 255, 0.999, 0.0039, 0.004, 1e-7, -0.0, -0.25, -3.0, 1.0001, 7.0, 0.75, 0.1, float(np.nextafter(F32(1), F32(0)))]
    grid += list(np.linspace(0.001, 0.999, 97))
    for a in grid:
        got, _ = api.line_graph_draws(_style(a), 5, 3, 16)
        if F32(a) == 0:
            assert (got["primitive"] == api.PRIM_LINE_STRIP).all()          # -0.0: no flood fill either
            continue
        fills = got[got["primitive"] == api.PRIM_LINES]
        assert len(fills) == 3 * 4
        assert (fills["rgba"][:, 3] == float_to_uint8(a)).all(), (a, fills["rgba"][:, 3], float_to_uint8(a))
        strips = got[got["primitive"] == api.PRIM_LINE_STRIP]
        want = [TWO[k][3] if s else ONE[k][3] for k, s in zip(strips["graph"], strips["side"])]
        assert strips["rgba"][:, 3].tolist() == want
    assert float_to_uint8(0.5) == 127 and float_to_uint8(1 / 255) == 1 and float_to_uint8(1.0) == 255 and float_to_uint8(-1) == 0


def test_zero_flood_alpha_means_no_fill_vertices():
    got, _ = api.line_graph_draws(_style(0.0), 1, 2, 10)
    assert len(got) == 2 * 2 and (got["count"] == 10).all()
    assert api.line_graph_vertex_count(1, 2, 10, False) == 40 and api.line_graph_vertex_count(5, 2, 10, True) == 240
    assert api.line_graph_vertex_count(8, 2, 10, True) == 0                      # unknown channel mode


def test_capacity_refusal():
    L = api.lib()
    st = _style(0.5)
    need = 4 * 2 * 2 * 2                                                         # pairs * graphs * sides * (fill + strip)
    buf = np.zeros(need, api.LINE_GRAPH_DRAW_DTYPE)
    buf["first"] = 777
    model = np.full(4, 9.0, F32)
    for cap in (0, 1, need - 1):
        cnt = C.c_uint32(cap)
        assert L.sgz_line_graph_draws(C.byref(st), 5, 4, 100, api._np_ptr(buf), C.byref(cnt), api._np_ptr(model)) == api.SGZ_EINVAL
        assert cnt.value == need and (buf["first"] == 777).all() and (model == 9.0).all()
    cnt = C.c_uint32(need + 5)
    assert L.sgz_line_graph_draws(C.byref(st), 5, 4, 100, api._np_ptr(buf), C.byref(cnt), api._np_ptr(model)) == api.SGZ_OK
    assert cnt.value == need and model[1] == 2.0
    cnt = C.c_uint32(need)
    assert L.sgz_line_graph_draws(None, 5, 4, 100, api._np_ptr(buf), C.byref(cnt), None) == api.SGZ_EINVAL
    assert L.sgz_line_graph_draws(C.byref(st), 5, 4, 100, api._np_ptr(buf), None, None) == api.SGZ_EINVAL
    for mode, pairs, P in [(8, 4, 100), (5, 0, 100), (5, 4, 0)]:
        cnt = C.c_uint32(need)
        assert L.sgz_line_graph_draws(C.byref(st), mode, pairs, P, api._np_ptr(buf), C.byref(cnt), None) == api.SGZ_EINVAL


def test_line_graph_kernel_in_the_code_object_without_scratch():
    import codeobj_report as cr
    lib = os.path.join(ROOT, "signalizer_amd", "libsgz.so")
    if not (os.path.exists(lib) and os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("library or llvm tools not present")
    rows = [r for r in cr.kernels(lib) if "lineGraphVertexKernel" in r["demangled"]]
    assert len(rows) == 1, [r["demangled"] for r in rows]
    r = rows[0]
    assert not r.get("private_segment_fixed_size", 0) and not r.get("vgpr_spill_count", 0) and not r.get("sgpr_spill_count", 0), r
    assert not r.get("group_segment_fixed_size", 0), r
