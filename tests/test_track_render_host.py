"""The batched frequency tracker (sgz_stage_track_peaks, sgz_stage_track_peaks_lines, sgz_spectrogram_track_device / _host; csrc/tracker.hip)
without a GPU: the exports, the refusals every call makes before it touches the device, the two kernels in the built gfx950 code object
(no scratch, no spill), and the kernels' scheme -- a strided (value, lowest index) reduction, then the boundary walk as the first hit among
256 neighbour pairs per step -- emulated in Python against the host function it restates."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("sgz_stage_track_peaks", "sgz_stage_track_peaks_lines", "sgz_spectrogram_track_device", "sgz_spectrogram_track_host")
NON_FINITE = (math.nan, math.inf, -math.inf)


@pytest.fixture(scope="module")
def plan():
    return api.Plan(config.spectrum_config(window_size=64, hop=16, axis_points=33))        # host tables only: never uploaded here


@pytest.fixture(scope="module")
def buf():
    """a host block that stands for any non-NULL buffer: every call here is refused before a buffer is looked at"""
    b = np.zeros(4096, np.float32)
    return b, b.ctypes.data_as(C.c_void_p)


def test_exports_exist():
    L = api.lib()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(L, name), name
    for name in ("track_peaks", "track_peaks_lines", "track_render"):
        assert callable(getattr(api.Plan, name))
    with open(os.path.join(ROOT, "include", "sgz.h")) as f:
        header = f.read()
    assert all(name + "(" in header for name in NAMES) and "#define SGZ_ABI_VERSION 5" in header


def test_null_arguments_are_refused(plan, buf):
    L = api.lib()
    _, p = buf
    ch = (C.c_void_p * 2)(p, p)
    E = api.SGZ_EINVAL
    assert L.sgz_stage_track_peaks(None, p, 1, 0.5, p, None) == E
    assert L.sgz_stage_track_peaks(plan.h, None, 1, 0.5, p, None) == E
    assert L.sgz_stage_track_peaks(plan.h, p, 1, 0.5, None, None) == E
    assert L.sgz_stage_track_peaks_lines(None, p, 1, 0, 0.5, p, None) == E
    assert L.sgz_stage_track_peaks_lines(plan.h, None, 1, 0, 0.5, p, None) == E
    assert L.sgz_stage_track_peaks_lines(plan.h, p, 1, 0, 0.5, None, None) == E
    assert L.sgz_spectrogram_track_device(None, p, 1024, 1024, 0, 0.5, p, None, p, None) == E
    assert L.sgz_spectrogram_track_device(plan.h, None, 1024, 1024, 0, 0.5, p, None, p, None) == E
    assert L.sgz_spectrogram_track_device(plan.h, p, 1024, 1024, 0, 0.5, p, None, None, None) == E
    assert L.sgz_spectrogram_track_host(None, ch, 2, 1024, 0, 0.5, p, p, None) == E
    assert L.sgz_spectrogram_track_host(plan.h, None, 2, 1024, 0, 0.5, p, p, None) == E
    assert L.sgz_spectrogram_track_host(plan.h, ch, 2, 1024, 0, 0.5, p, None, None) == E
    assert L.sgz_spectrogram_track_host(plan.h, (C.c_void_p * 2)(p, None), 2, 1024, 0, 0.5, p, p, None) == E
    assert L.sgz_spectrogram_track_host(plan.h, ch, 3, 1024, 0, 0.5, p, p, None) == E          # 2 * num_pairs channels, as the render


def test_graph_out_of_range_is_refused(plan, buf):
    L = api.lib()
    _, p = buf
    ch = (C.c_void_p * 2)(p, p)
    for graph in (api.NUM_GRAPHS, api.NUM_GRAPHS + 1, 0xffffffff):
        assert L.sgz_stage_track_peaks_lines(plan.h, p, 1, graph, 0.5, p, None) == api.SGZ_EINVAL
        assert L.sgz_spectrogram_track_device(plan.h, p, 1024, 1024, graph, 0.5, p, None, p, None) == api.SGZ_EINVAL
        assert L.sgz_spectrogram_track_host(plan.h, ch, 2, 1024, graph, 0.5, p, p, None) == api.SGZ_EINVAL


def test_non_finite_mouse_fraction_is_refused(plan, buf):
    L = api.lib()
    b, p = buf
    ch = (C.c_void_p * 2)(p, p)
    for mf in NON_FINITE:
        assert L.sgz_stage_track_peaks(plan.h, p, 1, mf, p, None) == api.SGZ_EINVAL
        assert L.sgz_stage_track_peaks_lines(plan.h, p, 1, 0, mf, p, None) == api.SGZ_EINVAL
        assert L.sgz_spectrogram_track_device(plan.h, p, 1024, 1024, 0, mf, p, None, p, None) == api.SGZ_EINVAL
        assert L.sgz_spectrogram_track_host(plan.h, ch, 2, 1024, 0, mf, p, p, None) == api.SGZ_EINVAL
    assert not b.any()


@pytest.mark.parametrize("mode", [config.CH_PHASE, config.CH_COMPLEX])
def test_raw_bin_branch_refuses_phase_and_complex(mode, buf):
    """sgz_stage_track_peak's refusals, in its order: the mode before the mouse position"""
    _, p = buf
    pl = api.Plan(config.spectrum_config(window_size=64, hop=16, axis_points=33, channel_mode=mode))
    L = api.lib()
    assert L.sgz_stage_track_peaks(pl.h, p, 1, 0.5, p, None) == api.SGZ_EUNSUPPORTED
    assert L.sgz_stage_track_peaks(pl.h, p, 0, math.nan, p, None) == api.SGZ_EUNSUPPORTED


def test_tracker_kernels_in_the_code_object_without_scratch():
    import codeobj_report as cr
    lib = api.LIB_PATH
    api.lib()
    if not (os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("llvm tools not present")
    rows = cr.kernels(lib)
    for kernel in ("trackPeaksKernel", "trackLinePeaksKernel", "trackPeakKernel"):
        mine = [r for r in rows if kernel + "(" in r["demangled"]]
        assert len(mine) == 1, [r["demangled"] for r in mine]
        for r in mine:
            assert not r.get("private_segment_fixed_size", 0) and not r.get("vgpr_spill_count", 0) and not r.get("sgpr_spill_count", 0), r


# ---- the kernels' scheme against the host function ------------------------------------------------------------------------------------
def _llround(x):
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def _first_hit(start, count, step, hit):
    """walkFirstHit (tracker.hip): 4 ballots of 64 candidates per step, the first set bit of the first non-empty ballot"""
    for c0 in range(0, count, 256):
        for j in range(4):
            m = [c0 + j * 64 + lane < count and hit(start + step * (c0 + j * 64 + lane)) for lane in range(64)]
            if any(m):
                return start + step * (c0 + j * 64 + m.index(True))
    return start + step * (count - 1) if count > 0 else start


def _emulated_line_peak(v, mf):
    """trackLinePeaksKernel's peak index: 256 threads stride through the range from left(start), butterfly and cross-wave combines under
    the host loop's own comparison, then the cooperative walk"""
    N = len(v)
    mf = min(max(mf, 0.0), 1.0)
    pivot, rg = _llround(N * mf), _llround(N * 0.03)
    lb, hb = (0 if rg > pivot else pivot - rg), (N if rg + pivot > N else rg + pivot)
    start = lb if lb < N else N - 1
    best, arg = [v[start]] * 256, [start] * 256
    for t in range(256):
        for i in range(lb + 1 + t, hb, 256):
            if best[t] < v[i]:
                best[t], arg[t] = v[i], i
    o = 32
    while o:
        nb, na = best[:], arg[:]
        for a in range(256):
            b = (a & ~63) | ((a & 63) ^ o)
            if best[a] < best[b] or (best[b] == best[a] and arg[b] < arg[a]):
                nb[a], na[a] = best[b], arg[b]
        best, arg, o = nb, na, o >> 1
    b, peak = best[0], arg[0]
    for w in (64, 128, 192):
        if b < best[w] or (best[w] == b and arg[w] < peak):
            b, peak = best[w], arg[w]
    if peak == lb and lb != 0:
        peak = _first_hit(peak, peak, -1, lambda k: k - 1 == 0 or v[k - 1] < v[k])
    elif hb != 0 and peak == hb - 1:
        peak = _first_hit(peak, N - peak, 1, lambda k: k + 1 == N or v[k + 1] < v[k])
    return peak


@pytest.mark.parametrize("P", [2, 16, 17, 33, 64, 1000])
def test_reduction_and_cooperative_walk_equal_the_host_loop(P):
    """peak_offset of sgz_track_peak_lines (the sequential loop and walks) == the kernels' scheme, on the contents that separate them:
    ties, ramps whose walk runs the whole axis, NaN at the start of the range / scattered / everywhere, +-inf"""
    plan = api.Plan(config.spectrum_config(window_size=64, hop=16, axis_points=P))
    rng = np.random.default_rng(P)
    lines = [rng.standard_normal(P), np.arange(P) * 1.0, -np.arange(P) * 1.0, np.zeros(P), np.full(P, np.nan), np.round(rng.random(P) * 3)]
    v = np.arange(P) * 1.0; v[::5] = np.nan; lines.append(v)
    v = -np.arange(P) * 1.0; v[1::3] = np.nan; lines.append(v)
    v = rng.standard_normal(P); v[rng.integers(0, P, P // 3 + 1)] = np.nan; lines.append(v)
    v = rng.standard_normal(P); v[P // 2] = np.inf; v[: P // 4] = -np.inf; lines.append(v)
    for v in lines:
        v = v.astype(np.float32)
        rec = np.stack([v, np.zeros(P, np.float32)], axis=1)
        for mf in (-1.0, 0.0, 0.02, 0.03, 0.31, 0.5, 0.97, 1.0, 2.0):
            assert plan.track_peak_lines(rec, mf)["peak_offset"] == _emulated_line_peak(list(v), mf), (P, mf)
