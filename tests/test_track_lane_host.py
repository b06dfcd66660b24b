"""The track lane without a GPU (sgz_track_peak_values, sgz_stage_track_peaks_values, sgz_pcm_stream_set_track / _track_for / _track_state;
csrc/tracker.hip, csrc/pcm.hip): the exports, the host form against its definition -- sgz_track_peak_lines on the interleaved copy, byte
for byte, whatever the second components hold -- every refusal that needs no device, and the three line-result kernels in the built gfx950
code object (no scratch, no spill)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_track_render import MOUSE, _line_pool  # noqa: E402  (the eight mouse positions, the twenty contents)

NAMES = ("sgz_track_peak_values", "sgz_stage_track_peaks_values", "sgz_pcm_stream_set_track", "sgz_pcm_stream_track_for",
         "sgz_pcm_stream_track_state")
NON_FINITE = (math.nan, math.inf, -math.inf)
E = api.SGZ_EINVAL
# the deviance floor applies (FFT, no Lanczos), does not (FFT with Lanczos), does not (RSNT)
PLANS = {
    "fft_linear": dict(bin_interp=config.INTERP_LINEAR),
    "fft_lanczos": dict(bin_interp=config.INTERP_LANCZOS),
    "rsnt": dict(algorithm=config.ALGO_RSNT),
}


def _lib():
    """the library with the lane's symbols looked up: a missing one fails here, by name"""
    L = api.lib()
    for name in NAMES:
        assert hasattr(L, name), f"libsgz.so does not export {name}"
    return L


def test_exports_exist():
    L = _lib()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(L, name), name
    for name in ("track_peak_values", "track_peaks_values"):
        assert callable(getattr(api.Plan, name))
    for name in ("set_track", "track_for", "track_state"):
        assert callable(getattr(api.PcmStream, name))
    with open(os.path.join(ROOT, "include", "sgz.h")) as f:
        header = f.read()
    assert all(name + "(" in header for name in NAMES) and "#define SGZ_ABI_VERSION 5" in header
    assert "(5, later: the track lane" in header


def _bits(peak):
    return np.frombuffer(bytes(peak), np.uint64).copy()


@pytest.mark.parametrize("kind", list(PLANS))
@pytest.mark.parametrize("P", [2, 16, 17, 33, 64, 1000, 4096])
def test_values_form_equals_the_lines_form_on_the_interleaved_copy(P, kind):
    L = _lib()
    # (host tables only; 4096 bins: at 1000 axis points and more the floor of half a bin binds at the bottom of the log axis and not at its top)
    plan = api.Plan(config.spectrum_config(window_size=4096, hop=1024, axis_points=P, **PLANS[kind]))
    pool = _line_pool(P, 100 + P)
    assert len(pool) == 20 and len(MOUSE) == 8
    rng = np.random.default_rng(P)
    floored = total = 0
    for k, values in enumerate(pool):
        values = np.ascontiguousarray(values, np.float32)
        seconds = (np.full(P, np.nan, np.float32), rng.standard_normal(P).astype(np.float32))
        for mf in MOUSE:
            got = api.LinePeak()
            assert L.sgz_track_peak_values(plan.h, values.ctypes.data_as(C.c_void_p), mf, C.byref(got)) == api.SGZ_OK
            for second in seconds:
                rec = np.ascontiguousarray(np.stack([values, second], axis=1))
                want = api.LinePeak()
                assert L.sgz_track_peak_lines(plan.h, rec.ctypes.data_as(C.c_void_p), mf, C.byref(want)) == api.SGZ_OK
                assert (_bits(got) == _bits(want)).all(), (P, kind, k, mf, got.asdict(), want.asdict())
            floored += got.peak_deviance == 0.5 * plan.N / P
            total += 1
    if kind == "fft_linear" and P >= 1000:
        assert 0 < floored < total, (floored, total)                         # the floor went both ways
    # the wrapper
    assert plan.track_peak_values(pool[0], 0.5) == plan.track_peak_lines(np.stack([pool[0], np.zeros(P, np.float32)], axis=1), 0.5)


def test_refusals_that_need_no_device():
    L = _lib()
    plan = api.Plan(config.spectrum_config(window_size=64, hop=16, axis_points=33))
    b = np.zeros(4096, np.float32)
    p = b.ctypes.data_as(C.c_void_p)
    out = api.LinePeak()
    assert L.sgz_track_peak_values(None, p, 0.5, C.byref(out)) == E
    assert L.sgz_track_peak_values(plan.h, None, 0.5, C.byref(out)) == E
    assert L.sgz_track_peak_values(plan.h, p, 0.5, None) == E
    assert L.sgz_stage_track_peaks_values(None, p, 1, 0.5, p, None) == E
    assert L.sgz_stage_track_peaks_values(plan.h, None, 1, 0.5, p, None) == E
    assert L.sgz_stage_track_peaks_values(plan.h, p, 1, 0.5, None, None) == E
    for mf in NON_FINITE:
        assert L.sgz_track_peak_values(plan.h, p, mf, C.byref(out)) == E
        assert L.sgz_stage_track_peaks_values(plan.h, p, 1, mf, p, None) == E
        assert L.sgz_stage_track_peaks_values(plan.h, p, 0, mf, p, None) == E                 # (before records == 0 is looked at)
    assert bytes(out) == bytes(api.LinePeak()) and not b.any()
    # the stream calls on no stream
    n = C.c_uint64(77)
    assert L.sgz_pcm_stream_set_track(None, 0, 0.5, p, 8) == E
    assert L.sgz_pcm_stream_set_track(None, 0, 0.5, None, 0) == E
    assert L.sgz_pcm_stream_track_state(None, C.byref(n)) == E and n.value == 77
    assert L.sgz_pcm_stream_track_state(None, None) == E
    assert L.sgz_pcm_stream_track_for(None, 1 << 20) == 0 and L.sgz_pcm_stream_track_for(None, 0) == 0


def test_line_result_kernels_in_the_code_object_without_scratch():
    """the check of tests/test_track_render_host.py, with the value-plane kernel beside the older two"""
    import codeobj_report as cr
    _lib()
    if not (os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("llvm tools not present")
    rows = cr.kernels(api.LIB_PATH)
    for kernel in ("trackValuePeaksKernel", "trackLinePeaksKernel", "trackPeaksKernel"):
        mine = [r for r in rows if kernel + "(" in r["demangled"]]
        assert len(mine) == 1, (kernel, [r["demangled"] for r in mine])
        for r in mine:
            assert not r.get("private_segment_fixed_size", 0) and not r.get("vgpr_spill_count", 0) and not r.get("sgpr_spill_count", 0), r
