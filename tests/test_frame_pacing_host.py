"""renderColourSpectrum's frame pacing without a GPU (sgz_frame_pacing_step): the pop loop of SpectrumRendering.cpp:681-735 transcribed
statement by statement into Python and EXECUTED -- a counter for the frame queue, processedFrames++ behind its short-circuit, localFrameZ1
recomputed behind every pop of the uncapped branch -- against the closed forms the library states in sgz.h.  pop is exact and z_next
bit-equal as doubles.  cpl::Math::round is not in the reference's tree: round(v) = floor(v + 0.5) is the library's rule (sgz.h).
columnsToImageKernel and imageUnrollKernel are checked in the built gfx950 code object: no scratch, no spills."""
import ctypes as C
import itertools
import math
import os
import struct
import sys

import numpy as np
import pytest

from signalizer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _round(v):
    return int(math.floor(v + 0.5))


def loop_ref(frames_per_update, smoothing, queued):
    """:681-735 as written; `queue` is frameQueue's element count, nobody adds to it.  Returns (frames popped, framesPerUpdate)"""
    queue = queued
    popped = 0
    local_frame_z1 = frames_per_update                                                            # :681
    processed_frames = 0                                                                          # :685
    approximate_frames = processed_frames + queue                                                 # :686
    local_frame_z1 = approximate_frames + smoothing * (frames_per_update - approximate_frames)    # :687
    frames_this_time = _round(frames_per_update)                                                  # :688
    should_cap = smoothing != 0.0                                                                 # :691
    while True:
        # :693  while ((!shouldCap || (processedFrames++ < framesThisTime)))
        if should_cap:
            go = processed_frames < frames_this_time
            processed_frames += 1
        else:
            go = True                                                                             # (the ++ is never evaluated)
        if not go:
            break
        if queue == 0:                                                                            # :696-697 popElement fails
            break
        queue -= 1
        popped += 1                                                                               # :721 updateSingleColumn
        if not should_cap:                                                                        # :727-732
            approximate_frames = processed_frames + queue
            local_frame_z1 = approximate_frames + smoothing * (frames_per_update - approximate_frames)
            frames_this_time = _round(local_frame_z1)
    return popped, float(local_frame_z1)                                                          # :735


def bits(v):
    return struct.pack("<d", v)


Z = [0, 0.49, 0.5, 1.5, 9.5, 10, 37.25]
SMOOTHING = [0, 1e-9, 0.5, 0.9, 0.996]


def test_grid_equals_the_executed_loop():
    for z, s, q in itertools.product(Z, SMOOTHING, range(11)):
        got = api.frame_pacing_step(float(z), float(s), q)
        want = loop_ref(float(z), float(s), q)
        assert got[0] == want[0] and bits(got[1]) == bits(want[1]), (z, s, q, got, want)


def test_random_triples_equal_the_executed_loop():
    rng = np.random.default_rng(20240611)
    for _ in range(2000):
        z = float(rng.choice([rng.uniform(0, 12), rng.uniform(0, 1), rng.uniform(0, 300), float(rng.integers(0, 12)) + 0.5]))
        s = float(rng.choice([0.0, rng.uniform(0, 0.996), rng.uniform(0, 1e-6), np.nextafter(1.0, 0.0)]))
        q = int(rng.integers(0, 11))
        got = api.frame_pacing_step(z, s, q)
        want = loop_ref(z, s, q)
        assert got[0] == want[0] and bits(got[1]) == bits(want[1]), (z, s, q, got, want)


def test_closed_forms_of_the_header():
    """the two branches as sgz.h states them"""
    for z, s, q in itertools.product(Z, SMOOTHING, range(11)):
        pop, zn = api.frame_pacing_step(float(z), float(s), q)
        if s != 0:
            assert pop == min(q, _round(z)) and bits(zn) == bits(q + s * (z - q))
        else:
            assert pop == q and bits(zn) == bits(0.0)


def test_closed_loop_follows_the_executed_loop():
    """300 video frames, one column arriving per frame, smoothing 0.9: the library's chain and the executed loop's stay equal, queue
    (capped at frameQueue's 10) included"""
    zl = zr = 0.0
    ql = qr = 0
    total = 0
    for step in range(300):
        ql, qr = min(ql + 1, 10), min(qr + 1, 10)
        pop, zl = api.frame_pacing_step(zl, 0.9, ql)
        want, zr = loop_ref(zr, 0.9, qr)
        assert pop == want and bits(zl) == bits(zr), (step, pop, want, zl, zr)
        ql -= pop
        qr -= want
        total += pop
    assert 0 < total <= 300


def test_first_frame_takes_nothing_when_capped():
    assert api.frame_pacing_step(0.0, 0.5, 7) == (0, 3.5)
    assert api.frame_pacing_step(0.0, 0.0, 7) == (7, 0.0)


def test_huge_frames_per_update_pops_what_is_there():
    assert api.frame_pacing_step(1e300, 0.5, 9)[0] == 9


def test_refusals():
    L = api.lib()
    pop, zn = C.c_uint32(77), C.c_double(5.5)
    nan, inf = float("nan"), float("inf")
    for z, s in ((nan, 0.5), (inf, 0.5), (-1.0, 0.5), (-1e-300, 0.0), (1.0, nan), (1.0, -0.1), (1.0, 1.0), (1.0, 1.5), (1.0, inf), (1.0, -inf)):
        assert L.sgz_frame_pacing_step(z, s, 3, C.byref(pop), C.byref(zn)) == api.SGZ_EINVAL, (z, s)
        assert pop.value == 77 and zn.value == 5.5
    assert L.sgz_frame_pacing_step(1.0, 0.5, 3, None, C.byref(zn)) == api.SGZ_EINVAL
    assert L.sgz_frame_pacing_step(1.0, 0.5, 3, C.byref(pop), None) == api.SGZ_EINVAL
    assert L.sgz_frame_pacing_step(1.0, float(np.nextafter(1.0, 0.0)), 3, C.byref(pop), C.byref(zn)) == api.SGZ_OK


def test_null_arguments_are_refused_without_a_gpu():
    """the stage and handle calls check their pointers before they touch the device"""
    L = api.lib()
    one = C.c_void_p(4096)
    assert L.sgz_columns_to_image_device(None, 1, 4, one, 4, 16, 0, None) == api.SGZ_EINVAL
    assert L.sgz_columns_to_image_device(one, 1, 4, None, 4, 16, 0, None) == api.SGZ_EINVAL
    for args in ((0, 4, 4, 16, 0), (5, 4, 4, 16, 0), (1, 0, 4, 16, 0), (1, 4, 0, 16, 0), (1, 4, 4, 12, 0), (1, 4, 4, 18, 0), (1, 4, 4, 16, 4)):
        n, P, cols, pitch, x0 = args
        assert L.sgz_columns_to_image_device(one, n, P, C.c_void_p(8192), cols, pitch, x0, None) == api.SGZ_EINVAL, args
    assert L.sgz_image_unroll_device(None, 4, 16, 4, 0, one, 16, None) == api.SGZ_EINVAL
    assert L.sgz_image_unroll_device(one, 4, 16, 4, 0, None, 16, None) == api.SGZ_EINVAL
    assert L.sgz_image_unroll_device(one, 4, 16, 4, 4, C.c_void_p(8192), 16, None) == api.SGZ_EINVAL          # x >= columns
    assert L.sgz_image_unroll_device(one, 4, 16, 4, 0, C.c_void_p(4096 + 32), 16, None) == api.SGZ_EINVAL     # overlap
    assert L.sgz_spectrum_set_pacing(None, 0.5) == api.SGZ_EINVAL
    assert L.sgz_spectrum_set_frozen(None, 1) == api.SGZ_EINVAL
    assert L.sgz_spectrum_render_columns(None, None, None, None) == api.SGZ_EINVAL
    assert L.sgz_spectrum_present(None, one, 16) == api.SGZ_EINVAL


def test_exports():
    L = api.lib()
    names = ["sgz_spectrum_set_pacing", "sgz_spectrum_set_frozen", "sgz_spectrum_render_columns", "sgz_spectrum_present",
             "sgz_frame_pacing_step", "sgz_columns_to_image_device", "sgz_image_unroll_device"]
    for name in names:
        assert name in api.EXPORTS and hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "sgz.h")).read()
    for name in names:
        assert f"{name}(" in hdr, name


@pytest.mark.parametrize("kernel,lds", [("columnsToImageKernel", 32 * 65 * 4), ("imageUnrollKernel", 0)])
def test_kernels_in_the_code_object_without_scratch(kernel, lds):
    import codeobj_report as cr
    lib = os.path.join(ROOT, "signalizer_amd", "libsgz.so")
    assert os.path.exists(lib), "libsgz.so is not built"
    assert os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy"), "llvm tools not present"
    rows = [r for r in cr.kernels(lib) if kernel in r["demangled"]]
    assert len(rows) == 1, [r["demangled"] for r in rows]
    r = rows[0]
    assert not r.get("private_segment_fixed_size", 0) and not r.get("vgpr_spill_count", 0) and not r.get("sgpr_spill_count", 0), r
    assert r.get("group_segment_fixed_size", 0) == lds, r     # the padded transpose tile and nothing else
