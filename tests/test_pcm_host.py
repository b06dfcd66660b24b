"""Interleaved PCM in (sgz.h "interleaved PCM in"): what needs no GPU -- the exports, the sample sizes, sgz_pcm_timing's layout, the
streamed render's frame arithmetic (sgz_stream_step) against a brute-force count, and the converter kernels' code objects."""
import ctypes as C
import os
import subprocess
import shutil
import sys

import numpy as np
import pytest

from signalizer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ["sgz_pcm_sample_bytes", "sgz_pcm_to_planar_device", "sgz_stream_step", "sgz_pcm_stream_create", "sgz_pcm_stream_destroy",
         "sgz_pcm_stream_frames_for", "sgz_pcm_stream_feed", "sgz_pcm_stream_reset", "sgz_spectrogram_render_pcm"]


def test_exports_exist():
    L = api.lib()
    assert [n for n in NAMES if not hasattr(L, n)] == []
    assert [n for n in NAMES if n not in api.EXPORTS] == []


def test_sample_bytes_of_every_format():
    L = api.lib()
    assert (api.PCM_F32, api.PCM_U8, api.PCM_S16, api.PCM_S24, api.PCM_S32, api.PCM_F64, api.PCM_END) == (0, 1, 2, 3, 4, 5, 6)
    assert [L.sgz_pcm_sample_bytes(f) for f in range(api.PCM_END)] == [4, 1, 2, 3, 4, 8]
    assert L.sgz_pcm_sample_bytes(api.PCM_END) == 0 and L.sgz_pcm_sample_bytes(1000) == 0
    assert api.PCM_SAMPLE_BYTES == {f: L.sgz_pcm_sample_bytes(f) for f in range(api.PCM_END)}


def test_timing_struct_layout(tmp_path):
    names = ["wall_ms", "h2d_ms", "convert_ms", "render_ms", "d2h_ms", "frames", "chunks"]
    assert [n for n, _ in api.PcmTiming._fields_] == names
    assert C.sizeof(api.PcmTiming) == 56 and [getattr(api.PcmTiming, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 48]
    if not shutil.which("gcc"):
        return
    # ... and against the compiler's own view of include/sgz.h
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sgz.h"\nint main(void) { printf("%zu", sizeof(sgz_pcm_timing)); '
                   + " ".join(f'printf(" %zu", offsetof(sgz_pcm_timing, {n}));' for n in names) + " return 0; }\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [56, 0, 8, 16, 24, 32, 40, 48]


def _brute_frames(total, W, hop, f=0):
    """frames with [f*hop, f*hop + W) inside [0, total), counted one by one (from f, which are known to be inside)"""
    while f * hop + W <= total:
        f += 1
    return f


def test_stream_step_against_brute_force():
    L = api.lib()
    rng = np.random.default_rng(7)
    for _ in range(2000):
        W = int(rng.integers(1, 300))
        hop = int(rng.integers(1, W + 1))
        held = total = made = brute = 0
        for _ in range(int(rng.integers(1, 12))):
            n = int(rng.choice([0, 1, int(rng.integers(0, hop + 1)), int(rng.integers(0, 3 * W + 1))]))
            frames, keep = api.stream_step(W, hop, held, n)
            total += n
            made += frames
            brute = _brute_frames(total, W, hop, brute)
            assert made == brute, (W, hop, total, made, brute)
            assert keep == held + n - frames * hop and keep < W, (W, hop, held, n, frames, keep)
            if held + n >= W:
                assert frames >= 1 and keep >= W - hop, (W, hop, held, n, frames, keep)
            held = keep
        assert made == max(0, L.sgz_num_frames(total, W, hop))


def test_stream_step_refusals():
    L = api.lib()
    f, k = C.c_uint64(5), C.c_uint64(5)
    assert L.sgz_stream_step(0, 1, 0, 10, C.byref(f), C.byref(k)) == api.SGZ_EINVAL
    assert L.sgz_stream_step(16, 0, 0, 10, C.byref(f), C.byref(k)) == api.SGZ_EINVAL
    assert L.sgz_stream_step(16, 17, 0, 40, C.byref(f), C.byref(k)) == api.SGZ_EINVAL       # samples between frames: not this arithmetic
    assert L.sgz_stream_step(16, 4, 0, 10, None, C.byref(k)) == api.SGZ_EINVAL
    assert (f.value, k.value) == (5, 5)
    assert L.sgz_stream_step(16, 16, 3, 13, C.byref(f), C.byref(k)) == api.SGZ_OK and (f.value, k.value) == (1, 0)
    assert api.stream_step(32768, 8192, 0, 2880000) == (348, 2880000 - 348 * 8192)


def test_converter_kernels_need_no_scratch():
    import codeobj_report as cr
    lib = os.path.join(ROOT, "signalizer_amd", "libsgz.so")
    if not (os.path.exists(lib) and os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("library or llvm tools not present")
    rows = [r for r in cr.kernels(lib) if "pcmToPlanarKernel" in r["demangled"]]
    assert len(rows) == 6, [r["demangled"] for r in rows]                      # one per format
    bad = [(r["demangled"], r.get("vgpr_spill_count"), r.get("sgpr_spill_count"), r.get("private_segment_fixed_size")) for r in rows
           if r.get("vgpr_spill_count", 0) or r.get("sgpr_spill_count", 0) or r.get("private_segment_fixed_size", 0)]
    assert not bad, bad
