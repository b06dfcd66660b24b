"""The waveform lane (sgz.h, "The waveform lane"): what needs no GPU -- the exports, the header, tests/wave_ref.py against a brute-force loop,
the fold of finer columns into coarser ones, and the new kernels' code objects."""
import math
import os
import re
import struct
import sys

import numpy as np
import pytest

from signalizer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wave_ref as wr  # noqa: E402

NAMES = ["sgz_stage_wave_columns", "sgz_wave_columns_limits", "sgz_pcm_stream_set_waveform", "sgz_pcm_stream_waveform_for",
         "sgz_pcm_stream_waveform_state", "sgz_pcm_stream_flush_waveform"]


def test_exports_exist():
    L = api.lib()
    assert [n for n in NAMES if not hasattr(L, n)] == []
    assert [n for n in NAMES if n not in api.EXPORTS] == []
    assert L.sgz_abi_version() == 5


def test_header_names_them_and_keeps_version_5():
    text = open(os.path.join(ROOT, "include", "sgz.h")).read()
    assert re.search(r"#define\s+SGZ_ABI_VERSION\s+5\b", text)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n                    # declared
    history = text[:text.index("#define SGZ_ABI_VERSION")]
    assert [n for n in NAMES if n not in history] == []                # and listed under the version-5 entry
    assert "The waveform lane" in text and "has no counterpart" in text[text.index("The waveform lane"):][:600]


def test_limits_are_the_documented_ones():
    switch, tile = api.wave_columns_limits()
    assert 1 <= switch <= tile and tile % 4 == 0, (switch, tile)
    text = open(os.path.join(ROOT, "include", "sgz.h")).read()
    lane = text[text.index("/* The waveform lane"):]
    assert f"({switch};" in lane and f"{tile} / m" in lane


def _less(a, b):
    """a before b in the total order (neither a NaN): IEEE <, and -0 before +0"""
    return a < b or (a == b and math.copysign(1.0, a) < math.copysign(1.0, b))


def _brute(x, m, flush):
    """the definition, sample by sample, on Python floats and struct-packed bits"""
    channels, S = x.shape
    columns = S // m + (1 if flush and S % m else 0)
    out = np.zeros((columns, channels, 2), np.uint32)
    for c in range(columns):
        for d in range(channels):
            lo = hi = None
            for i in range(c * m, min((c + 1) * m, S)):
                v = float(x[d, i])
                if v != v:
                    continue
                if lo is None or _less(v, lo):
                    lo = v
                if hi is None or _less(hi, v):
                    hi = v
            for j, v in enumerate((lo, hi)):
                out[c, d, j] = 0x7FC00000 if v is None else struct.unpack("<I", struct.pack("<f", v))[0]
    return out


def test_wave_ref_against_a_brute_force_loop():
    rng = np.random.default_rng(11)
    cases = 0
    for trial in range(300):
        S = int(rng.integers(0, 65))
        m = int(rng.choice([1, 2, 3, 7, int(rng.integers(1, 70))]))
        channels = int(rng.integers(1, 4))
        x = wr.content(["random", "constant", "ramp"][trial % 3], channels, S, m, seed=trial)
        if S:                                                           # more specials than content() sprinkles: a third of the samples
            b = x.view(np.uint32)
            pick = rng.random(x.shape) < 0.33
            b[pick] = wr.SPECIALS[rng.integers(0, len(wr.SPECIALS), size=int(pick.sum()))]
        for flush in (True, False):
            got, left = wr.columns_of(x, m, flush)
            assert left == (0 if flush else S % m)
            assert np.array_equal(got, _brute(x, m, flush)), (trial, S, m, channels, flush)
            cases += 1
    assert cases == 600
    # the corners by hand: -0 < +0, a denormal beside zero, NaNs take no part, a column of NaNs alone
    x = np.array([[0x00000000, 0x80000000, 0x7FC00000, 0x80000001, 0xFFC00000, 0x7F800001, 0x7F800000, 0xFF800000]], np.uint32).view(np.float32)
    got, _ = wr.columns_of(x, 2)
    assert got[:, 0].tolist() == [[0x80000000, 0x00000000], [0x80000001, 0x80000001], [0x7FC00000, 0x7FC00000], [0xFF800000, 0x7F800000]]


def test_a_coarser_column_is_the_fold_of_the_finer_ones():
    rng = np.random.default_rng(5)
    for trial in range(40):
        S = int(rng.integers(1, 400))
        m = int(rng.integers(1, 9))
        r = int(rng.integers(2, 6))                                     # the coarser column: r finer ones
        x = wr.content("random", 2, S, m, seed=100 + trial)
        fine, _ = wr.columns_of(x, m)
        coarse, _ = wr.columns_of(x, m * r)
        n = fine.shape[0]
        bounds = list(range(0, n, r)) + [n]
        assert np.array_equal(wr.fold(fine, bounds), coarse), (trial, S, m, r)
        # nested: a fold of a fold is the direct fold
        twice, _ = wr.columns_of(x, m * r * 2)
        n2 = coarse.shape[0]
        assert np.array_equal(wr.fold(coarse, list(range(0, n2, 2)) + [n2]), twice), (trial, S, m, r)


def test_wave_kernels_need_no_scratch():
    import codeobj_report as cr
    lib = os.path.join(ROOT, "signalizer_amd", "libsgz.so")
    if not (os.path.exists(lib) and os.path.exists(f"{cr.LLVM}/llvm-readelf") and os.path.exists(f"{cr.LLVM}/llvm-objcopy")):
        pytest.skip("library or llvm tools not present")
    rows = [r for r in cr.kernels(lib) if any(k in r["demangled"] for k in ("waveTileKernel", "waveSliceKernel", "waveEmitKernel"))]
    assert len(rows) == 3, [r["demangled"] for r in rows]
    bad = [(r["demangled"], r.get("vgpr_spill_count"), r.get("sgpr_spill_count"), r.get("private_segment_fixed_size")) for r in rows
           if r.get("vgpr_spill_count", 0) or r.get("sgpr_spill_count", 0) or r.get("private_segment_fixed_size", 0)]
    assert not bad, bad
