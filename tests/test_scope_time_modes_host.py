"""The Oscilloscope's time modes on the host (no GPU): sgz_scope_time_window against a restatement of handleFlagUpdates' window
step (Oscilloscope.cpp:293-307), the new entry points' exports, and the grown sgz_scope_config's layout."""
import ctypes as C
import itertools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from signalizer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_window(mode, value, sample_rate, bpm, cycle_samples):
    """Oscilloscope.cpp:293-307, expression for expression (Python floats are IEEE doubles)"""
    if mode == api.TIME_BEATS:
        w = sample_rate * (60 / (max(10.0, bpm) * value))
        return max(w, 128.0)
    if mode == api.TIME_CYCLES:
        return value * cycle_samples + 1
    return value


SRS = (44100.0, 48000.0, 96000.0, 192000.0, 22050.5)
VALUES = (0.25, 0.5, 1.0, 1.5, 3.0, 4.0, 7.3, 16.0, 128.0, 1000.0, 19200.0)
BPMS = (0.0, -5.0, 9.99, 10.0, 60.0, 97.3, 120.0, 174.25, 300.0, 999.0)
CYCLES = (0.0, 1.0, 44.1, 108.843537414966, 9600.0, 38400.0)


def test_time_window_matches_the_reference_formula():
    got_floor_128 = got_floor_10 = 0
    for mode, sr, value, bpm, cs in itertools.product((0, 1, 2), SRS, VALUES, BPMS, CYCLES):
        got = api.time_window(mode, value, sr, bpm, cs)
        want = _reference_window(mode, value, sr, bpm, cs)
        assert got == want, (mode, sr, value, bpm, cs, got, want)
        if mode == api.TIME_BEATS:
            got_floor_128 += got == 128.0
            got_floor_10 += bpm < 10 and got > 128.0
    assert got_floor_128 > 0 and got_floor_10 > 0                      # both floors are on the grid


def test_time_window_edge_values():
    # the reference's `double bpm {}`: no tempo yet is the 10 BPM floor
    assert api.time_window(api.TIME_BEATS, 4.0, 48000.0, 0.0) == 48000.0 * (60 / (10.0 * 4.0)) == 72000.0
    assert api.time_window(api.TIME_BEATS, 1.0, 48000.0, 120.0) == 24000.0
    assert api.time_window(api.TIME_BEATS, 64.0, 44100.0, 400.0) == 128.0     # 103.36 samples -> the 128 floor
    # a NaN tempo: std::max(10.0, NaN) is 10.0, as Python's max
    assert api.time_window(api.TIME_BEATS, 2.0, 48000.0, float("nan")) == api.time_window(api.TIME_BEATS, 2.0, 48000.0, 10.0)
    # Cycles before the first analysed frame (cycleSamples 0): one sample
    assert api.time_window(api.TIME_CYCLES, 3.0, 48000.0, 0.0, 0.0) == 1.0
    assert api.time_window(api.TIME_TIME, 1234.5, 48000.0, 120.0, 99.0) == 1234.5
    # Cycles is the same fp64 product the device computes (no contraction into an fma)
    v, cs = 2.7, 48000.0 / 441.3
    assert api.time_window(api.TIME_CYCLES, v, 48000.0, 0.0, cs) == float(np.float64(v) * np.float64(cs) + 1)


def test_new_symbols_are_exported_and_declared():
    L = api.lib()
    hdr = open(os.path.join(ROOT, "include", "sgz.h")).read()
    for sym in ("sgz_scope_set_tempo", "sgz_scope_effective_window", "sgz_scope_time_window"):
        assert hasattr(L, sym) and sym in api.EXPORTS
        assert f"{sym}(" in hdr
    assert "SGZ_TIME_CYCLES" in hdr and "time_mode" in hdr
    assert L.sgz_scope_effective_window(None) == 0.0
    assert L.sgz_scope_set_tempo(None, 120.0) == api.SGZ_EINVAL


def test_scope_config_layout_matches_header():
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.fail("no C compiler to read the header's layout with")
    fields = [name for name, _ in api.ScopeConfig._fields_]
    assert fields[-1] == "time_mode"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "layout.c")
        body = " ".join(f'printf("%zu ", offsetof(sgz_scope_config, {f}));' for f in fields)
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "sgz.h"\nint main(void) { '
                             f'{body} printf("%zu %d %d %d", sizeof(sgz_scope_config), SGZ_TIME_TIME, SGZ_TIME_CYCLES, SGZ_TIME_BEATS); return 0; }}\n')
        exe = os.path.join(d, "layout")
        subprocess.check_call([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    want = [getattr(api.ScopeConfig, f).offset for f in fields] + [C.sizeof(api.ScopeConfig), api.TIME_TIME, api.TIME_CYCLES, api.TIME_BEATS]
    assert got == want, (got, want)
    assert api.ScopeConfig().time_mode == 0                              # zero-initialised: the Time mode, the behaviour before
