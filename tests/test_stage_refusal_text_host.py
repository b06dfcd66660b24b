"""The text of every argument refusal of the eight sgz_stage_<lane>_columns calls (csrc/column_lanes.hpp checkStageArgs / checkStageBuffers, which
the eight calls share): sgz_last_error() word for word, as the calls worded it when each had checks of its own (the histogram and the run lane:
as they worded it when each still wrote its stage call out).  Host only: the refusals come before the device is touched, on fake addresses
that are never dereferenced."""
import ctypes as C

import pytest

from signalizer_amd import api

E = api.SGZ_EINVAL
LANES = ("wave", "level", "field", "truepeak", "loudness", "band", "hist", "run")
PLANAR, CARRY, OUT = 0x10000, 0x20000, 0x30000

# the arguments of a call that passes every check (100 samples, m = 8, flush), then one change per case
GOOD = dict(planar=PLANAR, stride=128, cells=1, n=100, filter="good", params="good", first=0, m=8, held=0, flush=1, continued=0, slices=0, carry=CARRY, out=OUT)
CASES = {
    "null d_planar": dict(planar=None),
    "null filter": dict(filter=None),
    "filter shape": dict(filter="W 64 L 48"),
    "filter too long": dict(filter="W 32768"),
    "null params": dict(params=None),
    "params hot 0": dict(params="hot 0"),
    "params quiet not below hot": dict(params="quiet = hot"),
    "cells 0": dict(cells=0),
    "cells above the most": dict(cells=65),
    "m 0": dict(m=0),
    "held not below m": dict(held=8, continued=1),
    "held without continued": dict(held=3),
    "stride below nsamples": dict(stride=99),
    "too many samples": dict(stride=2 ** 63, n=2 ** 62 + 1),
    "first_index": dict(first=2 ** 63),
    "slices": dict(slices=65),
    "d_planar alignment": dict(planar=PLANAR + 2),
    "d_carry alignment": dict(carry=CARRY + 4, held=3, continued=1),
    "output alignment": dict(out=OUT + 4),
    "null d_carry, written": dict(carry=None, flush=0),
    "null d_carry, read": dict(carry=None, n=0, held=3, continued=1),
    "null output": dict(out=None),
    "null output, flushed carry": dict(out=None, n=0, held=3, continued=1),
    # ... and the first check wins where two arguments are wrong
    "null d_planar and null filter": dict(planar=None, filter=None),
    "null filter and cells 0": dict(filter=None, cells=0),
    "null d_planar and null params": dict(planar=None, params=None),
    "null params and cells 0": dict(params=None, cells=0),
}


def _filter(lane, which):
    if which is None:
        return None
    f = api.loudness_filter_for_rate(48000.0) if lane == "loudness" else api.band_filter_for_rate(48000.0)
    if which == "W 64 L 48":
        f.W, f.L = 64, 48
    elif which == "W 32768":
        f.W, f.L = 32768, 64
    return C.byref(f)


def _params(which):
    if which is None:
        return None
    p = api.run_params_default()
    if which == "hot 0":
        p.hot = 0
    elif which == "quiet = hot":
        p.quiet = p.hot
    return C.byref(p)


def refusal(L, lane, case):
    """sgz_last_error() of the lane's stage call with the case's arguments; None where the lane has no such argument or refuses nothing"""
    a = dict(GOOD, **CASES[case])
    filtered, history = lane in ("loudness", "band"), lane in ("truepeak", "loudness", "band", "run")
    if (("filter" in CASES[case] or "first" in CASES[case]) and not filtered) or (case == "held without continued" and not history):
        return None
    if "params" in CASES[case] and lane != "run":
        return None
    if lane in ("level", "field") and case == "cells above the most":
        a["cells"] = 33
    call = getattr(L, f"sgz_stage_{lane}_columns")
    if filtered:
        st = call(a["planar"], a["stride"], a["cells"], a["n"], _filter(lane, a["filter"]), a["first"], a["m"], a["held"], a["flush"], a["continued"], a["slices"],
                  a["carry"], a["out"], None)
    elif history:
        front = (_params(a["params"]),) if lane == "run" else ()
        st = call(a["planar"], a["stride"], a["cells"], a["n"], *front, a["m"], a["held"], a["flush"], a["continued"], a["slices"], a["carry"], a["out"], None)
    else:
        st = call(a["planar"], a["stride"], a["cells"], a["n"], a["m"], a["held"], a["flush"], a["slices"], a["carry"], a["out"], None)
    if st == api.SGZ_OK:
        return None
    assert st == E, (lane, case, st)
    return L.sgz_last_error().decode()


# what the calls said before they shared their front (recorded from that build)
EXPECTED = {
    ("wave", "null d_planar"): "sgz_stage_wave_columns: null d_planar",
    ("wave", "cells 0"): "sgz_stage_wave_columns: 1 .. 64 channels",
    ("wave", "cells above the most"): "sgz_stage_wave_columns: 1 .. 64 channels",
    ("wave", "m 0"): "sgz_stage_wave_columns: m >= 1 samples per column",
    ("wave", "held not below m"): "sgz_stage_wave_columns: held < m",
    ("wave", "stride below nsamples"): "sgz_stage_wave_columns: channel_stride < nsamples",
    ("wave", "too many samples"): "sgz_stage_wave_columns: channel_stride < nsamples",
    ("wave", "slices"): "sgz_stage_wave_columns: slices 0 (automatic) or 1 .. 64",
    ("wave", "d_planar alignment"): "sgz_stage_wave_columns: d_planar aligned to 4 bytes, d_carry and d_wave to 8",
    ("wave", "d_carry alignment"): "sgz_stage_wave_columns: d_planar aligned to 4 bytes, d_carry and d_wave to 8",
    ("wave", "output alignment"): "sgz_stage_wave_columns: d_planar aligned to 4 bytes, d_carry and d_wave to 8",
    ("wave", "null d_carry, written"): "sgz_stage_wave_columns: d_carry is read (held > 0) or written (samples stay open)",
    ("wave", "null d_carry, read"): "sgz_stage_wave_columns: d_carry is read (held > 0) or written (samples stay open)",
    ("wave", "null output"): "sgz_stage_wave_columns: d_wave is written (a column closes)",
    ("wave", "null output, flushed carry"): "sgz_stage_wave_columns: d_wave is written (a column closes)",
    ("level", "null d_planar"): "sgz_stage_level_columns: null d_planar",
    ("level", "cells 0"): "sgz_stage_level_columns: 1 .. 32 pairs",
    ("level", "cells above the most"): "sgz_stage_level_columns: 1 .. 32 pairs",
    ("level", "m 0"): "sgz_stage_level_columns: m >= 1 samples per column",
    ("level", "held not below m"): "sgz_stage_level_columns: held < m",
    ("level", "stride below nsamples"): "sgz_stage_level_columns: channel_stride < nsamples",
    ("level", "too many samples"): "sgz_stage_level_columns: channel_stride < nsamples",
    ("level", "slices"): "sgz_stage_level_columns: slices 0 (automatic) or 1 .. 64",
    ("level", "d_planar alignment"): "sgz_stage_level_columns: d_planar aligned to 4 bytes, d_carry and d_level to 16",
    ("level", "d_carry alignment"): "sgz_stage_level_columns: d_planar aligned to 4 bytes, d_carry and d_level to 16",
    ("level", "output alignment"): "sgz_stage_level_columns: d_planar aligned to 4 bytes, d_carry and d_level to 16",
    ("level", "null d_carry, written"): "sgz_stage_level_columns: d_carry is read (held > 0) or written (samples stay open)",
    ("level", "null d_carry, read"): "sgz_stage_level_columns: d_carry is read (held > 0) or written (samples stay open)",
    ("level", "null output"): "sgz_stage_level_columns: d_level is written (a column closes)",
    ("level", "null output, flushed carry"): "sgz_stage_level_columns: d_level is written (a column closes)",
    ("field", "null d_planar"): "sgz_stage_field_columns: null d_planar",
    ("field", "cells 0"): "sgz_stage_field_columns: 1 .. 32 pairs",
    ("field", "cells above the most"): "sgz_stage_field_columns: 1 .. 32 pairs",
    ("field", "m 0"): "sgz_stage_field_columns: m >= 1 samples per column",
    ("field", "held not below m"): "sgz_stage_field_columns: held < m",
    ("field", "stride below nsamples"): "sgz_stage_field_columns: channel_stride < nsamples",
    ("field", "too many samples"): "sgz_stage_field_columns: channel_stride < nsamples",
    ("field", "slices"): "sgz_stage_field_columns: slices 0 (automatic) or 1 .. 64",
    ("field", "d_planar alignment"): "sgz_stage_field_columns: d_planar aligned to 4 bytes, d_carry and d_field to 16",
    ("field", "d_carry alignment"): "sgz_stage_field_columns: d_planar aligned to 4 bytes, d_carry and d_field to 16",
    ("field", "output alignment"): "sgz_stage_field_columns: d_planar aligned to 4 bytes, d_carry and d_field to 16",
    ("field", "null d_carry, written"): "sgz_stage_field_columns: d_carry is read (held > 0) or written (samples stay open)",
    ("field", "null d_carry, read"): "sgz_stage_field_columns: d_carry is read (held > 0) or written (samples stay open)",
    ("field", "null output"): "sgz_stage_field_columns: d_field is written (a column closes)",
    ("field", "null output, flushed carry"): "sgz_stage_field_columns: d_field is written (a column closes)",
    ("truepeak", "null d_planar"): "sgz_stage_truepeak_columns: null d_planar",
    ("truepeak", "cells 0"): "sgz_stage_truepeak_columns: 1 .. 64 channels",
    ("truepeak", "cells above the most"): "sgz_stage_truepeak_columns: 1 .. 64 channels",
    ("truepeak", "m 0"): "sgz_stage_truepeak_columns: m >= 1 samples per column",
    ("truepeak", "held not below m"): "sgz_stage_truepeak_columns: held < m",
    ("truepeak", "held without continued"): "sgz_stage_truepeak_columns: held > 0 needs continued != 0 (a stream that begins here has no open column)",
    ("truepeak", "stride below nsamples"): "sgz_stage_truepeak_columns: channel_stride < nsamples",
    ("truepeak", "too many samples"): "sgz_stage_truepeak_columns: channel_stride < nsamples",
    ("truepeak", "slices"): "sgz_stage_truepeak_columns: slices 0 (automatic) or 1 .. 64",
    ("truepeak", "d_planar alignment"): "sgz_stage_truepeak_columns: d_planar aligned to 4 bytes, d_carry and d_peaks to 16",
    ("truepeak", "d_carry alignment"): "sgz_stage_truepeak_columns: d_planar aligned to 4 bytes, d_carry and d_peaks to 16",
    ("truepeak", "output alignment"): "sgz_stage_truepeak_columns: d_planar aligned to 4 bytes, d_carry and d_peaks to 16",
    ("truepeak", "null d_carry, written"): "sgz_stage_truepeak_columns: d_carry is read (continued) or written (nsamples > 0)",
    ("truepeak", "null d_carry, read"): "sgz_stage_truepeak_columns: d_carry is read (continued) or written (nsamples > 0)",
    ("truepeak", "null output"): "sgz_stage_truepeak_columns: d_peaks is written (a column closes)",
    ("truepeak", "null output, flushed carry"): "sgz_stage_truepeak_columns: d_peaks is written (a column closes)",
    ("loudness", "null d_planar"): "sgz_stage_loudness_columns: null d_planar",
    ("loudness", "null filter"): "sgz_stage_loudness_columns: null filter",
    ("loudness", "filter shape"): "sgz_stage_loudness_columns: W and L are powers of two, 16 <= L <= W <= 65536",
    ("loudness", "filter too long"): "sgz_stage_loudness_columns: the device takes W <= 16384",
    ("loudness", "cells 0"): "sgz_stage_loudness_columns: 1 .. 64 channels",
    ("loudness", "cells above the most"): "sgz_stage_loudness_columns: 1 .. 64 channels",
    ("loudness", "m 0"): "sgz_stage_loudness_columns: m >= 1 samples per column",
    ("loudness", "held not below m"): "sgz_stage_loudness_columns: held < m",
    ("loudness", "held without continued"): "sgz_stage_loudness_columns: held > 0 needs continued != 0 (a stream that begins here has no open column)",
    ("loudness", "stride below nsamples"): "sgz_stage_loudness_columns: channel_stride < nsamples, or more than 2^40 samples",
    ("loudness", "too many samples"): "sgz_stage_loudness_columns: channel_stride < nsamples, or more than 2^40 samples",
    ("loudness", "first_index"): "sgz_stage_loudness_columns: first_index above 2^62",
    ("loudness", "slices"): "sgz_stage_loudness_columns: slices 0 (automatic) or 1 .. 64",
    ("loudness", "d_planar alignment"): "sgz_stage_loudness_columns: d_planar aligned to 4 bytes, d_carry and d_records to 16",
    ("loudness", "d_carry alignment"): "sgz_stage_loudness_columns: d_planar aligned to 4 bytes, d_carry and d_records to 16",
    ("loudness", "output alignment"): "sgz_stage_loudness_columns: d_planar aligned to 4 bytes, d_carry and d_records to 16",
    ("loudness", "null d_carry, written"): "sgz_stage_loudness_columns: d_carry is read (continued) or written (nsamples > 0)",
    ("loudness", "null d_carry, read"): "sgz_stage_loudness_columns: d_carry is read (continued) or written (nsamples > 0)",
    ("loudness", "null output"): "sgz_stage_loudness_columns: d_records is written (a column closes)",
    ("loudness", "null output, flushed carry"): "sgz_stage_loudness_columns: d_records is written (a column closes)",
    ("loudness", "null d_planar and null filter"): "sgz_stage_loudness_columns: null d_planar",
    ("loudness", "null filter and cells 0"): "sgz_stage_loudness_columns: null filter",
    ("band", "null d_planar"): "sgz_stage_band_columns: null d_planar",
    ("band", "null filter"): "sgz_stage_band_columns: null filter",
    ("band", "filter shape"): "sgz_stage_band_columns: W and L are powers of two, 16 <= L <= W <= 65536",
    ("band", "filter too long"): "sgz_stage_band_columns: the device takes W <= 16384",
    ("band", "cells 0"): "sgz_stage_band_columns: 1 .. 64 channels",
    ("band", "cells above the most"): "sgz_stage_band_columns: 1 .. 64 channels",
    ("band", "m 0"): "sgz_stage_band_columns: m >= 1 samples per column",
    ("band", "held not below m"): "sgz_stage_band_columns: held < m",
    ("band", "held without continued"): "sgz_stage_band_columns: held > 0 needs continued != 0 (a stream that begins here has no open column)",
    ("band", "stride below nsamples"): "sgz_stage_band_columns: channel_stride < nsamples, or more than 2^40 samples",
    ("band", "too many samples"): "sgz_stage_band_columns: channel_stride < nsamples, or more than 2^40 samples",
    ("band", "first_index"): "sgz_stage_band_columns: first_index above 2^62",
    ("band", "slices"): "sgz_stage_band_columns: slices 0 (automatic) or 1 .. 64",
    ("band", "d_planar alignment"): "sgz_stage_band_columns: d_planar aligned to 4 bytes, d_carry and d_records to 16",
    ("band", "d_carry alignment"): "sgz_stage_band_columns: d_planar aligned to 4 bytes, d_carry and d_records to 16",
    ("band", "output alignment"): "sgz_stage_band_columns: d_planar aligned to 4 bytes, d_carry and d_records to 16",
    ("band", "null d_carry, written"): "sgz_stage_band_columns: d_carry is read (continued) or written (nsamples > 0)",
    ("band", "null d_carry, read"): "sgz_stage_band_columns: d_carry is read (continued) or written (nsamples > 0)",
    ("band", "null output"): "sgz_stage_band_columns: d_records is written (a column closes)",
    ("band", "null output, flushed carry"): "sgz_stage_band_columns: d_records is written (a column closes)",
    ("band", "null d_planar and null filter"): "sgz_stage_band_columns: null d_planar",
    ("band", "null filter and cells 0"): "sgz_stage_band_columns: null filter",
    # the histogram and the run lane: recorded from the build in which each still wrote its stage call out
    ("hist", "null d_planar"): "sgz_stage_hist_columns: null d_planar",
    ("hist", "cells 0"): "sgz_stage_hist_columns: 1 .. 64 channels",
    ("hist", "cells above the most"): "sgz_stage_hist_columns: 1 .. 64 channels",
    ("hist", "m 0"): "sgz_stage_hist_columns: m >= 1 samples per column",
    ("hist", "held not below m"): "sgz_stage_hist_columns: held < m",
    ("hist", "stride below nsamples"): "sgz_stage_hist_columns: channel_stride < nsamples",
    ("hist", "too many samples"): "sgz_stage_hist_columns: channel_stride < nsamples",
    ("hist", "slices"): "sgz_stage_hist_columns: slices 0 (automatic) or 1 .. 64",
    ("hist", "d_planar alignment"): "sgz_stage_hist_columns: d_planar aligned to 4 bytes, d_carry and d_hist to 16",
    ("hist", "d_carry alignment"): "sgz_stage_hist_columns: d_planar aligned to 4 bytes, d_carry and d_hist to 16",
    ("hist", "output alignment"): "sgz_stage_hist_columns: d_planar aligned to 4 bytes, d_carry and d_hist to 16",
    ("hist", "null d_carry, written"): "sgz_stage_hist_columns: d_carry is read (held > 0) or written (samples stay open)",
    ("hist", "null d_carry, read"): "sgz_stage_hist_columns: d_carry is read (held > 0) or written (samples stay open)",
    ("hist", "null output"): "sgz_stage_hist_columns: d_hist is written (a column closes)",
    ("hist", "null output, flushed carry"): "sgz_stage_hist_columns: d_hist is written (a column closes)",
    ("run", "null d_planar"): "sgz_stage_run_columns: null d_planar",
    ("run", "null params"): "sgz_stage_run_columns: null params",
    ("run", "params hot 0"): "sgz_stage_run_columns: 1 <= hot <= 2^26 and quiet < hot",
    ("run", "params quiet not below hot"): "sgz_stage_run_columns: 1 <= hot <= 2^26 and quiet < hot",
    ("run", "cells 0"): "sgz_stage_run_columns: 1 .. 64 channels",
    ("run", "cells above the most"): "sgz_stage_run_columns: 1 .. 64 channels",
    ("run", "m 0"): "sgz_stage_run_columns: m >= 1 samples per column",
    ("run", "held not below m"): "sgz_stage_run_columns: held < m",
    ("run", "held without continued"): "sgz_stage_run_columns: held > 0 needs continued != 0 (a stream that begins here has no open column)",
    ("run", "stride below nsamples"): "sgz_stage_run_columns: channel_stride < nsamples",
    ("run", "too many samples"): "sgz_stage_run_columns: channel_stride < nsamples",
    ("run", "slices"): "sgz_stage_run_columns: slices 0 (automatic) or 1 .. 64",
    ("run", "d_planar alignment"): "sgz_stage_run_columns: d_planar aligned to 4 bytes, d_carry and d_runs to 16",
    ("run", "d_carry alignment"): "sgz_stage_run_columns: d_planar aligned to 4 bytes, d_carry and d_runs to 16",
    ("run", "output alignment"): "sgz_stage_run_columns: d_planar aligned to 4 bytes, d_carry and d_runs to 16",
    ("run", "null d_carry, written"): "sgz_stage_run_columns: d_carry is read (continued) or written (nsamples > 0)",
    ("run", "null d_carry, read"): "sgz_stage_run_columns: d_carry is read (continued) or written (nsamples > 0)",
    ("run", "null output"): "sgz_stage_run_columns: d_runs is written (a column closes)",
    ("run", "null output, flushed carry"): "sgz_stage_run_columns: d_runs is written (a column closes)",
    ("run", "null d_planar and null params"): "sgz_stage_run_columns: null d_planar",
    ("run", "null params and cells 0"): "sgz_stage_run_columns: null params",
}


@pytest.mark.parametrize("lane", LANES)
def test_stage_refusals_word_for_word(lane):
    L = api.lib()
    got = {(lane, case): refusal(L, lane, case) for case in CASES}
    want = {(lane, case): EXPECTED.get((lane, case)) for case in CASES}
    assert got == want
    assert sum(v is not None for v in want.values()) >= 15                   # (the table holds this lane's refusals, not a run of Nones)
