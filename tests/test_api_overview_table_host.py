"""The binding's table of overview kinds (signalizer_amd/api.py: OVERVIEW_KINDS) against sgz.h's layout comments, written out here, and the
public methods that read it: every record's int64 words are its dtype's bytes, the shapes the table gives at (C, sides, P, bands) = (3, 2, 5, 4)
are the literal ones below, and the fifteen Plan methods keep the signatures recorded from before they were written over the table."""
import inspect

import numpy as np
import pytest

from signalizer_amd import api

DIMS = (3, 2, 5, 4)                                  # C, sides, P, bands
BINS = 65                                            # N + 1 of a 64-point plan
F32, U8 = np.dtype(np.float32), np.dtype(np.uint8)

# kind -> (suffix, record dtype, itemsize, words, one frame of the stage call's input, carry / record cell,
#          outputs in C order: (want keyword, column shape, dtype, leading planes), decay state, _view forms)
EXPECTED = {
    "peaks": ("", F32, 4, 0, (3, 2, 5, 2), (3, 5),
              [("want_rgba", (5, 4), U8, False), ("want_peaks", (3, 5), F32, False)], True, True),
    "stats": ("_stats", api.OVERVIEW_STAT_DTYPE, 24, 3, (3, 2, 5, 2), (3, 5),
              [("want_rgba", (5, 4), U8, False), ("want_stats", (3, 5), api.OVERVIEW_STAT_DTYPE, False), ("want_means", (3, 5), F32, False)],
              True, True),
    "pct": ("_pct", api.OVERVIEW_PCT_DTYPE, 272, 34, (3, 2, 5, 2), (3, 5),
            [("want_rgba", (5, 4), U8, False), ("want_records", (3, 5), api.OVERVIEW_PCT_DTYPE, False), ("want_values", (3, 5), F32, True)],
            True, False),
    "power": ("_power", api.OVERVIEW_POWER_DTYPE, 32, 4, (3, 2, 5), (3, 2, 5),
              [("want_rgba", (5, 4), U8, False), ("want_power", (3, 2, 5), api.OVERVIEW_POWER_DTYPE, False), ("want_levels", (3, 2, 5), F32, False)],
              False, True),
    "cross": ("_cross", api.OVERVIEW_CROSS_DTYPE, 80, 10, (3, 65, 2), (3, 4), [(None, (3, 4), api.OVERVIEW_CROSS_DTYPE, False)], False, False),
    "flux": ("_flux", api.OVERVIEW_FLUX_DTYPE, 88, 11, (3, 2, 5), (3, 2), [(None, (3, 2), api.OVERVIEW_FLUX_DTYPE, False)], False, False),
}

SIGNATURES = {
    "overview_columns": "(self, lines, k: 'int', held: 'int' = 0, flush: 'bool' = True, slices: 'int' = 0, carry=None, want_rgba: 'bool' = True, want_peaks: 'bool' = False, stream=None)",
    "overview": "(self, planar, k: 'int', want_rgba: 'bool' = True, want_peaks: 'bool' = False, state=None, stream=None)",
    "overview_stats_columns": "(self, lines, k: 'int', held: 'int' = 0, flush: 'bool' = True, slices: 'int' = 0, carry=None, want_rgba: 'bool' = True, want_stats: 'bool' = False, want_means: 'bool' = False, stream=None)",
    "overview_stats": "(self, planar, k: 'int', want_rgba: 'bool' = True, want_stats: 'bool' = False, want_means: 'bool' = False, state=None, stream=None)",
    "overview_pct_columns": "(self, lines, k: 'int', q=0.5, held: 'int' = 0, flush: 'bool' = True, slices: 'int' = 0, carry=None, want_rgba: 'bool' = True, want_records: 'bool' = False, want_values: 'bool' = False, stream=None)",
    "overview_pct": "(self, planar, k: 'int', q=0.5, want_rgba: 'bool' = True, want_records: 'bool' = False, want_values: 'bool' = False, state=None, stream=None)",
    "overview_power_columns": "(self, mapped, k: 'int', held: 'int' = 0, flush: 'bool' = True, slices: 'int' = 0, carry=None, want_rgba: 'bool' = True, want_power: 'bool' = False, want_levels: 'bool' = False, stream=None)",
    "overview_power": "(self, planar, k: 'int', want_rgba: 'bool' = True, want_power: 'bool' = False, want_levels: 'bool' = False, stream=None)",
    "overview_cross_columns": "(self, bins, k: 'int', held: 'int' = 0, flush: 'bool' = True, slices: 'int' = 0, carry=None, stream=None)",
    "overview_cross": "(self, planar, k: 'int', stream=None)",
    "overview_flux_columns": "(self, mapped, k: 'int', held: 'int' = 0, flush: 'bool' = True, first_frame: 'int' = 0, slices: 'int' = 0, prev=None, carry=None, stream=None)",
    "overview_flux": "(self, planar, k: 'int', stream=None)",
    "overview_view": "(self, peaks, out_columns: 'int', x0: 'int' = 0, x1: 'int | None' = None, slices: 'int' = 0, want_rgba: 'bool' = True, want_peaks: 'bool' = False, stream=None)",
    "overview_stats_view": "(self, stats, out_columns: 'int', x0: 'int' = 0, x1: 'int | None' = None, slices: 'int' = 0, want_rgba: 'bool' = True, want_stats: 'bool' = False, want_means: 'bool' = False, stream=None)",
    "overview_power_view": "(self, power, out_columns: 'int', x0: 'int' = 0, x1: 'int | None' = None, slices: 'int' = 0, want_rgba: 'bool' = True, want_power: 'bool' = False, want_levels: 'bool' = False, stream=None)",
}


def test_the_table_holds_the_six_kinds():
    assert list(api.OVERVIEW_KINDS) == list(EXPECTED)


@pytest.mark.parametrize("name", list(EXPECTED))
def test_a_kind_is_what_sgz_h_says(name):
    suffix, dtype, itemsize, words, source, cell, outputs, state, view = EXPECTED[name]
    kind = api.OVERVIEW_KINDS[name]
    assert (kind.suffix, kind.words, bool(kind.state), bool(kind.view)) == (suffix, words, state, view)
    assert np.dtype(kind.dtype) == dtype and np.dtype(kind.dtype).itemsize == itemsize
    if name == "peaks":
        assert kind.words == 0 and np.dtype(kind.dtype).fields is None          # plain float32 on both sides, no word axis
    else:
        assert kind.words * 8 == np.dtype(kind.dtype).itemsize
    assert api._overview_shape(kind.source, (*DIMS, BINS)) == source
    assert api._overview_shape(kind.cell, DIMS) == cell
    wants = [i % 2 == 0 for i, o in enumerate(o for o in outputs if o[0])]      # a flag per optional output, alternating
    got = api._overview_outputs(kind, DIMS, wants, planes=7)
    assert len(got) == len(outputs) and len(kind.outputs) == len(outputs)
    flags = iter(wants)
    for entry, table, (want, shape, out_dtype, planes) in zip(got, kind.outputs, outputs):
        assert table[0] == want
        assert entry[0] is (next(flags) if want else True)
        assert entry[1] == shape and all(type(n) is int for n in entry[1])
        assert np.dtype(entry[2]) == out_dtype
        assert tuple(entry[3:]) == ((7,) if planes else ())


@pytest.mark.parametrize("name", list(EXPECTED))
def test_the_buffers_of_a_kind_are_never_empty_and_cut_to_the_columns(name):
    kind = api.OVERVIEW_KINDS[name]
    outputs = api._overview_outputs(kind, DIMS, [True] * len(kind.outputs), planes=2)
    for columns in (0, 3):
        for o in outputs:
            a = api._overview_out(columns, *o)
            lead = (2,) if o[3:] else ()
            assert isinstance(a, np.ndarray) and a.dtype == np.dtype(o[2]) and a.shape == (*lead, max(columns, 1), *o[1]) and not any(a.tobytes())
            assert api._overview_cut(a, columns, *o).shape == (*lead, columns, *o[1])
    assert api._overview_out(3, False, (5, 4), np.uint8) is None and api._overview_cut(None, 3, False, (5, 4), np.uint8) is None


@pytest.mark.parametrize("method", list(SIGNATURES))
def test_a_public_method_keeps_its_signature_and_docstring(method):
    f = getattr(api.Plan, method)
    assert str(inspect.signature(f)) == SIGNATURES[method]
    assert f.__doc__ and "sgz_" in f.__doc__


@pytest.mark.parametrize("name", list(EXPECTED))
def test_the_methods_of_a_kind_take_its_want_flags_in_the_table_s_order(name):
    kind = api.OVERVIEW_KINDS[name]
    wants = [o[0] for o in kind.outputs if o[0]]
    forms = ["_columns", ""] + (["_view"] if kind.view else [])
    for form in forms:
        parameters = list(inspect.signature(getattr(api.Plan, "overview" + kind.suffix + form)).parameters)
        assert [p for p in parameters if p.startswith("want_")] == wants, (name, form)
        assert ("state" in parameters) == (bool(kind.state) and form == ""), (name, form)
    assert hasattr(api.Plan, "overview" + kind.suffix + "_view") == bool(kind.view)


def test_timing_reads_as_a_dict():
    t = api.Timing(1.0, 2.0, 3.0, 4)
    assert t.asdict() == {"h2d_ms": 1.0, "kernel_ms": 2.0, "d2h_ms": 3.0, "frames": 4} and list(t.asdict()) == ["h2d_ms", "kernel_ms", "d2h_ms", "frames"]
