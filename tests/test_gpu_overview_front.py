"""The front that the per-pixel overview kinds share (csrc/overview_kinds.hpp: the step of a call, the column / slice bounds, a thread's
cell, the carry snapshot, the slice choice and the one launch or the slice-then-emit pair), held to itself across the four kinds
sgz_stage_overview, sgz_stage_overview_stats, sgz_stage_overview_power and sgz_stage_overview_pct.

One table of call geometries (k, held, frames, flush) runs through every kind at P in {2, 257} (a single partial block; a tail block of one
thread -- for the percentile kind's 64-lane workgroups and, with the power kind's two sides, 2 * 257 = 514 = 2 * 256 + 2 values, a tail block
of two), pairs in {1, 3} and slices in {0, 1, 2, 64} (64 is more than any column has frames: empty slices).  Bytes only, no tolerance:
  1. the call cut in two gives the bytes of the uncut call in every output, and in the carry where a column stays open (where none does the
     call leaves the carry alone, so there is nothing of the call's to compare); the second call's `held` is what the first one left;
  2. every output is one column larger than the call closes and pre-filled with a poison pattern: the surplus column still holds it.
A carry for held > 0 is made by the kind itself from `held` frames of other content.  What a kind computes is held to its restatement in its
own test file; nothing here knows a record's meaning."""
import ctypes as C

import numpy as np
import pytest

from signalizer_amd import api, config

pytestmark = pytest.mark.gpu

POISON = 0xA5
SLICES = (0, 1, 2, 64)
# (k, held, frames, flush): at most 23 frames each
GEOMETRIES = [
    (5, 0, 3, 0), (5, 2, 2, 0),                  # t < k: only an open column
    (5, 0, 10, 0), (5, 3, 7, 0), (1, 0, 4, 0),   # t a multiple of k: nothing stays open
    (5, 0, 13, 1), (5, 2, 9, 1), (1, 0, 7, 1),   # flush, with a remainder where k > 1
    (5, 3, 0, 1),                                # no frames, the held column flushed
    (5, 2, 11, 0), (5, 4, 23, 0),                # held > 0, more than one column, the last one open: column 0 reads the carry's snapshot
    (5, 0, 23, 0),
]
MOST = 23
Q = np.array([0.5], np.float64)                  # the percentile kind's one quantile: its value plane is [columns][pairs][P] like the others


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class Kind:
    """what a kind's stage call takes: the bytes of its carry and of one column of each output"""

    def __init__(self, name, pairs, sides, P):
        self.name = name
        cells = pairs * (sides if name == "power" else 1) * P
        record = {"peaks": 4, "stats": 24, "power": 32, "pct": 272}[name]
        self.carry_bytes = cells * record
        self.out_bytes = [P * 4, cells * record] + ([] if name == "peaks" else [cells * 4])

    def call(self, plan, d_in, frames, k, held, flush, slices, carry, outs):
        L = api.lib()
        head = (plan.h, d_in.data_ptr(), frames, k, held, flush, slices)
        ptrs = [carry.data_ptr()] + [o.data_ptr() for o in outs] + [_stream()]
        if self.name == "peaks":
            st = L.sgz_stage_overview(*head, *ptrs)
        elif self.name == "stats":
            st = L.sgz_stage_overview_stats(*head, *ptrs)
        elif self.name == "power":
            st = L.sgz_stage_overview_power(*head, *ptrs)
        else:
            st = L.sgz_stage_overview_pct(*head, Q.ctypes.data_as(C.c_void_p), 1, *ptrs)
        assert st == api.SGZ_OK, (self.name, L.sgz_last_error())


def _planted(x, rng):
    """NaN, +-inf and -0 planted in a float32 array: scattered, and one of each for certain"""
    values = np.float32([np.nan, np.inf, -np.inf, -0.0])
    for value in values:
        x[rng.random(x.shape) < 0.04] = value
    x.reshape(-1)[rng.choice(x.size, values.size, replace=False)] = values
    assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any() and ((x == 0) & np.signbit(x)).any()
    return x


def _inputs(name, frames, pairs, sides, P, rng):
    """the kind's input: mapped magnitudes [frames][pairs][sides][P], or line results [frames][pairs][G][P][2] with the values the kinds read
    (graph 0's first component, around the colour range) planted and noise elsewhere"""
    if name == "power":
        return _planted((10.0 ** rng.uniform(-6, 0.5, (frames, pairs, sides, P))).astype(np.float32), rng)
    lines = rng.standard_normal((frames, pairs, api.NUM_GRAPHS, P, 2)).astype(np.float32)
    lines[:, :, 0, :, 0] = _planted((rng.random((frames, pairs, P)) * 1.4 - 0.2).astype(np.float32), rng)
    return lines


def _poisoned(gpu, nbytes):
    import torch
    return torch.full((max(nbytes, 16),), POISON, dtype=torch.uint8, device=gpu)


@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("P", [2, 257])
@pytest.mark.parametrize("name", ["peaks", "stats", "power", "pct"])
def test_a_cut_call_is_the_uncut_call_and_no_surplus_column_is_written(gpu, name, P, pairs):
    import torch
    sides = 2
    cfg = config.spectrum_config(window_size=64, hop=16, axis_points=P, num_pairs=pairs, channel_mode=config.CH_SEPARATE,
                                 bin_interp=config.INTERP_LINEAR)
    plan = api.Plan(cfg).upload()
    assert (plan.C, plan.sides, plan.P) == (pairs, sides, P)
    kind = Kind(name, pairs, sides, P)
    rng = np.random.default_rng(1000 * P + 10 * pairs + len(name))
    d_x = torch.from_numpy(_inputs(name, MOST, pairs, sides, P, rng)).to(gpu)
    d_other = torch.from_numpy(_inputs(name, 4, pairs, sides, P, rng)).to(gpu)

    def outputs(closed):
        return [_poisoned(gpu, (closed + 1) * b) for b in kind.out_bytes]

    def at(outs, column):
        return [o[column * b:] for o, b in zip(outs, kind.out_bytes)]

    carries = {}                                 # (k, held) -> the kind's own carry of `held` frames of other content

    def carry_of(k, held):
        if (k, held) not in carries:
            c = _poisoned(gpu, kind.carry_bytes)
            if held:
                kind.call(plan, d_other, held, k, 0, 0, 1, c, outputs(0))
            carries[(k, held)] = c
        return carries[(k, held)].clone()

    for k, held, frames, flush in GEOMETRIES:
        closed, left = api.overview_step(k, held, frames, flush)
        cut = frames // 2
        closed1, held1 = api.overview_step(k, held, cut, 0)
        closed2, left2 = api.overview_step(k, held1, frames - cut, flush)
        assert (closed1 + closed2, left2) == (closed, left)
        for slices in SLICES:
            what = (name, P, pairs, k, held, frames, flush, slices)
            whole, whole_carry = outputs(closed), carry_of(k, held)
            kind.call(plan, d_x, frames, k, held, flush, slices, whole_carry, whole)
            parts, parts_carry = outputs(closed), carry_of(k, held)
            kind.call(plan, d_x, cut, k, held, 0, slices, parts_carry, parts)
            kind.call(plan, d_x[cut:], frames - cut, k, held1, flush, slices, parts_carry, at(parts, closed1))
            for a, b, width in zip(whole, parts, kind.out_bytes):
                a, b = a.cpu().numpy(), b.cpu().numpy()
                assert np.array_equal(a, b), what
                assert (a[closed * width:] == POISON).all(), what
                assert closed == 0 or not (a[:closed * width] == POISON).all(), what         # (the call did write its columns)
            if left:
                assert torch.equal(whole_carry, parts_carry), what
