"""The flux overview's stage call on the GPU (csrc/overview_flux.hip: overviewFluxColumnsKernel / SliceKernel in their three modes and the emit
kernel; sgz_stage_overview_flux) on arbitrary floats, no K_A in front.

Every comparison is on bytes against tests/overview_flux_ref.py (held to exact rational arithmetic in tests/test_overview_flux_host.py); no
tolerance anywhere.  Every output lies between sentinel rows, outputs that are not due stay untouched.
Shapes: P 2, 63, 64, 65, 257 (one pass of 1024 pixels, the previous a in registers), 1500 (two passes), 5000 (the previous frame in LDS) and
70 001 (fetched again; three frames whose top pixels are clamped, so that mom2 of one frame passes 2^64); pairs 1 and 3, sides 1 and 2.
The kernel's constants the frame counts aim at: a run of whole columns has at most 32 frames and shrinks while the launch would have fewer
than 512 workgroups; without an explicit count a column is sliced when k >= 16 and columns * rows < 512.
Inputs: magnitudes log-uniform over 2^-35 .. 2^5; NaN, +-inf and -0 planted; row 0 alternates between two frames, so that every even and
every odd frame has the same F and the maxima of a column tie across run, slice and call boundaries: the earliest index must win."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_flux_ref as ofr  # noqa: E402
from test_gpu_overview import Guarded, _stream  # noqa: E402

pytestmark = pytest.mark.gpu

RW = 22                                                      # 32-bit words of a record
SHAPES = [(1, 1, 2), (3, 2, 2), (1, 2, 63), (1, 1, 64), (3, 1, 65), (1, 2, 257), (1, 2, 1500), (1, 1, 5000)]
KS = (1, 3, 8)
SLICES = (0, 1, 5, 64)
FAR = 2 ** 32 + 12345                                        # a first_frame above 2^32
FRAMES = 40


def _f(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def _cfg(pairs, sides, P):
    return config.spectrum_config(window_size=64, hop=16, axis_points=P, num_pairs=pairs,
                                  channel_mode=config.CH_SEPARATE if sides == 2 else config.CH_LEFT, bin_interp=config.INTERP_LINEAR)


def _mapped(frames, rows, P, seed):
    """float32 [frames][rows][P]: see the module's text"""
    rng = np.random.default_rng(seed)
    x = (2.0 ** rng.uniform(-35, 5, (frames, rows, P))).astype(np.float32)
    two = (2.0 ** rng.uniform(-35, 5, (2, P))).astype(np.float32)
    x[:, 0] = two[np.arange(frames) % 2]
    special = np.array([np.nan, np.inf, -np.inf, -0.0, _f(0xFFC00001), 16.0, -17.0, 3 * 2.0 ** -31, 2.0 ** -31, 0.0], np.float32)
    for f in range(3, frames, 7):                            # (in the last row: row 0 keeps its ties where there is more than one row)
        at = rng.integers(0, P, 3)
        x[f, -1, at] = rng.choice(special, 3)
    if frames > 5:
        x[5, -1, P - 1] = np.nan
    return x


class Case:
    """one plan, its values on the device, another frame as the predecessor and other frames for the carries"""

    def __init__(self, gpu, pairs, sides, P, frames=FRAMES):
        import torch
        self.plan = api.Plan(_cfg(pairs, sides, P))                  # (the stage call reads no table of the plan: it is never uploaded)
        assert (self.plan.C, self.plan.sides, self.plan.P) == (pairs, sides, P)
        self.rows, self.P, self.gpu = pairs * sides, P, gpu
        seed = 1000 * pairs + 100 * sides + P
        self.x = _mapped(frames, self.rows, P, seed)
        self.before = _mapped(1, self.rows, P, seed + 1)[0]
        self.before[-1, 0] = np.nan                                  # a NaN predecessor counts as a = 0 and marks nothing
        self.other = _mapped(8, self.rows, P, seed + 2)
        self.d_x = torch.from_numpy(self.x).to(gpu)
        self.terms = {False: ofr.frame_terms(self.x), True: ofr.frame_terms(self.x, self.before)}

    def want(self, frames, k, held, flush, first, with_prev):
        carry = ofr.overview(self.other[:held], k, first_frame=first - held if first >= held else 0, flush=False)[1] if held else None
        terms = tuple(t[:frames] for t in self.terms[with_prev])
        cols, left = ofr.overview(self.x[:frames], k, first_frame=first, held=held, carry=carry, flush=flush, terms=terms)
        return cols, left, carry

    def call(self, frames, k, held, flush, first, slices, with_prev, carry, d_x=None, prev=None, carry_block=None):
        """the stage call between sentinels: (records [columns, rows], the carry block, the prev block)"""
        import torch
        columns, left = api.overview_step(k, held, frames, flush)
        out = Guarded(self.gpu, columns, self.rows * RW, torch.int32)
        cb = carry_block or Guarded(self.gpu, 1, self.rows * RW, torch.int32)
        if carry is not None:
            cb.set(ofr.pack(carry).view(np.uint32))
        pb = prev
        if with_prev and pb is None:
            pb = Guarded(self.gpu, 1, self.rows * self.P, torch.int32)
            pb.set(self.before.view(np.uint32))
        api.check(api.lib().sgz_stage_overview_flux(self.plan.h, (d_x if d_x is not None else self.d_x).data_ptr(), frames, k, held, int(flush), first, slices,
                                                    pb.ptr if pb is not None else None, cb.ptr, out.ptr, _stream()))
        torch.cuda.synchronize()
        got = np.ascontiguousarray(out.payload()).reshape(-1).view(ofr.DTYPE).reshape(columns, self.rows)
        return got, cb, pb


_cases = {}


def _case(gpu, shape):
    if shape not in _cases:
        _cases[shape] = Case(gpu, *shape)
    return _cases[shape]


def _bytes(a):
    return np.ascontiguousarray(a).tobytes()


def _check(c, frames, k, held, flush, first, slices, with_prev):
    want, left, carry = c.want(frames, k, held, flush, first, with_prev)
    got, cb, pb = c.call(frames, k, held, flush, first, slices, with_prev, carry)
    tag = (frames, k, held, flush, first, slices, with_prev)
    assert got.shape == want.shape and _bytes(got) == _bytes(want), tag
    if left is not None:
        assert _bytes(cb.payload()) == _bytes(ofr.pack(left)), tag       # the open column
    elif carry is not None:
        assert _bytes(cb.payload()) == _bytes(ofr.pack(carry)), tag      # read, not written
    else:
        assert cb.untouched(), tag
    if with_prev:
        assert _bytes(pb.payload()) == _bytes(c.x[frames - 1]), tag      # the call's last frame


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stage_call_equals_the_restatement(gpu, shape):
    c = _case(gpu, shape)
    calls = 0
    for k in KS:
        for frames in sorted({1, 2, k - 1, k, k + 1, FRAMES} - {0}):
            for held in sorted({0, k - 1}):
                for flush in (False, True):
                    for with_prev in (False, True):
                        _check(c, frames, k, held, flush, (0, FAR)[calls % 2], SLICES[(calls // 2) % 4], with_prev)
                        calls += 1
    # every slice count on one call with a carry, ties and a column that stays open
    for slices in SLICES + (2, 3):
        _check(c, FRAMES, 8, 7, False, FAR, slices, True)
        _check(c, FRAMES - 1, 3, 2, True, 0, slices, False)


@pytest.mark.parametrize("k,frames", [(16, 40), (64, 130), (64, 63), (100, 130)])
def test_columns_above_the_slice_threshold(gpu, k, frames):
    """k >= 16 with few columns: the call slices on its own (2, 8 and 12 slices); the bytes are those of one slice and of the restatement"""
    import torch
    rows, P = 2, 257
    c = Case(gpu, 1, 2, P, frames=frames)
    for held, flush, with_prev in ((0, True, False), (k - 1, False, True), (5, True, True)):
        for slices in (0, 1):
            _check(c, frames, k, held, flush, FAR, slices, with_prev)


@pytest.mark.parametrize("k,frames", [(1, 2751), (1, 2752), (1, 2753), (3, 2752), (1, 700), (8, 2753)])
def test_runs_of_several_columns(gpu, k, frames):
    """P = 2, six rows: enough columns for runs of 32 (k = 1), 30 (k = 3, ten columns), 8 (700 frames) and 32 (k = 8, four columns) frames --
    one below, at and one above a whole number of runs.  Row 0's ties fall on both sides of every run boundary"""
    key = ("runs", 2753)
    if key not in _cases:
        _cases[key] = Case(gpu, 3, 2, 2, frames=2753)
    c = _cases[key]
    _check(c, frames, k, 0, True, FAR, 0, True)
    _check(c, frames, k, k - 1, False, 0, 0, False)


def test_one_frame_whose_second_moment_passes_two_to_the_64(gpu):
    import torch
    P = 70001
    c = Case(gpu, 1, 1, P, frames=3)
    c.x[:, 0, P - 40:] = np.array([16.0, 1e30, np.inf], np.float32)[:, None]     # clamped: a = 2^34 at i ~ 2^16
    c.x[1, 0, P - 1] = np.nan
    c.d_x = torch.from_numpy(c.x).to(gpu)
    c.terms = {False: ofr.frame_terms(c.x), True: ofr.frame_terms(c.x, c.before)}
    one = ofr.overview(c.x[:1], 1)[0]
    assert ofr.unpack(one[0, 0])["mom2"] > 2 ** 64
    for k, held, flush, slices, with_prev in ((1, 0, True, 0, True), (3, 0, True, 0, False), (3, 0, True, 2, True), (8, 5, False, 0, True), (2, 1, True, 64, False)):
        _check(c, 3, k, held, flush, FAR, slices, with_prev)


@pytest.mark.parametrize("shape", [(3, 2, 65), (1, 2, 1500), (1, 1, 5000)], ids=lambda s: "x".join(map(str, s)))
def test_any_cut_into_calls_gives_the_bytes_of_one_call(gpu, shape):
    """two and three calls chained through d_carry and d_prev, each reading and writing the same buffers"""
    import torch
    c = _case(gpu, shape)
    n = 0
    for k in KS:
        whole, _, _ = c.want(FRAMES, k, 0, True, FAR, True)
        for cuts in ((1,), (k,), (k + 1,), (17,), (39,), (2, 3), (k, 2 * k + 1), (7, 24), (16, 17)):
            edges = (0,) + cuts + (FRAMES,)
            cb = Guarded(gpu, 1, c.rows * RW, torch.int32)
            pb = Guarded(gpu, 1, c.rows * c.P, torch.int32)
            pb.set(c.before.view(np.uint32))
            parts, held = [], 0
            for a, b in zip(edges[:-1], edges[1:]):
                last = b == FRAMES
                got, cb, pb = c.call(b - a, k, held, last, FAR + a, SLICES[n % 4], True, None, d_x=c.d_x[a:], prev=pb, carry_block=cb)
                n += 1
                parts.append(got)
                held = (held + b - a) % k
                assert _bytes(pb.payload()) == _bytes(c.x[b - 1])
            assert _bytes(np.concatenate(parts)) == _bytes(whole), (k, cuts)


def test_refusals_launch_nothing(gpu):
    import torch
    c = _case(gpu, (1, 2, 63))
    L = api.lib()
    out = Guarded(gpu, 8, c.rows * RW, torch.int32)
    cb = Guarded(gpu, 1, c.rows * RW, torch.int32)
    pb = Guarded(gpu, 1, c.rows * c.P, torch.int32)
    x = c.d_x.data_ptr()
    E = api.SGZ_EINVAL
    #                                            frames k held flush first slices
    assert L.sgz_stage_overview_flux(c.plan.h, x, 8, 0, 0, 1, 0, 0, pb.ptr, cb.ptr, out.ptr, _stream()) == E
    assert L.sgz_stage_overview_flux(c.plan.h, x, 8, 2, 2, 1, 0, 0, pb.ptr, cb.ptr, out.ptr, _stream()) == E
    assert L.sgz_stage_overview_flux(c.plan.h, x, 8, 2, 0, 1, 0, 65, pb.ptr, cb.ptr, out.ptr, _stream()) == E
    assert L.sgz_stage_overview_flux(c.plan.h, x, 8, 2, 0, 1, 0, 0, pb.ptr, cb.ptr, None, _stream()) == E
    assert L.sgz_stage_overview_flux(c.plan.h, x, 8, 2, 1, 1, 0, 0, pb.ptr, None, out.ptr, _stream()) == E
    assert L.sgz_stage_overview_flux(c.plan.h, x, 7, 2, 0, 0, 0, 0, pb.ptr, None, out.ptr, _stream()) == E
    assert L.sgz_stage_overview_flux(c.plan.h, x, 8, 2, 0, 1, 0, 0, pb.ptr + 2, cb.ptr, out.ptr, _stream()) == E
    assert L.sgz_stage_overview_flux(c.plan.h, x, 8, 2, 0, 1, 0, 0, pb.ptr, cb.ptr + 4, out.ptr, _stream()) == E
    assert L.sgz_stage_overview_flux(c.plan.h, x, 8, 2, 0, 1, 0, 0, pb.ptr, cb.ptr, out.ptr + 4, _stream()) == E
    assert L.sgz_stage_overview_flux(c.plan.h, None, 8, 2, 0, 1, 0, 0, pb.ptr, cb.ptr, out.ptr, _stream()) == E
    # nothing arrives and nothing is held: SGZ_OK, and nothing is launched either
    assert L.sgz_stage_overview_flux(c.plan.h, x, 0, 2, 0, 1, 0, 0, pb.ptr, cb.ptr, out.ptr, _stream()) == api.SGZ_OK
    torch.cuda.synchronize()
    assert out.untouched() and cb.untouched() and pb.untouched()


def test_binding_returns_the_columns(gpu):
    import torch
    c = _case(gpu, (3, 1, 65))
    prev = torch.from_numpy(c.before.copy()).to(gpu)
    carry = torch.zeros((3, 1, 11), dtype=torch.int64, device=gpu)
    recs, held = c.plan.overview_flux_columns(c.d_x.reshape(FRAMES, 3, 1, 65), 3, flush=False, first_frame=FAR, prev=prev, carry=carry)
    want, left, _ = c.want(FRAMES, 3, 0, False, FAR, True)
    assert held == 1 and _bytes(api.flux_from_device(recs).reshape(-1, 3)) == _bytes(want)
    assert _bytes(api.flux_from_device(carry).reshape(3)) == _bytes(ofr.pack(left))
    assert _bytes(prev.cpu().numpy()) == _bytes(c.x[-1])
