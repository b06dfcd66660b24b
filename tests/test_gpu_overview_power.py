"""The power overview's stage calls on the GPU (csrc/overview_power.hip: overviewPowerColumnsKernel / SliceKernel / EmitKernel and the three view
kernels; sgz_stage_overview_power, sgz_stage_overview_power_view, sgz_overview_power_view_host).

Every comparison is array_equal on bytes or bit patterns (records as bytes, levels as uint32 views); no tolerance anywhere:
  records      == tests/overview_power_ref.py (checked against exact rational arithmetic in tests/test_overview_power_host.py) on crafted and
               seeded mapped values, for every k, held / flush, slice count and combination of outputs; every output between sentinel rows,
               outputs that are not due untouched; every cut of the frames into two and three calls == one call;
  levels, image   held to EXISTING code: sgz_stage_decay_colour on a one-frame buffer of the expected rms values from a zero state gives the
               expected level (its graph-0 line result .x; side 1 by swapping the planes) and the expected image, column by column.  In the
               combinatorial loops the levels are held to the host helper sgz_overview_power_levels (itself held to the oracle's dB map in the
               host test) and the image to oracle.pyoracle.blend_column at side 0's levels;
  the view     == the restatement's fold at any range and width; cols == m recolours; a view of a view == the direct view where the
               boundaries nest; overlap is refused.
Shapes: (pairs, sides, P) in {(1, 1, 33), (2, 2, 33), (1, 2, 300)} at window 64, hop 16 -- 33 values are below one wave, 2 * 300 pass one
256-thread block; at most 70 frames."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_ref as ov  # noqa: E402
import overview_power_ref as opr  # noqa: E402
from test_gpu_overview import Guarded, _stream  # noqa: E402

pytestmark = pytest.mark.gpu

RW = 8                                                       # 32-bit words of a record
QNAN = 0x7FC00000
SHAPES = [(1, 1, 33), (2, 2, 33), (1, 2, 300)]
KS = (1, 2, 3, 7, 64, 100)
SLICES = (0, 1, 2, 3, 64)
FRAMES = 70
MODES = [(i, p, l) for i in (1, 0) for p in (1, 0) for l in (1, 0)][:-1]     # every allowed combination of (image, records, levels)


def _f(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


EDGE = np.array([0.0, -0.0, _f(1), _f(0x80000001), _f(0x007FFFFF), _f(0x00800000), 2.0 ** -31, 2.0 ** -30, 2.0 ** -7, 1.0, _f(0x407FFFFF), 4.0,
                 1e30, np.inf, -np.inf, _f(0x7FC12345), _f(0xFFC00001), -1.0, -2.0 ** -30, -_f(0x407FFFFF), -4.0, -0.75, 3.0 * 2.0 ** -31,
                 1.5 * 2.0 ** -30], np.float32)               # the host test's edge values


def _cfg(pairs, sides, P):
    return config.spectrum_config(window_size=64, hop=16, axis_points=P, num_pairs=pairs,
                                  channel_mode=config.CH_SEPARATE if sides == 2 else config.CH_LEFT, bin_interp=config.INTERP_LINEAR)


def _mapped(pairs, sides, P, seed, frames=FRAMES):
    """float32 [frames][pairs][sides][P]: seeded magnitudes over nine decades, with crafted rows at the first pixels of (pair 0, side 0) --
    pixel 0 the edge values in turn, pixel 1 NaN in the first 14 frames (count == 0 in the columns they fill), pixel 2 the value 2.0 (five
    frames carry into sum[1]), pixel 3 a NaN every third frame -- and the edge values scattered over the last pair and side"""
    rng = np.random.default_rng(seed)
    x = (10.0 ** rng.uniform(-8, 0.6, (frames, pairs, sides, P))).astype(np.float32)
    x[:, 0, 0, 0] = EDGE[np.arange(frames) % EDGE.size]
    x[:14, 0, 0, 1] = np.nan
    x[:, 0, 0, 2] = 2.0
    x[::3, 0, 0, 3] = _f(0xFFC00001)
    pick = rng.random((frames, P)) < 0.05
    pick[:, :4] = False                                      # (the crafted pixels stay as they are where the last pair and side are the first)
    x[:, -1, -1][pick] = rng.choice(EDGE, int(pick.sum()))
    return x


class Case:
    """one plan, its mapped values on the device and their one-frame records"""

    def __init__(self, gpu, oracle, pairs, sides, P):
        import torch
        self.cfg = _cfg(pairs, sides, P)
        self.plan = api.Plan(self.cfg).upload()
        assert (self.plan.C, self.plan.sides, self.plan.P) == (pairs, sides, P)
        self.params = oracle.params_from_dict(self.cfg)
        self.oracle = oracle
        self.x = _mapped(pairs, sides, P, 100 * pairs + 10 * sides + P)
        self.each = opr.records_of(self.x)
        self.d_x = torch.from_numpy(self.x).to(gpu)
        self.width = pairs * sides * P

    def levels_of(self, records):
        return self.plan.overview_power_levels(records).view(np.uint32)

    def image_of(self, level_bits):
        return ov.blend(self.oracle, self.params, np.ascontiguousarray(level_bits[:, :, 0, :]))


_cases = {}


def _case(gpu, oracle, shape):
    if shape not in _cases:
        _cases[shape] = Case(gpu, oracle, *shape)
    return _cases[shape]


def _records(guarded, *shape):
    return np.ascontiguousarray(guarded.payload()).reshape(*shape, RW).view(opr.DTYPE).reshape(shape)


def _words(records):
    return np.ascontiguousarray(records, opr.DTYPE).view(np.uint32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stage_call_equals_the_restatement(gpu, oracle, shape):
    import torch
    c = _case(gpu, oracle, shape)
    pairs, sides, P = shape
    L = api.lib()
    other = opr.records_of(_mapped(pairs, sides, P, 7, frames=max(KS)))       # what the carries are folded from
    calls = 0
    for frames in (1, 8, 9, FRAMES):
        for k in KS:
            for held in sorted({0, 1, k - 1} & set(range(k))):
                carry_in = opr.fold(other[:max(held, 1)])
                for flush in (0, 1):
                    want, want_carry, left = opr.columns_of(c.x[:frames], k, held, carry_in, bool(flush), each=c.each[:frames])
                    columns = want.shape[0]
                    assert (columns, left) == api.overview_step(k, held, frames, flush)
                    want_lv = c.levels_of(want) if columns else np.zeros((0, pairs, sides, P), np.uint32)
                    want_img = c.image_of(want_lv)
                    for slices in SLICES:
                        mode = MODES[calls % len(MODES)]
                        calls += 1
                        img = Guarded(gpu, columns, P * 4, torch.uint8)
                        pw = Guarded(gpu, columns, c.width * RW, torch.int32)
                        lv = Guarded(gpu, columns, c.width, torch.int32)
                        cy = Guarded(gpu, 1, c.width * RW, torch.int32)
                        cy.set(_words(carry_in))
                        st = L.sgz_stage_overview_power(c.plan.h, c.d_x.data_ptr(), frames, k, held, flush, slices, cy.ptr, img.ptr if mode[0] else None,
                                                        pw.ptr if mode[1] else None, lv.ptr if mode[2] else None, _stream())
                        assert st == api.SGZ_OK, L.sgz_last_error()
                        what = (shape, frames, k, held, flush, slices, mode)
                        assert np.array_equal(img.payload().reshape(columns, P, 4), want_img) if mode[0] else img.untouched(), what
                        assert opr.same(_records(pw, columns, pairs, sides, P), want) if mode[1] else pw.untouched(), what
                        assert np.array_equal(lv.payload().reshape(columns, pairs, sides, P), want_lv) if mode[2] else lv.untouched(), what
                        assert opr.same(_records(cy, pairs, sides, P), want_carry if want_carry is not None else carry_in), what
    assert calls >= 4 * 6 * 2 * 2 * 5
    # the crafted rows did what they are there for, at k = 7: empty records, a sum in the high word, the clamp
    want = opr.columns_of(c.x, 7, each=c.each)[0]
    assert (want["count"][:2, 0, 0, 1] == 0).all() and (want["nans"][:2, 0, 0, 1] == 7).all() and int(want["count"][2, 0, 0, 1]) == 7
    assert [int(w) for w in want["sum"][0, 0, 0, 2]] == [3 * 2 ** 62, 1]
    assert int(opr.sums(want)[1, 0, 0, 0]) >= 3 * opr.Q_MOST
    # the wrapper
    rgba, power, levels, left = c.plan.overview_power_columns(c.d_x, 7, want_power=True, want_levels=True)
    assert left == 0 and opr.same(api.power_from_device(power), want)
    assert np.array_equal(levels.cpu().numpy().view(np.uint32), c.levels_of(want))
    assert np.array_equal(rgba.cpu().numpy(), c.image_of(c.levels_of(want)))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_levels_and_image_equal_k_b_on_one_frame_of_the_rms_values(gpu, oracle, shape):
    """for each emitted column: sgz_stage_decay_colour (existing code) on a one-frame buffer of the expected rms values, zero state"""
    import torch
    c = _case(gpu, oracle, shape)
    pairs, sides, P = shape
    checked = images = 0
    for k in KS:
        want = opr.columns_of(c.x, k, each=c.each)[0]
        rms = opr.rms_bits(want).view(np.float32)
        rgba, power, levels, _ = c.plan.overview_power_columns(c.d_x, k, want_power=True, want_levels=True)
        assert opr.same(api.power_from_device(power), want)
        got_lv, got_img = levels.cpu().numpy().view(np.uint32), rgba.cpu().numpy()
        for col in range(want.shape[0]):
            empty = want["count"][col] == 0
            assert (got_lv[col][empty] == QNAN).all()
            frame = np.where(empty, np.float32(0), rms[col])[None]                                   # [1][pairs][sides][P]
            image, lines = c.plan.stage_decay_colour(torch.from_numpy(np.ascontiguousarray(frame)).to(gpu), want_lines=True)
            side0 = lines.cpu().numpy()[0, :, 0, :, 0]
            assert np.array_equal(got_lv[col, :, 0][~empty[:, 0]], side0.view(np.uint32)[~empty[:, 0]]), (shape, k, col)
            if sides == 2:
                swapped = np.ascontiguousarray(frame[:, :, ::-1])
                _, lines = c.plan.stage_decay_colour(torch.from_numpy(swapped).to(gpu), want_lines=True, want_rgba=False)
                side1 = lines.cpu().numpy()[0, :, 0, :, 0]
                assert np.array_equal(got_lv[col, :, 1][~empty[:, 1]], side1.view(np.uint32)[~empty[:, 1]]), (shape, k, col)
            checked += 1
            if not empty.any():                                                                      # columns without an empty record
                assert np.array_equal(got_img[col], image.cpu().numpy()[0]), (shape, k, col)
                images += 1
    assert checked == sum(-(-FRAMES // k) for k in KS) and images >= 40


def test_every_cut_into_two_and_three_calls_equals_one_call(gpu, oracle):
    """10 frames of the (2, 2, 33) plan: every 0 <= a <= b <= 10 as calls over [0, a), [a, b), [b, 10) with the carry in ONE buffer -- empty
    pieces, held && open && columns > 1, a flush of a held column with frames == 0 and a partial last column are all among them"""
    import torch
    shape = (2, 2, 33)
    c = _case(gpu, oracle, shape)
    pairs, sides, P = shape
    L = api.lib()
    frames = 10
    seen = set()
    for k in KS:
        want = opr.columns_of(c.x[:frames], k, each=c.each[:frames])[0]
        columns = want.shape[0]
        want_lv = c.levels_of(want)
        want_img = c.image_of(want_lv)
        for a in range(frames + 1):
            for b in range(a, frames + 1):
                cuts = [0, a, b, frames] if a != b else [0, a, frames]                               # two calls where the middle piece is empty
                if a == b == frames:
                    cuts = [0, frames, frames]                                                       # everything, then a flush without frames
                img = torch.zeros((columns, P, 4), dtype=torch.uint8, device=gpu)
                pw = torch.zeros((columns, c.width, RW), dtype=torch.int32, device=gpu)
                lv = torch.zeros((columns, c.width), dtype=torch.int32, device=gpu)
                cy = torch.zeros((c.width, RW), dtype=torch.int32, device=gpu)
                held = done = 0
                for n, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
                    last = n == len(cuts) - 2
                    got, left = api.overview_step(k, held, hi - lo, last)
                    if held and left and not last and got >= 1:
                        seen.add("snapshot")
                    if last and hi == lo and held:
                        seen.add("flush without frames")
                    st = L.sgz_stage_overview_power(c.plan.h, c.d_x.data_ptr() + lo * c.width * 4, hi - lo, k, held, int(last), SLICES[(n + a + b) % len(SLICES)],
                                                    cy.data_ptr(), img.data_ptr() + done * P * 4, pw.data_ptr() + done * c.width * RW * 4,
                                                    lv.data_ptr() + done * c.width * 4, _stream())
                    assert st == api.SGZ_OK, L.sgz_last_error()
                    held, done = left, done + got
                assert done == columns and held == 0
                if frames % k:
                    seen.add("partial last column")
                what = (k, cuts)
                assert opr.same(pw.cpu().numpy().view(np.uint32).reshape(columns, pairs, sides, P, RW).view(opr.DTYPE).reshape(columns, pairs, sides, P), want), what
                assert np.array_equal(lv.cpu().numpy().view(np.uint32).reshape(columns, pairs, sides, P), want_lv), what
                assert np.array_equal(img.cpu().numpy(), want_img), what
    assert seen == {"snapshot", "flush without frames", "partial last column"}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_view_equals_the_restatements_fold(gpu, oracle, shape):
    import torch
    c = _case(gpu, oracle, shape)
    pairs, sides, P = shape
    L = api.lib()
    frames, k = 64, 2
    kept = opr.columns_of(c.x[:frames], k, each=c.each[:frames])[0]           # n = 32 kept columns of 2 frames
    n = kept.shape[0]
    _, d_kept, _, _ = c.plan.overview_power_columns(c.d_x[:frames], k, want_rgba=False, want_power=True)
    assert opr.same(api.power_from_device(d_kept), kept)
    calls = 0
    for x0, x1 in ((0, n), (0, 1), (n - 1, n), (3, 30), (7, 20), (1, n - 2)):
        m = x1 - x0
        for cols in sorted({1, 2, 3, 5, m - 1, m, m + 4} - {0}):
            want = opr.view_of(kept, x0, x1, cols)
            want_lv = c.levels_of(want)
            want_img = c.image_of(want_lv)
            nc = want.shape[0]
            assert nc == api.overview_view_columns(n, x0, x1, cols)
            for slices in SLICES:
                mode = MODES[calls % len(MODES)]
                calls += 1
                img = Guarded(gpu, nc, P * 4, torch.uint8)
                pw = Guarded(gpu, nc, c.width * RW, torch.int32)
                lv = Guarded(gpu, nc, c.width, torch.int32)
                st = L.sgz_stage_overview_power_view(c.plan.h, d_kept.data_ptr(), n, x0, x1, cols, slices, img.ptr if mode[0] else None,
                                                     pw.ptr if mode[1] else None, lv.ptr if mode[2] else None, _stream())
                assert st == api.SGZ_OK, L.sgz_last_error()
                what = (shape, x0, x1, cols, slices, mode)
                assert np.array_equal(img.payload().reshape(nc, P, 4), want_img) if mode[0] else img.untouched(), what
                assert opr.same(_records(pw, nc, pairs, sides, P), want) if mode[1] else pw.untouched(), what
                assert np.array_equal(lv.payload().reshape(nc, pairs, sides, P), want_lv) if mode[2] else lv.untouched(), what
            if cols >= m:                                                    # cols == m: a pure recolour
                assert opr.same(want, kept[x0:x1])
    # the source is left as it was
    assert opr.same(api.power_from_device(d_kept), kept)
    # a view of records kept at k == the direct call at a multiple of k, and a view of a view == the direct view, where the boundaries nest
    _, mid, _ = c.plan.overview_power_view(d_kept, 16, want_rgba=False, want_power=True)
    for mult in (2, 4, 8, 16, 32):
        direct_img, direct, direct_lv, _ = c.plan.overview_power_columns(c.d_x[:frames], k * mult, want_power=True, want_levels=True)
        view_img, view, view_lv = c.plan.overview_power_view(d_kept, n // mult, want_power=True, want_levels=True)
        assert torch.equal(direct, view) and torch.equal(direct_img, view_img) and torch.equal(direct_lv.view(torch.int32), view_lv.view(torch.int32)), mult
        assert opr.same(api.power_from_device(view), opr.columns_of(c.x[:frames], k * mult, each=c.each[:frames])[0])
        again_img, again, again_lv = c.plan.overview_power_view(mid, n // mult, want_power=True, want_levels=True)
        assert torch.equal(again, view) and torch.equal(again_img, view_img) and torch.equal(again_lv.view(torch.int32), view_lv.view(torch.int32)), mult
    # the host form and the host helper agree with it
    h_img, h_power, h_lv, timing = c.plan.overview_power_view(kept, 7, 3, 30, want_power=True, want_levels=True)
    want = opr.view_of(kept, 3, 30, 7)
    assert opr.same(h_power, want) and opr.same(api.overview_power_fold(kept, 7, 3, 30), want) and timing["frames"] == 7
    assert np.array_equal(h_lv.view(np.uint32), c.levels_of(want)) and np.array_equal(h_img, c.image_of(c.levels_of(want)))
    # outputs that overlap the source range are refused, and nothing is written
    column = c.width * 32
    before = api.power_from_device(d_kept)
    base = d_kept.data_ptr()
    far = Guarded(gpu, 4, c.width * RW, torch.int32)
    for at in (base + 3 * column, base + 29 * column + column - 8, base + 10 * column + 8):
        assert L.sgz_stage_overview_power_view(c.plan.h, base, n, 3, 30, 4, 0, at, None, None, _stream()) == api.SGZ_EINVAL
        assert L.sgz_stage_overview_power_view(c.plan.h, base, n, 3, 30, 4, 0, None, at, None, _stream()) == api.SGZ_EINVAL
        assert L.sgz_stage_overview_power_view(c.plan.h, base, n, 3, 30, 4, 0, None, far.ptr, at, _stream()) == api.SGZ_EINVAL
    torch.cuda.synchronize()
    assert far.untouched() and opr.same(api.power_from_device(d_kept), before)
    # ... an output in the source array beside the range is taken: columns 0 .. 1 from the range 8 .. 32
    assert L.sgz_stage_overview_power_view(c.plan.h, base, n, 8, n, 2, 0, None, base, None, _stream()) == api.SGZ_OK
    after = api.power_from_device(d_kept)
    assert opr.same(after[:2], opr.view_of(kept, 8, n, 2)) and opr.same(after[2:], kept[2:])
