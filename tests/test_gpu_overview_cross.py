"""The cross overview's stage call on the GPU (csrc/overview_cross.hip: overviewCrossTileKernel / overviewCrossEmitKernel behind
sgz_stage_overview_cross, with the band tables of sgz_plan_set_cross_edges).

Bytes only, no tolerance: every comparison is an equality of 64-bit words, made on the device against the uploaded restatement
(tests/overview_cross_ref.py, held to exact rational arithmetic in tests/test_overview_cross_host.py).
  records      == the restatement on crafted complex bins for every k, held / flush, slice count and band table; every output between
               sentinel rows, an output that is not due untouched, the carry as documented;
  cuts         every cut of the frames into two and three calls == one call;
  bands        a coarse-band call == the band fold of a fine-band call (the restatement's and sgz_overview_cross_fold's);
  refusals     launch nothing.
Plans: Phase mode, window = N.  N = 64 (30 admitted bins, below one wave), 1024 (510 bins, past one 256-thread block), 8192 (4094 bins,
sixteen tiles), pairs 1 and 2, at most 40 frames (fewer at the larger N: every column rule is met by 9 frames already).
Bins: seeded values over nine decades up to the clamp; the host test's edge values down the bins 2 ..; a bin that is non-finite every third
frame; bins 10 .. 12 non-finite in the first seven frames, so that their bands are skipped in a whole column.
Band tables: every bin its own band; one band of all bins; octave thirds; a table with empty bands that starts past bin 1 and ends before
N/2 - 1; edges at every multiple of 64 and at those +- 1 (N >= 1024: there is no multiple of 64 among the bins of N = 64); seeded random tables."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_cross_ref as ocr  # noqa: E402
from test_gpu_overview import _stream  # noqa: E402
from test_overview_cross_host import edge_bins  # noqa: E402

pytestmark = pytest.mark.gpu

RW = 10                                                      # 64-bit words of a record
SENTINEL = 0x5A5A5A5A5A5A5A5A
SHAPES = [(N, pairs) for N in (64, 1024, 8192) for pairs in (1, 2)]
FRAMES = {64: 40, 1024: 20, 8192: 9}
KS = (1, 2, 3, 7, 64)
SLICES = (0, 1, 2, 3, 64)
SKIPPED_BINS = (10, 11, 12)                                  # non-finite in frames 0 .. 6
THIRD_BIN = 7                                                # non-finite every third frame


def _cfg(N, pairs):
    return config.spectrum_config(window_size=N, hop=N // 4, axis_points=33, num_pairs=pairs, channel_mode=config.CH_PHASE,
                                  bin_interp=config.INTERP_LINEAR)


def make_bins(N, pairs, frames, seed):
    """float32 [frames][pairs][N + 1][2]"""
    rng = np.random.default_rng(seed)
    shape = (frames, pairs, N + 1, 2)
    x = ((N / 2) * 10.0 ** rng.uniform(-8, 0.6, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    lr, li, rr, ri = edge_bins()
    for i in range(lr.size):                                 # the edge values down bins 2 .., pair 0 (past the crafted bins at N = 64: bins 13 ..)
        f, k = i % frames, 2 + i // frames
        if k >= THIRD_BIN:
            k += 13 - THIRD_BIN
        assert k <= N // 2 - 2
        x[f, 0, k] = (lr[i], li[i])
        x[f, 0, N - k] = (rr[i], ri[i])
    x[::3, 0, THIRD_BIN, 0] = np.nan
    for j, k in enumerate(SKIPPED_BINS):
        x[:7, 0, k if j % 2 == 0 else N - k, j % 2] = (np.nan, np.inf, -np.inf)[j]
    return x


def tables_of(N):
    half = N // 2
    rng = np.random.default_rng(N)
    t = {"bins": list(range(1, half)), "one": [1, half - 1],
         "thirds": [int(e) for e in api.cross_edges_octave(48000.0, N, 3, 20.0, 20000.0)[0]],
         "empty": [3, 3, 5, 9, 9, 9, max(9, N // 4), half - 3, half - 3]}
    if N >= 1024:
        t["64"] = sorted({e for m in range(0, half, 64) for e in (m - 1, m, m + 1) if 1 <= e <= half - 1})
    for i in range(2):
        t[f"random{i}"] = sorted(int(e) for e in rng.integers(1, half, int(rng.integers(2, min(60, half)))))
    return t


class Guarded:
    """a device block of `rows` rows of `width` int64 words between two sentinel rows; the checks stay on the device"""

    def __init__(self, gpu, rows, width):
        import torch
        self.t = torch.full((rows + 2, width), SENTINEL, dtype=torch.int64, device=gpu)
        self.ptr = self.t.data_ptr() + width * 8

    def set(self, words):
        self.t[1:-1] = words.reshape(self.t.shape[0] - 2, -1)

    def holds(self, want=None):
        """a device bool: the sentinel rows are whole and the rows between equal `want` (None: they are untouched)"""
        body = self.t[1:-1]
        inner = (body == SENTINEL).all() if want is None else (body == want.reshape(body.shape)).all()
        return (self.t[0] == SENTINEL).all() & (self.t[-1] == SENTINEL).all() & inner


def to_device(records, gpu):
    import torch
    r = np.ascontiguousarray(records, ocr.DTYPE)
    return torch.from_numpy(r.view(np.int64).reshape(-1, RW).copy()).to(gpu)


class Case:
    """one plan, its bins on the device, and per band table the records of every single frame"""

    def __init__(self, gpu, N, pairs):
        import torch
        self.N, self.pairs, self.frames = N, pairs, FRAMES[N]
        self.plan = api.Plan(_cfg(N, pairs)).upload()
        assert (self.plan.C, self.plan.N) == (pairs, N)
        self.x = make_bins(N, pairs, self.frames, 100 * pairs + N)
        self.d_x = torch.from_numpy(self.x).to(gpu)
        self.other = make_bins(N, pairs, max(KS), 7)          # what the carries are folded from
        self.tables = tables_of(N)
        self._each = {}

    def each(self, name):
        if name not in self._each:
            self._each[name] = (ocr.records_of(self.x, self.N, self.tables[name]), ocr.records_of(self.other, self.N, self.tables[name]))
        return self._each[name]


_cases = {}


def _case(gpu, shape):
    if shape not in _cases:
        _cases[shape] = Case(gpu, *shape)
    return _cases[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stage_call_equals_the_restatement(gpu, shape):
    import torch
    c = _case(gpu, shape)
    N, pairs = shape
    L = api.lib()
    calls = 0
    for name, edges in c.tables.items():
        c.plan.set_cross_edges(edges)
        B = len(edges) - 1
        each, other = c.each(name)
        width = pairs * B * RW
        for frames in (1, c.frames):
            for k in KS:
                for held in sorted({0, 1, k - 1} & set(range(k))):
                    carry_in = ocr.fold(other[:max(held, 1)])
                    d_carry_in = to_device(carry_in, gpu)
                    for flush in (0, 1):
                        want, want_carry, left = ocr.columns_of(each[:frames], k, held, carry_in, bool(flush))
                        columns = want.shape[0]
                        assert (columns, left) == api.overview_step(k, held, frames, flush)
                        d_want = to_device(want, gpu) if columns else None
                        d_want_carry = to_device(want_carry, gpu) if want_carry is not None else d_carry_in
                        flags = []
                        for slices in SLICES:
                            out = Guarded(gpu, max(columns, 1), width)
                            cy = Guarded(gpu, 1, width)
                            cy.set(d_carry_in)
                            st = L.sgz_stage_overview_cross(c.plan.h, c.d_x.data_ptr(), frames, k, held, flush, slices, cy.ptr, out.ptr, _stream())
                            assert st == api.SGZ_OK, L.sgz_last_error()
                            flags += [out.holds(d_want), cy.holds(d_want_carry)]
                            calls += 1
                        assert bool(torch.stack(flags).all()), (shape, name, frames, k, held, flush, [bool(f) for f in flags])
    assert calls == len(c.tables) * 2 * 12 * 2 * 5            # 12 (k, held) pairs: one at k = 1, two at k = 2, three at each other k
    # the crafted bins did what they are there for: at k = 7 with every bin its own band, column 0 of the skipped bins is empty
    c.plan.set_cross_edges(c.tables["bins"])
    want = ocr.columns_of(c.each("bins")[0], 7)[0]
    for k in SKIPPED_BINS:
        assert int(want["count"][0, 0, k - 1]) == 0 and int(want["skipped"][0, 0, k - 1]) == 7 and not want["ll"][0, 0, k - 1].any()
    assert int(want["skipped"][0, 0, THIRD_BIN - 1]) == 3 and int(want["count"][0, 0, THIRD_BIN - 1]) == 4
    assert int(want["skipped"].sum()) > 3 * 7 + 3                            # ... and the edge values' non-finite bins
    assert any(int(v) >= 2 ** 63 for v in ocr.sums(want, "ll").reshape(-1))  # sums that pass one word
    assert any(int(v) < 0 for v in ocr.sums(want, "re").reshape(-1)) and any(int(v) < 0 for v in ocr.sums(want, "im").reshape(-1))
    # the wrapper
    got, left = c.plan.overview_cross_columns(c.d_x, 7)
    assert left == 0 and ocr.same(api.cross_from_device(got), want)
    one = ocr.columns_of(c.each("one")[0], 7)[0]
    assert ocr.same(ocr.bands_of(want, c.tables["bins"], c.tables["one"]), one)


def test_every_cut_into_two_and_three_calls_equals_one_call(gpu):
    """10 frames of the (1024, 2) plan under the table of the multiples of 64: every 0 <= a <= b <= 10 as calls over [0, a), [a, b), [b, 10)
    with the carry in ONE buffer -- empty pieces, held && open && columns > 1, a flush of a held column with frames == 0 and a partial last
    column are all among them"""
    import torch
    shape = (1024, 2)
    c = _case(gpu, shape)
    N, pairs = shape
    L = api.lib()
    frames = 10
    edges = c.tables["64"]
    c.plan.set_cross_edges(edges)
    B = len(edges) - 1
    width = pairs * B * RW
    per_frame = pairs * (N + 1) * 8                          # bytes of a frame's bins
    each = c.each("64")[0][:frames]
    seen = set()
    for k in KS:
        want = ocr.columns_of(each, k)[0]
        columns = want.shape[0]
        d_want = to_device(want, gpu)
        flags = []
        for a in range(frames + 1):
            for b in range(a, frames + 1):
                cuts = [0, a, b, frames] if a != b else [0, a, frames]                               # two calls where the middle piece is empty
                if a == b == frames:
                    cuts = [0, frames, frames]                                                       # everything, then a flush without frames
                out = Guarded(gpu, columns, width)
                cy = torch.zeros((width,), dtype=torch.int64, device=gpu)
                held = done = 0
                for n, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
                    last = n == len(cuts) - 2
                    got, left = api.overview_step(k, held, hi - lo, last)
                    if held and left and not last and got >= 1:
                        seen.add("snapshot")
                    if last and hi == lo and held:
                        seen.add("flush without frames")
                    st = L.sgz_stage_overview_cross(c.plan.h, c.d_x.data_ptr() + lo * per_frame, hi - lo, k, held, int(last),
                                                    SLICES[(n + a + b) % len(SLICES)], cy.data_ptr(), out.ptr + done * width * 8, _stream())
                    assert st == api.SGZ_OK, L.sgz_last_error()
                    held, done = left, done + got
                assert done == columns and held == 0
                if frames % k:
                    seen.add("partial last column")
                flags.append(out.holds(d_want))
        assert bool(torch.stack(flags).all()), (k, [i for i, f in enumerate(flags) if not bool(f)])
    assert seen == {"snapshot", "flush without frames", "partial last column"}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_coarse_band_call_equals_the_band_fold_of_a_fine_band_call(gpu, shape):
    c = _case(gpu, shape)
    fine_edges = c.tables["bins"]
    c.plan.set_cross_edges(fine_edges)
    fine, _ = c.plan.overview_cross_columns(c.d_x, 3)
    fine = api.cross_from_device(fine)
    assert ocr.same(fine, ocr.columns_of(c.each("bins")[0], 3)[0])
    for name, edges in c.tables.items():
        c.plan.set_cross_edges(edges)
        got, _ = c.plan.overview_cross_columns(c.d_x, 3)
        got = api.cross_from_device(got)
        assert ocr.same(got, ocr.bands_of(fine, fine_edges, edges)), (shape, name)
        assert ocr.same(got, api.overview_cross_fold(fine, fine.shape[0], edges=fine_edges, coarse_edges=edges)), (shape, name)
        # ... and over columns as well: k = 6 is the fold of pairs of k = 3 columns wherever the boundaries coincide
        wide, _ = c.plan.overview_cross_columns(c.d_x[:6 * (c.frames // 6)], 6)
        n = 2 * (c.frames // 6)
        assert ocr.same(api.cross_from_device(wide), api.overview_cross_fold(fine[:n], n // 2, edges=fine_edges, coarse_edges=edges)), (shape, name)


def test_the_refusals_launch_nothing(gpu):
    import torch
    shape = (64, 2)
    c = _case(gpu, shape)
    N, pairs = shape
    L = api.lib()
    edges = c.tables["thirds"]
    c.plan.set_cross_edges(edges)
    width = pairs * (len(edges) - 1) * RW
    out, cy = Guarded(gpu, 4, width), Guarded(gpu, 1, width)
    x = c.d_x.data_ptr()
    E = api.SGZ_EINVAL
    for args in ((x, 8, 0, 0, 1, 0, cy.ptr, out.ptr), (x, 8, 2, 2, 1, 0, cy.ptr, out.ptr), (x, 8, 2, 3, 1, 0, cy.ptr, out.ptr),
                 (x, 8, 2, 0, 1, 65, cy.ptr, out.ptr), (None, 8, 2, 0, 1, 0, cy.ptr, out.ptr), (x, 8, 2, 0, 1, 0, cy.ptr, None),
                 (x, 8, 2, 1, 1, 0, None, out.ptr), (x, 7, 2, 0, 0, 0, None, out.ptr)):
        assert L.sgz_stage_overview_cross(c.plan.h, *args, _stream()) == E, args
    # a table that breaks the rule is refused and the old table stays
    bad = np.array([1, 9, 4, 31], np.uint32)
    assert L.sgz_plan_set_cross_edges(c.plan.h, bad.ctypes.data, 3) == E
    assert c.plan.overview_cross_columns(c.d_x, 7)[0].shape[2] == len(edges) - 1
    # nothing arrives and no column to flush: SGZ_OK, nothing written
    assert L.sgz_stage_overview_cross(c.plan.h, x, 0, 2, 0, 1, 0, cy.ptr, out.ptr, _stream()) == api.SGZ_OK
    assert L.sgz_stage_overview_cross(c.plan.h, x, 0, 2, 1, 0, 0, cy.ptr, out.ptr, _stream()) == api.SGZ_OK
    # a plan of another mode, and a Phase plan without a table
    other = api.Plan(config.spectrum_config(window_size=N, hop=N // 4, axis_points=33, num_pairs=pairs, channel_mode=config.CH_SEPARATE,
                                            bin_interp=config.INTERP_LINEAR)).upload()
    assert L.sgz_stage_overview_cross(other.h, x, 8, 2, 0, 1, 0, cy.ptr, out.ptr, _stream()) == api.SGZ_EUNSUPPORTED
    bare = api.Plan(_cfg(N, pairs)).upload()
    assert L.sgz_stage_overview_cross(bare.h, x, 8, 2, 0, 1, 0, cy.ptr, out.ptr, _stream()) == E
    torch.cuda.synchronize()
    assert bool(out.holds()) and bool(cy.holds())
