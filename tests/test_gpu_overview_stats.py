"""The mean overview on the GPU (csrc/overview_stats.hip: overviewStatsColumnsKernel / SliceKernel / EmitKernel and the three view kernels;
sgz_stage_overview_stats, sgz_spectrogram_overview_stats_device / _host, sgz_stage_overview_stats_view, sgz_overview_stats_view_host).

Every comparison is array_equal on bytes or bit patterns (records as bytes, means as uint32 views); no tolerance anywhere:
  stage call   records, means and image == tests/overview_stats_ref.py (checked against a brute-force loop in
               tests/test_overview_stats_host.py), the image == oracle.pyoracle.blend_column at the means; every output between sentinel rows,
               outputs that are not due untouched; hi == d_peaks of sgz_stage_overview on the same lines; any chain of calls == one call;
  the render   == sgz_spectrogram_render_host(lines_out) + the restatement, whatever the slab, host and device form;
  the view     == the restatement's fold at any range and width; kept at k == the direct call at a multiple of k; cols == m recolours;
  the means    are value planes: sgz_stage_track_peaks_values on them == sgz_track_peak_values on the restated means.
The shapes, the content kinds and the sentinel blocks are those of tests/test_gpu_overview.py, imported from there."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_ref as ov  # noqa: E402
import overview_stats_ref as osr  # noqa: E402
from test_gpu_overview import BYTE, FRAMES, SLICES, VARIANTS, WORD, G, Guarded, _case, _content, _ks, _lines_of, _stream  # noqa: E402

pytestmark = pytest.mark.gpu

RW = 6                                                       # 32-bit words of a record


def _beyond(x, rng):
    """the content of tests/test_gpu_overview.py with values at and beyond +-2048 scattered in: the quantiser's clamp"""
    x = x.copy()
    pick = rng.random(x.shape)
    x[pick < 0.04] = rng.choice(np.float32([2048.0, -2048.0, 2047.9999, -2047.9999, 5000.0, -1e30, 3e38, 2.0 ** -21, -3 * 2.0 ** -21]), int((pick < 0.04).sum()))
    return x


def _records(guarded, *shape):
    return np.ascontiguousarray(guarded.payload()).reshape(*shape, RW).view(osr.DTYPE).reshape(shape)


def _words(records):
    return np.ascontiguousarray(records, osr.DTYPE).view(np.uint32)


@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("P", [2, 65, 257, 1000])
def test_stage_call_equals_the_restatement(gpu, oracle, P, pairs):
    import torch
    cfg = config.spectrum_config(window_size=64, hop=16, axis_points=P, num_pairs=pairs, bin_interp=config.INTERP_LINEAR)
    plan = api.Plan(cfg).upload()
    params = oracle.params_from_dict(cfg)
    L = api.lib()
    rng = np.random.default_rng(2000 * pairs + P)
    calls = combo = 0
    for frames in FRAMES:
        pool = [_beyond(_content(frames, pairs, P, v, rng), rng) for v in range(VARIANTS)]
        d_lines = [torch.from_numpy(_lines_of(x[:frames], rng)).to(gpu) for x in pool]
        for k in _ks(frames):
            for held in sorted({0, 1, k - 1} & set(range(k))):
                for flush in (0, 1):
                    combo += 1
                    x = pool[combo % VARIANTS]
                    # the carry: the fold of `held` frames of another variant (held == 0: what the call must leave alone)
                    carry_in = osr.fold(osr.records_of(pool[(combo + 1) % VARIANTS][:max(held, 1)]))
                    want, want_carry, left = osr.columns_of(x[:frames], k, held, carry_in, bool(flush))
                    columns = want.shape[0]
                    assert (columns, left) == api.overview_step(k, held, frames, flush)
                    want_mean = osr.mean_bits(want)
                    want_img = ov.blend(oracle, params, want_mean)
                    # hi is V of the peak-hold overview on the same lines, carry included, bit for bit
                    pk = Guarded(gpu, columns, pairs * P, torch.int32)
                    cy = Guarded(gpu, 1, pairs * P, torch.int32)
                    cy.set(carry_in["hi"].view(np.uint32))
                    assert L.sgz_stage_overview(plan.h, d_lines[combo % VARIANTS].data_ptr(), frames, k, held, flush, 0, cy.ptr, None, pk.ptr, _stream()) == api.SGZ_OK
                    assert np.array_equal(pk.payload().reshape(columns, pairs, P), want["hi"].view(np.uint32)), (P, pairs, frames, k, held, flush)
                    for slices in SLICES:
                        calls += 1
                        mode = calls % 4                               # all three / the image alone / the records alone / the means alone
                        img = Guarded(gpu, columns, P * 4, torch.uint8)
                        st_ = Guarded(gpu, columns, pairs * P * RW, torch.int32)
                        mn = Guarded(gpu, columns, pairs * P, torch.int32)
                        cy = Guarded(gpu, 1, pairs * P * RW, torch.int32)
                        cy.set(_words(carry_in))
                        st = L.sgz_stage_overview_stats(plan.h, d_lines[combo % VARIANTS].data_ptr(), frames, k, held, flush, slices, cy.ptr,
                                                        img.ptr if mode in (0, 1) else None, st_.ptr if mode in (0, 2) else None,
                                                        mn.ptr if mode in (0, 3) else None, _stream())
                        assert st == api.SGZ_OK, L.sgz_last_error()
                        what = (P, pairs, frames, k, held, flush, slices, mode)
                        if mode in (0, 1):
                            assert np.array_equal(img.payload().reshape(columns, P, 4), want_img), what
                        else:
                            assert img.untouched(), what
                        if mode in (0, 2):
                            assert osr.same(_records(st_, columns, pairs, P), want), what
                        else:
                            assert st_.untouched(), what
                        if mode in (0, 3):
                            assert np.array_equal(mn.payload().reshape(columns, pairs, P), want_mean), what
                        else:
                            assert mn.untouched(), what
                        assert osr.same(_records(cy, pairs, P), want_carry if want_carry is not None else carry_in), what
    assert calls >= 5 * 2 * 6 * 8
    # one call == the same frames cut into 2 and into 5 chained calls at random cut points, the carry in ONE buffer throughout
    frames = FRAMES[-1]
    for k in _ks(frames):
        x = pool[k % VARIANTS]
        want, _, _ = osr.columns_of(x[:frames], k)
        want_mean = osr.mean_bits(want)
        want_img = ov.blend(oracle, params, want_mean)
        columns = want.shape[0]
        for pieces in (2, 5):
            cuts = [0] + sorted(int(c) for c in rng.integers(0, frames + 1, pieces - 1)) + [frames]
            img = Guarded(gpu, columns, P * 4, torch.uint8)
            st_ = Guarded(gpu, columns, pairs * P * RW, torch.int32)
            mn = Guarded(gpu, columns, pairs * P, torch.int32)
            cy = Guarded(gpu, 1, pairs * P * RW, torch.int32)
            held = done = 0
            for n, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                last = n == pieces - 1
                st = L.sgz_stage_overview_stats(plan.h, d_lines[k % VARIANTS].data_ptr() + a * pairs * G * P * 8, b - a, k, held, int(last),
                                                SLICES[(n + k) % len(SLICES)], cy.ptr, img.ptr + done * P * 4, st_.ptr + done * pairs * P * RW * 4,
                                                mn.ptr + done * pairs * P * 4, _stream())
                assert st == api.SGZ_OK, L.sgz_last_error()
                got, held = api.overview_step(k, held, b - a, last)
                done += got
            assert done == columns and held == 0
            assert np.array_equal(img.payload().reshape(columns, P, 4), want_img), (P, pairs, k, cuts)
            assert osr.same(_records(st_, columns, pairs, P), want), (P, pairs, k, cuts)
            assert np.array_equal(mn.payload().reshape(columns, pairs, P), want_mean), (P, pairs, k, cuts)
    # the wrapper
    rgba, stats, means, left = plan.overview_stats_columns(d_lines[0], 7, want_stats=True, want_means=True)
    want, _, _ = osr.columns_of(pool[0][:frames], 7)
    assert left == 0 and osr.same(api.stats_from_device(stats), want)
    assert np.array_equal(means.cpu().numpy().view(np.uint32), osr.mean_bits(want)) and np.array_equal(rgba.cpu().numpy(), osr.blend(oracle, params, want))


def test_k1_records_are_the_line_results(gpu):
    """k == 1: hi == lo == x bit for bit for a non-NaN x, sum == q(x), count == 1 -- and the image is the quantised value's, which need not be
    the frame render's"""
    plan, params, x, rgba, main = _case("w64")
    image, stats, means, _ = plan.overview_stats(x, 1, want_stats=True, want_means=True)
    assert osr.same(stats, osr.records_of(main))
    ok = ~np.isnan(main)
    assert np.array_equal(stats["hi"].view(np.uint32)[ok], main.view(np.uint32)[ok]) and np.array_equal(stats["lo"].view(np.uint32)[ok], main.view(np.uint32)[ok])
    assert (stats["count"][ok] == 1).all() and np.array_equal(stats["sum"], osr.quantise(main)[0])
    from oracle import pyoracle as po
    assert np.array_equal(image, osr.blend(po, params, stats)) and np.array_equal(means.view(np.uint32), osr.mean_bits(stats))


# ---- the render ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w64", "w256_two_pairs", "phase", "rsnt", "odd_hop"])
def test_stats_render_equals_render_then_restatement(gpu, name):
    import torch
    from oracle import pyoracle as po
    plan, params, x, rgba, main = _case(name)
    F = main.shape[0]
    d_x = torch.from_numpy(x).to(gpu)
    for k in sorted({1, 2, 5, 7, F, F + 3}):
        want, _, _ = osr.columns_of(main, k)
        want_mean, image = osr.mean_bits(want), osr.blend(po, params, want)
        assert np.array_equal(want["hi"].view(np.uint32), ov.columns_of(main, k)[0])
        for slab in (0, 1, 5):
            plan.set_option(api.OPT_OVERVIEW_SLAB, slab)
            got_image, got, got_mean = plan.overview_stats(d_x, k, want_stats=True, want_means=True)
            assert osr.same(api.stats_from_device(got), want), (name, k, slab)
            assert np.array_equal(got_mean.cpu().numpy().view(np.uint32), want_mean), (name, k, slab)
            assert np.array_equal(got_image.cpu().numpy(), image), (name, k, slab)
            h_image, h_stats, h_mean, timing = plan.overview_stats(x, k, want_stats=True, want_means=True)
            assert osr.same(h_stats, want) and np.array_equal(h_mean.view(np.uint32), want_mean) and np.array_equal(h_image, image), (name, k, slab)
            assert timing["frames"] == F
    plan.set_option(api.OPT_OVERVIEW_SLAB, 0)


def test_one_output_alone_and_short_input(gpu):
    import torch
    from oracle import pyoracle as po
    plan, params, x, rgba, main = _case("w256_two_pairs")
    L = api.lib()
    k = 5
    want, _, _ = osr.columns_of(main, k)
    want_mean, image = osr.mean_bits(want), osr.blend(po, params, want)
    columns, P, Cn = want.shape[0], plan.P, plan.C
    d_x = torch.from_numpy(x).to(gpu)
    S = x.shape[1]
    ptrs = (C.c_void_p * 4)(*[x[i].ctypes.data for i in range(4)])
    for only in range(3):
        img = Guarded(gpu, columns, P * 4, torch.uint8)
        st_ = Guarded(gpu, columns, Cn * P * RW, torch.int32)
        mn = Guarded(gpu, columns, Cn * P, torch.int32)
        st = L.sgz_spectrogram_overview_stats_device(plan.h, d_x.data_ptr(), d_x.stride(0), S, k, img.ptr if only == 0 else None,
                                                     st_.ptr if only == 1 else None, mn.ptr if only == 2 else None, None, _stream())
        assert st == api.SGZ_OK
        assert np.array_equal(img.payload().reshape(columns, P, 4), image) if only == 0 else img.untouched()
        assert osr.same(_records(st_, columns, Cn, P), want) if only == 1 else st_.untouched()
        assert np.array_equal(mn.payload().reshape(columns, Cn, P), want_mean) if only == 2 else mn.untouched()
        h_img = np.full((columns + 2, P, 4), BYTE, np.uint8)
        h_st = np.full((columns + 2, Cn, P, RW), WORD, np.uint32)
        h_mn = np.full((columns + 2, Cn, P), WORD, np.uint32)
        st = L.sgz_spectrogram_overview_stats_host(plan.h, ptrs, 4, S, k, h_img[1:].ctypes.data_as(C.c_void_p) if only == 0 else None,
                                                   h_st[1:].ctypes.data_as(C.c_void_p) if only == 1 else None,
                                                   h_mn[1:].ctypes.data_as(C.c_void_p) if only == 2 else None, None)
        assert st == api.SGZ_OK
        for h, s in ((h_img, BYTE), (h_st, WORD), (h_mn, WORD)):
            assert (h[0] == s).all() and (h[-1] == s).all()
        assert np.array_equal(h_img[1:-1], image) if only == 0 else (h_img == BYTE).all()
        assert np.array_equal(h_st[1:-1], _words(want).reshape(columns, Cn, P, RW)) if only == 1 else (h_st == WORD).all()
        assert np.array_equal(h_mn[1:-1], want_mean) if only == 2 else (h_mn == WORD).all()
    # fewer samples than a window: skipped, nothing written
    S = plan.cfg.window_size - 1
    xs = np.ascontiguousarray(x[:, :S])
    d_xs = torch.from_numpy(xs).to(gpu)
    img = Guarded(gpu, 1, P * 4, torch.uint8)
    st_ = Guarded(gpu, 1, Cn * P * RW, torch.int32)
    st = L.sgz_spectrogram_overview_stats_device(plan.h, d_xs.data_ptr(), d_xs.stride(0), S, k, img.ptr, st_.ptr, None, None, _stream())
    torch.cuda.synchronize()
    assert st == api.SGZ_SKIPPED_FRAME and img.untouched() and st_.untouched()
    assert plan.overview_stats(xs, k) is None and plan.overview_stats(d_xs, k) is None


# ---- the view ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairs,P", [(1, 65), (3, 257), (1, 1000), (3, 2)])
def test_view_equals_the_restatements_fold(gpu, oracle, pairs, P):
    import torch
    cfg = config.spectrum_config(window_size=64, hop=16, axis_points=P, num_pairs=pairs, bin_interp=config.INTERP_LINEAR)
    plan = api.Plan(cfg).upload()
    params = oracle.params_from_dict(cfg)
    L = api.lib()
    rng = np.random.default_rng(77 * pairs + P)
    frames, k = 80, 2
    x = _beyond(_content(frames, pairs, P, 3, rng), rng)[:frames]
    d_lines = torch.from_numpy(_lines_of(x, rng)).to(gpu)
    kept, _, _ = osr.columns_of(x, k)                                        # n = 40 kept columns of 2 frames
    n = kept.shape[0]
    _, d_kept, _, _ = plan.overview_stats_columns(d_lines, k, want_rgba=False, want_stats=True)
    assert osr.same(api.stats_from_device(d_kept), kept)
    calls = 0
    for x0, x1 in ((0, n), (0, 1), (n - 1, n), (3, 32), (7, 20), (1, n - 2)):
        m = x1 - x0
        for cols in sorted({1, 2, 3, 5, m - 1, m, m + 4} - {0}):
            want = osr.view_of(kept, x0, x1, cols)
            want_mean, want_img = osr.mean_bits(want), ov.blend(oracle, params, osr.mean_bits(want))
            c = want.shape[0]
            assert c == api.overview_view_columns(n, x0, x1, cols)
            for slices in SLICES:
                calls += 1
                mode = calls % 4
                img = Guarded(gpu, c, P * 4, torch.uint8)
                st_ = Guarded(gpu, c, pairs * P * RW, torch.int32)
                mn = Guarded(gpu, c, pairs * P, torch.int32)
                st = L.sgz_stage_overview_stats_view(plan.h, d_kept.data_ptr(), n, x0, x1, cols, slices, img.ptr if mode in (0, 1) else None,
                                                     st_.ptr if mode in (0, 2) else None, mn.ptr if mode in (0, 3) else None, _stream())
                assert st == api.SGZ_OK, L.sgz_last_error()
                what = (pairs, P, x0, x1, cols, slices, mode)
                assert np.array_equal(img.payload().reshape(c, P, 4), want_img) if mode in (0, 1) else img.untouched(), what
                assert osr.same(_records(st_, c, pairs, P), want) if mode in (0, 2) else st_.untouched(), what
                assert np.array_equal(mn.payload().reshape(c, pairs, P), want_mean) if mode in (0, 3) else mn.untouched(), what
            if cols >= m:                                                    # cols == m: a pure recolour
                assert osr.same(want, kept[x0:x1])
    # the source is left as it was
    assert osr.same(api.stats_from_device(d_kept), kept)
    # a view of records kept at k == the direct call at a multiple of k, where the boundaries coincide
    for mult in (2, 4, 5, 8, 20, 40):
        direct_img, direct, direct_mean, _ = plan.overview_stats_columns(d_lines, k * mult, want_stats=True, want_means=True)
        view_img, view, view_mean = plan.overview_stats_view(d_kept, n // mult, want_stats=True, want_means=True)
        assert torch.equal(direct, view) and torch.equal(direct_img, view_img) and torch.equal(direct_mean.view(torch.int32), view_mean.view(torch.int32)), mult
        assert osr.same(api.stats_from_device(view), osr.columns_of(x, k * mult)[0])
    # the host form and the host helper agree with it
    h_img, h_stats, h_means, timing = plan.overview_stats_view(kept, 7, 3, 32, want_stats=True, want_means=True)
    want = osr.view_of(kept, 3, 32, 7)
    assert osr.same(h_stats, want) and osr.same(api.overview_stats_fold(kept, 7, 3, 32), want) and timing["frames"] == 7
    assert np.array_equal(h_means.view(np.uint32), osr.mean_bits(want)) and np.array_equal(h_img, ov.blend(oracle, params, osr.mean_bits(want)))
    # outputs that overlap the source range are refused, and nothing is written
    column = pairs * P * 24
    before = api.stats_from_device(d_kept)
    base = d_kept.data_ptr()
    far = Guarded(gpu, 4, pairs * P * RW, torch.int32)
    for at in (base + 3 * column, base + 31 * column + column - 8, base + 10 * column + 8):
        assert L.sgz_stage_overview_stats_view(plan.h, base, n, 3, 32, 4, 0, at, None, None, _stream()) == api.SGZ_EINVAL
        assert L.sgz_stage_overview_stats_view(plan.h, base, n, 3, 32, 4, 0, None, at, None, _stream()) == api.SGZ_EINVAL
        assert L.sgz_stage_overview_stats_view(plan.h, base, n, 3, 32, 4, 0, None, far.ptr, at, _stream()) == api.SGZ_EINVAL
    assert far.untouched() and osr.same(api.stats_from_device(d_kept), before)
    # ... an output in the source array beside the range is taken: columns 0 .. 1 from the range 8 .. 40
    assert L.sgz_stage_overview_stats_view(plan.h, base, n, 8, n, 2, 0, None, base, None, _stream()) == api.SGZ_OK
    after = api.stats_from_device(d_kept)
    assert osr.same(after[:2], osr.view_of(kept, 8, n, 2)) and osr.same(after[2:], kept[2:])


# ---- the means are value planes ---------------------------------------------------------------------------------------------------------------
def test_the_tracker_takes_the_means(gpu):
    import torch
    plan, params, x, rgba, main = _case("w256_two_pairs")
    d_x = torch.from_numpy(x).to(gpu)
    for k in (1, 5):
        _, d_means = plan.overview_stats(d_x, k, want_rgba=False, want_means=True)[1:]
        want = osr.mean_bits(osr.columns_of(main, k)[0]).view(np.float32)
        for fraction in (0.1, 0.5, 0.93):
            got = plan.track_peaks_values(d_means, fraction).cpu().numpy()
            for c in range(want.shape[0]):
                for p in range(plan.C):
                    host = plan.track_peak_values(want[c, p], fraction)
                    row = np.array([host[name] for name, _ in api.LinePeak._fields_], np.float64)
                    assert np.array_equal(got[c, p].view(np.uint64), row.view(np.uint64)), (k, fraction, c, p)
