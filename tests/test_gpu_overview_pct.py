"""The percentile overview on the GPU (csrc/overview_pct.hip: overviewPctColumnsKernel / SliceKernel / EmitKernel; sgz_stage_overview_pct,
sgz_spectrogram_overview_pct_device / _host).

Every comparison with the restatement (tests/overview_pct_ref.py, held to a plain sort in tests/test_overview_pct_host.py) is array_equal on
bytes or bit patterns -- records as bytes, values as uint32 views --; no tolerance anywhere:
  stage call   records, values (nq 1 and 8, q = 0 and q = 1 among them) and image == the restatement, the image == oracle.pyoracle.blend_column
               at value plane 0; every output between sentinel rows, outputs that are not due untouched; slices 0 / 1 / 5 / 64 alike (64 is more
               slices than a column has frames); a call cut at every frame position == the uncut call; one long column in the sliced form;
  the stats    count and nans of the mean overview on the same lines are this record's, the highest / lowest non-empty bucket is the bucket
               of its hi / lo;
  the image    == sgz_overview_view_host of value plane 0 at out_columns == n.  csrc/overview.hip was read first: at cols == m output column
               b folds the one source column b, a value's key turns back into its own bits (order_key.hpp) and a NaN into 0x7FC00000, the
               only NaN a value plane holds -- the view is the identity on a value plane and colours it with the same blendColour / toRgba8;
  the render   == sgz_spectrogram_render_host(lines_out) + the restatement, whatever the slab, host and device form;
  known answer a steady tone plus a loud broadband burst in one frame of ten: the median is the render's without the bursts, q = 1 shows them;
  the values   are value planes: sgz_stage_track_peaks_values on them == sgz_track_peak_values on the restated values.
The content kinds, the sentinel blocks and the render cases are those of tests/test_gpu_overview.py, imported from there."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_pct_ref as opr  # noqa: E402
import overview_ref as ov  # noqa: E402
from test_gpu_overview import BYTE, WORD, G, Guarded, _case, _content, _lines_of, _stream  # noqa: E402

pytestmark = pytest.mark.gpu

RW = 68                                                      # 32-bit words of a record
Q8 = [0.5, 0.0, 1.0, 0.1, 0.95, 0.25, 0.999, 0.5]            # unsorted, with q = 0, q = 1 and a repeat
Q1 = [0.1]
SLICES = (0, 1, 5, 64)
FRAMES_OF_K = {1: 9, 3: 10, 7: 16, 64: 70}                   # k == 64: one whole column and six frames more


def _adversarial(x, rng):
    """the content of tests/test_gpu_overview.py (NaNs, +-0, +-inf, negative and >= 1 values included) with bucket edges, their float
    neighbours, denormals and clip values scattered in"""
    x = x.copy()
    edges = (rng.integers(0, 65, 16) / 64.0).astype(np.float32)
    pool = np.concatenate([edges, np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf)),
                           np.float32([1e-45, -1e-45, 1e-39, -1e-39, -8.333333, -1000.0, 1.0, 0.99999994, 3e38, -3e38])]).astype(np.float32)
    pick = rng.random(x.shape) < 0.15
    x[pick] = rng.choice(pool, int(pick.sum()))
    return x


def _records(guarded, *shape):
    return np.ascontiguousarray(guarded.payload()).reshape(*shape, RW).view(opr.DTYPE).reshape(shape)


def _words(records):
    return np.ascontiguousarray(records, opr.DTYPE).view(np.uint32)


def _qptr(q):
    a = np.ascontiguousarray(q, np.float64)
    return a, a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("P", [2, 65, 257, 1000])
def test_stage_call_equals_the_restatement(gpu, oracle, P, pairs):
    import torch
    cfg = config.spectrum_config(window_size=64, hop=16, axis_points=P, num_pairs=pairs, bin_interp=config.INTERP_LINEAR)
    plan = api.Plan(cfg).upload()
    params = oracle.params_from_dict(cfg)
    L = api.lib()
    rng = np.random.default_rng(3000 * pairs + P)
    calls = 0
    for k, frames in FRAMES_OF_K.items():
        x = _adversarial(_content(frames, pairs, P, k % 8, rng), rng)
        other = _adversarial(_content(frames, pairs, P, (k + 3) % 8, rng), rng)
        assert P < 65 or (np.isnan(x).any() and (x < 0).any() and (x >= 1).any() and (x == np.float32(0.5)).any())
        d_lines = torch.from_numpy(_lines_of(x[:frames], rng)).to(gpu)
        for held in sorted({0, min(k - 1, 2)}):
            for flush in (0, 1):
                # the carry: the fold of `held` frames of other content (held == 0: what the call must leave alone)
                carry_in = opr.fold(opr.records_of(other[:max(held, 1)]))
                want, want_carry, left = opr.columns_of(x[:frames], k, held, carry_in, bool(flush))
                columns = want.shape[0]
                assert (columns, left) == api.overview_step(k, held, frames, flush)
                for q in (Q1, Q8):
                    nq = len(q)
                    qa, qp = _qptr(q)
                    want_v = opr.quantile_bits(want, q)
                    want_img = ov.blend(oracle, params, want_v[0])
                    for slices in SLICES:
                        calls += 1
                        mode = (calls + calls // 4) % 4                # all three / the image alone / the records alone / the values alone
                        img = Guarded(gpu, columns, P * 4, torch.uint8)
                        rc = Guarded(gpu, columns, pairs * P * RW, torch.int32)
                        vl = Guarded(gpu, nq * columns, pairs * P, torch.int32)
                        cy = Guarded(gpu, 1, pairs * P * RW, torch.int32)
                        cy.set(_words(carry_in))
                        assert rc.ptr % 16 == 0 and cy.ptr % 16 == 0
                        st = L.sgz_stage_overview_pct(plan.h, d_lines.data_ptr(), frames, k, held, flush, slices, qp, nq, cy.ptr,
                                                      img.ptr if mode in (0, 1) else None, rc.ptr if mode in (0, 2) else None,
                                                      vl.ptr if mode in (0, 3) else None, _stream())
                        assert st == api.SGZ_OK, L.sgz_last_error()
                        what = (P, pairs, frames, k, held, flush, nq, slices, mode)
                        if mode in (0, 1):
                            assert np.array_equal(img.payload().reshape(columns, P, 4), want_img), what
                        else:
                            assert img.untouched(), what
                        if mode in (0, 2):
                            assert opr.same(_records(rc, columns, pairs, P), want), what
                        else:
                            assert rc.untouched(), what
                        if mode in (0, 3):
                            assert np.array_equal(vl.payload().reshape(nq, columns, pairs, P), want_v), what
                        else:
                            assert vl.untouched(), what
                        assert opr.same(_records(cy, pairs, P), want_carry if want_carry is not None else carry_in), what
    assert calls == (1 + 2 + 2 + 2) * 2 * 2 * 4
    # the wrapper
    rgba, records, values, left = plan.overview_pct_columns(d_lines, 7, Q8, want_records=True, want_values=True)
    want, _, _ = opr.columns_of(x[:frames], 7)
    assert left == 0 and opr.same(api.pct_from_device(records), want)
    assert np.array_equal(values.cpu().numpy().view(np.uint32), opr.quantile_bits(want, Q8))
    assert np.array_equal(rgba.cpu().numpy(), ov.blend(oracle, params, opr.quantile_bits(want, Q8)[0]))


def test_a_call_cut_at_every_frame_equals_the_uncut_call(gpu, oracle):
    import torch
    P, pairs, frames = 65, 3, 10
    cfg = config.spectrum_config(window_size=64, hop=16, axis_points=P, num_pairs=pairs, bin_interp=config.INTERP_LINEAR)
    plan = api.Plan(cfg).upload()
    params = oracle.params_from_dict(cfg)
    L = api.lib()
    rng = np.random.default_rng(41)
    x = _adversarial(_content(frames, pairs, P, 1, rng), rng)[:frames]
    d_lines = torch.from_numpy(_lines_of(x, rng)).to(gpu)
    qa, qp = _qptr(Q8)
    nq = len(Q8)
    for k in (3, 4, 64):
        for flush in (0, 1):
            want, want_carry, left = opr.columns_of(x, k, 0, None, bool(flush))
            columns = want.shape[0]
            want_v = opr.quantile_bits(want, Q8)
            want_img = ov.blend(oracle, params, want_v[0]) if columns else None
            for cut in range(frames + 1):
                img = Guarded(gpu, max(columns, 1), P * 4, torch.uint8)
                rc = Guarded(gpu, max(columns, 1), pairs * P * RW, torch.int32)
                cy = Guarded(gpu, 1, pairs * P * RW, torch.int32)
                planes = [Guarded(gpu, max(columns, 1), pairs * P, torch.int32) for _ in range(nq)]
                held = done = 0
                for n, (a, b) in enumerate(((0, cut), (cut, frames))):
                    last = n == 1
                    got, held_out = api.overview_step(k, held, b - a, bool(flush and last))
                    # the values of a call are [nq][its columns]: a call writes into a block of its own, copied to where its columns belong
                    vl = Guarded(gpu, nq * max(got, 1), pairs * P, torch.int32)
                    st = L.sgz_stage_overview_pct(plan.h, d_lines.data_ptr() + a * pairs * G * P * 8, b - a, k, held, int(flush and last),
                                                  SLICES[(n + cut) % len(SLICES)], qp, nq, cy.ptr, img.ptr + done * P * 4,
                                                  rc.ptr + done * pairs * P * RW * 4, vl.ptr, _stream())
                    assert st == api.SGZ_OK, L.sgz_last_error()
                    if got:
                        v = vl.payload().reshape(nq, got, pairs * P)
                        for j in range(nq):
                            planes[j].t[(1 + done) * pairs * P:(1 + done + got) * pairs * P] = torch.from_numpy(v[j].reshape(-1).view(np.int32).copy()).to(gpu)
                    else:
                        assert vl.untouched()
                    done, held = done + got, held_out
                what = (k, flush, cut)
                assert done == columns and held == left, what
                if columns:
                    assert np.array_equal(img.payload().reshape(columns, P, 4), want_img), what
                    assert opr.same(_records(rc, columns, pairs, P), want), what
                    assert np.array_equal(np.stack([p.payload().reshape(columns, pairs, P) for p in planes]), want_v), what
                else:
                    assert img.untouched() and rc.untouched(), what
                if left:
                    assert opr.same(_records(cy, pairs, P), want_carry), what


def test_one_long_column_takes_the_sliced_form(gpu, oracle):
    """a single column of 3000 frames at P = 65: two workgroups a pair, so the library cuts the column into slices (at least 64 frames each);
    every explicit slice count gives the same bytes"""
    import torch
    P, pairs, frames = 65, 1, 3000
    cfg = config.spectrum_config(window_size=64, hop=16, axis_points=P, num_pairs=pairs, bin_interp=config.INTERP_LINEAR)
    plan = api.Plan(cfg).upload()
    params = oracle.params_from_dict(cfg)
    rng = np.random.default_rng(77)
    x = _adversarial(_content(frames, pairs, P, 0, rng), rng)[:frames]
    d_lines = torch.from_numpy(_lines_of(x, rng)).to(gpu)
    want, _, _ = opr.columns_of(x, frames)
    want_v = opr.quantile_bits(want, Q8)
    for slices in (0, 1, 7, 64):
        rgba, records, values, left = plan.overview_pct_columns(d_lines, frames, Q8, slices=slices, want_records=True, want_values=True)
        assert left == 0 and opr.same(api.pct_from_device(records), want), slices
        assert np.array_equal(values.cpu().numpy().view(np.uint32), want_v), slices
        assert np.array_equal(rgba.cpu().numpy(), ov.blend(oracle, params, want_v[0])), slices
    assert int(want["bucket"].sum(axis=-1).max()) > 2000


def test_against_the_mean_overview_on_the_same_lines(gpu):
    import torch
    P, pairs, frames = 257, 3, 40
    cfg = config.spectrum_config(window_size=64, hop=16, axis_points=P, num_pairs=pairs, bin_interp=config.INTERP_LINEAR)
    plan = api.Plan(cfg).upload()
    rng = np.random.default_rng(9)
    x = _adversarial(_content(frames, pairs, P, 2, rng), rng)[:frames]
    d_lines = torch.from_numpy(_lines_of(x, rng)).to(gpu)
    for k in (1, 7, 40):
        _, d_stats, _, _ = plan.overview_stats_columns(d_lines, k, want_rgba=False, want_stats=True)
        _, d_pct, _, _ = plan.overview_pct_columns(d_lines, k, want_rgba=False, want_records=True)
        stats, pct = api.stats_from_device(d_stats), api.pct_from_device(d_pct)
        assert np.array_equal(pct["bucket"].sum(axis=-1), stats["count"]) and np.array_equal(pct["nans"], stats["nans"]) and not pct["reserved"].any()
        some = stats["count"] > 0
        assert some.any() and (k > 1 or (~some).any())
        filled = pct["bucket"] > 0
        highest = 65 - np.argmax(filled[..., ::-1], axis=-1)
        lowest = np.argmax(filled, axis=-1)
        assert np.array_equal(highest[some], opr.bucket_of(stats["hi"])[some]) and np.array_equal(lowest[some], opr.bucket_of(stats["lo"])[some]), k


# ---- the render ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w64", "w256_two_pairs", "phase", "rsnt", "odd_hop"])
def test_pct_render_equals_render_then_restatement(gpu, name):
    import torch
    from oracle import pyoracle as po
    plan, params, x, rgba, main = _case(name)
    F = main.shape[0]
    d_x = torch.from_numpy(x).to(gpu)
    for k in sorted({1, 2, 5, 7, F, F + 3}):
        want, _, _ = opr.columns_of(main, k)
        want_v = opr.quantile_bits(want, Q8)
        image = ov.blend(po, params, want_v[0])
        for slab in (1, 5, 0):                                   # several slabs, and the default last
            plan.set_option(api.OPT_OVERVIEW_SLAB, slab)
            got_image, got, got_v = plan.overview_pct(d_x, k, Q8, want_records=True, want_values=True)
            assert opr.same(api.pct_from_device(got), want), (name, k, slab)
            assert np.array_equal(got_v.cpu().numpy().view(np.uint32), want_v), (name, k, slab)
            assert np.array_equal(got_image.cpu().numpy(), image), (name, k, slab)
            h_image, h_records, h_v, timing = plan.overview_pct(x, k, Q8, want_records=True, want_values=True)
            assert opr.same(h_records, want) and np.array_equal(h_v.view(np.uint32), want_v) and np.array_equal(h_image, image), (name, k, slab)
            assert timing["frames"] == F
    # the image is the view of value plane 0 at equal width (see the module's text)
    n = want_v.shape[1]
    view_image, _ = plan.overview_view(np.ascontiguousarray(want_v[0].view(np.float32)), n)[:2]
    assert np.array_equal(view_image, image)


def test_one_output_alone_and_short_input(gpu):
    import torch
    from oracle import pyoracle as po
    plan, params, x, rgba, main = _case("w256_two_pairs")
    L = api.lib()
    k, q = 5, [0.5, 0.9, 0.1]
    nq = len(q)
    qa, qp = _qptr(q)
    want, _, _ = opr.columns_of(main, k)
    want_v = opr.quantile_bits(want, q)
    image = ov.blend(po, params, want_v[0])
    columns, P, Cn = want.shape[0], plan.P, plan.C
    d_x = torch.from_numpy(x).to(gpu)
    S = x.shape[1]
    ptrs = (C.c_void_p * 4)(*[x[i].ctypes.data for i in range(4)])
    for only in range(3):
        img = Guarded(gpu, columns, P * 4, torch.uint8)
        rc = Guarded(gpu, columns, Cn * P * RW, torch.int32)
        vl = Guarded(gpu, nq * columns, Cn * P, torch.int32)
        st = L.sgz_spectrogram_overview_pct_device(plan.h, d_x.data_ptr(), d_x.stride(0), S, k, qp, nq, img.ptr if only == 0 else None,
                                                   rc.ptr if only == 1 else None, vl.ptr if only == 2 else None, None, _stream())
        assert st == api.SGZ_OK
        assert np.array_equal(img.payload().reshape(columns, P, 4), image) if only == 0 else img.untouched()
        assert opr.same(_records(rc, columns, Cn, P), want) if only == 1 else rc.untouched()
        assert np.array_equal(vl.payload().reshape(nq, columns, Cn, P), want_v) if only == 2 else vl.untouched()
        h_img = np.full((columns + 2, P, 4), BYTE, np.uint8)
        h_rc = np.full((columns + 2, Cn, P, RW), WORD, np.uint32)
        h_vl = np.full((nq * columns + 2, Cn, P), WORD, np.uint32)
        st = L.sgz_spectrogram_overview_pct_host(plan.h, ptrs, 4, S, k, qp, nq, h_img[1:].ctypes.data_as(C.c_void_p) if only == 0 else None,
                                                 h_rc[1:].ctypes.data_as(C.c_void_p) if only == 1 else None,
                                                 h_vl[1:].ctypes.data_as(C.c_void_p) if only == 2 else None, None)
        assert st == api.SGZ_OK
        for h, s in ((h_img, BYTE), (h_rc, WORD), (h_vl, WORD)):
            assert (h[0] == s).all() and (h[-1] == s).all()
        assert np.array_equal(h_img[1:-1], image) if only == 0 else (h_img == BYTE).all()
        assert np.array_equal(h_rc[1:-1], _words(want).reshape(columns, Cn, P, RW)) if only == 1 else (h_rc == WORD).all()
        assert np.array_equal(h_vl[1:-1].reshape(nq, columns, Cn, P), want_v) if only == 2 else (h_vl == WORD).all()
    # fewer samples than a window: skipped, nothing written
    S = plan.cfg.window_size - 1
    xs = np.ascontiguousarray(x[:, :S])
    d_xs = torch.from_numpy(xs).to(gpu)
    img = Guarded(gpu, 1, P * 4, torch.uint8)
    rc = Guarded(gpu, 1, Cn * P * RW, torch.int32)
    st = L.sgz_spectrogram_overview_pct_device(plan.h, d_xs.data_ptr(), d_xs.stride(0), S, k, qp, nq, img.ptr, rc.ptr, None, None, _stream())
    torch.cuda.synchronize()
    assert st == api.SGZ_SKIPPED_FRAME and img.untouched() and rc.untouched()
    assert plan.overview_pct(xs, k) is None and plan.overview_pct(d_xs, k) is None


# ---- known answer ------------------------------------------------------------------------------------------------------------------------------
def test_the_median_ignores_one_loud_frame_in_ten_and_q1_shows_it(gpu):
    """A steady 6 kHz tone plus, once per column of 40 frames, a loud click of 4 samples: it lies in the windows of W / hop = 4 frames, one
    frame in ten.  No decay (pole 0: a frame's line result is its own spectrum).  The pixels compared are those whose bins do not reach the
    tone, chosen on the CPU from the clean render: below the render's peak pixel by half the axis in every frame, which leaves out the tone's
    pixels and its window's skirt (53 of 64 pixels qualify with the CPU oracle's render; some of them have a median above the floor).  Over
    them the median plane's bucket is the bucket of the clean render's median, and the q = 1 plane shows the clicks: the oracle's render puts
    them 26 buckets and more above the median; 8 buckets, 15 dB, are asked for."""
    W, hop, P, k, cols = 64, 16, 64, 40, 3
    frames = k * cols
    cfg = config.spectrum_config(window_size=W, hop=hop, axis_points=P, pole=(0.0, 0.0))
    plan = api.Plan(cfg).upload()
    S = W + hop * (frames - 1)
    rng = np.random.default_rng(1)
    t = np.arange(S) / cfg["sample_rate"]
    tone = (0.25 * np.sin(2 * np.pi * 6000.0 * t)).astype(np.float32)
    clean = np.stack([tone, tone])
    loud = clean.copy()
    f = np.arange(frames)
    hit = np.zeros(frames, bool)
    for c in range(cols):
        at = (c * k + 17) * hop + 5
        loud[:, at:at + 4] += (0.9 * rng.standard_normal(4)).astype(np.float32)
        hit |= (f * hop <= at + 3) & (f * hop + W > at)
    assert (hit.reshape(cols, k).sum(axis=1) == 4).all()
    _, lines_clean, _ = api.render_spectrogram_host(plan, clean, want_lines=True)
    main_clean = np.ascontiguousarray(lines_clean[:, :, 0, :, 0])
    away = (main_clean < main_clean.max() - 0.5).all(axis=(0, 1))               # (a NaN compares false: such a pixel is left out)
    assert away.sum() >= P // 2, away.sum()
    _, _, v_loud, _ = plan.overview_pct(loud, k, [0.5, 1.0], want_rgba=False, want_values=True)
    _, _, v_clean, _ = plan.overview_pct(clean, k, [0.5, 1.0], want_rgba=False, want_values=True)
    assert v_loud.shape == (2, cols, 1, P)
    b_med_loud, b_med_clean, b_top = opr.bucket_of(v_loud[0]), opr.bucket_of(v_clean[0]), opr.bucket_of(v_loud[1])
    assert np.array_equal(b_med_loud[..., away], b_med_clean[..., away])
    assert np.array_equal(b_med_clean, opr.bucket_of(opr.quantile_bits(opr.columns_of(main_clean, k)[0], 0.5)[0].view(np.float32)))
    assert (b_top[..., away] >= b_med_loud[..., away] + 8).all(), int((b_top - b_med_loud)[..., away].min())


# ---- the values are value planes ---------------------------------------------------------------------------------------------------------------
def test_the_tracker_takes_a_value_plane(gpu):
    import torch
    plan, params, x, rgba, main = _case("w256_two_pairs")
    d_x = torch.from_numpy(x).to(gpu)
    q = [0.5, 0.9]
    k = 5
    _, _, d_values = plan.overview_pct(d_x, k, q, want_rgba=False, want_values=True)
    want = opr.quantile_bits(opr.columns_of(main, k)[0], q).view(np.float32)
    for j in range(len(q)):
        plane = d_values[j]
        assert plane.is_contiguous()
        for fraction in (0.1, 0.93):
            got = plan.track_peaks_values(plane, fraction).cpu().numpy()
            for c in range(want.shape[1]):
                for p in range(plan.C):
                    host = plan.track_peak_values(want[j, c, p], fraction)
                    row = np.array([host[name] for name, _ in api.LinePeak._fields_], np.float64)
                    assert np.array_equal(got[c, p].view(np.uint64), row.view(np.uint64)), (j, fraction, c, p)
