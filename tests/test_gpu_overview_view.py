"""The view of kept peaks on the GPU (csrc/overview.hip overviewViewKernel / overviewViewSliceKernel / overviewViewEmitKernel;
sgz_stage_overview_view, sgz_overview_view_host).

Every comparison is array_equal on bytes or bit patterns (uint32 views); no tolerance anywhere:
  stage call    V' == the numpy key-max of tests/overview_ref.py over the columns ceil(b m / cols) <= j - x0 < ceil((b + 1) m / cols), which
                this file states itself in Python integers; the image == oracle.pyoracle.blend_column of V'; every output between
                sentinels, an output that is not asked for untouched; the host call == the stage call;
  composition   the view of peaks kept at k = 2 (the restatement of sgz_spectrogram_render_host's line results) at n / g columns == the
                overview render at k g, image and peaks, wherever the column boundaries coincide; a view of a view == the direct view
                where the boundaries nest;
  recolour      peaks of plan A viewed at cols == m through plan B (other colours and ratios) == plan B's own overview image."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_ref as ov  # noqa: E402
from test_gpu_overview import BYTE, WORD, Guarded, _content  # noqa: E402  (the sentinel blocks and the contents of the overview's own test)

pytestmark = pytest.mark.gpu


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def bounds_of(x0, x1, out_columns):
    """the definition's column boundaries, in Python integers: (cols, [x0 + ceil(b m / cols) for b = 0 .. cols])"""
    m = x1 - x0
    cols = min(out_columns, m)
    return cols, [x0 + -((-b * m) // cols) for b in range(cols + 1)]


def view_ref(v, x0, x1, out_columns, keys=None):
    """V' bits uint32 [cols][pairs][P] of float32 v [n][pairs][P] (keys: ov.order_key of all of v, where the caller has them already)"""
    cols, bounds = bounds_of(x0, x1, out_columns)
    keys = ov.order_key(v).reshape(v.shape) if keys is None else keys
    return ov.key_value(np.maximum.reduceat(keys[x0:x1], np.array(bounds[:-1]) - x0, axis=0))


# ---- stage call ----------------------------------------------------------------------------------------------------------------------------
NS = (1, 2, 7, 8, 9, 40, 1000)
SLICES = (0, 1, 2, 5, 64)


def _ranges(n):
    """whole, x0 > 0, x1 < n, a single column (inside where there is an inside)"""
    return sorted({(0, n), (min(3, n - 1), n), (0, max(1, n - 3)), (n // 2, n // 2 + 1)})


def _outs(m):
    return sorted({1, 2, 3, 7, max(1, m - 1), m, m + 1, 5000})


@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("P", [2, 63, 64, 65, 255, 256, 257, 1000])
def test_stage_call_equals_the_restatement(gpu, oracle, P, pairs):
    import torch
    cfg = config.spectrum_config(window_size=64, hop=16, axis_points=P, num_pairs=pairs, bin_interp=config.INTERP_LINEAR)
    plan = api.Plan(cfg).upload()
    params = oracle.params_from_dict(cfg)
    L = api.lib()
    rng = np.random.default_rng(2000 * pairs + P)
    calls = 0
    for number, n in enumerate(NS):
        v = _content(n - 1, pairs, P, number, rng)                  # float32 [n][pairs][P]: every kind of trace, by (pixel + pair + number) % 8
        assert v.shape == (n, pairs, P)
        if n >= 9 and P >= 8:                                       # (every kind of trace is there: the quiet NaN itself and a NaN with a payload)
            assert (v.view(np.uint32) == 0x7FC00000).any() and (v.view(np.uint32) == 0xFFC00123).any()
        keys = ov.order_key(v).reshape(v.shape)
        src = Guarded(gpu, n, pairs * P, torch.int32)
        src.set(v.view(np.uint32))
        for x0, x1 in _ranges(n):
            m = x1 - x0
            for out_columns in _outs(m):
                cols, bounds = bounds_of(x0, x1, out_columns)
                assert cols == api.overview_view_columns(n, x0, x1, out_columns)
                want_v = view_ref(v, x0, x1, out_columns, keys)
                want_img = ov.blend(oracle, params, want_v)
                for slices in SLICES:
                    calls += 1
                    mode = calls % 3                               # image and peaks / image alone / peaks alone
                    img = Guarded(gpu, cols, P * 4, torch.uint8)
                    pk = Guarded(gpu, cols, pairs * P, torch.int32)
                    st = L.sgz_stage_overview_view(plan.h, src.ptr, n, x0, x1, out_columns, slices, img.ptr if mode != 2 else None,
                                                   pk.ptr if mode != 1 else None, _stream())
                    assert st == api.SGZ_OK, api.lib().sgz_last_error()
                    what = (P, pairs, n, x0, x1, out_columns, slices, mode)
                    if mode != 2:
                        assert np.array_equal(img.payload().reshape(cols, P, 4), want_img), what
                    else:
                        assert img.untouched(), what
                    if mode != 1:
                        assert np.array_equal(pk.payload().reshape(cols, pairs, P), want_v), what
                    else:
                        assert pk.untouched(), what
                # the host call: only the range is uploaded; between sentinel rows on the host
                mode = calls % 3
                h_img = np.full((cols + 2, P, 4), BYTE, np.uint8)
                h_pk = np.full((cols + 2, pairs, P), WORD, np.uint32)
                st = L.sgz_overview_view_host(plan.h, v.ctypes.data_as(C.c_void_p), n, x0, x1, out_columns,
                                              h_img[1:].ctypes.data_as(C.c_void_p) if mode != 2 else None,
                                              h_pk[1:].ctypes.data_as(C.c_void_p) if mode != 1 else None, None)
                assert st == api.SGZ_OK, api.lib().sgz_last_error()
                assert (h_img[0] == BYTE).all() and (h_img[-1] == BYTE).all() and (h_pk[0] == WORD).all() and (h_pk[-1] == WORD).all()
                assert np.array_equal(h_img[1:-1], want_img) if mode != 2 else (h_img == BYTE).all(), (P, pairs, n, x0, x1, out_columns)
                assert np.array_equal(h_pk[1:-1], want_v) if mode != 1 else (h_pk == WORD).all(), (P, pairs, n, x0, x1, out_columns)
        assert np.array_equal(src.payload().reshape(n, pairs, P), v.view(np.uint32))          # the source and its sentinels as they were
    assert calls >= 5 * 7 * 8
    # an output that overlaps the source columns it is made from is refused, and nothing is written
    before = src.payload().copy()
    assert L.sgz_stage_overview_view(plan.h, src.ptr, n, 2, n, 4, 0, None, src.ptr + (n - 1) * pairs * P * 4, _stream()) == api.SGZ_EINVAL
    assert np.array_equal(src.payload(), before)
    # the wrappers
    rgba, peaks = plan.overview_view(src.t[pairs * P:pairs * P * (n + 1)].view(torch.float32).view(n, pairs, P), 7, x0=1, want_peaks=True)
    want_v = view_ref(v, 1, n, 7)
    assert np.array_equal(peaks.cpu().numpy().view(np.uint32), want_v) and np.array_equal(rgba.cpu().numpy(), ov.blend(oracle, params, want_v))
    h_rgba, h_peaks, timing = plan.overview_view(v, 7, x0=1, want_peaks=True)
    assert np.array_equal(h_peaks.view(np.uint32), want_v) and np.array_equal(h_rgba, rgba.cpu().numpy()) and timing["frames"] == 7


# ---- composition ---------------------------------------------------------------------------------------------------------------------------
LANES = {
    "w64": dict(window_size=64, hop=16, axis_points=33, pole=(0.3, 0.3)),
    "w256_two_pairs": dict(window_size=256, hop=64, axis_points=100, num_pairs=2, pole=(0.5, 0.5)),
    "phase": dict(window_size=256, hop=64, axis_points=100, channel_mode=config.CH_PHASE, pole=(0.3, 0.3)),
}
K0 = 2
_lanes = {}


def _lane(name, frames, **over):
    """(plan, planar, the k = 2 peaks float32 [n][pairs][P] restated from sgz_spectrogram_render_host's line results) -- made once"""
    key = (name, frames, tuple(sorted(over)))
    if key not in _lanes:
        cfg = config.spectrum_config(**dict(LANES[name], **over))
        plan = api.Plan(cfg).upload()
        x = ov.burst_signal(cfg["window_size"], cfg["hop"], frames, 2 * cfg["num_pairs"], cfg["sample_rate"], seed=5)
        assert plan.num_frames(x.shape[1]) == frames
        rgba, lines, _ = api.render_spectrogram_host(plan, x, want_lines=True)
        bits, _, _ = ov.columns_of(np.ascontiguousarray(lines[:, :, 0, :, 0]), K0)
        peaks = bits.view(np.float32)
        peaks.setflags(write=False)
        _lanes[key] = (plan, x, peaks)
    return _lanes[key]


# the columns of the view at ceil(n / g) columns whose source range is that of the direct overview's column of the same index, where n is
# no multiple of g (n = 13 fine columns; at a multiple, n = 12, every column coincides)
COINCIDE_13 = {2: [0, 1, 2, 3, 4, 5, 6], 3: [0, 1], 4: [0]}


@pytest.mark.parametrize("name", list(LANES))
def test_the_view_of_fine_peaks_is_the_coarser_overview(gpu, name):
    import torch
    for frames in (23, 25):                                        # 12 and 13 columns at k = 2, the last of one frame
        plan, x, fine = _lane(name, frames)
        n = fine.shape[0]
        assert n == -(-frames // K0)
        d_fine = torch.from_numpy(fine.copy()).to(gpu)
        for g in (2, 3, 4):
            image, peaks, _ = plan.overview(x, K0 * g, want_peaks=True)                 # the direct render: column c covers fine columns c g ..
            cols = -(-n // g)
            assert image.shape[0] == cols
            _, bounds = bounds_of(0, n, cols)
            same = [b for b in range(cols) if (bounds[b], bounds[b + 1]) == (b * g, min((b + 1) * g, n))]
            assert same == (list(range(cols)) if n % g == 0 else COINCIDE_13[g]), (name, frames, g, bounds, same)
            for slices in (0, 1, 3):
                got_image, got_peaks = plan.overview_view(d_fine, cols, slices=slices, want_peaks=True)
                assert np.array_equal(got_peaks.cpu().numpy().view(np.uint32)[same], peaks.view(np.uint32)[same]), (name, frames, g, slices)
                assert np.array_equal(got_image.cpu().numpy()[same], image[same]), (name, frames, g, slices)
            h_image, h_peaks, _ = plan.overview_view(fine, cols, want_peaks=True)
            assert np.array_equal(h_peaks.view(np.uint32)[same], peaks.view(np.uint32)[same]) and np.array_equal(h_image[same], image[same]), (name, frames, g)
            # a range that starts and ends on the coarse grid: fine columns [g, g (cols - 1)) are the direct columns 1 .. cols - 2
            if cols >= 3:
                got_image, got_peaks = plan.overview_view(d_fine, cols - 2, x0=g, x1=g * (cols - 1), want_peaks=True)
                assert np.array_equal(got_peaks.cpu().numpy().view(np.uint32), peaks.view(np.uint32)[1:cols - 1]), (name, frames, g)
                assert np.array_equal(got_image.cpu().numpy(), image[1:cols - 1]), (name, frames, g)


@pytest.mark.parametrize("name", list(LANES))
def test_a_view_of_a_view_is_the_direct_view_where_the_boundaries_nest(gpu, name):
    import torch
    nested = 0
    for frames, first, second in ((23, 6, 3), (23, 4, 2), (23, 12, 5), (25, 7, 4), (25, 13, 13), (25, 4, 2)):
        plan, x, fine = _lane(name, frames)
        n = fine.shape[0]
        d_fine = torch.from_numpy(fine.copy()).to(gpu)
        _, b1 = bounds_of(0, n, first)
        _, b2 = bounds_of(0, first, second)
        through = [b1[j] for j in b2]                               # the second view's boundaries in fine columns
        _, direct = bounds_of(0, n, second)
        same = [b for b in range(second) if (through[b], through[b + 1]) == (direct[b], direct[b + 1])]
        assert same, (frames, first, second, through, direct)
        nested += same == list(range(second))
        _, mid = plan.overview_view(d_fine, first, want_rgba=False, want_peaks=True)
        image2, peaks2 = plan.overview_view(mid, second, want_peaks=True)
        image1, peaks1 = plan.overview_view(d_fine, second, want_peaks=True)
        assert np.array_equal(peaks2.cpu().numpy().view(np.uint32)[same], peaks1.cpu().numpy().view(np.uint32)[same]), (name, frames, first, second)
        assert np.array_equal(image2.cpu().numpy()[same], image1.cpu().numpy()[same]), (name, frames, first, second)
    assert nested == 5                                              # (all but 13 -> 7 -> 4, of which column 0 alone coincides)


@pytest.mark.parametrize("name", list(LANES))
def test_recolour_through_another_plan(gpu, name):
    import torch
    other = dict(colours=[(0, 0, 0), (64, 0, 64), (255, 0, 128), (255, 128, 0), (255, 255, 255), (0, 255, 255)], ratios=(0.1, 0.3, 0.15, 0.25, 0.2))
    plan_a, x, _ = _lane(name, 23)
    plan_b, _, _ = _lane(name, 23, **other)
    for k in (1, 2, 5):
        image_a, peaks_a, _ = plan_a.overview(x, k, want_peaks=True)
        image_b, peaks_b, _ = plan_b.overview(x, k, want_peaks=True)
        assert np.array_equal(peaks_a.view(np.uint32), peaks_b.view(np.uint32)) and not np.array_equal(image_a, image_b), (name, k)
        m = peaks_a.shape[0]
        got, none = plan_b.overview_view(torch.from_numpy(peaks_a).to(gpu), m)
        assert none is None and np.array_equal(got.cpu().numpy(), image_b), (name, k)
        got, none, _ = plan_b.overview_view(peaks_a, m + 5)                              # (more columns than the range has: cols == m)
        assert none is None and np.array_equal(got, image_b), (name, k)
        back, _ = plan_a.overview_view(torch.from_numpy(peaks_a).to(gpu), m)
        assert np.array_equal(back.cpu().numpy(), image_a), (name, k)


# ---- also ----------------------------------------------------------------------------------------------------------------------------------
def test_the_view_is_the_same_beside_a_background_render(gpu):
    import torch
    from test_gpu_concurrency import BackgroundLoad
    lanes = [_lane(name, 25) for name in LANES]
    want = []
    for plan, x, fine in lanes:
        d_fine = torch.from_numpy(fine.copy()).to(gpu)
        want.append((d_fine, [tuple(t.cpu().numpy() for t in plan.overview_view(d_fine, cols, slices=s, want_peaks=True)) for cols, s in ((5, 0), (13, 1), (2, 7))]))
    with BackgroundLoad(gpu) as load:
        beside = 0
        for _ in range(400):                                         # (the load's threads build their plans first: go on until three rounds ran beside it)
            busy = load.renders > 0
            for (plan, x, fine), (d_fine, outs) in zip(lanes, want):
                for (cols, s), (image, peaks) in zip(((5, 0), (13, 1), (2, 7)), outs):
                    got_image, got_peaks = plan.overview_view(d_fine, cols, slices=s, want_peaks=True)
                    assert np.array_equal(got_image.cpu().numpy(), image) and np.array_equal(got_peaks.cpu().numpy().view(np.uint32), peaks.view(np.uint32))
                    h_image, h_peaks, _ = plan.overview_view(fine, cols, want_peaks=True)
                    assert np.array_equal(h_image, image) and np.array_equal(h_peaks.view(np.uint32), peaks.view(np.uint32))
            beside += busy
            if beside >= 3 or load.errors:
                break
        assert beside >= 3, (beside, load.errors)


def test_a_hundred_view_calls_do_not_grow_device_memory(gpu):
    import torch
    plan, x, fine = _lane("w256_two_pairs", 25)
    n = fine.shape[0]
    d_fine = torch.from_numpy(fine.copy()).to(gpu)

    def calls(count):
        for i in range(count):
            if i % 2:
                plan.overview_view(fine, 1 + i % n, x0=i % 3, want_rgba=bool(i % 4 == 1), want_peaks=True)
            else:
                out = plan.overview_view(d_fine, 1 + i % n, slices=(0, 1, 5, 64)[i % 4], want_peaks=bool(i % 3))
                del out
        gc.collect(); torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    free0 = calls(12)
    free1 = calls(100)
    assert free0 - free1 < 2 << 20, f"device memory: {(free0 - free1) / 2**20:.1f} MiB fewer free after 100 view calls"
