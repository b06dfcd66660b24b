"""The overview render on the GPU (csrc/overview.hip overviewColumnsKernel / overviewSliceKernel / overviewEmitKernel; sgz_stage_overview,
sgz_spectrogram_overview_device / _host).

Every comparison is array_equal on bytes or bit patterns (uint32 views: a NaN equals a NaN when the bits agree); no tolerance anywhere:
  stage call   V == the numpy key-max of tests/overview_ref.py (checked on hand-made groups in tests/test_overview_host.py), the image ==
               oracle.pyoracle.blend_column of V; every output between sentinels, outputs that are not due untouched;
  k == 1       the image == sgz_spectrogram_render_host's image, V == that render's line results (graph 0, first component);
  the render   == sgz_spectrogram_render_host(lines_out) + the restatement, whatever the slab.
(The issue lists P = 1 among the stage call's sizes; a plan needs axis_points >= 2 -- TransformConstant.h:127 --, so that size is
checked to be refused where a plan is made, and P = 2 is the smallest the kernels can see.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_ref as ov  # noqa: E402

pytestmark = pytest.mark.gpu

G = api.NUM_GRAPHS
SPLIT, SIDE_MAP = 8, 4                                       # SGZ_PATH_* (sgz.h)
BYTE, WORD = 0x5A, 0x5A5AA5A5                                # sentinels: image bytes, float words


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """a device block of `rows` rows of `width` elements between two sentinel rows"""

    def __init__(self, gpu, rows, width, dtype):
        import torch
        self.rows, self.width, self.byte = rows, width, dtype == torch.uint8
        fill = BYTE if self.byte else np.array([WORD], np.uint32).view(np.int32)[0]
        self.t = torch.full(((rows + 2) * width,), int(fill), dtype=torch.uint8 if self.byte else torch.int32, device=gpu)
        self.ptr = self.t.data_ptr() + width * (1 if self.byte else 4)

    def set(self, bits):
        import torch
        self.t[self.width:self.width * (self.rows + 1)] = torch.from_numpy(np.ascontiguousarray(bits, np.uint32).view(np.int32).reshape(-1)).to(self.t.device)

    def payload(self):
        h = self.t.cpu().numpy()
        h = h if self.byte else h.view(np.uint32)
        h = h.reshape(self.rows + 2, self.width)
        s = BYTE if self.byte else WORD
        assert (h[0] == s).all() and (h[-1] == s).all(), "a sentinel row was written"
        return h[1:-1]

    def untouched(self):
        s = BYTE if self.byte else WORD
        return bool((self.payload() == s).all())


# ---- stage call ----------------------------------------------------------------------------------------------------------------------------
FRAMES = (1, 2, 7, 8, 9, 40)
SLICES = (0, 1, 2, 5, 64)
VARIANTS = 8


def _content(frames, pairs, P, variant, rng):
    """float32 [frames + 1][pairs][P] (the extra row is a carry): the kind of a (pair, pixel) trace is (pixel + pair + variant) % 8 --
    random in the colour range / NaN scattered / NaN in whole groups / +-0 / +-inf / below 0 (the pair contributes nothing) / >= 0.999
    (the last colour) / constant"""
    n = frames + 1
    shape = (n, pairs, P)
    nan_b = np.array([0xFFC00123], np.uint32).view(np.float32)[0]               # a negative NaN with a payload

    def rnd():
        return rng.random(shape).astype(np.float32)

    def put(r, fraction, value):
        r[rng.random(shape) < fraction] = value
        return r

    kinds = [rnd(), put(put(rnd(), 0.3, np.float32(np.nan)), 0.1, nan_b), rnd(),
             np.where(rng.random(shape) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32),
             put(put(rnd(), 0.3, np.float32(np.inf)), 0.4, np.float32(-np.inf)),
             put((-2 * rnd()).astype(np.float32), 0.2, np.float32(-0.0)),
             put(put((np.float32(0.999) + rnd() * np.float32(0.5)).astype(np.float32), 0.3, np.float32(0.999)), 0.2, np.float32(0.99899995)),
             np.full(shape, 0.5, np.float32)]
    kinds[2][:min(9, n)] = np.nan                                 # whole columns of NaN for every k <= 9
    kinds[2][n // 2:n // 2 + 3] = np.nan
    kind = (np.arange(P)[None, :] + np.arange(pairs)[:, None] + variant) % VARIANTS
    x = np.empty(shape, np.float32)
    for j in range(VARIANTS):
        x[:, kind == j] = kinds[j][:, kind == j]
    return x


def _lines_of(x, rng):
    """[frames][pairs][G][P][2] with x as graph 0's first components and noise (NaNs included) everywhere else"""
    frames, pairs, P = x.shape
    lines = rng.standard_normal((frames, pairs, G, P, 2)).astype(np.float32)
    lines[rng.random(lines.shape) < 0.05] = np.nan
    lines[:, :, 0, :, 0] = x
    return lines


def _ks(frames):
    return sorted({1, 2, 3, 7, 8, 9, frames, frames + 1, 1000})


def test_a_plan_needs_two_axis_points():
    with pytest.raises(api.SgzError):
        api.Plan(config.spectrum_config(window_size=64, hop=16, axis_points=1))


@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("P", [2, 63, 64, 65, 255, 256, 257, 1000])
def test_stage_call_equals_the_restatement(gpu, oracle, P, pairs):
    import torch
    cfg = config.spectrum_config(window_size=64, hop=16, axis_points=P, num_pairs=pairs, bin_interp=config.INTERP_LINEAR)
    plan = api.Plan(cfg).upload()
    params = oracle.params_from_dict(cfg)
    L = api.lib()
    rng = np.random.default_rng(1000 * pairs + P)
    calls = combo = 0
    for frames in FRAMES:
        pool = [_content(frames, pairs, P, v, rng) for v in range(VARIANTS)]
        d_lines = [torch.from_numpy(_lines_of(x[:frames], rng)).to(gpu) for x in pool]
        for k in _ks(frames):
            for held in sorted({0, 1, k - 1} & set(range(k))):
                for flush in (0, 1):
                    combo += 1
                    x = pool[combo % VARIANTS]
                    carry_in = x[frames].view(np.uint32)
                    want_v, want_carry, left = ov.columns_of(x[:frames], k, held, carry_in, bool(flush))
                    columns = want_v.shape[0]
                    assert (columns, left) == api.overview_step(k, held, frames, flush)
                    want_img = ov.blend(oracle, params, want_v)
                    for slices in SLICES:
                        calls += 1
                        mode = calls % 3                               # image and peaks / image alone / peaks alone
                        img = Guarded(gpu, columns, P * 4, torch.uint8)
                        pk = Guarded(gpu, columns, pairs * P, torch.int32)
                        cy = Guarded(gpu, 1, pairs * P, torch.int32)
                        cy.set(carry_in)
                        st = L.sgz_stage_overview(plan.h, d_lines[combo % VARIANTS].data_ptr(), frames, k, held, flush, slices, cy.ptr,
                                                  img.ptr if mode != 2 else None, pk.ptr if mode != 1 else None, _stream())
                        assert st == api.SGZ_OK, api.lib().sgz_last_error()
                        what = (P, pairs, frames, k, held, flush, slices, mode)
                        if mode != 2:
                            assert np.array_equal(img.payload().reshape(columns, P, 4), want_img), what
                        else:
                            assert img.untouched(), what
                        if mode != 1:
                            assert np.array_equal(pk.payload().reshape(columns, pairs, P), want_v), what
                        else:
                            assert pk.untouched(), what
                        after = cy.payload().reshape(pairs, P)
                        assert np.array_equal(after, want_carry if want_carry is not None else carry_in.reshape(pairs, P)), what
    assert calls >= 5 * 2 * 6 * 8
    # one call == the same frames cut into 2 and into 5 chained calls at random cut points, the carry in ONE buffer throughout
    frames = FRAMES[-1]
    for k in _ks(frames):
        x = pool[k % VARIANTS]
        want_v, _, _ = ov.columns_of(x[:frames], k)
        want_img = ov.blend(oracle, params, want_v)
        columns = want_v.shape[0]
        for pieces in (2, 5):
            cuts = [0] + sorted(int(c) for c in rng.integers(0, frames + 1, pieces - 1)) + [frames]
            img = Guarded(gpu, columns, P * 4, torch.uint8)
            pk = Guarded(gpu, columns, pairs * P, torch.int32)
            cy = Guarded(gpu, 1, pairs * P, torch.int32)
            held = done = 0
            for n, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                last = n == pieces - 1
                st = L.sgz_stage_overview(plan.h, d_lines[k % VARIANTS].data_ptr() + a * pairs * G * P * 8, b - a, k, held, int(last),
                                          SLICES[(n + k) % len(SLICES)], cy.ptr, img.ptr + done * P * 4, pk.ptr + done * pairs * P * 4, _stream())
                assert st == api.SGZ_OK, api.lib().sgz_last_error()
                got, held = api.overview_step(k, held, b - a, last)
                done += got
            assert done == columns and held == 0
            assert np.array_equal(img.payload().reshape(columns, P, 4), want_img), (P, pairs, k, cuts)
            assert np.array_equal(pk.payload().reshape(columns, pairs, P), want_v), (P, pairs, k, cuts)
    # the wrapper
    rgba, peaks, left = plan.overview_columns(d_lines[0], 7, want_peaks=True)
    want_v, _, _ = ov.columns_of(pool[0][:frames], 7)
    assert left == 0 and np.array_equal(peaks.cpu().numpy().view(np.uint32), want_v)
    assert np.array_equal(rgba.cpu().numpy(), ov.blend(oracle, params, want_v))


# ---- the render ------------------------------------------------------------------------------------------------------------------------------
RENDER_CASES = {
    "w64": dict(cfg=dict(window_size=64, hop=16, axis_points=33, pole=(0.3, 0.3)), frames=23, bursts=True),
    "w256_two_pairs": dict(cfg=dict(window_size=256, hop=64, axis_points=100, num_pairs=2, pole=(0.5, 0.5)), frames=23, bursts=True),
    "n4096_two_pairs": dict(cfg=dict(window_size=4096, hop=1024, num_pairs=2, pole=(0.5, 0.5)), frames=23),
    "phase": dict(cfg=dict(window_size=256, hop=64, axis_points=100, channel_mode=config.CH_PHASE, pole=(0.3, 0.3)), frames=23),
    "complex": dict(cfg=dict(window_size=1024, hop=256, axis_points=200, channel_mode=config.CH_COMPLEX, pole=(0.5, 0.5)), frames=23),
    "n32768_split": dict(cfg=dict(window_size=32768, hop=8192, pole=(0.3, 0.3)), frames=12, path=SPLIT),
    "rsnt": dict(cfg=dict(algorithm=config.ALGO_RSNT, window_size=1024, hop=256, axis_points=128, pole=(0.5, 0.5)), frames=23),
    "odd_hop": dict(cfg=dict(window_size=1024, hop=333, axis_points=100, pole=(0.3, 0.3)), frames=10),
}
SLABS = (0, 1, 3, 8)
_refs = {}


def _case(name):
    """(plan, oracle params, planar, the parent's render: image and graph 0's first components [F][C][P]) -- rendered once and shared"""
    if name not in _refs:
        from oracle import pyoracle as po
        case = RENDER_CASES[name]
        cfg = config.spectrum_config(**case["cfg"])
        plan = api.Plan(cfg).upload()
        if "path" in case:
            assert plan.path & case["path"], (name, plan.path)
        frames, rsnt = case["frames"], cfg["algorithm"] == config.ALGO_RSNT
        x = ov.burst_signal(cfg["hop"] if rsnt else cfg["window_size"], cfg["hop"], frames, 2 * cfg["num_pairs"], cfg["sample_rate"], seed=5)
        assert plan.num_frames(x.shape[1]) == frames
        rgba, lines, _ = api.render_spectrogram_host(plan, x, want_lines=True)
        _refs[name] = (plan, po.params_from_dict(cfg), x, rgba, np.ascontiguousarray(lines[:, :, 0, :, 0]))
    return _refs[name]


def _want(name, k):
    from oracle import pyoracle as po
    plan, params, x, rgba, main = _case(name)
    v, _, _ = ov.columns_of(main, k)
    return v, ov.blend(po, params, v)


@pytest.mark.parametrize("mode", list(range(8)))
def test_k1_is_the_render_in_every_channel_mode(gpu, mode):
    cfg = config.spectrum_config(window_size=64, hop=16, axis_points=33, channel_mode=mode)
    plan = api.Plan(cfg).upload()
    x = synth.gen(90 + mode, 48000, 64 + 16 * 22, 2)
    rgba, lines, _ = api.render_spectrogram_host(plan, x, want_lines=True)
    for slab in (0, 5):
        plan.set_option(api.OPT_OVERVIEW_SLAB, slab)
        image, peaks, timing = plan.overview(x, 1, want_peaks=True)
        assert image.tobytes() == rgba.tobytes(), (mode, slab)
        assert np.array_equal(peaks.view(np.uint32), np.ascontiguousarray(lines[:, :, 0, :, 0]).view(np.uint32)), (mode, slab)
        assert timing["frames"] == 23


def test_k1_is_the_render_for_rsnt(gpu):
    plan, params, x, rgba, main = _case("rsnt")
    image, peaks, _ = plan.overview(x, 1, want_peaks=True)
    assert image.tobytes() == rgba.tobytes() and np.array_equal(peaks.view(np.uint32), main.view(np.uint32))


@pytest.mark.parametrize("name", ["w64", "w256_two_pairs"])
def test_the_burst_signals_cannot_pass_by_copying_a_frame(gpu, name):
    """the two conditions that make the render test mean something: inside a column the arg-max frame varies over the pixels, and at least
    one column differs from every single frame's column of its group"""
    plan, params, x, rgba, main = _case(name)
    F = main.shape[0]
    for k in (2, 5, 7):
        v, image = _want(name, k)
        varies = differs = 0
        for c in range(v.shape[0]):
            group = list(range(c * k, min((c + 1) * k, F)))
            arg = np.argmax(ov.order_key(main[group]).reshape(len(group), -1), axis=0)
            varies += len(set(arg.tolist())) > 1
            differs += all(not np.array_equal(image[c], rgba[f]) for f in group)
        assert varies >= 1 and differs >= 1, (name, k, varies, differs)


@pytest.mark.parametrize("name", ["w64", "w256_two_pairs", "n4096_two_pairs", "phase", "complex", "n32768_split", "rsnt", "odd_hop"])
def test_overview_render_equals_render_then_restatement(gpu, name):
    import torch
    plan, params, x, rgba, main = _case(name)
    F = main.shape[0]
    d_x = torch.from_numpy(x).to(gpu)
    for k in sorted({1, 2, 5, 7, F, F + 3}):
        v, image = _want(name, k)
        for slab in SLABS:
            plan.set_option(api.OPT_OVERVIEW_SLAB, slab)
            got_image, got_v = plan.overview(d_x, k, want_peaks=True)
            assert np.array_equal(got_v.cpu().numpy().view(np.uint32), v), (name, k, slab)
            assert np.array_equal(got_image.cpu().numpy(), image), (name, k, slab)
        h_image, h_v, timing = plan.overview(x, k, want_peaks=True)                     # the host form, at the last slab
        assert np.array_equal(h_v.view(np.uint32), v) and np.array_equal(h_image, image) and timing["frames"] == F, (name, k)
    plan.set_option(api.OPT_OVERVIEW_SLAB, 0)


@pytest.mark.parametrize("name", ["w64", "w256_two_pairs", "phase"])
def test_two_halves_with_carried_state_equal_the_whole(gpu, name):
    """cut at a multiple of k hop: the columns of the halves are the whole's, and the state out is the render's state out"""
    import torch
    plan, params, x, rgba, main = _case(name)
    cfg, F = plan.cfg, main.shape[0]
    W, hop = cfg.window_size, cfg.hop
    d_x = torch.from_numpy(x).to(gpu)
    state = torch.zeros((plan.C, G, plan.P, 2), dtype=torch.float32, device=gpu)
    plan.render(d_x, state=state)
    torch.cuda.synchronize()
    want_state = state.cpu().numpy().view(np.uint32).copy()
    for k, slab in ((2, 0), (5, 3), (3, 8)):
        plan.set_option(api.OPT_OVERVIEW_SLAB, slab)
        v, image = _want(name, k)
        h = k * ((F // 2) // k)
        state.zero_()
        whole_image, whole_v = plan.overview(d_x, k, want_peaks=True, state=state)
        assert np.array_equal(whole_v.cpu().numpy().view(np.uint32), v) and np.array_equal(whole_image.cpu().numpy(), image), (name, k)
        assert np.array_equal(state.cpu().numpy().view(np.uint32), want_state), (name, k)
        state.zero_()
        a_image, a_v = plan.overview(d_x[:, :W + hop * (h - 1)].contiguous(), k, want_peaks=True, state=state)
        b_image, b_v = plan.overview(d_x[:, hop * h:].contiguous(), k, want_peaks=True, state=state)
        assert np.array_equal(torch.cat([a_v, b_v]).cpu().numpy().view(np.uint32), v), (name, k)
        assert np.array_equal(torch.cat([a_image, b_image]).cpu().numpy(), image), (name, k)
        assert np.array_equal(state.cpu().numpy().view(np.uint32), want_state), (name, k)
    plan.set_option(api.OPT_OVERVIEW_SLAB, 0)


def test_peaks_alone_image_alone_and_short_input(gpu):
    import torch
    plan, params, x, rgba, main = _case("w256_two_pairs")
    L = api.lib()
    k = 5
    v, image = _want("w256_two_pairs", k)
    columns, P, Cn = v.shape[0], plan.P, plan.C
    d_x = torch.from_numpy(x).to(gpu)
    S = x.shape[1]
    ptrs = (C.c_void_p * 4)(*[x[i].ctypes.data for i in range(4)])
    for want_image, want_peaks in ((True, False), (False, True)):
        img = Guarded(gpu, columns, P * 4, torch.uint8)
        pk = Guarded(gpu, columns, Cn * P, torch.int32)
        st = L.sgz_spectrogram_overview_device(plan.h, d_x.data_ptr(), d_x.stride(0), S, k, img.ptr if want_image else None,
                                               pk.ptr if want_peaks else None, None, _stream())
        assert st == api.SGZ_OK
        if want_image:
            assert np.array_equal(img.payload().reshape(columns, P, 4), image) and pk.untouched()
        else:
            assert np.array_equal(pk.payload().reshape(columns, Cn, P), v) and img.untouched()
        h_img = np.full((columns + 2, P, 4), BYTE, np.uint8)
        h_pk = np.full((columns + 2, Cn, P), WORD, np.uint32)
        st = L.sgz_spectrogram_overview_host(plan.h, ptrs, 4, S, k, h_img[1:].ctypes.data_as(C.c_void_p) if want_image else None,
                                             h_pk[1:].ctypes.data_as(C.c_void_p) if want_peaks else None, None)
        assert st == api.SGZ_OK
        assert (h_img[0] == BYTE).all() and (h_img[-1] == BYTE).all() and (h_pk[0] == WORD).all() and (h_pk[-1] == WORD).all()
        if want_image:
            assert np.array_equal(h_img[1:-1], image) and (h_pk == WORD).all()
        else:
            assert np.array_equal(h_pk[1:-1], v) and (h_img == BYTE).all()
    # fewer samples than a window: skipped, nothing written
    S = plan.cfg.window_size - 1
    xs = np.ascontiguousarray(x[:, :S])
    d_xs = torch.from_numpy(xs).to(gpu)
    img = Guarded(gpu, 1, P * 4, torch.uint8)
    pk = Guarded(gpu, 1, Cn * P, torch.int32)
    st = L.sgz_spectrogram_overview_device(plan.h, d_xs.data_ptr(), d_xs.stride(0), S, k, img.ptr, pk.ptr, None, _stream())
    torch.cuda.synchronize()
    assert st == api.SGZ_SKIPPED_FRAME and img.untouched() and pk.untouched()
    h_img = np.full((3, P, 4), BYTE, np.uint8)
    h_pk = np.full((3, Cn, P), WORD, np.uint32)
    ptrs = (C.c_void_p * 4)(*[xs[i].ctypes.data for i in range(4)])
    st = L.sgz_spectrogram_overview_host(plan.h, ptrs, 4, S, k, h_img[1:].ctypes.data_as(C.c_void_p), h_pk[1:].ctypes.data_as(C.c_void_p), None)
    assert st == api.SGZ_SKIPPED_FRAME and (h_img == BYTE).all() and (h_pk == WORD).all()
    assert plan.overview(xs, k) is None and plan.overview(d_xs, k) is None


def test_overview_is_the_same_beside_a_background_render(gpu):
    """the pattern of tests/test_gpu_concurrency.py: two threads keep the device busy with renders on streams of their own"""
    from test_gpu_concurrency import BackgroundLoad
    names = ("n32768_split", "rsnt", "w256_two_pairs")
    want = {name: _want(name, 5) for name in names}
    for name in names:
        _case(name)[0].set_option(api.OPT_OVERVIEW_SLAB, 3)
    with BackgroundLoad(gpu) as load:
        beside = 0
        for _ in range(400):                                     # (the load's threads build their plans first: go on until three rounds ran beside it)
            busy = load.renders > 0
            for name in names:
                plan, params, x, rgba, main = _case(name)
                image, v, _ = plan.overview(x, 5, want_peaks=True)
                assert np.array_equal(v.view(np.uint32), want[name][0]) and np.array_equal(image, want[name][1]), name
            beside += busy
            if beside >= 3 or load.errors:
                break
        assert beside >= 3, (beside, load.errors)
    for name in names:
        _case(name)[0].set_option(api.OPT_OVERVIEW_SLAB, 0)


def test_a_hundred_overview_calls_do_not_grow_device_memory(gpu):
    import gc

    import torch
    plan, params, x, rgba, main = _case("n4096_two_pairs")
    d_x = torch.from_numpy(x).to(gpu)

    def calls(n):
        for i in range(n):
            plan.set_option(api.OPT_OVERVIEW_SLAB, (0, 3, 8)[i % 3])
            if i % 2:
                plan.overview(x, 1 + i % 7, want_rgba=bool(i % 4 == 1), want_peaks=True)
            else:
                out = plan.overview(d_x, 1 + i % 7)
                del out
        gc.collect(); torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    free0 = calls(12)
    free1 = calls(100)
    plan.set_option(api.OPT_OVERVIEW_SLAB, 0)
    assert free0 - free1 < 2 << 20, f"device memory: {(free0 - free1) / 2**20:.1f} MiB fewer free after 100 overview calls"
