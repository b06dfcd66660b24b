"""The render thread's colour-spectrum frame as the plugin runs it (Spectrum::renderColourSpectrum, SpectrumRendering.cpp:672-749):
sgz_spectrum_render_columns (the pop loop with frame pacing and freeze, all columns of a video frame in one launch),
sgz_spectrum_present (drawCircular) and the two stage calls behind them, sgz_columns_to_image_device and sgz_image_unroll_device.
Both kernels only move texels: every comparison is byte for byte, against numpy."""
import ctypes as C
import struct
import threading
import time

import numpy as np
import pytest

from signalizer_amd import api, config, synth

pytestmark = pytest.mark.gpu

DEPTH = 10                                                  # frameQueue(10), SpectrumDSP.cpp:47


def _sync():
    import torch
    torch.cuda.synchronize()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream or None


def _words(n, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)


def _to_gpu(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(gpu)


def _to_host(t):
    _sync()
    return t.cpu().numpy().view(np.uint32)


def _view(raw, P, pitch):
    return raw[:P * pitch // 4].reshape(P, pitch // 4)


def bits(v):
    return struct.pack("<d", v)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the stage calls

PS = [1, 3, 64, 1000, 1024, 4099]
COLUMNS = [1, 7, 256, 2049]


def _pitches(columns):
    return [4 * columns, 4 * columns + 4, 4 * columns + 64]


@pytest.mark.parametrize("columns", COLUMNS)
@pytest.mark.parametrize("P", PS)
def test_columns_to_image_equals_numpy(gpu, P, columns):
    cases = 0
    for n in sorted({1, 2, 10, columns}):
        if n > columns:
            continue
        cols = _words(n * P, seed=P * 7 + columns * 3 + n).reshape(n, P)
        d_cols = _to_gpu(cols, gpu)
        for x0 in sorted({0, 1, columns - 1, columns // 2}):
            if x0 >= columns:
                continue
            for pitch in _pitches(columns):
                before = _words(P * pitch // 4, seed=pitch + x0 + 11)
                d_img = _to_gpu(before, gpu)
                api.columns_to_image_device(d_cols, n, P, d_img, columns, pitch, x0, _stream())
                got = _view(_to_host(d_img), P, pitch)
                want = _view(before, P, pitch).copy()
                for k in range(n):
                    want[:, (x0 + k) % columns] = cols[k]
                assert np.array_equal(got, want), (P, columns, n, x0, pitch, int((got != want).sum()))
                assert np.array_equal(_to_host(d_cols).reshape(n, P), cols)
                cases += 1
    assert cases >= 3


def test_columns_to_image_at_an_unaligned_base(gpu):
    """an image that starts 4, 8 and 12 bytes off a 16-byte boundary (a view into a larger allocation)"""
    P, columns, n = 130, 100, 37
    cols = _words(n * P, seed=5).reshape(n, P)
    d_cols = _to_gpu(cols, gpu)
    for off in (1, 2, 3):
        for pitch in (4 * columns, 4 * columns + 4, 4 * columns + 8):
            before = _words(P * pitch // 4 + 4, seed=off + pitch)
            d_buf = _to_gpu(before, gpu)
            api.columns_to_image_device(d_cols, n, P, d_buf.data_ptr() + 4 * off, columns, pitch, 90, _stream())
            got = _to_host(d_buf)
            want = before.copy()
            img = _view(want[off:], P, pitch)
            for k in range(n):
                img[:, (90 + k) % columns] = cols[k]
            assert np.array_equal(got, want), (off, pitch)


def test_offline_render_as_a_texture(gpu):
    """348 frames of cfg2 through sgz_spectrogram_render_device, then one call: the [P rows][columns] texture is the numpy transpose"""
    import torch
    cfg = config.cfg2()
    frames = 348
    x = synth.gen(config.CFG2_SEED, 48000, cfg["window_size"] + (frames - 1) * cfg["hop"], 2)
    plan = api.Plan(cfg).upload()
    rgba = plan.render(torch.from_numpy(x).to(gpu))
    assert tuple(rgba.shape) == (frames, plan.P, 4)
    pitch = 4 * frames + 16
    before = _words(plan.P * pitch // 4, seed=348)
    d_img = _to_gpu(before, gpu)
    api.columns_to_image_device(rgba, frames, plan.P, d_img, frames, pitch, 0, _stream())
    _sync()
    cols = rgba.cpu().numpy().view(np.uint32)[:, :, 0]
    got = _view(_to_host(d_img), plan.P, pitch)
    assert cols.any()
    assert np.array_equal(got[:, :frames], cols.T)
    assert np.array_equal(got[:, frames:], _view(before, plan.P, pitch)[:, frames:])


@pytest.mark.parametrize("columns", COLUMNS)
@pytest.mark.parametrize("P", PS)
def test_image_unroll_equals_numpy_roll(gpu, P, columns):
    xs = sorted({x for x in (0, 1, 2, 3, columns // 2, columns // 2 + 1, columns // 2 + 2, columns // 2 + 3, columns - 1) if x < columns})
    if columns >= 4:
        assert {x % 4 for x in xs} == {0, 1, 2, 3}
    for sp in _pitches(columns):
        src = _words(P * sp // 4, seed=P + columns + sp)
        d_src = _to_gpu(src, gpu)
        for dp in _pitches(columns):
            if dp == sp:
                continue
            for x in xs:
                before = _words(P * dp // 4, seed=dp + x + 3)
                d_dst = _to_gpu(before, gpu)
                api.image_unroll_device(d_src, columns, sp, P, x, d_dst, dp, _stream())
                got = _view(_to_host(d_dst), P, dp)
                want = _view(before, P, dp).copy()
                want[:, :columns] = np.roll(_view(src, P, sp)[:, :columns], -x, axis=1)
                assert np.array_equal(got, want), (P, columns, sp, dp, x, int((got != want).sum()))
        assert np.array_equal(_to_host(d_src), src)                                 # the source is read only


def test_image_unroll_at_unaligned_bases(gpu):
    P, columns = 70, 259
    for so in (0, 1, 2, 3):
        for do in (0, 1, 2, 3):
            sp, dp = 4 * columns + 4 * so, 4 * columns + 12
            src = _words(P * sp // 4 + 4, seed=so * 4 + do)
            before = _words(P * dp // 4 + 4, seed=99 + so * 4 + do)
            d_src, d_dst = _to_gpu(src, gpu), _to_gpu(before, gpu)
            x = 100 + so + do
            api.image_unroll_device(d_src.data_ptr() + 4 * so, columns, sp, P, x, d_dst.data_ptr() + 4 * do, dp, _stream())
            want = before.copy()
            _view(want[do:], P, dp)[:, :columns] = np.roll(_view(src[so:], P, sp)[:, :columns], -x, axis=1)
            assert np.array_equal(_to_host(d_dst), want), (so, do)


def test_stage_calls_refuse_overlap_and_bad_arguments(gpu):
    buf = _to_gpu(_words(200 * 8 * 3, seed=3), gpu)
    raw = _to_host(buf).copy()
    L = api.lib()
    p = buf.data_ptr()
    for args in ((p, 8, 32, 200, 0, p, 32),                       # the same memory
                 (p, 8, 32, 200, 0, p + 32 * 100, 32),            # the destination starts inside the source
                 (p + 32 * 100, 8, 32, 200, 0, p, 32),            # the source starts inside the destination
                 (p, 8, 32, 200, 0, p + 16, 64),                  # interleaved rows still share the byte range
                 (p, 8, 28, 200, 0, p + 32 * 200, 32),            # pitch < 4 * columns
                 (p, 8, 32, 200, 0, p + 32 * 200, 34),            # pitch not a multiple of 4
                 (p, 8, 32, 200, 8, p + 32 * 200, 32),            # x >= columns
                 (p, 0, 32, 200, 0, p + 32 * 200, 32),
                 (p, 8, 32, 0, 0, p + 32 * 200, 32)):
        assert L.sgz_image_unroll_device(*args, None) == api.SGZ_EINVAL, args
    for args in ((p, 9, 200, p + 32 * 200, 8, 32, 0),             # n > columns
                 (p, 0, 200, p + 32 * 200, 8, 32, 0),
                 (p, 2, 200, p + 32 * 200, 8, 32, 8),             # x0 >= columns
                 (p, 2, 200, p + 32 * 200, 8, 28, 0),
                 (p, 2, 200, p + 32 * 200 + 2, 8, 32, 0)):
        assert L.sgz_columns_to_image_device(*args, None) == api.SGZ_EINVAL, args
    assert np.array_equal(_to_host(buf), raw)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the handle

HOP, W = 512, 4096


def _cfg(P=200, **over):
    return config.spectrum_config(window_size=W, hop=HOP, axis_points=P, **over)


def _create(cfg):
    c = api.config_from_dict(cfg)
    h = C.c_void_p()
    api.check(api.lib().sgz_spectrum_create(C.byref(c), C.byref(h)))
    return h


def _destroy(*handles):
    for h in handles:
        api.lib().sgz_spectrum_destroy(h)


def _push(h, x, block):
    for pos in range(0, x.shape[1], block):
        blk = np.ascontiguousarray(x[:, pos:pos + block])
        ptrs = (C.c_void_p * blk.shape[0])(*[blk[c].ctypes.data for c in range(blk.shape[0])])
        while True:
            st = api.lib().sgz_spectrum_push(h, ptrs, blk.shape[0], blk.shape[1])
            if st != api.SGZ_BUSY:
                break
        api.check(st)


def _settle(h):
    """everything pushed so far is in the queue and its copies have landed: queue counts are deterministic afterwards"""
    api.lib().sgz_spectrum_flush.argtypes = [C.c_void_p]
    api.check(api.lib().sgz_spectrum_flush(h))
    _sync()


def _pop_ready(h, P):
    cols, buf, ap = [], np.zeros((P, 4), np.uint8), C.c_uint32(0)
    while True:
        st = api.lib().sgz_spectrum_pop_column(h, buf.ctypes.data_as(C.c_void_p), C.byref(ap))
        if st != api.SGZ_OK:
            assert st == api.SGZ_EMPTY
            return cols
        assert ap.value == P
        cols.append(buf.view(np.uint32)[:, 0].copy())


def _stats(h):
    dropped, refused = C.c_uint64(0), C.c_uint64(0)
    api.check(api.lib().sgz_spectrum_stats(h, C.byref(dropped), C.byref(refused)))
    return dropped.value


class _Image:
    """a caller-owned device image of random texels, bound to a handle"""

    def __init__(self, h, P, columns, pad, gpu, seed):
        self.P, self.columns, self.pitch = P, columns, 4 * (columns + pad)
        self.t = _to_gpu(_words(P * self.pitch // 4, seed), gpu)
        if h is not None:
            api.check(api.lib().sgz_spectrum_bind_image(h, C.c_void_p(self.t.data_ptr()), columns, self.pitch))

    def read(self):
        return _view(_to_host(self.t), self.P, self.pitch).copy()


def _columns_of(cfg, x, block):
    """every column a handle of `cfg` makes of `x`, popped one push at a time (a twin that never drops)"""
    h = _create(cfg)
    try:
        cols = []
        for pos in range(0, x.shape[1], block):
            _push(h, x[:, pos:pos + block], block)
            _settle(h)
            cols += _pop_ready(h, cfg["axis_points"])
        return cols
    finally:
        _destroy(h)


@pytest.mark.parametrize("block,P", [(256, 200), (480, 200), (512, 200), (512, 1024), (480, 4099)])
def test_render_columns_at_smoothing_zero_is_the_pop_loop(gpu, block, P):
    """twin handles fed the same blocks: A drained with pop_column into a numpy image at a Python framePixelPosition, B with
    render_columns -- images, first_column and count agree, a lap around the 16-column image included"""
    columns, cfg = 16, _cfg(P)
    groups = [3, 1, 7, 10, 0, 2, 9, 5, 4]                    # hops of audio between consumer calls: 41 columns, two and a half laps
    x = synth.gen(71, 48000, HOP * sum(groups), 2)
    a, b = _create(cfg), _create(cfg)
    try:
        img = _Image(b, P, columns, 3, gpu, seed=block + P)
        ref = img.read()
        pos_a, at, total = 0, 0, 0
        for g in groups:
            piece = x[:, at:at + g * HOP]
            at += g * HOP
            for h in (a, b):
                _push(h, piece, block)
                _settle(h)
            popped = _pop_ready(a, P)
            first = pos_a
            for col in popped:
                ref[:, pos_a] = col
                pos_a = (pos_a + 1) % columns
            st, got_first, got_count, fpu = api.spectrum_render_columns(b)
            assert got_count == len(popped) and got_first == first, (g, got_first, got_count, first, len(popped))
            assert st == (api.SGZ_OK if popped else api.SGZ_EMPTY)
            assert bits(fpu) == bits(0.0)                       # (:729-731 with an emptied queue)
            got = img.read()
            assert np.array_equal(got, ref), (g, int((got != ref).sum()))
            total += len(popped)
        assert total == sum(groups) and total > 2 * columns
    finally:
        _destroy(a, b)


@pytest.mark.parametrize("smoothing", [0.5, 0.9])
def test_render_columns_paces_as_the_reference_loop(gpu, smoothing):
    P, columns = 200, 32
    cfg = _cfg(P)
    # hops of audio pushed before each call, picked so that the calls meet every queue length 0 ... 10 at both smoothings (asserted below)
    schedule = [4, 0, 5, 1, 1, 5, 0, 1, 5, 0, 0, 1, 3, 6, 3, 1, 1, 6, 1, 3, 1, 1, 1, 1, 0, 1, 1, 4, 8, 3, 0, 0, 1, 2]
    x = synth.gen(73, 48000, HOP * sum(schedule), 2)
    every = _columns_of(cfg, x, HOP)
    assert len(every) == sum(schedule)
    h = _create(cfg)
    try:
        img = _Image(h, P, columns, 1, gpu, seed=7)
        ref = img.read()
        api.spectrum_set_pacing(h, smoothing)
        queue, produced, z, pos, seen, dropped = [], 0, 0.0, 0, set(), 0
        for call, g in enumerate(schedule):
            _push(h, x[:, produced * HOP:(produced + g) * HOP], HOP)
            _settle(h)
            for k in range(produced, produced + g):             # a full queue drops the new column (SpectrumDSP.cpp:185-186)
                if len(queue) < DEPTH:
                    queue.append(k)
                else:
                    dropped += 1
            produced += g
            seen.add(len(queue))
            pop, z = api.frame_pacing_step(z, smoothing, len(queue))
            st, first, count, fpu = api.spectrum_render_columns(h)
            assert count == pop and bits(fpu) == bits(z), (call, count, pop, fpu, z)
            assert first == pos and st == (api.SGZ_OK if pop else api.SGZ_EMPTY)
            if call == 0:
                assert count == 0 and len(queue) == 4            # round(0): the first frame takes nothing
            for k in queue[:pop]:
                ref[:, pos] = every[k]
                pos = (pos + 1) % columns
            queue = queue[pop:]
            got = img.read()
            assert np.array_equal(got, ref), (call, int((got != ref).sum()))
        assert seen == set(range(DEPTH + 1)), sorted(seen)       # the calls met every queue length 0 ... 10
        assert _stats(h) == dropped and dropped > 0
    finally:
        _destroy(h)


def test_freeze_stops_the_image_not_the_audio(gpu):
    P, columns = 200, 16
    cfg = _cfg(P)
    x = synth.gen(79, 48000, HOP * 30, 2)
    every = _columns_of(cfg, x, HOP)
    h = _create(cfg)
    try:
        img = _Image(h, P, columns, 2, gpu, seed=9)
        out = _to_gpu(_words(P * columns, seed=10), gpu)
        api.spectrum_set_pacing(h, 0.5)
        _push(h, x[:, :HOP * 6], HOP)
        _settle(h)
        z = 0.0
        taken = 0
        for _ in range(2):                                      # (round(0) = 0 columns, then round(3) = 3 of the six)
            pop, z = api.frame_pacing_step(z, 0.5, 6 - taken)
            st, first, count, fpu = api.spectrum_render_columns(h)
            assert count == pop and bits(fpu) == bits(z)
            taken += count
        assert 0 < taken < 6 and z != 0.0
        before = img.read()
        api.spectrum_present(h, out, 4 * columns)
        shown = _to_host(out).copy()
        assert np.array_equal(shown.reshape(P, columns), np.roll(before[:, :columns], -taken, axis=1))
        api.spectrum_set_frozen(h, True)
        assert _stats(h) == 0
        for k in range(6, 24):                                  # 18 more columns: the queue holds 6 - taken + ... up to 10, the rest drop
            _push(h, x[:, HOP * k:HOP * (k + 1)], HOP)
            _settle(h)
            st, first, count, fpu = api.spectrum_render_columns(h)
            assert st == api.SGZ_EMPTY and count == 0 and first == taken and bits(fpu) == bits(z)
        assert np.array_equal(img.read(), before)
        queued = list(range(taken, taken + DEPTH))
        assert _stats(h) == 24 - taken - DEPTH                  # produced - taken - what the queue holds
        api.spectrum_present(h, out, 4 * columns)              # the same picture while frozen
        assert np.array_equal(_to_host(out), shown)
        api.spectrum_set_frozen(h, False)
        pop, z = api.frame_pacing_step(z, 0.5, DEPTH)
        st, first, count, fpu = api.spectrum_render_columns(h)
        assert st == api.SGZ_OK and first == taken and count == pop > 0 and bits(fpu) == bits(z)
        want = before.copy()
        for j, k in enumerate(queued[:pop]):
            want[:, (taken + j) % columns] = every[k]
        assert np.array_equal(img.read(), want)
    finally:
        _destroy(h)


def _hip_read(ptr, nbytes):
    _sync()
    host = np.zeros(nbytes // 4, np.uint32)
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0
    return host


@pytest.mark.parametrize("own", [False, True])
def test_present_unrolls_the_bound_image(gpu, own):
    P, columns = 200, 16
    cfg = _cfg(P)
    x = synth.gen(83, 48000, HOP * 19, 2)
    h = _create(cfg)
    try:
        if own:
            d_img, pitch = C.c_void_p(), C.c_size_t(0)
            api.check(api.lib().sgz_spectrum_create_image(h, columns, C.byref(d_img), C.byref(pitch), None))
            sp = pitch.value
            read = lambda: _view(_hip_read(d_img.value, P * sp), P, sp)          # noqa: E731
        else:
            img = _Image(h, P, columns, 3, gpu, seed=12)
            read = img.read
        dp = 4 * columns + 20
        pushed = 0
        for upto in (0, 5, 16 + 3):
            if upto > pushed:
                for k in range(pushed, upto):                   # (one call per column: the queue holds 10)
                    _push(h, x[:, HOP * k:HOP * (k + 1)], HOP)
                    _settle(h)
                    st, first, count, _ = api.spectrum_render_columns(h)
                    assert st == api.SGZ_OK and count == 1 and first == k % columns
                pushed = upto
            before = _words(P * dp // 4, seed=upto)
            out = _to_gpu(before, gpu)
            api.spectrum_present(h, out, dp)
            got = _view(_to_host(out), P, dp)
            ring = read()
            assert np.array_equal(got[:, :columns], np.roll(ring[:, :columns], -(upto % columns), axis=1)), upto
            assert np.array_equal(got[:, columns:], _view(before, P, dp)[:, columns:])
            if upto:
                assert ring[:, :min(upto, columns)].any()
    finally:
        _destroy(h)


def test_the_three_settings_survive_every_reconfiguration(gpu):
    P, columns = 200, 16
    cfg = _cfg(P)
    x = synth.gen(89, 48000, HOP * 16, 2)
    h = _create(cfg)
    try:
        img = _Image(h, P, columns, 0, gpu, seed=14)
        api.spectrum_set_pacing(h, 0.5)
        _push(h, x[:, :HOP * 4], HOP)
        _settle(h)
        z, q = 0.0, 4
        for _ in range(2):
            pop, z = api.frame_pacing_step(z, 0.5, q)
            st, _, count, fpu = api.spectrum_render_columns(h)
            assert count == pop and bits(fpu) == bits(z)
            q -= pop
        assert z == 3.0 and q == 2
        # pop_column and flush_columns read and write none of the three
        first, cnt = C.c_uint32(0), C.c_uint32(0)
        one, ap = np.zeros((P, 4), np.uint8), C.c_uint32(0)
        assert api.lib().sgz_spectrum_pop_column(h, one.ctypes.data_as(C.c_void_p), C.byref(ap)) == api.SGZ_OK      # one of the two left
        assert api.lib().sgz_spectrum_flush_columns(h, C.byref(first), C.byref(cnt)) == api.SGZ_OK and cnt.value == 1
        _push(h, x[:, HOP * 4:HOP * 6], HOP)
        _settle(h)
        pop, z = api.frame_pacing_step(z, 0.5, 2)
        st, _, count, fpu = api.spectrum_render_columns(h)
        assert (count, bits(fpu)) == (pop, bits(z)) and pop == 2
        api.spectrum_set_frozen(h, True)

        def still():
            st, _, count, fpu = api.spectrum_render_columns(h)
            assert st == api.SGZ_EMPTY and count == 0 and bits(fpu) == bits(z)

        still()
        api.spectrum_set_view(h, 0.1, 0.9)
        still()
        img2 = _Image(None, 240, columns, 1, gpu, seed=15)
        api.spectrum_resize(h, 240, img2.t, columns, img2.pitch)
        still()
        api.spectrum_update(h, dict(_cfg(240), view_left=0.1, view_right=0.9, low_db=-100.0))
        still()
        c = api.config_from_dict(cfg)
        api.check(api.lib().sgz_spectrum_configure(h, C.byref(c)))
        assert api.lib().sgz_spectrum_render_columns(h, None, None, None) == api.SGZ_EINVAL      # (a configure drops the binding)
        img3 = _Image(h, P, columns, 2, gpu, seed=16)
        still()
        api.check(api.lib().sgz_spectrum_bind_image(h, C.c_void_p(img.t.data_ptr()), columns, img.pitch))
        still()
        api.spectrum_set_frozen(h, False)
        _push(h, x[:, HOP * 6:HOP * 9], HOP)                   # (the configure emptied the queue: three columns)
        _settle(h)
        pop, z = api.frame_pacing_step(z, 0.5, 3)
        st, first, count, fpu = api.spectrum_render_columns(h)
        assert st == api.SGZ_OK and first == 0 and count == pop == 3 and bits(fpu) == bits(z) and z != 0.0
        del img3
    finally:
        _destroy(h)


def test_refusals(gpu):
    P, columns = 200, 16
    L = api.lib()
    h = _create(_cfg(P, display_mode=config.DISPLAY_LINE_GRAPH))
    try:
        buf = _to_gpu(_words(P * columns * 2, seed=17), gpu)
        assert L.sgz_spectrum_set_pacing(h, 0.5) == api.SGZ_EINVAL
        assert L.sgz_spectrum_set_frozen(h, 1) == api.SGZ_EINVAL
        assert L.sgz_spectrum_render_columns(h, None, None, None) == api.SGZ_EINVAL
        assert L.sgz_spectrum_present(h, C.c_void_p(buf.data_ptr()), 4 * columns) == api.SGZ_EINVAL
    finally:
        _destroy(h)
    h = _create(_cfg(P))
    try:
        raw = _to_host(buf).copy()
        assert L.sgz_spectrum_render_columns(h, None, None, None) == api.SGZ_EINVAL               # no image bound
        assert L.sgz_spectrum_present(h, C.c_void_p(buf.data_ptr()), 4 * columns) == api.SGZ_EINVAL
        for s in (float("nan"), float("inf"), -0.25, 1.0, 2.0):
            assert L.sgz_spectrum_set_pacing(h, s) == api.SGZ_EINVAL, s
        api.spectrum_set_pacing(h, 0.996)
        api.spectrum_set_pacing(h, 0.0)
        p = buf.data_ptr()
        api.check(L.sgz_spectrum_bind_image(h, C.c_void_p(p), columns, 4 * columns))
        for dst, pitch in ((p, 4 * columns), (p + 4 * columns * 100, 4 * columns), (p + 8, 8 * columns),     # into the bound image
                           (p + 4 * columns * P, 4 * columns - 4), (p + 4 * columns * P, 4 * columns + 2), (p + 4 * columns * P + 2, 4 * columns)):
            assert L.sgz_spectrum_present(h, C.c_void_p(dst), pitch) == api.SGZ_EINVAL, (dst - p, pitch)
        assert L.sgz_spectrum_present(h, None, 4 * columns) == api.SGZ_EINVAL
        assert np.array_equal(_to_host(buf), raw)
        api.spectrum_present(h, p + 4 * columns * P, 4 * columns)                                  # right behind it: fine
        got = _to_host(buf)
        assert np.array_equal(got[columns * P:], raw[:columns * P]) and np.array_equal(got[:columns * P], raw[:columns * P])
    finally:
        _destroy(h)


def test_render_columns_while_another_thread_pushes(gpu):
    """a producer thread pushes while the consumer renders: every column that lands is one the twin produced, in order (a full queue
    drops columns, so they form a subsequence), and landed + dropped = produced"""
    P, columns, block, blocks = 200, 256, 256, 400
    cfg = _cfg(P)
    x = synth.gen(97, 48000, block * blocks, 2)
    every = _columns_of(cfg, x, 2048)
    produced = block * blocks // HOP
    assert len(every) == produced
    h = _create(cfg)
    try:
        img = _Image(h, P, columns, 0, gpu, seed=19)
        before = img.read()
        done = threading.Event()

        def producer():
            for k in range(blocks):
                _push(h, x[:, k * block:(k + 1) * block], block)
                time.sleep(0.0002)
            done.set()

        t = threading.Thread(target=producer)
        t.start()
        landed, counts = 0, []
        while not done.is_set():
            st, first, count, fpu = api.spectrum_render_columns(h)
            assert st in (api.SGZ_OK, api.SGZ_EMPTY) and count <= DEPTH
            if count:
                assert first == landed
                counts.append(count)
            landed += count
        t.join()
        _settle(h)
        while True:
            st, first, count, _ = api.spectrum_render_columns(h)
            if st == api.SGZ_EMPTY:
                break
            assert first == landed
            landed += count
        assert 0 < landed <= produced < columns
        assert landed + _stats(h) == produced
        got = img.read()
        k = 0
        for j in range(landed):
            while k < produced and not np.array_equal(every[k], got[:, j]):
                k += 1
            assert k < produced, j
            k += 1
        assert np.array_equal(got[:, landed:], before[:, landed:])
    finally:
        _destroy(h)


def test_render_and_present_cycles_do_not_grow_memory(gpu):
    import torch

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    P, columns = 1024, 64
    cfg = _cfg(P)
    x = synth.gen(101, 48000, HOP * 4, 2)
    h = _create(cfg)
    try:
        img = _Image(h, P, columns, 0, gpu, seed=21)
        out = torch.zeros((P, columns), dtype=torch.int32, device=gpu)

        def cycle(k):
            _push(h, x[:, (k % 4) * HOP:(k % 4 + 1) * HOP], HOP)
            _settle(h)
            st, _, count, _ = api.spectrum_render_columns(h)
            assert st == api.SGZ_OK and count == 1
            api.spectrum_present(h, out, 4 * columns)

        for k in range(8):
            cycle(k)
        f0 = free()
        for k in range(200):
            cycle(k)
        f1 = free()
        assert f0 - f1 < (16 << 20), (f0 - f1)
        del img
    finally:
        _destroy(h)
