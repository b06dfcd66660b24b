"""sgz_spectrum_resize: a new axis size for a live spectrum handle (Spectrum::handleFlagUpdates' resized branch, Spectrum.cpp:503-515).
New plans and axis-sized buffers, both line graphs cleared, the bound spectrogram image resampled into the new one (oglImage.resize(w, h,
true)) -- and the audio history, the frame cadence and, at an unchanged size, the column queue kept.  Every comparison is bit for bit."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

from signalizer_amd import api, config, synth

pytestmark = pytest.mark.gpu


def _rows(P0, P1):
    """the row rule of sgz.h in numpy (float64, the header's order of operations)"""
    i = np.arange(P1, dtype=np.float64)
    r = (i * (P0 - 1.0)) / (P1 - 1.0)
    j = np.floor(r)
    w = np.floor((r - j) * 256.0 + 0.5)
    j = np.where(w == 256.0, j + 1.0, j)
    w = np.where(w == 256.0, 0.0, w)
    return j.astype(np.int64), w.astype(np.uint32)


def _cols(C0, x0, C1):
    """the column rule of sgz.h: (source column or -1 per new column, x1)"""
    x1 = x0 % C1
    c = np.arange(C1)
    age = (x1 - 1 - c) % C1
    return np.where(age < min(C0, C1), (x0 - 1 - age) % C0, -1), x1


def _resize(old, C0, x0, P1, C1, into):
    """numpy application of the rule: old [P0][>= C0] uint32 texels into `into` [P1][>= C1] (a copy is returned; texels beyond C1 kept)"""
    P0 = old.shape[0]
    j, w = _rows(P0, P1)
    cs, x1 = _cols(C0, x0, C1)
    out = into.copy()
    cc = np.clip(cs, 0, C0 - 1)
    a = np.ascontiguousarray(old[j][:, cc]).view(np.uint8).reshape(P1, C1, 4).astype(np.uint32)
    b = np.ascontiguousarray(old[np.minimum(j + 1, P0 - 1)][:, cc]).view(np.uint8).reshape(P1, C1, 4).astype(np.uint32)
    ww = w[:, None, None]
    blend = ((a * (256 - ww) + b * ww + 128) >> 8).astype(np.uint8)
    blend[:, cs < 0] = 0
    out[:, :C1] = blend.reshape(P1, C1 * 4).view(np.uint32)
    return out, x1


def _create(cfg):
    c = api.config_from_dict(cfg)
    h = C.c_void_p()
    api.check(api.lib().sgz_spectrum_create(C.byref(c), C.byref(h)))
    return h


def _flush(h):
    api.lib().sgz_spectrum_flush.argtypes = [C.c_void_p]
    api.check(api.lib().sgz_spectrum_flush(h))


def _push_all(h, x, block):
    for pos in range(0, x.shape[1], block):
        blk = np.ascontiguousarray(x[:, pos:pos + block])
        ptrs = (C.c_void_p * blk.shape[0])(*[blk[c].ctypes.data for c in range(blk.shape[0])])
        while True:
            st = api.lib().sgz_spectrum_push(h, ptrs, blk.shape[0], blk.shape[1])
            if st != api.SGZ_BUSY:
                break
        api.check(st)
    _flush(h)


def _pop_all(h, P, want, timeout=20.0):
    _flush(h)
    cols, buf, ap, t0 = [], np.zeros((P, 4), np.uint8), C.c_uint32(0), time.time()
    while len(cols) < want and time.time() - t0 < timeout:
        st = api.lib().sgz_spectrum_pop_column(h, buf.ctypes.data_as(C.c_void_p), C.byref(ap))
        if st == api.SGZ_OK:
            assert ap.value == P
            cols.append(buf.view(np.uint32)[:, 0].copy())
        else:
            assert st == api.SGZ_EMPTY
            time.sleep(0.001)
    assert len(cols) == want
    return np.stack(cols)


def _flush_columns(h, want, timeout=20.0):
    _flush(h)
    total, first, cnt, t0 = 0, C.c_uint32(0), C.c_uint32(0), time.time()
    while total < want and time.time() - t0 < timeout:
        st = api.lib().sgz_spectrum_flush_columns(h, C.byref(first), C.byref(cnt))
        if st == api.SGZ_OK:
            total += cnt.value
        else:
            assert st == api.SGZ_EMPTY
            time.sleep(0.001)
    assert total == want


def _hip_read(ptr, nbytes):
    torch_sync()
    host = np.zeros(nbytes // 4, np.uint32)
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0
    return host


def torch_sync():
    import torch
    torch.cuda.synchronize()


class _Buf:
    """caller-owned device memory holding random texels: images of any layout are views of it"""

    def __init__(self, words, gpu, seed):
        import torch
        rng = np.random.default_rng(seed)
        init = rng.integers(0, 2 ** 32, size=words, dtype=np.uint64).astype(np.uint32)
        self.t = torch.from_numpy(init.view(np.int32)).to(gpu)
        self.ptr = self.t.data_ptr()

    def raw(self):
        torch_sync()
        return self.t.cpu().numpy().view(np.uint32)


def _view(raw, P, pitch):
    return raw[:P * pitch // 4].reshape(P, pitch // 4)


def _pitch(columns, pad):
    return 4 * (columns + pad)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the stage call

@pytest.mark.parametrize("P0,P1", [(2, 3), (200, 2), (1024, 1080), (1080, 1024), (200, 200), (2160, 1024)])
@pytest.mark.parametrize("C0,x0,C1", [(7, 3, 7), (7, 0, 20), (300, 299, 40), (2048, 1024, 2048), (2048, 777, 3000), (2048, 0, 1000)])
def test_stage_call_resizes_an_image(gpu, P0, P1, C0, x0, C1):
    sp, dp = _pitch(C0, 3), _pitch(C1, 5)
    src = _Buf(P0 * sp // 4, gpu, seed=P0 * 31 + C0)
    dst = _Buf(P1 * dp // 4, gpu, seed=P1 * 17 + C1 + 1)
    old, before = src.raw(), dst.raw()
    x1 = api.image_resize_device(src.t, C0, sp, P0, x0, dst.t, C1, dp, P1)
    want, want_x1 = _resize(_view(old, P0, sp), C0, x0, P1, C1, _view(before, P1, dp))
    got = _view(dst.raw(), P1, dp)
    assert x1 == want_x1
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(got[:, C1:], _view(before, P1, dp)[:, C1:])          # pitch padding untouched
    assert np.array_equal(src.raw(), old)                                       # the source is read only


def test_stage_call_same_size_is_the_identity(gpu):
    P, C0, pitch = 1024, 2048, _pitch(2048, 2)
    src = _Buf(P * pitch // 4, gpu, seed=1)
    dst = _Buf(P * pitch // 4, gpu, seed=2)
    x1 = api.image_resize_device(src.t, C0, pitch, P, 1234, dst.t, C0, pitch, P)
    assert x1 == 1234
    assert np.array_equal(_view(dst.raw(), P, pitch)[:, :C0], _view(src.raw(), P, pitch)[:, :C0])


def test_stage_call_refuses_overlap_and_bad_layouts(gpu):
    buf = _Buf(200 * 32 // 4 * 3, gpu, seed=3)
    raw = buf.raw()
    L = api.lib()
    x1 = C.c_uint32(0)
    p = buf.ptr
    for args in ((p, 8, 32, 200, 0, p, 8, 32, 200),                 # the same memory
                 (p, 8, 32, 200, 0, p + 32 * 100, 8, 32, 200),      # the destination starts inside the source
                 (p + 32 * 100, 8, 32, 200, 0, p, 8, 32, 200),      # the source starts inside the destination
                 (p, 8, 28, 200, 0, p + 32 * 200, 8, 32, 200),      # pitch < 4 * columns
                 (p, 8, 32, 200, 8, p + 32 * 200, 8, 32, 200),      # x0 >= C0
                 (p, 8, 32, 200, 0, p + 32 * 200, 8, 32, 1)):       # P1 < 2
        assert L.sgz_image_resize_device(*args, C.byref(x1), None) == api.SGZ_EINVAL, args
    assert np.array_equal(buf.raw(), raw)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the history is kept

CASES = {
    # cfg2's shape: W = N = 32768, Separate: the channel-split kernel on both sides (SGZ_PATH_FUSED | SGZ_PATH_CHANNEL_SPLIT)
    "cfg2-1024-to-1080": (dict(window_size=32768, hop=8192), 1024, 1080, 24, 30, "caller"),
    "w4096-up": (dict(window_size=4096, hop=512), 200, 333, 24, 24, "caller"),
    "w4096-down": (dict(window_size=4096, hop=512), 333, 120, 24, 20, "caller"),
    "w4096-complex": (dict(window_size=4096, hop=512, channel_mode=config.CH_COMPLEX), 200, 256, 24, 24, "caller"),
    "w4096-phase": (dict(window_size=4096, hop=512, channel_mode=config.CH_PHASE), 256, 200, 24, 28, "caller"),
    "w4096-own-image": (dict(window_size=4096, hop=512), 200, 300, 24, 20, "own"),
    "w4096-own-image-kept": (dict(window_size=4096, hop=512), 200, 300, 24, 20, "own-in-place"),
    "w4096-in-place": (dict(window_size=4096, hop=512), 300, 200, 24, 30, "in-place"),
    "w4096-in-place-up": (dict(window_size=4096, hop=512), 200, 300, 24, 20, "in-place"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_history_is_kept(gpu, case):
    import torch
    over, P0, P1, C0, C1, kind = CASES[case]
    cfg_old = config.spectrum_config(axis_points=P0, **over)
    cfg_new = config.spectrum_config(axis_points=P1, **over)
    W, hop = over["window_size"], over["hop"]
    if case.startswith("cfg2"):
        assert api.Plan(cfg_old).path == 9 and api.Plan(cfg_new).path == 9
    x = synth.gen(17, 48000, hop * 19, 2)
    padded = np.ascontiguousarray(np.concatenate([np.zeros((2, W), np.float32), x], axis=1)[:, hop:])
    plan = api.Plan(cfg_new).upload()
    want = plan.render(torch.from_numpy(np.ascontiguousarray(padded[:, 8 * hop:])).to(gpu)).cpu().numpy().view(np.uint32)[:, :, 0]
    assert want.shape == (11, P1)

    h = _create(cfg_old)
    try:
        # the old image and where the new one lives
        if kind in ("own", "own-in-place"):
            d_img, pitch = C.c_void_p(), C.c_size_t(0)
            api.check(api.lib().sgz_spectrum_create_image(h, C0, C.byref(d_img), C.byref(pitch), None))
            old_ptr, sp = d_img.value, pitch.value
            old_words = P0 * sp // 4
            read_old = lambda: _hip_read(old_ptr, old_words * 4)          # noqa: E731
        else:
            sp = _pitch(C0, 3)
            buf = _Buf(max(P0 * sp, P1 * _pitch(C1, 2)) // 4, gpu, seed=3)
            old_ptr = buf.ptr
            api.check(api.lib().sgz_spectrum_bind_image(h, old_ptr, C0, sp))
            read_old = buf.raw
        if kind == "caller" or kind == "own":
            dp = _pitch(C1, 2)
            new = _Buf(P1 * dp // 4, gpu, seed=4)
            new_ptr, read_new = new.ptr, new.raw
        elif kind == "own-in-place":
            dp, new_ptr = sp, old_ptr                                   # (the library's own image, kept: the new size fits its 2 MiB)
            read_new = lambda: _hip_read(old_ptr, P1 * dp)             # noqa: E731
        else:
            dp, new_ptr, read_new = _pitch(C1, 2), old_ptr, buf.raw
        _push_all(h, x[:, :8 * hop], hop)
        _flush_columns(h, 8)
        before_old = read_old()
        before_new = read_new()
        api.spectrum_resize(h, P1, new_ptr, C1, dp)
        after = _view(read_new(), P1, dp)
        want_img, x1 = _resize(_view(before_old, P0, sp), C0, 8, P1, C1, _view(before_new, P1, dp))
        assert x1 == 8
        assert np.array_equal(after, want_img), int((after != want_img).sum())
        for k in range(8, 19):                                 # (one flush per column: the queue holds 10, SpectrumDSP.cpp:47)
            _push_all(h, x[:, k * hop:(k + 1) * hop], hop)
            _flush_columns(h, 1)
        got = _view(read_new(), P1, dp)
        assert np.array_equal(got[:, 8:19].T, want), int((got[:, 8:19].T != want).sum())
        assert np.array_equal(got[:, :8], after[:, :8]) and np.array_equal(got[:, 19:], after[:, 19:])
    finally:
        api.lib().sgz_spectrum_destroy(h)

    # the same columns through sgz_spectrum_configure: the history went back to silence, so they differ
    h = _create(cfg_old)
    try:
        _push_all(h, x[:, :8 * hop], hop)
        _pop_all(h, P0, 8)
        c = api.config_from_dict(cfg_new)
        api.check(api.lib().sgz_spectrum_configure(h, C.byref(c)))
        other = []
        for k in range(8, 19):
            _push_all(h, x[:, k * hop:(k + 1) * hop], hop)
            other.append(_pop_all(h, P1, 1)[0])
        other = np.stack(other)
        assert not np.array_equal(other, want)
    finally:
        api.lib().sgz_spectrum_destroy(h)


def test_strict_framing_cadence_is_kept(gpu):
    """strict-quirks framing with blocks that do not divide the hop: the cadence (sinceLast) crosses the resize"""
    P0, P1, hop, block = 200, 240, 512, 384
    over = dict(window_size=4096, hop=hop)
    x = synth.gen(19, 48000, block * 24, 2)
    cols = []
    for resize in (True, False):
        h = _create(config.spectrum_config(axis_points=P1 if not resize else P0, **over))
        try:
            api.check(api.lib().sgz_spectrum_set_option(h, api.RT_OPT_STRICT_REFERENCE_QUIRKS, 1))
            _push_all(h, x[:, :block * 11], block)
            n0 = (block * 11) // hop
            _pop_all(h, P1 if not resize else P0, n0)
            if resize:
                api.spectrum_resize(h, P1)
            else:
                api.check(api.lib().sgz_spectrum_clear_state(h))
            _push_all(h, x[:, block * 11:], block)
            cols.append(_pop_all(h, P1, (block * 24) // hop - n0))
        finally:
            api.lib().sgz_spectrum_destroy(h)
    assert np.array_equal(cols[0], cols[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the column queue

def test_unchanged_height_keeps_queued_columns(gpu):
    """Spectrum stretch: the same axis size, a new column count -- the queued columns land in the new image from x1 on"""
    hop, P, C0, C1 = 512, 200, 16, 12
    cfg = config.spectrum_config(window_size=4096, hop=hop, axis_points=P)
    x = synth.gen(41, 48000, hop * 8, 2)
    ref = _create(cfg)
    try:
        _push_all(ref, x, hop)
        want = _pop_all(ref, P, 8)
    finally:
        api.lib().sgz_spectrum_destroy(ref)
    h = _create(cfg)
    try:
        sp, dp = _pitch(C0, 1), _pitch(C1, 3)
        old = _Buf(P * sp // 4, gpu, seed=5)
        new = _Buf(P * dp // 4, gpu, seed=6)
        api.check(api.lib().sgz_spectrum_bind_image(h, old.ptr, C0, sp))
        _push_all(h, x[:, :hop * 5], hop)
        _flush_columns(h, 5)
        _push_all(h, x[:, hop * 5:], hop)                      # three columns wait in the queue
        before_old, before_new = old.raw(), new.raw()
        api.spectrum_resize(h, P, new.t, C1, dp)
        after = _view(new.raw(), P, dp)
        want_img, x1 = _resize(_view(before_old, P, sp), C0, 5, P, C1, _view(before_new, P, dp))
        assert x1 == 5 and np.array_equal(after, want_img)
        _flush_columns(h, 3)
        got = _view(new.raw(), P, dp)
        assert np.array_equal(got[:, 5:8].T, want[5:8])
        assert np.array_equal(got[:, :5], after[:, :5]) and np.array_equal(got[:, 8:], after[:, 8:])
    finally:
        api.lib().sgz_spectrum_destroy(h)


def test_unchanged_height_keeps_queued_columns_for_pop(gpu):
    hop, P = 512, 200
    cfg = config.spectrum_config(window_size=4096, hop=hop, axis_points=P)
    x = synth.gen(43, 48000, hop * 6, 2)
    ref = _create(cfg)
    try:
        _push_all(ref, x, hop)
        want = _pop_all(ref, P, 6)
    finally:
        api.lib().sgz_spectrum_destroy(ref)
    h = _create(cfg)
    try:
        _push_all(h, x, hop)
        api.spectrum_resize(h, P)
        got = _pop_all(h, P, 6)
    finally:
        api.lib().sgz_spectrum_destroy(h)
    assert np.array_equal(got, want)


def test_changed_height_discards_queued_columns(gpu):
    hop, P0, P1 = 512, 200, 240
    cfg = config.spectrum_config(window_size=4096, hop=hop, axis_points=P0)
    x = synth.gen(47, 48000, hop * 10, 2)
    h = _create(cfg)
    try:
        _push_all(h, x[:, :hop * 6], hop)                      # six columns in the queue, none popped
        _flush(h)
        dropped, refused = C.c_uint64(0), C.c_uint64(0)
        api.check(api.lib().sgz_spectrum_stats(h, C.byref(dropped), C.byref(refused)))
        stats = (dropped.value, refused.value)
        api.spectrum_resize(h, P1)
        buf, ap = np.zeros((P1, 4), np.uint8), C.c_uint32(0)
        assert api.lib().sgz_spectrum_pop_column(h, buf.ctypes.data_as(C.c_void_p), C.byref(ap)) == api.SGZ_EMPTY
        api.check(api.lib().sgz_spectrum_stats(h, C.byref(dropped), C.byref(refused)))
        assert (dropped.value, refused.value) == stats
        _push_all(h, x[:, hop * 6:], hop)
        assert _pop_all(h, P1, 4).shape == (4, P1)
    finally:
        api.lib().sgz_spectrum_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. tracker, line graph and RSNT

def test_line_graph_equals_a_fresh_handle(gpu):
    """LINE_GRAPH, FFT: after a resize (width) the first render_lines equals a fresh handle's of the new size fed the same audio"""
    P0, P1 = 200, 320
    over = dict(window_size=4096, hop=1024, display_mode=config.DISPLAY_LINE_GRAPH)
    x = synth.gen(29, 48000, 1024 * 10, 2)
    out0 = np.zeros((1, api.NUM_GRAPHS, P0, 2), np.float32)
    out = np.zeros((1, api.NUM_GRAPHS, P1, 2), np.float32)
    h = _create(config.spectrum_config(axis_points=P0, **over))
    try:
        _push_all(h, x[:, :4096], 1024)
        api.check(api.lib().sgz_spectrum_render_lines(h, None, out0.ctypes.data_as(C.c_void_p)))
        assert out0.any()
        _push_all(h, x[:, 4096:6144], 1024)
        api.spectrum_resize(h, P1)
        res = np.zeros((P1, 2), np.float32)
        for g in range(api.NUM_GRAPHS):
            api.check(api.lib().sgz_spectrum_line_results(h, 0, g, res.ctypes.data_as(C.c_void_p)))
            assert not res.any()
        _push_all(h, x[:, 6144:], 1024)
        api.check(api.lib().sgz_spectrum_render_lines(h, None, out.ctypes.data_as(C.c_void_p)))
        got = out.copy()
        api.check(api.lib().sgz_spectrum_render_lines(h, None, out.ctypes.data_as(C.c_void_p)))
        got2 = out.copy()
    finally:
        api.lib().sgz_spectrum_destroy(h)
    h = _create(config.spectrum_config(axis_points=P1, **over))
    try:
        _push_all(h, x, 1024)
        api.check(api.lib().sgz_spectrum_render_lines(h, None, out.ctypes.data_as(C.c_void_p)))
        want = out.copy()
        api.check(api.lib().sgz_spectrum_render_lines(h, None, out.ctypes.data_as(C.c_void_p)))
        want2 = out.copy()
    finally:
        api.lib().sgz_spectrum_destroy(h)
    assert got.any()
    assert np.array_equal(got, want) and np.array_equal(got2, want2)


def test_line_graph_handle_takes_no_image(gpu):
    P = 200
    h = _create(config.spectrum_config(window_size=4096, hop=512, axis_points=P, display_mode=config.DISPLAY_LINE_GRAPH))
    try:
        buf = _Buf(300 * 32 // 4, gpu, seed=11)
        raw = buf.raw()
        assert api.lib().sgz_spectrum_resize(h, 300, C.c_void_p(buf.ptr), 8, 32) == api.SGZ_EINVAL
        assert np.array_equal(buf.raw(), raw)
        api.spectrum_resize(h, 300)
    finally:
        api.lib().sgz_spectrum_destroy(h)


def test_tracker_equals_a_fresh_handle(gpu):
    P0, P1 = 200, 480
    over = dict(window_size=4096, hop=512)
    x = synth.gen(23, 48000, 512 * 12, 2)
    peaks = []
    for P, switch in ((P0, True), (P1, False)):
        h = _create(config.spectrum_config(axis_points=P, **over))
        try:
            _push_all(h, x, 512)
            _pop_all(h, P, 10)
            if switch:
                api.spectrum_resize(h, P1)
            res = []
            for mouse in (0.1, 0.37, 0.8):
                pk = api.Peak()
                api.check(api.lib().sgz_spectrum_track_peak(h, 0, mouse, C.byref(pk)))
                res.append(bytes(pk))
            peaks.append(res)
        finally:
            api.lib().sgz_spectrum_destroy(h)
    assert peaks[0] == peaks[1]


def test_colour_line_results_read_zeros_until_the_next_frame(gpu):
    over = dict(window_size=4096, hop=512)
    x = synth.gen(31, 48000, 512 * 10, 2)
    h = _create(config.spectrum_config(axis_points=200, **over))
    try:
        res = np.zeros((200, 2), np.float32)
        _push_all(h, x[:, :512 * 6], 512)
        _pop_all(h, 200, 6)
        api.check(api.lib().sgz_spectrum_line_results(h, 0, 0, res.ctypes.data_as(C.c_void_p)))
        assert res.any()
        api.spectrum_resize(h, 256)
        res = np.zeros((256, 2), np.float32)
        for g in range(api.NUM_GRAPHS):
            api.check(api.lib().sgz_spectrum_line_results(h, 0, g, res.ctypes.data_as(C.c_void_p)))
            assert not res.any()
        _push_all(h, x[:, 512 * 6:], 512)
        _pop_all(h, 256, 4)
        api.check(api.lib().sgz_spectrum_line_results(h, 0, 0, res.ctypes.data_as(C.c_void_p)))
        assert res.any()
    finally:
        api.lib().sgz_spectrum_destroy(h)


@pytest.mark.parametrize("mode", [config.CH_SEPARATE, config.CH_PHASE])
def test_resonators_restart_at_rest(gpu, mode):
    P0, P1, hop = 200, 256, 1024
    over = dict(algorithm=config.ALGO_RSNT, window_size=4096, hop=hop, channel_mode=mode)
    x = synth.gen(37, 48000, hop * 12, 2)
    h = _create(config.spectrum_config(axis_points=P0, **over))
    try:
        _push_all(h, x[:, :hop * 5], 256)                      # five frames: the next push starts on a frame boundary
        _pop_all(h, P0, 5)
        api.spectrum_resize(h, P1)
        _push_all(h, x[:, hop * 5:], 256)
        got = _pop_all(h, P1, 7)
    finally:
        api.lib().sgz_spectrum_destroy(h)
    h = _create(config.spectrum_config(axis_points=P1, **over))
    try:
        _push_all(h, x[:, hop * 5:], 256)
        want = _pop_all(h, P1, 7)
    finally:
        api.lib().sgz_spectrum_destroy(h)
    assert np.array_equal(got, want), int((got != want).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. robustness

def test_invalid_arguments_change_nothing(gpu):
    hop, P, C0 = 512, 200, 12
    cfg = config.spectrum_config(window_size=4096, hop=hop, axis_points=P)
    x = synth.gen(47, 48000, hop * 10, 2)
    results = []
    for call in (True, False):
        h = _create(cfg)
        try:
            sp = _pitch(C0, 1)
            img = _Buf(P * sp // 4, gpu, seed=9)
            spare = _Buf(4096, gpu, seed=10)
            api.check(api.lib().sgz_spectrum_bind_image(h, img.ptr, C0, sp))
            _push_all(h, x[:, :hop * 4], hop)
            _flush_columns(h, 4)
            _push_all(h, x[:, hop * 4:hop * 6], hop)           # two columns queued
            if call:
                before, spare_before = img.raw(), spare.raw()
                L = api.lib()
                s = spare.ptr
                for args in ((1, None, 0, 0), (0, None, 0, 0), ((1 << 20) + 1, None, 0, 0), (240, s + 2, 8, 32), (240, s, 8, 28),
                             (240, s, 8, 34), (240, s, 0, 32)):
                    assert L.sgz_spectrum_resize(h, args[0], C.c_void_p(args[1]) if args[1] else None, args[2], args[3]) == api.SGZ_EINVAL, args
                assert np.array_equal(img.raw(), before) and np.array_equal(spare.raw(), spare_before)
            _push_all(h, x[:, hop * 6:], hop)
            _flush_columns(h, 6)
            pk = api.Peak()
            api.check(api.lib().sgz_spectrum_track_peak(h, 0, 0.4, C.byref(pk)))
            res = np.zeros((P, 2), np.float32)
            api.check(api.lib().sgz_spectrum_line_results(h, 0, 1, res.ctypes.data_as(C.c_void_p)))
            results.append((img.raw(), bytes(pk), res))
        finally:
            api.lib().sgz_spectrum_destroy(h)
    assert np.array_equal(results[0][0], results[1][0]) and results[0][1] == results[1][1]
    assert np.array_equal(results[0][2], results[1][2])


def test_own_image_interior_pointer_is_refused(gpu):
    """a new image that starts inside the library's own image (which the call would free after the move) is refused"""
    P, columns = 200, 24
    h = _create(config.spectrum_config(window_size=4096, hop=512, axis_points=P))
    try:
        d_img, pitch = C.c_void_p(), C.c_size_t(0)
        api.check(api.lib().sgz_spectrum_create_image(h, columns, C.byref(d_img), C.byref(pitch), None))
        L = api.lib()
        assert L.sgz_spectrum_resize(h, P, C.c_void_p(d_img.value + pitch.value), columns, pitch.value) == api.SGZ_EINVAL
        _push_all(h, synth.gen(49, 48000, 512 * 9, 2), 512)
        _flush_columns(h, 9)                                    # (the binding stands)
    finally:
        api.lib().sgz_spectrum_destroy(h)


def test_push_is_refused_or_taken_while_the_size_changes(gpu):
    """a producer thread pushes while the consumer resizes back and forth: every push returns SGZ_OK or SGZ_BUSY, and afterwards the
    history is exactly the accepted blocks (the tracker equals a fresh handle fed them)"""
    block = 256
    over = dict(window_size=4096, hop=512)
    sizes = [200, 333, 200, 120]
    x = synth.gen(59, 48000, block * 400, 2)
    h = _create(config.spectrum_config(axis_points=sizes[0], **over))
    accepted, statuses = [], []
    stop = threading.Event()

    def producer():
        for k in range(400):
            blk = np.ascontiguousarray(x[:, k * block:(k + 1) * block])
            ptrs = (C.c_void_p * 2)(blk[0].ctypes.data, blk[1].ctypes.data)
            st = api.lib().sgz_spectrum_push(h, ptrs, 2, block)
            statuses.append(st)
            if st == api.SGZ_OK:
                accepted.append(blk)
            time.sleep(0.0002)
        stop.set()

    try:
        t = threading.Thread(target=producer)
        t.start()
        n = 0
        buf, ap = np.zeros((max(sizes), 4), np.uint8), C.c_uint32(0)
        while not stop.is_set():
            n += 1
            api.spectrum_resize(h, sizes[n % len(sizes)])
            while api.lib().sgz_spectrum_pop_column(h, buf.ctypes.data_as(C.c_void_p), C.byref(ap)) == api.SGZ_OK:
                assert ap.value == sizes[n % len(sizes)]
        t.join()
        final = sizes[n % len(sizes)]
        assert n >= 2
        assert set(statuses) <= {api.SGZ_OK, api.SGZ_BUSY}, set(statuses)
        assert accepted
        _flush(h)
        pk = api.Peak()
        api.check(api.lib().sgz_spectrum_track_peak(h, 0, 0.3, C.byref(pk)))
        got = bytes(pk)
    finally:
        api.lib().sgz_spectrum_destroy(h)
    h = _create(config.spectrum_config(axis_points=final, **over))
    try:
        _push_all(h, np.concatenate(accepted, axis=1), block)
        pk = api.Peak()
        api.check(api.lib().sgz_spectrum_track_peak(h, 0, 0.3, C.byref(pk)))
        assert bytes(pk) == got
    finally:
        api.lib().sgz_spectrum_destroy(h)


def test_resize_cycles_give_memory_back(gpu):
    import torch

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    cfg = config.spectrum_config(window_size=4096, hop=512, axis_points=1024)
    x = synth.gen(61, 48000, 4096, 2)

    def cycle():
        h = _create(cfg)
        try:
            api.check(api.lib().sgz_spectrum_create_image(h, 512, C.byref(C.c_void_p()), C.byref(C.c_size_t(0)), None))
            _push_all(h, x, 512)
            t = torch.zeros((1080, 600), dtype=torch.int32, device=gpu)
            api.spectrum_resize(h, 1080, t, 600, 2400)             # the library's image moves into a caller's and is freed
            api.spectrum_resize(h, 1080, t, 512, 2400)             # in place
            api.spectrum_resize(h, 700)                            # binding dropped
            api.spectrum_resize(h, 1024, t, 600, 2400)             # bound afresh
            api.spectrum_resize(h, 1024)
            del t
        finally:
            api.lib().sgz_spectrum_destroy(h)

    cycle()
    f0 = free()
    for _ in range(10):
        cycle()
    f1 = free()
    assert f0 - f1 < (16 << 20), (f0 - f1)
