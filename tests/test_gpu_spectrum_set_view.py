"""sgz_spectrum_set_view: zoom / pan of a live spectrum handle (Spectrum::handleFlagUpdates' viewChanged branch, Spectrum.cpp:532-575).
New plans for the view, both line graphs cleared, the bound spectrogram image translated (freeLinearVerticalTranslation) -- and the audio
history, the frame cadence, the column queue and the image binding kept.  Every comparison is bit for bit."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

from signalizer_amd import api, config, synth

pytestmark = pytest.mark.gpu

def _table(P, ol, orr, nl, nr):
    """the translation rule of sgz.h in numpy (float64, the header's order of operations)"""
    i = np.arange(P, dtype=np.float64)
    u = nl + (nr - nl) * (i / (P - 1.0))
    r = (u - ol) / (orr - ol) * (P - 1.0)
    ok = (r >= -0.5) & (r <= P - 0.5)
    r = np.clip(r, 0.0, P - 1.0)
    j = np.floor(r)
    w = np.floor((r - j) * 256.0 + 0.5)
    j = np.where(w == 256.0, j + 1.0, j)
    w = np.where(w == 256.0, 0.0, w)
    return np.where(ok, j, -1).astype(np.int64), np.where(ok, w, 0).astype(np.uint32)


def _translate(img, columns, P, old, new):
    """numpy application of the table to a [P][pitch / 4] uint32 image: rows blended byte by byte, texels beyond `columns` kept"""
    src, w = _table(P, *old, *new)
    out = img.copy()
    j = np.clip(src, 0, P - 1)
    a = img[j, :columns].view(np.uint8).reshape(P, columns, 4).astype(np.uint32)
    b = img[np.minimum(j + 1, P - 1), :columns].view(np.uint8).reshape(P, columns, 4).astype(np.uint32)
    ww = w[:, None, None]
    blend = ((a * (256 - ww) + b * ww + 128) >> 8).astype(np.uint8)
    blend[src < 0] = 0
    out[:, :columns] = blend.reshape(P, columns * 4).view(np.uint32)
    return out


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


class _Image:
    """a bound image: caller-owned (a torch tensor, random texels, a pitch wider than the image) or the library's own"""

    def __init__(self, h, P, columns, own, gpu, seed=0):
        import torch
        self.P, self.columns, self.own = P, columns, own
        if own:
            d_img, pitch = C.c_void_p(), C.c_size_t(0)
            api.check(api.lib().sgz_spectrum_create_image(h, columns, C.byref(d_img), C.byref(pitch), None))
            self.ptr, self.pitch = d_img.value, pitch.value
        else:
            self.pitch = 4 * (columns + 3)
            rng = np.random.default_rng(seed)
            init = rng.integers(0, 2 ** 32, size=(P, self.pitch // 4), dtype=np.uint64).astype(np.uint32)
            self.t = torch.from_numpy(init.view(np.int32)).to(gpu)
            self.ptr = self.t.data_ptr()
            api.check(api.lib().sgz_spectrum_bind_image(h, self.ptr, columns, self.pitch))

    def read(self):
        import torch
        torch.cuda.synchronize()
        if not self.own:
            return self.t.cpu().numpy().view(np.uint32)
        host = np.zeros((self.P, self.pitch // 4), np.uint32)
        hip = C.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(self.ptr), C.c_size_t(host.nbytes), 2) == 0
        return host


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the stage call

@pytest.mark.parametrize("P", [2, 200, 1024, 2160])
@pytest.mark.parametrize("columns", [1, 7, 2048])
@pytest.mark.parametrize("wide", [False, True])
def test_stage_call_translates_an_image(gpu, P, columns, wide):
    import torch
    pitch = 4 * columns + (4 * 5 if wide else 0)
    rng = np.random.default_rng(P * 7 + columns)
    views = [((0.0, 1.0), (0.25, 0.75)), ((0.3, 0.6), (0.0, 1.0)), ((0.2, 0.6), (0.35, 0.75)), ((0.5, 1.0), (0.0, 0.5)),
             ((0.0, 1.0), (0.0, 1.0)), ((0.2, 0.6), (0.2 + 0.1 / (P - 1), 0.6 + 0.1 / (P - 1)))]
    for old, new in views:
        img = rng.integers(0, 2 ** 32, size=(P, pitch // 4), dtype=np.uint64).astype(np.uint32)
        t = torch.from_numpy(img.view(np.int32)).to(gpu)
        torch.cuda.synchronize()
        api.view_translate_device(t, columns, pitch, P, *old, *new)
        got = t.cpu().numpy().view(np.uint32)
        want = _translate(img, columns, P, old, new)
        assert np.array_equal(got, want), (old, new, int((got != want).sum()))
        assert np.array_equal(got[:, columns:], img[:, columns:])


def test_stage_call_refuses_bad_arguments(gpu):
    import torch
    t = torch.zeros((200, 8), dtype=torch.int32, device=gpu)
    L = api.lib()
    assert L.sgz_view_translate_device(C.c_void_p(t.data_ptr()), 8, 32, 200, 0.0, 1.0, 0.7, 0.2, None) == api.SGZ_EINVAL
    assert L.sgz_view_translate_device(C.c_void_p(t.data_ptr()), 8, 28, 200, 0.0, 1.0, 0.2, 0.7, None) == api.SGZ_EINVAL
    assert L.sgz_view_translate_device(C.c_void_p(t.data_ptr()), 8, 32, 1, 0.0, 1.0, 0.2, 0.7, None) == api.SGZ_EINVAL
    assert not t.any().item()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the history is kept

CASES = {
    # W = N = 32768, Separate, log view: (0, 1) runs the channel-split kernel, (0.995, 1) the fused one -- and back
    "cfg2-split-to-fused": (dict(window_size=32768, hop=8192, axis_points=1024), (0.0, 1.0), (0.995, 1.0), False),
    "cfg2-fused-to-split-own-image": (dict(window_size=32768, hop=8192, axis_points=1024), (0.995, 1.0), (0.1, 0.9), True),
    "w4096-separate": (dict(window_size=4096, hop=512, axis_points=200), (0.0, 1.0), (0.2, 0.7), False),
    "w4096-complex": (dict(window_size=4096, hop=512, axis_points=200, channel_mode=config.CH_COMPLEX), (0.1, 0.9), (0.0, 0.5), False),
    "w4096-phase": (dict(window_size=4096, hop=512, axis_points=200, channel_mode=config.CH_PHASE), (0.0, 1.0), (0.3, 0.6), True),
    "w4096-own-image": (dict(window_size=4096, hop=512, axis_points=200), (0.4, 0.6), (0.0, 1.0), True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_history_is_kept(gpu, case):
    import torch
    over, old, new, own = CASES[case]
    cfg_old = config.spectrum_config(view_left=old[0], view_right=old[1], **over)
    cfg_new = config.spectrum_config(view_left=new[0], view_right=new[1], **over)
    W, hop, P, columns = over["window_size"], over["hop"], over["axis_points"], 24
    if case.startswith("cfg2"):
        # the switch of kernel family this case is for: SGZ_PATH_CHANNEL_SPLIT (8) on one side only
        assert bool(api.Plan(cfg_old).path & 8) != bool(api.Plan(cfg_new).path & 8)
    x = synth.gen(17, 48000, hop * 19, 2)
    padded = np.ascontiguousarray(np.concatenate([np.zeros((2, W), np.float32), x], axis=1)[:, hop:])
    plan = api.Plan(cfg_new).upload()
    want = plan.render(torch.from_numpy(np.ascontiguousarray(padded[:, 8 * hop:])).to(gpu)).cpu().numpy().view(np.uint32)[:, :, 0]
    assert want.shape[0] == 11

    h = _create(cfg_old)
    try:
        img = _Image(h, P, columns, own, gpu, seed=3)
        _push_all(h, x[:, :8 * hop], hop)
        _flush_columns(h, 8)
        before = img.read()
        api.spectrum_set_view(h, *new)
        after = img.read()
        assert np.array_equal(after, _translate(before, columns, P, old, new))
        assert not np.array_equal(after, before)
        for k in range(8, 19):                                 # (one flush per column: the queue holds 10, SpectrumDSP.cpp:47)
            _push_all(h, x[:, k * hop:(k + 1) * hop], hop)
            _flush_columns(h, 1)
        got = img.read()
        assert np.array_equal(got[:, 8:19].T, want), int((got[:, 8:19].T != want).sum())
        assert np.array_equal(got[:, :8], after[:, :8]) and np.array_equal(got[:, 19:], after[:, 19:])
    finally:
        api.lib().sgz_spectrum_destroy(h)

    # the same columns through sgz_spectrum_configure: the history went back to silence, so they differ
    h = _create(cfg_old)
    try:
        _push_all(h, x[:, :8 * hop], hop)
        _pop_all(h, P, 8)
        c = api.config_from_dict(cfg_new)
        api.check(api.lib().sgz_spectrum_configure(h, C.byref(c)))
        other = []
        for k in range(8, 19):
            _push_all(h, x[:, k * hop:(k + 1) * hop], hop)
            other.append(_pop_all(h, P, 1)[0])
        other = np.stack(other)
        assert not np.array_equal(other, want)
    finally:
        api.lib().sgz_spectrum_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. tracker and line graph

def test_tracker_follows_the_new_view(gpu):
    old, new = (0.0, 1.0), (0.1, 0.4)
    over = dict(window_size=4096, hop=512, axis_points=200)
    x = synth.gen(23, 48000, 512 * 12, 2)
    peaks = []
    for view, switch in ((old, True), (new, False)):
        h = _create(config.spectrum_config(view_left=view[0], view_right=view[1], **over))
        try:
            _push_all(h, x, 512)
            _pop_all(h, 200, 10)
            if switch:
                api.spectrum_set_view(h, *new)
            res = []
            for mouse in (0.1, 0.37, 0.8):
                pk = api.Peak()
                api.check(api.lib().sgz_spectrum_track_peak(h, 0, mouse, C.byref(pk)))
                res.append(bytes(pk))
            peaks.append(res)
        finally:
            api.lib().sgz_spectrum_destroy(h)
    assert peaks[0] == peaks[1]


@pytest.mark.parametrize("algorithm", [config.ALGO_FFT, config.ALGO_RSNT])
def test_line_graph_restarts_from_zero(gpu, algorithm):
    """LINE_GRAPH: after set_view the results read zeros, and the first render_lines equals a fresh handle's first one (FFT: fed the same
    audio; RSNT: fed only the audio pushed after the call -- the resonators restart at rest)"""
    old, new = (0.0, 1.0), (0.3, 0.9)
    over = dict(window_size=4096, hop=1024, axis_points=200, display_mode=config.DISPLAY_LINE_GRAPH, algorithm=algorithm)
    x = synth.gen(29, 48000, 1024 * 10, 2)
    P = 200
    out = np.zeros((1, api.NUM_GRAPHS, P, 2), np.float32)
    firsts = []
    for view, switch in ((old, True), (new, False)):
        h = _create(config.spectrum_config(view_left=view[0], view_right=view[1], **over))
        try:
            if switch:
                _push_all(h, x[:, :4096], 1024)
                api.check(api.lib().sgz_spectrum_render_lines(h, None, out.ctypes.data_as(C.c_void_p)))
                assert out.any()
                _push_all(h, x[:, 4096:6144], 1024)
                api.spectrum_set_view(h, *new)
                res = np.zeros((P, 2), np.float32)
                for g in range(api.NUM_GRAPHS):
                    api.check(api.lib().sgz_spectrum_line_results(h, 0, g, res.ctypes.data_as(C.c_void_p)))
                    assert not res.any()
                _push_all(h, x[:, 6144:], 1024)
            else:
                _push_all(h, x if algorithm == config.ALGO_FFT else x[:, 6144:], 1024)
            api.check(api.lib().sgz_spectrum_render_lines(h, None, out.ctypes.data_as(C.c_void_p)))
            firsts.append(out.copy())
        finally:
            api.lib().sgz_spectrum_destroy(h)
    assert firsts[0].any()
    assert np.array_equal(firsts[0], firsts[1])


def test_colour_line_results_read_zeros_until_the_next_frame(gpu):
    over = dict(window_size=4096, hop=512, axis_points=200)
    x = synth.gen(31, 48000, 512 * 10, 2)
    h = _create(config.spectrum_config(**over))
    try:
        res = np.zeros((200, 2), np.float32)
        _push_all(h, x[:, :512 * 6], 512)
        _pop_all(h, 200, 6)
        api.check(api.lib().sgz_spectrum_line_results(h, 0, 0, res.ctypes.data_as(C.c_void_p)))
        assert res.any()
        api.spectrum_set_view(h, 0.2, 0.5)
        api.check(api.lib().sgz_spectrum_line_results(h, 0, 0, res.ctypes.data_as(C.c_void_p)))
        assert not res.any()
        _push_all(h, x[:, 512 * 6:], 512)
        _pop_all(h, 200, 4)
        api.check(api.lib().sgz_spectrum_line_results(h, 0, 0, res.ctypes.data_as(C.c_void_p)))
        assert res.any()
    finally:
        api.lib().sgz_spectrum_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. RSNT

@pytest.mark.parametrize("mode", [config.CH_SEPARATE, config.CH_PHASE])
def test_resonators_restart_at_rest(gpu, mode):
    old, new = (0.0, 1.0), (0.2, 0.8)
    hop, P = 1024, 200
    over = dict(algorithm=config.ALGO_RSNT, window_size=4096, hop=hop, axis_points=P, channel_mode=mode)
    x = synth.gen(37, 48000, hop * 12, 2)
    h = _create(config.spectrum_config(view_left=old[0], view_right=old[1], **over))
    try:
        _push_all(h, x[:, :hop * 5], 256)                      # five frames: the next push starts on a frame boundary
        _pop_all(h, P, 5)
        api.spectrum_set_view(h, *new)
        _push_all(h, x[:, hop * 5:], 256)
        got = _pop_all(h, P, 7)
    finally:
        api.lib().sgz_spectrum_destroy(h)
    h = _create(config.spectrum_config(view_left=new[0], view_right=new[1], **over))
    try:
        _push_all(h, x[:, hop * 5:], 256)
        want = _pop_all(h, P, 7)
    finally:
        api.lib().sgz_spectrum_destroy(h)
    assert np.array_equal(got, want), int((got != want).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. queue and edge cases

def test_queued_columns_land_untranslated_after_the_translation(gpu):
    old, new = (0.0, 1.0), (0.25, 0.6)
    hop, P, columns = 512, 200, 16
    cfg = config.spectrum_config(window_size=4096, hop=hop, axis_points=P)
    x = synth.gen(41, 48000, hop * 8, 2)
    ref = _create(cfg)
    try:
        _push_all(ref, x, hop)
        want = _pop_all(ref, P, 8)                             # the old view's columns
    finally:
        api.lib().sgz_spectrum_destroy(ref)
    h = _create(cfg)
    try:
        img = _Image(h, P, columns, False, gpu, seed=5)
        _push_all(h, x[:, :hop * 5], hop)
        _flush_columns(h, 5)
        _push_all(h, x[:, hop * 5:], hop)                      # three columns wait in the queue
        before = img.read()
        api.spectrum_set_view(h, *new)
        after = img.read()
        assert np.array_equal(after, _translate(before, columns, P, old, new))
        _flush_columns(h, 3)
        got = img.read()
        assert np.array_equal(got[:, 5:8].T, want[5:8])
        assert np.array_equal(got[:, :5], after[:, :5]) and np.array_equal(got[:, 8:], after[:, 8:])
    finally:
        api.lib().sgz_spectrum_destroy(h)


def test_unchanged_rect_keeps_the_image_and_zeroes_the_states(gpu):
    hop, P, columns = 512, 200, 12
    cfg = config.spectrum_config(window_size=4096, hop=hop, axis_points=P, view_left=0.1, view_right=0.9)
    x = synth.gen(43, 48000, hop * 10, 2)
    h = _create(cfg)
    try:
        img = _Image(h, P, columns, False, gpu, seed=7)
        _push_all(h, x[:, :hop * 4], hop)
        _flush_columns(h, 4)
        before = img.read()
        api.spectrum_set_view(h, 0.1, 0.9)
        assert np.array_equal(img.read(), before)
        res = np.zeros((P, 2), np.float32)
        api.check(api.lib().sgz_spectrum_line_results(h, 0, 1, res.ctypes.data_as(C.c_void_p)))
        assert not res.any()
        _push_all(h, x[:, hop * 4:], hop)
        _flush_columns(h, 6)
        got = img.read()
    finally:
        api.lib().sgz_spectrum_destroy(h)
    # the columns after the call: those of a handle whose decay states were cleared at that point (clear_state)
    h = _create(cfg)
    try:
        _push_all(h, x[:, :hop * 4], hop)
        _pop_all(h, P, 4)
        api.check(api.lib().sgz_spectrum_clear_state(h))
        _push_all(h, x[:, hop * 4:], hop)
        want = _pop_all(h, P, 6)
    finally:
        api.lib().sgz_spectrum_destroy(h)
    assert np.array_equal(got[:, 4:10].T, want)


def test_invalid_view_changes_nothing(gpu):
    hop, P, columns = 512, 200, 12
    cfg = config.spectrum_config(window_size=4096, hop=hop, axis_points=P, view_left=0.1, view_right=0.9)
    x = synth.gen(47, 48000, hop * 10, 2)
    imgs = []
    for call in (True, False):
        h = _create(cfg)
        try:
            img = _Image(h, P, columns, False, gpu, seed=9)
            _push_all(h, x[:, :hop * 4], hop)
            _flush_columns(h, 4)
            if call:
                before = img.read()
                for l, r in ((0.5, 0.5), (0.6, 0.2), (-0.1, 0.5), (0.2, 1.1), (float("nan"), 0.5), (0.1, float("inf"))):
                    assert api.lib().sgz_spectrum_set_view(h, l, r) == api.SGZ_EINVAL
                assert np.array_equal(img.read(), before)
            _push_all(h, x[:, hop * 4:], hop)
            _flush_columns(h, 6)
            pk = api.Peak()
            api.check(api.lib().sgz_spectrum_track_peak(h, 0, 0.4, C.byref(pk)))
            imgs.append((img.read(), bytes(pk)))
        finally:
            api.lib().sgz_spectrum_destroy(h)
    assert np.array_equal(imgs[0][0], imgs[1][0]) and imgs[0][1] == imgs[1][1]


def test_line_graph_handle_has_no_translation(gpu):
    P, columns = 200, 8
    cfg = config.spectrum_config(window_size=4096, hop=512, axis_points=P, display_mode=config.DISPLAY_LINE_GRAPH)
    h = _create(cfg)
    try:
        img = _Image(h, P, columns, False, gpu, seed=11)
        _push_all(h, synth.gen(53, 48000, 4096, 2), 512)
        before = img.read()
        api.spectrum_set_view(h, 0.2, 0.4)
        assert np.array_equal(img.read(), before)
    finally:
        api.lib().sgz_spectrum_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. concurrency and lifetime

def test_push_is_refused_or_taken_while_the_view_changes(gpu):
    """a producer thread pushes while the consumer zooms back and forth: every push returns SGZ_OK or SGZ_BUSY, and afterwards the
    history is exactly the accepted blocks (the tracker equals a fresh handle fed them)"""
    block, P = 256, 200
    over = dict(window_size=4096, hop=512, axis_points=P)
    views = [(0.0, 1.0), (0.2, 0.7), (0.05, 0.3)]
    x = synth.gen(59, 48000, block * 400, 2)
    h = _create(config.spectrum_config(**over))
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
        buf, ap = np.zeros((P, 4), np.uint8), C.c_uint32(0)
        while not stop.is_set():
            api.spectrum_set_view(h, *views[n % len(views)])
            n += 1
            while api.lib().sgz_spectrum_pop_column(h, buf.ctypes.data_as(C.c_void_p), C.byref(ap)) == api.SGZ_OK:
                pass
        t.join()
        api.spectrum_set_view(h, *views[n % len(views)])
        final = views[n % len(views)]
        assert n >= 2
        assert set(statuses) <= {api.SGZ_OK, api.SGZ_BUSY}, set(statuses)
        assert accepted
        _flush(h)
        pk = api.Peak()
        api.check(api.lib().sgz_spectrum_track_peak(h, 0, 0.3, C.byref(pk)))
        got = bytes(pk)
    finally:
        api.lib().sgz_spectrum_destroy(h)
    h = _create(config.spectrum_config(view_left=final[0], view_right=final[1], **over))
    try:
        _push_all(h, np.concatenate(accepted, axis=1), block)
        pk = api.Peak()
        api.check(api.lib().sgz_spectrum_track_peak(h, 0, 0.3, C.byref(pk)))
        assert bytes(pk) == got
    finally:
        api.lib().sgz_spectrum_destroy(h)


def test_set_view_cycles_give_memory_back(gpu):
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
            for v in ((0.2, 0.8), (0.0, 1.0), (0.4, 0.45)):
                api.spectrum_set_view(h, *v)
            t = torch.zeros((1024, 256), dtype=torch.int32, device=gpu)
            api.check(api.lib().sgz_spectrum_bind_image(h, t.data_ptr(), 256, 1024))
            api.spectrum_set_view(h, 0.1, 0.3)
            del t
        finally:
            api.lib().sgz_spectrum_destroy(h)

    cycle()
    f0 = free()
    for _ in range(10):
        cycle()
    f1 = free()
    assert f0 - f1 < (16 << 20), (f0 - f1)
