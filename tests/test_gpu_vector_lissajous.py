"""The Vectorscope's Lissajous display mode (drawRectPlot, VectorscopeRendering.cpp:444-497) and stereo meter readout (drawStereoMeters,
:748-823) on the real-time handle and as a stateless stage: sgz_vector_lissajous_*, sgz_vector_meters.

The reference side is a plain fp32 restatement (numpy float32) fed from the handle's own parity hook, sgz_vector_history (ring +
cursor; tests/test_gpu_vector_stream.py holds those to the oracle).  vertex v of pair p = (right, left, fade - 1), fade = (float) v *
sampleFade, sampleFade = 1 / max(1, n - 1); colour = colours[p] * fade with fade_history, colours[p] without.  Every bar is bit for bit."""
import ctypes as C
import threading

import numpy as np
import pytest

from signalizer_amd import api, synth

pytestmark = pytest.mark.gpu

SR = 96000.0
F32 = np.float32
COLOURS = [(1.0, 0.5, 0.25), (0.2, 0.9, 0.4), (0.3, 0.3, 1.0), (0.7, 0.1, 0.6)]


def _push(dev, blk):
    while True:
        st = dev.push(np.ascontiguousarray(blk))
        if st == api.SGZ_OK:
            return
        assert st == api.SGZ_BUSY


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def lissajous_ref(left_mem, right_mem, cursor, fade, colour):
    """drawRectPlot over the ring as the polar stream reads it: [cursor, n) then [0, cursor)"""
    n = left_mem.shape[0]
    order = np.concatenate([np.arange(cursor, n), np.arange(0, cursor)])
    sample_fade = F32(1.0) / F32(max(1, n - 1))
    f = np.arange(n).astype(F32) * sample_fade                  # size_t -> float: round to nearest, then one fp32 product
    xyz = np.stack([right_mem[order], left_mem[order], f - F32(1.0)], axis=1).astype(F32)
    col = np.asarray(colour, F32)
    rgb = f[:, None] * col[None, :] if fade else np.broadcast_to(col, (n, 3))
    return xyz, np.ascontiguousarray(rgb, F32)


def _ref_from_handle(dev, pair, fade, colour):
    left, cur = dev.history(2 * pair)
    right, cur2 = dev.history(2 * pair + 1)
    assert cur == cur2
    return lissajous_ref(left, right, cur, fade, colour)


def _vector(channels, size, env_mode=1, fade=1, max_block=4096):
    return api.Vector(sample_rate=SR, num_channels=channels, window_size=size, envelope_mode=env_mode, lanes=8, fade_history=fade,
                      max_block=max_block, envelope_window=0.3, stereo_window=0.05, colours=COLOURS)


@pytest.mark.parametrize("env_mode", [0, 1, 2])
@pytest.mark.parametrize("fade", [0, 1])
@pytest.mark.parametrize("size", [1, 2, 13, 777, 9600, 65536])
@pytest.mark.parametrize("channels", [2, 8])
def test_handle_against_the_restatement(gpu, channels, size, fade, env_mode):
    """random block sizes (one longer than the window: the cursor lands mid-ring), reads before and after the ring has wrapped"""
    max_block = min(131072, 2 * size + 64)
    dev = _vector(channels, size, env_mode, fade, max_block)
    rng = np.random.default_rng(channels * 1000003 + size * 7 + fade * 3 + env_mode)
    x = synth.gen(int(size) % 97 + 3, SR, 4 * max_block + 8 * size, channels)
    pairs = channels // 2
    pos = 0
    first = max(1, size // 3)                                  # a read while most of the ring still holds its zeros
    plan = [[first], [int(rng.integers(1, max_block + 1)) for _ in range(3)], [size + 1 + int(rng.integers(0, min(size, max_block - size - 1) + 1))],
            [int(rng.integers(1, max(2, size // 2) + 1)) for _ in range(2)]]
    for rnd, blocks in enumerate(plan):
        for n in blocks:
            n = min(n, max_block)
            _push(dev, x[:, pos:pos + n]); pos += n
        if rnd % 2 == 0:
            xyz, rgb = dev.lissajous_all()
        else:
            got = [dev.lissajous(p) for p in range(pairs)]
            xyz, rgb = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
        for p in range(pairs):
            wx, wc = _ref_from_handle(dev, p, fade, COLOURS[p])
            assert np.array_equal(_bits(xyz[p]), _bits(wx)), (rnd, p, int((_bits(xyz[p]) != _bits(wx)).sum()))
            assert np.array_equal(_bits(rgb[p]), _bits(wc)), (rnd, p)
    dev.close()


def test_fade_rounds_above_2_to_24(gpu):
    """window 2^24 + 3: (float) v rounds for odd v past 2^24 -- z and the faded colours at the top of the strip stay the reference's"""
    import torch
    size = (1 << 24) + 3
    dev = _vector(2, size, 0, 1, 131072)
    x = synth.gen(31, SR, 3 * 131072, 2)
    for pos in range(0, x.shape[1], 131072):
        _push(dev, x[:, pos:pos + 131072])
    d_xyz = torch.full((size, 3), float("nan"), dtype=torch.float32, device=gpu)
    d_rgb = torch.full((size, 3), float("nan"), dtype=torch.float32, device=gpu)
    cnt = C.c_uint32(size)
    dev.flush()
    api.check(api.lib().sgz_vector_lissajous_vertices_device(dev.h, 0, C.c_void_p(d_xyz.data_ptr()), C.c_void_p(d_rgb.data_ptr()), C.byref(cnt)))
    assert cnt.value == size
    left, cur = dev.history(0)
    right, _ = dev.history(1)
    assert cur == 3 * 131072
    wx, wc = lissajous_ref(left, right, cur, 1, COLOURS[0])
    z = d_xyz[:, 2].cpu().numpy()
    assert np.array_equal(_bits(z), _bits(wx[:, 2]))
    top = slice(size - 65536, size)
    v = np.arange(size - 65536, size)
    assert (v.astype(F32).astype(np.int64) != v).any()        # the conversion does round here
    assert np.array_equal(_bits(d_xyz[top].cpu().numpy()), _bits(wx[top]))
    assert np.array_equal(_bits(d_rgb[top].cpu().numpy()), _bits(wc[top]))
    dev.close()


def test_all_equals_per_pair_calls_in_every_destination(gpu):
    """cfg4's shape (8 channels, 96 kHz, 9600-sample window): lissajous_vertices_all into pageable host, pinned device-mapped host and
    device memory writes the bytes of one sgz_vector_lissajous_vertices call per pair"""
    import torch
    dev = _vector(8, 9600, 1, 1, 512)
    x = synth.gen(4, SR, 48000, 8)
    for pos in range(0, 47000, 480):
        _push(dev, x[:, pos:pos + 480])
    per = [dev.lissajous(p) for p in range(4)]
    want_xyz, want_rgb = np.stack([g[0] for g in per]), np.stack([g[1] for g in per])
    h_xyz, h_rgb = dev.lissajous_all()
    assert np.array_equal(_bits(h_xyz), _bits(want_xyz)) and np.array_equal(_bits(h_rgb), _bits(want_rgb))
    pin = lambda: torch.full((4, 9600, 3), float("nan"), dtype=torch.float32).pin_memory()
    p_xyz, p_rgb = pin(), pin()
    dev.lissajous_all(p_xyz, p_rgb)
    assert np.array_equal(_bits(p_xyz.numpy()), _bits(want_xyz)) and np.array_equal(_bits(p_rgb.numpy()), _bits(want_rgb))
    d_xyz = torch.full((4, 9600, 3), float("nan"), dtype=torch.float32, device=gpu)
    d_rgb = torch.full((4, 9600, 3), float("nan"), dtype=torch.float32, device=gpu)
    dev.lissajous_all(d_xyz, d_rgb)
    assert np.array_equal(_bits(d_xyz.cpu().numpy()), _bits(want_xyz)) and np.array_equal(_bits(d_rgb.cpu().numpy()), _bits(want_rgb))
    d_only = torch.full((4, 9600, 3), float("nan"), dtype=torch.float32, device=gpu)
    dev.lissajous_all(d_only, None)                                   # no colours asked for
    assert np.array_equal(_bits(d_only.cpu().numpy()), _bits(want_xyz))
    for p in range(4):                                                # the device form of the per-pair call
        dx = torch.full((9600, 3), float("nan"), dtype=torch.float32, device=gpu)
        dc = torch.full((9600, 3), float("nan"), dtype=torch.float32, device=gpu)
        cnt = C.c_uint32(9600)
        api.check(api.lib().sgz_vector_lissajous_vertices_device(dev.h, p, C.c_void_p(dx.data_ptr()), C.c_void_p(dc.data_ptr()), C.byref(cnt)))
        assert np.array_equal(_bits(dx.cpu().numpy()), _bits(want_xyz[p])) and np.array_equal(_bits(dc.cpu().numpy()), _bits(want_rgb[p]))
    dev.close()


def test_polar_reads_are_unaffected(gpu):
    """polar -> Lissajous -> polar with no push between: the second polar result is the first's, byte for byte; again after a push"""
    dev = _vector(4, 3001, 1, 1, 2048)
    x = synth.gen(8, SR, 20000, 4)
    pos = 0
    for rnd in range(3):
        for n in (1500, 777, 2048)[: rnd + 1]:
            _push(dev, x[:, pos:pos + n]); pos += n
        a_xyz, a_rgb = dev.vertices_all()
        l_xyz, l_rgb = dev.lissajous_all()
        b_xyz, b_rgb = dev.vertices_all()
        assert np.array_equal(_bits(a_xyz), _bits(b_xyz)) and np.array_equal(_bits(a_rgb), _bits(b_rgb)), rnd
        for p in range(2):
            wx, wc = _ref_from_handle(dev, p, 1, COLOURS[p])
            assert np.array_equal(_bits(l_xyz[p]), _bits(wx)) and np.array_equal(_bits(l_rgb[p]), _bits(wc))
            s_xyz, s_rgb = dev.vertices(p)                              # the per-pair polar call after a Lissajous read
            assert np.array_equal(_bits(s_xyz), _bits(a_xyz[p])) and np.array_equal(_bits(s_rgb), _bits(a_rgb[p]))
    dev.close()


@pytest.mark.parametrize("option", [api.RT_OPT_PARK_PUSHES, api.RT_OPT_DEFER_SUBMIT])
def test_parked_blocks_reach_the_lissajous_read(gpu, option):
    """flush on read: with every push parked in the host FIFO (or left in the open batch), a Lissajous read -- the C call alone, no flush
    before it -- sees every block pushed so far"""
    channels, size = 4, 3000
    dev = _vector(channels, size, 1, 1, 1024).set_option(option, 1)
    x = synth.gen(19, SR, 30000, channels)
    mem = np.zeros((channels, size), F32)
    cursor, pos = 0, 0
    rng = np.random.default_rng(option)
    L = api.lib()
    for rnd in range(5):
        for _ in range(int(rng.integers(1, 24))):
            n = int(rng.integers(1, 1024))
            blk = np.ascontiguousarray(x[:, pos:pos + n])
            if blk.shape[1] == 0:
                break
            _push(dev, blk)
            mem[:, (cursor + np.arange(blk.shape[1])) % size] = blk
            cursor = (cursor + blk.shape[1]) % size
            pos += blk.shape[1]
        xyz = np.zeros((channels // 2, size, 3), F32)
        rgb = np.zeros((channels // 2, size, 3), F32)
        cnt = C.c_uint32(size)
        if rnd % 2:
            api.check(L.sgz_vector_lissajous_vertices_all(dev.h, api._np_ptr(xyz), api._np_ptr(rgb), C.byref(cnt)))
        else:
            for p in range(channels // 2):
                cnt = C.c_uint32(size)
                api.check(L.sgz_vector_lissajous_vertices(dev.h, p, api._np_ptr(xyz[p]), api._np_ptr(rgb[p]), C.byref(cnt)))
        for p in range(channels // 2):
            wx, wc = lissajous_ref(mem[2 * p], mem[2 * p + 1], cursor, 1, COLOURS[p])
            assert np.array_equal(_bits(xyz[p]), _bits(wx)), (rnd, p)
            assert np.array_equal(_bits(rgb[p]), _bits(wc)), (rnd, p)
    dev.close()


def test_stage_call(gpu):
    """sgz_vector_lissajous_device on caller-owned device memory: NaN payloads, infinities and -0 pass through as they are; d_rgb NULL"""
    import torch
    L = api.lib()
    rng = np.random.default_rng(3)
    for pairs, n, stride in [(3, 1000, 1024), (1, 1, 1), (2, 2, 5), (33, 300, 300)]:
        planar = rng.standard_normal((2 * pairs, stride)).astype(F32)
        specials = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -3e38], F32)
        bits = specials.view(np.uint32).copy()
        bits[0] = 0x7FC12345                                            # a quiet NaN with a payload
        specials = bits.view(F32)
        flat = planar.reshape(-1)
        idx = rng.choice(flat.size, size=min(flat.size, 64), replace=False)
        flat[idx] = specials[np.arange(idx.size) % specials.size]
        cols = rng.random((pairs, 3)).astype(F32)
        d = torch.from_numpy(planar).to(gpu)
        stream = torch.cuda.current_stream().cuda_stream
        for fade in (0, 1):
            d_xyz = torch.full((pairs, n, 3), float("nan"), dtype=torch.float32, device=gpu)
            d_rgb = torch.full((pairs, n, 3), float("nan"), dtype=torch.float32, device=gpu)
            api.check(L.sgz_vector_lissajous_device(d.data_ptr(), stride, pairs, n, fade, api._np_ptr(cols), d_xyz.data_ptr(), d_rgb.data_ptr(), stream))
            d_x2 = torch.full((pairs, n, 3), float("nan"), dtype=torch.float32, device=gpu)
            api.check(L.sgz_vector_lissajous_device(d.data_ptr(), stride, pairs, n, fade, None, d_x2.data_ptr(), None, stream))
            torch.cuda.synchronize()
            gx, gc, gx2 = d_xyz.cpu().numpy(), d_rgb.cpu().numpy(), d_x2.cpu().numpy()
            for p in range(pairs):
                wx, wc = lissajous_ref(planar[2 * p, :n], planar[2 * p + 1, :n], 0, fade, cols[p])
                assert np.array_equal(_bits(gx[p]), _bits(wx)), (pairs, n, fade, p)
                assert np.array_equal(_bits(gc[p]), _bits(wc)), (pairs, n, fade, p)
                assert np.array_equal(_bits(gx2[p]), _bits(wx)), (pairs, n, fade, p)


def test_meters_on_the_handle(gpu):
    """sgz_vector_meters = sgz_vector_meters_from_filters(sgz_vector_filters_get(...)) after random pushes"""
    dev = _vector(4, 4800, 1, 1, 2048)
    x = synth.gen(21, SR, 40000, 4)
    rng = np.random.default_rng(21)
    pos = 0
    for rnd in range(6):
        for _ in range(int(rng.integers(1, 6))):
            n = int(rng.integers(1, 2048))
            _push(dev, x[:, pos:pos + n]); pos += n
        m = dev.meters()
        f, _ = dev.filters()
        w = api.vector_meters_from_filters(f)
        assert np.array_equal(_bits(m.balance[:]), _bits(w.balance[:])) and np.array_equal(_bits(m.stereo[:]), _bits(w.stereo[:])), rnd
        assert 0.0 <= m.balance[0] <= 1.0 and 0.0 <= m.stereo[0] <= 1.0
    dev.close()


def test_argument_checks(gpu):
    """pair out of range, a count too small (the required size comes back), null pointers: SGZ_EINVAL and nothing written"""
    import torch
    L = api.lib()
    dev = _vector(4, 500, 1, 1, 512)
    _push(dev, synth.gen(2, SR, 400, 4))
    xyz = np.full((2, 500, 3), 7.0, F32)
    rgb = np.full((2, 500, 3), 7.0, F32)
    P = api._np_ptr

    def untouched():
        return (xyz == 7.0).all() and (rgb == 7.0).all()

    cnt = C.c_uint32(500)
    assert L.sgz_vector_lissajous_vertices(dev.h, 2, P(xyz), P(rgb), C.byref(cnt)) == api.SGZ_EINVAL and untouched() and cnt.value == 500
    cnt = C.c_uint32(499)
    assert L.sgz_vector_lissajous_vertices(dev.h, 0, P(xyz), P(rgb), C.byref(cnt)) == api.SGZ_EINVAL and untouched() and cnt.value == 500
    cnt = C.c_uint32(3)
    assert L.sgz_vector_lissajous_vertices_all(dev.h, P(xyz), P(rgb), C.byref(cnt)) == api.SGZ_EINVAL and untouched() and cnt.value == 500
    cnt = C.c_uint32(500)
    assert L.sgz_vector_lissajous_vertices(dev.h, 0, None, P(rgb), C.byref(cnt)) == api.SGZ_EINVAL and untouched()
    assert L.sgz_vector_lissajous_vertices(dev.h, 0, P(xyz), P(rgb), None) == api.SGZ_EINVAL and untouched()
    assert L.sgz_vector_lissajous_vertices(None, 0, P(xyz), P(rgb), C.byref(cnt)) == api.SGZ_EINVAL and untouched()
    assert L.sgz_vector_lissajous_vertices_all(dev.h, None, P(rgb), C.byref(cnt)) == api.SGZ_EINVAL and untouched()
    assert L.sgz_vector_lissajous_vertices_all(None, P(xyz), P(rgb), C.byref(cnt)) == api.SGZ_EINVAL and untouched()
    d_xyz = torch.full((500, 3), 7.0, dtype=torch.float32, device=gpu)
    cnt = C.c_uint32(500)
    assert L.sgz_vector_lissajous_vertices_device(dev.h, 5, C.c_void_p(d_xyz.data_ptr()), None, C.byref(cnt)) == api.SGZ_EINVAL
    cnt = C.c_uint32(10)
    assert L.sgz_vector_lissajous_vertices_device(dev.h, 0, C.c_void_p(d_xyz.data_ptr()), None, C.byref(cnt)) == api.SGZ_EINVAL and cnt.value == 500
    assert L.sgz_vector_lissajous_vertices_device(dev.h, 0, None, None, C.byref(cnt)) == api.SGZ_EINVAL
    torch.cuda.synchronize()
    assert (d_xyz == 7.0).all().item()
    # stage call: null input / output, colours missing for d_rgb, stride below n
    d_in = torch.zeros((2, 100), dtype=torch.float32, device=gpu)
    d_out = torch.full((100, 3), 7.0, dtype=torch.float32, device=gpu)
    d_col = torch.full((100, 3), 7.0, dtype=torch.float32, device=gpu)
    cols = np.ones((1, 3), F32)
    assert L.sgz_vector_lissajous_device(None, 100, 1, 100, 1, P(cols), d_out.data_ptr(), None, None) == api.SGZ_EINVAL
    assert L.sgz_vector_lissajous_device(d_in.data_ptr(), 100, 1, 100, 1, P(cols), None, None, None) == api.SGZ_EINVAL
    assert L.sgz_vector_lissajous_device(d_in.data_ptr(), 100, 1, 100, 1, None, d_out.data_ptr(), d_col.data_ptr(), None) == api.SGZ_EINVAL
    assert L.sgz_vector_lissajous_device(d_in.data_ptr(), 99, 1, 100, 1, P(cols), d_out.data_ptr(), None, None) == api.SGZ_EINVAL
    assert L.sgz_vector_lissajous_device(d_in.data_ptr(), 100, 0, 100, 1, P(cols), d_out.data_ptr(), None, None) == api.SGZ_EINVAL
    torch.cuda.synchronize()
    assert (d_out == 7.0).all().item() and (d_col == 7.0).all().item()
    # meters
    m = api.VectorMeters()
    assert L.sgz_vector_meters(None, C.byref(m)) == api.SGZ_EINVAL
    assert L.sgz_vector_meters(dev.h, None) == api.SGZ_EINVAL
    dev.close()


def test_audio_and_render_threads_run_concurrently(gpu):
    """an audio thread pushes flat out while a render thread draws every pair's Lissajous strip at about 60 Hz: no call fails, and
    the last read equals the restatement of the final ring"""
    import time
    import torch
    channels, size = 4, 4800
    dev = _vector(channels, size, 2, 1, 512)
    x = synth.gen(12, SR, 1500 * 200, channels)
    errors, frames = [], [0]
    done = threading.Event()
    outs = (torch.zeros((channels // 2, size, 3), dtype=torch.float32).pin_memory().numpy(),
            torch.zeros((channels // 2, size, 3), dtype=torch.float32).pin_memory().numpy())

    def producer():
        try:
            for pos in range(0, x.shape[1], 200):
                blk = np.ascontiguousarray(x[:, pos:pos + 200])
                while True:
                    st = dev.push(blk)
                    if st == api.SGZ_OK:
                        break
                    if st != api.SGZ_BUSY:
                        errors.append(("push", st)); return
        finally:
            done.set()

    def render():
        try:
            while not done.is_set() or frames[0] < 8:            # (at least eight frames however fast the producer is)
                t0 = time.perf_counter()
                dev.lissajous_all(*outs)
                frames[0] += 1
                time.sleep(max(0.0, 1 / 60 - (time.perf_counter() - t0)))
            dev.lissajous_all(*outs)                               # the last read: after the final push
        except Exception as e:                                     # noqa: BLE001
            errors.append(("render", repr(e)))

    tp, tr = threading.Thread(target=producer), threading.Thread(target=render)
    tr.start(); tp.start(); tp.join(timeout=180); tr.join(timeout=180)
    assert not errors and not tp.is_alive() and not tr.is_alive(), errors[:3]
    assert frames[0] >= 8
    mem = np.zeros((channels, size), F32)
    mem[:, (np.arange(x.shape[1])) % size] = x                      # the last `size` samples land where the ring keeps them
    cursor = x.shape[1] % size
    for p in range(channels // 2):
        wx, wc = lissajous_ref(mem[2 * p], mem[2 * p + 1], cursor, 1, COLOURS[p])
        assert np.array_equal(_bits(outs[0][p]), _bits(wx)), p
        assert np.array_equal(_bits(outs[1][p]), _bits(wc)), p
        hx, hc = _ref_from_handle(dev, p, 1, COLOURS[p])
        assert np.array_equal(_bits(hx), _bits(wx))
    dev.close()
