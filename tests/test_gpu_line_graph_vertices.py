"""The Spectrum line graph's vertex stream (renderTransformAsGraph, SpectrumRendering.cpp:794-897) on the real-time handle
(sgz_spectrum_render_line_vertices) and as a stateless stage (sgz_line_graph_vertices_device).

The reference side is a plain numpy float32 restatement of the vertex order fed from the handle's own sgz_spectrum_line_results, which
tests/test_gpu_stream_modes.py holds to the oracle: per pair, flood fills (k = 1, 0; right then left) as (i, y, z), (i, 0, z), then the
strips as (i, y, z); y = .second on the right side (z = -0.5), .first on the left (z = 0).  Every bar is bit for bit."""
import ctypes as C
import threading

import numpy as np
import pytest

from signalizer_amd import api, config, synth
from stream_windows import cut

pytestmark = pytest.mark.gpu

F32 = np.float32
TWO_SIDED = {config.CH_PHASE, config.CH_SEPARATE, config.CH_MIDSIDE}
L = None


def _lib():
    global L
    if L is None:
        L = api.lib()
    return L


def vertices_ref(results, mode, flood):
    """results float32 [pairs][graphs][P][2] -> float32 [vertices][3] in renderTransformAsGraph's order"""
    results = np.asarray(results, F32)
    pairs, G, P, _ = results.shape
    x = np.arange(P).astype(F32)
    out = []
    sides = [1, 0] if mode in TWO_SIDED else [0]
    for p in range(pairs):
        blocks = [(k, s) for k in (1, 0) for s in sides]
        if flood:
            for k, s in blocks:
                y = results[p, k, :, s]
                z = np.full(P, F32(-0.5) if s else F32(0.0), F32)
                v = np.empty((P, 2, 3), F32)
                v[:, 0, 0], v[:, 0, 1], v[:, 0, 2] = x, y, z
                v[:, 1, 0], v[:, 1, 1], v[:, 1, 2] = x, F32(0.0), z
                out.append(v.reshape(2 * P, 3))
        for k, s in blocks:
            out.append(np.stack([x, results[p, k, :, s], np.full(P, F32(-0.5) if s else F32(0.0), F32)], axis=1))
    return np.ascontiguousarray(np.concatenate(out), F32)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _create(cfg):
    c = api.config_from_dict(cfg)
    h = C.c_void_p()
    api.check(_lib().sgz_spectrum_create(C.byref(c), C.byref(h)))
    return h


def _push(h, blk):
    ptrs = (C.c_void_p * blk.shape[0])(*[blk[c].ctypes.data for c in range(blk.shape[0])])
    api.check(_lib().sgz_spectrum_push(h, ptrs, blk.shape[0], blk.shape[1]))
    api.check(_lib().sgz_spectrum_flush(h))


def _line_results(h, pairs, P):
    out = np.zeros((pairs, 2, P, 2), F32)
    for p in range(pairs):
        for k in range(2):
            api.check(_lib().sgz_spectrum_line_results(h, p, k, out[p, k].ctypes.data_as(C.c_void_p)))
    return out


def _render_lines(h, pairs, P, poles=None):
    out = np.zeros((pairs, 2, P, 2), F32)
    pl = (C.c_float * 2)(*poles) if poles is not None else None
    api.check(_lib().sgz_spectrum_render_lines(h, pl, out.ctypes.data_as(C.c_void_p)))
    return out


def _line_cfg(**kw):
    return config.spectrum_config(display_mode=config.DISPLAY_LINE_GRAPH, **kw)


@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("W", [4096, 32768])
@pytest.mark.parametrize("mode", range(8))
def test_handle_against_the_restatement(gpu, mode, W, pairs):
    """uneven push blocks interleaved with render calls, flood on and off by turns: every stream = the restatement of the results the
    call left for sgz_spectrum_line_results"""
    P = 300
    cfg = _line_cfg(window_size=W, hop=1024, axis_points=P, channel_mode=mode, num_pairs=pairs)
    x = synth.gen(50 + mode, 48000, W + 30000, 2 * pairs)
    blocks = cut(x, [480, 37, 4096, 1000, 20000])
    h = _create(cfg)
    try:
        calls = 0
        for k, blk in enumerate(blocks):
            _push(h, blk)
            if k % 2 == 0 and k not in (2, len(blocks) - 1):
                continue
            for flood in ((0, 1) if k == len(blocks) - 1 else (k % 3 == 0,)):
                n = api.line_graph_vertex_count(mode, pairs, P, flood)
                out = np.full((n, 3), np.nan, F32)
                assert api.spectrum_render_line_vertices(h, None, flood, out) == n
                want = vertices_ref(_line_results(h, pairs, P), mode, flood)
                assert np.array_equal(_bits(out), _bits(want)), (k, flood, int((_bits(out) != _bits(want)).sum()))
                calls += 1
        assert calls >= 4
        assert np.abs(_line_results(h, pairs, P)).max() > 0
    finally:
        _lib().sgz_spectrum_destroy(h)


@pytest.mark.parametrize("flood", [0, 1])
@pytest.mark.parametrize("mode", [config.CH_SEPARATE, config.CH_MERGE, config.CH_PHASE])
def test_rsnt_against_the_restatement(gpu, mode, flood):
    P = 200
    cfg = _line_cfg(window_size=1024, hop=256, axis_points=P, channel_mode=mode, algorithm=config.ALGO_RSNT)
    x = synth.gen(46, 48000, 6000, 2)
    h = _create(cfg)
    try:
        n = api.line_graph_vertex_count(mode, 1, P, flood)
        for k, blk in enumerate(cut(x, [480, 37, 512, 1000])):
            _push(h, blk)
            if k % 2:
                out = np.full((n, 3), np.nan, F32)
                api.spectrum_render_line_vertices(h, None, flood, out)
                assert np.array_equal(_bits(out), _bits(vertices_ref(_line_results(h, 1, P), mode, flood))), k
    finally:
        _lib().sgz_spectrum_destroy(h)


@pytest.mark.parametrize("mode", [config.CH_SEPARATE, config.CH_LEFT, config.CH_PHASE])
def test_filters_advance_once(gpu, mode):
    """two handles fed the same blocks with the same per-call poles, one through render_lines and one through render_line_vertices: their
    results stay identical call after call (each call advances both filters exactly once), and line_results / track_peak_lines agree"""
    P, W, pairs = 256, 4096, 2
    cfg = _line_cfg(window_size=W, hop=1024, axis_points=P, channel_mode=mode, num_pairs=pairs)
    x = synth.gen(61, 48000, 40000, 2 * pairs)
    ha, hb = _create(cfg), _create(cfg)
    rng = np.random.default_rng(mode)
    try:
        n = api.line_graph_vertex_count(mode, pairs, P, True)
        for k, blk in enumerate(cut(x, [700, 3000, 129])):
            _push(ha, blk); _push(hb, blk)
            for _ in range(1 + k % 3):                            # several renders without new audio, too
                poles = tuple(float(v) for v in rng.uniform(0.3, 0.99, 2))
                want = _render_lines(ha, pairs, P, poles)
                out = np.full((n, 3), np.nan, F32)
                api.spectrum_render_line_vertices(hb, poles, True, out)
                got = _line_results(hb, pairs, P)
                assert np.array_equal(_bits(got), _bits(want)), k
                assert np.array_equal(_bits(_line_results(ha, pairs, P)), _bits(want))
                assert np.array_equal(_bits(out), _bits(vertices_ref(want, mode, True))), k
                for p in range(pairs):
                    for g in range(2):
                        pa, pb = api.LinePeak(), api.LinePeak()
                        sa = _lib().sgz_spectrum_track_peak_lines(ha, p, g, 0.37, C.byref(pa))
                        sb = _lib().sgz_spectrum_track_peak_lines(hb, p, g, 0.37, C.byref(pb))
                        assert sa == sb, (k, p, g)
                        assert [repr(v) for v in pa.asdict().values()] == [repr(v) for v in pb.asdict().values()], (k, p, g)
        assert np.abs(want).max() > 0
    finally:
        _lib().sgz_spectrum_destroy(ha)
        _lib().sgz_spectrum_destroy(hb)


def test_destinations_give_identical_bytes(gpu):
    """pageable numpy, pageable torch, pinned torch and device torch: the same bytes (poles 0 and no audio between the calls: every call
    renders the same results)"""
    import torch
    P, W, pairs, mode = 1024, 32768, 2, config.CH_SEPARATE
    cfg = _line_cfg(window_size=W, hop=8192, axis_points=P, channel_mode=mode, num_pairs=pairs, pole=(0.0, 0.0))
    x = synth.gen(2, 48000, W + 5000, 2 * pairs)
    h = _create(cfg)
    try:
        for blk in cut(x, [16384]):
            _push(h, blk)
        for flood in (1, 0):
            n = api.line_graph_vertex_count(mode, pairs, P, flood)
            host = np.full((n, 3), np.nan, F32)
            api.spectrum_render_line_vertices(h, (0.0, 0.0), flood, host)
            want = vertices_ref(_line_results(h, pairs, P), mode, flood)
            assert np.array_equal(_bits(host), _bits(want))
            outs = [torch.full((n, 3), float("nan"), dtype=torch.float32),
                    torch.full((n, 3), float("nan"), dtype=torch.float32).pin_memory(),
                    torch.full((n, 3), float("nan"), dtype=torch.float32, device=gpu)]
            for o in outs:
                assert api.spectrum_render_line_vertices(h, (0.0, 0.0), flood, o) == n
                assert np.array_equal(_bits(o.cpu().numpy()), _bits(want)), o.device
            pinned_np = outs[1].numpy()                             # the pinned tensor's memory as a numpy array
            pinned_np[:] = np.nan
            api.spectrum_render_line_vertices(h, None, flood, pinned_np)
            assert np.array_equal(_bits(pinned_np), _bits(want))
            bigger = torch.full((n + 100, 3), 5.0, dtype=torch.float32, device=gpu)     # a larger buffer: only the stream is written
            assert api.spectrum_render_line_vertices(h, None, flood, bigger) == n
            b = bigger.cpu().numpy()
            assert np.array_equal(_bits(b[:n]), _bits(want)) and (b[n:] == 5.0).all()
    finally:
        _lib().sgz_spectrum_destroy(h)


def test_stage_call(gpu):
    """sgz_line_graph_vertices_device on arbitrary device results: NaN payloads, infinities and -0 pass through as they are"""
    import torch
    rng = np.random.default_rng(7)
    specials = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -3e38], F32)
    bits = specials.view(np.uint32).copy()
    bits[0] = 0x7FC12345
    specials = bits.view(F32)
    stream = torch.cuda.current_stream().cuda_stream
    for pairs, P in [(1, 2), (3, 3), (2, 300), (33, 1000), (1, 257)]:
        res = rng.standard_normal((pairs, 2, P, 2)).astype(F32)
        flat = res.reshape(-1)
        idx = rng.choice(flat.size, size=min(flat.size, 200), replace=False)
        flat[idx] = specials[np.arange(idx.size) % specials.size]
        d = torch.from_numpy(res).to(gpu)
        for mode in range(8):
            for flood in (0, 1):
                n = api.line_graph_vertex_count(mode, pairs, P, flood)
                d_xyz = torch.full((n + 7, 3), 3.0, dtype=torch.float32, device=gpu)
                api.check(_lib().sgz_line_graph_vertices_device(d.data_ptr(), pairs, P, mode, flood, d_xyz.data_ptr(), stream))
                torch.cuda.synchronize()
                got = d_xyz.cpu().numpy()
                assert np.array_equal(_bits(got[:n]), _bits(vertices_ref(res, mode, flood))), (pairs, P, mode, flood)
                assert (got[n:] == 3.0).all()
    assert _lib().sgz_line_graph_vertices_device(None, 1, 2, 0, 0, d.data_ptr(), stream) == api.SGZ_EINVAL
    assert _lib().sgz_line_graph_vertices_device(d.data_ptr(), 1, 2, 0, 0, None, stream) == api.SGZ_EINVAL
    assert _lib().sgz_line_graph_vertices_device(d.data_ptr(), 1, 2, 8, 0, d.data_ptr(), stream) == api.SGZ_EINVAL


def test_refusals_write_nothing(gpu):
    """SGZ_EINVAL on a COLOUR_SPECTRUM handle and for a buffer one vertex too small (count holds the size needed): nothing written, and
    the refused call leaves the filters alone (the next render equals a twin handle's that never saw it)"""
    import torch
    L = _lib()
    P = 128
    hc = _create(config.spectrum_config(window_size=2048, hop=512, axis_points=P))
    try:
        buf = np.full((4 * P * 3, 3), 7.0, F32)
        cnt = C.c_uint32(buf.shape[0])
        assert L.sgz_spectrum_render_line_vertices(hc, None, 1, api._np_ptr(buf), C.byref(cnt)) == api.SGZ_EINVAL
        assert (buf == 7.0).all() and cnt.value == buf.shape[0]
    finally:
        L.sgz_spectrum_destroy(hc)
    cfg = _line_cfg(window_size=2048, hop=512, axis_points=P, channel_mode=config.CH_SEPARATE)
    ha, hb = _create(cfg), _create(cfg)
    try:
        x = synth.gen(5, 48000, 5000, 2)
        for blk in cut(x, [1000]):
            _push(ha, blk); _push(hb, blk)
        _render_lines(ha, 1, P); _render_lines(hb, 1, P)
        n = api.line_graph_vertex_count(config.CH_SEPARATE, 1, P, True)
        assert n == 4 * P * 3
        small = np.full((n - 1, 3), 7.0, F32)
        d_small = torch.full((n - 1, 3), 7.0, dtype=torch.float32, device=gpu)
        for ptr in (api._np_ptr(small), C.c_void_p(d_small.data_ptr())):
            cnt = C.c_uint32(n - 1)
            assert L.sgz_spectrum_render_line_vertices(hb, (C.c_float * 2)(0.1, 0.2), 1, ptr, C.byref(cnt)) == api.SGZ_EINVAL
            assert cnt.value == n
        cnt = C.c_uint32(n)
        assert L.sgz_spectrum_render_line_vertices(hb, None, 1, None, C.byref(cnt)) == api.SGZ_EINVAL
        assert L.sgz_spectrum_render_line_vertices(hb, None, 1, api._np_ptr(small), None) == api.SGZ_EINVAL
        assert L.sgz_spectrum_render_line_vertices(None, None, 1, api._np_ptr(small), C.byref(cnt)) == api.SGZ_EINVAL
        torch.cuda.synchronize()
        assert (small == 7.0).all() and (d_small == 7.0).all().item()
        assert np.array_equal(_bits(_render_lines(ha, 1, P)), _bits(_render_lines(hb, 1, P)))
        cnt = C.c_uint32(n - 1)                                      # flood off needs a third: the same buffer is now large enough
        assert L.sgz_spectrum_render_line_vertices(hb, None, 0, api._np_ptr(small), C.byref(cnt)) == api.SGZ_OK and cnt.value == n // 3
    finally:
        L.sgz_spectrum_destroy(ha)
        L.sgz_spectrum_destroy(hb)


def test_render_thread_and_audio_thread_run_concurrently(gpu):
    """a producer thread pushes flat out while the render thread draws the line graph into a pinned buffer: no call fails, and once the
    producer has stopped the stream is the restatement of the final window's results (poles 0: the newest window alone)"""
    import torch
    W, P, pairs, mode = 4096, 200, 2, config.CH_SEPARATE
    cfg = _line_cfg(window_size=W, hop=1024, axis_points=P, channel_mode=mode, num_pairs=pairs, pole=(0.0, 0.0))
    x = synth.gen(49, 48000, 2000 * 160, 2 * pairs)
    blocks = cut(x, [160])
    L = _lib()
    h = _create(cfg)
    n = api.line_graph_vertex_count(mode, pairs, P, True)
    out = torch.zeros((n, 3), dtype=torch.float32).pin_memory()
    errors, renders = [], [0]
    stop = threading.Event()

    def producer():
        try:
            for blk in blocks:
                ptrs = (C.c_void_p * blk.shape[0])(*[blk[c].ctypes.data for c in range(blk.shape[0])])
                st = L.sgz_spectrum_push(h, ptrs, blk.shape[0], blk.shape[1])
                if st != api.SGZ_OK:
                    errors.append(("push", st))
                    return
        finally:
            stop.set()

    def consumer():
        cnt = C.c_uint32(n)
        while not stop.is_set():
            cnt.value = n
            st = L.sgz_spectrum_render_line_vertices(h, None, 1, C.c_void_p(out.data_ptr()), C.byref(cnt))
            if st != api.SGZ_OK or cnt.value != n:
                errors.append(("render", st, L.sgz_last_error()))
                return
            renders[0] += 1

    tp, tc = threading.Thread(target=producer), threading.Thread(target=consumer)
    try:
        tc.start(); tp.start(); tp.join(timeout=120); tc.join(timeout=120)
        assert not errors and not tp.is_alive() and not tc.is_alive(), errors[:3]
        assert renders[0] > 10
        api.check(L.sgz_spectrum_flush(h))
        assert api.spectrum_render_line_vertices(h, None, True, out) == n
        res = _line_results(h, pairs, P)
        assert np.array_equal(_bits(out.numpy()), _bits(vertices_ref(res, mode, True)))
        # the same final window pushed alone into a fresh handle: identical results
        hf = _create(cfg)
        try:
            _push(hf, np.ascontiguousarray(x[:, -W:]))
            assert np.array_equal(_bits(_render_lines(hf, pairs, P)), _bits(res))
        finally:
            L.sgz_spectrum_destroy(hf)
    finally:
        L.sgz_spectrum_destroy(h)
