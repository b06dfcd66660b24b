"""The Oscilloscope's dense stream (sgz_scope_dense_*, csrc/scope_dense.hip): the frame's Linear strip reduced on the device to a minimum
and a maximum vertex per column.

The definition (include/sgz.h) is restated in numpy below (_dense_indices).  The expected bytes are gathered with it from the SAME
handle's sgz_scope_vertices output -- the Linear strip, which tests/test_gpu_scope_stream.py holds to the oracle -- or from a LINEAR
twin fed the same blocks when the handle draws Lanczos / Rectangular / None strips.  Every comparison is byte for byte: the dense stream
is a subsequence of the Linear one.

The kernel takes two forms by the longest column's length (scope_dense.hip kLongColumn = 1024 samples: a wave per column up to it, chunks
of 2048 samples and a fold launch above it); the shapes below straddle that length and the chunk's."""
import ctypes as C
import gc
import threading

import numpy as np
import pytest

from signalizer_amd import api

pytestmark = pytest.mark.gpu

SR = 192000.0
BANDS = ((1.0, 0.2, 0.1), (0.1, 1.0, 0.3), (0.2, 0.3, 1.0))
NONE, SPECTRAL, WINDOW, ENVELOPE_HOLD, ZERO_CROSSING = 0, 1, 2, 3, 4
LINEAR, LANCZOS = 2, 3
LONG_COLUMN, CHUNK = 1024, 2048           # scope_dense.hip: kLongColumn, kChunk
NARROW = api.ScopeView(0.0, 0.0, 1.0, 1.0, 2, 0)      # two pixels: far below one pixel per sample -> every handle draws the Linear strip


# ------------------------------------------------------------------------------------------------------------- the definition in numpy

def _bounds(n, columns):
    cols = min(columns, n)
    return [(b * n + cols - 1) // cols for b in range(cols + 1)]        # ceil(b n / cols), Python integers


def _dense_indices(y, columns):
    """indices into V of the dense stream: per column min(lo, hi), max(lo, hi)"""
    st = _bounds(len(y), columns)
    out = np.empty(2 * (len(st) - 1), np.int64)
    for b in range(len(st) - 1):
        seg = y[st[b]:st[b + 1]]
        assert seg.size > 0
        ok = ~np.isnan(seg)
        if not ok.any():
            lo = hi = 0
        else:
            lo = int(np.flatnonzero(seg == seg[ok].min())[0])            # (== : -0 and +0 tie; the lowest index)
            hi = int(np.flatnonzero(seg == seg[ok].max())[0])
        out[2 * b], out[2 * b + 1] = st[b] + min(lo, hi), st[b] + max(lo, hi)
    return out


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _push(dev, blk):
    while True:
        st = dev.push(np.ascontiguousarray(blk))
        if st == api.SGZ_OK:
            return
        assert st == api.SGZ_BUSY


def _feed(devs, x, block=3000):
    for pos in range(0, x.shape[1], block):
        for d in devs:
            _push(d, x[:, pos:pos + block])


def _cfg(**over):
    cfg = dict(sample_rate=SR, window_size=1000.0, num_channels=2, trigger_mode=NONE, channel_mode=0, envelope_mode=0, interpolation=LINEAR,
               max_block=4096, trigger_threshold=0.05, trigger_channel=1.0, envelope_window=0.3, colours=[(10, 20, 30, 255), (200, 100, 50, 255)])
    cfg.update(over)
    return cfg


def _coloured(**over):
    return _cfg(colour_by_frequency=1, frequency_colouring_blend=0.7, colour_smoothing_ms=3.0, band_colours=BANDS, **over)


def _noise(seed, n, channels=2):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    return np.stack([(0.5 * np.sin(2 * np.pi * 441.7 * (1 + 0.3 * c) * t) + 0.3 * rng.standard_normal(n)) for c in range(channels)]).astype(np.float32)


def _check(dev, columns, evaluator=0, linear=None, src=None, want_colours=True):
    """dense(columns) == the definition applied to the Linear strip (`linear`: that strip if the caller has it already)"""
    xyz, rgba = linear if linear is not None else (src or dev).vertices(NARROW, evaluator, 0)
    idx = _dense_indices(xyz[:, 1], columns)
    assert dev.dense_vertex_count(columns) == idx.size == 2 * min(columns, xyz.shape[0])
    got_xyz, got_rgba = dev.dense_vertices(columns, evaluator, 0, want_colours=want_colours)
    assert _same(got_xyz, xyz[idx]), (columns, evaluator, np.flatnonzero((got_xyz.view(np.uint32) != xyz[idx].view(np.uint32)).any(axis=1))[:8])
    if want_colours:
        assert np.array_equal(got_rgba, rgba[idx]), (columns, evaluator)
    else:
        assert got_rgba is None
    return got_xyz, got_rgba


# ------------------------------------------------------------------------------------------------------------------------------ shapes

def test_window_of_one_sample(gpu):
    """n = 2 (max(2, ceil(window))): columns 1, 2 and more than n"""
    dev = api.Scope(**_cfg(window_size=1.0))
    _feed([dev], _noise(1, 777))
    assert dev.vertices(NARROW, 0, 0)[0].shape[0] == 2
    for columns in (1, 2, 3, 1000):
        _check(dev, columns)
    dev.close()


@pytest.mark.parametrize("colour", [0, 1])
def test_thousand_samples_every_column_count_and_evaluator(gpu, colour):
    """n = 1000: one column, coprime counts, 999 / 1000 / 1001 and 5000 (cols = n: columns of one sample); all four evaluators; the winners'
    ring colours (colour_by_frequency) or the channel key; rgba = NULL"""
    dev = api.Scope(**(_coloured() if colour else _cfg()))
    _feed([dev], _noise(2, 7000))
    for evaluator in (0, 1, 2, 3):
        linear = dev.vertices(NARROW, evaluator, 0)
        assert linear[0].shape[0] == 1000
        if colour:
            assert len(np.unique(linear[1].view(np.uint32))) > 10          # (per-sample colours, not the key)
        for columns in (1, 7, 333, 999, 1000, 1001, 5000):
            _check(dev, columns, evaluator, linear=linear)
        _check(dev, 7, evaluator, linear=linear, want_colours=False)
    dev.close()


@pytest.mark.parametrize("total,wrap_at", [(3 * 1001 + 714, 286), (3 * 1001 + 700, 300), (5 * 1001 + 1, 999), (4 * 1001, 1000)])
def test_ring_wrap_inside_a_column_and_at_a_column_boundary(gpu, total, wrap_at):
    """window 1000: a ring of 1001 samples, vertex i reads memory (cursor + 1 + i) mod 1001 -- the strip wraps at i = 1000 - cursor.  With
    seven columns (bounds 0, 143, 286, 429, ..) that is at a column boundary (286), inside a column (300), at the last vertex (999), or past the strip (1000: no wrap)"""
    dev = api.Scope(**_cfg())
    _feed([dev], _noise(3, total), block=977)
    mem, cur = dev.front(0)
    assert mem.size == 1001 and (1000 - cur) % 1001 == wrap_at % 1001
    assert _bounds(1000, 7)[:3] == [0, 143, 286]
    linear = dev.vertices(NARROW, 0, 0)
    for columns in (7, 1, 64, 1000):
        _check(dev, columns, linear=linear)
    dev.close()


@pytest.mark.parametrize("n,columns", [
    (3 * LONG_COLUMN - 3, 3), (3 * LONG_COLUMN, 3), (3 * LONG_COLUMN + 3, 3),      # every column 1023 / 1024 / 1025 samples: the switch-over
    (3 * LONG_COLUMN + 1, 3),                                                       # 1025, 1024, 1024: the longest column decides
    (2 * CHUNK, 2), (2 * CHUNK + 1, 2), (2 * CHUNK + 2, 2),                         # one chunk / two with an empty one / two
    (5 * CHUNK + 77, 1), (4099, 4), (4099, 5),
])
def test_column_lengths_around_the_switch_over(gpu, n, columns):
    dev = api.Scope(**_cfg(window_size=float(n)))
    _feed([dev], _noise(4, n + 1500), block=4000)                  # (1500 past one ring: the strip wraps the memory)
    linear = dev.vertices(NARROW, 0, 0)
    assert linear[0].shape[0] == n
    _check(dev, columns, 0, linear=linear)
    _check(dev, columns, 3, want_colours=False)
    dev.close()


@pytest.fixture(scope="module")
def million(gpu):
    """n = 2^20 + 3 in the long form: one handle and its Linear strips, shared"""
    n = (1 << 20) + 3
    dev = api.Scope(**_cfg(window_size=float(n), max_block=65536))
    x = _noise(5, n + 40000)
    x[0, -n + 5] = 9.0; x[0, -7] = -9.0                            # (known extremes near both ends of the strip)
    _feed([dev], x, block=65536)
    linear = {e: dev.vertices(NARROW, e, 0) for e in (0, 2)}
    assert linear[0][0].shape[0] == n
    yield dev, linear
    dev.close()


@pytest.mark.parametrize("columns", [1, 2, 3, 1024])
def test_long_form_at_a_million_samples(million, columns):
    dev, linear = million
    got, _ = _check(dev, columns, 0, linear=linear[0])
    if columns == 1:
        n = linear[0][0].shape[0]
        assert got[0, 0] == 5.0 and got[1, 0] == float(n - 7) and got[0, 1] == 9.0 and got[1, 1] == -9.0
    _check(dev, columns, 2, linear=linear[2], want_colours=False)


# ----------------------------------------------------------------------------------------------------------- trigger and time modes

@pytest.mark.parametrize("trigger", [NONE, ZERO_CROSSING, ENVELOPE_HOLD])
@pytest.mark.parametrize("window", [3000.0, 2777.5])
def test_trigger_modes(gpu, trigger, window):
    dev = api.Scope(**_coloured(window_size=window, trigger_mode=trigger, trigger_hysteresis=0.1, interpolation=LANCZOS))
    _feed([dev], _noise(6, 30000), block=1999)
    dev.analyse(0, 0)
    for evaluator in (0, 3):
        linear = dev.vertices(NARROW, evaluator, 0)
        assert linear[0].shape[0] == int(np.ceil(window))
        for columns in (2, 500):
            _check(dev, columns, evaluator, linear=linear)
    dev.close()


def test_window_trigger_follows_the_transport(gpu):
    dev = api.Scope(**_cfg(window_size=1000.0, trigger_mode=WINDOW))
    _feed([dev], _noise(7, 9000), block=1999)
    strips = []
    for transport in (40000 + 317, 123456789):
        dev.set_transport(transport)
        strips.append(_check(dev, 11)[0])
        _check(dev, 1000, 1)
    assert not _same(strips[0], strips[1])
    dev.close()


@pytest.mark.parametrize("custom", [330.0, 0.0])
def test_spectral_trigger_adds_the_quantized_cycle(gpu, custom):
    """Spectral: n = ceil(window) + ceil(cycleSamples), read from the frame's ring of ring_size samples inside the larger physical one.  A
    named trigger frequency gives cycleSamples = 48000 / 330 from the first frame on (ring_size 8192 of 11600); without one the first
    frame has the 5 Hz floor, cycleSamples = 9600: the strip is the whole physical ring"""
    sr, window = 48000.0, 2000.0
    dev = api.Scope(**_cfg(sample_rate=sr, window_size=window, trigger_mode=SPECTRAL, trigger_threshold=0.02, trigger_hysteresis=0.1,
                           trigger_phase_offset=15.0, interpolation=LANCZOS, custom_trigger=int(custom > 0), custom_trigger_frequency=custom))
    t = np.arange(30000) / sr
    x = np.stack([np.sin(2 * np.pi * 330.0 * t + 0.3) + 0.3 * np.sin(2 * np.pi * 660.0 * t), 0.5 * np.sin(2 * np.pi * 660.0 * t)]).astype(np.float32)
    _feed([dev], x, block=1500)
    ts = dev.analyse(0, 0)
    q = int(np.ceil(ts.cycle_samples))
    size = dev.front(0)[0].size
    assert size == 11600 and q > 0
    if custom:
        assert q == 146 and ts.ring_size == 8192                           # (the frame's ring is cut out of a larger physical one)
    for evaluator in (0, 2):
        linear = dev.vertices(NARROW, evaluator, 0)
        assert linear[0].shape[0] == 2000 + q
        for columns in (1, 13, 700, 3000):
            _check(dev, columns, evaluator, linear=linear)
    dev.close()


def test_cycles_time_mode(gpu):
    sr = 48000.0
    dev = api.Scope(**_cfg(sample_rate=sr, window_size=3.0, time_mode=api.TIME_CYCLES, trigger_mode=SPECTRAL, trigger_threshold=0.02,
                           trigger_hysteresis=0.0, trigger_phase_offset=30.0))
    t = np.arange(24000) / sr
    x = np.stack([np.sin(2 * np.pi * 441.3 * t), 0.6 * np.sin(2 * np.pi * 441.3 * t + 1.0)]).astype(np.float32)
    for frame in range(3):
        _feed([dev], x[:, frame * 8000:(frame + 1) * 8000], block=2000)
        ts = dev.analyse(0, 0)
    window = dev.effective_window()
    assert window > 100.0 and ts.cycle_samples > 0
    linear = dev.vertices(NARROW, 0, 0)
    assert linear[0].shape[0] == int(np.ceil(window)) + int(np.ceil(ts.cycle_samples))
    for columns in (1, 9, 200):
        _check(dev, columns, linear=linear)
    dev.close()


def test_beats_time_mode(gpu):
    sr = 48000.0
    dev = api.Scope(**_cfg(sample_rate=sr, window_size=8.0, time_mode=api.TIME_BEATS, trigger_mode=ZERO_CROSSING))
    dev.set_tempo(120.0)
    dev.analyse(0, 0)
    window = api.time_window(api.TIME_BEATS, 8.0, sr, 120.0)
    assert dev.effective_window() == window == 3000.0
    _feed([dev], _noise(8, 12000), block=1500)
    for columns in (1, 77, 3000):
        _check(dev, columns, 1)
    dev.set_tempo(90.0)                                                # the next frame's window: 4000 samples, through a reconfiguration
    dev.analyse(0, 0)
    _feed([dev], _noise(9, 9000), block=1500)
    assert dev.dense_vertex_count(1 << 20) == 2 * 4000
    _check(dev, 77, 0)
    dev.close()


@pytest.mark.parametrize("interpolation,width", [(LANCZOS, 4001), (1, 4001), (0, 4001), (LANCZOS, 300)])
def test_the_stream_depends_on_neither_interpolation_nor_view(gpu, interpolation, width):
    """a handle that draws Lanczos / Rectangular / None strips at more than a pixel per sample: its dense stream is the one of a LINEAR
    twin fed the same blocks"""
    cfg = _coloured(window_size=2000.0, trigger_mode=ZERO_CROSSING)
    dev, twin = api.Scope(**dict(cfg, interpolation=interpolation)), api.Scope(**cfg)
    _feed([dev, twin], _noise(10, 15000), block=1234)
    view = api.ScopeView(0.0, 0.0, 1.0, 1.0, width, 0)
    own = dev.vertices(view, 2, 0)[0]
    linear = twin.vertices(view, 2, 0)
    if width == 4001 and interpolation != 0:
        assert own.shape[0] != linear[0].shape[0]                          # (the handle's own strip is another one)
    for columns in (5, 640):
        _check(dev, columns, 2, linear=linear)
    dev.close(); twin.close()


# ----------------------------------------------------------------------------------------------------------------------------- signals

def _load(x, **over):
    """trigger None: the strip is the newest n samples pushed, V[i] = x[-n + i]"""
    dev = api.Scope(**_cfg(**over))
    _feed([dev], x, block=1777)
    return dev


def test_constant_signal_all_ties(gpu):
    x = np.full((2, 5000), 0.25, np.float32)
    dev = _load(x)
    for columns in (1, 7, 1000):
        got, _ = _check(dev, columns)
        st = _bounds(1000, columns)
        assert np.array_equal(got[0::2, 0], np.array(st[:-1], np.float32)) and np.array_equal(got[1::2, 0], got[0::2, 0])   # the column's first vertex, twice
    dev.close()
    dev = _load(np.full((2, 9000), -1.5, np.float32), window_size=5000.0)          # the long form
    got, _ = _check(dev, 2)
    assert got[:, 0].tolist() == [0.0, 0.0, 2500.0, 2500.0]
    dev.close()


def test_square_wave_and_ramp(gpu):
    n = 6000
    square = np.where((np.arange(n) // 37) % 2 == 0, 0.8, -0.8)
    ramp = np.linspace(-1.0, 1.0, n)
    dev = _load(np.stack([square, ramp]).astype(np.float32))
    for columns in (1, 7, 27, 500):
        _check(dev, columns, 0)                                    # square: long runs of ties, the first of each wins
        got, _ = _check(dev, columns, 1)                           # rising ramp: the column's first and last vertex
        st = _bounds(1000, columns)
        assert np.array_equal(got[0::2, 0], np.array(st[:-1], np.float32)) and np.array_equal(got[1::2, 0], np.array(st[1:], np.float32) - 1)
    dev.close()
    dev = _load(np.stack([ramp[::-1], square]).astype(np.float32))    # falling ramp: lo is the later vertex -> stream order swaps them
    got, _ = _check(dev, 10, 0)
    assert np.all(got[0::2, 0] < got[1::2, 0]) and np.all(got[0::2, 1] > got[1::2, 1])
    dev.close()


@pytest.mark.parametrize("window,columns", [(1000.0, 10), (1000.0, 1000), (1000.0, 1), (6144.0, 3), (6144.0, 2)])
def test_nan_inf_and_signed_zeros(gpu, window, columns):
    """NaN, +-inf and +-0.0 placed first, last and alone in a column, an all-NaN column, columns of only infinities and only zeros of both
    signs; the y bits (NaN payloads, the zero's sign) are the Linear strip's"""
    n = int(window)
    rng = np.random.default_rng(11)
    v = (0.5 * rng.standard_normal((2, n))).astype(np.float32)
    st = _bounds(n, min(columns, 10)) if columns != 1000 else _bounds(n, 10)
    nan, inf = np.float32("nan"), np.float32("inf")
    payload = np.array([0x7fc12345], np.uint32).view(np.float32)[0]
    width = st[1] - st[0]
    if len(st) > 10:
        v[0, st[0]] = nan; v[0, st[1] - 1] = inf                                # NaN first, +inf last
        v[0, st[1]] = -inf; v[0, st[2] - 1] = payload                           # -inf first, a NaN with a payload last
        v[0, st[2]:st[3]] = nan                                                 # an all-NaN column
        v[0, st[3]:st[4]] = nan; v[0, st[3] + width // 2] = 0.125              # one number alone among NaN
        v[0, st[4]:st[5]] = inf                                                 # only +inf: both winners the first
        v[0, st[5]:st[6]] = -inf; v[0, st[6] - 1] = inf
        v[0, st[6]:st[7]] = 0.0; v[0, st[6] + 3] = -0.0; v[0, st[6]] = -0.0     # zeros of both signs tie: the first, with ITS sign
        v[0, st[7]:st[8]] = -0.0; v[0, st[7] + 1] = 0.0
        v[0, st[8]] = -0.0; v[0, st[8] + 1:st[9]] = np.abs(v[0, st[8] + 1:st[9]]) + 0.01     # -0 first as the minimum
        v[0, st[9]:st[10]] = nan; v[0, st[10] - 1] = -inf                       # -inf alone, last
    else:
        v[0, 0] = nan; v[0, n - 1] = -0.0; v[0, n // 2:n // 2 + 5] = (inf, -inf, nan, 0.0, -0.0)
        v[0, st[1] + 5:st[1] + 705] = payload
    v[1] = v[0][::-1] * np.float32(0.5)                                         # Mid / Side of specials: inf - inf, NaN arithmetic
    x = np.concatenate([_noise(12, 2500), v], axis=1)
    dev = _load(x, window_size=window, max_block=4096)
    for evaluator in (0, 1, 2, 3):
        linear = dev.vertices(NARROW, evaluator, 0)
        if evaluator == 0:
            assert _same(linear[0][:, 1], v[0])
        _check(dev, columns, evaluator, linear=linear)
    dev.close()


# ------------------------------------------------------------------------------------------------------------------------ destinations

def _buffers(kind, shape, dtype, gpu):
    import torch
    t = torch.zeros(shape, dtype=dtype)
    if kind == "pinned":
        return t.pin_memory()
    return t.to(gpu) if kind == "device" else t


def _host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("window,columns", [(3000.0, 640), (9000.0, 4)])
def test_all_and_device_destinations_equal_the_single_calls(gpu, window, columns):
    import torch
    dev = api.Scope(**_coloured(window_size=window))
    _feed([dev], _noise(13, 20000))
    items = (0, 1, 2, 3)
    singles = [_check(dev, columns, e) for e in items]
    n = singles[0][0].shape[0]
    for kind in ("pageable", "pinned", "device"):
        outs = [(_buffers(kind, (n + 3, 3), torch.float32, gpu), _buffers(kind, (n + 3, 4), torch.uint8, gpu)) for _ in items]
        torch.cuda.synchronize()
        got = dev.dense_vertices_all(columns, items, (0,) * 4, outs)
        for (gx, gc), (wx, wc) in zip(got, singles):
            assert gx.shape[0] == n and _same(_host(gx), wx) and np.array_equal(_host(gc), wc), kind
        assert all(not _host(o[0][n:]).any() and not _host(o[1][n:]).any() for o in outs)          # nothing past the count
        # without colours; and a single call into each kind of memory
        outs = [(_buffers(kind, (n, 3), torch.float32, gpu), None) for _ in items]
        torch.cuda.synchronize()
        got = dev.dense_vertices_all(columns, items, (0,) * 4, outs)
        assert all(_same(_host(g[0]), w[0]) for g, w in zip(got, singles))
        out = (_buffers(kind, (n, 3), torch.float32, gpu), _buffers(kind, (n, 4), torch.uint8, gpu))
        torch.cuda.synchronize()
        gx, gc = dev.dense_vertices(columns, 3, 0, out=out)
        assert _same(_host(gx), singles[3][0]) and np.array_equal(_host(gc), singles[3][1])
    # sgz_scope_dense_vertices_device
    L = api.lib()
    d_xyz = torch.full((n, 3), float("nan"), dtype=torch.float32, device=gpu)
    d_rgba = torch.zeros((n, 4), dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    cnt = C.c_uint32(n)
    api.check(L.sgz_scope_dense_vertices_device(dev.h, columns, 2, 0, d_xyz.data_ptr(), d_rgba.data_ptr(), C.byref(cnt)))
    assert cnt.value == n and _same(_host(d_xyz), singles[2][0]) and np.array_equal(_host(d_rgba), singles[2][1])
    cnt = C.c_uint32(n)
    api.check(L.sgz_scope_dense_vertices_device(dev.h, columns, 1, 0, d_xyz.data_ptr(), None, C.byref(cnt)))
    assert cnt.value == n and _same(_host(d_xyz), singles[1][0])
    cnt = C.c_uint32(n - 1)
    assert L.sgz_scope_dense_vertices_device(dev.h, columns, 1, 0, d_xyz.data_ptr(), None, C.byref(cnt)) == api.SGZ_EINVAL and cnt.value == n
    assert _same(_host(d_xyz), singles[1][0])
    dev.close()


STAGE_SHAPES = [(1000, 1000, 7, 1), (1000, 2, 5, 2), (1001, 1000, 1000, 3), (4096, 3000, 1, 2), (5000, 4099, 4, 1), (5000, 4099, 5, 3),
                (3 * 1024, 3 * 1024, 3, 2), (3 * 1024 + 1, 3 * 1024 + 1, 3, 2), (70000, 65536 + 3, 2, 2), (70000, 70000, 640, 1),
                (333, 1, 9, 4), (100, 250, 3, 2)]


@pytest.mark.parametrize("length,n,columns,channels", STAGE_SHAPES)
def test_stage_call_against_numpy(gpu, length, n, columns, channels):
    """sgz_scope_dense_device on rings in time order: V[i] = (i, ring[(len - n + i) mod len]) (n > len reads the ring round again)"""
    import torch
    rng = np.random.default_rng(length + n)
    stride = length + 5
    ring = rng.standard_normal((channels, stride)).astype(np.float32)
    ring[0, rng.integers(0, length, 20)] = np.nan
    ring[-1, rng.integers(0, length, 20)] = 0.0
    cols = min(columns, n)
    d_ring = torch.from_numpy(ring).to(gpu)
    d_xy = torch.full((channels, 2 * cols, 2), float("nan"), dtype=torch.float32, device=gpu)
    torch.cuda.synchronize()
    api.scope_dense_device(d_ring, n, columns, d_xy, length=length)
    torch.cuda.synchronize()
    got = d_xy.cpu().numpy()
    for c in range(channels):
        y = ring[c, (length - n + np.arange(n)) % length]
        idx = _dense_indices(y, columns)
        want = np.stack([idx.astype(np.float32), y[idx]], axis=1)
        assert _same(got[c], want), c
    assert api.lib().sgz_scope_dense_device(d_ring.data_ptr(), length, stride, channels, n, 0, d_xy.data_ptr(), None) == api.SGZ_EINVAL
    assert api.lib().sgz_scope_dense_device(None, length, stride, channels, n, columns, d_xy.data_ptr(), None) == api.SGZ_EINVAL


# ------------------------------------------------------------------------------------------------------------ capacity and arguments

def test_refusals_write_nothing_and_leave_the_handle_as_it_was(gpu):
    L = api.lib()
    dev = api.Scope(**_coloured(window_size=3000.0, num_channels=4))
    _feed([dev], _noise(14, 10000, 4))
    before = dev.vertices(NARROW, 0, 0)
    want = _check(dev, 100, 0, linear=before)
    xyz = np.full((200, 3), 7.0, np.float32); rgba = np.full((200, 4), 7, np.uint8)
    px, pc = xyz.ctypes.data_as(C.c_void_p), rgba.ctypes.data_as(C.c_void_p)

    def refused(columns, evaluator, channel, x, c, count, need=None):
        cnt = C.c_uint32(count or 0)
        st = L.sgz_scope_dense_vertices(dev.h, columns, evaluator, channel, x, c, C.byref(cnt) if count is not None else None)
        assert st == api.SGZ_EINVAL and (xyz == 7.0).all() and (rgba == 7).all()
        if need is not None:
            assert cnt.value == need
        else:
            assert count is None or cnt.value == count
    assert L.sgz_scope_dense_vertex_count(dev.h, 100) == 200 and L.sgz_scope_dense_vertex_count(dev.h, 0) == 0
    refused(100, 0, 0, px, pc, 199, need=200)                      # too small: the need, nothing written
    refused(100, 0, 0, px, pc, 0, need=200)
    refused(5000, 0, 0, px, pc, 200, need=6000)
    refused(0, 0, 0, px, pc, 200)                                  # columns == 0
    refused(100, 4, 0, px, pc, 200); refused(100, 5, 0, px, pc, 200); refused(100, 77, 0, px, pc, 200)   # SEPARATE / MIDSIDE are no evaluators
    refused(100, 0, 4, px, pc, 200); refused(100, 1, 3, px, pc, 200); refused(100, 2, 3, px, pc, 200)    # channel (+ 1) out of range
    refused(100, 0, 0, None, pc, 200); refused(100, 0, 0, px, pc, None)
    assert L.sgz_scope_dense_vertices(None, 100, 0, 0, px, pc, C.byref(C.c_uint32(200))) == api.SGZ_EINVAL
    # _all: any bad item refuses the call; a small buffer reports every need
    ev = (C.c_uint32 * 2)(0, 1); ch = (C.c_uint32 * 2)(0, 0)
    xs = (C.c_void_p * 2)(xyz.ctypes.data, xyz.ctypes.data); cnts = (C.c_uint32 * 2)(200, 150)
    assert L.sgz_scope_dense_vertices_all(dev.h, 100, 2, ev, ch, xs, None, cnts) == api.SGZ_EINVAL and list(cnts) == [200, 200]
    bad = (C.c_uint32 * 2)(0, 9)
    assert L.sgz_scope_dense_vertices_all(dev.h, 100, 2, bad, ch, xs, None, cnts) == api.SGZ_EINVAL
    assert L.sgz_scope_dense_vertices_all(dev.h, 0, 2, ev, ch, xs, None, cnts) == api.SGZ_EINVAL
    assert (xyz == 7.0).all()
    # the handle is as it was: the same Linear strip, the same dense strip; pairs of a 4-channel handle work at channel 2
    after = dev.vertices(NARROW, 0, 0)
    assert _same(after[0], before[0]) and np.array_equal(after[1], before[1])
    again = _check(dev, 100, 0, linear=before)
    assert _same(again[0], want[0]) and np.array_equal(again[1], want[1])
    for evaluator in (0, 1, 2, 3):
        xyz2, rgba2 = dev.vertices(NARROW, evaluator, 2)
        idx = _dense_indices(xyz2[:, 1], 33)
        gx, gc = dev.dense_vertices(33, evaluator, 2)
        assert _same(gx, xyz2[idx]) and np.array_equal(gc, rgba2[idx])
    dev.close()


@pytest.mark.parametrize("option", [api.RT_OPT_PARK_PUSHES, api.RT_OPT_DEFER_SUBMIT])
def test_a_read_sees_parked_and_deferred_blocks(gpu, option):
    """flush on read: blocks that wait in the host FIFO (PARK_PUSHES) or in the open batch (DEFER_SUBMIT) reach the GPU in front of the
    dense kernels -- the strip is the one of a handle that took the same blocks at once"""
    cfg = _cfg(window_size=2000.0, max_block=512)
    dev, plain = api.Scope(**cfg), api.Scope(**cfg)
    x = _noise(15, 6000)
    _feed([dev, plain], x[:, :4000], block=500)
    first = _check(dev, 50)[0]
    dev.set_option(option, 1)
    _feed([dev, plain], x[:, 4000:], block=500)
    linear = plain.vertices(NARROW, 0, 0)
    got = _check(dev, 50, 0, linear=linear)[0]                     # (the dense call is the first reader behind the pushes)
    assert not _same(got, first)
    dev.close(); plain.close()


# --------------------------------------------------------------------------------------------------------------------------- lifecycle

def test_pushes_beside_dense_reads(gpu):
    """a producer thread pushes flat out while this thread reads dense strips of both forms: no call fails, and the rings end where a
    handle that only took the pushes ends"""
    cfg = _cfg(window_size=6000.0, trigger_mode=ZERO_CROSSING, trigger_threshold=0.02)
    dev, plain = api.Scope(**cfg), api.Scope(**cfg)
    x = _noise(16, 600 * 160)
    errors, frames = [], [0]
    done = threading.Event()

    def producer():
        try:
            for pos in range(0, x.shape[1], 160):
                blk = np.ascontiguousarray(x[:, pos:pos + 160])
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
            while not done.is_set() or frames[0] < 8:
                for columns in (640, 3):
                    got = dev.dense_vertices_all(columns, (0, 1), (0, 0), [(np.empty((2 * columns, 3), np.float32), np.empty((2 * columns, 4), np.uint8)) for _ in (0, 1)])
                    for gx, _ in got:
                        if gx.shape[0] != 2 * columns or not np.all(np.diff(gx[:, 0]) >= 0) or gx[-1, 0] > 5999:
                            errors.append(("strip", columns))
                frames[0] += 1
        except Exception as e:                                     # noqa: BLE001
            errors.append(("render", repr(e)))

    tp, tr = threading.Thread(target=producer), threading.Thread(target=render)
    tr.start(); tp.start(); tp.join(timeout=120); tr.join(timeout=120)
    assert not errors and not tp.is_alive() and not tr.is_alive(), errors[:3]
    assert frames[0] >= 8
    _feed([plain], x, block=160)
    assert dev.state() == plain.state()
    for c in range(2):
        (got, gcur), (want, wcur) = dev.front(c), plain.front(c)
        assert gcur == wcur and _same(got, want)
    _check(dev, 640)
    dev.close(); plain.close()


def test_create_read_destroy_gives_the_memory_back(gpu):
    """200 create -> push -> dense read (short and long form: the handle's scratch) -> destroy cycles after 8 to settle the allocators"""
    import os
    import psutil
    import torch
    x = _noise(17, 9000)

    def cycle():
        dev = api.Scope(**_cfg(window_size=8192.0, max_block=8192))
        _push(dev, x[:, :8192])
        dev.dense_vertices(640, 0, 0)
        dev.dense_vertices(2, 2, 0)
        dev.close()

    def free():
        gc.collect(); torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0], psutil.Process().memory_info().rss
    for _ in range(8):
        cycle()
    free0, rss0 = free()
    for _ in range(200):
        cycle()
    free1, rss1 = free()
    if "PYTEST_XDIST_WORKER" not in os.environ:                   # (the figure is the DEVICE's: other workers' allocations move it)
        assert free0 - free1 < 64 << 20, f"device memory: {(free0 - free1) / 2**20:.1f} MiB fewer free after 200 cycles"
    assert rss1 - rss0 < 96 << 20, f"host memory: resident set grew by {(rss1 - rss0) / 2**20:.1f} MiB over 200 cycles"
