"""The Oscilloscope's time modes (sgz_scope_config::time_mode, sgz_scope_set_tempo, sgz_scope_effective_window): handleFlagUpdates'
window step (Oscilloscope.cpp:291-307) at the top of every sgz_scope_analyse.

Cycles is held to the oracle's Spectral chain (oracle/scope_spectral.c) driven with the window the reference computes per frame,
cycles * (the last frame's cycleSamples) + 1, at the bars of tests/test_gpu_scope_stream.py::test_spectral_trigger_against_the_oracle.
Beats is held byte for byte to a Time handle given the same window (at creation, or by configure at the same frame boundaries), and
with the Spectral trigger to the oracle chain."""
import gc
import threading

import numpy as np
import pytest

from signalizer_amd import api

pytestmark = pytest.mark.gpu

BANDS = ((1.0, 0.2, 0.1), (0.1, 1.0, 0.3), (0.2, 0.3, 1.0))
LANCZOS, LINEAR = 3, 2
EM = {0: 0, 1: 0, 2: 1, 3: 2}          # evaluator -> the oracle's eval mode


def _push(dev, blk):
    """push never waits: SGZ_BUSY means the block was not taken -- offer it again"""
    while True:
        st = dev.push(blk)
        if st == api.SGZ_OK:
            return
        assert st == api.SGZ_BUSY


def _cfg(**over):
    cfg = dict(sample_rate=48000.0, window_size=2000.0, num_channels=2, trigger_mode=1, channel_mode=0, envelope_mode=2, interpolation=LANCZOS,
               max_block=4096, trigger_threshold=0.02, trigger_channel=1.0, envelope_window=0.3, trigger_hysteresis=0.0,
               trigger_phase_offset=30.0)
    cfg.update(over)
    return cfg


def _tone(n, sr, f0, seed, f1=None, harmonics=(1.0, 0.5, 0.25)):
    """a harmonic tone whose pitch glides geometrically from f0 to f1 (f1 None: constant), stereo, a little noise"""
    rng = np.random.default_rng(seed)
    f = np.full(n, f0) if f1 is None else f0 * (f1 / f0) ** (np.arange(n) / n)
    ph = 2 * np.pi * np.cumsum(f) / sr
    x = sum(a * np.sin((k + 1) * ph + 0.7 * k) for k, a in enumerate(harmonics))
    return np.stack([x + 0.01 * rng.standard_normal(n), 0.6 * x + 0.01 * rng.standard_normal(n)]).astype(np.float32)


def _eval_mem(mem, evaluator):
    return (mem[1], mem[1]) if evaluator == 1 else (mem[0], mem[1]) if EM[evaluator] else (mem[0], mem[0])


def _logical(m, cur, size):
    t = np.concatenate([m[cur:], m[:cur]])
    return t[len(t) - size:]


def _check_analysis(got, ts, frame):
    """the bars of test_spectral_trigger_against_the_oracle"""
    assert got.record_index == ts.record.index, (frame, got.record_index, ts.record.index)
    assert abs(got.record_value - ts.record.value) <= 1e-9 * max(1.0, ts.record.value)
    assert abs(got.record_offset - ts.record.offset) <= 1e-8
    assert abs(got.fundamental - ts.fundamental) <= 1e-8 * ts.fundamental
    assert abs(got.cycle_samples - ts.cycle_samples) <= 1e-8 * ts.cycle_samples
    assert abs(got.sample_offset - ts.sample_offset) <= 1e-6, (frame, got.sample_offset, ts.sample_offset)


def _check_vertices(po, dev, ref, got, window, sz, evaluator, trigger_mode=1):
    """this frame's vertices, Lanczos and Linear, against drawWavePlot on the reference's ring of the moment (the device's own
    window, cycleSamples and sampleOffset): x bit for bit, y within the existing bounds"""
    a, b = _eval_mem([ref.logical(c, sz) for c in (0, 1)], evaluator)
    # (at most 40001 pixels: the device places vertex p at left + p * inc, the oracle keeps a running sum, and over the 600 000 vertices
    # of a 300 000-sample window the two meet a float rounding boundary; a wider window than 20000 samples draws the Linear fallback)
    for interp, width in ((LANCZOS, min(2 * int(window) + 1, 40001)), (LINEAR, 300)):
        dev.configure(interpolation=interp)
        assert dev.effective_window() == window                           # (a configure keeps the frame's window)
        v = api.ScopeView(0.0, 0.0, 1.0, 1.0, width, 0)                   # (window_size is the handle's)
        vo = po.ScopeView(window, 0.0, 1.0, 1.0, width, 0)
        want, _ = po.scope_wave_plot_ex(vo, trigger_mode, interp, a, b, EM[evaluator], 0, got.cycle_samples, got.sample_offset)
        g, _ = dev.vertices(v, evaluator, 0)
        assert g.shape == want.shape, (interp, g.shape, want.shape)
        assert np.array_equal(g[:, 0], want[:, 0]), interp
        assert np.abs(g[:, 1] - want[:, 1]).max() <= (2e-6 if interp == LANCZOS else 0.0), interp


# ---------------------------------------------------------------------------------------------------------------------------- Cycles

@pytest.mark.parametrize("sr,cycles,f0,f1,evaluator,hyst,custom", [
    (48000.0, 2.0, 441.3, None, 0, 0.0, 0.0),              # steady pitch
    (44100.0, 0.5, 150.0, 420.0, 2, 0.3, 0.0),             # half a period, a rising glide across the frames, Mid
    (192000.0, 8.0, 1234.5, None, 1, 0.1, 0.0),            # eight periods at 192 kHz, Right
    (48000.0, 3.5, 900.0, 260.0, 3, 0.0, 0.0),             # a falling glide, Side
    (48000.0, 4.0, 220.0, None, 0, 0.0, 219.7),            # a custom trigger frequency
])
def test_cycles_matches_the_oracle_frame_by_frame(gpu, oracle, sr, cycles, f0, f1, evaluator, hyst, custom):
    po = oracle
    cfg = _cfg(sample_rate=sr, window_size=cycles, trigger_hysteresis=hyst, time_mode=api.TIME_CYCLES,
               custom_trigger=int(custom > 0), custom_trigger_frequency=custom)
    block, per_frame, frames = 1777, 6, 12
    x = _tone(block * per_frame * frames + 1, sr, f0, seed=4, f1=f1)
    dev = api.Scope(**cfg)
    assert dev.effective_window() == 1.0                                   # cycleSamples 0 before the first frame
    # the oracle's stream keeps the Spectral ring for the largest window Cycles can reach
    ref = po.ScopeStream(2, sr, cycles * (sr / 5.0) + 1, 1, 0.02, 0, 1.0, 2, 0.3)
    ts = po.SpectralState()
    sz = 8192                                                              # the ring before the first frame: window 1
    prev_dev_cs = 0.0
    pos = 0
    glide_seen = set()
    for frame in range(frames):
        for _ in range(per_frame):
            _push(dev, x[:, pos:pos + block]); ref.audio(x[:, pos:pos + block]); pos += block
        eff = cycles * ts.cycle_samples + 1                                # handleFlagUpdates, with the oracle's last cycleSamples
        a, b = _eval_mem([ref.logical(c, sz) for c in (0, 1)], evaluator)
        po.scope_analyse(ts, a, b, EM[evaluator], 0, eff, sr, 0.02, hyst, 30.0, custom)
        got = dev.analyse(evaluator, 0)
        window = dev.effective_window()
        assert window == cycles * prev_dev_cs + 1, (frame, window, cycles * prev_dev_cs + 1)     # bit for bit, computed on the device
        assert np.ceil(window) == np.ceil(eff), (frame, window, eff)
        _check_analysis(got, ts, frame)
        sz = max(int(0.5 + ts.cycle_samples + np.ceil(eff)), 8192)
        assert got.ring_size == sz, (frame, got.ring_size, sz)
        glide_seen.add(round(got.fundamental))
        if frame in (0, 1, 2, 7, 11):
            _check_vertices(po, dev, ref, got, window, sz, evaluator)
        prev_dev_cs = got.cycle_samples
    if f1 is not None:
        assert len(glide_seen) > 4                                         # the window really moved with the pitch
    dev.close()


# ----------------------------------------------------------------------------------------------------------------------------- Beats

def _full_state(dev, evaluator=0):
    """everything a frame reads from a handle, flush on read first"""
    ts = dev.analyse(evaluator, 0)
    out = dict(analyse=bytes(ts), state=dev.state(), gains=dev.gains(), window=dev.effective_window())
    size = int(ts.ring_size)
    for c in range(dev.cfg.num_channels):
        m, cur = dev.front(c)
        out[f"front{c}"] = (_logical(m, cur, size) if dev.cfg.trigger_mode == 1 else m).tobytes()
        out[f"cursor{c}"] = cur if dev.cfg.trigger_mode != 1 else None
        if dev.cfg.colour_by_frequency:
            for aux in (False, True):
                col = dev.front_colours(c, aux)
                out[f"colour{c}{aux}"] = (_logical(col, cur, size) if dev.cfg.trigger_mode == 1 else col).tobytes()
    return out


def _assert_same_frame(beats, twin, evaluator=0):
    a, b = _full_state(beats, evaluator), _full_state(twin, evaluator)
    for k in a:
        if k == "gains":
            assert a[k][0] == b[k][0] and np.array_equal(a[k][1].view(np.uint32), b[k][1].view(np.uint32)), k
        else:
            assert a[k] == b[k], k
    for interp, width in ((LANCZOS, 2 * int(a["window"]) + 1), (LINEAR, 333)):
        for h in (beats, twin):
            h.configure(interpolation=interp)
        v = api.ScopeView(0.0, 0.0, 1.0, 1.0, width, 0)
        for ev in range(4):
            (gx, gc), (wx, wc) = beats.vertices(v, ev, 0), twin.vertices(v, ev, 0)
            assert gx.shape == wx.shape and np.array_equal(gx.view(np.uint32), wx.view(np.uint32)), (interp, ev)
            assert np.array_equal(gc, wc), (interp, ev)


def _beats_cfg(trigger, **over):
    cfg = _cfg(trigger_mode=trigger, trigger_threshold=0.05, trigger_hysteresis=0.1, envelope_mode=1 if trigger != 1 else 2,
               colour_by_frequency=1, frequency_colouring_blend=0.6, colour_smoothing_ms=3.0, band_colours=BANDS,
               colours=[(10, 20, 30, 255), (200, 100, 50, 255)])
    cfg.update(over)
    return cfg


@pytest.mark.parametrize("trigger", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("sr,value,bpm", [
    (48000.0, 4.0, 120.0),      # 6000 samples
    (48000.0, 64.0, None),      # no tempo ever set: the 10 BPM floor, 4500 samples
    (44100.0, 128.0, 300.0),    # 68.9 samples -> the 128-sample floor
])
def test_beats_at_a_constant_tempo_is_the_time_mode(gpu, trigger, sr, value, bpm):
    cfg = _beats_cfg(trigger, sample_rate=sr)
    window = api.time_window(api.TIME_BEATS, value, sr, 0.0 if bpm is None else bpm)
    beats = api.Scope(**dict(cfg, window_size=value, time_mode=api.TIME_BEATS))
    twin = api.Scope(**dict(cfg, window_size=window))
    if bpm is not None:
        beats.set_tempo(bpm)
    for h in (beats, twin):
        h.set_transport(123457)
    beats.analyse(0, 0)
    twin.analyse(0, 0)
    assert beats.effective_window() == window == twin.effective_window()
    x = _tone(40000, sr, 441.3, seed=7)
    pos = 0
    rng = np.random.default_rng(3)
    for frame in range(4):
        for _ in range(4):
            n = int(rng.integers(200, 2500))
            for h in (beats, twin):
                _push(h, x[:, pos:pos + n])
            pos += n
        _assert_same_frame(beats, twin, evaluator=frame % 4)
    if trigger == 4:
        assert twin.state()["swaps"] > 5
    beats.close(); twin.close()


TEMPI = [120.0, 120.0, 90.0, 90.5, 200.0, 60.0, 60.0, 333.3, 37.0, 120.0]


@pytest.mark.parametrize("trigger", [0, 2, 3, 4])
def test_beats_tempo_changes_are_configures(gpu, trigger):
    """another trigger than Spectral: a new frame window does what configure(window_size = window) does, at the same frame boundary"""
    sr, value = 48000.0, 2.0
    cfg = _beats_cfg(trigger, sample_rate=sr)
    beats = api.Scope(**dict(cfg, window_size=value, time_mode=api.TIME_BEATS))
    twin = api.Scope(**dict(cfg, window_size=api.time_window(api.TIME_BEATS, value, sr, 0.0)))
    assert beats.effective_window() == twin.effective_window()
    x = _tone(len(TEMPI) * 5 * 1500, sr, 300.0, seed=9, f1=700.0)
    pos = 0
    rng = np.random.default_rng(5)
    last = beats.effective_window()
    sizes = set()
    for frame, bpm in enumerate(TEMPI):
        beats.set_tempo(bpm)
        window = api.time_window(api.TIME_BEATS, value, sr, bpm)
        beats.analyse(0, 0)
        if window != last:
            twin.configure(window_size=window)
            last = window
        assert beats.effective_window() == window
        _assert_same_frame(beats, twin, evaluator=frame % 4)
        sizes.add(beats.front(0)[0].size)
        for _ in range(5):
            n = int(rng.integers(100, 3000))
            for h in (beats, twin):
                _push(h, x[:, pos:pos + n])
            pos += n
    _assert_same_frame(beats, twin)
    assert len(sizes) >= 5                                               # the rings really were resized
    beats.close(); twin.close()


def test_beats_spectral_tempo_changes_against_the_oracle(gpu, oracle):
    """the Spectral trigger: the frame's window follows the tempo, the ring is never reallocated or cleared"""
    po = oracle
    sr, value, evaluator = 48000.0, 4.0, 0
    cfg = _cfg(sample_rate=sr, window_size=value, time_mode=api.TIME_BEATS, trigger_hysteresis=0.1)
    dev = api.Scope(**cfg)
    ref = po.ScopeStream(2, sr, api.time_window(api.TIME_BEATS, value, sr, 0.0), 1, 0.02, 0, 1.0, 2, 0.3)
    ts = po.SpectralState()
    x = _tone(len(TEMPI) * 6 * 1777 + 1, sr, 441.3, seed=4)
    size0 = dev.front(0)[0].size
    sz = None
    pos = 0
    for frame, bpm in enumerate(TEMPI):
        for _ in range(6):
            _push(dev, x[:, pos:pos + 1777]); ref.audio(x[:, pos:pos + 1777]); pos += 1777
        dev.set_tempo(bpm)
        eff = api.time_window(api.TIME_BEATS, value, sr, bpm)
        if sz is None:
            sz = max(int(0.5 + 0.0 + np.ceil(eff)), 8192)                  # the ring before the first frame: the first frame's window
        a, b = _eval_mem([ref.logical(c, sz) for c in (0, 1)], evaluator)
        po.scope_analyse(ts, a, b, EM[evaluator], 0, eff, sr, 0.02, 0.1, 30.0)
        got = dev.analyse(evaluator, 0)
        assert dev.effective_window() == eff
        _check_analysis(got, ts, frame)
        sz = max(int(0.5 + ts.cycle_samples + np.ceil(eff)), 8192)
        assert got.ring_size == sz, (frame, got.ring_size, sz)
        # nothing cleared: the handle's ring holds every sample pushed (as the oracle's), older tempi's included
        m, cur = dev.front(0)
        assert m.size == size0
        keep = min(pos, m.size, ref.size)
        assert np.array_equal(_logical(m, cur, keep), ref.logical(0, keep)), frame
        if frame in (0, 3, 7):
            _check_vertices(po, dev, ref, got, eff, sz, evaluator)
    dev.close()


# ------------------------------------------------------------------------------------------------------------ refusals and lifecycle

def _results(dev):
    """what the handle holds (a Spectral analyse is itself a step of the state: only the other modes' is read here)"""
    ts = bytes(dev.analyse(0, 0)) if dev.cfg.trigger_mode != 1 else None
    return ts, dev.state(), dev.front(0)[0].tobytes(), dev.front(0)[1], dev.effective_window()


@pytest.mark.parametrize("base", [
    dict(trigger_mode=4, window_size=1000.0),
    dict(trigger_mode=1, window_size=2.0, time_mode=api.TIME_CYCLES),
    dict(trigger_mode=3, window_size=4.0, time_mode=api.TIME_BEATS),
])
def test_invalid_time_modes_are_refused_and_change_nothing(gpu, base):
    cfg = _cfg(**base)
    dev = api.Scope(**cfg)
    dev.set_tempo(140.0)
    x = _tone(20000, 48000.0, 330.0, seed=2)
    for pos in range(0, 20000, 2000):
        _push(dev, x[:, pos:pos + 2000])
    before = _results(dev)
    bad = [dict(time_mode=api.TIME_CYCLES, trigger_mode=t, window_size=2.0) for t in (0, 2, 3, 4)]      # Cycles needs Spectral
    for mode in (api.TIME_CYCLES, api.TIME_BEATS):
        for trig in (1, 4):
            if mode == api.TIME_CYCLES and trig != 1:
                continue
            bad += [dict(time_mode=mode, trigger_mode=trig, window_size=v) for v in (0.0, -1.0, float("nan"), float("inf"))]
    bad += [dict(time_mode=api.TIME_CYCLES, trigger_mode=1, window_size=2000.0, sample_rate=192000.0),  # 2000 * 38400 + 1 > 2^26
            dict(time_mode=api.TIME_CYCLES, trigger_mode=1, window_size=2.0, custom_trigger=1, custom_trigger_frequency=0.001),
            dict(time_mode=api.TIME_BEATS, trigger_mode=4, window_size=0.01, sample_rate=192000.0),    # 1.152e8 samples at 10 BPM
            dict(time_mode=api.TIME_BEATS, trigger_mode=1, window_size=0.01, sample_rate=192000.0),
            dict(time_mode=3, trigger_mode=4, window_size=1000.0)]
    for over in bad:
        with pytest.raises(api.SgzError) as e:
            api.Scope(**_cfg(**dict(base, **over)))
        assert e.value.status == api.SGZ_EINVAL, over
        saved = api.ScopeConfig.from_buffer_copy(dev.cfg)
        with pytest.raises(api.SgzError) as e:
            dev.configure(**over)
        assert e.value.status == api.SGZ_EINVAL, over
        dev.cfg = saved
        assert _results(dev) == before, over
    # the bounds are not tighter than they say: a Cycles ring for 100 periods of 5 Hz, Beats at 1/16 of a beat of 10 BPM
    api.Scope(**_cfg(time_mode=api.TIME_CYCLES, trigger_mode=1, window_size=100.0)).close()
    api.Scope(**_cfg(time_mode=api.TIME_BEATS, trigger_mode=4, window_size=1 / 16)).close()
    dev.close()


def test_set_tempo_beside_a_pushing_thread(gpu):
    """set_tempo on a second thread while a third pushes and this one renders frames: push only ever says OK or BUSY (a frame that
    resizes the rings holds the handle; the push is refused, it never waits or fails)"""
    cfg = _cfg(trigger_mode=4, trigger_threshold=0.05, window_size=2.0, time_mode=api.TIME_BEATS, envelope_mode=1)
    dev = api.Scope(**cfg)
    x = _tone(512 * 64, 48000.0, 330.0, seed=1)
    stop = threading.Event()
    statuses = []

    def producer():
        i = 0
        while not stop.is_set():
            statuses.append(dev.push(x[:, (i % 64) * 512:(i % 64 + 1) * 512]))
            i += 1

    def tempo():
        rng = np.random.default_rng(0)
        while not stop.is_set():
            dev.set_tempo(float(rng.uniform(40, 240)))

    threads = [threading.Thread(target=producer), threading.Thread(target=tempo)]
    for t in threads:
        t.start()
    windows = set()
    try:
        for _ in range(200):
            dev.analyse(0, 0)
            windows.add(dev.effective_window())
    finally:
        stop.set()
        for t in threads:
            t.join(60)
    assert not any(t.is_alive() for t in threads)
    assert statuses and set(statuses) <= {api.SGZ_OK, api.SGZ_BUSY}, set(statuses)
    assert len(windows) > 20
    dev.state()                                                          # the handle still works
    dev.close()


@pytest.mark.parametrize("trigger", [1, 4])
def test_tempo_changes_leave_device_memory_flat(gpu, trigger):
    import torch
    dev = api.Scope(**_cfg(trigger_mode=trigger, trigger_threshold=0.05, window_size=1.0, time_mode=api.TIME_BEATS))
    x = _tone(4096, 48000.0, 330.0, seed=1)

    def changes(k0, n):
        for k in range(k0, k0 + n):
            dev.set_tempo(60.0 + 7.3 * (k % 23))
            dev.analyse(0, 0)
            _push(dev, x[:, :1024])
        dev.flush()

    changes(0, 10)
    gc.collect(); torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    changes(10, 100)
    gc.collect(); torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    import os
    if "PYTEST_XDIST_WORKER" not in os.environ:
        assert free0 - free1 < 16 << 20, f"device memory: {(free0 - free1) / 2**20:.1f} MiB fewer free after 100 tempo changes"
    dev.close()
