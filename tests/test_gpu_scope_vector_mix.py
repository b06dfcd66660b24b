"""Host-graph routing on the Oscilloscope and Vectorscope handles (sgz_scope_set_mix / sgz_vector_set_mix, MixGraphListener::deliver):
the ingest launch sums the routed source channels into the destination rows itself.

Built on twin handles: handle A gets set_mix(M) and the source channels; handle B keeps the identity and gets the same blocks mixed on
the host in numpy float32 (np.zeros, then each routed source added in ascending order, as copyFromHead<true> into a cleared row does).
Everything the handles expose must then match bit for bit."""
import ctypes as C
import gc
import threading

import numpy as np
import pytest

from signalizer_amd import api

pytestmark = pytest.mark.gpu

SR = 192000.0
VSR = 96000.0
BANDS = [(1.0, 0.25, 0.1), (0.2, 1.0, 0.3), (0.15, 0.35, 1.0)]
KEYS = [(10, 20, 30, 255), (200, 100, 50, 255), (0, 255, 0, 128), (90, 90, 255, 255)]


def _mix(M, src):
    """the reference's deliver() on the host: destination d = 0.0f + the routed sources in ascending order"""
    out = np.zeros((M.shape[0], src.shape[1]), np.float32)
    for d in range(M.shape[0]):
        for c in range(M.shape[1]):
            if M[d, c]:
                out[d] = out[d] + src[c]
    return out


def _matrix(seed, dst, src):
    """random routing with a source sent to several destinations and (with more than one destination) a destination with no source"""
    rng = np.random.default_rng(seed)
    M = (rng.random((dst, src)) < 0.35).astype(np.uint8)
    M[: min(dst, 3), 0] = 1                                    # source 0 -> up to three destinations
    if dst > 1:
        M[-1] = 0                                              # the last destination is silence
    return M


def _sources(seed, n, channels, sr=SR, f0=441.7, nonfinite=False):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = np.zeros((channels, n), np.float32)
    for c in range(channels):
        x[c] = (0.5 * np.sin(2 * np.pi * f0 * (1 + 0.13 * c) * t + 0.4 * c) + 0.2 * np.sin(2 * np.pi * 4.7 * f0 * t)
                + 0.05 * rng.standard_normal(n)).astype(np.float32)
    for c in range(channels):                                  # negative zeros: +0.0 once mixed (0.0f + -0.0f)
        x[c, rng.integers(0, n, 40)] = -0.0
        x[c, 3000 + 64 * c: 3100 + 64 * c] = -0.0
    if nonfinite:
        x[0, 5000] = np.nan
        x[min(1, channels - 1), 7000] = np.inf
        x[channels - 1, 9000] = -np.inf
    return x


def _push(dev, blk):
    while True:
        st = dev.push(blk)
        if st == api.SGZ_OK:
            return
        assert st == api.SGZ_BUSY


def _same(a, b, nan=False):
    a, b = np.asarray(a), np.asarray(b)
    if nan and a.dtype.kind == "f":
        return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- Oscilloscope ----------------------------------------------------------------------------------------------------------------------

def _scope_cfg(**over):
    cfg = dict(sample_rate=SR, window_size=1500.5, num_channels=2, trigger_mode=4, channel_mode=0, envelope_mode=1, interpolation=3,
               max_block=4096, trigger_threshold=0.05, trigger_channel=1.0, envelope_window=0.3)
    cfg.update(over)
    return cfg


def _scope_equal(a, b, cfg, nan=False):
    """every reader of the two handles, called the same way on both"""
    C_ = cfg["num_channels"]
    assert a.state() == b.state()
    for c in range(C_):
        fa, ca = a.front(c)
        fb, cb = b.front(c)
        assert ca == cb and _same(fa, fb, nan), f"front ring of channel {c}"
        if cfg.get("colour_by_frequency"):
            for aux in (False, True):
                assert _same(a.front_colours(c, aux), b.front_colours(c, aux)), f"colour ring of channel {c} (aux {aux})"
    ga, ea = a.gains()
    gb, eb = b.gains()
    assert (ga == gb or (nan and np.isnan(ga) and np.isnan(gb))) and _same(ea, eb, nan)
    pa, pb = a.peak_filter(1 / 60, 8), b.peak_filter(1 / 60, 8)
    assert pa == pb or (nan and np.isnan(pa) and np.isnan(pb))
    if cfg["trigger_mode"] == 1:
        for ev in (0, 2):
            ta, tb = a.analyse(ev, 0), b.analyse(ev, 0)
            assert bytes(ta) == bytes(tb), f"spectral trigger state (evaluator {ev})"
    view = api.ScopeView(cfg["window_size"], 0.0, 1.0, 1.0, 900, 0)
    for ev in (0, 2):
        for ch in range(0, C_, max(2, C_ // 4)):
            xa, ra = a.vertices(view, ev, ch)
            xb, rb = b.vertices(view, ev, ch)
            assert _same(xa, xb, nan) and _same(ra, rb), f"vertices (evaluator {ev}, channel {ch})"


SCOPE_CASES = [
    # (config, num_sources, block)
    (dict(trigger_mode=4, channel_mode=0, colour_by_frequency=1, frequency_colouring_blend=0.6, colour_smoothing_ms=4.0), 6, 512),
    (dict(trigger_mode=3, channel_mode=2, num_channels=4, window_size=3000.0, trigger_hysteresis=0.1, interpolation=2), 1, 333),
    (dict(trigger_mode=1, channel_mode=4, num_channels=64, window_size=2000.0, trigger_threshold=0.02, trigger_hysteresis=0.1,
          trigger_phase_offset=30.0, sample_rate=48000.0, envelope_mode=2), 64, 4096),
    (dict(trigger_mode=0, channel_mode=5, window_size=900.0, colour_by_frequency=1, frequency_colouring_blend=0.3, colour_smoothing_ms=1.0), 64, 480),
    (dict(trigger_mode=4, channel_mode=4, num_channels=4, trigger_channel=3.0, interpolation=2), 6, 480),
]


def _scope_pair(cfg, defer=False, park=False):
    extra = dict(band_colours=BANDS, colours=KEYS * 16) if cfg.get("colour_by_frequency") else {}
    a, b = api.Scope(**cfg, **extra), api.Scope(**cfg, **extra)
    for h in (a, b):
        if defer:
            h.set_option(api.RT_OPT_DEFER_SUBMIT, 1)
        if park:
            h.set_option(api.RT_OPT_PARK_PUSHES, 1)
    return a, b


@pytest.mark.parametrize("case", range(len(SCOPE_CASES)))
@pytest.mark.parametrize("defer", [False, True])
def test_scope_mix_equals_the_host_mixed_twin(gpu, case, defer):
    over, S, block = SCOPE_CASES[case]
    cfg = _scope_cfg(**over)
    D = cfg["num_channels"]
    M = _matrix(10 + case, D, S)
    x = _sources(case, 24 * block if block < 4096 else 8 * block, S, cfg["sample_rate"])
    a, b = _scope_pair(cfg, defer=defer)
    a.set_mix(M)
    for pos in range(0, x.shape[1], block):
        blk = x[:, pos:pos + block]
        _push(a, blk)
        _push(b, _mix(M, blk))
    _scope_equal(a, b, cfg)
    a.close(); b.close()


def test_scope_mix_with_non_finite_sources(gpu):
    cfg = _scope_cfg(trigger_mode=4, channel_mode=4, num_channels=4, envelope_mode=1)
    M = _matrix(3, 4, 6)
    x = _sources(5, 20000, 6, nonfinite=True)
    a, b = _scope_pair(cfg)
    a.set_mix(M)
    for pos in range(0, x.shape[1], 512):
        _push(a, x[:, pos:pos + 512])
        _push(b, _mix(M, x[:, pos:pos + 512]))
    _scope_equal(a, b, cfg, nan=True)
    a.close(); b.close()


def test_scope_mix_against_the_oracle(gpu, oracle):
    """the numpy-mixed stream through the oracle's restatement of the audio-thread state machine"""
    po = oracle
    cfg = _scope_cfg(trigger_mode=4, channel_mode=2, num_channels=4, envelope_mode=1, window_size=777.0, trigger_threshold=0.1)
    M = _matrix(7, 4, 6)
    x = _sources(9, 40000, 6)
    dev = api.Scope(**cfg)
    dev.set_mix(M)
    ref = po.ScopeStream(cfg["num_channels"], cfg["sample_rate"], cfg["window_size"], cfg["trigger_mode"], cfg["trigger_threshold"],
                         cfg["channel_mode"], cfg["trigger_channel"], cfg["envelope_mode"], cfg["envelope_window"])
    rng = np.random.default_rng(2)
    pos = 0
    while pos < x.shape[1]:
        n = int(rng.integers(1, 2000))
        blk = x[:, pos:pos + n]
        _push(dev, blk)
        ref.audio(_mix(M, blk))
        pos += blk.shape[1]
    assert dev.state() == ref.state()
    for c in range(4):
        got, gcur = dev.front(c)
        want, wcur = ref.front(c)
        assert gcur == wcur and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    dev.close()


# ---- Vectorscope -----------------------------------------------------------------------------------------------------------------------

def _vector_cfg(**over):
    cfg = dict(sample_rate=VSR, num_channels=2, window_size=2000, envelope_mode=1, lanes=8, fade_history=1, max_block=4096,
               envelope_window=0.3, stereo_window=0.05, colours=[(1.0, 0.5, 0.25), (0.2, 0.9, 0.4)] * 16)
    cfg.update(over)
    return cfg


def _vector_equal(a, b, cfg, nan=False):
    D = cfg["num_channels"]
    for c in range(D):
        ha, ca = a.history(c)
        hb, cb = b.history(c)
        assert ca == cb and _same(ha, hb, nan), f"history of channel {c}"
    fa, ga = a.filters()
    fb, gb = b.filters()
    assert bytes(fa) == bytes(fb) or (nan and _same(np.frombuffer(bytes(fa), np.float32), np.frombuffer(bytes(fb), np.float32), True))
    assert ga == gb or (nan and np.isnan(ga) and np.isnan(gb))
    if not nan:
        assert bytes(a.meters()) == bytes(b.meters())
    pa, pb = a.peak_filter(1 / 60), b.peak_filter(1 / 60)
    assert pa == pb or (nan and np.isnan(pa) and np.isnan(pb))
    for pair in range(0, D // 2, max(1, D // 8)):
        for draw in (a.vertices, a.lissajous):
            other = getattr(b, draw.__name__)
            xa, ra = draw(pair)
            xb, rb = other(pair)
            assert _same(xa, xb, nan) and _same(ra, rb, nan), f"{draw.__name__} of pair {pair}"


VECTOR_CASES = [
    # (config, num_sources, block)
    (dict(num_channels=2, envelope_mode=2, fade_history=1), 6, 512),
    (dict(num_channels=4, envelope_mode=1, fade_history=0, window_size=777), 1, 333),
    (dict(num_channels=64, envelope_mode=0, fade_history=1, window_size=4096), 64, 4096),
    (dict(num_channels=2, envelope_mode=1, fade_history=0, window_size=9600), 64, 480),
    (dict(num_channels=4, envelope_mode=2, fade_history=1), 6, 333),
]


@pytest.mark.parametrize("case", range(len(VECTOR_CASES)))
@pytest.mark.parametrize("defer", [False, True])
def test_vector_mix_equals_the_host_mixed_twin(gpu, case, defer):
    over, S, block = VECTOR_CASES[case]
    cfg = _vector_cfg(**over)
    D = cfg["num_channels"]
    M = _matrix(20 + case, D, S)
    x = _sources(30 + case, 24 * block if block < 4096 else 8 * block, S, VSR)
    a, b = api.Vector(**cfg), api.Vector(**cfg)
    if defer:
        a.set_option(api.RT_OPT_DEFER_SUBMIT, 1); b.set_option(api.RT_OPT_DEFER_SUBMIT, 1)
    a.set_mix(M)
    for pos in range(0, x.shape[1], block):
        blk = x[:, pos:pos + block]
        _push(a, blk)
        _push(b, _mix(M, blk))
    _vector_equal(a, b, cfg)
    a.close(); b.close()


def test_vector_mix_with_non_finite_sources(gpu):
    cfg = _vector_cfg(num_channels=4, envelope_mode=1)
    M = _matrix(4, 4, 6)
    x = _sources(6, 20000, 6, VSR, nonfinite=True)
    a, b = api.Vector(**cfg), api.Vector(**cfg)
    a.set_mix(M)
    for pos in range(0, x.shape[1], 512):
        _push(a, x[:, pos:pos + 512])
        _push(b, _mix(M, x[:, pos:pos + 512]))
    _vector_equal(a, b, cfg, nan=True)
    a.close(); b.close()


def test_vector_mix_against_the_oracle(gpu, oracle):
    """the numpy-mixed stream through the oracle's ring + audioProcessing (as tests/test_gpu_vector_stream.py drives it)"""
    po = oracle
    cfg = _vector_cfg(num_channels=4, window_size=1000, envelope_mode=1)
    M = _matrix(8, 4, 6)
    x = _sources(12, 30000, 6, VSR)
    dev = api.Vector(**cfg)
    dev.set_mix(M)
    size = cfg["window_size"]
    mem = np.zeros((4, size), np.float32)
    cursor = 0
    f = po.VectorFilters()
    ec = float(np.float32(np.exp(-1.0 / (0.3 * VSR))))
    sc = float(np.float32(np.exp(-1.0 / (0.05 * VSR))))
    gain = 1.0
    rng = np.random.default_rng(3)
    pos = 0
    while pos < x.shape[1]:
        n = int(rng.integers(1, 3000))
        blk = x[:, pos:pos + n]
        _push(dev, blk)
        m = _mix(M, blk)
        mem[:, (cursor + np.arange(m.shape[1])) % size] = m
        cursor = int((cursor + m.shape[1]) % size)
        g = po.vector_audio_processing(f, m[0], m[1], ec, sc, 0.25, 1, 8)
        if np.isfinite(g):
            gain = g
        pos += blk.shape[1]
    for c in range(4):
        got, cur = dev.history(c)
        assert cur == cursor and np.array_equal(got.view(np.uint32), mem[c].view(np.uint32))
    fd, gd = dev.filters()
    assert np.array_equal(np.array(fd.env[:], np.float32).view(np.uint32), np.array(f.env[:], np.float32).view(np.uint32))
    gb = np.array([list(r) for r in fd.balance], np.float32)
    rb = np.array([list(r) for r in f.balance], np.float32)
    assert np.array_equal(gb.view(np.uint32), rb.view(np.uint32))
    assert np.float32(gd) == np.float32(gain)
    dev.close()


# ---- both handles: routing changes, identity, configure, limits, threads, lifecycle ----------------------------------------------------

def _handles(kind, cfg, defer=False, park=False):
    if kind == "scope":
        return _scope_pair(cfg, defer, park)
    a, b = api.Vector(**cfg), api.Vector(**cfg)
    for h in (a, b):
        if defer:
            h.set_option(api.RT_OPT_DEFER_SUBMIT, 1)
        if park:
            h.set_option(api.RT_OPT_PARK_PUSHES, 1)
    return a, b


def _equal(kind, a, b, cfg):
    (_scope_equal if kind == "scope" else _vector_equal)(a, b, cfg)


def _kind_cfg(kind, channels=4):
    return _scope_cfg(num_channels=channels, channel_mode=4, trigger_channel=1.0) if kind == "scope" else _vector_cfg(num_channels=channels)


@pytest.mark.parametrize("kind", ["scope", "vector"])
@pytest.mark.parametrize("opt", ["defer", "park"])
def test_routing_change_mid_stream(gpu, kind, opt):
    """blocks under M1, set_mix(M2) with blocks still waiting (deferred in the open batch, or parked in the host FIFO), more blocks:
    the waiting blocks went through M1"""
    cfg = _kind_cfg(kind)
    M1, M2 = _matrix(40, 4, 6), _matrix(41, 4, 3)
    x1, x2 = _sources(42, 512 * 11, 6), _sources(43, 512 * 9, 3)
    a, b = _handles(kind, cfg, defer=opt == "defer", park=opt == "park")
    a.set_mix(M1)
    for pos in range(0, x1.shape[1], 512):
        _push(a, x1[:, pos:pos + 512]); _push(b, _mix(M1, x1[:, pos:pos + 512]))
    a.set_mix(M2)
    for pos in range(0, x2.shape[1], 512):
        _push(a, x2[:, pos:pos + 512]); _push(b, _mix(M2, x2[:, pos:pos + 512]))
    _equal(kind, a, b, cfg)
    a.close(); b.close()


@pytest.mark.parametrize("kind", ["scope", "vector"])
def test_identity_set_mix_is_the_default_path(gpu, kind):
    cfg = _kind_cfg(kind)
    x = _sources(50, 512 * 20, 4)
    a, b = _handles(kind, cfg)
    a.set_mix(np.eye(4, dtype=np.uint8))
    for pos in range(0, x.shape[1], 480):
        _push(a, x[:, pos:pos + 480]); _push(b, x[:, pos:pos + 480])
    _equal(kind, a, b, cfg)
    a.close(); b.close()


def _raw_push(h, kind, blk):
    blk = np.ascontiguousarray(blk, np.float32)
    ptrs = (C.c_void_p * blk.shape[0])(*[blk[c].ctypes.data for c in range(blk.shape[0])])
    return getattr(api.lib(), f"sgz_{kind}_push")(h.h, ptrs, blk.shape[0], blk.shape[1])


@pytest.mark.parametrize("kind", ["scope", "vector"])
def test_source_count_refusals_leave_the_stream_unchanged(gpu, kind):
    """bad set_mix arguments are refused and change nothing; push takes num_sources channels after set_mix and num_channels again after
    configure; every refused push leaves the stream as it was"""
    L = api.lib()
    set_mix = getattr(L, f"sgz_{kind}_set_mix")
    cfg = _kind_cfg(kind)
    M = _matrix(60, 4, 6)
    xs, xd = _sources(61, 512 * 8, 6), _sources(62, 512 * 8, 4)
    a, b = _handles(kind, cfg)
    a.set_mix(M)
    m = np.ascontiguousarray(M)
    assert set_mix(a.h, 6, None) == api.SGZ_EINVAL
    assert set_mix(a.h, 0, m.ctypes.data) == api.SGZ_EINVAL
    big = np.ones((4, 65), np.uint8)
    assert set_mix(a.h, 65, big.ctypes.data) == api.SGZ_EINVAL
    for pos in range(0, 512 * 4, 512):                             # still M over 6 sources
        assert _raw_push(a, kind, xd[:, pos:pos + 512]) == api.SGZ_EINVAL
        _push(a, xs[:, pos:pos + 512]); _push(b, _mix(M, xs[:, pos:pos + 512]))
    for h in (a, b):                                               # the same configuration again: only the routing is reset
        api.check(getattr(L, f"sgz_{kind}_configure")(h.h, C.byref(h.cfg)))
    for pos in range(512 * 4, 512 * 8, 512):                       # identity over num_channels again
        assert _raw_push(a, kind, xs[:, pos:pos + 512]) == api.SGZ_EINVAL
        _push(a, xd[:, pos:pos + 512]); _push(b, xd[:, pos:pos + 512])
    _equal(kind, a, b, cfg)
    a.close(); b.close()


@pytest.mark.parametrize("kind", ["scope", "vector"])
def test_both_handles_answer_misuse_with_the_same_status(gpu, kind):
    """one walk through the entry points' refusals, the same for both handles: every refused call returns its status and leaves the
    stream alone, and the handle ends up equal to a twin that only saw the accepted blocks"""
    L = api.lib()
    call = lambda name, h, *args: getattr(L, f"sgz_{kind}_{name}")(h.h, *args)      # noqa: E731
    if kind == "scope":
        cfg = _scope_cfg(num_channels=2, window_size=64.0, max_block=16, trigger_mode=0)
    else:
        cfg = _vector_cfg(num_channels=2, window_size=64, max_block=16)
    x = _sources(90, 3 * 8, 3, cfg["sample_rate"])
    a, b = _handles(kind, cfg)
    assert _raw_push(a, kind, x[:, :8]) == api.SGZ_EINVAL                  # 3 channels into a 2-channel handle
    assert _raw_push(a, kind, x[:2, :0]) == api.SGZ_OK                     # no samples: accepted, nothing consumed
    assert _raw_push(a, kind, np.zeros((2, 17), np.float32)) == api.SGZ_EINVAL      # longer than max_block
    assert call("set_option", a, 99, 1) == api.SGZ_EINVAL                  # no such option
    assert call("set_mix", a, 0, np.ones((2, 1), np.uint8).ctypes.data) == api.SGZ_EINVAL
    assert call("set_mix", a, 65, np.ones((2, 65), np.uint8).ctypes.data) == api.SGZ_EINVAL
    assert call("set_option", a, api.RT_OPT_PARK_PUSHES, 1) == api.SGZ_OK
    for pos in range(0, 24, 8):
        assert _raw_push(a, kind, x[:2, pos:pos + 8]) == api.SGZ_OK        # parked in the host FIFO
        _push(b, x[:2, pos:pos + 8])
    assert call("flush", a) == api.SGZ_OK
    for c in range(2):
        got, gcur = a.front(c) if kind == "scope" else a.history(c)
        want, wcur = b.front(c) if kind == "scope" else b.history(c)
        assert gcur == wcur and _same(got, want), f"channel {c}"
    a.close(); b.close()


@pytest.mark.parametrize("kind", ["scope", "vector"])
def test_full_batch_at_the_maximum_shape(gpu, kind):
    """64 sources into 64 channels at max_block 8192, deferred submission: every batch is a full slot"""
    if kind == "scope":
        cfg = _scope_cfg(num_channels=64, channel_mode=4, trigger_mode=4, max_block=8192, window_size=3000.0, envelope_mode=1)
    else:
        cfg = _vector_cfg(num_channels=64, max_block=8192, window_size=6000, envelope_mode=1)
    M = _matrix(70, 64, 64)
    x = _sources(71, 8192 * 3 + 512 * 16, 64)
    a, b = _handles(kind, cfg, defer=True)
    a.set_mix(M)
    for pos in range(0, 8192 * 3, 8192):
        _push(a, x[:, pos:pos + 8192]); _push(b, _mix(M, x[:, pos:pos + 8192]))
    for pos in range(8192 * 3, x.shape[1], 512):                   # sixteen blocks: the batch's block table full as well
        _push(a, x[:, pos:pos + 512]); _push(b, _mix(M, x[:, pos:pos + 512]))
    _equal(kind, a, b, cfg)
    a.close(); b.close()


@pytest.mark.parametrize("kind", ["scope", "vector"])
def test_set_mix_while_the_audio_thread_pushes(gpu, kind):
    """a producer thread pushes flat out while the consumer switches the routing (and renders): every push returns OK or BUSY at once,
    and the handle equals the twin fed exactly the accepted blocks, each under the routing it was accepted with.  The history is long
    enough to hold the whole stream, and the two routings send different sources to destination 0, so the stream itself says where
    the switch fell."""
    n_blocks, blk_n = 600, 160
    total = n_blocks * blk_n
    if kind == "scope":
        cfg = _scope_cfg(num_channels=2, trigger_mode=0, envelope_mode=1, window_size=float(total + 16), max_block=4096)
    else:
        cfg = _vector_cfg(num_channels=2, window_size=total + 16, envelope_mode=1)
    M1 = np.array([[1, 0, 0], [0, 1, 1]], np.uint8)
    M2 = np.array([[0, 1, 0], [1, 0, 1]], np.uint8)
    x = _sources(80, total, 3)
    x[1] = x[0] + np.float32(0.5)                                # source 1 differs from source 0 in every sample
    a = api.Vector(**cfg) if kind == "vector" else api.Scope(**cfg)
    a.set_mix(M1)
    errors, accepted, switched = [], [], [None, None]
    done = threading.Event()

    def producer():
        try:
            for i in range(n_blocks):
                blk = np.ascontiguousarray(x[:, i * blk_n:(i + 1) * blk_n])
                while True:
                    st = a.push(blk)
                    if st == api.SGZ_OK:
                        accepted.append(i)
                        break
                    if st != api.SGZ_BUSY:
                        errors.append(("push", st)); return
        except Exception as e:                                 # noqa: BLE001
            errors.append(("push", repr(e)))
        finally:
            done.set()

    def consumer():                                            # (readers only: the peak filters would move the envelope state of A alone)
        try:
            while len(accepted) < n_blocks // 3 and not done.is_set():
                (a.state() if kind == "scope" else a.filters())
            switched[0] = len(accepted)
            a.set_mix(M2)
            switched[1] = len(accepted)
            frames = 0
            while not done.is_set() or frames < 4:
                (a.front(0) if kind == "scope" else a.vertices(0))
                frames += 1
        except Exception as e:                                 # noqa: BLE001
            errors.append(("consumer", repr(e)))

    tp, tc = threading.Thread(target=producer), threading.Thread(target=consumer)
    tc.start(); tp.start(); tp.join(timeout=300); tc.join(timeout=300)
    assert not errors and not tp.is_alive() and not tc.is_alive(), errors[:3]
    assert len(accepted) == n_blocks and accepted == list(range(n_blocks))
    # where did the switch fall?  destination 0 is source 0 under M1 and source 1 under M2
    got, _ = a.front(0) if kind == "scope" else a.history(0)    # (triggering off: the front ring is the history; it has not wrapped)
    stream = got[:total]
    k = 0
    while k < n_blocks and np.array_equal(stream[k * blk_n:(k + 1) * blk_n].view(np.uint32),
                                          _mix(M1, x[:, k * blk_n:(k + 1) * blk_n])[0].view(np.uint32)):
        k += 1
    assert switched[0] <= k <= n_blocks, (switched, k)
    b = api.Vector(**cfg) if kind == "vector" else api.Scope(**cfg)
    for i in range(n_blocks):
        blk = x[:, i * blk_n:(i + 1) * blk_n]
        _push(b, _mix(M1 if i < k else M2, blk))
    _equal(kind, a, b, cfg)
    a.close(); b.close()


def _free_device_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _rss():
    import psutil
    return psutil.Process().memory_info().rss


@pytest.mark.parametrize("kind", ["scope", "vector"])
def test_set_mix_create_destroy_gives_the_memory_back(gpu, kind):
    """create -> set_mix growing and shrinking the source count -> destroy cycles: device and host memory come back (as
    tests/test_gpu_lifecycle.py)"""
    cfg = _kind_cfg(kind, 8)

    def cycle(seed):
        h = api.Scope(**cfg) if kind == "scope" else api.Vector(**cfg)
        for S in (3, 64, 12, 1):
            h.set_mix(_matrix(seed + S, 8, S))
            blk = _sources(seed, 1024, S)
            _push(h, blk)
        h.flush()
        h.close()

    for i in range(3):
        cycle(i)
    gc.collect()
    free0, rss0 = _free_device_bytes(), _rss()
    for i in range(30):
        cycle(i)
    gc.collect()
    free1, rss1 = _free_device_bytes(), _rss()
    import os
    if "PYTEST_XDIST_WORKER" not in os.environ:
        assert free0 - free1 < 64 << 20, f"device memory: {(free0 - free1) / 2**20:.1f} MiB fewer free after 30 cycles"
    assert rss1 - rss0 < 96 << 20, f"host memory: resident set grew by {(rss1 - rss0) / 2**20:.1f} MiB over 30 cycles"
