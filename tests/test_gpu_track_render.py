"""The batched frequency tracker on the GPU (csrc/tracker.hip trackLinePeaksKernel / trackPeaksKernel, sgz_spectrogram_track_device / _host).

Every comparison is of struct bytes (uint64 views: a NaN equals a NaN when the bits agree), and there is no tolerance anywhere:
  lines stage call   record (f, p) == sgz_track_peak_lines on that record's host copy -- the host function is the definition;
  bins stage call    record r == sgz_stage_track_peak on d_bins + r (N + 1) -- the single-frame kernel is the definition;
  the render         track == sgz_spectrogram_render_host(..., lines_out) followed by sgz_track_peak_lines per (frame, pair), and the image ==
                     that render's image.
Every output lies between two sentinel records that must stay untouched."""
import ctypes as C
import math

import numpy as np
import pytest

from signalizer_amd import api, config, synth

pytestmark = pytest.mark.gpu

MOUSE = (-1.0, 0.0, 0.02, 0.03, 0.5, 0.97, 1.0, 2.0)
GENERIC, FUSED, HALVES, SIDE_MAP, SPLIT = 0, 1, 2, 4, 8      # SGZ_PATH_* (sgz.h)
LP, PK = len(api.LinePeak._fields_), len(api.Peak._fields_)  # doubles per record
SENTINEL = 0x5A5AA5A5C3C33C3C
G = api.NUM_GRAPHS


def _llround(x):
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _guarded(gpu, records, width):
    """a device block of records + 2 sentinel records; (whole uint64 tensor, pointer to record 0)"""
    import torch
    t = torch.full(((records + 2) * width,), SENTINEL, dtype=torch.int64, device=gpu)
    return t, t.data_ptr() + width * 8


def _payload(t, records, width):
    """the records between the sentinels as uint64 [records][width], after checking the sentinels"""
    h = t.cpu().numpy().view(np.uint64).reshape(records + 2, width)
    assert (h[0] == SENTINEL).all() and (h[-1] == SENTINEL).all(), "a sentinel record was written"
    return h[1:-1]


def _host_line_peak(plan, record, mf):
    """sgz_track_peak_lines on a host float2 [P] record, as uint64 [6]"""
    out = api.LinePeak()
    r = np.ascontiguousarray(record, np.float32)
    api.check(api.lib().sgz_track_peak_lines(plan.h, r.ctypes.data_as(C.c_void_p), float(mf), C.byref(out)))
    return np.frombuffer(bytes(out), np.uint64).copy()


def _host_track(plan, lines, graph, mf):
    """the parent's way to a track: the host loop over line results [F][C][G][P][2]"""
    F, Cn = lines.shape[:2]
    return np.stack([np.stack([_host_line_peak(plan, lines[f, p, graph], mf) for p in range(Cn)]) for f in range(F)])


# ---- lines stage call ----------------------------------------------------------------------------------------------------------------
def _line_pool(P, seed):
    """left magnitudes [K][P] float32: every content the walks and the search can go wrong on; the range bounds used to place features are
    those of mouse_fraction 0.5"""
    rng = np.random.default_rng(seed)
    pivot, rg = _llround(P * 0.5), _llround(P * 0.03)
    lb, hb = max(pivot - rg, 0), min(pivot + rg, P)
    nan = np.float32(np.nan)
    pool = []

    def add(v):
        pool.append(np.asarray(v, np.float32).copy())

    rnd = [rng.standard_normal(P).astype(np.float32) for _ in range(4)]
    add(rnd[0]); add(rnd[1])
    add(np.arange(P))                                            # strictly rising: the upward walk runs to the last point
    add(-np.arange(P, dtype=np.float32))                         # strictly falling: the downward walk stops at index 1
    add(np.full(P, 0.25)); add(np.zeros(P))                      # ties: the first largest, and both walks to the end of the axis
    v = np.zeros(P); v[max(lb - 3, 0):min(lb + 4, P)] = 1; add(v)     # plateaus that straddle either boundary of the range
    v = np.zeros(P); v[max(hb - 4, 0):min(hb + 3, P)] = 1; add(v)
    v = rnd[2].copy(); v[min(lb, P - 1)] = nan; add(v)           # NaN on either boundary
    v = rnd[2].copy(); v[max(hb - 1, 0)] = nan; add(v)
    v = rnd[3].copy(); v[min(lb + int(np.argmax(v[lb:hb])) if hb > lb else lb, P - 1)] = nan; add(v)       # NaN at the peak
    add(np.full(P, np.uint32(0xffc12345)).view(np.float32))      # NaN in every entry (sign and payload set)
    v = np.arange(P, dtype=np.float32); v[::5] = nan; add(v)     # NaNs along a rising edge: they never stop a walk
    v = -np.arange(P, dtype=np.float32); v[1::3] = nan; add(v)
    v = rnd[0].copy(); v[min(pivot, P - 1)] = np.inf; add(v)     # +-inf
    add(np.full(P, -np.inf)); add(np.full(P, np.inf))
    v = rnd[1].copy(); v[:max(lb, 1)] = -np.inf; v[min(hb, P - 1):] = np.inf; add(v)
    v = np.zeros(P, np.float32); v[::2] = -0.0; add(v)           # -0 against +0: equal, the first stays
    v = np.zeros(P, np.float32); v[1::2] = -0.0; add(v)
    return np.stack(pool)


@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("P", [2, 16, 17, 33, 64, 1000, 4096])
def test_lines_stage_call_equals_the_host_function(gpu, P, pairs):
    import torch
    plan = api.Plan(config.spectrum_config(window_size=64, hop=16, axis_points=P, num_pairs=pairs, bin_interp=config.INTERP_LINEAR)).upload()
    pool = _line_pool(P, 100 + P)
    K = len(pool)
    rng = np.random.default_rng(P)
    want = {}

    def ref(k, mf):
        if (k, mf) not in want:
            rec = np.stack([pool[k], np.zeros(P, np.float32)], axis=1)       # (the right halves are never looked at)
            want[(k, mf)] = _host_line_peak(plan, rec, mf)
        return want[(k, mf)]

    L = api.lib()
    checked = 0
    for frames in (1, 2, 7):
        slots = frames * pairs * G
        for shift in (0, 1):                                                  # every content under either graph
            for base in range(shift, K + shift, slots):
                which = (base + np.arange(slots)) % K
                lines = np.empty((frames, pairs, G, P, 2), np.float32)
                lines[..., 0] = pool[which].reshape(frames, pairs, G, P)
                lines[..., 1] = rng.standard_normal((frames, pairs, G, P)).astype(np.float32)
                d_lines = torch.from_numpy(lines).to(gpu)
                for graph in range(G):
                    for mf in MOUSE:
                        t, ptr = _guarded(gpu, frames * pairs, LP)
                        api.check(L.sgz_stage_track_peaks_lines(plan.h, d_lines.data_ptr(), frames, graph, mf, ptr, _stream()))
                        got = _payload(t, frames * pairs, LP)
                        for r in range(frames * pairs):
                            k = int(which[r * G + graph])
                            assert (got[r] == ref(k, mf)).all(), (P, pairs, frames, graph, mf, k, r, got[r].view(np.float64), ref(k, mf).view(np.float64))
                            checked += 1
    assert checked >= 2 * K * G * len(MOUSE)
    # the wrapper, and frames == 0: nothing launched
    out = plan.track_peaks_lines(d_lines, 1, 0.5).cpu().numpy().view(np.uint64)
    assert (out.reshape(-1, LP)[0] == ref(int(which[1]), 0.5)).all()
    t, ptr = _guarded(gpu, 1, LP)
    assert L.sgz_stage_track_peaks_lines(plan.h, d_lines.data_ptr(), 0, 0, 0.5, ptr, _stream()) == api.SGZ_OK
    assert (t.cpu().numpy().view(np.uint64) == SENTINEL).all()


# ---- bins stage call -----------------------------------------------------------------------------------------------------------------
BINS_CASES = {
    "w32": dict(cfg=dict(window_size=32, hop=8, axis_points=16), frames=5, path=GENERIC),
    "w1000_padded": dict(cfg=dict(window_size=1000, hop=250), frames=4, path=GENERIC),
    "n4096_two_pairs": dict(cfg=dict(window_size=4096, hop=1024, num_pairs=2), frames=4, path=FUSED),
    "n32768_split_separate": dict(cfg=dict(window_size=32768, hop=8192), frames=3, path=FUSED | SPLIT),
    "n32768_split_left": dict(cfg=dict(window_size=32768, hop=8192, channel_mode=config.CH_LEFT), frames=3, path=FUSED | SPLIT),
}


def _bin_bounds(plan, cfg, mf):
    """the raw-FFT branch's search range (SpectrumRendering.cpp:383-392), only to PLACE features in hand-made records"""
    mapped, P, N, sr = plan.mapped_frequencies(), plan.P, plan.N, cfg["sample_rate"]
    out = []
    for d in (-0.03, 0.03):
        i = min(max(_llround(P * (mf + d)), 0), P - 1)
        out.append(min(max(_llround(float(np.float32(N) * mapped[i]) / sr), 0), N))
    return out


def _hand_made_bins(plan, cfg, seed):
    N = plan.N
    rng = np.random.default_rng(seed)
    lower, higher = _bin_bounds(plan, cfg, 0.5)
    recs = [np.zeros(N + 1, np.float32)]                                     # silence: non-normal fits, the walk down to bin 1
    v = np.zeros(N + 1, np.float32); v[max(higher - 1, 0):] = 1; recs.append(v)        # a plateau from higher - 1 on: the walk up to N
    v = np.zeros(N + 1, np.float32); v[:lower + 1] = 1; recs.append(v)                 # ... and up to lower: the walk down to bin 1
    v = np.zeros(N + 1, np.float32); v[max(lower - 2, 0):lower + 3] = 2; recs.append(v)   # a plateau that straddles the lower bound
    recs.append(np.arange(N + 1, 0, -1).astype(np.float32))                  # falling: the peak on the lower bound, rising to the left
    recs.append(np.full(N + 1, np.nan, np.float32))                          # NaN bins: everywhere, and scattered
    v = rng.random(N + 1).astype(np.float32); v[::3] = np.nan; recs.append(v)
    v = rng.random(N + 1).astype(np.float32) * 0.1; v[0] = 5; recs.append(v)           # a peak at bin 0 and at bin N
    v = rng.random(N + 1).astype(np.float32) * 0.1; v[N] = 5; recs.append(v)
    v = -rng.random(N + 1).astype(np.float32); v[max(higher - 1, 0)] = -3; recs.append(v)   # signed entries: the square decides
    return np.stack(recs)


@pytest.mark.parametrize("name", list(BINS_CASES))
def test_bins_stage_call_equals_the_single_frame_call(gpu, name):
    import torch
    case = BINS_CASES[name]
    cfg = config.spectrum_config(**case["cfg"])
    plan = api.Plan(cfg).upload()
    assert plan.path & ~SIDE_MAP == case["path"], (name, plan.path)
    N, Cn, frames = plan.N, plan.C, case["frames"]
    S = cfg["window_size"] + cfg["hop"] * (frames - 1)
    x = torch.from_numpy(synth.gen(40 + len(name), int(cfg["sample_rate"]), S, 2 * Cn)).to(gpu)
    hand = torch.from_numpy(_hand_made_bins(plan, cfg, N)).to(gpu)
    staged = frames * Cn
    records = staged + hand.shape[0]
    bins = torch.zeros((records, N + 1), dtype=torch.float32, device=gpu)    # (the channel-split mono form leaves csf[N/2 + 1 .. N] alone)
    L = api.lib()
    api.check(L.sgz_stage_bins(plan.h, x.data_ptr(), x.stride(0), S, bins.data_ptr(), _stream()))
    bins[staged:] = hand
    torch.cuda.synchronize()
    for mf in MOUSE + ((0.9,) if N == 32768 else ()):
        t, ptr = _guarded(gpu, records, PK)
        api.check(L.sgz_stage_track_peaks(plan.h, bins.data_ptr(), records, mf, ptr, _stream()))
        got = _payload(t, records, PK)
        for r in range(records):
            one = api.Peak()
            api.check(L.sgz_stage_track_peak(plan.h, bins.data_ptr() + r * (N + 1) * 4, mf, C.byref(one), _stream()))
            want = np.frombuffer(bytes(one), np.uint64)
            assert (got[r] == want).all(), (name, mf, r, got[r].view(np.float64), want.view(np.float64))
    assert (plan.track_peaks(bins, mf).cpu().numpy().view(np.uint64) == got).all()          # the wrapper, at the last position


@pytest.mark.parametrize("mode", [config.CH_PHASE, config.CH_COMPLEX])
def test_bins_stage_call_refuses_phase_and_complex_and_writes_nothing(gpu, mode):
    import torch
    plan = api.Plan(config.spectrum_config(window_size=1024, hop=256, channel_mode=mode)).upload()
    bins = torch.ones((3, (plan.N + 1) * 2), dtype=torch.float32, device=gpu)
    t, ptr = _guarded(gpu, 3, PK)
    assert api.lib().sgz_stage_track_peaks(plan.h, bins.data_ptr(), 3, 0.5, ptr, _stream()) == api.SGZ_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (t.cpu().numpy().view(np.uint64) == SENTINEL).all()


def test_bins_stage_call_with_no_records_launches_nothing(gpu):
    import torch
    plan = api.Plan(config.spectrum_config(window_size=1024, hop=256)).upload()
    bins = torch.ones((1, plan.N + 1), dtype=torch.float32, device=gpu)
    t, ptr = _guarded(gpu, 1, PK)
    assert api.lib().sgz_stage_track_peaks(plan.h, bins.data_ptr(), 0, 0.5, ptr, _stream()) == api.SGZ_OK
    torch.cuda.synchronize()
    assert (t.cpu().numpy().view(np.uint64) == SENTINEL).all()


# ---- the render ----------------------------------------------------------------------------------------------------------------------
RENDER_CASES = {
    "n1024_separate": dict(cfg=dict(window_size=1024, hop=256), frames=9),                      # one pair, two chunks: the one-launch K_B
    "phase_generic": dict(cfg=dict(window_size=2048, hop=512, channel_mode=config.CH_PHASE), frames=6),
    "complex": dict(cfg=dict(window_size=4096, hop=1024, channel_mode=config.CH_COMPLEX), frames=5),
    "n32768_split": dict(cfg=dict(window_size=32768, hop=8192), frames=5, path=FUSED | SPLIT),
    "two_pairs": dict(cfg=dict(window_size=4096, hop=1024, num_pairs=2), frames=7),
    "rsnt_small": dict(cfg=dict(algorithm=config.ALGO_RSNT, window_size=1024, hop=256, axis_points=128), frames=8),
}
RENDER_MOUSE = (0.0, 0.37, 0.97)
_render_refs = {}


def _render_case(name):
    """(plan, planar, the parent's render: image and line results) -- rendered once per case and shared"""
    if name not in _render_refs:
        case = RENDER_CASES[name]
        cfg = config.spectrum_config(**case["cfg"])
        plan = api.Plan(cfg).upload()
        if "path" in case:
            assert plan.path & ~SIDE_MAP == case["path"], (name, plan.path)
        frames = case["frames"]
        S = cfg["hop"] * frames if cfg["algorithm"] == config.ALGO_RSNT else cfg["window_size"] + cfg["hop"] * (frames - 1)
        x = synth.gen(60 + len(name), int(cfg["sample_rate"]), S, 2 * cfg["num_pairs"])
        assert plan.num_frames(S) == frames
        rgba, lines, _ = api.render_spectrogram_host(plan, x, want_lines=True)
        _render_refs[name] = (plan, x, rgba, lines)
    return _render_refs[name]


@pytest.mark.parametrize("name", list(RENDER_CASES))
def test_track_render_equals_render_then_host_loop(gpu, name):
    plan, x, rgba, lines = _render_case(name)
    for graph in range(G):
        for mf in RENDER_MOUSE:
            want = _host_track(plan, lines, graph, mf)
            track, image, timing = plan.track_render(x, graph, mf)
            assert (track.view(np.uint64) == want).all(), (name, graph, mf)
            assert image.tobytes() == rgba.tobytes(), (name, graph, mf)
            assert timing["frames"] == lines.shape[0]
            track_only, none, _ = plan.track_render(x, graph, mf, want_rgba=False)
            assert none is None and (track_only.view(np.uint64) == want).all(), (name, graph, mf)


@pytest.mark.parametrize("name", ["n1024_separate", "two_pairs", "complex"])
def test_track_device_in_two_halves_with_carried_state_equals_the_whole(gpu, name):
    """FFT plans: frames [0, h) then [h, F) with d_state carried == all F frames, track and image -- what a chunked stream relies on"""
    import torch
    plan, x, rgba, lines = _render_case(name)
    cfg, F = plan.cfg, lines.shape[0]
    h = F // 2
    W, hop = cfg.window_size, cfg.hop
    d_x = torch.from_numpy(x).to(gpu)
    want = _host_track(plan, lines, 1, 0.37)
    state = torch.zeros((plan.C, G, plan.P, 2), dtype=torch.float32, device=gpu)
    whole_track, whole_image = plan.track_render(d_x, 1, 0.37, state=state)
    assert (whole_track.cpu().numpy().view(np.uint64) == want).all() and whole_image.cpu().numpy().tobytes() == rgba.tobytes()
    state.zero_()
    a_track, a_image = plan.track_render(d_x[:, :W + hop * (h - 1)].contiguous(), 1, 0.37, state=state)
    b_track, b_image = plan.track_render(d_x[:, hop * h:].contiguous(), 1, 0.37, state=state)
    got = torch.cat([a_track, b_track]).cpu().numpy().view(np.uint64)
    assert got.shape == want.shape and (got == want).all()
    assert torch.cat([a_image, b_image]).cpu().numpy().tobytes() == rgba.tobytes()


def test_fewer_samples_than_a_window_are_skipped_and_nothing_is_written(gpu):
    import torch
    plan, x, _, _ = _render_case("n1024_separate")
    L = api.lib()
    S = plan.cfg.window_size - 1
    d_x = torch.from_numpy(x[:, :S].copy()).to(gpu)
    t, ptr = _guarded(gpu, 1, LP)
    img = torch.full((plan.P * 4,), 0x5A, dtype=torch.uint8, device=gpu)
    assert L.sgz_spectrogram_track_device(plan.h, d_x.data_ptr(), d_x.stride(0), S, 0, 0.5, img.data_ptr(), None, ptr, _stream()) == api.SGZ_SKIPPED_FRAME
    torch.cuda.synchronize()
    assert (t.cpu().numpy().view(np.uint64) == SENTINEL).all() and (img.cpu().numpy() == 0x5A).all()
    xs = np.ascontiguousarray(x[:, :S])
    track = np.full((3, LP), SENTINEL, np.uint64)
    image = np.full(plan.P * 4, 0x5A, np.uint8)
    ptrs = (C.c_void_p * 2)(xs[0].ctypes.data, xs[1].ctypes.data)
    st = L.sgz_spectrogram_track_host(plan.h, ptrs, 2, S, 0, 0.5, image.ctypes.data_as(C.c_void_p), track[1:].ctypes.data_as(C.c_void_p), None)
    assert st == api.SGZ_SKIPPED_FRAME and (track == SENTINEL).all() and (image == 0x5A).all()
    assert plan.track_render(xs, 0, 0.5) is None and plan.track_render(d_x, 0, 0.5) is None


def test_track_is_the_same_beside_a_background_render(gpu):
    """the pattern of tests/test_gpu_concurrency.py: two threads keep the device busy with renders on streams of their own"""
    import torch
    from test_gpu_concurrency import BackgroundLoad
    quiet = {}
    for name in ("n32768_split", "rsnt_small", "two_pairs"):
        plan, x, rgba, lines = _render_case(name)
        quiet[name] = _host_track(plan, lines, 0, 0.37)
    plan_l = api.Plan(config.spectrum_config(window_size=64, hop=16, axis_points=4096)).upload()
    d_lines = torch.from_numpy(np.zeros((7, 1, G, 4096, 2), np.float32)).to(gpu)          # silence: the walk runs the whole axis
    want_l = plan_l.track_peaks_lines(d_lines, 0, 0.5).cpu().numpy().view(np.uint64)
    with BackgroundLoad(gpu) as load:
        beside = 0
        for _ in range(400):                                     # (the load's threads build their plans first: go on until three rounds ran beside it)
            busy = load.renders > 0
            for name, want in quiet.items():
                plan, x, rgba, _ = _render_case(name)
                track, image, _ = plan.track_render(x, 0, 0.37)
                assert (track.view(np.uint64) == want).all() and image.tobytes() == rgba.tobytes(), name
            assert (plan_l.track_peaks_lines(d_lines, 0, 0.5).cpu().numpy().view(np.uint64) == want_l).all()
            beside += busy
            if beside >= 3 or load.errors:
                break
        assert beside >= 3, (beside, load.errors)


def test_a_hundred_track_calls_do_not_grow_device_memory(gpu):
    import gc

    import torch
    plan, x, _, _ = _render_case("two_pairs")
    d_x = torch.from_numpy(x).to(gpu)

    def calls(n):
        for i in range(n):
            if i % 2:
                plan.track_render(x, i % G, 0.37, want_rgba=bool(i % 4 == 1))
            else:
                out = plan.track_render(d_x, i % G, 0.37)
                del out
        gc.collect(); torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    free0 = calls(4)
    free1 = calls(100)
    assert free0 - free1 < 2 << 20, f"device memory: {(free0 - free1) / 2**20:.1f} MiB fewer free after 100 track calls"
