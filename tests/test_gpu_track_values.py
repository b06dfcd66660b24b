"""The tracker on value planes on the GPU (sgz_stage_track_peaks_values; csrc/tracker.hip trackValuePeaksKernel).

Every comparison is of struct bytes (uint64 views: a NaN equals a NaN when the bits agree), no tolerance anywhere:
  the stage call       record r == sgz_track_peak_values on that record's host copy (tests/test_track_lane_host.py holds the host form to
                       sgz_track_peak_lines);
  overview peaks       the peaks of Plan.overview(k = 1) tracked == Plan.track_render(graph 0) of the same planar floats;
  view peaks           the peaks of Plan.overview_view tracked on the device == the host call on the same V'.
Every output lies between two sentinel records that must stay untouched."""
import ctypes as C
import gc
import math
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_ref as ov  # noqa: E402
from test_gpu_track_render import LP, MOUSE, SENTINEL, _guarded, _line_pool, _payload, _stream  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("sgz_track_peak_values", "sgz_stage_track_peaks_values")
KINDS = {
    "fft_linear": dict(bin_interp=config.INTERP_LINEAR),
    "fft_lanczos": dict(bin_interp=config.INTERP_LANCZOS),
    "rsnt": dict(algorithm=config.ALGO_RSNT),
}


def _lib():
    L = api.lib()
    for name in NAMES:
        assert hasattr(L, name), f"libsgz.so does not export {name}"
    return L


def _host_value_peak(plan, values, mf):
    """sgz_track_peak_values on a host float [P] record, as uint64 [6]"""
    out = api.LinePeak()
    v = np.ascontiguousarray(values, np.float32)
    api.check(_lib().sgz_track_peak_values(plan.h, v.ctypes.data_as(C.c_void_p), float(mf), C.byref(out)))
    return np.frombuffer(bytes(out), np.uint64).copy()


def _host_values_track(plan, planes, mf):
    """the host call per record of planes [..., P] -> uint64 [..., 6]"""
    flat = planes.reshape(-1, planes.shape[-1])
    return np.stack([_host_value_peak(plan, v, mf) for v in flat]).reshape(planes.shape[:-1] + (LP,))


def _misaligned(gpu, values):
    """the records on the device from an address 4 bytes behind a 16-byte boundary; (the tensor that owns them, the address)"""
    import torch
    t = torch.zeros(values.size + 8, dtype=torch.float32, device=gpu)
    start = next(i for i in range(8) if (t.data_ptr() + 4 * i) % 16 == 4)
    t[start:start + values.size] = torch.from_numpy(values.reshape(-1)).to(gpu)
    return t, t.data_ptr() + 4 * start


@pytest.mark.parametrize("P", [2, 16, 17, 33, 64, 1000, 4096])
def test_stage_call_equals_the_host_function(gpu, P):
    import torch
    L = _lib()
    pool = _line_pool(P, 100 + P)
    K = len(pool)
    assert K == 20
    checked = 0
    for kind, over in KINDS.items():
        plan = api.Plan(config.spectrum_config(window_size=64, hop=16, axis_points=P, **over)).upload()
        want = {}

        def ref(k, mf):
            if (k, mf) not in want:
                want[k, mf] = _host_value_peak(plan, pool[k], mf)
            return want[k, mf]

        for shape in ((1,), (2,), (7,), (3, 5)):
            records = int(np.prod(shape))
            for base in range(0, K, records):                                # every content under every record count
                which = (base + np.arange(records)) % K
                values = np.ascontiguousarray(pool[which])
                if (base // records) % 2:
                    owner, ptr_in = _misaligned(gpu, values)
                    assert ptr_in % 16 == 4
                else:
                    owner = torch.from_numpy(values).to(gpu)
                    ptr_in = owner.data_ptr()
                for mf in MOUSE:
                    t, ptr = _guarded(gpu, records, LP)
                    api.check(L.sgz_stage_track_peaks_values(plan.h, ptr_in, records, mf, ptr, _stream()))
                    got = _payload(t, records, LP)
                    for r in range(records):
                        k = int(which[r])
                        assert (got[r] == ref(k, mf)).all(), (P, kind, shape, base, mf, k, r, got[r].view(np.float64), ref(k, mf).view(np.float64))
                        checked += 1
        # the wrapper keeps the leading shape; records == 0: nothing launched
        d = torch.from_numpy(np.ascontiguousarray(pool[:15]).reshape(3, 5, P)).to(gpu)
        out = plan.track_peaks_values(d, 0.5)
        assert tuple(out.shape) == (3, 5, LP)
        assert (out.cpu().numpy().view(np.uint64) == np.stack([ref(k, 0.5) for k in range(15)]).reshape(3, 5, LP)).all()
        t, ptr = _guarded(gpu, 1, LP)
        assert L.sgz_stage_track_peaks_values(plan.h, d.data_ptr(), 0, 0.5, ptr, _stream()) == api.SGZ_OK
        torch.cuda.synchronize()
        assert (t.cpu().numpy().view(np.uint64) == SENTINEL).all()
    assert checked >= 3 * 4 * K * len(MOUSE)


OVERVIEW_CASES = {
    "w64_p64": (dict(window_size=64, hop=16, axis_points=64, pole=(0.3, 0.3)), 23),
    "n4096_two_pairs_p257": (dict(window_size=4096, hop=1024, axis_points=257, num_pairs=2, pole=(0.5, 0.5)), 9),
    "phase": (dict(window_size=256, hop=64, axis_points=100, channel_mode=config.CH_PHASE, pole=(0.3, 0.3)), 23),
}
_made = {}


def _overview_case(name, gpu):
    """(plan, planar floats, the peaks of Plan.overview(k = 1) on the device [F][C][P]) -- once"""
    import torch
    if name not in _made:
        over, frames = OVERVIEW_CASES[name]
        cfg = config.spectrum_config(**over)
        x = ov.burst_signal(cfg["window_size"], cfg["hop"], frames, 2 * cfg["num_pairs"], cfg["sample_rate"], seed=11)
        plan = api.Plan(cfg).upload()
        assert plan.num_frames(x.shape[1]) == frames
        _, peaks = plan.overview(torch.from_numpy(x).to(gpu), 1, want_rgba=False, want_peaks=True)
        torch.cuda.synchronize()
        assert tuple(peaks.shape) == (frames, plan.C, plan.P)
        _made[name] = (plan, x, peaks)
    return _made[name]


@pytest.mark.parametrize("name", list(OVERVIEW_CASES))
def test_overview_peaks_tracked_equal_the_track_render(gpu, name):
    _lib()
    plan, x, peaks = _overview_case(name, gpu)
    for mf in MOUSE:
        want, _, _ = plan.track_render(x, 0, mf, want_rgba=False)
        got = plan.track_peaks_values(peaks, mf).cpu().numpy()
        assert got.shape == want.shape and (got.view(np.uint64) == want.view(np.uint64)).all(), (name, mf)


@pytest.mark.parametrize("name", list(OVERVIEW_CASES))
def test_view_peaks_tracked_equal_the_host_call(gpu, name):
    """V' of overview_view at g = 3 source columns per output column (the last one narrower where the count does not divide)"""
    _lib()
    plan, x, peaks = _overview_case(name, gpu)
    n = peaks.shape[0]
    for x0, x1 in ((0, n), (2, n - 1)):
        cols = -(-(x1 - x0) // 3)
        _, view = plan.overview_view(peaks, cols, x0, x1, want_rgba=False, want_peaks=True)
        assert tuple(view.shape) == (cols, plan.C, plan.P)
        host = view.cpu().numpy()
        for mf in MOUSE:
            got = plan.track_peaks_values(view, mf).cpu().numpy().view(np.uint64)
            assert (got == _host_values_track(plan, host, mf)).all(), (name, x0, x1, mf)


def test_refusals_launch_nothing(gpu):
    import torch
    L = _lib()
    plan = api.Plan(config.spectrum_config(window_size=64, hop=16, axis_points=33)).upload()
    d = torch.ones((3, 33), dtype=torch.float32, device=gpu)
    t, ptr = _guarded(gpu, 3, LP)
    E = api.SGZ_EINVAL
    assert L.sgz_stage_track_peaks_values(None, d.data_ptr(), 3, 0.5, ptr, _stream()) == E
    assert L.sgz_stage_track_peaks_values(plan.h, None, 3, 0.5, ptr, _stream()) == E
    assert L.sgz_stage_track_peaks_values(plan.h, d.data_ptr(), 3, 0.5, None, _stream()) == E
    for mf in (math.nan, math.inf, -math.inf):
        assert L.sgz_stage_track_peaks_values(plan.h, d.data_ptr(), 3, mf, ptr, _stream()) == E
    assert L.sgz_stage_track_peaks_values(plan.h, d.data_ptr(), 0, 0.5, ptr, _stream()) == api.SGZ_OK
    torch.cuda.synchronize()
    assert (t.cpu().numpy().view(np.uint64) == SENTINEL).all()


def test_values_track_is_the_same_beside_a_background_render(gpu):
    """another plan's renders in flight on a second stream while the call runs on the current one"""
    import torch
    _lib()
    plan, x, peaks = _overview_case("n4096_two_pairs_p257", gpu)
    plan_l = api.Plan(config.spectrum_config(window_size=64, hop=16, axis_points=4096)).upload()
    silence = torch.zeros((7, 4096), dtype=torch.float32, device=gpu)               # the walk runs the whole axis
    want = plan.track_peaks_values(peaks, 0.37).cpu().numpy().view(np.uint64)
    want_l = plan_l.track_peaks_values(silence, 0.5).cpu().numpy().view(np.uint64)
    cfg = config.spectrum_config(window_size=4096, hop=1024, channel_mode=config.CH_COMPLEX)
    load = api.Plan(cfg).upload()
    y = torch.from_numpy(ov.burst_signal(4096, 1024, 300, 2, cfg["sample_rate"], seed=5)).to(gpu)
    side = torch.cuda.Stream(device=gpu)
    image = load.render(y, stream=side.cuda_stream)
    side.synchronize()
    first = image.clone()
    for _ in range(20):
        for _ in range(8):
            load.render(y, rgba=image, stream=side.cuda_stream)
        got = plan.track_peaks_values(peaks, 0.37).cpu().numpy().view(np.uint64)
        got_l = plan_l.track_peaks_values(silence, 0.5).cpu().numpy().view(np.uint64)
        assert (got == want).all() and (got_l == want_l).all()
    side.synchronize()
    assert torch.equal(image, first)


def test_a_hundred_calls_do_not_grow_device_memory(gpu):
    import torch
    _lib()
    plan, x, peaks = _overview_case("w64_p64", gpu)
    out = torch.empty((peaks.shape[0], plan.C, LP), dtype=torch.float64, device=gpu)

    def calls(n):
        for i in range(n):
            plan.track_peaks_values(peaks, MOUSE[i % len(MOUSE)], out=out)
        gc.collect(); torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    free0 = calls(4)
    free1 = calls(100)
    assert free0 - free1 < 2 << 20, f"device memory: {(free0 - free1) / 2**20:.1f} MiB fewer free after 100 calls"
