"""The binding's overview methods (signalizer_amd/api.py: Plan.overview*_columns, Plan.overview*, Plan.overview*_view), each held to the C call
it wraps: the method is called, the same lib() call is made here on buffers made here, and every returned output must be the same kind of
array (numpy or torch) of the same dtype and shape holding the same bytes, None exactly where it was not asked for, in a tuple of the same
length.  Nothing here knows what a record means; the shapes, word counts and argument orders below are sgz.h's, written out.

Plans: window 64, hop 16, 5 axis points, 2 pairs, linear interpolation -- CH_SEPARATE for the peak hold, stats, pct, power and flux kinds,
CH_PHASE with three bands for cross.  Audio: seeded noise, S = 64 + 6 * 16 (7 frames), k = 3: three columns, the last a remainder.  Each form
(stage at flush and not, render host, render device, view host, view device over x0 = 1, out_columns = 2) runs with each single want_* and with
all of them; pct takes q = (0.1, 0.5), so its value planes are cut as [:, :columns].  Host forms end in the timing dict (for the renders, frames
== 7; a view's dict is held to the direct call's).  S = 63 gives None from all twelve render branches."""
import ctypes as C

import numpy as np
import pytest

from signalizer_amd import api, config

pytestmark = pytest.mark.gpu

W, HOP, P, PAIRS, BANDS = 64, 16, 5, 2, 3
FRAMES, K, COLUMNS = 7, 3, 3
S = W + (FRAMES - 1) * HOP
Q = (0.1, 0.5)
TIMING_KEYS = {"h2d_ms", "kernel_ms", "d2h_ms", "frames"}

# kind -> (C suffix, the stage call's input, carry / record cell, record words on the device (0: plain float32), record dtype on the host,
#          outputs in C order: (want keyword or None where the output is not optional, column shape, host dtype, device words, planes))
SIDES = 2
_RGBA = ("want_rgba", (P, 4), np.uint8, 0, None)
KINDS = {
    "peaks": ("", "lines", (PAIRS, P), 0, np.float32,
              [_RGBA, ("want_peaks", (PAIRS, P), np.float32, 0, None)]),
    "stats": ("_stats", "lines", (PAIRS, P), 3, api.OVERVIEW_STAT_DTYPE,
              [_RGBA, ("want_stats", (PAIRS, P), api.OVERVIEW_STAT_DTYPE, 3, None), ("want_means", (PAIRS, P), np.float32, 0, None)]),
    "pct": ("_pct", "lines", (PAIRS, P), 34, api.OVERVIEW_PCT_DTYPE,
            [_RGBA, ("want_records", (PAIRS, P), api.OVERVIEW_PCT_DTYPE, 34, None), ("want_values", (PAIRS, P), np.float32, 0, len(Q))]),
    "power": ("_power", "mapped", (PAIRS, SIDES, P), 4, api.OVERVIEW_POWER_DTYPE,
              [_RGBA, ("want_power", (PAIRS, SIDES, P), api.OVERVIEW_POWER_DTYPE, 4, None),
               ("want_levels", (PAIRS, SIDES, P), np.float32, 0, None)]),
    "cross": ("_cross", "bins", (PAIRS, BANDS), 10, api.OVERVIEW_CROSS_DTYPE, [(None, (PAIRS, BANDS), api.OVERVIEW_CROSS_DTYPE, 10, None)]),
    "flux": ("_flux", "mapped", (PAIRS, SIDES), 11, api.OVERVIEW_FLUX_DTYPE, [(None, (PAIRS, SIDES), api.OVERVIEW_FLUX_DTYPE, 11, None)]),
}
VIEWS = ("peaks", "stats", "power")
TAKES_STATE = ("peaks", "stats", "pct")


def _want_sets(kind):
    """each single want_* and all of them; the kinds with one compulsory output: the one call"""
    names = [o[0] for o in KINDS[kind][5] if o[0]]
    if not names:
        return [{}]
    return [{n: n == one for n in names} for one in names] + [{n: True for n in names}]


def _method(plan, kind, form):
    return getattr(plan, "overview" + KINDS[kind][0] + form)


def _quantiles():
    q = np.array(Q, np.float64)
    return q, q.ctypes.data_as(C.c_void_p), len(Q)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _buffers(kind, wants, columns, device):
    """caller-made outputs of the direct call, as sgz.h sizes them (never empty): numpy zeros, or torch.empty on `device`"""
    import torch
    out = []
    for want, shape, dtype, words, planes in KINDS[kind][5]:
        if want is not None and not wants[want]:
            out.append(None)
            continue
        full = (max(columns, 1), *shape) if planes is None else (planes, max(columns, 1), *shape)
        if device is None:
            out.append(np.zeros(full, dtype))
        elif words:
            out.append(torch.empty((*full, words), dtype=torch.int64, device=device))
        else:
            out.append(torch.empty(full, dtype={np.uint8: torch.uint8, np.float32: torch.float32}[dtype], device=device))
    return out


def _ptr(a):
    if a is None:
        return None
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data_as(C.c_void_p)


def _cut(kind, arrays, columns):
    return [None if a is None else a[:columns] if o[4] is None else a[:, :columns] for a, o in zip(arrays, KINDS[kind][5])]


def _same(got, want, what):
    import torch
    assert type(got) is type(want), (what, type(got), type(want))
    if want is None:
        return
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    if torch.is_tensor(want):
        assert got.device == want.device, what
        got, want = got.cpu().numpy(), want.cpu().numpy()
    assert np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes(), what


def _same_outputs(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, (*what, i))


def _timing(d, what):
    assert isinstance(d, dict) and set(d) == TIMING_KEYS, (what, d)


@pytest.fixture(scope="module")
def world(gpu):
    """the two plans, the audio on both sides and every kind's stage input, made once and left unchanged"""
    import torch
    common = dict(window_size=W, hop=HOP, axis_points=P, num_pairs=PAIRS, bin_interp=config.INTERP_LINEAR)
    separate = api.Plan(config.spectrum_config(channel_mode=config.CH_SEPARATE, **common)).upload()
    phase = api.Plan(config.spectrum_config(channel_mode=config.CH_PHASE, **common)).upload()
    assert (separate.C, separate.sides, separate.P) == (PAIRS, SIDES, P) and separate.num_frames(S) == FRAMES
    phase.set_cross_edges([1, 4, 9, 20])
    assert phase.cross_bands == BANDS
    x = (np.random.default_rng(20261021).standard_normal((2 * PAIRS, S)) * 0.25).astype(np.float32)
    d_x = torch.from_numpy(x).to(gpu)
    mapped = separate.stage_mapped(d_x)
    _, lines = separate.stage_decay_colour(mapped, want_lines=True, want_rgba=False)
    bins = phase.stage_bins(d_x)
    assert tuple(bins.shape) == (FRAMES, PAIRS, phase.N + 1, 2) and tuple(lines.shape) == (FRAMES, PAIRS, api.NUM_GRAPHS, P, 2)
    torch.cuda.synchronize()
    return {"plans": {kind: phase if kind == "cross" else separate for kind in KINDS}, "x": x, "d_x": d_x,
            "inputs": {"lines": lines, "mapped": mapped, "bins": bins}}


@pytest.mark.parametrize("flush", [True, False])
@pytest.mark.parametrize("kind", list(KINDS))
def test_stage(world, gpu, kind, flush):
    import torch
    suffix, source, cell, words, _, _ = KINDS[kind]
    plan, d_in = world["plans"][kind], world["inputs"][source]
    columns, left = (3, 0) if flush else (2, 1)
    assert api.overview_step(K, 0, FRAMES, flush) == (columns, left)

    def carry():
        return torch.zeros((*cell, words) if words else cell, dtype=torch.int64 if words else torch.float32, device=gpu)

    for wants in _want_sets(kind):
        what = (kind, "stage", flush, tuple(wants.items()))
        front = {"q": Q} if kind == "pct" else {}
        got_carry, want_carry = carry(), carry()
        got = _method(plan, kind, "_columns")(d_in, K, held=0, flush=flush, slices=0, carry=got_carry, **front, **wants)
        arrays = _buffers(kind, wants, columns, gpu)
        head = (plan.h, d_in.data_ptr(), FRAMES, K, 0, int(flush))
        if kind == "pct":
            qa, qp, nq = _quantiles()
            args = (*head, 0, qp, nq, want_carry.data_ptr())
        elif kind == "flux":
            args = (*head, 0, 0, None, want_carry.data_ptr())                    # (first_frame, slices, prev)
        else:
            args = (*head, 0, want_carry.data_ptr())
        assert getattr(api.lib(), "sgz_stage_overview" + suffix)(*args, *[_ptr(a) for a in arrays], _stream()) == api.SGZ_OK, what
        assert isinstance(got, tuple) and got[-1] == left and type(got[-1]) is type(left), what
        _same_outputs(got[:-1], _cut(kind, arrays, columns), what)
        _same(got_carry, want_carry, (*what, "carry"))


@pytest.mark.parametrize("kind", list(KINDS))
def test_render_host(world, kind):
    suffix = KINDS[kind][0]
    plan, x = world["plans"][kind], world["x"]
    ptrs = (C.c_void_p * x.shape[0])(*[x[i].ctypes.data for i in range(x.shape[0])])
    for wants in _want_sets(kind):
        what = (kind, "render host", tuple(wants.items()))
        front = {"q": Q} if kind == "pct" else {}
        got = _method(plan, kind, "")(x, K, **front, **wants)
        arrays = _buffers(kind, wants, COLUMNS, None)
        qa, qp, nq = _quantiles()
        mid = (qp, nq) if kind == "pct" else ()
        t = api.Timing()
        st = getattr(api.lib(), f"sgz_spectrogram_overview{suffix}_host")(plan.h, ptrs, x.shape[0], S, K, *mid, *[_ptr(a) for a in arrays], C.byref(t))
        assert st == api.SGZ_OK, what
        assert isinstance(got, tuple), what
        _timing(got[-1], what)
        assert got[-1]["frames"] == FRAMES == t.frames, (what, got[-1])
        _same_outputs(got[:-1], _cut(kind, arrays, COLUMNS), what)


@pytest.mark.parametrize("kind,with_state", [(kind, False) for kind in KINDS] + [(kind, True) for kind in TAKES_STATE])
def test_render_device(world, gpu, kind, with_state):
    import torch
    suffix = KINDS[kind][0]
    plan, d_x = world["plans"][kind], world["d_x"]

    def state():
        return torch.full((PAIRS, api.NUM_GRAPHS, P, 2), 0.125, dtype=torch.float32, device=gpu) if with_state else None

    for wants in _want_sets(kind):
        what = (kind, "render device", with_state, tuple(wants.items()))
        front = {"q": Q} if kind == "pct" else {}
        got_state, want_state = state(), state()
        if kind in TAKES_STATE:
            front["state"] = got_state
        got = _method(plan, kind, "")(d_x, K, **front, **wants)
        arrays = _buffers(kind, wants, COLUMNS, gpu)
        qa, qp, nq = _quantiles()
        mid = (qp, nq) if kind == "pct" else ()
        tail = (_ptr(want_state),) if kind in TAKES_STATE else ()
        st = getattr(api.lib(), f"sgz_spectrogram_overview{suffix}_device")(plan.h, d_x.data_ptr(), d_x.stride(0), S, K, *mid,
                                                                          *[_ptr(a) for a in arrays], *tail, _stream())
        assert st == api.SGZ_OK, what
        want = _cut(kind, arrays, COLUMNS)
        if kind in ("cross", "flux"):
            assert torch.is_tensor(got), (what, type(got))                   # (a bare tensor, not a 1-tuple)
            got = (got,)
        assert isinstance(got, tuple), what
        _same_outputs(got, want, what)
        _same(got_state, want_state, (*what, "state"))


@pytest.mark.parametrize("kind", VIEWS)
def test_view_host_and_device(world, gpu, kind):
    import torch
    suffix, _, cell, words, _, outputs = KINDS[kind]
    plan = world["plans"][kind]
    everything = {o[0]: True for o in outputs}
    kept = _method(plan, kind, "")(world["x"], K, **everything)[1]            # the kind's records (peaks: float32) of all three columns
    d_kept = _method(plan, kind, "")(world["d_x"], K, **everything)[1]
    assert kept.shape == (COLUMNS, *cell) and tuple(d_kept.shape) == ((COLUMNS, *cell, words) if words else (COLUMNS, *cell))
    x0, x1, out_columns, cols = 1, COLUMNS, 2, 2
    assert api.overview_view_columns(COLUMNS, x0, x1, out_columns) == cols
    for wants in _want_sets(kind):
        what = (kind, "view host", tuple(wants.items()))
        got = _method(plan, kind, "_view")(kept, out_columns, x0=x0, **wants)
        arrays = _buffers(kind, wants, cols, None)
        t = api.Timing()
        st = getattr(api.lib(), f"sgz_overview{suffix}_view_host")(plan.h, _ptr(kept), COLUMNS, x0, x1, out_columns, *[_ptr(a) for a in arrays], C.byref(t))
        assert st == api.SGZ_OK, what
        assert isinstance(got, tuple), what
        _timing(got[-1], what)
        assert got[-1]["frames"] == t.frames, (what, got[-1], t.frames)
        _same_outputs(got[:-1], _cut(kind, arrays, cols), what)

        what = (kind, "view device", tuple(wants.items()))
        got = _method(plan, kind, "_view")(d_kept, out_columns, x0=x0, slices=0, **wants)
        arrays = _buffers(kind, wants, cols, gpu)
        st = getattr(api.lib(), f"sgz_stage_overview{suffix}_view")(plan.h, d_kept.data_ptr(), COLUMNS, x0, x1, out_columns, 0,
                                                                  *[_ptr(a) for a in arrays], _stream())
        assert st == api.SGZ_OK, what
        assert isinstance(got, tuple), what
        _same_outputs(got, _cut(kind, arrays, cols), what)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", list(KINDS))
def test_fewer_samples_than_a_window_is_none_from_both_branches(world, kind):
    plan = world["plans"][kind]
    front = {"q": Q} if kind == "pct" else {}
    assert _method(plan, kind, "")(world["x"][:, :W - 1], K, **front) is None
    assert _method(plan, kind, "")(world["d_x"][:, :W - 1], K, **front) is None
