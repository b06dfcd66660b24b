"""The pixel map, peak decay, dB scale and colour of every map form of the kernels, held to the numpy restatement of tests/fp64_map.py,
which shares no code with the oracle or the kernels.  tests/parity_chain.py's links 2 and 3 are bit-exact against the oracle, and the
oracle and the kernels were written from one reading of TransformDSP.inl; tests/test_map_fp64_host.py anchors the oracle to the
restatement, and this file anchors the kernels to it directly.  Phase mode is out of scope (fp64_map's docstring): it shows the values of
an arg-max bin and has the lazily normalised boundary Q6; tests/test_gpu_phase.py and parity_chain.py's tie rule hold it.

The map forms and the shapes that reach them (each case asserts plan.path, SGZ_PATH_SIDE_MAP included, so that a change of a plan default
fails here instead of quietly dropping coverage; tests/test_map_fp64_host.py asserts the same paths without a GPU):
  generic map                N = 32 (W = 20), 1024, 2048, and 16384 with OPT_CHANNEL_SPLIT 0
  MapPixelsBalanced, fused   N = 4096, and 32768 with OPT_CHANNEL_SPLIT 0
  halves                     N = 8192 with the per-side map kernel (the side-map bit) and without it (Complex)
  channel-split chunk scan   N = 16384, 32768 in a mono mode and in Separate / Mid-Side, one 65536 case; the image-only render of a
                             one-pair Separate plan at 32768 is the launch that takes the second channel's late pixels in K_B
  tall view, serial map      (4096, P = 2500) and (32768, P = 3000), the shapes of test_gpu_spectrum.py::test_tall_view_serial_map_fallback
Spread over those: the three interpolations, both views, zoomed views, Complex with its return to interpolation, three-pair renders, the
slope / dB-range / Blackman-Harris case, and one case that renders its frames in two calls with the decay state carried.

Per case: Plan.stage_mapped against the restated planes, Plan.render(lines=...) against the restated line results of both graphs and the
restated colour, and the image-only render (no lines: a different launch form) against the restated colour.  Every output is allocated
over NaN (test_gpu_full_size._poison_next) and its address checked: an entry a launch never writes is NaN (alpha 127 in an image), not a
stale copy of a right answer.

The bars, their derivations, the skipped pixels and their caps are those of tests/test_map_fp64_host.py's docstring, with
tol = sum|w_j| (MAP_TOL scale + WIN_ABS norm) for a mapped pixel.  Signals: that file's (synth.gen plus white noise 40 dB down, a rise
and a 40 dB drop); six frames, three at N >= 16384.
"""
import numpy as np
import pytest

from signalizer_amd import api, config

import test_map_fp64_host as host
from parity_chain import MAP_TOL, WIN_ABS
from test_map_fp64_host import CPLX, L, LANCZOS, LIN, LINEAR, LOG, MERGE, MS, NONE, R, SEP, SIDE, SLOPE_DB

pytestmark = pytest.mark.gpu

GENERIC, FUSED, HALVES, SIDE_MAP, SPLIT = 0, 1, 2, 4, 8     # SGZ_PATH_* (sgz.h)
OFF = {api.OPT_CHANNEL_SPLIT: 0}
ZOOM_LOG = dict(view_left=0.35, view_right=0.8)
ZOOM_LIN = dict(view_left=0.1, view_right=0.95)


def _c(path, W, mode, interp, view, P, opts=None, wants=(), split_at=0, **kw):
    N = max(32, 1 << (W - 1).bit_length())
    kw.setdefault("frames", 3 if N >= 16384 else 6)
    c = host.case(W, mode, interp, view, P, **kw)
    c.update(path=path, opts=opts or {}, wants=tuple(wants), split_at=split_at)
    return c


# wants: facts about the restated structure a case is there for (check_structure); split_at: render frames [0, k) and [k, F) in two calls
CASES = {
    # generic map (spectrum_generic.hip)
    "gen32_separate_lanczos_log": _c(GENERIC | SIDE_MAP, 20, SEP, LANCZOS, LOG, 16, hop=7),
    "gen32_left_linear_lin": _c(GENERIC | SIDE_MAP, 20, L, LINEAR, LIN, 24, hop=7, wants=("never_breaks",)),
    "gen32_complex_none_log": _c(GENERIC, 20, CPLX, NONE, LOG, 40, hop=7, wants=("zeros",)),
    "gen1024_left_none_log": _c(GENERIC | SIDE_MAP, 1000, L, NONE, LOG, 333),
    "gen1024_right_linear_lin": _c(GENERIC | SIDE_MAP, 1024, R, LINEAR, LIN, 333),
    "gen1024_merge_lanczos_log": _c(GENERIC | SIDE_MAP, 1000, MERGE, LANCZOS, LOG, 333),
    "gen1024_side_none_lin": _c(GENERIC | SIDE_MAP, 1024, SIDE, NONE, LIN, 700, wants=("never_breaks",)),
    "gen1024_separate_linear_log": _c(GENERIC | SIDE_MAP, 1000, SEP, LINEAR, LOG, 333),
    "gen1024_midside_lanczos_lin": _c(GENERIC | SIDE_MAP, 1024, MS, LANCZOS, LIN, 333),
    "gen1024_complex_lanczos_returns": _c(GENERIC, 1024, CPLX, LANCZOS, LOG, 1400, wants=("returns",)),
    "gen1024_complex_none_log": _c(GENERIC, 1000, CPLX, NONE, LOG, 333, wants=("zeros",)),
    "gen2048_complex_linear_zoom": _c(GENERIC, 2048, CPLX, LINEAR, LIN, 900, **ZOOM_LIN),
    "gen2048_separate_slope_db": _c(GENERIC | SIDE_MAP, 2048, SEP, LANCZOS, LOG, 500, **SLOPE_DB),
    "gen2048_midside_none_three_pairs": _c(GENERIC | SIDE_MAP, 2048, MS, NONE, LOG, 500, pairs=3),
    "gen16384_left_lanczos_log": _c(GENERIC | SIDE_MAP, 16384, L, LANCZOS, LOG, 777, opts=OFF),
    "gen16384_separate_none_lin": _c(GENERIC | SIDE_MAP, 16384, SEP, NONE, LIN, 1024, opts=OFF),
    # fused path: MapPixelsBalanced (stft_body.hpp)
    "fused4096_separate_lanczos_log": _c(FUSED, 4096, SEP, LANCZOS, LOG, 1024),
    "fused4096_left_linear_log": _c(FUSED, 4096, L, LINEAR, LOG, 777),
    "fused4096_midside_none_lin": _c(FUSED, 3000, MS, NONE, LIN, 500),
    "fused4096_complex_linear_log": _c(FUSED, 4096, CPLX, LINEAR, LOG, 777),
    "fused4096_complex_lanczos_returns": _c(FUSED, 4096, CPLX, LANCZOS, LOG, 5000, wants=("returns",)),
    "fused4096_separate_zoom_log": _c(FUSED, 4096, SEP, LANCZOS, LOG, 700, **ZOOM_LOG),
    "fused4096_midside_all_runs": _c(FUSED, 4096, MS, NONE, LOG, 120, view_left=0.6, view_right=0.95, wants=("all_runs",)),
    "fused4096_separate_slope_db_three_pairs": _c(FUSED, 4096, SEP, LINEAR, LOG, 500, pairs=3, **SLOPE_DB),
    "fused32768_separate_linear_log": _c(FUSED, 32768, SEP, LINEAR, LOG, 1024, opts=OFF),
    # halves path: the per-side map kernel (the side-map bit), and the generic map kernel behind the halves (Complex)
    "halves8192_separate_lanczos_log": _c(HALVES | SIDE_MAP, 8192, SEP, LANCZOS, LOG, 1024),
    "halves8192_left_none_log": _c(HALVES | SIDE_MAP, 5000, L, NONE, LOG, 777),
    "halves8192_midside_linear_lin": _c(HALVES | SIDE_MAP, 8192, MS, LINEAR, LIN, 500),
    "halves8192_complex_lanczos_log": _c(HALVES, 8192, CPLX, LANCZOS, LOG, 1024),
    "halves8192_complex_none_lin": _c(HALVES, 8192, CPLX, NONE, LIN, 777),
    # channel-split path (spectrum_real.hip): the chunk-scan map
    "split16384_left_lanczos_log": _c(GENERIC | SIDE_MAP | SPLIT, 16384, L, LANCZOS, LOG, 1024),
    "split16384_side_none_lin": _c(GENERIC | SIDE_MAP | SPLIT, 16384, SIDE, NONE, LIN, 777),
    "split16384_separate_lanczos_log": _c(GENERIC | SIDE_MAP | SPLIT, 16384, SEP, LANCZOS, LOG, 1024),
    "split16384_midside_linear_log": _c(GENERIC | SIDE_MAP | SPLIT, 16384, MS, LINEAR, LOG, 777),
    "split32768_merge_linear_log": _c(FUSED | SPLIT, 32768, MERGE, LINEAR, LOG, 1024),
    "split32768_right_none_zoom_log": _c(FUSED | SPLIT, 32768, R, NONE, LOG, 777, **ZOOM_LOG),
    "split32768_separate_lanczos_log": _c(FUSED | SPLIT, 32768, SEP, LANCZOS, LOG, 1024),
    "split32768_separate_two_calls": _c(FUSED | SPLIT, 32768, SEP, LANCZOS, LOG, 1024, frames=4, split_at=2),
    "split32768_midside_none_lin": _c(FUSED | SPLIT, 32768, MS, NONE, LIN, 777),
    "split32768_separate_slope_db_three_pairs": _c(FUSED | SPLIT, 32768, SEP, LANCZOS, LOG, 500, pairs=3, **SLOPE_DB),
    "split65536_separate_lanczos_log": _c(HALVES | SIDE_MAP | SPLIT, 65536, SEP, LANCZOS, LOG, 1024, sample_rate=96000.0),
    # tall views: the arg-max pieces do not fit in LDS beside csf, the serial per-pixel scan
    "tall4096_separate": _c(FUSED, 4096, SEP, LANCZOS, LOG, 2500, wants=("tall",)),
    "tall32768_separate": _c(FUSED | SPLIT, 32768, SEP, LANCZOS, LOG, 3000, wants=("tall",)),
}


def make_plan(c):
    """the case's plan with its options set, not uploaded (host tables and the path need no GPU)"""
    plan = api.Plan(c["cfg"])
    for o, v in c["opts"].items():
        plan.set_option(o, v)
    return plan


def check_structure(name, c, s):
    """the facts about the restated structure (fp64_map.Structure) a case is in the table for"""
    run = ~s.interp
    P = s.pos.size
    for want in c["wants"]:
        if want == "returns":
            assert s.complex and s.returns and s.interp[0] and s.interp[-1] and run.any(), (name, s.breaks, s.returns)
        elif want == "never_breaks":
            assert s.breaks == [P - 1] and s.interp[:P - 1].all() and s.lo[P - 1] == s.hi[P - 1], (name, s.breaks)
        elif want == "all_runs":
            assert s.breaks == [0] and run.all(), (name, s.breaks)
        elif want == "zeros":
            assert (np.floor(s.pos[s.interp].astype(np.float64) + 0.5) >= s.N).any(), name
        elif want == "tall":
            assert (s.lo[run] == s.hi[run]).sum() > 100 and ((s.hi - s.lo)[run] > 2).any(), name
        else:
            raise ValueError(want)


def _poison_next(gpu, shape):
    from test_gpu_full_size import _poison_next as poison
    return poison(gpu, shape)


def _fresh(gpu, shape, dtype):
    """an output tensor over a NaN-filled block (the same size in bytes), its landing on the block checked"""
    import torch
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    assert nbytes % 4 == 0
    poisoned = _poison_next(gpu, (nbytes // 4,))
    t = torch.empty(shape, dtype=dtype, device=gpu)
    assert t.data_ptr() == poisoned, "the output did not land on the NaN-filled block"
    return t


def _render(plan, xg, gpu, F, want_lines, state=None):
    import torch
    rgba = _fresh(gpu, (F, plan.P, 4), torch.uint8)
    lines = _fresh(gpu, (F, plan.C, 2, plan.P, 2), torch.float32) if want_lines else None
    plan.render(xg, rgba=rgba, lines=lines, state=state)
    return rgba.cpu().numpy(), lines.cpu().numpy() if want_lines else None


@pytest.mark.parametrize("name", list(CASES))
def test_map_decay_colour_against_fp64(gpu, name):
    import torch
    c = CASES[name]
    cfg = c["cfg"]
    plan = make_plan(c).upload()
    assert plan.path == c["path"], (name, plan.path, c["path"])
    W, hop, C, F, P = cfg["window_size"], cfg["hop"], cfg["num_pairs"], c["frames"], cfg["axis_points"]
    x = host.signal(c, seed=sum(map(ord, name)))
    assert plan.num_frames(x.shape[1]) == F
    ref = host.restate(cfg, plan.mapped_frequencies(), plan.slope_map(), x, [plan.colour_table(i) for i in range(C)], plan.colour_ratios())
    check_structure(name, c, ref.structure)
    xg = torch.from_numpy(x).to(gpu)
    poisoned = _poison_next(gpu, (F, C, plan.sides, P))        # (uploaded first: the output must be the next allocation)
    mapped = plan.stage_mapped(xg)
    assert mapped.data_ptr() == poisoned, (name, "the mapped planes did not land on the NaN-filled block")
    planes = mapped.cpu().numpy()
    del mapped
    k = c["split_at"]
    if k:
        state = torch.zeros((C, 2, P, 2), dtype=torch.float32, device=gpu)
        first, second = xg[:, :W + (k - 1) * hop].contiguous(), xg[:, k * hop:].contiguous()
        parts = [_render(plan, first, gpu, k, True, state), _render(plan, second, gpu, F - k, True, state)]
        rgba, lines = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    else:
        rgba, lines = _render(plan, xg, gpu, F, True)
    image_only, _ = _render(plan, xg, gpu, F, False)
    r = host.compare(cfg, ref, planes, lines, rgba, MAP_TOL, WIN_ABS)
    r2 = host.compare(cfg, ref, None, None, image_only, MAP_TOL, WIN_ABS)
    msg = f"{host.describe(name, r)}; image-only colour {r2['colour']:.3g} (path {plan.path}, {F} frames x {C} pairs)"
    print(msg)
    assert not r["problems"] and not r2["problems"], (name, r["problems"], r2["problems"])
    assert r["mapped"] <= 1, (msg, r.get("mapped_at"))
    assert r["lines"] <= 1, (msg, r.get("lines_at"))
    assert r["colour"] <= 1 and r2["colour"] <= 1, (msg, r.get("colour_at"), r2.get("colour_at"))
    assert r["lines_skipped"] <= host.SKIP_CAP and r["colour_skipped"] <= host.SKIP_CAP, msg
