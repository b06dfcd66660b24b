"""The power overview's render on the GPU (sgz_spectrogram_overview_power_device / _host; csrc/api.hip runOverviewPowerSlabs): the records
equal the restatement (tests/overview_power_ref.py) applied to Plan.stage_mapped of the same audio, byte for byte, on every K_A path -- the
generic small plan, one side, MidSide, two pairs, the halves path and the channel-split pair path, where the late pixels decide: the render
must complete them as sgz_stage_mapped does, since no K_B runs behind it.  Levels are held to the host helper, the image to the oracle's
blend at side 0's levels (both held to K_B's own arithmetic in tests/test_gpu_overview_power.py).  The bytes do not depend on the slab."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api, config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overview_ref as ov  # noqa: E402
import overview_power_ref as opr  # noqa: E402
from test_gpu_overview import BYTE, WORD, Guarded, _stream  # noqa: E402

pytestmark = pytest.mark.gpu

RW = 8
HALVES, SPLIT = 2, 8                                         # SGZ_PATH_* (sgz.h)
CASES = {
    "w64_separate": dict(cfg=dict(window_size=64, hop=16, axis_points=33), frames=23),
    "w64_left": dict(cfg=dict(window_size=64, hop=16, axis_points=33, channel_mode=config.CH_LEFT), frames=23),
    "w64_midside": dict(cfg=dict(window_size=64, hop=16, axis_points=33, channel_mode=config.CH_MIDSIDE), frames=23),
    "w256_two_pairs": dict(cfg=dict(window_size=256, hop=64, axis_points=100, num_pairs=2), frames=23),
    "n8192_halves": dict(cfg=dict(window_size=8192, hop=2048, axis_points=200), frames=7, path=HALVES, mask=3),
    "n32768_split": dict(cfg=dict(window_size=32768, hop=8192), frames=6, path=SPLIT, mask=SPLIT),
}
SLABS = (0, 1, 3)
_refs = {}


def _case(name, gpu):
    """(plan, oracle params, planar, its device copy, Plan.stage_mapped of it [F][C][sides][P], the one-frame records) -- made once"""
    if name not in _refs:
        import torch
        from oracle import pyoracle as po
        case = CASES[name]
        cfg = config.spectrum_config(**case["cfg"])
        plan = api.Plan(cfg).upload()
        if "path" in case:
            assert plan.path & case["mask"] == case["path"], (name, plan.path)
        x = ov.burst_signal(cfg["window_size"], cfg["hop"], case["frames"], 2 * cfg["num_pairs"], cfg["sample_rate"], seed=5)
        assert plan.num_frames(x.shape[1]) == case["frames"]
        d_x = torch.from_numpy(x).to(gpu)
        mapped = plan.stage_mapped(d_x).cpu().numpy()
        _refs[name] = (plan, po.params_from_dict(cfg), x, d_x, mapped, opr.records_of(mapped))
    return _refs[name]


@pytest.mark.parametrize("name", list(CASES))
def test_power_render_equals_stage_mapped_then_restatement(gpu, name):
    from oracle import pyoracle as po
    plan, params, x, d_x, mapped, each = _case(name, gpu)
    F = mapped.shape[0]
    assert not np.isnan(mapped).any() and (mapped > 0).any()
    for k in sorted({1, 2, 5, F, F + 3}):
        want = opr.columns_of(mapped, k, each=each)[0]
        want_lv = plan.overview_power_levels(want).view(np.uint32)
        image = ov.blend(po, params, np.ascontiguousarray(want_lv[:, :, 0, :]))
        for slab in SLABS:
            plan.set_option(api.OPT_OVERVIEW_SLAB, slab)
            got_image, got, got_lv = plan.overview_power(d_x, k, want_power=True, want_levels=True)
            assert opr.same(api.power_from_device(got), want), (name, k, slab)
            assert np.array_equal(got_lv.cpu().numpy().view(np.uint32), want_lv), (name, k, slab)
            assert np.array_equal(got_image.cpu().numpy(), image), (name, k, slab)
        h_image, h_power, h_lv, timing = plan.overview_power(x, k, want_power=True, want_levels=True)      # (the last slab setting: 3)
        assert opr.same(h_power, want) and np.array_equal(h_lv.view(np.uint32), want_lv) and np.array_equal(h_image, image), (name, k)
        assert timing["frames"] == F
    plan.set_option(api.OPT_OVERVIEW_SLAB, 0)
    # stage_mapped is unchanged by the renders in between (they use the plan's scratch, never the caller's buffers)
    import torch
    assert np.array_equal(plan.stage_mapped(d_x).cpu().numpy().view(np.uint32), mapped.view(np.uint32))
    torch.cuda.synchronize()


def test_k1_rms_is_the_mapped_magnitude(gpu):
    """k == 1: lo == hi == x, and rms == |x| bit for bit wherever 2^-7 <= |x| < 4"""
    plan, params, x, d_x, mapped, each = _case("w256_two_pairs", gpu)
    _, power, _, _ = plan.overview_power(x, 1, want_rgba=False, want_power=True)
    assert opr.same(power, each)
    assert np.array_equal(power["lo"].view(np.uint32), mapped.view(np.uint32)) and np.array_equal(power["hi"].view(np.uint32), mapped.view(np.uint32))
    _, rms, _, _ = api.overview_power_readout(power)
    inside = (np.abs(mapped) >= 2.0 ** -7) & (np.abs(mapped) < 4.0)
    assert inside.any() and np.array_equal(rms[inside].view(np.uint32), np.abs(mapped[inside]).view(np.uint32))


def test_one_output_alone_and_short_input(gpu):
    import torch
    from oracle import pyoracle as po
    plan, params, x, d_x, mapped, each = _case("w256_two_pairs", gpu)
    L = api.lib()
    k = 5
    want = opr.columns_of(mapped, k, each=each)[0]
    want_lv = plan.overview_power_levels(want).view(np.uint32)
    image = ov.blend(po, params, np.ascontiguousarray(want_lv[:, :, 0, :]))
    columns, P, width = want.shape[0], plan.P, plan.C * plan.sides * plan.P
    S = x.shape[1]
    ptrs = (C.c_void_p * 4)(*[x[i].ctypes.data for i in range(4)])
    for only in range(3):
        img = Guarded(gpu, columns, P * 4, torch.uint8)
        pw = Guarded(gpu, columns, width * RW, torch.int32)
        lv = Guarded(gpu, columns, width, torch.int32)
        st = L.sgz_spectrogram_overview_power_device(plan.h, d_x.data_ptr(), d_x.stride(0), S, k, img.ptr if only == 0 else None,
                                                     pw.ptr if only == 1 else None, lv.ptr if only == 2 else None, _stream())
        assert st == api.SGZ_OK
        assert np.array_equal(img.payload().reshape(columns, P, 4), image) if only == 0 else img.untouched()
        assert opr.same(np.ascontiguousarray(pw.payload()).reshape(columns, width, RW).view(opr.DTYPE).reshape(want.shape), want) if only == 1 else pw.untouched()
        assert np.array_equal(lv.payload().reshape(want.shape), want_lv) if only == 2 else lv.untouched()
        h_img = np.full((columns + 2, P, 4), BYTE, np.uint8)
        h_pw = np.full((columns + 2, width, RW), WORD, np.uint32)
        h_lv = np.full((columns + 2, width), WORD, np.uint32)
        st = L.sgz_spectrogram_overview_power_host(plan.h, ptrs, 4, S, k, h_img[1:].ctypes.data_as(C.c_void_p) if only == 0 else None,
                                                   h_pw[1:].ctypes.data_as(C.c_void_p) if only == 1 else None,
                                                   h_lv[1:].ctypes.data_as(C.c_void_p) if only == 2 else None, None)
        assert st == api.SGZ_OK
        for h, s in ((h_img, BYTE), (h_pw, WORD), (h_lv, WORD)):
            assert (h[0] == s).all() and (h[-1] == s).all()
        assert np.array_equal(h_img[1:-1], image) if only == 0 else (h_img == BYTE).all()
        assert np.array_equal(h_pw[1:-1], np.ascontiguousarray(want).view(np.uint32).reshape(columns, width, RW)) if only == 1 else (h_pw == WORD).all()
        assert np.array_equal(h_lv[1:-1], want_lv.reshape(columns, width)) if only == 2 else (h_lv == WORD).all()
    # fewer samples than a window: skipped, nothing written
    S = plan.cfg.window_size - 1
    xs = np.ascontiguousarray(x[:, :S])
    d_xs = torch.from_numpy(xs).to(gpu)
    img = Guarded(gpu, 1, P * 4, torch.uint8)
    pw = Guarded(gpu, 1, width * RW, torch.int32)
    st = L.sgz_spectrogram_overview_power_device(plan.h, d_xs.data_ptr(), d_xs.stride(0), S, k, img.ptr, pw.ptr, None, _stream())
    torch.cuda.synchronize()
    assert st == api.SGZ_SKIPPED_FRAME and img.untouched() and pw.untouched()
    assert plan.overview_power(xs, k) is None and plan.overview_power(d_xs, k) is None


@pytest.mark.parametrize("over", [dict(channel_mode=config.CH_PHASE), dict(algorithm=config.ALGO_RSNT)], ids=["phase", "rsnt"])
def test_phase_and_rsnt_are_refused(gpu, over):
    import torch
    cfg = config.spectrum_config(window_size=1024, hop=256, axis_points=128, **over)
    plan = api.Plan(cfg).upload()
    L = api.lib()
    x = ov.burst_signal(1024, 256, 9, 2, seed=1)
    d_x = torch.from_numpy(x).to(gpu)
    img = Guarded(gpu, 12, 128 * 4, torch.uint8)
    pw = Guarded(gpu, 12, 2 * 128 * RW, torch.int32)
    st = L.sgz_spectrogram_overview_power_device(plan.h, d_x.data_ptr(), d_x.stride(0), x.shape[1], 1, img.ptr, pw.ptr, None, _stream())
    torch.cuda.synchronize()
    assert st == api.SGZ_EUNSUPPORTED and img.untouched() and pw.untouched()
    with pytest.raises(api.SgzError) as e:
        plan.overview_power(x, 2)
    assert e.value.status == api.SGZ_EUNSUPPORTED
    # the plan renders as before
    assert plan.render(d_x).shape[0] == plan.num_frames(x.shape[1])
    torch.cuda.synchronize()
