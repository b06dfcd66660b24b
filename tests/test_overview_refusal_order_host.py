"""The order in which the overviews' host calls refuse (csrc/api.hip): every case gives a call two faults at once and holds sgz_last_error() to
the text of the fault the call names first -- the texts and the order are those of the build in which each call still had a body of its own.
Host only: every refusal here comes before the plan is looked at for its upload, on plans that are created and never uploaded, with fake
addresses that are never dereferenced."""
import ctypes as C

import pytest

from signalizer_amd import api, config

AUDIO, OUT = 0x10000, 0x20000
K_TEXT = "overview: k >= 1 frames per column"
CHANNELS_TEXT = "num_channels must equal 2*num_pairs (SpectrumDSP.cpp:65-72)"
RANGE_TEXT = "overview view: x0 < x1 <= n"
SMALL = dict(window_size=64, hop=16, axis_points=33, bin_interp=config.INTERP_LINEAR)
_plans = {}


def _plan(which):
    """a plan that is created and never uploaded: "fft" (Separate), "phase", "rsnt" """
    if which not in _plans:
        over = {"fft": {}, "phase": dict(channel_mode=config.CH_PHASE), "rsnt": dict(algorithm=config.ALGO_RSNT)}[which]
        _plans[which] = api.Plan(config.spectrum_config(**{**SMALL, **over}))
    return _plans[which]


def _planar(*channels):
    return (C.c_void_p * len(channels))(*channels)


# kind -> (the host render, its outputs, the plan its kind supports, a plan its kind refuses or None)
RENDERS = {
    "peaks": ("sgz_spectrogram_overview_host", 2, "fft", None),
    "stats": ("sgz_spectrogram_overview_stats_host", 3, "fft", None),
    "power": ("sgz_spectrogram_overview_power_host", 3, "fft", "rsnt"),
    "cross": ("sgz_spectrogram_overview_cross_host", 1, "phase", "fft"),
    "flux": ("sgz_spectrogram_overview_flux_host", 1, "fft", "rsnt"),
}


def _render(kind, plan, planar, num_channels, k, outs):
    L = api.lib()
    st = getattr(L, RENDERS[kind][0])(plan.h, planar, num_channels, 1000, k, *outs, None)
    return st, L.sgz_last_error().decode()


@pytest.mark.parametrize("kind", list(RENDERS))
def test_k_0_and_no_output(kind):
    """k == 0 together with no output: k is named first, but by the cross and flux renders, whose one output is among the null arguments"""
    outputs, good = RENDERS[kind][1], RENDERS[kind][2]
    st, text = _render(kind, _plan(good), _planar(AUDIO, AUDIO), 2, 0, [None] * outputs)
    assert st == api.SGZ_EINVAL
    assert text == ("null argument" if kind in ("cross", "flux") else K_TEXT)
    # ... and k alone, and the missing outputs alone
    st, text = _render(kind, _plan(good), _planar(AUDIO, AUDIO), 2, 0, [OUT] * outputs)
    assert (st, text) == (api.SGZ_EINVAL, K_TEXT)
    st, text = _render(kind, _plan(good), _planar(AUDIO, AUDIO), 2, 3, [None] * outputs)
    assert st == api.SGZ_EINVAL
    assert text == {"peaks": "overview: an image, the peaks or both", "stats": "overview stats: an image, the records, the means or any of them",
                    "power": "overview power: an image, the records, the levels or any of them", "cross": "null argument", "flux": "null argument"}[kind]


@pytest.mark.parametrize("kind", list(RENDERS))
def test_wrong_num_channels_and_an_unsupported_plan(kind):
    """a wrong num_channels together with a plan the kind does not take (the peak hold and the mean overview take every plan: together with a
    null channel): the channels are named first"""
    outputs, good, bad = RENDERS[kind][1:]
    st, text = _render(kind, _plan(bad or good), _planar(AUDIO, None, AUDIO), 3, 3, [OUT] * outputs)
    assert (st, text) == (api.SGZ_EINVAL, CHANNELS_TEXT)
    # ... then a null channel, then the plan
    st, text = _render(kind, _plan(bad or good), _planar(AUDIO, None), 2, 3, [OUT] * outputs)
    assert (st, text) == (api.SGZ_EINVAL, "null channel")
    if bad:
        st, text = _render(kind, _plan(bad), _planar(AUDIO, AUDIO), 2, 3, [OUT] * outputs)
        assert st == api.SGZ_EUNSUPPORTED
        assert text == {"power": "the power overview reduces transform magnitudes: RSNT plans are not supported",
                        "cross": "the cross overview reduces the complex bins of both channels: only SGZ_CH_PHASE plans keep them",
                        "flux": "the flux overview reduces transform magnitudes: RSNT plans are not supported"}[kind]


def test_the_cross_render_without_a_band_table():
    """a Phase plan without edges: refused behind the channels, in front of the upload"""
    st, text = _render("cross", _plan("phase"), _planar(AUDIO, AUDIO), 2, 3, [OUT])
    assert (st, text) == (api.SGZ_EINVAL, "overview cross: the plan has no band table (sgz_plan_set_cross_edges)")


VIEWS = {
    "peaks": ("sgz_overview_view_host", 2, "sgz_overview_view_host: an image, the peaks or both"),
    "stats": ("sgz_overview_stats_view_host", 3, "sgz_overview_stats_view_host: an image, the records, the means or any of them"),
    "power": ("sgz_overview_power_view_host", 3, "sgz_overview_power_view_host: an image, the records, the levels or any of them"),
}


@pytest.mark.parametrize("kind", list(VIEWS))
def test_a_bad_range_and_no_output(kind):
    """a bad range together with no output: the range is named first"""
    L, (call, outputs, none_text) = api.lib(), VIEWS[kind]
    plan = _plan("fft")
    for x0, x1, text in ((5, 5, RANGE_TEXT), (0, 11, RANGE_TEXT), (0, 10, none_text)):
        assert getattr(L, call)(plan.h, OUT, 10, x0, x1, 4, *[None] * outputs, None) == api.SGZ_EINVAL
        assert L.sgz_last_error().decode() == text
    assert getattr(L, call)(plan.h, OUT, 10, 0, 10, 0, *[None] * outputs, None) == api.SGZ_EINVAL
    assert L.sgz_last_error().decode() == "overview view: out_columns >= 1"
