"""sgz_spectrum_update_effects (host only): what sgz_spectrum_update does for a change of configuration -- the field classes of
Spectrum::handleFlagUpdates (Spectrum.cpp:351-616) restated in Python and compared over every single-field change and a seeded sweep of
multi-field changes, refusals included."""
import ctypes as C
import random

import pytest

from signalizer_amd import api, config

PIECE = 16384

LOOK = ("low_db", "high_db", "clip_db", "colours", "ratios", "pole", "slope_a", "slope_b", "bin_interp")
WINDOW = ("window_type", "window_symmetry", "window_alpha", "window_beta", "free_q")
VIEW = ("view_scaling", "min_log_freq", "view_left", "view_right", "channel_mode")


def _cap(c):
    return ((c["hop"] if c["algorithm"] == config.ALGO_RSNT else c["window_size"]) + 2 * PIECE + 63) & ~63


def _valid(c):
    """what sgz_spectrum_create refuses (buildPlan's checks and the handle's own), for the values this file generates"""
    if c["num_pairs"] > 16 or c["display_mode"] > 1 or c["window_size"] < 1 or c["hop"] < 1 or c["axis_points"] < 2:
        return False
    if c["window_size"] > 1 << 24 or c["axis_points"] > 1 << 20 or c["channel_mode"] > 7 or c["bin_interp"] > 2 or c["view_scaling"] > 1:
        return False
    if c["window_type"] >= 13 or c["algorithm"] > 1:
        return False
    if not (0.0 <= c["view_left"] < c["view_right"] <= 1.0):
        return False
    if c["view_scaling"] == 1 and not (0.0 < c["min_log_freq"] < c["sample_rate"] * 0.5):
        return False
    return c["high_db"] > c["low_db"]


def _same(a, b, k):
    if k in ("colours", "ratios", "pole"):
        return [tuple(x) if isinstance(x, (list, tuple)) else x for x in a[k]] == [tuple(x) if isinstance(x, (list, tuple)) else x for x in b[k]]
    return a[k] == b[k]


def _expected(a, b):
    """(status, effects) of the table in sgz.h"""
    if not _valid(b):
        return api.SGZ_EINVAL, None
    if a["sample_rate"] != b["sample_rate"] or a["num_pairs"] != b["num_pairs"] or a["display_mode"] != b["display_mode"]:
        return api.SGZ_EUNSUPPORTED, None
    if a["axis_points"] != b["axis_points"]:
        return api.SGZ_EINVAL, None
    ch = lambda keys: any(not _same(a, b, k) for k in keys)
    look, window, view = ch(LOOK), ch(WINDOW), ch(VIEW)
    size, hop, algo = ch(("window_size",)), ch(("hop",)), ch(("algorithm",))
    rect = ch(("view_left", "view_right"))
    fx = 0
    if look or window or size or hop or view or algo:
        fx |= api.UPDATE_PLANS
    if view or algo:
        fx |= api.UPDATE_CLEAR_LINES
    if algo:
        fx |= api.UPDATE_CLEAR_STATE
    if b["algorithm"] == config.ALGO_RSNT and (window or size or view or algo):
        fx |= api.UPDATE_RESONATORS_AT_REST
    if b["display_mode"] == 1 and rect:
        fx |= api.UPDATE_TRANSLATE_IMAGE
    if _cap(a) != _cap(b):
        fx |= api.UPDATE_RING_MOVED
    return api.SGZ_OK, fx


def _effects(a, b):
    ca, cb, fx = api.config_from_dict(a), api.config_from_dict(b), C.c_uint32(0xdead)
    st = api.lib().sgz_spectrum_update_effects(C.byref(ca), C.byref(cb), C.byref(fx))
    return st, (fx.value if st == api.SGZ_OK else None)


def _base(**over):
    c = config.spectrum_config(window_size=4096, hop=512, axis_points=200)
    c.update(over)
    return c


# one changed value per field (several for the fields whose change moves the ring or is refused)
SINGLE = [
    ("low_db", -90.0), ("high_db", 6.0), ("clip_db", -200.0), ("slope_a", 0.5), ("slope_b", 2.0), ("bin_interp", 0), ("bin_interp", 1),
    ("pole", (0.5, 0.99)), ("pole", (0.9, 0.5)), ("ratios", (0.1, 0.2, 0.3, 0.2, 0.2)),
    ("colours", [(1, 0, 0), (0, 0, 64), (0, 128, 255), (0, 255, 128), (255, 255, 0), (255, 64, 0)]),
    ("window_type", config.WIN_BLACKMAN), ("window_symmetry", 0), ("window_alpha", 0.3),
    ("window_beta", 0.7), ("free_q", 1),
    ("window_size", 32768), ("window_size", 4097), ("window_size", 4100), ("window_size", 100), ("window_size", 0), ("window_size", (1 << 24) + 1),
    ("hop", 1536), ("hop", 1), ("hop", 0), ("hop", 16385),
    ("view_scaling", 0), ("min_log_freq", 20.0), ("min_log_freq", 24000.0), ("view_left", 0.2), ("view_right", 0.8), ("view_left", 1.0),
    ("channel_mode", 2), ("channel_mode", 4), ("channel_mode", 7), ("channel_mode", 8),
    ("algorithm", 1), ("algorithm", 2),
    ("sample_rate", 44100.0), ("num_pairs", 2), ("num_pairs", 17), ("display_mode", 0), ("display_mode", 2),
    ("axis_points", 201), ("axis_points", 1),
]


@pytest.mark.parametrize("algorithm", [config.ALGO_FFT, config.ALGO_RSNT])
@pytest.mark.parametrize("display_mode", [0, 1])
@pytest.mark.parametrize("field,value", SINGLE, ids=[f"{f}={v}" for f, v in SINGLE])
def test_single_field_changes(field, value, algorithm, display_mode):
    a = _base(algorithm=algorithm, display_mode=display_mode)
    b = dict(a)
    b[field] = value
    st, fx = _effects(a, b)
    want = _expected(a, b)
    assert (st, fx) == want


@pytest.mark.parametrize("algorithm", [config.ALGO_FFT, config.ALGO_RSNT])
@pytest.mark.parametrize("display_mode", [0, 1])
def test_equal_configurations_have_no_effects(algorithm, display_mode):
    a = _base(algorithm=algorithm, display_mode=display_mode)
    assert _effects(a, dict(a)) == (api.SGZ_OK, 0)


def test_the_table_rows():
    a = _base()
    F = api.spectrum_update_effects
    assert F(a, dict(a, low_db=-100.0)) == api.UPDATE_PLANS
    assert F(a, dict(a, window_type=4)) == api.UPDATE_PLANS
    assert F(a, dict(a, window_size=32768)) == api.UPDATE_PLANS | api.UPDATE_RING_MOVED
    assert F(a, dict(a, hop=1536)) == api.UPDATE_PLANS
    assert F(a, dict(a, channel_mode=2)) == api.UPDATE_PLANS | api.UPDATE_CLEAR_LINES
    assert F(a, dict(a, view_left=0.1)) == api.UPDATE_PLANS | api.UPDATE_CLEAR_LINES | api.UPDATE_TRANSLATE_IMAGE
    assert F(a, dict(a, algorithm=1)) == (api.UPDATE_PLANS | api.UPDATE_CLEAR_LINES | api.UPDATE_CLEAR_STATE | api.UPDATE_RESONATORS_AT_REST
                                          | api.UPDATE_RING_MOVED)
    r = _base(algorithm=1)
    assert F(r, dict(r, hop=1536)) == api.UPDATE_PLANS | api.UPDATE_RING_MOVED
    assert F(r, dict(r, window_type=4)) == api.UPDATE_PLANS | api.UPDATE_RESONATORS_AT_REST
    assert F(r, dict(r, window_size=8192)) == api.UPDATE_PLANS | api.UPDATE_RESONATORS_AT_REST
    assert F(r, dict(r, high_db=3.0)) == api.UPDATE_PLANS
    with pytest.raises(api.SgzError) as e:
        F(a, dict(a, sample_rate=44100.0))
    assert e.value.status == api.SGZ_EUNSUPPORTED
    with pytest.raises(api.SgzError) as e:
        F(a, dict(a, axis_points=300))
    assert e.value.status == api.SGZ_EINVAL


def _mutate(rng, c):
    k = rng.choice(["low_db", "high_db", "clip_db", "slope_a", "slope_b", "bin_interp", "pole", "ratios", "colours", "window_type",
                    "window_symmetry", "window_alpha", "window_beta", "free_q", "window_size", "hop", "view_scaling", "min_log_freq",
                    "view_left", "view_right", "channel_mode", "algorithm", "sample_rate", "num_pairs", "display_mode", "axis_points"])
    choices = {
        "low_db": [-120.0, -90.0, 10.0], "high_db": [0.0, 6.0, -130.0], "clip_db": [-384.0, -200.0], "slope_a": [0.0, 0.5],
        "slope_b": [1.0, 2.0], "bin_interp": [0, 1, 2], "pole": [(0.9, 0.99), (0.5, 0.99)], "ratios": [(0.2,) * 5, (0.1, 0.2, 0.3, 0.2, 0.2)],
        "colours": [c["colours"], [(9, 9, 9)] + list(c["colours"])[1:]], "window_type": [1, 4, 12], "window_symmetry": [0, 1],
        "window_alpha": [0.0, 0.3], "window_beta": [0.0, 0.7], "free_q": [0, 1], "window_size": [4096, 4100, 32768, 100],
        "hop": [512, 1536, 2048, 40000], "view_scaling": [0, 1], "min_log_freq": [10.0, 20.0, 30000.0], "view_left": [0.0, 0.2, 0.9],
        "view_right": [1.0, 0.8, 0.1], "channel_mode": [0, 2, 4, 5, 7], "algorithm": [0, 1], "sample_rate": [48000.0, 44100.0],
        "num_pairs": [1, 2], "display_mode": [0, 1], "axis_points": [200, 256],
    }
    c[k] = rng.choice(choices[k])


def test_random_multi_field_changes():
    rng = random.Random(20261016)
    seen = set()
    for _ in range(3000):
        a = _base(algorithm=rng.choice([0, 1]), display_mode=rng.choice([0, 1]))
        b = dict(a)
        for _ in range(rng.randint(2, 6)):
            _mutate(rng, b)
        st, fx = _effects(a, b)
        want = _expected(a, b)
        assert (st, fx) == want, (a, b)
        seen.add(st if fx is None else fx)
    assert api.SGZ_EINVAL in seen and api.SGZ_EUNSUPPORTED in seen and len(seen) > 12


def test_null_arguments_are_refused():
    L = api.lib()
    a = api.config_from_dict(_base())
    fx = C.c_uint32(0)
    assert L.sgz_spectrum_update(None, C.byref(a)) == api.SGZ_EINVAL
    assert L.sgz_spectrum_update(None, None) == api.SGZ_EINVAL
    assert L.sgz_spectrum_update_effects(None, C.byref(a), C.byref(fx)) == api.SGZ_EINVAL
    assert L.sgz_spectrum_update_effects(C.byref(a), None, C.byref(fx)) == api.SGZ_EINVAL
    assert L.sgz_spectrum_update_effects(C.byref(a), C.byref(a), None) == api.SGZ_EINVAL


def test_ring_resize_refuses_null_rings_without_a_device():
    L = api.lib()
    assert L.sgz_ring_resize_device(None, 64, None, 64, 1, 0, None) == api.SGZ_EINVAL


def test_new_symbols_are_exported():
    L = api.lib()
    for name in ("sgz_spectrum_update", "sgz_spectrum_update_effects", "sgz_ring_resize_device"):
        assert name in api.EXPORTS
        assert hasattr(L, name)
