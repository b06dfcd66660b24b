"""sgz_view_translation_rows (host only): the row table of the spectrogram image's translation on a change of view
(freeLinearVerticalTranslation, Spectrum.cpp:560-561) against an independent numpy restatement of the rule in sgz.h."""
import numpy as np
import pytest

from signalizer_amd import api


def table(P, ol, orr, nl, nr):
    """the rule of sgz.h, vectorised in float64 (every operation is one IEEE operation, in the order the header gives)"""
    S0, S1 = orr - ol, nr - nl
    i = np.arange(P, dtype=np.float64)
    u = nl + S1 * (i / (P - 1.0))
    r = (u - ol) / S0 * (P - 1.0)
    ok = (r >= -0.5) & (r <= P - 0.5)
    r = np.clip(r, 0.0, P - 1.0)
    j = np.floor(r)
    w = np.floor((r - j) * 256.0 + 0.5)
    carry = w == 256.0
    j = np.where(carry, j + 1.0, j)
    w = np.where(carry, 0.0, w)
    src = np.where(ok, j, -1).astype(np.int32)
    weight = np.where(ok, w, 0).astype(np.uint16)
    return src, weight


SIZES = [2, 3, 200, 1024, 2160, 1 << 20]
# (old, new) view rects: zoom in, zoom out (rows with no source), pans both ways, views touching 0 and 1, a move of less than half a row
CASES = [
    ((0.0, 1.0), (0.25, 0.75)),
    ((0.1, 0.9), (0.3, 0.4)),
    ((0.25, 0.75), (0.0, 1.0)),
    ((0.4, 0.5), (0.1, 0.9)),
    ((0.2, 0.6), (0.3, 0.7)),
    ((0.3, 0.7), (0.2, 0.6)),
    ((0.0, 0.5), (0.5, 1.0)),
    ((0.5, 1.0), (0.0, 0.5)),
    ((0.0, 0.3), (0.0, 0.6)),
    ((0.7, 1.0), (0.4, 1.0)),
    ((0.0, 1.0), (1e-7, 1.0 - 1e-7)),
    ((0.123456789, 0.87654321), (0.123456789 + 3e-5, 0.87654321 + 3e-5)),
]


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("old,new", CASES)
def test_rows_match_the_rule(P, old, new):
    src, weight = api.view_translation_rows(P, *old, *new)
    want_src, want_w = table(P, *old, *new)
    assert np.array_equal(src, want_src)
    assert np.array_equal(weight, want_w)
    assert src.max() <= P - 1 and weight.max() <= 255
    assert ((src >= 0) | (weight == 0)).all()


@pytest.mark.parametrize("P", SIZES)
def test_rows_with_and_without_a_source(P):
    """zooming out leaves rows outside the old view without a source; zooming in gives every row one"""
    src, _ = api.view_translation_rows(P, 0.4, 0.6, 0.0, 1.0)
    assert (src == -1).any() and ((src >= 0).any() or P == 2)         # (P = 2: both rows lie outside the old view)
    src, _ = api.view_translation_rows(P, 0.0, 1.0, 0.4, 0.6)
    assert (src >= 0).all()


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("view", [(0.0, 1.0), (0.25, 0.75), (0.1, 0.2), (0.999, 1.0)])
def test_unchanged_rect_is_the_identity(P, view):
    src, weight = api.view_translation_rows(P, *view, *view)
    assert np.array_equal(src, np.arange(P, dtype=np.int32))
    assert not weight.any()


def test_sub_row_move_blends_neighbours():
    """a rect that moves by less than half a row keeps every row's source and blends it with the next one"""
    P = 1024
    d = 0.3 / (P - 1)                                          # 0.3 rows in the old view's units
    src, weight = api.view_translation_rows(P, 0.2, 0.6, 0.2 + 0.4 * d, 0.6 + 0.4 * d)
    assert np.array_equal(src[:-1], np.arange(P - 1, dtype=np.int32))
    assert (weight[:-1] == 77).all()                          # floor(0.3 * 256 + 0.5), up to the fp64 rounding of the view fractions
    assert src[-1] == P - 1 and weight[-1] == 0               # beyond the last row by less than half a row: clamped to it


@pytest.mark.parametrize("args", [
    (1, 0.0, 1.0, 0.0, 1.0),
    (200, 0.5, 0.5, 0.0, 1.0),
    (200, 0.0, 1.0, 0.6, 0.4),
    (200, -0.1, 1.0, 0.0, 1.0),
    (200, 0.0, 1.0, 0.0, 1.5),
    (200, 0.0, float("nan"), 0.0, 1.0),
    (200, 0.0, 1.0, float("-inf"), 1.0),
])
def test_invalid_views_are_refused(args):
    with pytest.raises(api.SgzError) as e:
        api.view_translation_rows(*args)
    assert e.value.status == api.SGZ_EINVAL


def test_invalid_arguments_of_the_gpu_entry_points_are_refused_without_a_gpu():
    """argument checks come before any device work: a null handle / image and an invalid view are refused on any machine"""
    L = api.lib()
    assert L.sgz_spectrum_set_view(None, 0.0, 1.0) == api.SGZ_EINVAL
    assert L.sgz_view_translate_device(None, 4, 16, 200, 0.0, 1.0, 0.2, 0.8, None) == api.SGZ_EINVAL
    assert L.sgz_view_translate_device(0x1000, 4, 16, 200, 0.0, 1.0, 0.8, 0.2, None) == api.SGZ_EINVAL
    assert L.sgz_view_translate_device(0x1000, 4, 12, 200, 0.0, 1.0, 0.2, 0.8, None) == api.SGZ_EINVAL
    assert L.sgz_view_translate_device(0x1000, 4, 16, 1, 0.0, 1.0, 0.2, 0.8, None) == api.SGZ_EINVAL
    for name in ("sgz_spectrum_set_view", "sgz_view_translation_rows", "sgz_view_translate_device"):
        assert name in api.EXPORTS
