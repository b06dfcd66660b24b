"""sgz_image_resize_rows / sgz_image_resize_columns (host only): the tables of the spectrogram image's resize (oglImage.resize(w, h, true),
Spectrum.cpp:503-515) against an independent numpy restatement of the rule in sgz.h."""
import ctypes as C

import numpy as np
import pytest

from signalizer_amd import api


def rows(P0, P1):
    """the row rule of sgz.h, vectorised in float64 (every operation is one IEEE operation, in the order the header gives)"""
    i = np.arange(P1, dtype=np.float64)
    r = (i * (P0 - 1.0)) / (P1 - 1.0)
    j = np.floor(r)
    w = np.floor((r - j) * 256.0 + 0.5)
    carry = w == 256.0
    j = np.where(carry, j + 1.0, j)
    w = np.where(carry, 0.0, w)
    return j.astype(np.int32), w.astype(np.uint16)


def columns(C0, x0, C1):
    """the column rule of sgz.h, in Python integers"""
    x1 = x0 % C1
    src = np.full(C1, -1, np.int32)
    for c in range(C1):
        a = (x1 - 1 - c) % C1
        if a < min(C0, C1):
            src[c] = (x0 - 1 - a) % C0
    return src, x1


SIZES = [2, 3, 200, 1024, 1080, 2160]


@pytest.mark.parametrize("P0", SIZES)
@pytest.mark.parametrize("P1", SIZES)
def test_rows_match_the_rule(P0, P1):
    src, weight = api.image_resize_rows(P0, P1)
    want_src, want_w = rows(P0, P1)
    assert np.array_equal(src, want_src)
    assert np.array_equal(weight, want_w)
    assert src.min() >= 0 and src.max() <= P0 - 1 and weight.max() <= 255
    assert src[0] == 0 and weight[0] == 0 and src[-1] == P0 - 1 and weight[-1] == 0       # the end points map onto each other
    assert (np.diff(src) >= 0).all()


@pytest.mark.parametrize("P", SIZES + [1 << 20])
def test_same_height_copies_the_rows(P):
    src, weight = api.image_resize_rows(P, P)
    assert np.array_equal(src, np.arange(P, dtype=np.int32))
    assert not weight.any()


def test_large_axis_sizes_match_the_rule():
    for P0, P1 in ((1 << 20, 1080), (1080, 1 << 20), ((1 << 20) - 1, 1 << 20)):
        src, weight = api.image_resize_rows(P0, P1)
        want_src, want_w = rows(P0, P1)
        assert np.array_equal(src, want_src) and np.array_equal(weight, want_w)


def _column_cases():
    out = []
    for C0, C1 in ((2048, 1024), (2048, 2048), (2048, 3000), (7, 3), (7, 7), (7, 20), (1, 1), (1, 5), (5, 1), (24, 24), (24, 12), (12, 24)):
        for x0 in sorted({0, C0 // 2, C0 - 1}):
            out.append((C0, x0, C1))
    return out


@pytest.mark.parametrize("C0,x0,C1", _column_cases())
def test_columns_match_the_rule(C0, x0, C1):
    src, x1 = api.image_resize_columns(C0, x0, C1)
    want_src, want_x1 = columns(C0, x0, C1)
    assert x1 == want_x1
    assert np.array_equal(src, want_src)
    kept = src[src >= 0]
    assert len(kept) == min(C0, C1) and len(set(kept.tolist())) == len(kept)     # every kept old column once
    if C0 <= C1:
        assert sorted(kept.tolist()) == list(range(C0))
    # the newest column stays the newest: the one written just before x
    assert src[(x1 - 1) % C1] == (x0 - 1) % C0


@pytest.mark.parametrize("C,x0", [(1, 0), (7, 0), (7, 3), (7, 6), (2048, 0), (2048, 1023), (2048, 2047)])
def test_same_width_is_the_identity(C, x0):
    src, x1 = api.image_resize_columns(C, x0, C)
    assert x1 == x0
    assert np.array_equal(src, np.arange(C, dtype=np.int32))


@pytest.mark.parametrize("P0,P1", [(1, 200), (200, 1), (0, 200), (200, (1 << 20) + 1), ((1 << 20) + 1, 200)])
def test_bad_axis_sizes_are_refused(P0, P1):
    L = api.lib()
    src = np.zeros(max(P1, 1), np.int32)
    weight = np.zeros(max(P1, 1), np.uint16)
    assert L.sgz_image_resize_rows(P0, P1, src.ctypes.data_as(C.c_void_p), weight.ctypes.data_as(C.c_void_p)) == api.SGZ_EINVAL


@pytest.mark.parametrize("C0,x0,C1", [(0, 0, 4), (4, 0, 0), (4, 4, 4), (4, 9, 8), (1 << 31, 0, 4), (4, 0, 1 << 31)])
def test_bad_column_arguments_are_refused(C0, x0, C1):
    L = api.lib()
    src = np.zeros(8, np.int32)
    x1 = C.c_uint32(0)
    assert L.sgz_image_resize_columns(C0, x0, C1, src.ctypes.data_as(C.c_void_p), C.byref(x1)) == api.SGZ_EINVAL


def test_null_tables_are_refused():
    L = api.lib()
    buf = np.zeros(8, np.int32)
    x1 = C.c_uint32(0)
    assert L.sgz_image_resize_rows(4, 8, None, buf.ctypes.data_as(C.c_void_p)) == api.SGZ_EINVAL
    assert L.sgz_image_resize_rows(4, 8, buf.ctypes.data_as(C.c_void_p), None) == api.SGZ_EINVAL
    assert L.sgz_image_resize_columns(4, 0, 8, None, C.byref(x1)) == api.SGZ_EINVAL
    assert L.sgz_image_resize_columns(4, 0, 8, buf.ctypes.data_as(C.c_void_p), None) == api.SGZ_EINVAL


def test_invalid_arguments_of_the_gpu_entry_points_are_refused_without_a_gpu():
    """argument checks come before any device work: a null handle or image, a bad size or layout and overlapping images are refused on any
    machine"""
    L = api.lib()
    x1 = C.c_uint32(0)
    assert L.sgz_spectrum_resize(None, 1080, None, 0, 0) == api.SGZ_EINVAL
    A, B = 0x100000, 0x900000                                   # (never dereferenced)
    ok = (A, 8, 32, 200, 0, B, 8, 32, 300)
    dev = L.sgz_image_resize_device

    def call(src, c0, sp, p0, x0, dst, c1, dp, p1):
        return dev(src, c0, sp, p0, x0, dst, c1, dp, p1, C.byref(x1), None)

    assert call(None, *ok[1:]) == api.SGZ_EINVAL
    assert call(*ok[:5], None, *ok[6:]) == api.SGZ_EINVAL
    assert call(A, 8, 28, 200, 0, B, 8, 32, 300) == api.SGZ_EINVAL          # pitch < 4 * columns
    assert call(A, 8, 32, 200, 0, B, 8, 34, 300) == api.SGZ_EINVAL          # pitch not a multiple of 4
    assert call(A + 2, 8, 32, 200, 0, B, 8, 32, 300) == api.SGZ_EINVAL      # unaligned
    assert call(A, 0, 32, 200, 0, B, 8, 32, 300) == api.SGZ_EINVAL          # no columns
    assert call(A, 8, 32, 200, 8, B, 8, 32, 300) == api.SGZ_EINVAL          # x0 >= C0
    assert call(A, 8, 32, 1, 0, B, 8, 32, 300) == api.SGZ_EINVAL            # P0 < 2
    assert call(A, 8, 32, 200, 0, B, 8, 32, (1 << 20) + 1) == api.SGZ_EINVAL
    # overlapping byte ranges: the same memory, a destination starting inside the source, a source starting inside the destination
    assert call(A, 8, 32, 200, 0, A, 8, 32, 300) == api.SGZ_EINVAL
    assert call(A, 8, 32, 200, 0, A + 32 * 199, 8, 32, 300) == api.SGZ_EINVAL
    assert call(A + 32 * 299, 8, 32, 200, 0, A, 8, 32, 300) == api.SGZ_EINVAL
    for name in ("sgz_spectrum_resize", "sgz_image_resize_rows", "sgz_image_resize_columns", "sgz_image_resize_device"):
        assert name in api.EXPORTS
        assert hasattr(L, name)
