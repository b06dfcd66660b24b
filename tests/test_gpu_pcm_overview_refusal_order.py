"""The order in which the five overview feeds of sgz_pcm_stream refuse (csrc/pcm.hip, pcmOverviewFeed and the calls' own checks): every case
gives a feed two faults at once and holds sgz_last_error() to the text of the fault the feed names first -- the texts and the order are those
of the build in which each feed still had a body of its own.  A refused feed consumes nothing.  Window 64, hop 16, 224 samples of 16-bit
stereo (11 frames), k = 3; the cross feed on the same stream in Phase mode."""
import ctypes as C

import numpy as np
import pytest

from signalizer_amd import api, config

pytestmark = pytest.mark.gpu

W, HOP, P, K = 64, 16, 33, 3
N = W + 10 * HOP                                               # 11 frames
FIRST = W + 3 * HOP + 5                                        # 4 frames: one column closes, one frame stays open
EDGES = [1, 2, 3, 5, 8, 13, 21, 31]
RAW = (np.random.default_rng(5).integers(-20000, 20000, 2 * N)).astype("<i2")
K_TEXT = "overview: k >= 1 frames per column"

# kind -> (the feed call's suffix, its outputs, the index of its records among them, the kind whose open column stands in its way)
KINDS = {"peaks": ("", 2, 1, "stats"), "stats": ("_stats", 3, 1, "peaks"), "power": ("_power", 3, 1, "peaks"), "cross": ("_cross", 1, 0, "peaks"),
         "flux": ("_flux", 1, 0, "peaks")}
WORDS = {"peaks": "peak-hold", "stats": "mean", "power": "power", "cross": "cross", "flux": "flux"}


def _stream(kind):
    mode = config.CH_PHASE if kind == "cross" else config.CH_SEPARATE
    s = api.PcmStream(config.spectrum_config(window_size=W, hop=HOP, axis_points=P, pole=(0.3, 0.3), channel_mode=mode), api.PCM_S16, 2)
    if kind == "cross":
        s.set_cross_edges(EDGES)
    return s


def _open(s, kind, nsamples=FIRST):
    """feeds the first samples into the kind's overview: a column of that kind stays open"""
    feed = {"peaks": s.feed_overview, "stats": s.feed_overview_stats, "power": s.feed_overview_power, "cross": s.feed_overview_cross, "flux": s.feed_overview_flux}[kind]
    feed(RAW[:2 * nsamples], K)
    assert s.open_frames() == 1


_blocks = [np.zeros(1 << 16, np.uint64) for _ in range(3)]      # room for every output of the feeds below, were one of them not refused


def _feed(s, kind, k, outs, capacity, nsamples=N - FIRST, offset=FIRST):
    """the C call as it is, on addresses: (status, columns_out, sgz_last_error()); the stream is where it was"""
    L = api.lib()
    before = (s.open_frames(), s.frames_for(nsamples))
    c = C.c_uint64(0)
    st = getattr(L, "sgz_pcm_stream_feed_overview" + KINDS[kind][0])(s.h, api._np_ptr(RAW[2 * offset:]), nsamples, k, 0, *outs, capacity, C.byref(c), None)
    assert st != api.SGZ_OK and (s.open_frames(), s.frames_for(nsamples)) == before
    return st, int(c.value), L.sgz_last_error().decode()


def _outs(kind, misaligned=False):
    outs = [C.c_void_p(b.ctypes.data) for b in _blocks[:KINDS[kind][1]]]
    if misaligned:
        assert outs[KINDS[kind][2]].value % 8 == 0
        outs[KINDS[kind][2]] = C.c_void_p(outs[KINDS[kind][2]].value + 4)
    return outs


@pytest.mark.parametrize("kind", list(KINDS))
def test_k_0_and_null_outputs(gpu, kind):
    s = _stream(kind)
    assert _feed(s, kind, 0, [None] * KINDS[kind][1], 64, N, 0) == (api.SGZ_EINVAL, 0, K_TEXT)
    s.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_misaligned_records_pointer_and_an_open_column_of_another_kind(gpu, kind):
    """the pointer is named first (the peak hold's peaks are floats: 4 bytes off is aligned, and the open column is what is named)"""
    s, (call, _, _, other) = _stream(kind), KINDS[kind]
    _open(s, other)
    name = "sgz_pcm_stream_feed_overview" + call
    want = {"peaks": f"{name}: the open column is a mean overview's -- flush it (sgz_pcm_stream_feed_overview_stats) or reset the stream first",
            "stats": f"{name}: stats_out is not aligned to 8 bytes", "power": f"{name}: power_out is not aligned to 8 bytes",
            "cross": f"{name}: cross_out is not aligned to 8 bytes", "flux": f"{name}: flux_out is not aligned to 8 bytes"}[kind]
    assert _feed(s, kind, K, _outs(kind, misaligned=True), 64) == (api.SGZ_EINVAL, 0, want)
    # ... and the pointer in order, the open column is what is left
    want = f"{name}: the open column is a {WORDS[other]} overview's -- flush it (sgz_pcm_stream_feed_overview{KINDS[other][0]}) or reset the stream first"
    assert _feed(s, kind, K, _outs(kind), 64) == (api.SGZ_EINVAL, 0, want)
    s.close()


@pytest.mark.parametrize("kind", ["power", "cross", "flux"])
def test_the_track_lane_armed_and_an_open_column_of_another_kind(gpu, kind):
    s = _stream(kind)
    s.set_track(0, 0.5, np.zeros((64, 1, 6), np.float64))
    _open(s, "peaks")
    want = (f"sgz_pcm_stream_feed_overview_{kind}: the track lane is armed and a {kind} feed has no line results to search -- disarm it "
            "(sgz_pcm_stream_set_track) first")
    assert _feed(s, kind, K, _outs(kind), 64) == (api.SGZ_EINVAL, 0, want)
    s.close()


@pytest.mark.parametrize("kind", ["cross", "flux"])
def test_a_capacity_too_small_and_null_records(gpu, kind):
    """the capacity is named first, and the need is reported; with room for the columns, the missing records are named"""
    s, name = _stream(kind), "sgz_pcm_stream_feed_overview_" + kind
    assert _feed(s, kind, K, [None], 2, N, 0) == (api.SGZ_EINVAL, 3, f"{name}: capacity_columns below what this feed yields (see *columns_out)")
    assert _feed(s, kind, K, [None], 3, N, 0) == (api.SGZ_EINVAL, 3, f"{name}: null {kind}_out")
    s.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_another_k_and_a_capacity_too_small(gpu, kind):
    """k is named first (and no need is reported for a k the open column does not have)"""
    s, name = _stream(kind), "sgz_pcm_stream_feed_overview" + KINDS[kind][0]
    _open(s, kind)
    assert _feed(s, kind, K + 1, _outs(kind), 0) == (api.SGZ_EINVAL, 0, f"{name}: k differs from the open column's -- flush or reset first")
    # ... and at the column's k, the capacity
    assert _feed(s, kind, K, _outs(kind), 1) == (api.SGZ_EINVAL, 2, f"{name}: capacity_columns below what this feed yields (see *columns_out)")
    s.close()
