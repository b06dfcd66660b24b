"""sgz_stage_band_columns on the GPU (csrc/band_columns.hip): byte for byte, no tolerance, against tests/band_ref.py.

Every call goes through `stage`, which poisons everything around what the call may write -- the padding between the channel rows, a record
in front of the output and the records behind its last column, words in front of and behind the carry -- and checks it afterwards; a call
with samples must write the whole carry (the open column or zeros, the history, the zero word), a call without must leave it alone.  The
sizes follow the code through api.band_columns_limits() and the filter's own W and L.  The shapes are the smallest at which each mechanism
can go wrong, mostly with the tiny filter (W = 64, L = 16: 256 segments in a run tile, four rounds of the runs)."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import band_ref as br  # noqa: E402
import wave_ref as wr  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = np.uint32(0xDEADBEEF)
WORDS = br.DTYPE.itemsize // 4
E = api.SGZ_EINVAL
_filters = {}


def filt(which):
    if which not in _filters:
        if which == "tiny":
            _filters[which] = api.band_filter(br.TINY.c, br.TINY.W, br.TINY.L)
        elif which == "wide":                                       # the widest memory the device takes, four segments in a tile
            _filters[which] = api.band_filter(br.TINY.c, 16384, 1024)
        else:
            _filters[which] = api.band_filter_for_rate(which)
    return _filters[which]


def limits(f, channels=1):
    return api.band_columns_limits(f, channels)


def _dev(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def loud(channels, S, seed):
    """float32 [channels][S]: around and beyond the quantiser's clamp at +-8.0, with infinities"""
    rng = np.random.default_rng(seed)
    values = np.array([8.0, -8.0, 8.000001, -8.000001, 7.9999995, -7.9999995, 100.0, -100.0, np.inf, -np.inf, 3.0, -0.5], np.float32)
    return values[rng.integers(0, len(values), size=(channels, S))]


def content(kind, channels, S, m, seed):
    if kind == "loud":
        return loud(channels, S, seed)
    if kind == "sine":
        n = np.arange(S, dtype=np.float64)
        return np.stack([((0.9 - 0.1 * d) * np.sin(0.05 * (d + 1) * n) + 0.2).astype(np.float32) for d in range(channels)])
    return wr.content(kind, channels, S, m, seed)     # random / constant / ramp: NaN, +-inf, +-0, denormals first, last, alone; all-NaN columns


KINDS = ("random", "sine", "loud", "constant", "ramp", "plain")


class Planar:
    """x float32 [channels][S] on the device: rows `stride` = S + pad apart, the first one `offset` floats behind a 16-byte boundary, poison in
    front, between and behind"""

    def __init__(self, x, offset=0, pad=0):
        self.channels, self.S = x.shape
        self.stride = self.S + pad
        self.offset = offset
        flat = np.full(4 + self.channels * self.stride + 8, POISON, np.uint32)
        for d in range(self.channels):
            flat[offset + d * self.stride:offset + d * self.stride + self.S] = wr.bits_of(x[d])
        self.before = flat
        self.t = _dev(flat)
        assert self.t.data_ptr() % 16 == 0

    def at(self, sample):
        return self.t[self.offset + sample:]

    def unchanged(self):
        return np.array_equal(_host(self.t), self.before)


def stage(p, at, n, f, first_index, m, held=0, flush=True, continued=False, slices=0, carry=None, extra=3, stream=None):
    """the call on samples [at, at + n) of p with the carry (uint32 words [channels][16 + W + L], or None: poison) -> (records
    [columns][channels], the carry afterwards or None where the call must not write it); asserts SGZ_OK, the counts, and that nothing but
    the documented bytes changed"""
    import torch
    channels = p.channels
    cwords = br.carry_bytes(f) // 4
    columns, left = api.overview_step(m, held, n, flush)
    out = _dev(np.full((1 + columns + extra) * channels * WORDS, POISON, np.uint32))
    carry_before = np.full(4 + channels * cwords + 4, POISON, np.uint32)
    if carry is not None:
        carry_before[4:4 + channels * cwords] = np.ascontiguousarray(carry, np.uint32).reshape(-1)
    c = _dev(carry_before)
    st = api.stage_band_columns(p.at(at), p.stride, channels, n, f, first_index, m, held, flush, continued, slices, c[4:], out[channels * WORDS:],
                                stream=stream)
    assert st == api.SGZ_OK, (st, api.lib().sgz_last_error())
    torch.cuda.synchronize()
    got, carry_after = _host(out), _host(c)
    first, last = channels * WORDS, (1 + columns) * channels * WORDS
    assert (got[:first] == POISON).all() and (got[last:] == POISON).all(), "bytes in front of the output or behind the last column were written"
    assert p.unchanged(), "the source or its padding was written"
    records = np.ascontiguousarray(got[first:last]).view(br.DTYPE).reshape(columns, channels)
    assert not records["reserved"].any()
    if n:
        assert (carry_after[:4] == POISON).all() and (carry_after[4 + channels * cwords:] == POISON).all()
        after = np.ascontiguousarray(carry_after[4:4 + channels * cwords]).reshape(channels, cwords)
        assert not after[:, -1].any(), "the word behind the history is written as 0"
        if not left:
            assert not after[:, :WORDS].any(), "no sample stays open: the open column is written as zeros"
        return records, after
    assert np.array_equal(carry_after, carry_before), "the carry was written by a call without samples"
    return records, None


def expect(x, f, m, held, flush, history, base):
    """x [channels][held + n]: the stream behind `history` (int [channels][any] or None), its first sample at index `base`; the call takes the
    last n -> (carry in or None, records, carry out or None)"""
    channels, n = x.shape[0], x.shape[1] - held
    carry_in = None
    if history is not None:
        open_ = np.zeros(channels, br.DTYPE)
        if held:
            open_ = br.records_of(x[:, :held], f, m, True, history, base)[0][0]
        else:
            open_["sumsq"], open_["count"], open_["reserved"] = 0xABABABABABABABAB, 0xABABABAB, 0xABABABAB       # read iff held > 0
        carry_in = br.carry_of(f, open_, br.history_after(x[:, :held], f, history))
        carry_in[:, -1] = 0xFFFFFFFF                                                                           # (never read)
    every, _ = br.records_of(x, f, m, True, history, base)
    open_ = (not flush) and (held + n) % m != 0
    carry_out = None
    if n:
        carry_out = br.carry_of(f, every[-1] if open_ else np.zeros(channels, br.DTYPE), br.history_after(x, f, history))
    return carry_in, (every[:-1] if open_ else every), carry_out


def check(x, f, m, held, flush, slices=0, offset=0, pad=0, history=None, base=0, what=None):
    n = x.shape[1] - held
    carry_in, want, carry_out = expect(x, f, m, held, flush, history, base)
    p = Planar(x, offset, pad)
    got, carry = stage(p, held, n, f, base + held, m, held, flush, history is not None, slices, carry_in)
    assert _same(got, want), what
    assert (carry is None) == (carry_out is None) and (carry is None or _same(carry, carry_out)), what
    return got, carry


def random_history(f, channels, seed, length=None):
    """int [channels][length] (default: W + L - 1, all the carry holds); a shorter one has zeros in front of it"""
    rng = np.random.default_rng(seed)
    length = br.hist_len(f) if length is None else length
    h = rng.integers(-br.CLAMP, br.CLAMP + 1, size=(channels, length))
    h[:, seed % h.shape[1]] = (br.CLAMP, -br.CLAMP)[seed % 2]
    return h


def test_limits(gpu):
    import ctypes as C
    for which in ("tiny", 48000, "wide"):
        f = filt(which)
        for channels in (1, 3, 64):
            assert limits(f, channels) == (1024, 4096, channels * br.carry_bytes(f))
    assert limits(api.band_filter(br.TINY.c, 16384, 16384))[1] == 16384
    L = api.lib()
    assert L.sgz_band_columns_limits(C.byref(api.band_filter(br.TINY.c, 32768, 64)), 1, None, None, None) == E     # W above what the LDS takes
    assert L.sgz_band_columns_limits(C.byref(api.band_filter(br.TINY.c, 64, 24)), 1, None, None, None) == E
    assert L.sgz_band_columns_limits(C.byref(filt("tiny")), 65, None, None, None) == E
    assert L.sgz_band_columns_limits(None, 1, None, None, None) == E


# n = 1, L - 1, L, L + 1, one below, at and one above a tile, two tiles and one; with each: every m of the list, first_index % L of 0, 1 and
# L - 1, continued 0 and 1 with a history shorter than W, of W and of W + L - 1, 1 to 3 channels, row offsets of 0 to 3 floats, padding, held
NS = (1, 15, 16, 17, 4095, 4096, 4097, 8193)


@pytest.mark.parametrize("ni", range(len(NS)))
def test_records_equal_the_definition(gpu, ni):
    f = filt("tiny")
    W, L = f.W, f.L
    switch, tile, _ = limits(f)
    assert (L, tile) == (16, 4096) and NS[4:7] == (tile - 1, tile, tile + 1)
    n = NS[ni]
    i = 5 * ni
    for m in (1, 3, L, 3 * L + 5, switch, switch + 1):
        held = (0, 1 % m, m - 1)[i % 3]
        flush = bool(i % 2)
        channels, offset, pad = (1, 2, 3)[i % 3], i % 4, (0, 1, 7, 64)[(i // 3) % 4]
        kind = KINDS[(i // 2) % len(KINDS)]
        base = (0, 1, L - 1, 5 * L + 1, 2 ** 40 + L - 1, L)[i % 6]
        hist_len = (None, 5, W, W + L - 1, W - 1)[i % 5]               # None: the stream begins here (continued = 0)
        x = content(kind, channels, held + n, m, seed=1000 * m + i)
        history = random_history(f, channels, i, hist_len or W) if held or hist_len else None
        check(x, f, m, held, flush, offset=offset, pad=pad, history=history, base=base,
              what=(n, m, held, flush, channels, offset, pad, kind, base, hist_len))
        i += 1


def test_every_phase_of_the_segment_grid(gpu):
    """first_index % L = 0 .. L - 1 on one stream: the first segment is re-run from its start out of the history, its earlier samples not stored"""
    f = filt("tiny")
    x = content("sine", 2, 200, 7, seed=3)
    history = random_history(f, 2, 9)
    for phase in range(f.L):
        check(x, f, 7, 3, False, offset=1, pad=2, history=history, base=4 * f.L + phase - 3, what=phase)


def test_one_case_with_the_48_kHz_filter(gpu):
    f = filt(48000)
    assert (f.W, f.L) == (1024, 64)
    tile = limits(f)[1]
    x = content("sine", 2, 3 + 2 * tile + f.L + 1, 1000, seed=48)
    check(x, f, 1000, 3, False, offset=1, pad=3, history=random_history(f, 2, 1), base=f.L - 2)
    x = content("random", 1, f.W + 1, 7, seed=49)
    check(x, f, 7, 0, True, offset=3, pad=1)


def test_one_case_with_the_widest_memory(gpu):
    """W = 16384, L = 1024: four segments in a tile, 64 lanes on every dot product, two tiles"""
    f = filt("wide")
    tile = limits(f)[1]
    x = content("loud", 1, 1 + 2 * tile, 1025, seed=5)
    check(x, f, 1025, 1, True, offset=1, history=random_history(f, 1, 2), base=1000)


def test_a_long_segment_is_a_tile_of_its_own(gpu):
    """L = W = 8192: one segment per tile, every lane on the one dot product (folded through LDS), eight rounds of the runs"""
    f = api.band_filter(br.TINY.c, 8192, 8192)
    x = content("sine", 1, 8192 + 5, 1000, seed=5)
    check(x, f, 1000, 0, True, offset=1, base=8000)


def test_forced_slices_give_the_same_bytes(gpu):
    f = filt("tiny")
    tile = limits(f)[1]
    for m, n in ((3, 1000), (3 * tile, 3 * tile + 2 * tile + 5)):       # (a column of 3 tiles: two of them, and an open one)
        for channels, pad in ((1, 1), (3, 2)):
            x = content(("random", "loud")[channels == 3], channels, 2 + n, m, seed=m)
            history = random_history(f, channels, m)
            auto, carry0 = check(x, f, m, 2 % m, False, slices=0, offset=3, pad=pad, history=history, base=17, what=(m, n, channels))
            for slices in (1, 2, 7, 64):
                got, carry = check(x, f, m, 2 % m, False, slices=slices, offset=3, pad=pad, history=history, base=17, what=(m, n, channels, slices))
                assert _same(got, auto) and _same(carry, carry0)


def chain(p, x, f, m, cuts, base=0, flush_last=True):
    """the calls on [0, cuts[0]), [cuts[0], cuts[1]), ..: the concatenated records; the carry is checked after every call"""
    parts, at, held, carry, continued = [], 0, 0, None, False
    S = x.shape[1]
    for cut in cuts:
        last = cut == S and flush_last
        got, after = stage(p, at, cut - at, f, base + at, m, held, flush=last, continued=continued, carry=carry)
        parts.append(got)
        if after is not None:
            carry, continued = after, True
            assert np.array_equal(after[:, WORDS:-1].view(np.int32), br.history_after(x[:, :cut], f)), cut
        held, at = (0 if last else (held + cut - at) % m), cut
    return np.concatenate(parts), carry


def test_a_chain_cut_at_random_places_equals_one_call(gpu):
    f = filt("tiny")
    tile = limits(f)[1]
    S = 2 * tile + 77
    x = content("random", 2, S, 50, seed=11)
    p = Planar(x, offset=1, pad=3)
    rng = np.random.default_rng(2024)
    for m, base in ((50, 5), (1500, 0)):
        want, _ = br.records_of(x, f, m, True, None, base)
        single, _ = stage(p, 0, S, f, base, m)
        assert _same(single, want)
        cuts = sorted(set(rng.integers(1, S, size=12).tolist()) | {int(rng.integers(1, f.L)), S})
        got, _ = chain(p, x, f, m, cuts, base)
        assert _same(got, want), (m, cuts)


def test_cuts_around_L_and_W(gpu):
    """the second call's history is shorter than W, exactly W, W + L - 1 and longer"""
    f = filt("tiny")
    W, L = f.W, f.L
    S = 2 * W + 3 * L + 5
    x = content("sine", 2, S, 10, seed=12)
    x[:, 50] = np.nan
    p = Planar(x, offset=3, pad=1)
    for m in (7, 100):
        want, _ = br.records_of(x, f, m, True, None, 3)
        for cuts in ([1], [L - 1, L + 1], [L, W + 1], [1, W - 1], [W - 1, W], [W], [W + L - 1], [W + L - 1, W + L + 1], [L - 1, L, L + 1], [W + 1, 2 * W - 1, 2 * W + L]):
            got, _ = chain(p, x, f, m, cuts + [S], 3)
            assert _same(got, want), (m, cuts)


def test_a_flush_does_not_move_the_segment_grid(gpu):
    f = filt("tiny")
    S, n1 = 3 * f.W + 11, f.W + f.L // 2 + 3                            # the flush falls inside a segment
    x = content("sine", 2, S, 50, seed=13)
    p = Planar(x, pad=2)
    m = 50
    head, _ = br.records_of(x[:, :n1], f, m, True)
    tail, _ = br.records_of(x[:, n1:], f, m, True, br.quantise(x[:, :n1])[0], n1)
    # the flush with the samples, then more samples
    a, carry = stage(p, 0, n1, f, 0, m, flush=True)
    b, _ = stage(p, n1, S - n1, f, n1, m, flush=True, continued=True, carry=carry)
    assert _same(a, head) and _same(b, tail)
    # the flush alone (nsamples == 0), on the carry of a call that left the column open: the carry stays, and so does the history
    a0, carry = stage(p, 0, n1, f, 0, m, flush=False)
    a1, none = stage(p, n1, 0, f, n1, m, held=n1 % m, flush=True, continued=True, carry=carry)
    assert none is None and _same(np.concatenate([a0, a1]), head)
    b, _ = stage(p, n1, S - n1, f, n1, m, flush=True, continued=True, carry=carry)
    assert _same(b, tail)


def test_special_values(gpu):
    f = filt("tiny")
    tile = limits(f)[1]
    for m in (1, 64, 1025):
        for kind in ("random", "constant", "ramp", "loud"):
            x = content(kind, 2, tile + 3 * m + 1, m, seed=m)
            got, _ = check(x, f, m, 0, True, offset=2, pad=3, what=(m, kind))
            if kind == "random":
                assert (got["count"] < np.minimum(m, x.shape[1])).any()     # some NaNs were not counted
    x = np.full((2, 300), np.nan, np.float32)
    got, _ = check(x, f, 10, 0, True)
    assert got.tobytes() == bytes(got.nbytes)
    d = np.full((1, 200), 1e-40, np.float32)                            # denormals quantise to 0
    got, _ = check(d, f, 50, 0, True)
    assert not got["sumsq"].any() and (got["count"] == 50).all()
    # the clamp: a run of +8.0 and beyond drives every band's q to what the definition says, far above one column's 64-bit sum
    x = np.full((1, 3000), np.inf, np.float32)
    got, _ = check(x, f, 3000, 0, True)
    assert int(got["sumsq"][0, 0, 0, 1]) > 0                            # the low band's sum passed 2^64


def test_refusals_write_nothing(gpu):
    import torch
    f = filt("tiny")
    x = wr.content("plain", 1, 100, 8, seed=1)
    p = Planar(x, pad=4)
    cwords = br.carry_bytes(f) // 4
    out = _dev(np.full(64 * WORDS, POISON, np.uint32))
    carry = _dev(np.full(2 * cwords, POISON, np.uint32))
    call = api.stage_band_columns
    c = [list(r) for r in br.TINY.c]
    big = [[0.0, 2.5, 0.0, 0.0, 0.0]] + c[1:]                                                          # z0 of lp1a after one step is 2.5: 2.5 * 2^30 is no int32
    bad_taps = api.band_filter(big, 64, 16)
    assert br.taps(bad_taps) is None
    #                  planar stride ch n   f  first m held flush continued slices
    assert call(None, p.stride, 1, 100, f, 0, 8, 0, True, False, 0, carry, out) == E                  # a null d_planar
    assert call(p.at(0), p.stride, 1, 100, None, 0, 8, 0, True, False, 0, carry, out) == E            # a null filter
    assert call(p.at(0), p.stride, 1, 100, bad_taps, 0, 8, 0, True, False, 0, carry, out) == E        # a filter whose table is refused
    assert call(p.at(0), p.stride, 1, 100, api.band_filter(br.TINY.c, 96, 16), 0, 8, 0, True, False, 0, carry, out) == E
    assert call(p.at(0), p.stride, 1, 100, api.band_filter(br.TINY.c, 32768, 2048), 0, 8, 0, True, False, 0, carry, out) == E     # W > 16384
    assert call(p.at(0), p.stride, 0, 100, f, 0, 8, 0, True, False, 0, carry, out) == E               # channels 0
    assert call(p.at(0), p.stride, 65, 100, f, 0, 8, 0, True, False, 0, carry, out) == E              # channels above 64
    assert call(p.at(0), p.stride, 1, 100, f, 0, 0, 0, True, False, 0, carry, out) == E               # m == 0
    assert call(p.at(0), p.stride, 1, 100, f, 0, 8, 8, True, True, 0, carry, out) == E                # held >= m
    assert call(p.at(0), p.stride, 1, 100, f, 0, 8, 3, True, False, 0, carry, out) == E               # held > 0 where the stream begins
    assert call(p.at(0), 99, 1, 100, f, 0, 8, 0, True, False, 0, carry, out) == E                     # channel_stride < nsamples
    assert call(p.at(0), 2 ** 41, 1, 2 ** 40 + 1, f, 0, 8, 0, True, False, 0, carry, out) == E        # nsamples above 2^40
    assert call(p.at(0), p.stride, 1, 100, f, 2 ** 62 + 1, 8, 0, True, False, 0, carry, out) == E     # first_index above 2^62
    assert call(p.at(0), p.stride, 1, 100, f, 0, 8, 0, True, False, 65, carry, out) == E              # slices > 64
    assert call(p.at(0), p.stride, 1, 100, f, 0, 8, 0, True, False, 0, None, out) == E                # the carry is written: samples arrive
    assert call(p.at(0), p.stride, 1, 0, f, 0, 8, 0, True, True, 0, None, out) == E                   # the carry is read: continued
    assert call(p.at(0), p.stride, 1, 100, f, 0, 8, 0, True, False, 0, carry, None) == E              # columns close
    assert call(p.at(0), p.stride, 1, 0, f, 0, 8, 3, True, True, 0, carry, None) == E                 # the flushed carry is a column
    for off in (1, 2, 3):                                                                             # 4, 8 and 12 bytes off a 16-byte boundary
        assert call(p.at(0), p.stride, 1, 100, f, 0, 8, 0, True, False, 0, carry[off:], out) == E     # a carry that is not aligned to 16 bytes
        assert call(p.at(0), p.stride, 1, 100, f, 0, 8, 0, True, False, 0, carry, out[off:]) == E     # nor the output
    torch.cuda.synchronize()
    assert (_host(out) == POISON).all() and (_host(carry) == POISON).all() and p.unchanged()
    # nothing closes: d_records may be NULL; nothing arrives and nothing is flushed: SGZ_OK, nothing launched, everything may be NULL
    assert call(p.at(0), p.stride, 1, 5, f, 0, 8, 0, False, False, 0, carry, None) == api.SGZ_OK
    assert call(p.at(0), p.stride, 1, 0, f, 0, 8, 0, True, False, 0, None, None) == api.SGZ_OK
    out2 = _dev(np.full(2 * WORDS, POISON, np.uint32))
    carry2 = _dev(np.full(cwords, POISON, np.uint32))
    assert call(p.at(0), p.stride, 1, 0, f, 0, 8, 3, False, True, 0, carry2, out2) == api.SGZ_OK
    torch.cuda.synchronize()
    assert (_host(out2) == POISON).all() and (_host(carry2) == POISON).all() and (_host(out) == POISON).all()
    after = _host(carry)[:cwords]
    assert _same(after[None, :], br.carry_of(f, br.records_of(x[:, :5], f, 8)[0][0], br.history_after(x[:, :5], f)))
    assert (_host(carry)[cwords:] == POISON).all()
