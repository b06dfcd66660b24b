"""sgz_stage_loudness_columns on the GPU (csrc/loudness_columns.hip): byte for byte, no tolerance, against tests/loudness_ref.py.

Every call goes through `stage`, which poisons everything around what the call may write -- the padding between the channel rows, a record
in front of the output and the records behind its last column, words in front of and behind the carry -- and checks it afterwards; a call
with samples must write the whole carry (the open column or zeros, the history, the zero word), a call without must leave it alone.  The
sizes follow the code through api.loudness_columns_limits() and the filter's own W and L."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness_ref as lr  # noqa: E402
import wave_ref as wr  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = np.uint32(0xDEADBEEF)
WORDS = lr.DTYPE.itemsize // 4
E = api.SGZ_EINVAL
_filters = {}


def filt(which):
    if which not in _filters:
        _filters[which] = api.loudness_filter(lr.TINY.b, lr.TINY.a, lr.TINY.W, lr.TINY.L) if which == "tiny" else api.loudness_filter_for_rate(which)
    return _filters[which]


def limits(f, channels=1):
    return api.loudness_columns_limits(f, channels)


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
    """the call on samples [at, at + n) of p with the carry (uint32 words [channels][8 + W + L], or None: poison) -> (records
    [columns][channels], the carry afterwards or None where the call must not write it); asserts SGZ_OK, the counts, and that nothing but
    the documented bytes changed"""
    import torch
    channels = p.channels
    cwords = lr.carry_bytes(f) // 4
    columns, left = api.overview_step(m, held, n, flush)
    out = _dev(np.full((1 + columns + extra) * channels * WORDS, POISON, np.uint32))
    carry_before = np.full(4 + channels * cwords + 4, POISON, np.uint32)
    if carry is not None:
        carry_before[4:4 + channels * cwords] = np.ascontiguousarray(carry, np.uint32).reshape(-1)
    c = _dev(carry_before)
    st = api.stage_loudness_columns(p.at(at), p.stride, channels, n, f, first_index, m, held, flush, continued, slices, c[4:], out[channels * WORDS:],
                                    stream=stream)
    assert st == api.SGZ_OK, (st, api.lib().sgz_last_error())
    torch.cuda.synchronize()
    got, carry_after = _host(out), _host(c)
    first, last = channels * WORDS, (1 + columns) * channels * WORDS
    assert (got[:first] == POISON).all() and (got[last:] == POISON).all(), "bytes in front of the output or behind the last column were written"
    assert p.unchanged(), "the source or its padding was written"
    records = np.ascontiguousarray(got[first:last]).view(lr.DTYPE).reshape(columns, channels)
    assert not records["reserved"].any()
    if n:
        assert (carry_after[:4] == POISON).all() and (carry_after[4 + channels * cwords:] == POISON).all()
        after = np.ascontiguousarray(carry_after[4:4 + channels * cwords]).reshape(channels, cwords)
        assert not after[:, -1].any(), "the word behind the history is written as 0"
        if not left:
            assert not after[:, :8].any(), "no sample stays open: the open column is written as zeros"
        return records, after
    assert np.array_equal(carry_after, carry_before), "the carry was written by a call without samples"
    return records, None


def expect(x, f, m, held, flush, history, base):
    """x [channels][held + n]: the stream behind `history` (int [channels][any] or None), its first sample at index `base`; the call takes the
    last n -> (carry in or None, records, carry out or None)"""
    channels, n = x.shape[0], x.shape[1] - held
    carry_in = None
    if history is not None:
        open_ = np.zeros(channels, lr.DTYPE)
        if held:
            open_ = lr.records_of(x[:, :held], f, m, True, history, base)[0][0]
        else:
            open_["sumsq"], open_["count"], open_["reserved"] = 0xABABABABABABABAB, 0xABABABAB, 0xABABABAB       # read iff held > 0
        carry_in = lr.carry_of(f, open_, lr.history_after(x[:, :held], f, history))
        carry_in[:, -1] = 0xFFFFFFFF                                                                           # (never read)
    every, _ = lr.records_of(x, f, m, True, history, base)
    open_ = (not flush) and (held + n) % m != 0
    carry_out = None
    if n:
        carry_out = lr.carry_of(f, every[-1] if open_ else np.zeros(channels, lr.DTYPE), lr.history_after(x, f, history))
    return carry_in, (every[:-1] if open_ else every), carry_out


def check(x, f, m, held, flush, slices=0, offset=0, pad=0, history=None, base=0, what=None):
    n = x.shape[1] - held
    carry_in, want, carry_out = expect(x, f, m, held, flush, history, base)
    p = Planar(x, offset, pad)
    got, carry = stage(p, held, n, f, base + held, m, held, flush, history is not None, slices, carry_in)
    assert _same(got, want), what
    assert (carry is None) == (carry_out is None) and (carry is None or _same(carry, carry_out)), what
    return got, carry


def random_history(f, channels, seed):
    rng = np.random.default_rng(seed)
    h = rng.integers(-lr.CLAMP, lr.CLAMP + 1, size=(channels, lr.hist_len(f)))
    h[:, seed % h.shape[1]] = (lr.CLAMP, -lr.CLAMP)[seed % 2]
    return h


def _ns(f):
    W, L = f.W, f.L
    tile = limits(f)[1]
    return sorted({0, 1, L - 1, L, L + 1, W - 1, W, W + 1, 3 * W + 5, tile - 1, tile, tile + 1, 2 * tile + 1})


def _ms(f, n):
    switch = limits(f)[0]
    return sorted({1, 7, f.L, f.L + 1, 1000, switch - 1, switch, switch + 1, 4096, n + 3})


def test_limits(gpu):
    for which, tile in (("tiny", 4096), (8000, 4096), (48000, 4096), (192000, 4096)):
        f = filt(which)
        for channels in (1, 3, 64):
            switch, t, carry = limits(f, channels)
            assert (switch, t, carry) == (1024, tile, channels * lr.carry_bytes(f))
    big = api.loudness_filter(lr.TINY.b, lr.TINY.a, 16384, 16384)
    assert limits(big)[1] == 16384
    L = api.lib()
    import ctypes as C
    assert L.sgz_loudness_columns_limits(C.byref(api.loudness_filter(lr.TINY.b, lr.TINY.a, 32768, 64)), 1, None, None, None) == E     # W above what the LDS takes
    assert L.sgz_loudness_columns_limits(C.byref(api.loudness_filter(lr.TINY.b, lr.TINY.a, 64, 24)), 1, None, None, None) == E
    assert L.sgz_loudness_columns_limits(C.byref(filt("tiny")), 65, None, None, None) == E
    assert L.sgz_loudness_columns_limits(None, 1, None, None, None) == E


@pytest.mark.parametrize("which", ["tiny", 8000])
@pytest.mark.parametrize("ni", range(13))
def test_records_equal_the_definition(gpu, which, ni):
    f = filt(which)
    n = _ns(f)[ni]
    i = 7 * ni
    for m in _ms(f, n):
        held = (0, 1 % m, m - 1)[i % 3]
        flush = bool(i % 2)
        channels, offset, pad = (1, 2, 3)[i % 3], i % 4, (0, 1, 7, 64)[(i // 3) % 4]
        kind = KINDS[(i // 2) % len(KINDS)]
        base = (0, 1, f.L - 1, f.L, 5 * f.L + 3, 2 ** 40 + 5)[i % 6]
        x = content(kind, channels, held + n, m, seed=1000 * m + i)
        history = random_history(f, channels, i) if held or (i // 6) % 2 else None
        check(x, f, m, held, flush, offset=offset, pad=pad, history=history, base=base, what=(which, n, m, held, flush, channels, offset, pad, kind, base, history is not None))
        i += 1


def test_one_case_at_48_kHz(gpu):
    f = filt(48000)
    tile = limits(f)[1]
    x = content("sine", 2, 3 + 2 * tile + f.L + 1, 4800, seed=48)
    check(x, f, 4800, 3, False, offset=1, pad=3, history=random_history(f, 2, 1), base=f.L - 2)
    x = content("random", 1, f.W + 1, 7, seed=49)
    check(x, f, 7, 0, True, offset=3, pad=1)


def test_a_long_segment_is_a_tile_of_its_own(gpu):
    """L = W = 8192: one segment per tile, every lane on the one dot product"""
    f = api.loudness_filter(lr.TINY.b, lr.TINY.a, 8192, 8192)
    x = content("sine", 1, 2 * 8192 + 5, 1000, seed=5)
    check(x, f, 1000, 0, True, offset=1, base=8000)


def test_channel_counts_strides_and_base_offsets(gpu):
    for which in ("tiny", 8000):
        f = filt(which)
        tile = limits(f)[1]
        for channels in (1, 2, 3, 64):
            n = (tile + 1, f.W + f.L + 1)[channels == 64]
            for offset in ((0, 1, 2, 3) if channels < 64 else (1,)):
                m, pad = ((7, 3), (1025, 0), (f.L, 1))[(channels + offset) % 3]
                x = content(KINDS[(channels + offset) % len(KINDS)], channels, 1 + n, m, seed=m + 10 * channels + offset)
                check(x, f, m, 1 % m, False, offset=offset, pad=pad, history=random_history(f, channels, offset), base=3 * f.L + offset,
                      what=(which, channels, offset, m, pad))


def test_forced_slices_give_the_same_bytes(gpu):
    for which, m, n in (("tiny", 3, 1000), ("tiny", 1025, 3 * 4096 + 5), (8000, 64, 4096 + 9), (8000, 5000, 20001), (8000, 50000, 20001)):
        f = filt(which)
        for channels, pad in ((1, 1), (3, 2)):
            x = content(("random", "loud")[channels == 3], channels, 2 + n, m, seed=m)
            history = random_history(f, channels, m)
            auto, carry0 = check(x, f, m, 2 % m, False, slices=0, offset=3, pad=pad, history=history, base=17, what=(which, m, n, channels))
            for slices in (1, 2, 7, 64):
                got, carry = check(x, f, m, 2 % m, False, slices=slices, offset=3, pad=pad, history=history, base=17, what=(which, m, n, channels, slices))
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
            assert np.array_equal(after[:, 8:-1].view(np.int32), lr.history_after(x[:, :cut], f)), cut
        held, at = (0 if last else (held + cut - at) % m), cut
    return np.concatenate(parts), carry


def test_every_cut_of_a_short_stream(gpu):
    f = filt("tiny")
    S = 2 * f.W + 3
    x = content("random", 2, S, 7, seed=11)
    p = Planar(x, offset=1, pad=3)
    for m, base in ((7, 5), (40, 0)):
        want, _ = lr.records_of(x, f, m, True, None, base)
        single, _ = stage(p, 0, S, f, base, m)
        assert _same(single, want)
        for cut in range(S + 1):
            got, _ = chain(p, x, f, m, [cut, S], base)
            assert _same(got, want), (m, cut)


def test_two_and_three_cuts_around_L_and_W(gpu):
    f = filt(8000)
    W, L = f.W, f.L
    S = 2 * W + 3 * L + 5
    x = content("sine", 2, S, 100, seed=12)
    x[:, 50] = np.nan
    p = Planar(x, offset=3, pad=1)
    for m in (100, 1500):                                            # (held > 0 at every cut: no cut below is a multiple of either)
        want, _ = lr.records_of(x, f, m, True, None, 3)
        for cuts in ([L - 1, L + 1], [L, W + 1], [1, W - 1], [W - 1, W], [W + L - 1, W + L + 1], [L - 1, L, L + 1], [1, W, W + L + 7], [W + 1, 2 * W - 1, 2 * W + L]):
            got, _ = chain(p, x, f, m, cuts + [S], 3)
            assert _same(got, want), (m, cuts)


def test_one_sample_calls(gpu):
    f = filt("tiny")
    x = content("random", 2, 70, 7, seed=4)
    p = Planar(x, offset=1, pad=3)
    for m in (1, 7, 13):
        want, _ = lr.records_of(x, f, m, True, None, 9)
        got, _ = chain(p, x, f, m, list(range(1, 71)), 9)
        assert _same(got, want), m


def test_a_flush_does_not_move_the_segment_grid(gpu):
    for which in ("tiny", 8000):
        f = filt(which)
        S, n1 = 3 * f.W + 11, f.W + f.L // 2 + 3                        # the flush falls inside a segment
        x = content("sine", 2, S, 50, seed=13)
        p = Planar(x, pad=2)
        m = 50
        head, _ = lr.records_of(x[:, :n1], f, m, True)
        tail, _ = lr.records_of(x[:, n1:], f, m, True, lr.quantise(x[:, :n1])[0], n1)
        # the flush with the samples, then more samples
        a, carry = stage(p, 0, n1, f, 0, m, flush=True)
        b, _ = stage(p, n1, S - n1, f, n1, m, flush=True, continued=True, carry=carry)
        assert _same(a, head) and _same(b, tail), which
        # the flush alone (nsamples == 0), on the carry of a call that left the column open: the carry stays, and so does the history
        a0, carry = stage(p, 0, n1, f, 0, m, flush=False)
        a1, none = stage(p, n1, 0, f, n1, m, held=n1 % m, flush=True, continued=True, carry=carry)
        assert none is None and _same(np.concatenate([a0, a1]), head), which
        b, _ = stage(p, n1, S - n1, f, n1, m, flush=True, continued=True, carry=carry)
        assert _same(b, tail), which


def test_special_values(gpu):
    f = filt(8000)
    tile = limits(f)[1]
    for m in (1, 64, 1025):
        for kind in ("random", "constant", "ramp", "loud"):
            x = content(kind, 2, tile + 3 * m + 1, m, seed=m)
            got, _ = check(x, f, m, 0, True, offset=2, pad=3, what=(m, kind))
            if kind == "random":
                assert (got["count"] < np.minimum(m, x.shape[1])).any()     # some NaNs were not counted
    x = np.full((2, 300), np.nan, np.float32)
    got, _ = check(x, filt("tiny"), 10, 0, True)
    assert got.tobytes() == bytes(got.nbytes)
    d = np.full((1, 200), 1e-40, np.float32)                            # denormals quantise to 0
    got, _ = check(d, filt("tiny"), 50, 0, True)
    assert not got["sumsq"].any() and (got["count"] == 50).all()


def test_the_worst_case_reaches_the_accumulator_bound(gpu):
    """|v| = 2^26 with the sign of C[2][k] at v[j L - 1 - k]: the 64-bit sum of component t1 reaches its bound, far above 2^53, where the
    conversion to fp64 rounds"""
    f = filt(8000)
    C = lr.taps(f)
    W, L = f.W, f.L
    bound = int(np.abs(C[2]).sum()) << 26
    assert 2 ** 53 < bound < 2 ** 62
    j = W // L + 3
    S = (j + 2) * L + 5
    rng = np.random.default_rng(3)
    x = loud(1, S, 3)
    k = np.arange(W)
    x[0, j * L - 1 - k] = np.where(C[2] < 0, np.float32(-100.0), np.float32(np.inf))
    v, _ = lr.quantise(x)
    assert int((C[2] * v[0, j * L - 1 - k]).sum()) == bound
    # the bound itself is a multiple of 2^26 and converts exactly; three odd samples on the same side make the sum one that has to be rounded
    x[0, j * L - 1 - np.array([5, 6, 7])] = (np.sign(C[2][5:8]) * 12345677 / 2.0 ** 23).astype(np.float32)
    v, _ = lr.quantise(x)
    total = int((C[2] * v[0, j * L - 1 - k]).sum())
    assert 2 ** 58 < total < bound and int(float(total)) != total
    for m, slices in ((1, 0), (L, 0), (1025, 0), (L, 7)):
        check(x, f, m, 0, True, slices=slices, offset=int(rng.integers(0, 4)), what=(m, slices))
    # and the same segment start met through the history of a second call
    p = Planar(x, offset=1)
    want, _ = lr.records_of(x, f, L + 1, True)
    got, _ = chain(p, x, f, L + 1, [j * L, S])
    assert _same(got, want)
    got, _ = chain(p, x, f, L + 1, [j * L + 1, S])
    assert _same(got, want)


def test_refusals_write_nothing(gpu):
    import torch
    f = filt("tiny")
    x = wr.content("plain", 1, 100, 8, seed=1)
    p = Planar(x, pad=4)
    cwords = lr.carry_bytes(f) // 4
    out = _dev(np.full(64 * WORDS, POISON, np.uint32))
    carry = _dev(np.full(2 * cwords, POISON, np.uint32))
    call = api.stage_loudness_columns
    bad_taps = api.loudness_filter([[0.0, 0.6, 0.0], [1.0, 0.0, 0.0]], [[0.0, 0.0], [0.0, 0.0]], 64, 16)
    #                  planar stride ch n   f  first m held flush continued slices
    assert call(None, p.stride, 1, 100, f, 0, 8, 0, True, False, 0, carry, out) == E                  # a null d_planar
    assert call(p.at(0), p.stride, 1, 100, None, 0, 8, 0, True, False, 0, carry, out) == E            # a null filter
    assert call(p.at(0), p.stride, 1, 100, bad_taps, 0, 8, 0, True, False, 0, carry, out) == E        # a filter whose table is refused
    assert call(p.at(0), p.stride, 1, 100, api.loudness_filter(lr.TINY.b, lr.TINY.a, 96, 16), 0, 8, 0, True, False, 0, carry, out) == E
    assert call(p.at(0), p.stride, 1, 100, api.loudness_filter(lr.TINY.b, lr.TINY.a, 32768, 2048), 0, 8, 0, True, False, 0, carry, out) == E
    assert call(p.at(0), p.stride, 0, 100, f, 0, 8, 0, True, False, 0, carry, out) == E               # channels 0
    assert call(p.at(0), p.stride, 65, 100, f, 0, 8, 0, True, False, 0, carry, out) == E              # channels above 64
    assert call(p.at(0), p.stride, 1, 100, f, 0, 0, 0, True, False, 0, carry, out) == E               # m == 0
    assert call(p.at(0), p.stride, 1, 100, f, 0, 8, 8, True, True, 0, carry, out) == E                # held >= m
    assert call(p.at(0), p.stride, 1, 100, f, 0, 8, 3, True, False, 0, carry, out) == E               # held > 0 where the stream begins
    assert call(p.at(0), 99, 1, 100, f, 0, 8, 0, True, False, 0, carry, out) == E                     # channel_stride < nsamples
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
    assert _same(after[None, :], lr.carry_of(f, lr.records_of(x[:, :5], f, 8)[0][0], lr.history_after(x[:, :5], f)))
    assert (_host(carry)[cwords:] == POISON).all()


def test_a_launch_beside_work_on_a_second_stream(gpu):
    import torch
    f = filt(8000)
    tile = limits(f)[1]
    side, mine = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=gpu)
    cases = []
    for m in (7, 1025):
        x = wr.content("random", 3, 3 * tile + 5, m, seed=m)
        cases.append((m, Planar(x, offset=1, pad=3), lr.records_of(x, f, m)[0]))
    torch.cuda.synchronize()
    for rounds in range(3):
        with torch.cuda.stream(side):
            for _ in range(20):
                a = torch.tanh(a @ a * 1e-3)
        for m, p, want in cases:
            got, _ = stage(p, 0, p.S, f, 0, m, stream=mine.cuda_stream)
            assert _same(got, want), (rounds, m)
    torch.cuda.synchronize()
