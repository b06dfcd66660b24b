"""sgz_stage_hist_columns on the GPU (csrc/hist_columns.hip): byte for byte, no tolerance, against tests/hist_ref.py.

Every call goes through `stage`, which poisons everything around what the call may write -- the padding between the channel rows, a record
in front of the output and the records behind its last column, a record in front of and behind the carry, the carry itself where it is not
written -- and checks it afterwards.  The sizes follow the code through api.hist_columns_limits(): the switch-over between the tile form and
the sliced form, and the tile's samples; TABLES is the header's number of LDS tables of a tile ("min(4096 / m, 64) whole columns").  A
stream here is a tile and 1237 samples: a partial last tile, and for every m of the sweep a partial last column."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hist_ref as hr  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = np.uint32(0xDEADBEEF)
WORDS = hr.DTYPE.itemsize // 4                                         # a record as 112 words
E = api.SGZ_EINVAL
TABLES = 64
SIGNALS = ("noise", "silence", "two_level", "s16", "positive", "ramp", "edges", "corners")
_limits, _signals = {}, {}


def limits():
    if not _limits:
        _limits["v"] = api.hist_columns_limits()
    return _limits["v"]


def S_of():
    return limits()[1] + 1237


def _dev(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _records(words, *shape):
    return np.ascontiguousarray(words, np.uint32).view(hr.DTYPE).reshape(*shape)


def _same(a, b):
    if a is None or b is None:                                         # (no carry: nothing stays open)
        return a is b
    return a.shape == b.shape and np.ascontiguousarray(a, hr.DTYPE).tobytes() == np.ascontiguousarray(b, hr.DTYPE).tobytes()


def _row(kind, d, S):
    if kind == "noise":
        return hr.noise(S, seed=20 + d)
    if kind == "silence":
        return hr.silence(S, seed=d)
    if kind == "two_level":                                             # in alternation, and 48 / 16 of every wave either way round
        return hr.two_level(S, ((1, 1), (48, 16), (16, 48))[d % 3])
    if kind == "s16":
        return hr.s16(S, seed=30 + d)
    if kind == "positive":
        return hr.positive(S, seed=40 + d)
    if kind == "ramp":
        return np.roll(hr.ramp(S), d)
    if kind == "edges":
        return np.roll(hr.edge_values(S), 3 * d)
    return hr.corners(S, seed=50 + d)


def signal(kind, channels, S=None):
    """float32 [channels][S]; every channel a variation of the same kind -- once per (kind, channels, S)"""
    S = S_of() if S is None else S
    if (kind, channels, S) not in _signals:
        _signals[kind, channels, S] = np.stack([_row(kind, d, S) for d in range(channels)])
    return _signals[kind, channels, S]


class Planar:
    """x float32 [channels][S] on the device: rows `stride` = S + pad apart (an odd pad: neighbouring rows differ in alignment), the first one
    `offset` floats behind a 16-byte boundary, poison in front, between and behind"""

    def __init__(self, x, offset=0, pad=0):
        self.channels, self.S = x.shape
        self.stride = self.S + pad
        self.offset = offset
        flat = np.full(4 + self.channels * self.stride + 8, POISON, np.uint32)
        for d in range(self.channels):
            flat[offset + d * self.stride:offset + d * self.stride + self.S] = np.ascontiguousarray(x[d], np.float32).view(np.uint32)
        self.before = flat
        self.t = _dev(flat)
        assert self.t.data_ptr() % 16 == 0

    def at(self, sample):
        return self.t[self.offset + sample:]

    def unchanged(self):
        return np.array_equal(_host(self.t), self.before)


def stage(p, at, n, m, held=0, flush=True, slices=0, carry=None, extra=2, stream=None):
    """the call on samples [at, at + n) of p with the open column's carry records [channels] (or None) -> (records [columns][channels], carry
    afterwards or None); asserts SGZ_OK, the counts, and that nothing but the documented bytes changed"""
    import torch
    channels = p.channels
    columns, left = api.overview_step(m, held, n, flush)
    hist = _dev(np.full((1 + columns + extra) * channels * WORDS, POISON, np.uint32))
    carry_before = np.full((1 + channels + 1) * WORDS, POISON, np.uint32)
    if carry is not None:
        carry_before[WORDS:(1 + channels) * WORDS] = np.ascontiguousarray(carry, hr.DTYPE).reshape(-1).view(np.uint32)
    c = _dev(carry_before)
    st = api.stage_hist_columns(p.at(at), p.stride, channels, n, m, held, flush, slices, c[WORDS:], hist[channels * WORDS:], stream=stream)
    assert st == api.SGZ_OK, (st, api.lib().sgz_last_error())
    torch.cuda.synchronize()                                           # (the call's stream need not be torch's current one)
    got, carry_after = _host(hist), _host(c)
    first, last = channels * WORDS, (1 + columns) * channels * WORDS
    assert (got[:first] == POISON).all() and (got[last:] == POISON).all(), "bytes in front of the output or behind the last column were written"
    assert p.unchanged(), "the source or its padding was written"
    records = _records(got[first:last], columns, channels)
    assert (records["bucket"].sum(axis=-1, dtype=np.uint64) == records["count"]).all(), "count is the sum of the buckets in every record"
    if left:
        assert (carry_after[:WORDS] == POISON).all() and (carry_after[(1 + channels) * WORDS:] == POISON).all()
        return records, _records(carry_after[WORDS:(1 + channels) * WORDS], channels)
    assert np.array_equal(carry_after, carry_before), "the carry was written though nothing stays open"
    return records, None


def expect(x, m, held, flush):
    """x [channels][held + n]: the stream so far, of which the call takes the last n -> (carry in or None, records, carry out or None)"""
    carry_in = hr.columns(x[:, :held], m, flush=False)[1] if held else None
    want, carry_out = hr.columns(x[:, held:], m, held=held, flush=flush, carry=carry_in)
    return carry_in, want, carry_out


_whole = {}


def whole(kind, channels, m):
    """the flushed records of the whole stream -- once per (kind, channels, m)"""
    if (kind, channels, m) not in _whole:
        _whole[kind, channels, m] = hr.columns(signal(kind, channels), m)[0]
    return _whole[kind, channels, m]


def check(x, m, held, flush, slices=0, offset=0, pad=0, what=None):
    carry_in, want, carry_out = expect(x, m, held, flush)
    p = Planar(x, offset, pad)
    got, carry = stage(p, held, x.shape[1] - held, m, held, flush, slices, carry_in)
    assert _same(got, want), what
    assert (carry is None) == (carry_out is None) and (carry is None or _same(carry, carry_out)), what
    return got, carry


def _m_of(m):
    switch, tile = limits()
    most = max(k for k in range(1, tile) if tile // k > TABLES)        # the largest m with more columns in a full row than tables
    return {"tables": most, "tables+1": most + 1, "switch": switch, "over": switch + 1, "above": S_of() + 7}.get(m, m)


@pytest.mark.parametrize("m", [1, 7, "tables", "tables+1", 64, 1000, "switch", "over", "above"])
def test_records_equal_the_definition(gpu, m):
    m = _m_of(m)
    S = S_of()
    assert m == 1 or S % m != 0                                         # a partial flushed column
    i = 0
    for kind in SIGNALS:
        for held, flush in ((0, True), (1 % m, False), (min(m - 1, 1000), True)):     # (the first `held` samples are the earlier calls')
            channels, offset, pad = (1, 2, 3)[i % 3], i % 4, (1, 0, 7, 64)[(i // 2) % 4]
            check(signal(kind, channels), m, held, flush, offset=offset, pad=pad, what=(m, kind, held, flush, channels, offset, pad))
            i += 1
    # fewer samples than a column, one sample, none
    x = signal("corners", 1)
    for n in sorted({0, 1, max(m - 1, 0), m, m + 1}):
        if n <= S - 1:
            check(x[:, :1 % m + n], m, 1 % m, True, offset=3, pad=5, what=(m, n))
            check(x[:, :n], m, 0, False, offset=1, pad=2, what=(m, n))


def test_every_signal_is_what_it_says(gpu):
    """on the CPU: noise fills some 49 buckets, the fullest about a tenth; silence sits in bucket 0 alone; two_level in two buckets; ramp holds
    every reachable bucket in one column; s16 has no bit below 2^-15; positive no negative sample -- and the device gives those records"""
    S = S_of()
    got, _ = check(signal("noise", 1), S, 0, True)
    share = got[0, 0]["bucket"] / S
    assert 45 <= int((share > 0).sum()) <= 53 and 0.08 <= share.max() <= 0.12, ((share > 0).sum(), share.max())
    got, _ = check(signal("silence", 1), 256, 0, True)
    assert int(got["bucket"][:, :, 0].sum()) == S and int(got["bucket"][:, :, 1:].sum()) == 0 and not got["negative"].any() and not got["bits_or"].any()
    got, _ = check(signal("two_level", 3), 256, 0, True)
    assert {int(b) for b in np.nonzero(got["bucket"].sum(axis=(0, 1)))[0]} == {int(hr.bucket_of(1 << 21)), int(hr.bucket_of(1 << 13))}
    got, _ = check(signal("ramp", 1), S, 0, True)
    assert [int(b) for b in np.nonzero(got[0, 0]["bucket"])[0]] == hr.reachable() and 0 < got[0, 0]["negative"] < got[0, 0]["count"]
    got, _ = check(signal("edges", 1), S, 0, True)
    assert [int(b) for b in np.nonzero(got[0, 0]["bucket"])[0]] == hr.reachable() and int(got[0, 0]["peak"]) == 1 << 26
    got, _ = check(signal("s16", 1), 1000, 0, True)
    assert all(api.hist_readout(r)["effective_bits"] == 16 for r in got[:, 0])
    got, _ = check(signal("positive", 1), 1000, 0, True)
    assert not got["negative"].any() and (got["bits_or"] >> 27 == 0).all()
    got, _ = check(signal("corners", 1), 1000, 0, True)
    assert int(got["skipped"].sum()) > 1000 and (got[:, 0]["skipped"] == 1000).any()      # a column of NaNs alone: the identity beside `skipped`
    lone = got[:, 0][got[:, 0]["skipped"] == 1000][0]
    assert int(lone["count"]) == 0 and int(lone["bits_and"]) == 0xFFFFFFFF and int(lone["bits_or"]) == 0


def test_channels_every_base_offset_and_row_alignment(gpu):
    switch, tile = limits()
    S = S_of()
    for m in (3, 64, switch, switch + 1):
        for channels in (1, 3, 64):
            for offset in range(4):
                if channels == 64 and (offset not in (1, 2) or m == 3):  # (the widest case twice per m, and not a record per three samples)
                    continue
                pad = (3, 4)[offset % 2]                                # odd strides: neighbouring rows differ in alignment; and rows aligned alike
                pad += (-(S + pad)) % 4 if pad == 4 else 0
                x = signal(SIGNALS[(channels + offset) % len(SIGNALS)], channels)
                check(x, m, 1 % m, False, offset=offset, pad=pad, what=(m, channels, offset, pad))


def test_a_chain_of_calls_equals_the_single_call(gpu):
    switch, tile = limits()
    rng = np.random.default_rng(9)
    S = S_of()
    for m in (1, 5, 64, 257, switch, switch + 1, 3000):
        for channels in (1, 2):
            kind = ("corners", "silence")[channels - 1]
            x = signal(kind, channels)
            p = Planar(x, offset=int(rng.integers(0, 4)), pad=int(rng.integers(0, 9)))
            single, none = stage(p, 0, S, m)
            assert none is None and _same(single, whole(kind, channels, m)), (m, channels)
            # random cuts, the tile's end and either side of it, a first and a last call of one sample
            cuts = sorted(set(int(v) for v in rng.integers(0, S + 1, size=5)) | {1, tile - 1, tile, tile + 1, S - 1, S})
            parts, at, held, carry = [], 0, 0, None
            for cut in [0] + cuts:                                      # (the first call is empty)
                last = cut == S
                got, carry = stage(p, at, cut - at, m, held, flush=last, carry=carry)
                parts.append(got)
                held, at = (0 if last else (held + cut - at) % m), cut
            assert carry is None and _same(np.concatenate(parts), single), (m, channels, cuts)
            # nsamples = 0 with flush: the flush alone, on the carry of everything but a column's end
            if S % m:
                body, carry = stage(p, 0, S, m, flush=False)
                tail, none = stage(p, S, 0, m, held=S % m, flush=True, carry=carry)
                assert none is None and _same(np.concatenate([body, tail]), single), (m, channels)


def test_forced_slices_give_the_same_bytes(gpu):
    switch, tile = limits()
    S = S_of()
    for m, n in ((3, 1000), (64, tile + 9), (switch + 1, S - 2), (5000, S - 2), (50000, S - 2)):
        for channels, kind in ((1, "corners"), (2, "two_level"), (1, "silence")):
            x = signal(kind, channels)[:, :2 + n]
            auto, carry0 = check(x, m, 2 % m, False, slices=0, offset=3, pad=channels, what=(m, n, channels))
            for slices in (1, 2, 3, 64):
                got, carry = check(x, m, 2 % m, False, slices=slices, offset=3, pad=channels, what=(m, n, channels, slices))
                assert _same(got, auto) and _same(carry, carry0)


def test_refusals_write_nothing(gpu):
    import torch
    x = signal("noise", 1)[:, :100]
    p = Planar(x, pad=4)
    hist = _dev(np.full(16 * WORDS, POISON, np.uint32))
    carry = _dev(np.full(2 * WORDS, POISON, np.uint32))
    call = api.stage_hist_columns
    assert call(None, p.stride, 1, 100, 8, 0, True, 0, carry, hist) == E                      # a null d_planar
    assert call(p.at(0), p.stride, 0, 100, 8, 0, True, 0, carry, hist) == E                   # channels 0
    assert call(p.at(0), p.stride, 65, 100, 8, 0, True, 0, carry, hist) == E                  # channels above 64
    assert call(p.at(0), p.stride, 1, 100, 0, 0, True, 0, carry, hist) == E                   # m == 0
    assert call(p.at(0), p.stride, 1, 100, 8, 8, True, 0, carry, hist) == E                   # held >= m
    assert call(p.at(0), 99, 1, 100, 8, 0, True, 0, carry, hist) == E                         # channel_stride < nsamples
    assert call(p.at(0), p.stride, 1, 100, 8, 0, True, 65, carry, hist) == E                  # slices > 64
    assert call(p.at(0), p.stride, 1, 100, 8, 3, True, 0, None, hist) == E                    # the carry is read: held > 0
    assert call(p.at(0), p.stride, 1, 100, 8, 0, False, 0, None, hist) == E                   # the carry is written: 100 % 8 samples stay open
    assert call(p.at(0), p.stride, 1, 100, 8, 0, True, 0, carry, None) == E                   # columns close
    assert call(p.at(0), p.stride, 1, 0, 8, 3, True, 0, carry, None) == E                     # the flushed carry is a column
    for off in (1, 2, 3):                                                                     # 4, 8 and 12 bytes off a 16-byte boundary
        assert call(p.at(0), p.stride, 1, 100, 8, 3, True, 0, carry[off:], hist) == E         # a carry that is not aligned to 16 bytes
        assert call(p.at(0), p.stride, 1, 100, 8, 0, True, 0, carry, hist[off:]) == E         # nor the output
    torch.cuda.synchronize()
    assert (_host(hist) == POISON).all() and (_host(carry) == POISON).all() and p.unchanged()
    # what needs neither: allowed with NULL
    assert call(p.at(0), p.stride, 1, 96, 8, 0, False, 0, None, hist) == api.SGZ_OK          # nothing held, nothing left open
    assert call(p.at(0), p.stride, 1, 5, 8, 0, False, 0, carry, None) == api.SGZ_OK          # nothing closes
    # nothing arrives and nothing is flushed: SGZ_OK, nothing launched
    hist2 = _dev(np.full(2 * WORDS, POISON, np.uint32))
    carry2 = _dev(np.full(WORDS, POISON, np.uint32))
    assert call(p.at(0), p.stride, 1, 0, 8, 0, True, 0, None, None) == api.SGZ_OK
    assert call(p.at(0), p.stride, 1, 0, 8, 3, False, 0, carry2, hist2) == api.SGZ_OK
    torch.cuda.synchronize()
    assert (_host(hist2) == POISON).all() and (_host(carry2) == POISON).all()
    assert _same(_records(_host(hist)[:12 * WORDS], 12, 1), hr.columns(x[:, :96], 8)[0])
    assert _same(_records(_host(carry)[:WORDS], 1), hr.columns(x[:, :5], 8, flush=False)[1])


def test_a_launch_beside_work_on_a_second_stream(gpu):
    import torch
    switch, tile = limits()
    side, mine = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=gpu)
    cases = []
    for m in (7, switch + 1):
        cases.append((m, Planar(signal("corners", 2), offset=1, pad=3), whole("corners", 2, m)))
    torch.cuda.synchronize()
    for rounds in range(3):
        with torch.cuda.stream(side):
            for _ in range(20):
                a = torch.tanh(a @ a * 1e-3)
        for m, p, want in cases:
            got, _ = stage(p, 0, p.S, m, stream=mine.cuda_stream)
            assert _same(got, want), (rounds, m)
    torch.cuda.synchronize()
