"""sgz_stage_field_columns on the GPU (csrc/field_columns.hip): byte for byte, no tolerance, against tests/field_ref.py.

Every call goes through `stage`, which poisons everything around what the call may write -- the padding between the channel rows, a record
in front of the output and the records behind its last column, a record in front of and behind the carry, the carry itself where it is not
written -- and checks it afterwards.  The sizes follow the code through api.field_columns_limits(): the switch-over between the tile form
and the sliced form, and the tile's sample frames.  A stream here is a tile and 1237 frames: a partial last tile, and for every m of the
sweep a partial last column."""
import gc
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = np.uint32(0xDEADBEEF)
WORDS = fr.DTYPE.itemsize // 4                                         # a record as 132 words
E = api.SGZ_EINVAL
SIGNALS = ("noise", "mono", "left", "antiphase", "mixed")
_limits, _signals = {}, {}


def limits():
    if not _limits:
        _limits["v"] = api.field_columns_limits()
    return _limits["v"]


def S_of():
    return limits()[1] + 1237


def _dev(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _records(words, *shape):
    return np.ascontiguousarray(words, np.uint32).view(fr.DTYPE).reshape(*shape)


def _same(a, b):
    if a is None or b is None:                                         # (no carry: nothing stays open)
        return a is b
    return a.shape == b.shape and np.ascontiguousarray(a, fr.DTYPE).tobytes() == np.ascontiguousarray(b, fr.DTYPE).tobytes()


def _specials(S):
    """float32 [2][S] of noise with the boundary-hugging frames (all 32 boundaries, j < 8, both sides) and the corner frames embedded"""
    x = fr.correlated(S, seed=11)
    at = 5
    for k in range(32):
        for j in range(8):
            for vl, vr in fr.hugging(k, j):
                x[0, at], x[1, at] = vl * 2.0**-23, vr * 2.0**-23
                at += 7                                                # (512 frames, 7 apart: the first 3600 samples)
    nan, inf, tiny = np.float32(np.nan), np.float32(np.inf), np.array([1], np.uint32).view(np.float32)[0]
    corners = [(inf, inf), (inf, -inf), (-inf, 0.0), (nan, 0.5), (0.5, nan), (nan, nan), (0.0, 0.0), (-0.0, 0.0), (tiny, -tiny), (100.0, 4.0),
               (-9.0, 8.5), (1.0, 0.0), (0.0, 1.0), (0.5, 0.5), (0.5, -0.5), (tiny, 2.0**-23)]
    for i, (l, r) in enumerate(corners * 4):
        x[0, S - 1 - 13 * i], x[1, S - 1 - 13 * i] = l, r             # from the last frame backwards
    x[:, 3700:3764] = 0.0                                              # a run of silence, and one of NaNs: whole short columns of either
    x[:, 3800:3864] = nan
    return x


def signal(kind, pairs, S=None):
    """float32 [2 pairs][S]; every pair a variation of the same kind -- once per (kind, pairs, S)"""
    S = S_of() if S is None else S
    if (kind, pairs, S) not in _signals:
        rows = []
        for p in range(pairs):
            if kind == "mixed":
                pair = _specials(S) if p % 2 == 0 else fr.correlated(S, seed=40 + p)
            else:
                pair = fr.correlated(S, seed=20 + p)
                if kind == "mono":
                    pair[1] = pair[0]                                   # every frame in sector 16 (or silent)
                elif kind == "left":
                    pair[1] = 0.0
                elif kind == "antiphase":
                    pair[1] = -pair[0]
            rows.append(pair)
        _signals[kind, pairs, S] = np.concatenate(rows)
    return _signals[kind, pairs, S]


class Planar:
    """x float32 [channels][S] on the device: rows `stride` = S + pad apart (an odd pad: the rows of a pair differ in alignment), the first one
    `offset` floats behind a 16-byte boundary, poison in front, between and behind"""

    def __init__(self, x, offset=0, pad=0):
        self.channels, self.S = x.shape
        self.pairs = self.channels // 2
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
    """the call on samples [at, at + n) of p with the open column's carry records [pairs] (or None) -> (records [columns][pairs], carry
    afterwards or None); asserts SGZ_OK, the counts, and that nothing but the documented bytes changed"""
    import torch
    pairs = p.pairs
    columns, left = api.overview_step(m, held, n, flush)
    field = _dev(np.full((1 + columns + extra) * pairs * WORDS, POISON, np.uint32))
    carry_before = np.full((1 + pairs + 1) * WORDS, POISON, np.uint32)
    if carry is not None:
        carry_before[WORDS:(1 + pairs) * WORDS] = np.ascontiguousarray(carry, fr.DTYPE).reshape(-1).view(np.uint32)
    c = _dev(carry_before)
    st = api.stage_field_columns(p.at(at), p.stride, pairs, n, m, held, flush, slices, c[WORDS:], field[pairs * WORDS:], stream=stream)
    assert st == api.SGZ_OK, (st, api.lib().sgz_last_error())
    torch.cuda.synchronize()                                           # (the call's stream need not be torch's current one)
    got, carry_after = _host(field), _host(c)
    first, last = pairs * WORDS, (1 + columns) * pairs * WORDS
    assert (got[:first] == POISON).all() and (got[last:] == POISON).all(), "bytes in front of the output or behind the last column were written"
    assert p.unchanged(), "the source or its padding was written"
    if left:
        assert (carry_after[:WORDS] == POISON).all() and (carry_after[(1 + pairs) * WORDS:] == POISON).all()
        return _records(got[first:last], columns, pairs), _records(carry_after[WORDS:(1 + pairs) * WORDS], pairs)
    assert np.array_equal(carry_after, carry_before), "the carry was written though nothing stays open"
    return _records(got[first:last], columns, pairs), None


def expect(x, m, held, n, flush):
    """x [channels][held + n]: the stream so far, of which the call takes the last n -> (carry in or None, records, carry out or None)"""
    carry_in = fr.columns(x[:, :held], m)[0][0] if held else None
    every, _ = fr.columns(x, m)                                        # (flushed: the open column is the last one)
    open_ = (not flush) and (held + n) % m != 0
    return carry_in, (every[:-1] if open_ else every), (every[-1] if open_ else None)


def check(x, m, held, flush, slices=0, offset=0, pad=0, what=None):
    n = x.shape[1] - held
    carry_in, want, carry_out = expect(x, m, held, n, flush)
    p = Planar(x, offset, pad)
    got, carry = stage(p, held, n, m, held, flush, slices, carry_in)
    assert _same(got, want), what
    assert (carry is None) == (carry_out is None) and (carry is None or _same(carry, carry_out)), what
    return got, carry


def _m_of(m):
    switch, tile = limits()
    return {"below": switch - 1, "switch": switch, "over": switch + 1, "above": S_of() + 7}.get(m, m)


@pytest.mark.parametrize("m", [1, 2, 3, 7, 63, 64, 65, 255, 256, 257, "below", "switch", "over", "above"])
def test_records_equal_the_definition(gpu, m):
    m = _m_of(m)
    S = S_of()
    assert m == 1 or S % m != 0                                         # a partial flushed column
    i = 0
    for kind in SIGNALS:
        for held in sorted({0, 1 % m, min(m - 1, 1000)}):               # (the first `held` samples are the earlier calls')
            for flush in (True, False):
                pairs, offset, pad = (1, 2, 1)[i % 3], i % 4, (1, 0, 7, 64)[(i // 2) % 4]
                x = signal(kind, pairs)
                check(x, m, held, flush, offset=offset, pad=pad, what=(m, kind, held, flush, pairs, offset, pad))
                i += 1
    # fewer samples than a column, one sample, none
    x = signal("mixed", 1)
    for n in sorted({0, 1, max(m - 1, 0), m, m + 1}):
        if n <= S - 1:
            check(x[:, :1 % m + n], m, 1 % m, True, offset=3, pad=5, what=(m, n))
            check(x[:, :n], m, 0, False, offset=1, pad=2, what=(m, n))


def test_every_signal_is_what_it_says(gpu):
    """the histograms of the four plain signals: the contended one (all-mono) sits in sector 16 alone"""
    for kind, sectors in (("mono", {16}), ("left", {8}), ("antiphase", {0})):
        x = signal(kind, 1)
        got, _ = check(x, 256, 0, True, what=kind)
        used = {int(b) for b in np.nonzero(got["count"].sum(axis=(0, 1)))[0]}
        assert used == sectors, (kind, used)
        assert int(got["count"].sum()) + int(got["silent"].sum()) == x.shape[1]
    got, _ = check(signal("noise", 1), 256, 0, True)
    assert len(np.nonzero(got["count"].sum(axis=(0, 1)))[0]) == 32


def test_32_pairs_every_base_offset_and_row_alignment(gpu):
    switch, tile = limits()
    S = S_of()
    for m in (3, 64, switch, switch + 1):
        for pairs in (1, 2, 32):
            for offset in range(4):
                if pairs == 32 and offset not in (1, 2):                # (the widest case twice per m)
                    continue
                pad = (3, 4)[offset % 2]                                # the rows of a pair 16-byte-aligned alike (stride % 4 == 0) and not
                pad += (-(S + pad)) % 4 if pad == 4 else 0
                x = signal(SIGNALS[(pairs + offset) % 5], pairs)
                check(x, m, 1 % m, False, offset=offset, pad=pad, what=(m, pairs, offset, pad))


def test_a_chain_of_calls_equals_the_single_call(gpu):
    switch, tile = limits()
    rng = np.random.default_rng(9)
    S = S_of()
    for m in (1, 5, 64, 257, switch, switch + 1, 3000):
        for pairs in (1, 2):
            x = signal(("mixed", "mono")[pairs - 1], pairs)
            p = Planar(x, offset=int(rng.integers(0, 4)), pad=int(rng.integers(0, 9)))
            single, none = stage(p, 0, S, m)
            assert none is None and _same(single, fr.columns(x, m)[0]), (m, pairs)
            cuts = sorted(set(int(v) for v in rng.integers(0, S + 1, size=7)) | {1, S - 1, S})      # a first and a last call of one sample
            parts, at, held, carry = [], 0, 0, None
            for cut in [0] + cuts:                                      # (the first call is empty; two cuts may coincide: another empty call)
                last = cut == S
                got, carry = stage(p, at, cut - at, m, held, flush=last, carry=carry)
                parts.append(got)
                held, at = (0 if last else (held + cut - at) % m), cut
            assert carry is None and _same(np.concatenate(parts), single), (m, pairs, cuts)
            # nsamples = 0 with flush: the flush alone, on the carry of everything but a column's end
            if S % m:
                body, carry = stage(p, 0, S, m, flush=False)
                tail, none = stage(p, S, 0, m, held=S % m, flush=True, carry=carry)
                assert none is None and _same(np.concatenate([body, tail]), single), (m, pairs)


def test_forced_slices_give_the_same_bytes(gpu):
    switch, tile = limits()
    S = S_of()
    for m, n in ((3, 1000), (64, tile + 9), (switch + 1, S - 2), (5000, S - 2), (50000, S - 2)):
        for pairs, kind in ((1, "mixed"), (2, "mono")):
            x = signal(kind, pairs)[:, :2 + n]
            auto, carry0 = check(x, m, 2 % m, False, slices=0, offset=3, pad=pairs, what=(m, n, pairs))
            for slices in (1, 2, 7, 64):
                got, carry = check(x, m, 2 % m, False, slices=slices, offset=3, pad=pairs, what=(m, n, pairs, slices))
                assert _same(got, auto) and _same(carry, carry0)


def test_refusals_write_nothing(gpu):
    import torch
    x = signal("noise", 1)[:, :100]
    p = Planar(x, pad=4)
    field = _dev(np.full(16 * WORDS, POISON, np.uint32))
    carry = _dev(np.full(2 * WORDS, POISON, np.uint32))
    call = api.stage_field_columns
    assert call(None, p.stride, 1, 100, 8, 0, True, 0, carry, field) == E                     # a null d_planar
    assert call(p.at(0), p.stride, 0, 100, 8, 0, True, 0, carry, field) == E                  # pairs 0
    assert call(p.at(0), p.stride, 33, 100, 8, 0, True, 0, carry, field) == E                 # pairs above 32
    assert call(p.at(0), p.stride, 1, 100, 0, 0, True, 0, carry, field) == E                  # m == 0
    assert call(p.at(0), p.stride, 1, 100, 8, 8, True, 0, carry, field) == E                  # held >= m
    assert call(p.at(0), 99, 1, 100, 8, 0, True, 0, carry, field) == E                        # channel_stride < nsamples
    assert call(p.at(0), p.stride, 1, 100, 8, 0, True, 65, carry, field) == E                 # slices > 64
    assert call(p.at(0), p.stride, 1, 100, 8, 3, True, 0, None, field) == E                   # the carry is read: held > 0
    assert call(p.at(0), p.stride, 1, 100, 8, 0, False, 0, None, field) == E                  # the carry is written: 100 % 8 samples stay open
    assert call(p.at(0), p.stride, 1, 100, 8, 0, True, 0, carry, None) == E                   # columns close
    assert call(p.at(0), p.stride, 1, 0, 8, 3, True, 0, carry, None) == E                     # the flushed carry is a column
    for off in (1, 2, 3):                                                                     # 4, 8 and 12 bytes off a 16-byte boundary
        assert call(p.at(0), p.stride, 1, 100, 8, 3, True, 0, carry[off:], field) == E        # a carry that is not aligned to 16 bytes
        assert call(p.at(0), p.stride, 1, 100, 8, 0, True, 0, carry, field[off:]) == E        # nor the output
    torch.cuda.synchronize()
    assert (_host(field) == POISON).all() and (_host(carry) == POISON).all() and p.unchanged()
    # what needs neither: allowed with NULL
    assert call(p.at(0), p.stride, 1, 96, 8, 0, False, 0, None, field) == api.SGZ_OK         # nothing held, nothing left open
    assert call(p.at(0), p.stride, 1, 5, 8, 0, False, 0, carry, None) == api.SGZ_OK          # nothing closes
    # nothing arrives and nothing is flushed: SGZ_OK, nothing launched
    field2 = _dev(np.full(2 * WORDS, POISON, np.uint32))
    carry2 = _dev(np.full(WORDS, POISON, np.uint32))
    assert call(p.at(0), p.stride, 1, 0, 8, 0, True, 0, None, None) == api.SGZ_OK
    assert call(p.at(0), p.stride, 1, 0, 8, 3, False, 0, carry2, field2) == api.SGZ_OK
    torch.cuda.synchronize()
    assert (_host(field2) == POISON).all() and (_host(carry2) == POISON).all()
    assert _same(_records(_host(field)[:12 * WORDS], 12, 1), fr.columns(x[:, :96], 8)[0])
    assert _same(_records(_host(carry)[:WORDS], 1), fr.columns(x[:, :5], 8)[0][0])


def test_a_launch_beside_work_on_a_second_stream(gpu):
    import torch
    switch, tile = limits()
    side, mine = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=gpu)
    cases = []
    for m in (7, switch + 1):
        x = signal("mixed", 2)
        cases.append((m, Planar(x, offset=1, pad=3), fr.columns(x, m)[0]))
    torch.cuda.synchronize()
    for rounds in range(5):
        with torch.cuda.stream(side):
            for _ in range(20):
                a = torch.tanh(a @ a * 1e-3)
        for m, p, want in cases:
            got, _ = stage(p, 0, p.S, m, stream=mine.cuda_stream)
            assert _same(got, want), (rounds, m)
    torch.cuda.synchronize()


def test_200_calls_give_the_memory_back(gpu):
    import torch
    switch, tile = limits()
    x = signal("noise", 1)
    want = {m: fr.columns(x, m)[0] for m in (64, switch + 1)}

    def cycle(i):
        m = (64, switch + 1)[i % 2]
        s = torch.cuda.Stream()
        p = Planar(x, offset=i % 4)
        got, _ = stage(p, 0, p.S, m, slices=(0, 7)[(i // 2) % 2], stream=s.cuda_stream)
        assert _same(got, want[m]), i

    for i in range(8):
        cycle(i)
    gc.collect()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for i in range(200):
        cycle(i)
    gc.collect()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    if "PYTEST_XDIST_WORKER" not in os.environ:                   # (the figure is the DEVICE's: under pytest -n the other workers' allocations move it)
        assert free0 - free1 < 64 << 20, f"device memory: {(free0 - free1) / 2**20:.1f} MiB fewer free after 200 calls"
