"""sgz_stage_level_columns on the GPU (csrc/level_columns.hip): byte for byte, no tolerance, against tests/level_ref.py.

Every call goes through `stage`, which poisons everything around what the call may write -- the padding between the channel rows, a record
in front of the output and the records behind its last column, a record in front of and behind the carry, the carry itself where it is not
written -- and checks it afterwards.  The sizes follow the code through api.level_columns_limits(): the switch-over between the tile form
and the sliced form, and the tile's samples."""
import gc
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import level_ref as lr  # noqa: E402
import wave_ref as wr  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = np.uint32(0xDEADBEEF)
WORDS = lr.DTYPE.itemsize // 4                                         # a record as 20 words
E = api.SGZ_EINVAL
_limits = {}


def limits():
    if not _limits:
        _limits["v"] = api.level_columns_limits()
    return _limits["v"]


def _dev(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _records(words, *shape):
    return np.ascontiguousarray(words, np.uint32).view(lr.DTYPE).reshape(*shape)


def _same(a, b):
    if a is None or b is None:                                         # (no carry: nothing stays open)
        return a is b
    return a.shape == b.shape and np.ascontiguousarray(a, lr.DTYPE).tobytes() == np.ascontiguousarray(b, lr.DTYPE).tobytes()


def content(kind, channels, S, m, seed):
    return lr.saturated(channels, S, seed) if kind == "saturated" else wr.content(kind, channels, S, m, seed)


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
            flat[offset + d * self.stride:offset + d * self.stride + self.S] = wr.bits_of(x[d])
        self.before = flat
        self.t = _dev(flat)
        assert self.t.data_ptr() % 16 == 0

    def at(self, sample):
        return self.t[self.offset + sample:]

    def unchanged(self):
        return np.array_equal(_host(self.t), self.before)


def stage(p, at, n, m, held=0, flush=True, slices=0, carry=None, extra=3, stream=None):
    """the call on samples [at, at + n) of p with the open column's carry records [pairs] (or None) -> (records [columns][pairs], carry
    afterwards or None); asserts SGZ_OK, the counts, and that nothing but the documented bytes changed"""
    import torch
    pairs = p.pairs
    columns, left = api.overview_step(m, held, n, flush)
    level = _dev(np.full((1 + columns + extra) * pairs * WORDS, POISON, np.uint32))
    carry_before = np.full((1 + pairs + 1) * WORDS, POISON, np.uint32)
    if carry is not None:
        carry_before[WORDS:(1 + pairs) * WORDS] = np.ascontiguousarray(carry, lr.DTYPE).reshape(-1).view(np.uint32)
    c = _dev(carry_before)
    st = api.stage_level_columns(p.at(at), p.stride, pairs, n, m, held, flush, slices, c[WORDS:], level[pairs * WORDS:], stream=stream)
    assert st == api.SGZ_OK, (st, api.lib().sgz_last_error())
    torch.cuda.synchronize()                                           # (the call's stream need not be torch's current one)
    got, carry_after = _host(level), _host(c)
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
    carry_in = lr.records_of(x[:, :held], m)[0][0] if held else None
    every, _ = lr.records_of(x, m)                                     # (flushed: the open column is the last one)
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


def _ns(m):
    tile = limits()[1]
    return sorted({0, 1, max(m - 1, 0), m, m + 1, tile - 1, tile, tile + 1, 3 * tile + 5})


KINDS = ("random", "constant", "saturated", "ramp")


@pytest.mark.parametrize("m", [1, 2, 3, 7, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, "above"])
def test_records_equal_the_definition(gpu, m):
    switch, tile = limits()
    assert switch == 1024                                               # the sweep brackets the switch-over: 1023 / 1024 / 1025
    m = 3 * tile + 6 if m == "above" else m                             # above every nsamples of the sweep
    i = 0
    for n in _ns(m) + [m // 2 if m > 2 else 0]:                         # (the last: m above nsamples, beside n = 1 and m - 1)
        for held in sorted({0, 1 % m, m - 1}):
            for flush in (True, False):
                pairs, offset, pad = (1, 2, 5)[i % 3], i % 4, (0, 1, 7, 64)[(i // 3) % 4]
                kind = KINDS[(i // 2) % 4]
                x = content(kind, 2 * pairs, held + n, m, seed=1000 * m + i)
                check(x, m, held, flush, offset=offset, pad=pad, what=(m, n, held, flush, pairs, offset, pad, kind))
                i += 1


def test_every_pair_count_base_offset_and_row_alignment(gpu):
    switch, tile = limits()
    for m in (3, 64, switch, switch + 1):
        for pairs in (1, 2, 5):
            for offset in range(4):
                for n, pad in ((tile + 1, 3), (3 * tile + 5, 4)):       # the rows of a pair 16-byte-aligned alike (stride % 4 == 0) and not
                    pad += (-(1 + n + pad)) % 4 if pad == 4 else 0
                    x = content(KINDS[(pairs + offset) % 4], 2 * pairs, 1 + n, m, seed=m + 10 * pairs + offset)
                    check(x, m, 1 % m, False, offset=offset, pad=pad, what=(m, pairs, offset, n, pad))


def test_a_long_stream_on_one_pair(gpu):
    switch, tile = limits()
    n = 2**20 + 3
    x = wr.content("random", 2, n, 4096, seed=3)
    p = Planar(x, offset=1, pad=2)
    for m in (1, 7, switch, switch + 1, 4096, n + 1):
        want, _ = lr.records_of(x, m)
        got, carry = stage(p, 0, n, m)
        assert carry is None and _same(got, want), m
    got, carry = stage(p, 0, n, n + 1, flush=False)
    assert got.shape[0] == 0 and _same(carry, lr.records_of(x, n + 1)[0][0])
    # saturated: a 1024-sample column reaches 2^62, the one long column carries into the high words
    x = lr.saturated(2, n, 5)
    p = Planar(x, offset=3, pad=1)
    for m in (switch, n + 1):
        want, _ = lr.records_of(x, m)
        got, carry = stage(p, 0, n, m)
        assert carry is None and _same(got, want), m
    assert int(want["sumsq"][0, 0, 0, 1]) == (n << 52) >> 64 > 0 and {int(v) for v in lr.records_of(x, switch)[0]["sumsq"][:-1, 0, :, 0].reshape(-1)} == {1 << 62}
    crosses = [lr.unpack(r)["cross"] for r in lr.records_of(x, switch)[0][:, 0]]
    assert min(crosses) == -(1 << 62) and max(crosses) == 1 << 62       # the cross term at both ends


def test_a_chain_of_calls_equals_the_single_call(gpu):
    switch, tile = limits()
    rng = np.random.default_rng(9)
    for m in (1, 5, 64, 257, switch, switch + 1, 3000):
        for pairs in (1, 2, 5):
            S = 2 * tile + 77 + int(rng.integers(0, 3 * m))
            x = content(KINDS[(m + pairs) % 4], 2 * pairs, S, m, seed=m + pairs)
            p = Planar(x, offset=int(rng.integers(0, 4)), pad=int(rng.integers(0, 9)))
            single, none = stage(p, 0, S, m)
            assert none is None and _same(single, lr.records_of(x, m)[0]), (m, pairs)
            cuts = sorted(set(int(v) for v in rng.integers(0, S + 1, size=9)) | {1, S})
            parts, at, held, carry = [], 0, 0, None
            for k, cut in enumerate([0] + cuts):                        # (the first call is empty; two cuts may coincide: another empty call)
                last = cut == S
                got, carry = stage(p, at, cut - at, m, held, flush=last, carry=carry)
                parts.append(got)
                held, at = (0 if last else (held + cut - at) % m), cut
            assert carry is None and _same(np.concatenate(parts), single), (m, pairs, cuts)
            # the flush alone, on the carry of everything but a column's end
            if S % m:
                body, carry = stage(p, 0, S, m, flush=False)
                tail, none = stage(p, S, 0, m, held=S % m, flush=True, carry=carry)
                assert none is None and _same(np.concatenate([body, tail]), single), (m, pairs)


def test_forced_slices_give_the_same_bytes(gpu):
    switch, tile = limits()
    for m, n in ((3, 1000), (64, tile + 9), (switch + 1, 3 * tile + 5), (5000, 40001), (50000, 40001)):
        for pairs, pad in ((1, 1), (5, 2)):
            x = content(("random", "saturated")[pairs == 5], 2 * pairs, 2 + n, m, seed=m)
            auto, carry0 = check(x, m, 2 % m, False, slices=0, offset=3, pad=pad, what=(m, n, pairs))
            for slices in (1, 2, 7, 64):
                got, carry = check(x, m, 2 % m, False, slices=slices, offset=3, pad=pad, what=(m, n, pairs, slices))
                assert _same(got, auto) and _same(carry, carry0)


def test_refusals_write_nothing(gpu):
    import torch
    x = wr.content("plain", 2, 100, 8, seed=1)
    p = Planar(x, pad=4)
    level = _dev(np.full(64 * WORDS, POISON, np.uint32))
    carry = _dev(np.full(2 * WORDS, POISON, np.uint32))
    call = api.stage_level_columns
    assert call(None, p.stride, 1, 100, 8, 0, True, 0, carry, level) == E                     # a null d_planar
    assert call(p.at(0), p.stride, 0, 100, 8, 0, True, 0, carry, level) == E                  # pairs 0
    assert call(p.at(0), p.stride, 33, 100, 8, 0, True, 0, carry, level) == E                 # pairs above 32
    assert call(p.at(0), p.stride, 1, 100, 0, 0, True, 0, carry, level) == E                  # m == 0
    assert call(p.at(0), p.stride, 1, 100, 8, 8, True, 0, carry, level) == E                  # held >= m
    assert call(p.at(0), 99, 1, 100, 8, 0, True, 0, carry, level) == E                        # channel_stride < nsamples
    assert call(p.at(0), p.stride, 1, 100, 8, 0, True, 65, carry, level) == E                 # slices > 64
    assert call(p.at(0), p.stride, 1, 100, 8, 3, True, 0, None, level) == E                   # the carry is read: held > 0
    assert call(p.at(0), p.stride, 1, 100, 8, 0, False, 0, None, level) == E                  # the carry is written: 100 % 8 samples stay open
    assert call(p.at(0), p.stride, 1, 100, 8, 0, True, 0, carry, None) == E                   # columns close
    assert call(p.at(0), p.stride, 1, 0, 8, 3, True, 0, carry, None) == E                     # the flushed carry is a column
    for off in (1, 2, 3):                                                                     # 4, 8 and 12 bytes off a 16-byte boundary
        assert call(p.at(0), p.stride, 1, 100, 8, 3, True, 0, carry[off:], level) == E        # a carry that is not aligned to 16 bytes
        assert call(p.at(0), p.stride, 1, 100, 8, 0, True, 0, carry, level[off:]) == E        # nor the output
    torch.cuda.synchronize()
    assert (_host(level) == POISON).all() and (_host(carry) == POISON).all() and p.unchanged()
    # what needs neither: allowed with NULL
    assert call(p.at(0), p.stride, 1, 96, 8, 0, False, 0, None, level) == api.SGZ_OK         # nothing held, nothing left open
    assert call(p.at(0), p.stride, 1, 5, 8, 0, False, 0, carry, None) == api.SGZ_OK          # nothing closes
    # nothing arrives and nothing is flushed: SGZ_OK, nothing launched
    level2 = _dev(np.full(2 * WORDS, POISON, np.uint32))
    carry2 = _dev(np.full(WORDS, POISON, np.uint32))
    assert call(p.at(0), p.stride, 1, 0, 8, 0, True, 0, None, None) == api.SGZ_OK
    assert call(p.at(0), p.stride, 1, 0, 8, 3, False, 0, carry2, level2) == api.SGZ_OK
    torch.cuda.synchronize()
    assert (_host(level2) == POISON).all() and (_host(carry2) == POISON).all()
    assert _same(_records(_host(level)[:12 * WORDS], 12, 1), lr.records_of(x[:, :96], 8)[0])
    assert _same(_records(_host(carry)[:WORDS], 1), lr.records_of(x[:, :5], 8)[0][0])


def test_a_launch_beside_work_on_a_second_stream(gpu):
    import torch
    switch, tile = limits()
    side, mine = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=gpu)
    cases = []
    for m in (7, switch + 1):
        x = wr.content("random", 4, 3 * tile + 5, m, seed=m)
        cases.append((m, Planar(x, offset=1, pad=3), lr.records_of(x, m)[0]))
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
    x = wr.content("plain", 2, 2 * tile + 3, 64, seed=2)
    want = {m: lr.records_of(x, m)[0] for m in (64, switch + 1)}

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
