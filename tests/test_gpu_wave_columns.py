"""sgz_stage_wave_columns on the GPU (csrc/wave_columns.hip): bit for bit (uint32 views), no tolerance, against tests/wave_ref.py.

Every call goes through `stage`, which poisons everything around what the call may write -- the padding between the channel rows, the
output behind the last column, the carry where it is not written -- and checks it afterwards.  The sizes follow the code through
api.wave_columns_limits(): the switch-over between the tile form and the sliced form, and the tile's samples."""
import gc
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wave_ref as wr  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = np.uint32(0xDEADBEEF)
E = api.SGZ_EINVAL
_limits = {}


def limits():
    if not _limits:
        _limits["v"] = api.wave_columns_limits()
    return _limits["v"]


def _dev(bits):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


class Planar:
    """x float32 [channels][S] on the device: rows `stride` = S + pad apart, the first one `offset` floats behind a 16-byte boundary, poison
    in front, between and behind"""

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


def stage(p, at, n, m, held=0, flush=True, slices=0, carry=None, extra=3, stream=None):
    """the call on samples [at, at + n) of p with the open column's carry bits [channels][2] (or None) -> (wave bits [columns][channels][2],
    carry bits afterwards or None); asserts SGZ_OK, the counts, and that nothing but the documented bytes changed"""
    import torch
    ch = p.channels
    columns, left = api.overview_step(m, held, n, flush)
    wave = _dev(np.full((columns + extra) * ch * 2, POISON, np.uint32))
    carry_before = np.full(ch * 2 + 2, POISON, np.uint32)
    if carry is not None:
        carry_before[:ch * 2] = np.asarray(carry, np.uint32).reshape(-1)
    c = _dev(carry_before)
    st = api.stage_wave_columns(p.at(at), p.stride, ch, n, m, held, flush, slices, c, wave, stream=stream)
    assert st == api.SGZ_OK, (st, api.lib().sgz_last_error())
    torch.cuda.synchronize()                                           # (the call's stream need not be torch's current one)
    got, carry_after = _host(wave), _host(c)
    assert (got[columns * ch * 2:] == POISON).all(), "bytes behind the last column were written"
    assert p.unchanged(), "the source or its padding was written"
    if left:
        assert (carry_after[ch * 2:] == POISON).all()
        return got[:columns * ch * 2].reshape(columns, ch, 2), carry_after[:ch * 2].reshape(ch, 2)
    assert np.array_equal(carry_after, carry_before), "the carry was written though nothing stays open"
    return got[:columns * ch * 2].reshape(columns, ch, 2), None


def expect(x, m, held, n, flush):
    """x [channels][held + n]: the stream so far, of which the call takes the last n -> (carry in or None, columns, carry out or None)"""
    carry_in = wr.columns_of(x[:, :held], m)[0][0] if held else None
    every, _ = wr.columns_of(x, m)                                     # (flushed: the open column is the last one)
    open_ = (not flush) and (held + n) % m != 0
    return carry_in, (every[:-1] if open_ else every), (every[-1] if open_ else None)


def check(x, m, held, flush, slices=0, offset=0, pad=0, what=None):
    n = x.shape[1] - held
    carry_in, want, carry_out = expect(x, m, held, n, flush)
    p = Planar(x, offset, pad)
    got, carry = stage(p, held, n, m, held, flush, slices, carry_in)
    assert np.array_equal(got, want), what
    assert (carry is None) == (carry_out is None) and (carry is None or np.array_equal(carry, carry_out)), what
    return got, carry


def _ms():
    switch, tile = limits()
    return sorted({1, 2, 3, 7, 63, 64, 65, 255, 256, 257, switch - 1, switch, switch + 1})


def _ns(m):
    tile = limits()[1]
    return sorted({0, 1, max(m - 1, 0), m, m + 1, tile - 1, tile, tile + 1, 3 * tile + 5})


@pytest.mark.parametrize("m", [1, 2, 3, 7, 63, 64, 65, 255, 256, 257, "switch-1", "switch", "switch+1"])
def test_columns_equal_the_definition(gpu, m):
    switch, tile = limits()
    m = {"switch-1": switch - 1, "switch": switch, "switch+1": switch + 1}.get(m, m)
    assert m in _ms()
    i = 0
    for n in _ns(m) + [m // 2 if m > 2 else 0]:                         # (the last: m above nsamples, beside n = 1 and m - 1)
        for held in sorted({0, 1 % m, m - 1}):
            for flush in (True, False):
                channels, offset, pad = (1, 2, 5)[i % 3], i % 4, (0, 1, 7, 64)[(i // 3) % 4]
                kind = ("random", "constant", "ramp")[(i // 2) % 3]
                x = wr.content(kind, channels, held + n, m, seed=1000 * m + i)
                check(x, m, held, flush, offset=offset, pad=pad, what=(m, n, held, flush, channels, offset, pad, kind))
                i += 1


def test_every_channel_count_and_base_offset(gpu):
    switch, tile = limits()
    for m in (3, 64, switch, switch + 1):
        for channels in (1, 2, 5):
            for offset in range(4):
                for n in (tile + 1, 3 * tile + 5):
                    x = wr.content("random", channels, 1 + n, m, seed=m + 10 * channels + offset)
                    check(x, m, 1 % m, False, offset=offset, pad=3, what=(m, channels, offset, n))


def test_a_long_stream_on_one_channel(gpu):
    switch, tile = limits()
    n = 2**20 + 3
    x = wr.content("random", 1, n, 4096, seed=3)
    p = Planar(x, offset=1, pad=2)
    for m in (1, 7, switch, switch + 1, 4096, n + 1):
        want, _ = wr.columns_of(x, m)
        got, carry = stage(p, 0, n, m)
        assert carry is None and np.array_equal(got, want), m
    got, carry = stage(p, 0, n, n + 1, flush=False)
    assert got.shape[0] == 0 and np.array_equal(carry, wr.columns_of(x, n + 1)[0][0])


def test_a_chain_of_calls_equals_the_single_call(gpu):
    switch, tile = limits()
    rng = np.random.default_rng(9)
    for m in (1, 5, 64, 257, switch, switch + 1, 3000):
        for channels in (1, 2, 5):
            S = 2 * tile + 77 + int(rng.integers(0, 3 * m))
            x = wr.content("random", channels, S, m, seed=m + channels)
            p = Planar(x, offset=int(rng.integers(0, 4)), pad=int(rng.integers(0, 9)))
            single, none = stage(p, 0, S, m)
            assert none is None and np.array_equal(single, wr.columns_of(x, m)[0]), (m, channels)
            cuts = sorted(set(int(v) for v in rng.integers(0, S + 1, size=9)) | {1, S})
            parts, at, held, carry = [], 0, 0, None
            for k, cut in enumerate([0] + cuts):                        # (the first call is empty; two cuts may coincide: another empty call)
                last = cut == S
                got, carry = stage(p, at, cut - at, m, held, flush=last, carry=carry)
                parts.append(got)
                held, at = (0 if last else (held + cut - at) % m), cut
            assert carry is None and np.array_equal(np.concatenate(parts), single), (m, channels, cuts)
            # the flush alone, on the carry of everything but a column's end
            if S % m:
                body, carry = stage(p, 0, S, m, flush=False)
                tail, none = stage(p, S, 0, m, held=S % m, flush=True, carry=carry)
                assert none is None and np.array_equal(np.concatenate([body, tail]), single), (m, channels)


def test_forced_slices_give_the_same_bits(gpu):
    switch, tile = limits()
    for m, n in ((3, 1000), (64, tile + 9), (switch + 1, 3 * tile + 5), (5000, 40001), (50000, 40001)):
        for channels in (1, 5):
            x = wr.content("random", channels, 2 + n, m, seed=m)
            auto, carry0 = check(x, m, 2 % m, False, slices=0, offset=3, pad=1, what=(m, n, channels))
            for slices in (1, 2, 7, 64):
                got, carry = check(x, m, 2 % m, False, slices=slices, offset=3, pad=1, what=(m, n, channels, slices))
                assert np.array_equal(got, auto) and np.array_equal(carry, carry0)


def test_refusals_write_nothing(gpu):
    import torch
    x = wr.content("plain", 2, 100, 8, seed=1)
    p = Planar(x, pad=4)
    wave = _dev(np.full(64 * 2 * 2, POISON, np.uint32))
    carry = _dev(np.full(2 * 2, POISON, np.uint32))
    call = api.stage_wave_columns
    assert call(None, p.stride, 2, 100, 8, 0, True, 0, carry, wave) == E                      # a null d_planar
    assert call(p.at(0), p.stride, 0, 100, 8, 0, True, 0, carry, wave) == E                   # channels 0
    assert call(p.at(0), p.stride, 65, 100, 8, 0, True, 0, carry, wave) == E                  # channels above 64
    assert call(p.at(0), p.stride, 2, 100, 0, 0, True, 0, carry, wave) == E                   # m == 0
    assert call(p.at(0), p.stride, 2, 100, 8, 8, True, 0, carry, wave) == E                   # held >= m
    assert call(p.at(0), 99, 2, 100, 8, 0, True, 0, carry, wave) == E                         # channel_stride < nsamples
    assert call(p.at(0), p.stride, 2, 100, 8, 0, True, 65, carry, wave) == E                  # slices > 64
    assert call(p.at(0), p.stride, 2, 100, 8, 3, True, 0, None, wave) == E                    # the carry is read: held > 0
    assert call(p.at(0), p.stride, 2, 100, 8, 0, False, 0, None, wave) == E                   # the carry is written: 100 % 8 samples stay open
    assert call(p.at(0), p.stride, 2, 100, 8, 0, True, 0, carry, None) == E                   # columns close
    assert call(p.at(0), p.stride, 2, 0, 8, 3, True, 0, carry, None) == E                     # the flushed carry is a column
    assert call(p.at(0), p.stride, 2, 100, 8, 3, True, 0, carry[1:], wave) == E               # a carry that is not aligned to float2
    assert call(p.at(0), p.stride, 2, 100, 8, 0, True, 0, carry, wave[1:]) == E               # nor the output
    torch.cuda.synchronize()
    assert (_host(wave) == POISON).all() and (_host(carry) == POISON).all() and p.unchanged()
    # what needs neither: allowed with NULL
    assert call(p.at(0), p.stride, 2, 96, 8, 0, False, 0, None, wave) == api.SGZ_OK          # nothing held, nothing left open
    assert call(p.at(0), p.stride, 2, 5, 8, 0, False, 0, carry, None) == api.SGZ_OK          # nothing closes
    # nothing arrives and nothing is flushed: SGZ_OK, nothing launched
    wave2 = _dev(np.full(8, POISON, np.uint32))
    carry2 = _dev(np.full(4, POISON, np.uint32))
    assert call(p.at(0), p.stride, 2, 0, 8, 0, True, 0, None, None) == api.SGZ_OK
    assert call(p.at(0), p.stride, 2, 0, 8, 3, False, 0, carry2, wave2) == api.SGZ_OK
    torch.cuda.synchronize()
    assert (_host(wave2) == POISON).all() and (_host(carry2) == POISON).all()
    assert np.array_equal(_host(wave)[:12 * 2 * 2].reshape(12, 2, 2), wr.columns_of(x[:, :96], 8)[0])


def test_a_launch_beside_work_on_a_second_stream(gpu):
    import torch
    switch, tile = limits()
    side, mine = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=gpu)
    cases = []
    for m in (7, switch + 1):
        x = wr.content("random", 2, 3 * tile + 5, m, seed=m)
        cases.append((m, Planar(x, offset=1, pad=3), wr.columns_of(x, m)[0]))
    torch.cuda.synchronize()
    for rounds in range(5):
        with torch.cuda.stream(side):
            for _ in range(20):
                a = torch.tanh(a @ a * 1e-3)
        for m, p, want in cases:
            got, _ = stage(p, 0, p.S, m, stream=mine.cuda_stream)
            assert np.array_equal(got, want), (rounds, m)
    torch.cuda.synchronize()


def test_200_cycles_give_the_memory_back(gpu):
    import torch
    switch, tile = limits()
    x = wr.content("plain", 2, 2 * tile + 3, 64, seed=2)
    want = {m: wr.columns_of(x, m)[0] for m in (64, switch + 1)}

    def cycle(i):
        m = (64, switch + 1)[i % 2]
        s = torch.cuda.Stream()
        p = Planar(x, offset=i % 4)
        got, _ = stage(p, 0, p.S, m, slices=(0, 7)[(i // 2) % 2], stream=s.cuda_stream)
        assert np.array_equal(got, want[m]), i

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
        assert free0 - free1 < 64 << 20, f"device memory: {(free0 - free1) / 2**20:.1f} MiB fewer free after 200 cycles"
