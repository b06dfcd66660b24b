"""sgz_stage_truepeak_columns on the GPU (csrc/truepeak_columns.hip): byte for byte, no tolerance, against tests/truepeak_ref.py.

Every call goes through `stage`, which poisons everything around what the call may write -- the padding between the channel rows, a record
in front of the output and the records behind its last column, a carry in front of and behind the carry -- and checks it afterwards; a call
with samples must write the whole carry (the open column or zeros, the history, reserved == 0), a call without must leave it alone.  The
sizes follow the code through api.truepeak_columns_limits(): the switch-over between the tile form and the sliced form, and the tile's
samples."""
import gc
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import truepeak_ref as tr  # noqa: E402
import wave_ref as wr  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = np.uint32(0xDEADBEEF)
WORDS, CWORDS = tr.DTYPE.itemsize // 4, tr.CARRY_DTYPE.itemsize // 4     # a record as 4 words, a carry as 16
E = api.SGZ_EINVAL
_limits = {}


def limits():
    if not _limits:
        _limits["v"] = api.truepeak_columns_limits()
    return _limits["v"]


def _dev(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _same(a, b, dtype=tr.DTYPE):
    return a.shape == b.shape and np.ascontiguousarray(a, dtype).tobytes() == np.ascontiguousarray(b, dtype).tobytes()


def content(kind, channels, S, m, seed):
    n = np.arange(S, dtype=np.float64)
    if kind == "saturated":
        return tr.saturated(channels, S, seed)
    if kind == "nyquist":                                               # alternating +-1.0
        return np.where(n % 2 == 0, 1.0, -1.0).astype(np.float32)[None, :].repeat(channels, axis=0).copy()
    if kind == "fs4":                                                   # the fs/4 sine at 45 degrees: sample peaks 0.707 A, true peak A
        return np.stack([((0.9 + 0.2 * d) * np.sin(0.5 * np.pi * n + 0.25 * np.pi)).astype(np.float32) for d in range(channels)])
    return wr.content(kind, channels, S, m, seed)


KINDS = ("random", "constant", "saturated", "ramp", "nyquist", "fs4")


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


def stage(p, at, n, m, held=0, flush=True, continued=False, slices=0, carry=None, extra=3, stream=None):
    """the call on samples [at, at + n) of p with the carry [channels] (or None: poison) -> (records [columns][channels], the carry afterwards
    or None where the call must not write it); asserts SGZ_OK, the counts, and that nothing but the documented bytes changed"""
    import torch
    channels = p.channels
    columns, left = api.overview_step(m, held, n, flush)
    peaks = _dev(np.full((1 + columns + extra) * channels * WORDS, POISON, np.uint32))
    carry_before = np.full((1 + channels + 1) * CWORDS, POISON, np.uint32)
    if carry is not None:
        carry_before[CWORDS:(1 + channels) * CWORDS] = np.ascontiguousarray(carry, tr.CARRY_DTYPE).reshape(-1).view(np.uint32)
    c = _dev(carry_before)
    st = api.stage_truepeak_columns(p.at(at), p.stride, channels, n, m, held, flush, continued, slices, c[CWORDS:], peaks[channels * WORDS:], stream=stream)
    assert st == api.SGZ_OK, (st, api.lib().sgz_last_error())
    torch.cuda.synchronize()
    got, carry_after = _host(peaks), _host(c)
    first, last = channels * WORDS, (1 + columns) * channels * WORDS
    assert (got[:first] == POISON).all() and (got[last:] == POISON).all(), "bytes in front of the output or behind the last column were written"
    assert p.unchanged(), "the source or its padding was written"
    records = np.ascontiguousarray(got[first:last]).view(tr.DTYPE).reshape(columns, channels)
    if n:
        assert (carry_after[:CWORDS] == POISON).all() and (carry_after[(1 + channels) * CWORDS:] == POISON).all()
        after = np.ascontiguousarray(carry_after[CWORDS:(1 + channels) * CWORDS]).view(tr.CARRY_DTYPE).reshape(channels)
        assert not after["reserved"].any()
        if not left:
            assert after["open"].tobytes() == bytes(16 * channels), "no sample stays open: the open column is written as zeros"
        return records, after
    assert np.array_equal(carry_after, carry_before), "the carry was written by a call without samples"
    return records, None


def expect(x, m, held, flush, history):
    """x [channels][held + n]: the stream behind `history` (int [channels][11] or None), of which the call takes the last n ->
    (carry in or None, records, carry out or None)"""
    channels, n = x.shape[0], x.shape[1] - held
    carry_in = None
    if history is not None:
        carry_in = np.zeros(channels, tr.CARRY_DTYPE)
        carry_in["hist"] = tr.history_after(x[:, :held], history)
        carry_in["reserved"] = 0xFFFFFFFF                               # (never read)
        if held:
            carry_in["open"] = tr.records_of(x[:, :held], m, True, history)[0][0]
        else:
            carry_in["open"] = (0xABABABABABABABAB, 0xABABABAB, 0xABABABAB)     # read iff held > 0
    every, _ = tr.records_of(x, m, True, history)
    open_ = (not flush) and (held + n) % m != 0
    carry_out = None
    if n:
        carry_out = np.zeros(channels, tr.CARRY_DTYPE)
        carry_out["hist"] = tr.history_after(x, history)
        if open_:
            carry_out["open"] = every[-1]
    return carry_in, (every[:-1] if open_ else every), carry_out


def check(x, m, held, flush, slices=0, offset=0, pad=0, history=None, what=None):
    n = x.shape[1] - held
    carry_in, want, carry_out = expect(x, m, held, flush, history)
    p = Planar(x, offset, pad)
    got, carry = stage(p, held, n, m, held, flush, history is not None, slices, carry_in)
    assert _same(got, want), what
    assert (carry is None) == (carry_out is None) and (carry is None or _same(carry, carry_out, tr.CARRY_DTYPE)), what
    return got, carry


def random_history(channels, seed):
    rng = np.random.default_rng(seed)
    h = rng.integers(-tr.CLAMP, tr.CLAMP + 1, size=(channels, 11))
    h[:, seed % 11] = (tr.CLAMP, -tr.CLAMP)[seed % 2]
    return h


def _ns(m):
    tile = limits()[1]
    return sorted({0, 1, 10, 11, 12, max(m - 1, 0), m, m + 1, tile - 1, tile, tile + 1, 3 * tile + 5})


@pytest.mark.parametrize("m", [1, 2, 3, 7, 11, 12, 13, 63, 64, 65, 255, 256, 257, "switch-1", "switch", "switch+1", "above"])
def test_records_equal_the_definition(gpu, m):
    switch, tile = limits()
    m = {"switch-1": switch - 1, "switch": switch, "switch+1": switch + 1, "above": 3 * tile + 6}.get(m, m)
    i = 0
    for n in _ns(m):
        for held in sorted({0, 1 % m, m - 1}):
            for flush in (True, False):
                channels, offset, pad = (1, 2, 5)[i % 3], i % 4, (0, 1, 7, 64)[(i // 3) % 4]
                kind = KINDS[(i // 2) % len(KINDS)]
                x = content(kind, channels, held + n, m, seed=1000 * m + i)
                history = random_history(channels, i) if held or (i // 6) % 2 else None
                check(x, m, held, flush, offset=offset, pad=pad, history=history, what=(m, n, held, flush, channels, offset, pad, kind, history is not None))
                i += 1


def test_every_channel_count_and_base_offset(gpu):
    switch, tile = limits()
    for m in (3, 64, switch, switch + 1):
        for channels in (1, 2, 5):
            for offset in range(4):
                n, pad = ((tile + 1, 3), (3 * tile + 5, 4))[(channels + offset) % 2]
                x = content(KINDS[(channels + offset) % len(KINDS)], channels, 1 + n, m, seed=m + 10 * channels + offset)
                check(x, m, 1 % m, False, offset=offset, pad=pad, history=random_history(channels, offset), what=(m, channels, offset, n, pad))


def test_a_long_stream_on_one_channel(gpu):
    switch, tile = limits()
    n = 2**20 + 3
    x = wr.content("random", 1, n, 4096, seed=3)
    p = Planar(x, offset=1, pad=2)
    for m in (1, 7, switch, switch + 1, n + 1):
        want, _ = tr.records_of(x, m)
        got, carry = stage(p, 0, n, m)
        assert _same(got, want) and np.array_equal(carry["hist"], tr.history_after(x)), m
    # nothing but +-inf and +-100: the bound 2^26 * 2073548 is reached, and every sample behind the first six is an over (phase 0)
    x = tr.saturated(1, 3 * tile + 5, 5)
    for m in (12, switch, switch + 1):
        got, _ = check(x, m, 0, True, offset=3, pad=1, what=m)
        assert int(got["peak"].max()) == 2**26 * 2073548 and int(got["overs"].sum()) >= x.shape[1] - 6


def test_impulses(gpu):
    """an impulse at every position mod 16 and at a tile's first and last sample: its 12 outputs cross lane runs, columns, tiles and slices"""
    switch, tile = limits()
    S = 2 * tile + 40
    for pos in list(range(16)) + [tile - 1, tile, 2 * tile - 1, 2 * tile, S - 1]:
        x = np.zeros((2, S), np.float32)
        x[0, pos], x[1, (pos + 5) % S] = 0.75, -1.0
        for m, slices in ((1, 0), (16, 0), (64, 0), (switch, 0), (switch + 1, 0), (64, 3)):
            check(x, m, 0, True, slices=slices, offset=pos % 4, pad=1, what=(pos, m, slices))


def test_specials_first_last_and_alone(gpu):
    switch, tile = limits()
    for m in (1, 5, 64, switch + 1):
        for kind in ("random", "constant", "ramp"):                    # wave_ref.content: NaN / +-inf / +-0 / denormals first, last, alone, all-NaN columns
            x = wr.content(kind, 2, tile + 3 * m + 1, m, seed=m)
            got, _ = check(x, m, 0, True, offset=2, pad=3, what=(m, kind))
        assert (got["count"] < np.minimum(m, x.shape[1])).any()         # some NaNs were not counted
    x = np.full((2, 100), np.nan, np.float32)
    got, _ = check(x, 10, 0, True)
    assert got.tobytes() == bytes(got.nbytes)


def test_a_chain_of_calls_equals_the_single_call(gpu):
    switch, tile = limits()
    rng = np.random.default_rng(9)
    for m in (1, 5, 12, 64, 257, switch, switch + 1, 3000):
        channels = (1, 2, 5)[m % 3]
        S = 2 * tile + 77 + int(rng.integers(0, 3 * m))
        x = content(KINDS[m % len(KINDS)], channels, S, m, seed=m + channels)
        p = Planar(x, offset=int(rng.integers(0, 4)), pad=int(rng.integers(0, 9)))
        single, carry = stage(p, 0, S, m)
        assert _same(single, tr.records_of(x, m)[0]), (m, channels)
        cuts = set(int(v) for v in rng.integers(0, S + 1, size=6)) | {S}
        at = int(rng.integers(0, S - 200))
        for step in range(1, 12):                                       # cuts of 1 .. 11 samples among them
            at += step
            cuts.add(at)
        cuts = sorted(cuts)
        parts, at, held, carry, continued = [], 0, 0, None, False
        for cut in [0] + cuts:                                          # (the first call is empty)
            last = cut == S
            got, after = stage(p, at, cut - at, m, held, flush=last, continued=continued, carry=carry)
            parts.append(got)
            if after is not None:
                carry, continued = after, True
                assert np.array_equal(carry["hist"], tr.history_after(x[:, :cut])), (m, cut)
            held, at = (0 if last else (held + cut - at) % m), cut
        assert _same(np.concatenate(parts), single), (m, channels, cuts)
        # the flush alone, on the carry of everything but a column's end: the history stays
        if S % m:
            body, carry = stage(p, 0, S, m, flush=False)
            tail, none = stage(p, S, 0, m, held=S % m, flush=True, continued=True, carry=carry)
            assert none is None and _same(np.concatenate([body, tail]), single), (m, channels)


def test_a_chain_of_one_sample_calls(gpu):
    x = content("random", 2, 60, 7, seed=4)
    h0 = random_history(2, 3)
    p = Planar(x, offset=1, pad=3)
    for m in (1, 7, 13):
        want, _ = tr.records_of(x, m, True, h0)
        carry = np.zeros(2, tr.CARRY_DTYPE)
        carry["hist"] = h0
        parts, held = [], 0
        for i in range(60):
            got, carry = stage(p, i, 1, m, held, flush=(i == 59), continued=True, carry=carry)
            parts.append(got)
            held = (held + 1) % m
            assert np.array_equal(carry["hist"], tr.history_after(x[:, :i + 1], h0)), (m, i)
        assert _same(np.concatenate(parts), want), m


def test_forced_slices_give_the_same_bytes(gpu):
    switch, tile = limits()
    for m, n, counts in ((3, 1000, (1, 2, 7, 64)), (7, 300, (5,)), (64, tile + 9, (1, 2, 7, 64)), (switch + 1, 3 * tile + 5, (1, 2, 7, 64)),
                         (5000, 40001, (1, 2, 7, 64)), (50000, 40001, (1, 2, 7, 64))):
        for channels, pad in ((1, 1), (5, 2)):
            x = content(("random", "saturated")[channels == 5], channels, 2 + n, m, seed=m)
            history = random_history(channels, m)
            auto, carry0 = check(x, m, 2 % m, False, slices=0, offset=3, pad=pad, history=history, what=(m, n, channels))
            for slices in counts:
                got, carry = check(x, m, 2 % m, False, slices=slices, offset=3, pad=pad, history=history, what=(m, n, channels, slices))
                assert _same(got, auto) and _same(carry, carry0, tr.CARRY_DTYPE)


def test_refusals_write_nothing(gpu):
    import torch
    x = wr.content("plain", 1, 100, 8, seed=1)
    p = Planar(x, pad=4)
    peaks = _dev(np.full(64 * WORDS, POISON, np.uint32))
    carry = _dev(np.full(2 * CWORDS, POISON, np.uint32))
    call = api.stage_truepeak_columns
    #                  planar stride ch n  m held flush continued slices
    assert call(None, p.stride, 1, 100, 8, 0, True, False, 0, carry, peaks) == E                  # a null d_planar
    assert call(p.at(0), p.stride, 0, 100, 8, 0, True, False, 0, carry, peaks) == E               # channels 0
    assert call(p.at(0), p.stride, 65, 100, 8, 0, True, False, 0, carry, peaks) == E              # channels above 64
    assert call(p.at(0), p.stride, 1, 100, 0, 0, True, False, 0, carry, peaks) == E               # m == 0
    assert call(p.at(0), p.stride, 1, 100, 8, 8, True, True, 0, carry, peaks) == E                # held >= m
    assert call(p.at(0), p.stride, 1, 100, 8, 3, True, False, 0, carry, peaks) == E               # held > 0 where the stream begins
    assert call(p.at(0), 99, 1, 100, 8, 0, True, False, 0, carry, peaks) == E                     # channel_stride < nsamples
    assert call(p.at(0), p.stride, 1, 100, 8, 0, True, False, 65, carry, peaks) == E              # slices > 64
    assert call(p.at(0), p.stride, 1, 100, 8, 0, True, False, 0, None, peaks) == E                # the carry is written: samples arrive
    assert call(p.at(0), p.stride, 1, 0, 8, 0, True, True, 0, None, peaks) == E                   # the carry is read: continued
    assert call(p.at(0), p.stride, 1, 100, 8, 0, True, False, 0, carry, None) == E                # columns close
    assert call(p.at(0), p.stride, 1, 0, 8, 3, True, True, 0, carry, None) == E                   # the flushed carry is a column
    for off in (1, 2, 3):                                                                         # 4, 8 and 12 bytes off a 16-byte boundary
        assert call(p.at(0), p.stride, 1, 100, 8, 0, True, False, 0, carry[off:], peaks) == E     # a carry that is not aligned to 16 bytes
        assert call(p.at(0), p.stride, 1, 100, 8, 0, True, False, 0, carry, peaks[off:]) == E     # nor the output
    torch.cuda.synchronize()
    assert (_host(peaks) == POISON).all() and (_host(carry) == POISON).all() and p.unchanged()
    # nothing closes: d_peaks may be NULL; nothing arrives and nothing is flushed: SGZ_OK, nothing launched, everything may be NULL
    assert call(p.at(0), p.stride, 1, 5, 8, 0, False, False, 0, carry, None) == api.SGZ_OK
    assert call(p.at(0), p.stride, 1, 0, 8, 0, True, False, 0, None, None) == api.SGZ_OK
    peaks2 = _dev(np.full(2 * WORDS, POISON, np.uint32))
    carry2 = _dev(np.full(CWORDS, POISON, np.uint32))
    assert call(p.at(0), p.stride, 1, 0, 8, 3, False, True, 0, carry2, peaks2) == api.SGZ_OK
    torch.cuda.synchronize()
    assert (_host(peaks2) == POISON).all() and (_host(carry2) == POISON).all() and (_host(peaks) == POISON).all()
    after = np.ascontiguousarray(_host(carry)[:CWORDS]).view(tr.CARRY_DTYPE)
    assert _same(after["open"], tr.records_of(x[:, :5], 8)[0][0]) and np.array_equal(after["hist"], tr.history_after(x[:, :5]))


def test_a_launch_beside_work_on_a_second_stream(gpu):
    import torch
    switch, tile = limits()
    side, mine = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=gpu)
    cases = []
    for m in (7, switch + 1):
        x = wr.content("random", 3, 3 * tile + 5, m, seed=m)
        cases.append((m, Planar(x, offset=1, pad=3), tr.records_of(x, m)[0]))
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
    want = {m: tr.records_of(x, m)[0] for m in (64, switch + 1)}

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
