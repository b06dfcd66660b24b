"""sgz_stage_run_columns on the GPU (csrc/run_columns.hip): byte for byte, no tolerance, against tests/run_ref.py -- the per-sample
definition, not the fold.

Every call goes through `stage`, which poisons everything around what the call may write -- the padding between the channel rows, a record
in front of the output and the records behind its last column, a carry in front of and behind the carry -- and checks it afterwards; a call
with samples must write the whole carry (the open column or zeros, the two-sample history, reserved == 0), a call without must leave it
alone.  The sizes follow the code through api.run_columns_limits(): the switch-over between the tile form and the sliced form, and the
tile's samples.  The shapes are the smallest that put a seam of every kind -- column, wave (64 samples), tile, slice -- inside the data."""
import os
import sys

import numpy as np
import pytest

from signalizer_amd import api

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import run_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = np.uint32(0xDEADBEEF)
WORDS, CWORDS = rr.DTYPE.itemsize // 4, rr.CARRY_DTYPE.itemsize // 4     # a record as 24 words, a carry as 28
E = api.SGZ_EINVAL
SMALL = (3, 1)                          # thresholds that rr.busy's small integers straddle
SEAM = (1 << 22, 1)                     # thresholds that leave _ramp's samples neither hot nor quiet
_limits = {}


def limits():
    if not _limits:
        _limits["v"] = api.run_columns_limits()
    return _limits["v"]


def _dev(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _same(a, b, dtype=rr.DTYPE):
    return a.shape == b.shape and np.ascontiguousarray(a, dtype).tobytes() == np.ascontiguousarray(b, dtype).tobytes()


def _params(p):
    return api.RunParams(*p)


def busy(channels, S, seed):
    return np.stack([rr.busy(S, seed=seed + 17 * d) for d in range(channels)]) if S else np.zeros((channels, 0), np.float32)


class Planar:
    """x float32 [channels][S] on the device: rows `stride` = S + pad apart, the first one `offset` floats behind a 16-byte boundary, poison in
    front, between and behind"""

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


def stage(p, at, n, m, params=SMALL, held=0, flush=True, continued=False, slices=0, carry=None, extra=3, stream=None):
    """the call on samples [at, at + n) of p with the carry [channels] (or None: poison) -> (records [columns][channels], the carry afterwards
    or None where the call must not write it); asserts SGZ_OK, the counts, and that nothing but the documented bytes changed"""
    import torch
    channels = p.channels
    columns, left = api.overview_step(m, held, n, flush)
    runs = _dev(np.full((1 + columns + extra) * channels * WORDS, POISON, np.uint32))
    carry_before = np.full((1 + channels + 1) * CWORDS, POISON, np.uint32)
    if carry is not None:
        carry_before[CWORDS:(1 + channels) * CWORDS] = np.ascontiguousarray(carry, rr.CARRY_DTYPE).reshape(-1).view(np.uint32)
    c = _dev(carry_before)
    st = api.stage_run_columns(p.at(at), p.stride, channels, n, _params(params), m, held, flush, continued, slices, c[CWORDS:], runs[channels * WORDS:],
                               stream=stream)
    assert st == api.SGZ_OK, (st, api.lib().sgz_last_error())
    torch.cuda.synchronize()
    got, carry_after = _host(runs), _host(c)
    first, last = channels * WORDS, (1 + columns) * channels * WORDS
    assert (got[:first] == POISON).all() and (got[last:] == POISON).all(), "bytes in front of the output or behind the last column were written"
    assert p.unchanged(), "the source or its padding was written"
    records = np.ascontiguousarray(got[first:last]).view(rr.DTYPE).reshape(columns, channels)
    if n:
        assert (carry_after[:CWORDS] == POISON).all() and (carry_after[(1 + channels) * CWORDS:] == POISON).all()
        after = np.ascontiguousarray(carry_after[CWORDS:(1 + channels) * CWORDS]).view(rr.CARRY_DTYPE).reshape(channels)
        assert not after["reserved"].any()
        if not left:
            assert after["open"].tobytes() == bytes(rr.DTYPE.itemsize * channels), "no sample stays open: the open column is written as zeros"
        return records, after
    assert np.array_equal(carry_after, carry_before), "the carry was written by a call without samples"
    return records, None


def expect(x, m, params, held, flush, history):
    """x [channels][held + n]: the stream behind `history` (int [channels][2] or None), of which the call takes the last n ->
    (carry in or None, records, carry out or None)"""
    channels, n = x.shape[0], x.shape[1] - held
    carry_in = None
    if history is not None:
        carry_in = np.zeros(channels, rr.CARRY_DTYPE)
        carry_in["prev"] = rr.history_after(x[:, :held], history)
        carry_in["reserved"] = 0xFFFFFFFF                               # (never read)
        if held:
            carry_in["open"] = rr.records(x[:, :held], m, params, True, history)[0][0]
        else:
            carry_in["open"] = np.frombuffer(b"\xab" * rr.DTYPE.itemsize, rr.DTYPE)[0]      # read iff held > 0
    every, _ = rr.records(x, m, params, True, history)
    open_ = (not flush) and (held + n) % m != 0
    carry_out = None
    if n:
        carry_out = np.zeros(channels, rr.CARRY_DTYPE)
        carry_out["prev"] = rr.history_after(x, history)
        if open_:
            carry_out["open"] = every[-1]
    return carry_in, (every[:-1] if open_ else every), carry_out


def check(x, m, held=0, flush=True, params=SMALL, slices=0, offset=0, pad=0, history=None, what=None):
    n = x.shape[1] - held
    carry_in, want, carry_out = expect(x, m, params, held, flush, history)
    p = Planar(x, offset, pad)
    got, carry = stage(p, held, n, m, params, held, flush, history is not None, slices, carry_in)
    assert _same(got, want), what
    assert (carry is None) == (carry_out is None) and (carry is None or _same(carry, carry_out, rr.CARRY_DTYPE)), what
    return got, carry


def some_history(channels, seed):
    """(v[-1], v[-2]) per channel: small integers that rr.busy's samples meet again, a mark among them"""
    rng = np.random.default_rng(seed)
    h = rng.integers(-3, 4, size=(channels, 2)).astype(np.int64)
    if seed % 3 == 0:
        h[0, seed % 2] = rr.NAN
    if seed % 5 == 0:
        h[-1, 0] = rr.CLAMP
    return h


@pytest.mark.parametrize("m", [1, 2, 3, 7, 63, 64, 65, 1000, "switch", "switch+1", "above"])
def test_records_equal_the_definition(gpu, m):
    """1 / 3 / 64 channels, every base offset 0 .. 3 floats, odd row strides, a held column, either flush, a history or none"""
    switch, tile = limits()
    m = {"switch": switch, "switch+1": switch + 1, "above": 3 * tile + 6}.get(m, m)
    # (n: nothing, one sample, around a column, around a wave, more than one tile -- where the reference's column loop stays quick -- and more
    # than one column of the sliced form)
    ns = sorted({0, 1, 2, max(m - 1, 0), m, m + 1, 129, 3 * m + 5} | ({tile + 3 * m + 5} if m >= 7 else {1300}))
    i = 0
    for n in ns:
        for held in sorted({0, 1 % m, m - 1}):
            flush = bool(i % 2)
            channels, offset, pad = (1, 3, 1, 3, 1, 3, 64)[i % 7], i % 4, (0, 1, 7, 65)[(i // 3) % 4]
            if channels * ((held + n + m - 1) // m) > 6000:             # (the reference walks every column in Python)
                channels = 3
            x = busy(channels, held + n, seed=1000 * m + i)
            history = some_history(channels, i) if held or (i // 5) % 2 else None
            check(x, m, held, flush, offset=offset, pad=pad, history=history, what=(m, n, held, flush, channels, offset, pad, history is not None))
            i += 1
    if m == 1:                                                          # more than one tile of one-sample columns, once
        check(busy(1, tile + 5, seed=5), 1, offset=3, pad=1, what="m = 1 over a tile")


def test_64_channels_in_every_form(gpu):
    switch, tile = limits()
    for m, n in ((7, 500), (64, tile + 100), (switch + 1, 3 * switch + 8)):
        check(busy(64, 1 + n, seed=m), m, held=1, flush=False, offset=m % 4, pad=3, history=some_history(64, m), what=(m, n))


def test_default_thresholds_on_16_bit_signals(gpu):
    switch, tile = limits()
    x = np.stack([rr.clipped(tile + 700), rr.s16(tile + 700), np.zeros(tile + 700, np.float32)])
    for m in (64, 1000, switch + 1):
        got, _ = check(x, m, params=rr.DEFAULT, offset=1, pad=3, what=m)
        assert int(got["of"]["longest"][:, 0, rr.HOT].max()) >= 10 and int(got["of"]["runs"][:, 0, rr.HOT].sum()) > 2 * (tile + 700) // 53 - 3       # both rails
        assert int(got["of"]["count"][:, 1, rr.HOT].sum()) == 0
        assert (got["of"]["head"][:, 2, rr.QUIET] == got["len"][:, 2]).all() and int(got["of"]["runs"][:, 2, rr.QUIET].sum()) == 1
        assert int(got["of"]["runs"][:, 2, rr.FLAT].sum()) == 1 and int(got["of"]["count"][:, 2, rr.FLAT].sum()) == tile + 699


# the forms and their seams: (m, slices, n, the sample indices at which a new column / wave step / tile / slice / wave quarter begins)
def _forms():
    switch, tile = limits()
    forms = []
    m = 8                                                               # the packed form: 8 columns share a wave's masks; a tile is 4096 samples
    forms.append((m, 0, tile + 200, [64, 72, tile]))
    m = 100                                                             # a wave walks a column: steps of 64 from the column's start; a tile is 40 columns
    forms.append((m, 0, (tile // m) * m + 350, [100, 164, 200, (tile // m) * m, (tile // m) * m + 64]))
    m = 3000                                                            # the sliced form, three slices of 1000; a wave takes 256 of them, 64 a step
    forms.append((m, 3, 2 * m + 500, [64, 256, 512, 768, 1000, 1064, 2000, 3000, 3064, 4000, 4256]))
    return forms


def _ramp(S):
    """no two neighbours equal, none hot or quiet under SMALL, all positive"""
    return ((np.arange(S) % 50 + 10) / 8388608.0).astype(np.float32)


def _column_of(i, m):
    return i // m, i % m


@pytest.mark.parametrize("form", [0, 1, 2])
def test_signals_on_every_seam(gpu, form):
    """signals built to sit on the seams; the fields are asserted as well as the bytes, so that each signal is what it says"""
    for m, slices, S, seams in _forms()[form:form + 1]:
        columns = -(-S // m)

        def run(x, what):
            got, _ = check(x[None, :], m, params=SEAM, slices=slices, offset=len(what) % 4, pad=1, what=(m, what))
            return got[:, 0]

        # one run covering all columns
        x = np.full(S, 1.0, np.float32)
        got = run(x, "all hot")
        for k, first in ((rr.HOT, 0), (rr.FLAT, 1)):                    # (sample 0 of the stream has nothing before it: it is not flat)
            assert (got["of"]["head"][first:, k] == got["len"][first:]).all() and (got["of"]["tail"][:, k] == got["len"] - (got["of"]["at"][:, k])).all()
            assert (got["of"]["longest"][first:, k] == got["len"][first:]).all() and not got["of"]["at"][first:, k].any()
            assert got["of"]["runs"][:, k].tolist() == [1] + [0] * (columns - 1)
        f0 = got["of"][0, rr.FLAT]
        assert (int(f0["count"]), int(f0["head"]), int(f0["at"]), int(f0["longest"]), int(f0["tail"])) == (m - 1, 0, 1, m - 1, m - 1)
        for s in seams:
            c, o = _column_of(s, m)
            # a run of 5 ending exactly on the seam's last sample, and one starting on its first
            if o >= 5 or o == 0:
                x = _ramp(S)
                x[s - 5:s] = 1.0
                h = run(x, f"ends at {s}")["of"][:, rr.HOT]
                cc, oo = _column_of(s - 5, m)
                assert int(h["count"].sum()) == 5 and int(h["runs"].sum()) == 1 and (int(h["longest"][cc]), int(h["at"][cc])) == (5, oo)
                assert int(h["tail"][cc]) == (5 if o == 0 else 0) and int(h["head"][c]) == 0
            x = _ramp(S)
            x[s:s + 5] = -1.0
            got = run(x, f"starts at {s}")
            h = got["of"][:, rr.HOT]
            assert int(h["runs"].sum()) == 1 and (int(h["longest"][c]), int(h["at"][c])) == (5, o) and int(h["head"][c]) == (5 if o == 0 else 0)
            assert int(got["crossings"].sum()) == 2 and int(got["crossings"][c]) >= 1              # a sign change across the seam, and back
            f = got["of"][:, rr.FLAT]
            assert int(f["count"].sum()) == 4 and (int(f["longest"][c]), int(f["at"][c])) == (4, o + 1)
            # equal-length runs twice in a column, on either side of the seam where it lies inside one: the earlier one is located
            lo = s - 6 if o >= 6 else s + 1
            x = _ramp(S)
            x[lo:lo + 4] = 1.0
            x[lo + 7:lo + 11] = 1.0
            h = run(x, f"twice around {s}")["of"][:, rr.HOT]
            cc, oo = _column_of(lo, m)
            if _column_of(lo + 10, m)[0] == cc:
                assert (int(h["runs"][cc]), int(h["longest"][cc]), int(h["at"][cc]), int(h["count"][cc])) == (2, 4, oo, 8)
            # a NaN on either side of the seam in a run that would cover it
            for side in (s - 1, s):
                x = _ramp(S)
                x[s - 4:s + 4] = 1.0
                x[side] = np.nan
                got = run(x, f"NaN at {side}")
                h = got["of"][:, rr.HOT]
                assert int(got["skipped"].sum()) == 1 and int(got["skipped"][side // m]) == 1 and int(h["count"].sum()) == 7
                assert int(h["runs"].sum()) == 2 and int(h["longest"].max()) <= 4
                assert int(got["of"]["count"][:, rr.FLAT].sum()) == 5          # 3 + 2: the sample behind a NaN is not flat
            # two equal samples split by the seam
            x = _ramp(S)
            x[s] = x[s - 1]
            f = run(x, f"flat across {s}")["of"][:, rr.FLAT]
            assert int(f["count"].sum()) == 1 and (int(f["count"][c]), int(f["runs"][c]), int(f["at"][c]), int(f["longest"][c])) == (1, 1, o, 1)
            # v = 0 beside negatives; -0.0 and +0.0 and denormals are all v = 0: quiet and flat; +-inf and what clamps are hot, and equal
            x = -_ramp(S)
            x[s - 2:s + 2] = (-0.0, 1e-42, 0.0, -1e-42)
            got = run(x, f"zeros around {s}")
            q = got["of"][:, rr.QUIET]
            assert int(q["count"].sum()) == 4 and int(q["runs"].sum()) == 1 and int(got["crossings"].sum()) == 2
            assert int(got["of"]["count"][:, rr.FLAT].sum()) == 3
            x = _ramp(S)
            x[s - 2:s + 2] = (np.inf, 20.0, 8.0, 9.5)
            x[s + 2:s + 4] = (-np.inf, -8.0)
            got = run(x, f"clamped around {s}")
            assert int(got["of"]["count"][:, rr.HOT].sum()) == 6 and int(got["of"]["runs"][:, rr.HOT].sum()) == 1
            assert int(got["of"]["count"][:, rr.FLAT].sum()) == 4 and int(got["of"]["runs"][:, rr.FLAT].sum()) == 2 and int(got["crossings"].sum()) == 2


def test_a_chain_of_calls_equals_the_single_call(gpu):
    switch, tile = limits()
    rng = np.random.default_rng(9)
    for m in (1, 5, 64, 257, switch, switch + 1, 3000):
        channels = (1, 2, 3)[m % 3]
        S = (600 if m < 64 else tile + 77) + int(rng.integers(0, 3 * m))
        x = busy(channels, S, seed=m + channels)
        p = Planar(x, offset=int(rng.integers(0, 4)), pad=int(rng.integers(0, 9)))
        single, carry = stage(p, 0, S, m)
        assert _same(single, rr.records(x, m, SMALL)[0]), (m, channels)
        cuts = set(int(v) for v in rng.integers(0, S + 1, size=6)) | {S}
        at = int(rng.integers(0, S - 200))
        for step in (1, 2, 1, 1, 2, 2, 3, 1):                           # calls of 1 and 2 samples: the two-sample history shifts
            at += step
            cuts.add(at)
        cuts = sorted(cuts)
        parts, at, held, carry, continued = [], 0, 0, None, False
        for cut in [0] + cuts:                                          # (the first call is empty)
            last = cut == S
            got, after = stage(p, at, cut - at, m, held=held, flush=last, continued=continued, carry=carry)
            parts.append(got)
            if after is not None:
                carry, continued = after, True
                assert _same(carry, rr.carry_after(x[:, :cut], m, SMALL, flushed=last), rr.CARRY_DTYPE), (m, cut)
            held, at = (0 if last else (held + cut - at) % m), cut
        assert _same(np.concatenate(parts), single), (m, channels, cuts)
        # the flush alone, on the carry of everything but a column's end: the carry stays
        if S % m:
            body, carry = stage(p, 0, S, m, flush=False)
            tail, none = stage(p, S, 0, m, held=S % m, flush=True, continued=True, carry=carry)
            assert none is None and _same(np.concatenate([body, tail]), single), (m, channels)


def test_a_chain_of_one_sample_calls_and_a_carry_of_marks(gpu):
    x = busy(2, 60, seed=4)
    p = Planar(x, offset=1, pad=3)
    for m in (1, 7, 13):
        for h0 in (some_history(2, 3), None):
            want, _ = rr.records(x, m, SMALL, True, h0)
            carry = np.zeros(2, rr.CARRY_DTYPE)
            carry["prev"] = rr.NAN if h0 is None else h0                # continued == 0 is exactly a history of two marks
            parts, held = [], 0
            for i in range(60):
                got, carry = stage(p, i, 1, m, held=held, flush=(i == 59), continued=True, carry=carry)
                parts.append(got)
                held = (held + 1) % m
                assert np.array_equal(carry["prev"], rr.history_after(x[:, :i + 1], h0)), (m, i)
            assert _same(np.concatenate(parts), want), m
    # ... for longer calls too, in both forms
    switch, tile = limits()
    x = np.full((1, 2 * switch + 9), 0.0, np.float32)                   # flat from the first sample on: what a history would change
    p = Planar(x)
    for m in (64, switch + 1):
        marks = np.zeros(1, rr.CARRY_DTYPE)
        marks["prev"] = rr.NAN
        a, ca = stage(p, 0, p.S, m, continued=False)
        b, cb = stage(p, 0, p.S, m, continued=True, carry=marks)
        assert _same(a, b) and _same(ca, cb, rr.CARRY_DTYPE) and int(a["of"]["count"][0, 0, rr.FLAT]) == m - 1


def test_a_flush_in_the_middle_keeps_the_history(gpu):
    switch, tile = limits()
    for m in (64, switch + 1):
        S, cut = 3 * m + 50, m + 21
        x = np.full((2, S), 0.5, np.float32)                            # one flat run through the flush
        x[1] = busy(1, S, seed=m)[0]
        p = Planar(x, offset=2, pad=1)
        first, carry = stage(p, 0, cut, m, flush=True)
        assert _same(first, rr.records(x[:, :cut], m, SMALL)[0]) and _same(carry, rr.carry_after(x[:, :cut], m, SMALL, flushed=True), rr.CARRY_DTYPE)
        rest, _ = stage(p, cut, S - cut, m, flush=True, continued=True, carry=carry)
        assert _same(rest, rr.records(x[:, cut:], m, SMALL, True, rr.history_after(x[:, :cut]))[0])
        f = rest["of"][:, 0, rr.FLAT]
        assert int(f["runs"].sum()) == 0 and int(f["head"][0]) == m     # the first sample after the flush relates to the one before it
        fresh, _ = stage(p, cut, S - cut, m, flush=True)                # without the history a run begins
        assert int(fresh["of"]["runs"][:, 0, rr.FLAT].sum()) == 1 and int(fresh["of"]["head"][0, 0, rr.FLAT]) == 0


def test_forced_slices_give_the_same_bytes(gpu):
    switch, tile = limits()
    for m, n, counts in ((3, 700, (1, 2, 7, 64)), (7, 300, (5,)), (64, tile + 9, (1, 2, 7, 64)), (switch + 1, 3 * tile + 5, tuple(range(1, 65))),
                         (5000, 20001, (1, 2, 3, 7, 33, 64)), (50000, 20001, (1, 2, 7, 63, 64))):
        for channels, pad in ((1, 1), (3, 2)):
            x = busy(channels, 2 + n, seed=m)
            x[0, 100:min(n, 9000)] = 1.0                                # a run across slices, waves and steps
            history = some_history(channels, m)
            carry_in, want, carry_out = expect(x, m, SMALL, 2 % m, False, history)
            p = Planar(x, 3, pad)
            for slices in (0,) + counts:
                got, carry = stage(p, 2 % m, n, m, SMALL, 2 % m, False, True, slices, carry_in)
                assert _same(got, want) and _same(carry, carry_out, rr.CARRY_DTYPE), (m, n, channels, slices)


def test_refusals_write_nothing(gpu):
    import torch
    x = busy(1, 100, seed=1)
    p = Planar(x, pad=4)
    runs = _dev(np.full(64 * WORDS, POISON, np.uint32))
    carry = _dev(np.full(2 * CWORDS, POISON, np.uint32))
    call = api.stage_run_columns
    ok = _params(SMALL)
    #                  planar stride ch n params m held flush continued slices
    assert call(None, p.stride, 1, 100, ok, 8, 0, True, False, 0, carry, runs) == E                  # a null d_planar
    assert call(p.at(0), p.stride, 1, 100, None, 8, 0, True, False, 0, carry, runs) == E             # null params
    for bad in ((0, 0), (2**26 + 1, 0), (4, 4)):
        assert call(p.at(0), p.stride, 1, 100, _params(bad), 8, 0, True, False, 0, carry, runs) == E # invalid params
    assert call(p.at(0), p.stride, 0, 100, ok, 8, 0, True, False, 0, carry, runs) == E               # channels 0
    assert call(p.at(0), p.stride, 65, 100, ok, 8, 0, True, False, 0, carry, runs) == E              # channels above 64
    assert call(p.at(0), p.stride, 1, 100, ok, 0, 0, True, False, 0, carry, runs) == E               # m == 0
    assert call(p.at(0), p.stride, 1, 100, ok, 8, 8, True, True, 0, carry, runs) == E                # held >= m
    assert call(p.at(0), p.stride, 1, 100, ok, 8, 3, True, False, 0, carry, runs) == E               # held > 0 where the stream begins
    assert call(p.at(0), 99, 1, 100, ok, 8, 0, True, False, 0, carry, runs) == E                     # channel_stride < nsamples
    assert call(p.at(0), p.stride, 1, 100, ok, 8, 0, True, False, 65, carry, runs) == E              # slices > 64
    assert call(p.at(0), p.stride, 1, 100, ok, 8, 0, True, False, 0, None, runs) == E                # the carry is written: samples arrive
    assert call(p.at(0), p.stride, 1, 0, ok, 8, 0, True, True, 0, None, runs) == E                   # the carry is read: continued
    assert call(p.at(0), p.stride, 1, 100, ok, 8, 0, True, False, 0, carry, None) == E               # columns close
    assert call(p.at(0), p.stride, 1, 0, ok, 8, 3, True, True, 0, carry, None) == E                  # the flushed carry is a column
    for off in (1, 2, 3):                                                                            # 4, 8 and 12 bytes off a 16-byte boundary
        assert call(p.at(0), p.stride, 1, 100, ok, 8, 0, True, False, 0, carry[off:], runs) == E     # a carry that is not aligned to 16 bytes
        assert call(p.at(0), p.stride, 1, 100, ok, 8, 0, True, False, 0, carry, runs[off:]) == E     # nor the output
    torch.cuda.synchronize()
    assert (_host(runs) == POISON).all() and (_host(carry) == POISON).all() and p.unchanged()
    # nothing closes: d_runs may be NULL; nothing arrives and nothing is flushed: SGZ_OK, nothing launched, everything may be NULL
    assert call(p.at(0), p.stride, 1, 5, ok, 8, 0, False, False, 0, carry, None) == api.SGZ_OK
    assert call(p.at(0), p.stride, 1, 0, ok, 8, 0, True, False, 0, None, None) == api.SGZ_OK
    runs2 = _dev(np.full(2 * WORDS, POISON, np.uint32))
    carry2 = _dev(np.full(CWORDS, POISON, np.uint32))
    assert call(p.at(0), p.stride, 1, 0, ok, 8, 3, False, True, 0, carry2, runs2) == api.SGZ_OK
    torch.cuda.synchronize()
    assert (_host(runs2) == POISON).all() and (_host(carry2) == POISON).all() and (_host(runs) == POISON).all()
    after = np.ascontiguousarray(_host(carry)[:CWORDS]).view(rr.CARRY_DTYPE)
    assert _same(after, rr.carry_after(x[:, :5], 8, SMALL), rr.CARRY_DTYPE)


def test_a_launch_beside_work_on_a_second_stream(gpu):
    import torch
    switch, tile = limits()
    side, mine = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=gpu)
    cases = []
    for m in (7, 100, switch + 1):
        x = busy(3, (600 if m == 7 else tile + 505), seed=m)
        cases.append((m, Planar(x, offset=1, pad=3), rr.records(x, m, SMALL)[0]))
    torch.cuda.synchronize()
    for rounds in range(3):
        with torch.cuda.stream(side):
            for _ in range(20):
                a = torch.tanh(a @ a * 1e-3)
        for m, p, want in cases:
            got, _ = stage(p, 0, p.S, m, stream=mine.cuda_stream)
            assert _same(got, want), (rounds, m)
    torch.cuda.synchronize()
