"""Interleaved PCM in on the GPU (sgz.h "interleaved PCM in"): the convert-and-de-interleave kernel against numpy, bit for bit, and the
stream handle / one-shot render against sgz_spectrogram_render_host of the numpy-converted floats, byte for byte, for every way of
cutting the stream.  The converter's values are defined exactly (sgz.h), so every comparison is of uint32 views; numpy's
astype(np.float32) rounds to nearest even."""
import ctypes as C
import gc

import numpy as np
import pytest

from signalizer_amd import api, config

pytestmark = pytest.mark.gpu

FORMATS = [api.PCM_F32, api.PCM_U8, api.PCM_S16, api.PCM_S24, api.PCM_S32, api.PCM_F64]
NAME = {api.PCM_F32: "f32", api.PCM_U8: "u8", api.PCM_S16: "s16", api.PCM_S24: "s24", api.PCM_S32: "s32", api.PCM_F64: "f64"}
BYTES = api.PCM_SAMPLE_BYTES
ALIGN = {api.PCM_F32: 4, api.PCM_U8: 1, api.PCM_S16: 2, api.PCM_S24: 1, api.PCM_S32: 4, api.PCM_F64: 8}
SENTINEL = 0x7FC0DEAD                 # a NaN no conversion of the random sources produces


# ---- the CPU reference ------------------------------------------------------------------------------------------------------------------
def to_bytes(values, fmt):
    """sample values (ints, or floats for F32 / F64) -> their little-endian bytes as a uint8 array"""
    if fmt == api.PCM_U8:
        return np.asarray(values, np.uint8).copy()
    if fmt == api.PCM_S16:
        return np.asarray(values, "<i2").view(np.uint8).copy()
    if fmt == api.PCM_S24:
        v = np.asarray(values, np.int64) & 0xFFFFFF
        return np.stack([v & 0xFF, (v >> 8) & 0xFF, v >> 16], axis=-1).astype(np.uint8).reshape(-1)
    if fmt == api.PCM_S32:
        return np.asarray(values, "<i4").view(np.uint8).copy()
    if fmt == api.PCM_F32:
        return np.asarray(values, "<f4").view(np.uint8).copy()
    return np.asarray(values, "<f8").view(np.uint8).copy()


def convert_ref(raw, fmt, channels):
    """interleaved bytes -> planar float32 [channels, n], by sgz.h's table"""
    raw = np.ascontiguousarray(raw, np.uint8)
    if fmt == api.PCM_U8:
        v = (raw.astype(np.int32) - 128).astype(np.float32) * np.float32(2.0 ** -7)
    elif fmt == api.PCM_S16:
        v = np.frombuffer(raw.tobytes(), "<i2").astype(np.float32) * np.float32(2.0 ** -15)
    elif fmt == api.PCM_S24:
        b = raw.reshape(-1, 3).astype(np.int32)
        x = b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16
        v = ((x ^ 0x800000) - 0x800000).astype(np.float32) * np.float32(2.0 ** -23)
    elif fmt == api.PCM_S32:
        v = np.frombuffer(raw.tobytes(), "<i4").astype(np.float32) * np.float32(2.0 ** -31)
    elif fmt == api.PCM_F32:
        v = np.frombuffer(raw.tobytes(), "<f4")
    else:
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            v = np.frombuffer(raw.tobytes(), "<f8").astype(np.float32)
    return np.ascontiguousarray(v.reshape(-1, channels).T)


def random_bytes(rng, fmt, count):
    """`count` random samples' bytes; the float formats draw finite values of many magnitudes (random bit patterns would be mostly huge)"""
    if fmt == api.PCM_F32:
        return to_bytes((rng.standard_normal(count) * 10.0 ** rng.integers(-6, 3, count)).astype(np.float32), fmt)
    if fmt == api.PCM_F64:
        return to_bytes(rng.standard_normal(count) * 10.0 ** rng.integers(-30, 20, count), fmt)
    return rng.integers(0, 256, count * BYTES[fmt], dtype=np.uint8)


def same_floats(got, want, src64=None):
    """bit for bit; where an F64 source is NaN, NaN-ness only (sgz.h leaves the payload open)"""
    g, w = got.view(np.uint32), want.view(np.uint32)
    if src64 is not None:
        nan = np.isnan(src64)
        return np.array_equal(g[~nan], w[~nan]) and bool(np.all(np.isnan(got[nan])))
    return np.array_equal(g, w)


def device_source(raw, offset, gpu):
    """the bytes on the device in an allocation of exactly offset + len(raw) bytes, first sample at byte `offset` of it"""
    import torch
    buf = torch.empty(offset + raw.size, dtype=torch.uint8, device=gpu)
    assert buf.data_ptr() % 16 == 0
    buf[offset:] = torch.from_numpy(raw).to(gpu)
    return buf, buf[offset:]


def run_converter(src, fmt, channels, n, cmap, rows, stride, gpu, guard_rows=1):
    """-> uint32 [rows + guard_rows, stride] as the device left it (prefilled with the sentinel)"""
    import torch
    out = torch.full((rows + guard_rows, stride), SENTINEL, dtype=torch.int32, device=gpu)
    api.pcm_to_planar_device(src, fmt, channels, n, out, channel_map=cmap, num_channels=rows, channel_stride=stride)
    return out.cpu().numpy().view(np.uint32)


def maps_for(channels):
    return {"identity": (None, channels), "reversed": (list(range(channels))[::-1], channels),
            "one-to-all": ([channels - 1] * 4, 4), "subset": ([channels - 1, channels // 2], 2)}


# ---- the converter ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("fmt", FORMATS, ids=[NAME[f] for f in FORMATS])
def test_converter_layouts(gpu, fmt, channels):
    """every sample count x base-pointer residue x channel map x row stride: the rows bit for bit, row padding and a guard row behind the
    last row untouched.  (4099 samples are more than one tile at every frame size here; the tile starts fall inside frames and S24 samples
    wherever frame_bytes does not divide 16.)"""
    rng = np.random.default_rng(1000 * fmt + channels)
    nmax = 4099
    raw_all = random_bytes(rng, fmt, nmax * channels)
    fb = channels * BYTES[fmt]
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4099):
        raw = raw_all[:n * fb]
        ref = convert_ref(raw, fmt, channels).view(np.uint32)
        for offset in range(0, 16, ALIGN[fmt]):
            buf, src = device_source(raw, offset, gpu)
            for name, (cmap, rows) in maps_for(channels).items():
                for stride in (n, (n + 63) // 64 * 64 + 64):
                    got = run_converter(src, fmt, channels, n, cmap, rows, stride, gpu)
                    want = np.full_like(got, SENTINEL)
                    for d in range(rows):
                        want[d, :n] = ref[cmap[d] if cmap is not None else d]
                    assert np.array_equal(got, want), (NAME[fmt], channels, n, offset, name, stride, np.argwhere(got != want)[:4])


VALUES = {
    api.PCM_U8: [0, 255, 127, 128, 129, 1],
    api.PCM_S16: [-32768, 32767, -1, 1, 0],
    api.PCM_S24: [-8388608, 8388607, -1, 1, 0, 0x7FFF00, 255, 65536, -65536],
    api.PCM_S32: [-2 ** 31, 2 ** 31 - 1, -1, 1, 0] + [s * v for s in (1, -1) for v in (2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 + 2, 2 ** 25 + 6)],
    api.PCM_F32: None,
    api.PCM_F64: [0.0, -0.0, 5e-324, -5e-324, 1e-40, -1e-40, np.inf, -np.inf, np.nan, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1e39, -1e39, 1e-46,
                  2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150, 2.0 ** -126 - 2.0 ** -150, 3.4028235677973366e38],
}


@pytest.mark.parametrize("fmt", FORMATS, ids=[NAME[f] for f in FORMATS])
def test_converter_values(gpu, fmt):
    """type extremes, +-1, 0, the round-to-nearest-even ties of S32 and F64, signed zeros, denormals, infinities and NaNs, then random ones"""
    rng = np.random.default_rng(77 + fmt)
    if fmt == api.PCM_F32:       # bit patterns: +-0, the smallest and largest denormals, +-inf, quiet and signalling NaNs with payloads
        special = to_bytes(np.array([0, 0x80000000, 1, 0x80000001, 0x007FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC12345,
                                     0x7FA00000, 0x3F800000], np.uint32).view(np.float32), fmt)
        rand = rng.integers(0, 256, 4 * 5000, dtype=np.uint8)                 # every bit pattern is a legal source
    else:
        special = to_bytes(VALUES[fmt], fmt)
        rand = random_bytes(rng, fmt, 5000)
    raw = np.concatenate([special, rand])
    n = raw.size // BYTES[fmt]
    ref = convert_ref(raw, fmt, 1)
    buf, src = device_source(raw, 0, gpu)
    got = run_converter(src, fmt, 1, n, None, 1, n, gpu)[:1].view(np.float32)
    src64 = np.frombuffer(raw.tobytes(), "<f8").reshape(1, -1) if fmt == api.PCM_F64 else None
    assert same_floats(got, ref, src64), (NAME[fmt], np.argwhere(got.view(np.uint32) != ref.view(np.uint32))[:6])
    k = len(special) // BYTES[fmt]
    g = got[0, :k]
    if fmt == api.PCM_S32:       # the reference itself, spelled out for the ties: 2^24+1 -> 2^24, 2^24+3 -> 2^24+4, 2^25+2 -> 2^25, 2^25+6 -> 2^25+8
        assert [float(v) * 2.0 ** 31 for v in g[5:9]] == [2.0 ** 24, 2.0 ** 24 + 4, 2.0 ** 25, 2.0 ** 25 + 8]
        assert [float(v) * 2.0 ** 31 for v in g[9:13]] == [-2.0 ** 24, -2.0 ** 24 - 4, -2.0 ** 25, -2.0 ** 25 - 8]
        assert float(g[0]) == -1.0 and float(g[1]) == 1.0
    if fmt == api.PCM_F64:
        assert float(g[9]) == 1.0 and float(g[10]) == 1 + 2.0 ** -22 and np.isposinf(g[11]) and np.isneginf(g[12]) and float(g[13]) == 0.0
        assert np.isnan(g[8]) and g[1:2].view(np.uint32)[0] == 0x80000000 and float(g[4]) != 0.0          # -0 kept; 1e-40 is a denormal, not 0
    if fmt == api.PCM_S24:
        assert float(g[0]) == -1.0 and float(g[1]) == 1 - 2.0 ** -23
    if fmt == api.PCM_U8:
        assert [float(v) for v in g[:4]] == [-1.0, 127 / 128, -1 / 128, 0.0]
    if fmt == api.PCM_S16:
        assert [float(v) for v in g[:2]] == [-1.0, 32767 / 32768]


def test_converter_64_channels_and_tile_of_one_group(gpu):
    """the widest frame (64 x F64 = 512 bytes: a tile is one group of 64 samples) and a repeated, gappy map of 64 rows"""
    rng = np.random.default_rng(5)
    n, channels = 200, 64
    cmap = [int(v) for v in rng.integers(0, 64, 64)]
    for fmt in (api.PCM_F64, api.PCM_S24):
        raw = random_bytes(rng, fmt, n * channels)
        ref = convert_ref(raw, fmt, channels).view(np.uint32)
        buf, src = device_source(raw, 8, gpu)
        got = run_converter(src, fmt, channels, n, cmap, 64, n + 3, gpu)
        want = np.full_like(got, SENTINEL)
        want[:64, :n] = ref[cmap]
        assert np.array_equal(got, want)


def test_converter_offsets_above_4_gib(gpu):
    """64-channel U8, 2^26 + 1000 samples: the source is 4 GiB + 64000 bytes.  Its 64 MiB blocks all differ (one random block XOR the block's
    index), so an offset that wrapped at 2^32 would read another block's bytes."""
    import torch
    channels, n = 64, (1 << 26) + 1000
    block = torch.randint(0, 256, (1 << 26,), dtype=torch.uint8, device=gpu, generator=torch.Generator(device=gpu).manual_seed(3))
    src = torch.empty(n * channels, dtype=torch.uint8, device=gpu)
    for i in range(0, src.numel(), block.numel()):
        part = src[i:i + block.numel()]
        part.copy_(block[:part.numel()] ^ (i // block.numel()))
    cmap = [63, 0]
    out = torch.full((3, n), SENTINEL, dtype=torch.int32, device=gpu)
    api.pcm_to_planar_device(src, api.PCM_U8, channels, n, out, channel_map=cmap, num_channels=2, channel_stride=n)
    for lo, hi in ((0, 3000), ((1 << 26) - 3000, (1 << 26) + 1000), ((1 << 25) - 100, (1 << 25) + 100)):
        ref = convert_ref(src[lo * channels:hi * channels].cpu().numpy(), api.PCM_U8, channels).view(np.uint32)
        got = out[:, lo:hi].cpu().numpy().view(np.uint32)
        assert np.array_equal(got[0], ref[63]) and np.array_equal(got[1], ref[0]), (lo, hi)
    assert bool((out[2] == SENTINEL).all())
    # the whole rows once, on the device (torch's integer -> float conversion of |x| <= 128 is exact)
    want = (src.view(n, channels)[:, [63, 0]].T.to(torch.float32) - 128.0) * (2.0 ** -7)
    assert bool((out[:2].view(torch.float32) == want).all())


def test_converter_refusals(gpu):
    import torch
    L = api.lib()
    src = torch.zeros(4096, dtype=torch.uint8, device=gpu)
    out = torch.full((4, 64), SENTINEL, dtype=torch.int32, device=gpu)
    ident = None
    m = lambda *v: (C.c_uint32 * len(v))(*v)
    call = lambda pcm, fmt, sch, n, cmap, nch, dst, stride: L.sgz_pcm_to_planar_device(pcm, fmt, sch, n, cmap, nch, dst, stride, None)
    s, d = src.data_ptr(), out.data_ptr()
    cases = {
        "null pcm": (None, api.PCM_S16, 2, 8, ident, 2, d, 64), "null planar": (s, api.PCM_S16, 2, 8, ident, 2, None, 64),
        "format END": (s, api.PCM_END, 2, 8, ident, 2, d, 64), "format 99": (s, 99, 2, 8, ident, 2, d, 64),
        "src 0": (s, api.PCM_S16, 0, 8, m(0, 0), 2, d, 64), "src 65": (s, api.PCM_U8, 65, 8, ident, 2, d, 64),
        "rows 0": (s, api.PCM_S16, 2, 8, ident, 0, d, 64), "rows 65": (s, api.PCM_U8, 64, 8, m(*([0] * 65)), 65, d, 64),
        "map entry": (s, api.PCM_S16, 2, 8, m(0, 2), 2, d, 64), "identity too wide": (s, api.PCM_S16, 2, 8, ident, 3, d, 64),
        "stride": (s, api.PCM_S16, 2, 65, ident, 2, d, 64),
        "s16 odd": (s + 1, api.PCM_S16, 2, 8, ident, 2, d, 64), "s32 +2": (s + 2, api.PCM_S32, 2, 8, ident, 2, d, 64),
        "f32 +1": (s + 1, api.PCM_F32, 2, 8, ident, 2, d, 64), "f64 +4": (s + 4, api.PCM_F64, 2, 8, ident, 2, d, 64),
    }
    for name, a in cases.items():
        assert call(*a) == api.SGZ_EINVAL, name
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call(s + 1, api.PCM_S24, 2, 8, ident, 2, d, 64) == api.SGZ_OK and call(s + 3, api.PCM_U8, 2, 8, ident, 2, d, 64) == api.SGZ_OK
    out.fill_(SENTINEL)
    assert call(s, api.PCM_S16, 2, 0, ident, 2, d, 64) == api.SGZ_OK and call(None, api.PCM_S16, 2, 0, ident, 2, d, 64) == api.SGZ_EINVAL
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- the stream handle and the one-shot call --------------------------------------------------------------------------------------------
FUSED, HALVES, SIDE_MAP, CHANNEL_SPLIT = 1, 2, 4, 8


def _case(name):
    """-> (cfg, format, src_channels, channel_map, nsamples, want_lines, expected sgz_plan_path)"""
    if name == "fused-s16":
        return config.spectrum_config(window_size=4096, hop=1024), api.PCM_S16, 2, None, 4096 + 23 * 1024, True, FUSED
    if name == "generic-s24-7ch":
        return (config.spectrum_config(window_size=1000, hop=333, num_pairs=3), api.PCM_S24, 7, [6, 0, 3, 3, 1, 5],
                1000 + 30 * 333 + 77, True, SIDE_MAP)
    if name == "split-f32-image":
        return config.spectrum_config(window_size=32768, hop=8192), api.PCM_F32, 2, None, 32768 + 8 * 8192, False, FUSED | CHANNEL_SPLIT
    if name == "phase-f64":
        return config.spectrum_config(window_size=2048, hop=512, channel_mode=config.CH_PHASE), api.PCM_F64, 2, [1, 0], 2048 + 19 * 512 + 5, True, 0
    if name == "merge-u8-mono":
        return config.spectrum_config(window_size=8192, hop=2048, channel_mode=config.CH_MERGE), api.PCM_U8, 1, [0, 0], 8192 + 11 * 2048, True, HALVES | SIDE_MAP
    raise KeyError(name)


CASES = ["fused-s16", "generic-s24-7ch", "split-f32-image", "phase-f64", "merge-u8-mono"]
_truth = {}


def _signal_bytes(fmt, channels, n, seed):
    """a few sines and noise per channel, quantised to the format"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None]
    x = 0.4 * np.sin(2 * np.pi * t * (0.001 + 0.013 * np.arange(1, channels + 1))) + 0.2 * np.sin(2 * np.pi * t * 0.21) + 0.05 * rng.standard_normal((n, channels))
    if fmt == api.PCM_F32 or fmt == api.PCM_F64:
        return to_bytes(x.reshape(-1), fmt)
    bits = 8 * BYTES[fmt]
    q = np.clip(np.round(x * 2.0 ** (bits - 1)), -2.0 ** (bits - 1), 2.0 ** (bits - 1) - 1).astype(np.int64).reshape(-1)
    return to_bytes(q + 128 if fmt == api.PCM_U8 else q, fmt)


def truth(name):
    """the case's PCM bytes and what sgz_spectrogram_render_host makes of their numpy conversion (computed once, read-only)"""
    if name not in _truth:
        cfg, fmt, channels, cmap, n, want_lines, path = _case(name)
        raw = _signal_bytes(fmt, channels, n, len(name))
        planar = convert_ref(raw, fmt, channels)[cmap if cmap is not None else slice(None)]
        plan = api.Plan(cfg).upload()
        assert plan.path == path, (name, plan.path)
        rgba, lines, _ = api.render_spectrogram_host(plan, planar, want_lines=want_lines)
        plan.close()
        for a in (raw, rgba, lines):
            if a is not None:
                a.setflags(write=False)
        _truth[name] = (raw, rgba, lines)
    return _truth[name]


def _same(got_rgba, got_lines, rgba, lines):
    if not np.array_equal(got_rgba, rgba):
        bad = np.argwhere(got_rgba != rgba)
        return f"image differs at {len(bad)} bytes, first (frame, pixel, byte) {bad[0].tolist()}"
    if lines is not None and not np.array_equal(got_lines.view(np.uint32), lines.view(np.uint32)):
        bad = np.argwhere(got_lines.view(np.uint32) != lines.view(np.uint32))
        return f"lines differ at {len(bad)} words, first {bad[0].tolist()}"
    return ""


@pytest.mark.parametrize("chunk", ["default", 1000, "W+hop-1", 7919])
@pytest.mark.parametrize("name", CASES)
def test_one_shot_equals_host_render(gpu, name, chunk):
    """the whole buffer in one call, cut into pieces of chunk_samples inside: sgz_spectrogram_render_pcm (the default) and one feed of a
    stream with the given chunk_samples"""
    cfg, fmt, channels, cmap, n, want_lines, _ = _case(name)
    raw, rgba, lines = truth(name)
    if chunk == "default":
        st, got_rgba, got_lines, t = api.render_spectrogram_pcm(cfg, raw, fmt, channels, cmap, want_lines=want_lines)
        assert st == api.SGZ_OK and t["chunks"] == 1
    else:
        c = cfg["window_size"] + cfg["hop"] - 1 if chunk == "W+hop-1" else chunk
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=c)
        got_rgba, got_lines, t = s.feed(raw, want_lines=want_lines)
        s.close()
        assert t["chunks"] == -(-n // c)
    assert t["frames"] == rgba.shape[0]
    assert _same(got_rgba, got_lines, rgba, lines) == "", (name, chunk)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("name", CASES[:2])
def test_random_feed_splits_equal_the_one_shot(gpu, name, seed):
    """the stream in random pieces of 0 .. 3 W samples, among them empty and one-sample ones, pieces shorter than the hop and shorter than
    the held tail; frames_for foretells every feed"""
    cfg, fmt, channels, cmap, n, want_lines, _ = _case(name)
    raw, rgba, lines = truth(name)
    W, hop, fb = cfg["window_size"], cfg["hop"], channels * BYTES[fmt]
    rng = np.random.default_rng(seed)
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=[0, 1500, 2 * W + 1][seed - 1])
    at, parts_rgba, parts_lines, sizes = 0, [], [], []
    forced = [1, 0, hop - 1, W, 1, 0, W - hop - 1, 5]             # (whatever the seed: these kinds of pieces, before and after the first frame)
    while at < n:
        kind = rng.integers(0, 6)
        k = [0, 1, int(rng.integers(1, hop)), int(rng.integers(1, W - hop + 1)), int(rng.integers(0, 3 * W + 1)), int(rng.integers(0, 3 * W + 1))][kind]
        k = min(forced.pop(0) if forced else k, n - at)
        need = s.frames_for(k)
        a, b, t = s.feed(raw[at * fb:(at + k) * fb], nsamples=k, want_lines=want_lines)
        assert a.shape[0] == need == t["frames"]
        parts_rgba.append(a)
        parts_lines.append(b)
        sizes.append(k)
        at += k
    s.close()
    assert 0 in sizes and 1 in sizes, sizes
    got_lines = np.concatenate(parts_lines) if want_lines else None
    assert _same(np.concatenate(parts_rgba), got_lines, rgba, lines) == "", (name, seed, sizes)


def test_capacity_reset_short_streams_and_rsnt(gpu):
    name = "fused-s16"
    cfg, fmt, channels, cmap, n, want_lines, _ = _case(name)
    raw, rgba, lines = truth(name)
    W, hop, P, fb = cfg["window_size"], cfg["hop"], cfg["axis_points"], channels * BYTES[fmt]
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=3000)
    # a capacity below the need is refused with the need reported; the same feed then succeeds, unchanged
    first = W + 5 * hop + 17
    need = s.frames_for(first)
    assert need == 6
    small = np.zeros((need - 1, P, 4), np.uint8)
    st, f, _ = s.feed_into(raw, first, small, None, need - 1)
    assert st == api.SGZ_EINVAL and f == need and not small.any() and s.frames_for(first) == need
    st, f, _ = s.feed_into(None, first, small, None, need)
    assert st == api.SGZ_EINVAL and s.frames_for(first) == need                         # a null pcm: nothing consumed either
    a, la, _ = s.feed(raw[:first * fb], want_lines=True)
    b, lb, _ = s.feed(raw[first * fb:], want_lines=True)
    assert _same(np.concatenate([a, b]), np.concatenate([la, lb]), rgba, lines) == ""
    # no reset: a second file continues the first -- the concatenation's render; reset: two renders of their own
    half = (n // 2) * fb
    both = np.concatenate([raw, raw[:half]])
    plan = api.Plan(cfg).upload()
    whole, whole_lines, _ = api.render_spectrogram_host(plan, convert_ref(both, fmt, channels), want_lines=True)
    second, second_lines, _ = api.render_spectrogram_host(plan, convert_ref(raw[:half], fmt, channels), want_lines=True)
    plan.close()
    c, lc, _ = s.feed(raw[:half], want_lines=True)
    assert _same(np.concatenate([a, b, c]), np.concatenate([la, lb, lc]), whole, whole_lines) == ""
    s.reset()
    assert s.frames_for(W - 1) == 0 and s.frames_for(W) == 1
    c, lc, _ = s.feed(raw[:half], want_lines=True)
    assert _same(c, lc, second, second_lines) == ""
    # a stream below W: the feeds are fine and yield nothing; the one-shot call skips
    s.reset()
    for k in (0, 1, hop - 1, W - hop - 1):
        a, _, t = s.feed(raw[:k * fb], nsamples=k)
        assert a.shape[0] == 0 and t["frames"] == 0
    assert s.frames_for(0) == 0 and s.frames_for(1) == 1                                 # W - 1 samples are held
    s.close()
    st, a, _, _ = api.render_spectrogram_pcm(cfg, raw[:(W - 1) * fb], fmt, channels, cmap)
    assert st == api.SGZ_SKIPPED_FRAME and a.shape[0] == 0
    # refusals at create
    for kw, status in ((dict(algorithm=config.ALGO_RSNT), api.SGZ_EUNSUPPORTED), (dict(window_size=0), api.SGZ_EINVAL), (dict(hop=0), api.SGZ_EINVAL)):
        with pytest.raises(api.SgzError) as e:
            api.PcmStream(dict(cfg, **kw), fmt, channels, cmap)
        assert e.value.status == status, kw
    for args in ((api.PCM_END, 2, None), (fmt, 0, None), (fmt, 65, None), (fmt, 1, None), (fmt, 2, [0, 2])):
        with pytest.raises(api.SgzError) as e:
            api.PcmStream(cfg, *args)
        assert e.value.status == api.SGZ_EINVAL, args


def test_pinned_memory_gives_the_same_bytes(gpu):
    import torch
    for name in ("fused-s16", "split-f32-image"):
        cfg, fmt, channels, cmap, n, want_lines, _ = _case(name)
        raw, rgba, lines = truth(name)
        pcm = torch.from_numpy(raw.copy()).pin_memory()
        out = torch.zeros(rgba.shape, dtype=torch.uint8).pin_memory()
        out_lines = torch.zeros(lines.shape, dtype=torch.float32).pin_memory() if want_lines else None
        s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=5000)
        st, f, t = s.feed_into(pcm, n, out, out_lines, rgba.shape[0])
        s.close()
        assert st == api.SGZ_OK and f == rgba.shape[0] and t.chunks == -(-n // 5000)
        assert _same(out.numpy(), out_lines.numpy() if want_lines else None, rgba, lines) == "", name


def test_feed_beside_a_background_render(gpu):
    """another plan's renders in flight on a stream of their own while the feed runs"""
    import torch
    name = "split-f32-image"
    cfg, fmt, channels, cmap, n, want_lines, _ = _case(name)
    raw, rgba, lines = truth(name)
    other = api.Plan(config.spectrum_config(window_size=32768, hop=8192)).upload()
    x = torch.randn((2, 32768 + 299 * 8192), device=gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    s = api.PcmStream(cfg, fmt, channels, cmap, chunk_samples=20000)
    outs = [other.render(x, stream=side.cuda_stream) for _ in range(6)]
    got, _, _ = s.feed(raw)
    side.synchronize()
    s.close()
    assert _same(got, None, rgba, None) == ""
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    other.close()


def test_create_feed_destroy_gives_the_memory_back(gpu):
    """200 create -> feed -> destroy cycles after 5 to settle the allocators: the device's free memory ends where it was (64 MiB of slack, as
    test_gpu_lifecycle.py: the runtime's own pools move by a few MiB)"""
    import os

    import torch
    cfg = config.spectrum_config(window_size=1024, hop=256, axis_points=128)
    raw = _signal_bytes(api.PCM_S16, 2, 1024 + 20 * 256, 9)

    def cycle():
        s = api.PcmStream(cfg, api.PCM_S16, 2, chunk_samples=2000)
        a, b, _ = s.feed(raw, want_lines=True)
        s.close()
        return a

    first = [cycle() for _ in range(5)][0]
    gc.collect()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(200):
        assert np.array_equal(cycle(), first)
    gc.collect()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    if "PYTEST_XDIST_WORKER" not in os.environ:                   # (the figure is the DEVICE's: under pytest -n the other workers' allocations move it)
        assert free0 - free1 < 64 << 20, f"device memory: {(free0 - free1) / 2**20:.1f} MiB fewer free after 200 cycles"
