"""What the interleaved-PCM front of the offline render costs, on cfg2's buffer (stereo, 2 880 000 samples, N = W = 32768, hop 8192: 348 frames).
    python tools/bench_pcm_render.py [--reps 7] [--out gpu_out/pcm_render.json]
  (a) the path a caller had to run before from an interleaved S16 buffer: numpy de-interleave + convert to planar fp32, then
      sgz_spectrogram_render_host on a plan it keeps -- conversion and render apart and together; and with sgz_spectrogram_render (the
      plan built inside the call), the like of (b)'s one-shot call
  (b) the same S16 buffer through the PCM front: sgz_spectrogram_render_pcm (plan and stream built inside the call), and one feed of a kept
      sgz_pcm_stream (reset between files) from pageable S16, from its F32 interleaved form, and from pinned memory (source and image)
  (c) a kept stream at chunk_samples 2^16 .. 2^22, pageable S16; and a stream eight times as long (the buffer fed eight times without reset)
      per sample beside the short one
  (d) the converter alone, S16 stereo and the other formats: 20 launches after 3 warm-ups between events, median, as bytes moved (read +
      written) per second; on a buffer of 64 Mi samples so that the source does not sit in the 256 MiB Infinity Cache
Wall times are the host's clock around the call, median of --reps after one warm-up."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from signalizer_amd import api, config, synth


def med(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = config.cfg2()
    S = int(config.CFG2_SECONDS * 48000)
    x = synth.gen(config.CFG2_SEED, 48000, S, 2)
    s16 = np.ascontiguousarray(np.clip(np.round(x.T * 32768.0), -32768, 32767).astype(np.int16))          # [S][2] interleaved
    f32 = np.ascontiguousarray(s16.astype(np.float32) * np.float32(2.0 ** -15))
    res = {"samples": S, "frames": int(api.lib().sgz_num_frames(S, cfg["window_size"], cfg["hop"]))}

    # (a)
    plan = api.Plan(cfg).upload()
    conv = lambda: np.ascontiguousarray(s16.T).astype(np.float32) * np.float32(2.0 ** -15)
    planar = conv()
    ref, _, _ = api.render_spectrogram_host(plan, planar)
    res["a_numpy_convert_ms"] = med(conv, a.reps)
    res["a_render_host_ms"] = med(lambda: api.render_spectrogram_host(plan, planar), a.reps)
    res["a_together_ms"] = med(lambda: api.render_spectrogram_host(plan, conv()), a.reps)
    _, _, t = api.render_spectrogram_host(plan, planar)
    res["a_render_host_stages"] = t
    res["a_one_shot_together_ms"] = med(lambda: api.render_spectrogram(cfg, conv()), a.reps)       # the plan built inside the call, as (b)'s one-shot

    # (b)
    got = api.render_spectrogram_pcm(cfg, s16, api.PCM_S16, 2)[1]
    res["b_equals_a"] = bool(np.array_equal(got, ref))
    res["b_one_shot_s16_ms"] = med(lambda: api.render_spectrogram_pcm(cfg, s16, api.PCM_S16, 2), a.reps)
    F, P = ref.shape[0], ref.shape[1]
    out = np.zeros((F, P, 4), np.uint8)

    def kept(stream, pcm, n, dst, timing=False):
        stream.reset()
        st, f, t = stream.feed_into(pcm, n, dst, None, F * (n // S), timing=timing)
        assert st == 0, st
        return t

    st16 = api.PcmStream(cfg, api.PCM_S16, 2)
    res["b_kept_s16_ms"] = med(lambda: kept(st16, s16, S, out), a.reps)
    res["b_kept_s16_stages"] = kept(st16, s16, S, out, timing=True).asdict()
    assert np.array_equal(out, ref)
    st32 = api.PcmStream(cfg, api.PCM_F32, 2)
    res["b_kept_f32_ms"] = med(lambda: kept(st32, f32, S, out), a.reps)
    st32.close()
    pin = torch.from_numpy(s16).pin_memory()
    pout = torch.zeros((F, P, 4), dtype=torch.uint8).pin_memory()
    res["b_kept_s16_pinned_ms"] = med(lambda: kept(st16, pin, S, pout), a.reps)
    res["b_kept_s16_pinned_stages"] = kept(st16, pin, S, pout, timing=True).asdict()
    assert np.array_equal(pout.numpy(), ref)
    st16.close()

    # (c)
    res["c_chunk_sweep_ms"] = {}
    for lg in range(16, 23):
        s = api.PcmStream(cfg, api.PCM_S16, 2, chunk_samples=1 << lg)
        res["c_chunk_sweep_ms"][f"2^{lg}"] = med(lambda: kept(s, s16, S, out), a.reps)
        s.close()
    long16 = np.ascontiguousarray(np.concatenate([s16] * 8))
    s = api.PcmStream(cfg, api.PCM_S16, 2)
    nl = long16.shape[0]
    Fl = s.frames_for(nl)
    lout = np.zeros((Fl, P, 4), np.uint8)

    def long_feed():
        s.reset()
        st, f, t = s.feed_into(long16, nl, lout, None, Fl, timing=False)
        assert st == 0 and f == Fl
    long_ms = med(long_feed, max(3, a.reps // 2))
    s.close()
    res["c_long_stream"] = {"samples": nl, "ms": long_ms, "ns_per_sample": round(long_ms * 1e6 / nl, 3),
                            "short_ns_per_sample": round(res["b_kept_s16_ms"] * 1e6 / S, 3)}

    # (d)
    n = 64 << 20
    res["d_converter"] = {}
    for fmt, name in ((api.PCM_S16, "s16"), (api.PCM_S24, "s24"), (api.PCM_F32, "f32"), (api.PCM_U8, "u8"), (api.PCM_S32, "s32"), (api.PCM_F64, "f64")):
        sb = api.PCM_SAMPLE_BYTES[fmt]
        src = torch.randint(0, 256, (n * 2 * sb,), dtype=torch.uint8, device="cuda:0")
        dst = torch.empty((2, n), dtype=torch.float32, device="cuda:0")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = []
        for k in range(23):
            ev[0].record()
            api.pcm_to_planar_device(src, fmt, 2, n, dst)
            ev[1].record()
            ev[1].synchronize()
            if k >= 3:
                ts.append(ev[0].elapsed_time(ev[1]))
        ms = statistics.median(ts)
        moved = n * 2 * (sb + 4)
        res["d_converter"][name] = {"ms": round(ms, 4), "bytes_moved": moved, "tb_per_s": round(moved / ms / 1e9, 3)}
        del src, dst
    plan.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
