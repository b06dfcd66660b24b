#!/usr/bin/env python3
"""bench.py -- 32768-pt stereo STFT frames/sec (75 % overlap) on MI355X, BASELINE.json metric.

A "step" = one pass of the whole Spectrum hot path (window x audio -> FFT -> split -> |X| -> log-frequency
pixel mapping -> peak decay -> dB -> colour map -> RGBA8 columns) over BASELINE.json configs[1]:
stereo 48 kHz, 60 s, N = W = 32768, hop 8192 => 348 frames, P = 1024.  Audio is resident in HBM when the
timed region starts.  N GPUs: time-chunk sharding -- every rank renders its own 60 s chunk of a
60*N s stream (weak scaling); halo samples travel neighbour to neighbour (ncclSend / ncclRecv), the decay carry in one RCCL
all-gather; `--workload cfg5` splits ONE 64-channel 65536-pt job over the ranks instead (strong scaling).

  python bench.py --gpus 1 --steps 200 --warmup 20
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK_GBPS = 8000.0            # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md
DUMP_LIMIT_BYTES = 64 << 20       # --dump-outputs: all files of one run together


def dump_outputs(directory: str, arrays: dict, limit: int = DUMP_LIMIT_BYTES) -> None:
    """--dump-outputs: what the last timed step computed, each array as DIR/<name>.npy in float32 (float64 stays float64; RGBA8 bytes
    convert exactly).  Every array gets an equal share of `limit`; one larger than its share is written as a fixed, seeded sample of its
    elements (flattened; the same positions on every run), so that two builds can be compared output for output."""
    os.makedirs(directory, exist_ok=True)
    share = limit // max(len(arrays), 1) - 4096                         # (room for the .npy header)
    for name, a in arrays.items():
        a = np.asarray(a)
        a = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share // a.itemsize, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(directory, name + ".npy"), np.ascontiguousarray(a))


def _hip():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return ctypes.CDLL(name)
        except OSError:
            continue
    raise RuntimeError("libamdhip64.so not found")


class HipEvents:
    """HIP events on an explicit stream (torch.cuda.Event only sees torch's current stream)."""

    def __init__(self, n: int):
        self.h = _hip()
        self.ev = [ctypes.c_void_p() for _ in range(n)]
        for e in self.ev:
            assert self.h.hipEventCreate(ctypes.byref(e)) == 0

    def record(self, i: int, stream: int):
        assert self.h.hipEventRecord(self.ev[i], ctypes.c_void_p(stream)) == 0

    def elapsed_ms(self, a: int, b: int) -> float:
        ms = ctypes.c_float()
        assert self.h.hipEventSynchronize(self.ev[b]) == 0
        assert self.h.hipEventElapsedTime(ctypes.byref(ms), self.ev[a], self.ev[b]) == 0
        return float(ms.value)


def measured_traffic():
    """HBM bytes per K_A launch from the last committed PMC pass (tools/profile.sh -> profiles/traffic_latest.json;
    rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes, gfx950 correction applied), or None."""
    try:
        with open(os.path.join(ROOT, "profiles", "traffic_latest.json")) as fh:
            return int(json.load(fh)["traffic_bytes_per_launch"])
    except (OSError, KeyError, ValueError):
        return None


def _native_oracle():
    """the oracle built for THIS host's ISA (gcc -O3 -march=native, contraction allowed) in a temp dir: timing only;
    None when the build fails"""
    import subprocess
    import tempfile
    try:
        out = os.path.join(tempfile.mkdtemp(prefix="sgz_oracle_native_"), "libsgz_oracle_native.so")
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "native", f"OUT={out}"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        L = ctypes.CDLL(out)
        L.sgzo_spectrogram_range.restype = ctypes.c_long
        return L
    except Exception:                                              # noqa: BLE001 -- no compiler on the box, unknown -march: report the strict build only
        return None


def cpu_baseline(cfg: dict, x: np.ndarray, budget_s: float = 14.0) -> dict:
    """The CPU oracle (a restatement: 'port') timed on this host, 1 thread (the reference transforms one stereo pair on one thread,
    SpectrumDSP.cpp:83), on a bounded sample of the same workload: the first frames of the same buffer, ~budget_s of CPU work in all.
    Two builds of the same C: the parity build (gcc -O3, strict fp, generic x86-64) and the host's own (gcc -O3 -march=native, contraction
    allowed -- SURVEY.md 8(d)); `value` is the faster."""
    from oracle import pyoracle as po
    p = po.params_from_dict(cfg)
    xs = np.ascontiguousarray(x, np.float32)
    ptrs = (ctypes.c_void_p * xs.shape[0])(*[xs[c].ctypes.data for c in range(xs.shape[0])])

    def run(L, nfr):
        t0 = time.perf_counter()
        L.sgzo_spectrogram_range(ctypes.byref(p), ptrs, ctypes.c_size_t(xs.shape[1]), ctypes.c_long(0), ctypes.c_long(nfr), None)
        return time.perf_counter() - t0

    builds = [("strict", po.lib())]
    nat = _native_oracle()
    if nat is not None:
        builds.append(("native", nat))
    rates = {}
    nfr_used = 0
    for name, L in builds:
        per = run(L, 4) / 4
        nfr = int(max(8, min(348, (budget_s / len(builds)) / max(per, 1e-6))))
        rates[name] = nfr / run(L, nfr)
        nfr_used = max(nfr_used, nfr)
    best = max(rates, key=rates.get)
    # the same chain on a transform the compiler vectorises (oracle/fft_simd.c: radix-4 Stockham on split arrays) -- the reference's
    # transform is pffft (SIMD), so the port's scalar radix-2 alone would overstate the GPU / CPU ratio by about the vector width
    sb, sL = ("native", nat) if nat is not None else ("strict", po.lib())
    sL.sgzo_spectrogram_range_simd.restype = ctypes.c_long

    def run_simd(nfr):
        t0 = time.perf_counter()
        sL.sgzo_spectrogram_range_simd(ctypes.byref(p), ptrs, ctypes.c_size_t(xs.shape[1]), ctypes.c_long(0), ctypes.c_long(nfr), None)
        return time.perf_counter() - t0

    per = run_simd(4) / 4
    nfr_simd = int(max(8, min(348, 5.0 / max(per, 1e-6))))
    flags = "gcc -O3 -march=native -ffp-contract=fast" if sb == "native" else "gcc -O3 -ffp-contract=off (generic x86-64)"
    simd = {"simd_value": nfr_simd / run_simd(nfr_simd), "simd_kind": "port-simd-fft", "simd_cores": 1,
            "simd_sample": f"first {nfr_simd} of 348 frames, 1 thread, {sb} build ({flags}): the port with its radix-2 transform replaced by "
                           f"oracle/fft_simd.c (radix-4 Stockham, split re / im arrays, auto-vectorised); every other stage unchanged"}
    try:
        simd.update(cpu_baseline_third_party_fft(cfg, xs, sL, sb))
    except Exception as e:                                          # noqa: BLE001 -- a third opinion: scipy absent or changed must not cost the line
        simd["third_party_fft_value"] = None
        simd["third_party_fft_sample"] = f"not measured: {e}"
    return {"value": rates[best], "unit": "frames/s", "cores": 1, "kind": "port", "build": best,
            "strict_build_value": rates["strict"], "native_build_value": rates.get("native"), **simd,
            "sample": f"first {nfr_used} (at most) of 348 frames of the same 60 s stereo buffer, oracle/*.c (scalar radix-2 FFT): parity build gcc -O3 strict fp "
                      f"and host build gcc -O3 -march=native, 1 thread of {os.cpu_count()} (the reference runs one thread per stereo pair)"}


def cpu_baseline_third_party_fft(cfg: dict, xs: np.ndarray, L, build: str, budget_s: float = 4.0) -> dict:
    """The same chain with the transform on a SIMD FFT, as the reference's is (TransformDSP.inl:487-502 -> cpl::dsp::UniFFT -> pffft,
    SSE / AVX; absent here): window / pack, pixel mapping, decay + dB and the colour blend stay the oracle's C (build `build`), the
    32768-point complex transform is scipy.fft's pocketfft (C++, complex64, workers=1; pocketfft vectorises ACROSS transforms, a single
    1-D transform runs its scalar kernels).  A third opinion beside the port and the port on fft_simd.c; the first frame's bins are
    held to the port's transform (relative to the largest bin)."""
    import ctypes as C
    import scipy
    import scipy.fft
    from oracle import pyoracle as po
    vp = C.c_void_p
    L.sgzo_window.restype = C.c_double
    L.sgzo_window.argtypes = [C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_uint32, vp]
    L.sgzo_map_to_linear_space.argtypes = [C.POINTER(po.SpectrumParams), vp, C.c_double, vp, C.c_uint32, vp]
    L.sgzo_prepare_transform.argtypes = [C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32, vp]
    L.sgzo_blend_column.argtypes = [C.POINTER(po.SpectrumParams), vp, vp, C.c_uint32, vp]
    p = po.params_from_dict(cfg)
    W, P, hop = p.window_size, p.axis_points, p.hop
    N = W
    ptr = lambda a: a.ctypes.data_as(vp)                                     # noqa: E731
    window = np.zeros(N, np.float32)
    scale = L.sgzo_window(p.window_type, p.window_symmetry, p.window_alpha, p.window_beta, W, ptr(window))
    mapped, slope, ratios = np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(po.NUM_SPEC_COLOURS + 1, np.float32)
    L.sgzo_remap_frequencies(C.byref(p), ptr(mapped))
    L.sgzo_slope_map(C.byref(p), ptr(mapped), ptr(slope))
    L.sgzo_colour_ratios(ptr(np.asarray([p.ratios[i] for i in range(po.NUM_SPEC_COLOURS)], np.float64)), ptr(ratios))
    csf = np.zeros(N + 1, np.complex64)
    csp = np.zeros(2 * P, np.complex64)
    states = np.zeros((po.NUM_GRAPHS, P), np.complex64)
    results = np.zeros((po.NUM_GRAPHS, P), np.complex64)
    rgba = np.zeros((P, 4), np.uint8)
    total = (xs.shape[1] - W) // hop + 1
    bin_err = [0.0]

    def run(nfr, check=False):
        states[:] = 0
        t0 = time.perf_counter()
        for f in range(nfr):
            s = f * hop
            L.sgzo_prepare_transform(p.channel_mode, ptr(xs[0, s:]), ptr(xs[1, s:]), ptr(window), W, N, ptr(csf))
            if check:
                want = po.fft32(csf[:N])
            csf[:N] = scipy.fft.fft(csf[:N], workers=1)
            csf[N] = 0
            if check:
                bin_err[0] = float(np.max(np.abs(csf[:N] - want)) / np.max(np.abs(want)))
            csp[:] = 0
            L.sgzo_map_to_linear_space(C.byref(p), ptr(mapped), scale, ptr(csf), N, ptr(csp))
            L.sgzo_map_and_transform_filters(C.byref(p), ptr(slope), ptr(csp), ptr(states), ptr(results))
            L.sgzo_blend_column(C.byref(p), ptr(ratios), ptr(results), 1, ptr(rgba))
        return time.perf_counter() - t0

    assert scipy.fft.fft(csf[:N], workers=1).dtype == np.complex64
    run(1, check=True)
    per = run(4) / 4
    nfr = int(max(8, min(total, budget_s / max(per, 1e-6))))
    rate = nfr / run(nfr)
    return {"third_party_fft_value": rate,
            "third_party_fft_sample": f"first {nfr} of {total} frames of the same buffer, 1 thread: scipy.fft {scipy.__version__} (pocketfft, complex64, workers=1) for the "
                           f"{N}-point transform, every other stage oracle/*.c ({build} build: "
                           f"{'gcc -O3 -march=native -ffp-contract=fast' if build == 'native' else 'gcc -O3 -ffp-contract=off'}); "
                           f"first frame's bins vs the port's transform: {bin_err[0]:.1e} of the largest bin"}


def cpu_baseline_pairs(cfg: dict, x: np.ndarray, budget_s: float = 12.0) -> dict:
    """cfg5's CPU baseline: the reference parallelises across stereo pairs only (SpectrumDSP.cpp:83), so the
    oracle runs one thread per pair, min(pairs, cores) at a time (ctypes releases the GIL around the C calls), each on its own pair's
    two channels; the cross-pair colour blend (SpectrumDSP.cpp:177-180, a few operations per pixel) is left out of the timed sample."""
    import concurrent.futures as cf
    from oracle import pyoracle as po
    pairs = cfg["num_pairs"]
    cores = os.cpu_count() or 1
    threads = max(1, min(pairs, cores))
    one = dict(cfg, num_pairs=1)
    p = po.params_from_dict(one)
    W, hop = cfg["window_size"], cfg["hop"]
    total = (x.shape[1] - W) // hop + 1

    def job(pair, nfr):
        po.spectrogram_range(p, np.ascontiguousarray(x[2 * pair:2 * pair + 2]), 0, nfr)

    t0 = time.perf_counter()
    job(0, 2)
    per = (time.perf_counter() - t0) / 2                        # seconds per (frame, pair) on one thread
    rounds = -(-pairs // threads)
    nfr = int(max(2, min(total, budget_s / max(per * rounds, 1e-6))))
    t0 = time.perf_counter()
    with cf.ThreadPoolExecutor(max_workers=threads) as ex:
        list(ex.map(lambda pr: job(pr, nfr), range(pairs)))
    dt = time.perf_counter() - t0
    return {"value": nfr / dt, "unit": "frames/s", "cores": threads, "kind": "port",
            "sample": f"first {nfr} of {total} frames of all {pairs} pairs of the same 60 s buffer, oracle/libsgz_oracle.so (gcc -O3, strict fp), "
                      f"one thread per pair, {threads} at a time, of {cores} cores; the cross-pair colour blend is not in the sample"}


class CAbiShard:
    """this rank's share of the job through sgz_spectrogram_render_sharded on an RCCL communicator of its own (the ids travel over
    torch.distributed, which is only the launcher's rendezvous here)"""

    def __init__(self, plan, chunk, rank, world, dev, rotate_bytes=0):
        import ctypes as C
        import torch
        import torch.distributed as dist
        from signalizer_amd import api
        self.C, self.torch, self.api, self.plan, self.rank, self.world = C, torch, api, plan, rank, world
        L = api.lib()
        uid = (C.c_uint8 * 128)()
        if rank == 0:
            api.check(L.sgz_comm_unique_id(uid))
        t = torch.tensor(list(uid), dtype=torch.uint8, device=dev)
        dist.broadcast(t, 0)
        uid = (C.c_uint8 * 128)(*t.cpu().tolist())
        self.comm = C.c_void_p()
        api.check(L.sgz_comm_create(uid, rank, world, C.byref(self.comm)))
        nch, S = chunk.shape
        self.S = S
        self.buf = torch.zeros((nch, (S + plan.cfg.window_size + 63) // 64 * 64), dtype=torch.float32, device=dev)
        self.buf[:, :S] = chunk
        self.bufs = [self.buf] + [self.buf.clone() for _ in range(max(0, -(-rotate_bytes // (self.buf.numel() * 4)) - 1))] if rotate_bytes > 0 else [self.buf]
        self.turn = 0
        lf = C.c_uint64(0)
        api.check(L.sgz_shard_layout(plan.h, rank, world, S, C.byref(lf), None, None, None))
        self.local_frames = int(lf.value)
        self.rgba = torch.empty((max(self.local_frames, 1), plan.P, 4), dtype=torch.uint8, device=dev)

    def render(self):
        lf = self.C.c_uint64(0)
        self.turn = (self.turn + 1) % len(self.bufs)
        self.buf = self.bufs[self.turn]
        self.api.check(self.api.lib().sgz_spectrogram_render_sharded(
            self.plan.h, self.comm, self.rank, self.world, self.buf.data_ptr(), self.buf.stride(0), self.S, self.rgba.data_ptr(),
            self.C.byref(lf), self.torch.cuda.current_stream().cuda_stream))
        return self.rgba

    def close(self):
        self.api.lib().sgz_comm_destroy(self.comm)


def views_workload(args, rank, world, dev, workload=None, steps=None, emit=True):
    """BASELINE configs[2] (Oscilloscope) / configs[3] (Vectorscope) through the real-time handles, the way the plugin would drive
    them: per rendered frame (60 Hz) the audio thread's callbacks (512 samples each, host buffers in) and then the render thread's
    calls (peak filter, vertices of every channel / pair, host buffers out).  The handles own their streams and `vertices` waits for
    its result, so a step is timed on the host clock; the dominant kernel is timed separately through its stateless stage call on
    the launch stream with HIP events (same view, same data volume) for the roofline object."""
    import ctypes as C
    import torch
    from signalizer_amd import api, synth
    L = api.lib()
    scope = (workload or args.workload) == "cfg3"
    nsteps = steps or args.steps
    if scope:
        sr, W, nch = 192000.0, 19200, 2
        per_frame = int(sr / 60)
        width = 8 * W + 1
        h = api.Scope(sample_rate=sr, window_size=float(W), num_channels=nch, trigger_mode=4, channel_mode=0, envelope_mode=2,
                      interpolation=3, max_block=512, trigger_threshold=0.05, trigger_channel=1.0, envelope_window=0.3)
        view = api.ScopeView(float(W), 0.0, 1.0, 1.0, width, 0)
    else:
        sr, W, nch = 96000.0, 9600, 8
        per_frame = int(sr / 60)
        h = api.Vector(sample_rate=sr, num_channels=nch, window_size=W, envelope_mode=2, lanes=8, fade_history=1, max_block=512,
                       envelope_window=0.3, stereo_window=0.1)
    x = synth.gen(31 + rank, int(sr), per_frame * 64, nch)
    refused = 0
    # the vertex streams are read back into pinned buffers the caller keeps (what a plugin's render thread would hand to glBufferSubData)
    pinned = lambda shape, dt: torch.empty(shape, dtype=dt).pin_memory().numpy()
    if scope:
        nv = L.sgz_scope_vertex_count(h.h, ctypes.byref(view))
        outs = [(pinned((nv, 3), torch.float32), pinned((nv, 4), torch.uint8)) for _ in (0, 1)]
    else:
        outs = (pinned((nch // 2, W, 3), torch.float32), pinned((nch // 2, W, 3), torch.float32))

    def push(block):
        nonlocal refused
        while h.push(block) == api.SGZ_BUSY:                       # never waits; a refused block is offered again
            refused += 1

    frame = 0
    units = 0

    def step():
        nonlocal frame, units
        a = (frame % 64) * per_frame
        for pos in range(a, a + per_frame, 512):
            push(x[:, pos:min(pos + 512, a + per_frame)])
        if scope:
            h.peak_filter(1 / 60, 8)
            n = sum(xyz.shape[0] for xyz, _ in h.vertices_all(view, (0, 1), (0, 0), outs))      # both channels' strips, one wait
        else:
            h.peak_filter(1 / 60)
            xyz, _ = h.vertices_all(out=outs)                      # every pair's vertex stream, one wait for the GPU
            n = xyz.shape[0] * xyz.shape[1]
        frame += 1
        units = n

    for _ in range(max(args.warmup, 70)):                          # at least one lap of the signal: rings full, triggers running
        step()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(nsteps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt_python = time.perf_counter() - t0

    def last_step():                                               # --dump-outputs: the caller's destination buffers as the last step left them
        if scope:
            return {f"{k}_ch{c}": np.array(a) for c, (xyz, col) in enumerate(outs) for k, a in (("xyz", xyz), ("rgba", col))}
        return {"xyz": np.array(outs[0]), "rgb": np.array(outs[1])}
    dump = last_step() if args.dump_outputs and emit else None
    # the same loop with the host side in C++ (tools/rt_driver.cpp -> signalizer_amd/librtdriver.so: what a plugin's audio callback and
    # paint would execute; the Python loop above pays 60-100 us of interpreter and ctypes time per frame on top of the library's own)
    dt = dt_python
    host = "python"
    dt_resident = None
    from signalizer_amd import build as sgz_build
    if os.path.exists(sgz_build.DRIVER) and not os.environ.get("SGZ_LIB"):
        D = C.CDLL(sgz_build.DRIVER)
        busy, verts = C.c_uint64(0), C.c_uint32(0)
        xc = np.ascontiguousarray(x)
        if scope:
            D.sgz_bench_scope_loop.restype = C.c_double
            ev = (C.c_uint32 * 2)(0, 1); ch = (C.c_uint32 * 2)(0, 0)

            def loop(xs, cs):                                      # the destination arrays are arguments: no late binding of rebound names
                return lambda warm, n: D.sgz_bench_scope_loop(h.h, C.c_void_p(xc.ctypes.data), C.c_size_t(xc.shape[1]), C.c_uint32(nch), C.c_uint32(per_frame),
                                                              C.c_uint32(512), C.c_uint32(64), C.byref(view), C.c_uint32(2), ev, ch, xs, cs, C.c_uint32(nv),
                                                              C.c_double(1 / 60), C.c_uint32(8), C.c_int(warm), C.c_int(n), C.byref(busy), C.byref(verts))
            run = loop((C.c_void_p * 2)(outs[0][0].ctypes.data, outs[1][0].ctypes.data), (C.c_void_p * 2)(outs[0][1].ctypes.data, outs[1][1].ctypes.data))
        else:
            D.sgz_bench_vector_loop.restype = C.c_double

            def loop(xyz_ptr, rgb_ptr):
                return lambda warm, n: D.sgz_bench_vector_loop(h.h, C.c_void_p(xc.ctypes.data), C.c_size_t(xc.shape[1]), C.c_uint32(nch), C.c_uint32(per_frame),
                                                               C.c_uint32(512), C.c_uint32(64), C.c_void_p(xyz_ptr), C.c_void_p(rgb_ptr),
                                                               C.c_uint32(W), C.c_double(1 / 60), C.c_int(warm), C.c_int(n), C.byref(busy), C.byref(verts))
            run = loop(outs[0].ctypes.data, outs[1].ctypes.data)
        if world > 1:
            dist.barrier()
        d = run(70, nsteps)
        if world > 1:
            dist.barrier()
        if d < 0:
            raise RuntimeError(f"rt_driver: C-ABI call failed ({d})")
        dt, host = float(d), "c++ (tools/rt_driver.cpp)"
        if dump is not None:
            dump = last_step()
        refused += busy.value
        assert verts.value == units, (verts.value, units)
        # the same frames with the vertex streams left in HBM (caller-owned DEVICE buffers: a mapped vertex buffer object / exported memory
        # the display GPU imported -- SURVEY 8(f) #1): nothing crosses PCIe on the way out
        busy.value, verts.value = 0, 0
        if scope:
            dxs = [torch.empty((nv, 3), dtype=torch.float32, device=dev) for _ in (0, 1)]
            dcs = [torch.empty((nv, 4), dtype=torch.uint8, device=dev) for _ in (0, 1)]
            run_resident = loop((C.c_void_p * 2)(dxs[0].data_ptr(), dxs[1].data_ptr()), (C.c_void_p * 2)(dcs[0].data_ptr(), dcs[1].data_ptr()))
        else:
            dxyz = torch.empty((nch // 2, W, 3), dtype=torch.float32, device=dev); drgb = torch.empty((nch // 2, W, 3), dtype=torch.float32, device=dev)
            run_resident = loop(dxyz.data_ptr(), drgb.data_ptr())
        d2 = run_resident(20, nsteps)
        if d2 < 0:
            raise RuntimeError(f"rt_driver (device-resident): C-ABI call failed ({d2})")
        refused += busy.value
        assert verts.value == units, (verts.value, units)
        dt_resident = float(d2)
    if dump is not None:
        dump_outputs(args.dump_outputs, {(k if world == 1 else f"{k}_rank{rank}"): a for k, a in dump.items()}, DUMP_LIMIT_BYTES // world)
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    # The kernel that dominates the timed step (profiles/r05*/cfg{3,4}_kernel_summary.txt), timed on the HANDLE's own stream with HIP
    # events around the call that launches it, SURVEY 8(d)'s bytes:
    #   cfg3: scopeWaveLanczosKernel<2>, both channel strips in one launch (2 x (19 200 samples in, 153 601 vertices x 12 B + colours out)), with
    #         the strips going to HBM (kernel_ms) and to the caller's pinned buffers over PCIe (kernel_ms_pinned_destination);
    #   cfg4: vectorIngestKernel, one launch per 512-sample callback of 8 channels when the GPU keeps up (ring + eight one-pole filters).
    hstream = (L.sgz_scope_stream if scope else L.sgz_vector_stream)(h.h)
    ev = HipEvents(2)
    h.flush()
    torch.cuda.synchronize()
    extra_kernel = {}
    if scope:
        dxs = [torch.empty((nv, 3), dtype=torch.float32, device=dev) for _ in (0, 1)]
        dcs = [torch.empty((nv, 4), dtype=torch.uint8, device=dev) for _ in (0, 1)]
        evs = (C.c_uint32 * 2)(0, 1); chs = (C.c_uint32 * 2)(0, 0)

        def strips(xptrs, cptrs, reps=30):
            cnts = (C.c_uint32 * 2)(nv, nv)
            tot = 0.0
            for _ in range(reps):
                cnts[0] = cnts[1] = nv
                ev.record(0, hstream)
                api.check(L.sgz_scope_vertices_all(h.h, C.byref(view), 2, evs, chs, xptrs, cptrs, cnts))
                ev.record(1, hstream)
                torch.cuda.synchronize()
                tot += ev.elapsed_ms(0, 1)
            return tot / reps                                           # ONE launch for both strips (shared tap weights)
        kern_ms = strips((C.c_void_p * 2)(dxs[0].data_ptr(), dxs[1].data_ptr()), (C.c_void_p * 2)(dcs[0].data_ptr(), dcs[1].data_ptr()))
        extra_kernel["kernel_ms_pinned_destination"] = strips((C.c_void_p * 2)(outs[0][0].ctypes.data, outs[1][0].ctypes.data),
                                                              (C.c_void_p * 2)(outs[0][1].ctypes.data, outs[1][1].ctypes.data))
        alg = 2 * (W * 4 + nv * 12)
        kname = "scopeWaveLanczosKernel<2> (both channels' strips in one launch, shared tap weights; vertices + colours to HBM)"
    else:
        blk = np.ascontiguousarray(x[:, :512])
        tot, reps = 0.0, 60
        for _ in range(reps):
            h.flush()
            torch.cuda.synchronize()
            ev.record(0, hstream)
            push(blk)                                                   # an idle handle starts the block at once: one vectorIngestKernel
            ev.record(1, hstream)
            torch.cuda.synchronize()
            tot += ev.elapsed_ms(0, 1)
        kern_ms = tot / reps
        alg = nch * 512 * 4 * 2                                         # 512 samples of 8 channels in, the same into the history ring
        kname = "vectorIngestKernel (one 512-sample callback of 8 channels per launch)"
    if rank == 0:
        achieved = alg / (kern_ms * 1e-3) / 1e9
        out = {
            "metric": ("oscilloscope vertices/sec: Lanczos-10 8x resample + zero-crossing trigger, stereo 192 kHz, 100 ms window" if scope else
                       "vectorscope vertices/sec: L/R -> polar + envelope decay, 8-channel 96 kHz, 100 ms window"),
            "value": units * world * nsteps / dt, "unit": "vertices/s", "n_gpus": world, "steps": nsteps, "warmup": args.warmup,
            "ms_per_step": dt / nsteps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32 (f64 kernel weights)" if scope else "f32",
            "data": "synthetic",
            "config": {"workload": ("BASELINE.json configs[2]: Oscilloscope, stereo 192 kHz, 19 200-sample window, zero-crossing trigger at 0.05, "
                                    "Lanczos-10 at 8 points per sample (153 601 vertices per channel), peak-decay envelope" if scope else
                                    "BASELINE.json configs[3]: Vectorscope, 8 channels (4 pairs) 96 kHz, 9 600-sample history, peak-decay envelope, fade colours"),
                       "step": "one rendered frame at 60 Hz through the real-time handle: 1/60 s of audio in 512-sample callbacks from host buffers "
                               "(one staged copy + one kernel each), then peak filter and the vertices of every channel / pair into host buffers "
                               "(vectorscope: sgz_vector_vertices_all, one wait for the four pairs)",
                       "parallelism": "replicas only" if world > 1 else "single device", "vertices_per_step": units,
                       "realtime_factor": (1 / 60) / (dt / nsteps), "pushes_refused_busy": refused, "host_loop": host,
                       "ms_per_step_python_host": dt_python / nsteps * 1e3,
                       "ms_per_step_device_resident": (dt_resident / nsteps * 1e3) if dt_resident is not None else None,
                       "device_resident_note": "the same frames with every vertex stream written to caller-owned DEVICE buffers (sgz_*_vertices_all on device memory)"},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
                         "traffic": None, "kernel": kname, "kernel_ms": kern_ms, "algorithmic_bytes_per_launch": alg, **extra_kernel,
                         "note": "the kernel that dominates the timed step, HIP events on the handle's stream around the call that launches it "
                                 "(an event pair around one launch includes ~2 us of event overhead); a few MB per launch at most: bound by launch "
                                 "latency, the PCIe stores (pinned destination) and (scope) its fp64 weight arithmetic, not by HBM"},
        }
        if emit:
            print(json.dumps(out), flush=True)
    else:
        out = None
    h.close()
    return out


def cfg5_extra(dev) -> dict:
    """BASELINE configs[4] on ONE GPU, the largest single-GPU configuration (348 frames x 32 pairs at N = 65536): whole step and K_A alone,
    the same protocol as the contract line (spin-up, K_A as batches of launches between one HIP event pair on the launch stream).  The 64
    channels are the two channels of the cfg5 signal repeated (timing does not depend on the values; 1.5 GB of audio resident in HBM)."""
    import torch
    from signalizer_amd import api, config, sharding, synth
    cfg = config.cfg5()
    pairs, sr = cfg["num_pairs"], int(cfg["sample_rate"])
    S = int(60 * sr)
    two = torch.from_numpy(synth.gen(5, sr, S, 2)).to(dev)
    x = two.repeat(pairs, 1).contiguous()
    plan = api.Plan(cfg).upload()
    F = plan.num_frames(S)
    rgba = torch.empty((F, plan.P, 4), dtype=torch.uint8, device=dev)
    for _ in range(6):
        plan.render(x, rgba=rgba)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps = 10
    for _ in range(steps):
        plan.render(x, rgba=rgba)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    timer = sharding.TimeChunkRenderer(plan, x, rank=0, world=1)
    kern_ms = timer.time_stft_kernel(iters=6, spin_ms=30.0)
    bytes_per = 2 * cfg["window_size"] * 4 + 4 * plan.P
    achieved = F * pairs * bytes_per / (kern_ms * 1e-3) / 1e9
    return {"metric": "65536-pt stereo-pair STFT frames/sec, 32 pairs (75% overlap), one GPU", "value": F * pairs / dt, "unit": "frame-pairs/s",
            "ms_per_step": dt * 1e3, "frames": F, "pairs": pairs, "kernel": "stftRealKernel<5, true, 0>", "kernel_ms": kern_ms,
            "algorithmic_bytes_per_launch": F * pairs * bytes_per, "roofline_frac": achieved / HBM_PEAK_GBPS,
            "note": "BASELINE.json configs[4] as ONE 60 s job on one GPU (the sharded form is --workload cfg5 --gpus N); audio resident in HBM"}


def rsnt_extra(dev, x_host) -> dict:
    """the Spectrum view's other transform algorithm (RSNT, the resonator bank: resonator.hip) on the same 60 s buffer: one render =
    351 frames (one per hop), 2 signals x 3 vectors x 1024 resonators advanced by every sample.  `value`: the default form (block sums on
    the fp32 matrix cores); `bf16_form`: the opt-in three-part bf16 kernel (sgz.h SGZ_OPT_MATRIX_RESONATOR = 1: twice as fast, and on these
    boxes its instruction stream disturbs FFT kernels that run beside it -- NOTES.md round 6)"""
    import torch
    from signalizer_amd import api, config
    cfg = config.spectrum_config(algorithm=config.ALGO_RSNT)
    xs = torch.from_numpy(x_host[:2]).to(dev)

    def timed(form):
        plan = api.Plan(cfg)
        if form is not None:
            plan.set_option(api.OPT_MATRIX_RESONATOR, form)
        plan.upload()
        F = plan.num_frames(xs.shape[1])
        rgba = torch.empty((F, plan.P, 4), dtype=torch.uint8, device=dev)
        V = plan.resonator()[0].shape[0]
        plan.render(xs, rgba=rgba)
        torch.cuda.synchronize()
        ts = []
        for _ in range(10):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); plan.render(xs, rgba=rgba); b.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts)), F, V, plan.P
    ms, F, V, P = timed(None)
    ms_bf16 = timed(1)[0]
    flops = 8.0 * F * cfg["hop"] * 2 * V * P
    # what the matrix kernels EXECUTE: per frame (all from rest), (signal, vector, 32 resonators) wave and 1024-sample tile
    #   fp32 form: 32 v_mfma_f32_32x32x2_f32 (sixteen for the real, sixteen for the imaginary weights) of 32 * 32 * 2 multiply-adds
    #   bf16 form: 24 v_mfma_f32_32x32x16_bf16 (six bf16 x bf16 part products x two K halves, real and imaginary) of 32 * 32 * 16
    tiles = F * 2 * V * (P // 32) * (cfg["hop"] // 1024)
    f32_flops, bf16_flops = tiles * 32 * 32 * 32 * 2 * 2, tiles * 24 * 32 * 32 * 16 * 2
    F32_MFMA_PEAK, BF16_MFMA_PEAK = 157.3, 2500.0
    return {"metric": "RSNT (resonator bank) spectrogram frames/sec, stereo 48 kHz, 1024 axis points, Hann (3 vectors), one frame per 8192 samples",
            "value": F / ms * 1e3, "unit": "frames/s", "ms_per_step": ms, "frames": F, "realtime_factor": 60.0 / (ms * 1e-3),
            "kernel": "resonateMfmaKernel (block sums on the fp32 matrix cores: exact fp32 multiply-add chains) + "
                      "resonatorSegmentKernel / SegmentFoldKernel / ChainWindowKernel<3> + K_B",
            "mfma_instructions": tiles * 32, "mfma_tflops": f32_flops / (ms * 1e-3) / 1e12, "mfma_frac_of_peak": f32_flops / (ms * 1e-3) / 1e12 / F32_MFMA_PEAK,
            "recurrence_equivalent_tflops": flops / (ms * 1e-3) / 1e12,
            "bf16_form": {"ms_per_step": ms_bf16, "value": F / ms_bf16 * 1e3, "mfma_instructions": tiles * 24,
                          "mfma_tflops": bf16_flops / (ms_bf16 * 1e-3) / 1e12, "mfma_frac_of_peak": bf16_flops / (ms_bf16 * 1e-3) / 1e12 / BF16_MFMA_PEAK,
                          "note": "SGZ_OPT_MATRIX_RESONATOR = 1 (resonateMfmaBf16Kernel: every fp32 value as three exact bf16 parts, six part products); "
                                  "opt-in since round 6"},
            "note": "compute-bound.  mfma_tflops = multiply-adds the matrix kernel executes (x 2) over the WHOLE render's time (chain, window and K_B "
                    "kernels included) against the dense matrix peak of its type (fp32 157 TFLOP/s, bf16 2500 TFLOP/s; six bf16 products stand for one "
                    "fp32 product); profiles/r04a / r04c rsnt_* hold the kernels' own durations and the MFMA counters.  "
                    "recurrence_equivalent_tflops prices the sample-by-sample recurrence the reference runs (8 flops per sample, resonator, "
                    "vector and signal) at the same time: a statement about the algorithm, not about the pipe"}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--graph", action="store_true", help="single device: replay ONE hipGraph of the K timed steps instead of enqueuing them one by one "
                                                          "(immune to a descheduled host thread; ~0.7 us per step slower at K = 20, equal at K = 200)")
    ap.add_argument("--spinup-ms", type=float, default=150.0, help="untimed back-to-back steps before the warm-up steps, so that the device runs at "
                                                                   "its sustained clock when the timed region starts (0: none)")
    ap.add_argument("--rotate-mb", type=float, default=288.0, help="consecutive steps read distinct copies of the audio, this many MB of them in "
                    "total (default: past the 256 MB Infinity Cache, so that every step streams its input from HBM; 0: one buffer, "
                    "which stays cache-resident: K_A then measures 11-13 %% faster, profiles/r05a)")
    ap.add_argument("--no-extras", action="store_true", help="skip the measurements outside the contract line (tail-free launch, step with state "
                                                              "outputs): tools/profile.sh, so that the profiled dispatches are the workload's only")
    ap.add_argument("--workload", choices=("cfg2", "cfg5", "cfg3", "cfg4"), default="cfg2",
                    help="cfg2 (default): BASELINE.json's metric; with N GPUs every rank renders its own 60 s (weak scaling).  cfg5: the "
                         "64-channel 65536-pt job of BASELINE configs[4] -- ONE 60 s x 32-pair job split over the N ranks by time "
                         "chunk (strong scaling, 7.5 s per rank at N = 8): the curve SURVEY 8(e) asks for.  cfg3 / cfg4: the Oscilloscope / "
                         "Vectorscope real-time handles on BASELINE configs[2] / configs[3] (one step = one rendered frame at 60 Hz: the audio "
                         "callbacks of 1/60 s, then the render-thread calls); these paths do not shard: N ranks run N replicas")
    ap.add_argument("--shard-impl", choices=("c_abi", "torch"), default="c_abi",
                    help="N > 1: sgz_spectrogram_render_sharded on its own RCCL communicator (default), or signalizer_amd.sharding over "
                         "torch.distributed's nccl backend")
    ap.add_argument("--halo", choices=("p2p", "allgather"), default="p2p", help="torch implementation only: halo exchange form")
    ap.add_argument("--strict-shard-impl", action="store_true",
                    help="N > 1 with --shard-impl c_abi: exit non-zero if the library's own RCCL path fails on any rank.  By default such a run "
                         "times signalizer_amd.sharding instead (the same HIP kernels through the C ABI's stage calls, the collectives issued by "
                         "torch.distributed's RCCL backend) and SAYS SO: on stderr and in config.shard_impl of the line (with the error) -- a "
                         "scaling record with a disclosed fall-back instead of none")
    ap.add_argument("--allow-torch-fallback", action="store_true", help="(the default since round 5; kept for old command lines)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (the arrays its caller receives: the RGBA8 columns; "
                         "cfg3 / cfg4: the vertex and colour buffers) as DIR/<name>.npy in float32, at most 64 MB in all; the inputs are "
                         "seeded, so two builds run with the same arguments can be compared output for output.  N ranks: <name>_rank<r>")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    import torch
    from signalizer_amd import api, config, synth
    from signalizer_amd import sharding

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run for --gpus > 1")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)

    if args.workload in ("cfg3", "cfg4"):
        views_workload(args, rank, world, dev)
        if world > 1:
            dist.destroy_process_group()
        return
    strong = args.workload == "cfg5"
    if strong:
        cfg = config.cfg5()
        sr = 96000
        total = 60 * sr
        S = total // world                            # ONE 60 s job of 64 channels, cut into `world` time chunks
        assert S * world == total and S >= cfg["window_size"]
    else:
        cfg = config.cfg2()
        sr = 48000
        S = int(config.CFG2_SECONDS * sr)             # per-rank chunk: 2 880 000 samples (weak scaling: a world-times-longer stream)
    hop, W = cfg["hop"], cfg["window_size"]
    pairs = cfg["num_pairs"]
    bytes_per_frame = 2 * W * 4 + 4 * cfg["axis_points"]      # algorithmic bytes per stereo frame
    # rank r owns samples [r*S, (r+1)*S) of the stream
    x_host = synth.gen(config.CFG2_SEED + 100 * rank, sr, S, 2 * pairs)
    plan = api.Plan(cfg).upload()
    x_dev = torch.from_numpy(x_host).to(dev)
    rotate_bytes = int(args.rotate_mb * 1e6)
    timer = sharding.TimeChunkRenderer(plan, x_dev, rank=rank, world=world, halo=args.halo, rotate_bytes=rotate_bytes)   # kernel / collective probes (and the torch path)
    shard, shard_note = timer, ("single device" if world == 1 else "torch")
    if world > 1 and args.shard_impl == "c_abi":
        # every rank must take the same path: agree on whether the library's own RCCL communicator came up everywhere
        try:
            cand, err = CAbiShard(plan, x_dev, rank, world, dev, rotate_bytes), ""
        except Exception as e:                                     # noqa: BLE001 -- any failure here means "use the torch path"
            cand, err = None, f"{type(e).__name__}: {e}"
        ok = torch.tensor([1 if cand is not None else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 1:
            # ... and on whether one render goes through everywhere (a rank that fails aborts its communicator, so its peers fail
            # instead of waiting: sharded.hip)
            try:
                cand.render()
                torch.cuda.synchronize()
            except Exception as e:                                 # noqa: BLE001
                err = f"{type(e).__name__}: {e}"
                ok.zero_()
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 1:
            shard, shard_note = cand, "c_abi"
        elif not args.strict_shard_impl:
            shard_note = "torch (the library's own RCCL path failed on some rank" + (f": {err}" if err else "") + ")"
            sys.stderr.write(f"[bench rank {rank}] sgz_spectrogram_render_sharded / sgz_comm_create failed" + (f": {err}" if err else " on another rank")
                             + " -- timing the torch.distributed twin instead (config.shard_impl says so; --strict-shard-impl exits here)\n")
        else:
            # loud: sgz_spectrogram_render_sharded is what a scaling run is meant to measure
            sys.stderr.write(f"[bench rank {rank}] sgz_spectrogram_render_sharded / sgz_comm_create failed" + (f": {err}" if err else " on another rank")
                             + " (--strict-shard-impl: not falling back to the torch path)\n")
            dist.destroy_process_group()
            raise SystemExit(3)
    frames_per_rank = shard.local_frames
    stream = torch.cuda.current_stream().cuda_stream

    def step():
        shard.render()

    # The GPU reaches its sustained clock only under sustained load (tools/clock_ramp_probe.py: K_A back to back takes 35-38 us per
    # launch for the first ~4 ms from idle and settles at ~31 us after ~35 ms).  SURVEY.md 8(d)'s steady-state protocol repeats the job
    # back to back; a timed region of K = 20 steps is 0.8 ms.  So the device is spun up with the same steps first (untimed, not part
    # of the W warm-up steps), and the line says for how long.
    # (the number of steps is the same on every rank -- a step of a sharded render holds collectives: 32 steps are timed, the slowest
    # rank's time decides)
    # --graph: the K timed steps as ONE hipGraph launch (single device) -- the same launches in the same order on the same rotating inputs,
    # captured once from the library's own calls on the capturing stream and replayed: the timed region then holds one launch call and one
    # wait, so a host thread that is descheduled for a few milliseconds between two enqueues (seen once in this round's ~15 runs of the
    # default line: 74.8 us per step in the main region, 32-35 us in every other region of the same process) cannot sit inside it.
    # Measured (profiles/r06g): equal at K = 200 (31.8 | 31.6 us per step), 0.6-0.9 us per step slower at K = 20 (the graph's own launch),
    # which is why it is an option and not the default.  `ms_per_step_enqueued` is the one-by-one figure beside it.
    graph, graph_note = None, "steps enqueued one by one"
    if world == 1 and shard is timer and not strong and args.graph:
        try:
            warm = torch.cuda.Stream(device=dev)
            warm.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(warm):
                for _ in range(3):
                    step()
            torch.cuda.current_stream().wait_stream(warm)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(args.steps):
                    step()
            graph.replay()
            torch.cuda.synchronize()
            graph_note = f"one hipGraph of the {args.steps} steps (captured from the library's launches)"
        except Exception as e:                                       # noqa: BLE001 -- any failure: time the enqueue loop
            graph, graph_note = None, f"steps enqueued one by one (graph capture failed: {type(e).__name__})"
            torch.cuda.synchronize()
    spun = 0
    if args.spinup_ms > 0:
        torch.cuda.synchronize()
        spin_t0 = time.perf_counter()
        for _ in range(32):
            step()
        torch.cuda.synchronize()
        probe = torch.tensor([time.perf_counter() - spin_t0], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(probe, op=dist.ReduceOp.MAX)
        per_step_ms = max(float(probe.item()) * 1e3 / 32, 1e-3)          # (measured from idle with a wait at the end: an overestimate)
        spun = 32
        todo = min(int(args.spinup_ms / per_step_ms), 20000) // 32 * 32
        for i in range(todo):
            step()
            if i % 256 == 255:
                torch.cuda.synchronize()
        spun += todo
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    # the timed region holds the K steps and nothing else (until round 5 two HIP event records sat inside it for the gpu_ms diagnostic:
    # 0.3-0.6 us per step of a 20-step region, tools/steps20_probe.py -- that diagnostic is now taken from a second, untimed pass)
    t0 = time.perf_counter()
    if graph is not None:
        graph.replay()
    else:
        for _ in range(args.steps):
            step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.dump_outputs:                                           # (untimed; before the passes below overwrite the step's image)
        dump_outputs(args.dump_outputs, {"rgba" if world == 1 else f"rgba_rank{rank}": shard.rgba[:frames_per_rank].cpu().numpy()},
                     DUMP_LIMIT_BYTES // world)
    enq_ms = None
    if graph is not None:                                           # the same K steps enqueued one by one (diagnostic, untimed for `value`)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        enq_ms = (time.perf_counter() - t1) / args.steps * 1e3
    ev = HipEvents(2)
    ev.record(0, stream)
    for _ in range(args.steps):
        step()
    ev.record(1, stream)
    torch.cuda.synchronize()
    gpu_ms = ev.elapsed_ms(0, 1)

    # ---- outside the timed region ------------------------------------------------------------------------------------------------
    # dominant kernel (K_A): its own launches timed with HIP events on the launch stream
    kern_ms = timer.time_stft_kernel(iters=50)
    # latency of one render from an idle GPU, and the collectives on their own
    shots = []
    for _ in range(20):
        torch.cuda.synchronize()
        ts = time.perf_counter()
        step()
        torch.cuda.synchronize()
        shots.append((time.perf_counter() - ts) * 1e3)
    single_shot_ms = float(np.median(shots))
    coll_ms = timer.time_collectives(iters=20) if world > 1 else 0.0
    extra = {}
    if world == 1 and shard is timer and len(timer._bufs) > 1:
        # the same steps on ONE buffer (rounds 1-4 measured this): each XCD's slice of a 23 MB input then stays in its L2 from launch to launch
        kept = timer._bufs
        timer._bufs, timer._turn = kept[:1], 0
        timer.buf = kept[0]
        for _ in range(64):
            step()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        one = (time.perf_counter() - t1) / args.steps
        extra["one_buffer"] = {"ms_per_step": one * 1e3, "kernel_ms": timer.time_stft_kernel(iters=50)}
        timer._bufs = kept
    if world == 1 and not strong and not args.no_extras:
        # (i) the same kernel on a tail-free launch: 8 stereo pairs of the same buffer = 2784 workgroups on 256 CUs, so that the
        #     2-rounds-for-1.36-rounds-of-work tail of the 348-frame headline and the kernel's own efficiency can be told apart
        cfg8 = dict(cfg, num_pairs=8)
        plan8 = api.Plan(cfg8).upload()
        x8 = torch.from_numpy(synth.gen(config.CFG2_SEED, sr, S, 16)).to(dev)
        t8 = sharding.TimeChunkRenderer(plan8, x8, rank=0, world=1)
        k8 = t8.time_stft_kernel(iters=20)
        extra["no_tail"] = {"tasks": t8.local_frames * 8, "kernel_ms": k8,
                            "achieved": t8.local_frames * 8 * bytes_per_frame / (k8 * 1e-3) / 1e9}
        del t8, x8, plan8
        # (ii) the step that also produces what the reference updates on every frame -- lineGraphs[k].states and .results
        #      (TransformDSP.inl:1299-1435): line results of both graphs for every frame + the decay state after the last one
        F = frames_per_rank
        lines = torch.empty((F, pairs, 2, plan.P, 2), dtype=torch.float32, device=dev)
        state = torch.zeros((pairs, 2, plan.P, 2), dtype=torch.float32, device=dev)
        rgba = torch.empty((F, plan.P, 4), dtype=torch.uint8, device=dev)
        view = timer._view()
        state.zero_()
        for _ in range(5):
            plan.render(view, rgba=rgba, lines=lines, state=state)
        torch.cuda.synchronize()
        ts = time.perf_counter()
        for _ in range(50):                                                   # (the state carries over from buffer to buffer, as in a long job)
            plan.render(view, rgba=rgba, lines=lines, state=state)
        torch.cuda.synchronize()
        extra["ms_per_step_with_state"] = (time.perf_counter() - ts) / 50 * 1e3
        # (ii-b) ... and the step that leaves what the reference HOLDS once the buffer has gone through: the image and the decay state after
        #        the last frame (lineGraphs[k].results is one buffer, overwritten by every frame: only the last frame's survives)
        state.zero_()
        for _ in range(5):
            plan.render(view, rgba=rgba, state=state)
        torch.cuda.synchronize()
        ts = time.perf_counter()
        for _ in range(50):
            plan.render(view, rgba=rgba, state=state)
        torch.cuda.synchronize()
        extra["ms_per_step_with_end_state"] = (time.perf_counter() - ts) / 50 * 1e3
        # (iii) two buffers in flight: independent renders (two plans -- a plan owns its scratch --, two streams) alternate, so that one
        #       buffer's K_B and the partly filled last round of its K_A overlap the other buffer's K_A.  What a job of many buffers gets;
        #       NOT the contract line's value (steps there run one after the other on one stream), and a kernel's own duration grows under it.
        plan_b = api.Plan(cfg).upload()
        x_b = torch.from_numpy(synth.gen(config.CFG2_SEED + 7, sr, S, 2 * pairs)).to(dev)
        rg = [torch.empty((F, plan.P, 4), dtype=torch.uint8, device=dev) for _ in range(2)]
        st = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
        job = [(plan, view, rg[0], st[0].cuda_stream), (plan_b, x_b, rg[1], st[1].cuda_stream)]
        for i in range(10):
            pl, xx, out_, s_ = job[i & 1]
            pl.render(xx, rgba=out_, stream=s_)
        torch.cuda.synchronize()
        ts = time.perf_counter()
        n2 = 2 * max(50, args.steps // 2)
        for i in range(n2):
            pl, xx, out_, s_ = job[i & 1]
            pl.render(xx, rgba=out_, stream=s_)
        torch.cuda.synchronize()
        two = (time.perf_counter() - ts) / n2
        extra["two_in_flight"] = {"ms_per_step": two * 1e3, "value": F * pairs / two,
                                  "note": "two independent buffers alternate on two streams (two plans); steps of the contract line do not overlap"}
        del plan_b, x_b
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        fr = torch.tensor([frames_per_rank], dtype=torch.float64, device=dev)
        dist.all_reduce(fr, op=dist.ReduceOp.SUM)
        total_frames = int(fr.item())
    else:
        total_frames = frames_per_rank

    if rank == 0:
        value = total_frames * pairs * args.steps / dt
        achieved = frames_per_rank * pairs * bytes_per_frame / (kern_ms * 1e-3) / 1e9
        traffic = measured_traffic() if not strong else None
        out = {
            "metric": "32768-pt stereo STFT frames/sec (75% overlap); achieved HBM GB/s vs peak" if not strong else
                      "65536-pt stereo-pair STFT frames/sec, 32 pairs (75% overlap), time-chunk sharded; achieved HBM GB/s vs peak",
            "value": value, "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong" if strong else "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            # top level, so that no consumer of `value` can miss it: True = the library's own RCCL path (sgz_spectrogram_render_sharded)
            # failed on some rank and the line times the torch.distributed twin of it (same kernels through the stage calls)
            "fallback": world > 1 and args.shard_impl == "c_abi" and shard_note != "c_abi",
            "config": {"workload": ("BASELINE.json configs[1]: stereo 48 kHz spectrogram, 32768-pt FFT, 75% overlap "
                                    "(hop 8192), 60 s buffer => 348 frames/GPU, P=1024, Hann, Separate, Lanczos, log view")
                       if not strong else
                       ("BASELINE.json configs[4]: 64-channel 96 kHz spectrogram, 65536-pt FFT, 75% overlap (hop 16384), ONE 60 s job "
                        f"(348 frames x 32 pairs) split into {world} time chunks, P=1024, Hann, Separate, Lanczos, log view"),
                       "frames_per_gpu": frames_per_rank, "parallelism": f"time-chunk x{world}",
                       "step": "K_A + K_B -> RGBA8 columns; line results and the decay end state are not requested in the timed step "
                               "(the image does not depend on them; ms_per_step_with_state times the step that writes them)",
                       "shard_impl": shard_note, "timed_region": graph_note,
                       "gpu_ms_per_step_rank0": gpu_ms / args.steps, "single_shot_ms": single_shot_ms,
                       "collectives_ms_per_step": coll_ms,
                       "input_rotation": {"buffers": len(timer._bufs), "mb": args.rotate_mb,
                                          "note": "consecutive steps (and the K_A launches of roofline.kernel_ms) read distinct copies of the audio, "
                                                  "more of them than the 256 MB Infinity Cache holds: every step streams its input from HBM "
                                                  "(--rotate-mb 0: one cache-resident buffer, K_A 11-13 % faster: profiles/r05a/one_buffer.txt)"},
                       "spin_up": {"ms": args.spinup_ms, "steps": spun,
                                   "note": "untimed back-to-back steps before the W warm-up steps: the device's clock needs ~35 ms of sustained "
                                           "load to settle (tools/clock_ramp_probe.py); single_shot_ms is a render from an idle device"}},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBPS, "traffic": traffic,
                         "traffic_source": None if traffic is None else "profiles/traffic_latest.json (committed rocprofv3 --pmc pass of this "
                                                                        "workload, gfx950 correction applied; not collected in this run)",
                         "kernel": ("stftRealKernel<4, true, 0>" if plan.path & 8 else "stftMapKernel<5, 0, true, true>") if not strong else
                                   ("stftRealKernel<5, true, 0> (one K_A pass)" if plan.path & 8 else "stftHalfKernel + mapSideKernel (one K_A pass)"),
                         "kernel_ms": kern_ms, "algorithmic_bytes_per_launch": frames_per_rank * pairs * bytes_per_frame},
        }
        if world == 1 and not strong and not args.no_extras:
            # (iv) the library's own form of that: sgz_render_queue (include/sgz.h) -- a job of many independent buffers submitted round-robin over
            #      `depth` lanes (a plan + a stream each), nothing waited for between submissions; the inputs rotate over the same distinct
            #      copies as the contract line's (past the Infinity Cache).  What a batch job gets per buffer; NOT the contract line's value.
            try:
                bufs = [b[:, timer.sp.local_offset:timer.sp.local_offset + timer.sp.local_samples] for b in timer._bufs]
                piped, lanes = {}, {}
                for depth in (2, 3, 4, 6):
                    q = api.RenderQueue(cfg, depth)
                    lanes[depth] = q.distinct_lanes
                    qo = [torch.empty((F, plan.P, 4), dtype=torch.uint8, device=dev) for _ in range(depth)]
                    for i in range(2400):                          # (~60 ms of work: the queue was just built on an idle device, whose clock has dropped -- config.spin_up)
                        q.submit(bufs[i % len(bufs)], qo[i % depth])
                    q.wait()
                    nq = 600
                    ts = time.perf_counter()
                    for i in range(nq):
                        q.submit(bufs[i % len(bufs)], qo[i % depth])
                    q.wait()
                    piped[depth] = (time.perf_counter() - ts) / nq
                    q.close()
                best = min(piped, key=piped.get)
                extra["pipelined"] = {"ms_per_step": piped[best] * 1e3, "value": F * pairs / piped[best], "depth": best,
                                      "ms_per_step_by_depth": {str(d): v * 1e3 for d, v in piped.items()},
                                      "lanes_on_own_hardware_queue_by_depth": {str(d): v for d, v in lanes.items()},
                                      "note": "sgz_render_queue: independent 60 s buffers submitted round-robin over `depth` lanes (plan + stream each; "
                                              "K_B as 16-pixel workgroups), no host wait between submissions, input rotated as for the contract line: one "
                                              "buffer's K_B and half-empty last K_A generation run beside the next buffers' K_A.  A render's kernels take "
                                              "LONGER than ms_per_step here (they overlap); the contract line's steps do not overlap"}
            except Exception as e:                                     # noqa: BLE001 -- an extra: must not cost the line
                extra["pipelined"] = {"error": f"{type(e).__name__}: {e}"}
        if "no_tail" in extra:
            nt = extra["no_tail"]
            out["roofline"]["frac_no_tail"] = nt["achieved"] / HBM_PEAK_GBPS
            out["roofline"]["no_tail"] = {"tasks": nt["tasks"], "kernel_ms": nt["kernel_ms"], "achieved": nt["achieved"],
                                          "note": "8 stereo pairs of the cfg2 buffer: many rounds of workgroups, so the partial last round does not count (the same channel-split kernel as the headline launch)"}
        # the like-for-like step (the reference updates lineGraphs[k].states / .results on every frame, TransformDSP.inl:1336-1349) and the
        # cold number, beside `value` at top level
        out["single_shot"] = {"ms": single_shot_ms, "value": total_frames * pairs / (single_shot_ms * 1e-3), "unit": "frames/s",
                              "note": "one render from an idle device (host clock around enqueue + wait; the device is at its idle clock)"}
        if "ms_per_step_with_state" in extra:
            out["config"]["ms_per_step_with_state"] = extra["ms_per_step_with_state"]
            out["ms_per_step_with_state"] = extra["ms_per_step_with_state"]
            out["value_with_state"] = total_frames * pairs / (extra["ms_per_step_with_state"] * 1e-3)
        if "ms_per_step_with_end_state" in extra:
            out["ms_per_step_with_end_state"] = extra["ms_per_step_with_end_state"]
            out["value_with_end_state"] = total_frames * pairs / (extra["ms_per_step_with_end_state"] * 1e-3)
            out["config"]["with_state_note"] = ("value_with_state: line results of both graphs for EVERY frame + the decay state after the last one; "
                                                "value_with_end_state: the image + the decay state after the last frame (what the reference holds "
                                                "after the same audio: its line results are one buffer that every frame overwrites)")
        if "two_in_flight" in extra:
            out["config"]["two_in_flight"] = extra["two_in_flight"]
        if "pipelined" in extra:
            out["pipelined"] = extra["pipelined"]
            if "value" in extra["pipelined"]:
                out["value_pipelined"] = extra["pipelined"]["value"]
        if enq_ms is not None:
            out["ms_per_step_enqueued"] = enq_ms
            out["value_enqueued"] = total_frames * pairs / (enq_ms * 1e-3)
        if "one_buffer" in extra:
            ob = extra["one_buffer"]
            out["value_one_buffer"] = total_frames * pairs / (ob["ms_per_step"] * 1e-3)
            out["ms_per_step_one_buffer"] = ob["ms_per_step"]
            out["roofline"]["kernel_ms_one_buffer"] = ob["kernel_ms"]
            out["roofline"]["frac_one_buffer"] = frames_per_rank * pairs * bytes_per_frame / (ob["kernel_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBPS
            out["config"]["one_buffer_note"] = ("value_one_buffer / roofline.*_one_buffer: the protocol of rounds 1-4 -- every step re-renders the SAME 23 MB "
                                                "buffer, whose per-XCD slices stay L2-resident from launch to launch; the contract line above streams "
                                                "its input from HBM (config.input_rotation)")
        if world == 1 and not strong and not args.no_extras:
            # BASELINE configs[2] / configs[3] on the same box, so that the driver's record of this run holds them too (their own lines:
            # --workload cfg3 / cfg4)
            out["extras"] = {}
            for w in ("cfg3", "cfg4"):
                v = views_workload(args, 0, 1, dev, workload=w, steps=120, emit=False)
                out["extras"][w] = {"metric": v["metric"], "value": v["value"], "unit": v["unit"], "ms_per_step": v["ms_per_step"],
                                    "vertices_per_step": v["config"]["vertices_per_step"], "realtime_factor": v["config"]["realtime_factor"],
                                    "pushes_refused_busy": v["config"]["pushes_refused_busy"], "kernel": v["roofline"]["kernel"],
                                    "kernel_ms": v["roofline"]["kernel_ms"], "roofline_frac": v["roofline"]["frac"],
                                    "ms_per_step_device_resident": v["config"]["ms_per_step_device_resident"],
                                    "kernel_ms_pinned_destination": v["roofline"].get("kernel_ms_pinned_destination")}
            out["extras"]["rsnt"] = rsnt_extra(dev, x_host)
            out["extras"]["cfg5"] = cfg5_extra(dev)
        if not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline_pairs(cfg, x_host) if strong else cpu_baseline(cfg, x_host)
        if out["fallback"]:
            out["metric"] += " [FALLBACK: torch.distributed twin timed, not the C-ABI sharded path]"
        print(json.dumps(out), flush=True)
    if world > 1:
        if shard is not timer:
            shard.close()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
