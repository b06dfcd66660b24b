"""The image-only launch of cfg2 (348 frames: 348 channel workgroups of side 0 and the Nyquist workgroups, spectrum_real.hip) and the
whole step, in both input protocols: rotated over 13 copies of the audio (288 MB, past the Infinity Cache: bench.py's default) and one
buffer (bench.py --rotate-mb 0).  Same timing loop as tools/ka_time.py (sustained clock, batches between one event pair).
K_A here is sgz_stage_nyquist(image_only = 1): the launch itself and the 2.8 KB copy of the Nyquist words behind it, the same for
every build; the launch alone is in a rocprofv3 pass (tools/profile.sh).
usage: [SGZ_LIB=...] ka_image_time.py [iters] [frames]      prints one dict"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from signalizer_amd import api, config, synth
from ka_time import timeit

ROTATE_BYTES = 288e6


def protocols(plan, x, S, iters):
    """{protocol: (K_A median, K_A min, step median, step min)} in us"""
    L = api.lib()
    stream = torch.cuda.current_stream().cuda_stream
    F = plan.num_frames(S)
    ny = torch.empty((F, plan.C, 2), dtype=torch.float32, device="cuda")
    rgba = torch.empty((F, plan.P, 4), dtype=torch.uint8, device="cuda")
    nyf, low = C.c_uint32(0), C.c_uint32(0)
    out = {}
    for name, nbuf in (("rotated", max(1, -int(-ROTATE_BYTES // (x.numel() * 4)))), ("one_buffer", 1)):
        xs = [x] + [x.clone() for _ in range(nbuf - 1)]
        turn = [0]

        def nextx():
            turn[0] = (turn[0] + 1) % nbuf
            return xs[turn[0]]

        def ka():
            b = nextx()
            api.check(L.sgz_stage_nyquist(plan.h, b.data_ptr(), b.stride(0), S, 1, ny.data_ptr(), C.byref(nyf), C.byref(low), stream))

        def step():
            plan.render(nextx(), rgba=rgba)

        ka()
        assert nyf.value >= 1, "not an image-only launch"
        m, mn = timeit(ka, iters)
        sm, smn = timeit(step, iters)
        out[name] = (round(m, 2), round(mn, 2), round(sm, 2), round(smn, 2))
        del xs
    return out


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    cfg = config.cfg2()
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 348
    S = cfg["window_size"] + cfg["hop"] * (frames - 1)
    x = torch.from_numpy(synth.gen(config.CFG2_SEED, 48000, S, 2)).cuda()
    plan = api.Plan(cfg).upload()
    print({k: dict(ka_us=v[0], ka_min_us=v[1], step_us=v[2], step_min_us=v[3]) for k, v in protocols(plan, x, S, iters).items()})


if __name__ == "__main__":
    main()
