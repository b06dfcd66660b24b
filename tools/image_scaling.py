"""tools/real_scaling.py for the IMAGE-ONLY launch form: K_A (and the step) against the number of frames at cfg2's settings, rotated
input and one buffer (tools/ka_image_time.py): what a CU costs with one channel workgroup, with a Nyquist workgroup beside it, with two.
usage: [SGZ_LIB=...] [SGZ_IMAGE_SPLIT=n] image_scaling.py [frames ...]
       (SGZ_IMAGE_SPLIT: SGZ_OPT_IMAGE_ONLY_SPLIT of the plan -- n >= 2 forces n frames per Nyquist workgroup; default 1, the automatic size)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from signalizer_amd import api, config, synth
from ka_image_time import protocols

cfg = config.cfg2()
frames = [int(a) for a in sys.argv[1:]] or [128, 256, 300, 348, 400, 512]
plan = api.Plan(cfg)
plan.set_option(api.OPT_IMAGE_ONLY_SPLIT, int(os.environ.get("SGZ_IMAGE_SPLIT", "1")))
plan.upload()
xall = torch.from_numpy(synth.gen(config.CFG2_SEED, 48000, cfg["window_size"] + cfg["hop"] * (max(frames) - 1), 2)).cuda()
print("frames  Nyquist wgs  | rotated: K_A+copy  step | one buffer: K_A+copy  step   (us, median of 5 batches of 40)")
for F in frames:
    S = cfg["window_size"] + cfg["hop"] * (F - 1)
    x = xall[:, :S].contiguous()
    r = protocols(plan, x, S, 40)
    _, nyf, _ = plan.stage_nyquist(x, True)
    print(f"{F:6d}  {-(-F // nyf):11d}  | {r['rotated'][0]:8.2f} {r['rotated'][2]:8.2f} | {r['one_buffer'][0]:8.2f} {r['one_buffer'][2]:8.2f}", flush=True)
