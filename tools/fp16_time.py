"""Dev: the fp16 release step against the bf16 one at C2 (64 frames of 27 x 27, hidden 896), in ONE process, arms alternated.
usage: fp16_time.py [rounds=7] [steps=20]

  bf16   a bf16 projector on bf16 inputs (bench.py's module and call, without hipGraph replay)
  fp16   the same weights as an fp16 projector on fp16 inputs: the fused step on the fp16 tokens (HIComProjector._forward_half)
  cast   the cost the fp16 width had before: cast16(frames_feature) + cast16(frames_embed) + the bf16 forward

Inputs rotate through 3 distinct sets per arm as in bench.py (HBM-resident, not cache-resident).  Each round times `steps` calls of every
arm back to back (order rotated per round); the line per arm gives the median over the rounds and the spread (min .. max) in us per step."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from hicom_amd import native as nv

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev = torch.device("cuda", 0)
cfg = bench.release_config(896, 64)
m16 = bench.make_projector(cfg, dev)
m16.graph_replay = False
mh = bench.make_projector(cfg, dev).half()
mh.graph_replay = False
m16.return_fp32 = mh.return_fp32 = False
gen = torch.Generator(device=dev).manual_seed(1234)
sets_bf, sets_h = [], []
for i in range(bench.N_INPUT_SETS):
    ff = torch.randn(64, 27, 27, 1152, device=dev, generator=gen)
    fe = torch.randn(64, 27, 27, 1152, device=dev, generator=gen)
    g = torch.randn(1152, device=dev, generator=gen)
    sets_bf.append((ff.bfloat16(), fe.bfloat16(), g.bfloat16()))
    sets_h.append((ff.half(), fe.half(), g.half()))
    del ff, fe, g
ctr = {"bf16": 0, "fp16": 0, "cast": 0}


def run(arm):
    i = ctr[arm] % len(sets_bf)
    ctr[arm] += 1
    if arm == "bf16":
        a, b, g = sets_bf[i]
        return m16(a, b, g, "video", None)
    if arm == "fp16":
        a, b, g = sets_h[i]
        return mh(a, b, g, "video", None)
    a, b, g = sets_h[i]
    return m16(nv.cast16(a, torch.bfloat16), nv.cast16(b, torch.bfloat16), nv.cast16(g, torch.bfloat16), "video", None)


arms = ["bf16", "fp16", "cast"]
times = {k: [] for k in arms}
with torch.no_grad():
    for k in arms:
        for _ in range(10):
            run(k)
    plan = mh.__dict__["_bf16_twin"][0].__dict__.get("_last_plan")
    print(f"fp16 arm on the fused fp16 step: {bool(plan is not None and plan.args.tok_dt == nv.DT_F16 and plan.fused)}")
    for r in range(rounds):
        for k in arms[r % 3:] + arms[:r % 3]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                run(k)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / steps * 1e6)
for k in arms:
    v = times[k]
    print(f"{k}: median {statistics.median(v):.1f} us/step  (min {min(v):.1f}, max {max(v):.1f}; {rounds} rounds x {steps} steps)")
print(f"fp16 / bf16: {statistics.median(times['fp16']) / statistics.median(times['bf16']):.4f}   "
      f"cast / bf16: {statistics.median(times['cast']) / statistics.median(times['bf16']):.4f}")
