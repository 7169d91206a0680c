"""Times HIComProjector.forward_batch against a loop of B forward() calls on the same inputs (the per-item path), one process, HIP
events, after warm-up; inputs rotate through three sets.  Writes profiles/batch_step.json, or with --recipe adaptkv (the k / v adaptor
recipe local43_adaptkv_global32, timed the same way) profiles/batch_step_adaptkv.json.

    python tools/batch_bench.py [--recipe plain|adaptkv] [--iters 30] [--warmup 5] [--out profiles/batch_step.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                           # noqa: E402  (release_config / make_projector: the benchmark's module)

D, GRID, SETS = 1152, 27, 3
SHAPES = [("image", 1, b) for b in (1, 4, 16, 64)] + [("video", 8, b) for b in (4, 16)]
RECIPES = {"plain": "local43_global32_coarse", "adaptkv": "local43_adaptkv_global32"}


def recipe_projector(recipe, hidden, frames, dev):
    """The benchmark's module for a recipe of the batched / ragged step (alphas = 0.5 by bench.make_projector: live adaptor branches)."""
    cfg = bench.release_config(hidden, frames)
    cfg.mm_projector_type = RECIPES[recipe]
    return bench.make_projector(cfg, dev)


def default_out(stem, recipe):
    return os.path.join(ROOT, "profiles", stem + ("" if recipe == "plain" else "_" + recipe) + ".json")


def timed(fn, sets, iters, warmup):
    for i in range(warmup):
        fn(sets[i % SETS])
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for i, (a, b) in enumerate(evs):
        a.record()
        fn(sets[i % SETS])
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in evs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--recipe", choices=sorted(RECIPES), default="plain")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or default_out("batch_step", args.recipe)
    dev = torch.device("cuda")
    m = recipe_projector(args.recipe, args.hidden, 8, dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    rows = []
    with torch.no_grad():
        for modal, T, B in SHAPES:
            sets = [tuple(torch.randn(s, device=dev, generator=gen).bfloat16()
                          for s in ((B, T, GRID, GRID, D), (B, T, GRID, GRID, D), (B, D))) for _ in range(SETS)]
            batched = lambda s: m.forward_batch(s[0], s[1], s[2], modal)
            loop = lambda s: [m(s[0][b], s[1][b], s[2][b], modal) for b in range(B)]
            want = torch.stack(loop(sets[0])).float()
            dev_abs = float((batched(sets[0]).float() - want).abs().max())
            t_b, t_l = timed(batched, sets, args.iters, args.warmup), timed(loop, sets, args.iters, args.warmup)
            rows.append(dict(recipe=args.recipe, modal=modal, T=T, B=B, grid=GRID, hidden=args.hidden, batch_us=round(t_b, 1), loop_us=round(t_l, 1),
                             loop_over_batch=round(t_l / t_b, 2), max_abs_vs_loop=dev_abs))
            print(json.dumps(rows[-1]), flush=True)
            del sets
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/batch_bench.py", recipe=args.recipe, device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       timing="median of HIP-event intervals around one call (batched) or the B-call loop, inputs rotate through 3 sets",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
