"""Times HIComProjector.forward_ragged on mixed batches (single images next to clips of several lengths) against the two ways a user
has without it, on the same inputs: (b) a loop of forward() per item, (c) bucketing the items by shape, one forward_batch per bucket
and the torch.stack copies that needs.  One process, HIP events, after warm-up; inputs rotate through three sets.  Writes
profiles/ragged_step.json, or with --recipe adaptkv (the k / v adaptor recipe, timed the same three ways) profiles/ragged_step_adaptkv.json.

    python tools/ragged_bench.py [--recipe plain|adaptkv] [--iters 30] [--warmup 5] [--out profiles/ragged_step.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from batch_bench import timed, recipe_projector, default_out, RECIPES, D, GRID, SETS           # noqa: E402

# name -> [(modal, T)] in batch order (images and clips interleaved as a data loader would deliver them)
MIXES = {
    "12 images + 4 clips of 8": [("image", 1)] * 12 + [("video", 8)] * 4,
    "8 images + 2 clips each of 4, 8, 16, 32": [("image", 1)] * 8 + [("video", t) for t in (4, 8, 16, 32) for _ in range(2)],
    "16 equal images (control)": [("image", 1)] * 16,
}


def interleave(items):
    """Clips spread between the images (stable for a given mix)."""
    img = [x for x in items if x[0] == "image"]
    vid = [x for x in items if x[0] == "video"]
    if not vid:
        return img
    out, per = [], max(1, len(img) // len(vid))
    while img or vid:
        out += img[:per]
        img = img[per:]
        if vid:
            out.append(vid.pop(0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--recipe", choices=sorted(RECIPES), default="plain")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or default_out("ragged_step", args.recipe)
    dev = torch.device("cuda")
    m = recipe_projector(args.recipe, args.hidden, 32, dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    rows = []
    with torch.no_grad():
        for name, items in MIXES.items():
            items = interleave(items)
            modals, splits = [x[0] for x in items], [x[1] for x in items]
            B, frames = len(items), sum(splits)
            t0 = [sum(splits[:i]) for i in range(B)]
            buckets = {}
            for i, key in enumerate(items):
                buckets.setdefault(key, []).append(i)
            sets = [tuple(torch.randn(s, device=dev, generator=gen).bfloat16()
                          for s in ((frames, GRID, GRID, D), (frames, GRID, GRID, D), (B, D))) for _ in range(SETS)]

            def rag(s):
                return m.forward_ragged(s[0], s[1], s[2], splits, modals)

            def loop(s):
                return [m(s[0][t0[i]:t0[i] + splits[i]], s[1][t0[i]:t0[i] + splits[i]], s[2][i], modals[i]) for i in range(B)]

            def bucketed(s):
                out = [None] * B
                for (modal, T), idx in buckets.items():
                    ff = torch.stack([s[0][t0[i]:t0[i] + T] for i in idx])
                    fe = torch.stack([s[1][t0[i]:t0[i] + T] for i in idx])
                    res = m.forward_batch(ff, fe, s[2][idx], modal)
                    for k, i in enumerate(idx):
                        out[i] = res[k]
                return out

            want = loop(sets[0])
            dev_abs = max(float((a.float() - b.float()).abs().max()) for a, b in zip(rag(sets[0]), want))
            dev_abs_c = max(float((a.float() - b.float()).abs().max()) for a, b in zip(bucketed(sets[0]), want))
            t_a, t_b, t_c = (timed(f, sets, args.iters, args.warmup) for f in (rag, loop, bucketed))
            row = dict(recipe=args.recipe, mix=name, B=B, frames=frames, buckets=len(buckets), grid=GRID, hidden=args.hidden, ragged_us=round(t_a, 1),
                       loop_us=round(t_b, 1), bucketed_us=round(t_c, 1), loop_over_ragged=round(t_b / t_a, 2),
                       bucketed_over_ragged=round(t_c / t_a, 2), max_abs_vs_loop=dev_abs, bucketed_max_abs_vs_loop=dev_abs_c)
            if len(buckets) == 1:                       # the control: forward_batch on the 5-D view of the same tensor, no copy
                (modal, T), _ = next(iter(buckets.items()))
                view = lambda s: m.forward_batch(s[0].view(B, T, GRID, GRID, D), s[1].view(B, T, GRID, GRID, D), s[2], modal)
                row["batch_view_us"] = round(timed(view, sets, args.iters, args.warmup), 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del sets
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/ragged_bench.py", recipe=args.recipe, device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       timing="median of HIP-event intervals around one forward_ragged call (ragged), the per-item forward() loop (loop) or "
                              "one forward_batch per shape bucket with its torch.stack copies (bucketed); inputs rotate through 3 sets",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
