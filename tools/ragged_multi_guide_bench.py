"""Times HIComProjector.forward_ragged_multi_guide (B items of unequal length, item i with its own Q_i instructions, one call) against the
three ways a caller had before it, on the same inputs: the loop of forward_multi_guide per item, forward_ragged on tokens replicated per
guide (the replication copy counted), and the loop of sum Q_i forward() calls.  One process, HIP events, after warm-up; inputs rotate
through three sets.  Writes profiles/ragged_multi_guide_step.json.

    python tools/ragged_multi_guide_bench.py [--shapes clips8x3_T8 ...] [--iters 30] [--warmup 5] [--out profiles/ragged_multi_guide_step.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench                                           # noqa: E402  (release_config / make_projector: the benchmark's module)
from batch_bench import D, GRID, SETS, timed            # noqa: E402

# name -> (frames per item, guides per item)
SHAPES = {
    "clips8x3_T8": ([8] * 8, [3] * 8),
    "clips8x3_T64": ([64] * 8, [3] * 8),
    "images16x4": ([1] * 16, [4] * 16),
    "mixed": ([1, 4, 1, 8, 16, 1, 8, 4, 16, 1], [1, 2, 3, 4, 5, 6, 3, 2, 1, 4]),
    "one_clip_T8_Q3": ([8], [3]),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_multi_guide_step.json"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(7)
    m = bench.make_projector(bench.release_config(args.hidden, 64), dev)
    rows = []
    with torch.no_grad():
        for name in args.shapes:
            splits, counts = SHAPES[name]
            modals = ["image" if t == 1 else "video" for t in splits]
            sets = [(torch.randn((sum(splits), GRID, GRID, D), device=dev, generator=gen).bfloat16(),
                     torch.randn((sum(splits), GRID, GRID, D), device=dev, generator=gen).bfloat16(),
                     torch.randn((sum(counts), D), device=dev, generator=gen).bfloat16()) for _ in range(SETS)]
            pairs = [(i, q) for i, n in enumerate(counts) for q in range(n)]
            rep_splits, rep_modals = [splits[i] for i, _ in pairs], [modals[i] for i, _ in pairs]

            def items(s):
                return list(zip(s[0].split(splits), s[1].split(splits), s[2].split(counts)))

            new = lambda s: m.forward_ragged_multi_guide(s[0], s[1], s[2], splits, counts, modals)
            mg_loop = lambda s: [m.forward_multi_guide(ff, fe, g, modal) for (ff, fe, g), modal in zip(items(s), modals)]

            def ragged_replicated(s):                   # every item's tokens written Q_i times, then read by forward_ragged
                parts = items(s)
                ff = torch.cat([parts[i][0] for i, _ in pairs])
                fe = torch.cat([parts[i][1] for i, _ in pairs])
                return m.forward_ragged(ff, fe, s[2], rep_splits, rep_modals)

            fwd_loop = lambda s: [m(ff, fe, g[q], modal) for (ff, fe, g), modal in zip(items(s), modals) for q in range(g.shape[0])]
            want = fwd_loop(sets[0])
            got = new(sets[0])
            dev_abs = max(float((got[i][q].float() - want[k].float()).abs().max()) for k, (i, q) in enumerate(pairs))
            t_new, t_mg, t_rag, t_fwd = (timed(fn, sets, args.iters, args.warmup) for fn in (new, mg_loop, ragged_replicated, fwd_loop))
            rows.append(dict(shape=name, frames=splits, guides=counts, pairs=len(pairs), grid=GRID, hidden=args.hidden,
                             ragged_multi_guide_us=round(t_new, 1), multi_guide_loop_us=round(t_mg, 1), ragged_replicated_us=round(t_rag, 1),
                             forward_loop_us=round(t_fwd, 1), multi_guide_loop_over_new=round(t_mg / t_new, 2),
                             ragged_replicated_over_new=round(t_rag / t_new, 2), forward_loop_over_new=round(t_fwd / t_new, 2),
                             max_abs_vs_forward_loop=dev_abs))
            print(json.dumps(rows[-1]), flush=True)
            del sets, want, got
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/ragged_multi_guide_bench.py", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       timing="median of HIP-event intervals around one forward_ragged_multi_guide call, the per-item forward_multi_guide loop, "
                              "forward_ragged on the per-guide replicated tokens (its torch.cat copies included), or the sum Q_i forward() loop; "
                              "inputs rotate through 3 sets",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
