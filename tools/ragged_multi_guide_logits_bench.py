"""Times the ragged multi-guide step WITHOUT frames_embed against the pipeline it replaces, on the same box and the same
inputs:

    new      siglip_head_scores_ragged(x, head, guides, splits, counts)  ->  forward_ragged_multi_guide(x, None, guides, ..., local_logits=L)
    parent   siglip_head_embed(x, head)                                  ->  forward_ragged_multi_guide(x, fe, guides, ...)
    loop     per clip: siglip_head_scores_multi + forward_multi_guide(local_logits=)          (`--loop-shapes`, default the 64-frame point)

(the tower's hidden states double as frames_feature; the head has the so400m widths 1152 -> 4304 -> 1152; the shapes are those of
tools/ragged_multi_guide_bench.py).  The head step and the compressor step of the new and the parent pipeline are timed on their own as
well.  The method is tools/multi_guide_logits_bench.py's: one process, HIP events around one whole pipeline (or step), after warm-up;
inputs rotate through three sets; every figure is the median of `iters` intervals, measured `repeats` times: the median of those medians
is reported, and their range (max - min) as the run-to-run spread.  `new_wins` says whether the new pipeline is faster than the parent by
more than the two spreads together.  Writes profiles/ragged_multi_guide_logits_step.json.

    python tools/ragged_multi_guide_logits_bench.py [--shapes clips8x3_T64 clips8x3_T8 images16x4] [--iters 20] [--warmup 5] [--repeats 3]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench                                           # noqa: E402  (release_config / make_projector: the benchmark's module)
from batch_bench import D, GRID, SETS                   # noqa: E402
from hicom_amd import siglip_head_embed, siglip_head_scores_multi, siglip_head_scores_ragged           # noqa: E402
from multi_guide_logits_bench import make_head, repeated                    # noqa: E402
from ragged_multi_guide_bench import SHAPES             # noqa: E402

POINTS = ["clips8x3_T64", "clips8x3_T8", "images16x4"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--shapes", nargs="+", default=POINTS, choices=list(SHAPES))
    ap.add_argument("--loop-shapes", nargs="*", default=["clips8x3_T64"], choices=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_multi_guide_logits_step.json"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(7)
    head = make_head(dev)
    m = bench.make_projector(bench.release_config(args.hidden, 64), dev)
    rows = []
    with torch.no_grad():
        for name in args.shapes:
            splits, counts = SHAPES[name]
            modals = ["image" if t == 1 else "video" for t in splits]
            sets = [(torch.randn((sum(splits), GRID, GRID, D), device=dev, generator=gen).bfloat16(),
                     torch.randn((sum(counts), D), device=dev, generator=gen).bfloat16()) for _ in range(SETS)]
            scores = lambda s: siglip_head_scores_ragged(s[0], head, s[1], splits, counts)
            new = lambda s: m.forward_ragged_multi_guide(s[0], None, s[1], splits, counts, modals, local_logits=scores(s))
            old = lambda s: m.forward_ragged_multi_guide(s[0], siglip_head_embed(s[0], head), s[1], splits, counts, modals)

            def loop(s):
                return [m.forward_multi_guide(x, None, g, modal, local_logits=siglip_head_scores_multi(x, head, g))
                        for x, g, modal in zip(s[0].split(splits), s[1].split(counts), modals)]

            dev_abs = max(float((a.float() - b.float()).abs().max()) for a, b in zip(new(sets[0]), old(sets[0])))
            # the steps on their own: the compressor steps on precomputed logits / frames_embed (one per input set)
            pre = [(x, g, scores((x, g)), siglip_head_embed(x, head)) for x, g in sets]
            steps = dict(head_scores_ragged=(scores, sets),
                         head_embed=(lambda s: siglip_head_embed(s[0], head), sets),
                         step_logits=(lambda s: m.forward_ragged_multi_guide(s[0], None, s[1], splits, counts, modals, local_logits=s[2]), pre),
                         step_keyed=(lambda s: m.forward_ragged_multi_guide(s[0], s[3], s[1], splits, counts, modals), pre))
            (t_new, sp_new), (t_old, sp_old) = (repeated(fn, sets, args.iters, args.warmup, args.repeats) for fn in (new, old))
            row = dict(shape=name, frames=splits, guides=counts, grid=GRID, hidden=args.hidden, logits_bytes=4 * max(counts) * sum(splits) * GRID * GRID,
                       frames_embed_bytes=2 * sum(splits) * GRID * GRID * D, new_us=round(t_new, 1), new_spread_us=round(sp_new, 1),
                       parent_us=round(t_old, 1), parent_spread_us=round(sp_old, 1), parent_over_new=round(t_old / t_new, 3),
                       new_wins=bool(t_old - t_new > sp_new + sp_old), max_abs_new_vs_parent=dev_abs)
            if name in args.loop_shapes:
                t_loop, sp_loop = repeated(loop, sets, args.iters, args.warmup, args.repeats)
                row.update(per_clip_loop_us=round(t_loop, 1), per_clip_loop_spread_us=round(sp_loop, 1), per_clip_loop_over_new=round(t_loop / t_new, 3))
            for step, (fn, data) in steps.items():
                t, sp = repeated(fn, data, args.iters, args.warmup, args.repeats)
                row[step + "_us"], row[step + "_spread_us"] = round(t, 1), round(sp, 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del sets, pre
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/ragged_multi_guide_logits_bench.py", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       repeats=args.repeats,
                       timing="HIP-event intervals around one whole pipeline (head step + compressor step) or one step; median of `iters` intervals, "
                              "repeated `repeats` times: median of the medians and their range (the spread); inputs rotate through 3 sets; "
                              "new_wins: parent - new > the two spreads together",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
