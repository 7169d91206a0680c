"""Times the multi-guide step WITHOUT frames_embed against the pipeline it replaces, on the same box and the same inputs:

    new      siglip_head_scores_multi(x, head, guides)  ->  forward_multi_guide(x, None, guides, "video", local_logits=L)
    parent   siglip_head_embed(x, head)                 ->  forward_multi_guide(x, fe, guides, "video")

(the tower's hidden states double as frames_feature, as in bench.py's neighbours sweep; the head has the so400m widths 1152 -> 4304 -> 1152).
The head step and the compressor step of either pipeline are timed on their own as well.  One process, HIP events around one whole
pipeline (or step), after warm-up; inputs rotate through three sets; every figure is the median of `iters` intervals, measured `repeats`
times: the median of those medians is reported, and their range (max - min) as the run-to-run spread.  `new_wins` says whether the new
pipeline is faster by more than the two spreads together.  Writes profiles/multi_guide_logits_step.json.

    python tools/multi_guide_logits_bench.py [--frames 64 8] [--guides 1 3 6 16] [--iters 20] [--warmup 5] [--repeats 3]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench                                           # noqa: E402  (release_config / make_projector: the benchmark's module)
from batch_bench import D, GRID, SETS, timed            # noqa: E402
from hicom_amd import siglip_head_embed, siglip_head_scores_multi           # noqa: E402

INTER = 4304


def make_head(dev):
    head = torch.nn.Module()
    head.layernorm = torch.nn.LayerNorm(D, eps=1e-6)
    head.mlp = torch.nn.Module()
    head.mlp.fc1, head.mlp.fc2 = torch.nn.Linear(D, INTER), torch.nn.Linear(INTER, D)
    return head.to(torch.bfloat16).to(dev).eval()


def repeated(fn, sets, iters, warmup, repeats):
    """(median of the repeats' medians, their range), microseconds."""
    meds = [timed(fn, sets, iters, warmup) for _ in range(repeats)]
    return statistics.median(meds), max(meds) - min(meds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--frames", type=int, nargs="+", default=[64, 8])
    ap.add_argument("--guides", type=int, nargs="+", default=[1, 3, 6, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_guide_logits_step.json"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(7)
    head = make_head(dev)
    rows = []
    with torch.no_grad():
        for T in args.frames:
            m = bench.make_projector(bench.release_config(args.hidden, T), dev)
            clips = [torch.randn((T, GRID, GRID, D), device=dev, generator=gen).bfloat16() for _ in range(SETS)]
            for Q in args.guides:
                sets = [(x, torch.randn((Q, D), device=dev, generator=gen).bfloat16()) for x in clips]
                new = lambda s: m.forward_multi_guide(s[0], None, s[1], "video", local_logits=siglip_head_scores_multi(s[0], head, s[1]))
                old = lambda s: m.forward_multi_guide(s[0], siglip_head_embed(s[0], head), s[1], "video")
                dev_abs = float((new(sets[0]).float() - old(sets[0]).float()).abs().max())
                # the steps on their own: the compressor steps on precomputed logits / frames_embed (one per input set)
                pre = [(x, g, siglip_head_scores_multi(x, head, g), siglip_head_embed(x, head)) for x, g in sets]
                steps = dict(head_scores_multi=(lambda s: siglip_head_scores_multi(s[0], head, s[1]), sets),
                             head_embed=(lambda s: siglip_head_embed(s[0], head), sets),
                             step_logits=(lambda s: m.forward_multi_guide(s[0], None, s[1], "video", local_logits=s[2]), pre),
                             step_keyed=(lambda s: m.forward_multi_guide(s[0], s[3], s[1], "video"), pre))
                (t_new, sp_new), (t_old, sp_old) = (repeated(fn, sets, args.iters, args.warmup, args.repeats) for fn in (new, old))
                row = dict(T=T, Q=Q, grid=GRID, hidden=args.hidden, new_us=round(t_new, 1), new_spread_us=round(sp_new, 1), parent_us=round(t_old, 1),
                           parent_spread_us=round(sp_old, 1), parent_over_new=round(t_old / t_new, 3), new_wins=bool(t_old - t_new > sp_new + sp_old),
                           max_abs_new_vs_parent=dev_abs)
                for name, (fn, data) in steps.items():
                    t, sp = repeated(fn, data, args.iters, args.warmup, args.repeats)
                    row[name + "_us"], row[name + "_spread_us"] = round(t, 1), round(sp, 1)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del sets, pre
            del clips, m
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/multi_guide_logits_bench.py", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       repeats=args.repeats,
                       timing="HIP-event intervals around one whole pipeline (head step + compressor step) or one step; median of `iters` intervals, "
                              "repeated `repeats` times: median of the medians and their range (the spread); inputs rotate through 3 sets; "
                              "new_wins: parent - new > the two spreads together",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
