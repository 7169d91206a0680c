"""Times one stage-1 / stage-2 training step of a mixed batch WITHOUT frames_embed against the keyed path it replaces, on the
same box, the same projector and the same inputs.  The SigLIP head is frozen; one step is head + forward_ragged_train + backward to .grad:

    new      siglip_head_scores_ragged(x, head, guides, splits, (1,) * B)  ->  forward_ragged_train(x, None, guides, ..., local_logits=L)
    keyed    siglip_head_embed(x, head)                                   ->  forward_ragged_train(x, fe, guides, ...)

(the tower's hidden states double as frames_feature; the head has the so400m widths 1152 -> 4304 -> 1152; the points are those of
tools/ragged_train_bench.py, 27 x 27, hidden 896).  The head step of each pipeline is timed on its own as well.  One process, HIP events
around one whole step after warm-up; inputs rotate through three sets; every figure is the median of `iters` intervals, measured `repeats`
times: the median of those medians is reported, and their range (max - min) as the run-to-run spread.  `new_wins` says whether the new step
is faster than the keyed one by more than the two spreads together, `inside_the_range` whether the two differ by less than that.  Writes
profiles/ragged_train_logits_step.json.

    python tools/ragged_train_logits_bench.py [--points images,mix] [--iters 20] [--warmup 6] [--repeats 3]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from batch_bench import recipe_projector, D, GRID, SETS           # noqa: E402
from hicom_amd import siglip_head_embed, siglip_head_scores_ragged           # noqa: E402
from multi_guide_logits_bench import make_head, repeated          # noqa: E402
from ragged_train_bench import POINTS                              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--points", default=None, help="comma-separated substrings of the point names to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_train_logits_step.json"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    m = recipe_projector("plain", args.hidden, 64, dev).train()
    head = make_head(dev).requires_grad_(False)
    gen = torch.Generator(device=dev).manual_seed(7)
    rows = []
    for name, splits in POINTS.items():
        if args.points and not any(s in name for s in args.points.split(",")):
            continue
        modals = ["image" if t == 1 else "video" for t in splits]
        B, frames = len(splits), sum(splits)
        ones = (1,) * B
        sets = [tuple(torch.randn(s, device=dev, generator=gen).bfloat16() for s in ((frames, GRID, GRID, D), (B, D))) for _ in range(SETS)]

        def scores(s):
            with torch.no_grad():
                return siglip_head_scores_ragged(s[0], head, s[1], splits, ones)

        def embed(s):
            with torch.no_grad():
                return siglip_head_embed(s[0], head)

        def new(s):
            m.zero_grad(set_to_none=True)
            sum(o.float().sum() for o in m.forward_ragged_train(s[0], None, s[1], splits, modals, local_logits=scores(s))).backward()

        def keyed(s):
            m.zero_grad(set_to_none=True)
            sum(o.float().sum() for o in m.forward_ragged_train(s[0], embed(s), s[1], splits, modals)).backward()

        new(sets[0])
        g_new = {n: p.grad.float().clone() for n, p in m.named_parameters() if p.grad is not None}
        keyed(sets[0])
        rel = max(float((p.grad.float() - g_new[n]).abs().max() / (g_new[n].abs().max() + 1e-30)) for n, p in m.named_parameters() if p.grad is not None)
        (t_new, sp_new), (t_old, sp_old) = (repeated(fn, sets, args.iters, args.warmup, args.repeats) for fn in (new, keyed))
        (t_sc, sp_sc), (t_em, sp_em) = (repeated(fn, sets, args.iters, args.warmup, args.repeats) for fn in (scores, embed))
        row = dict(point=name, B=B, frames=frames, grid=GRID, hidden=args.hidden, logits_bytes=4 * frames * GRID * GRID,
                   frames_embed_bytes=2 * frames * GRID * GRID * D, new_us=round(t_new, 1), new_spread_us=round(sp_new, 1), keyed_us=round(t_old, 1),
                   keyed_spread_us=round(sp_old, 1), keyed_over_new=round(t_old / t_new, 3), new_wins=bool(t_old - t_new > sp_new + sp_old),
                   inside_the_range=bool(abs(t_old - t_new) <= sp_new + sp_old), head_scores_us=round(t_sc, 1), head_scores_spread_us=round(sp_sc, 1),
                   head_embed_us=round(t_em, 1), head_embed_spread_us=round(sp_em, 1), max_rel_grad_diff_vs_keyed=rel)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del sets
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/ragged_train_logits_bench.py", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       repeats=args.repeats,
                       timing="HIP-event intervals around one whole training step: frozen head (scores or embed), zero_grad, forward_ragged_train, loss, "
                              "backward to .grad; median of `iters` intervals, repeated `repeats` times: median of the medians and their range (the "
                              "spread); inputs rotate through 3 sets; new_wins: keyed - new > the two spreads together; inside_the_range: |keyed - new| "
                              "<= the two spreads together",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
