"""Times one stage-3 training step -- zero_grad, forward, loss, backward to .grad with frames_feature, frames_embed and guide_embeds all
requiring grad -- of HIComProjector.forward_ragged_multi_guide_train(input_grads=True) against the two things a user can do without it, in the
same process:
  replicated  forward_ragged_train(input_grads=True) on every item's tokens replicated Q_i times, the replication inside the timed region
              (autograd's cat backward folds the Q_i token-sized gradients back into the item's);
  loop        forward() + backward() per (item, guide) pair, `graph_backward` at its default.
A point whose items all have one guide is timed against forward_ragged_train(input_grads=True) itself (no replication).  HIP events, after
warm-up; inputs rotate through three sets; median and run-to-run range.  The five points of tools/ragged_multi_guide_train_bench.py, at
27 x 27, hidden 896.  Writes profiles/ragged_multi_guide_train_inputs_step.json.

    python tools/ragged_multi_guide_train_inputs_bench.py [--iters 20] [--warmup 6] [--out profiles/ragged_multi_guide_train_inputs_step.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from batch_bench import recipe_projector, D, GRID, SETS           # noqa: E402
from ragged_multi_guide_train_bench import POINTS                 # noqa: E402
from ragged_train_bench import timed                              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--points", default=None, help="comma-separated substrings of the point names to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_multi_guide_train_inputs_step.json"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    m = recipe_projector("plain", args.hidden, 64, dev).train()
    gen = torch.Generator(device=dev).manual_seed(7)
    rows = []
    for name, (splits, counts) in POINTS.items():
        if args.points and not any(s in name for s in args.points.split(",")):
            continue
        modals = ["image" if t == 1 else "video" for t in splits]
        B, frames, M = len(splits), sum(splits), sum(counts)
        t0 = [sum(splits[:i]) for i in range(B)]
        pairs = [(i, q) for i in range(B) for q in range(counts[i])]
        pair0 = [sum(counts[:i]) for i in range(B)]
        rep_splits, rep_modals = [splits[i] for i, _ in pairs], [modals[i] for i, _ in pairs]
        single = all(q == 1 for q in counts)
        sets = [tuple(torch.randn(s, device=dev, generator=gen).bfloat16().requires_grad_(True)
                      for s in ((frames, GRID, GRID, D), (frames, GRID, GRID, D), (M, D))) for _ in range(SETS)]

        def clear(s):
            m.zero_grad(set_to_none=True)
            for t in s:
                t.grad = None

        def new(s):
            clear(s)
            sum(o.float().sum() for o in m.forward_ragged_multi_guide_train(s[0], s[1], s[2], splits, counts, modals, input_grads=True)).backward()

        def replicated(s):
            clear(s)
            if single:
                ff, fe = s[0], s[1]
            else:                                                   # the token-sized copies (and their backward) are part of what this path costs
                ff = torch.cat([s[0][t0[i]:t0[i] + splits[i]] for i, _ in pairs])
                fe = torch.cat([s[1][t0[i]:t0[i] + splits[i]] for i, _ in pairs])
            sum(o.float().sum() for o in m.forward_ragged_train(ff, fe, s[2], rep_splits, rep_modals, input_grads=True)).backward()

        def loop(s):
            clear(s)
            for i, q in pairs:
                m(s[0][t0[i]:t0[i] + splits[i]], s[1][t0[i]:t0[i] + splits[i]], s[2][pair0[i] + q], modals[i]).float().sum().backward()

        new(sets[0])
        g_new = [t.grad.float().clone() for t in sets[0]]
        replicated(sets[0])
        rel = [float((t.grad.float() - g).abs().max() / (g.abs().max() + 1e-30)) for t, g in zip(sets[0], g_new)]
        t_new, t_rep, t_loop = (timed(f, sets, args.iters, args.warmup) for f in (new, replicated, loop))
        best = min(("train", t_new[0]), ("replicated", t_rep[0]), ("loop", t_loop[0]), key=lambda kv: kv[1])[0]
        row = dict(point=name, B=B, frames=frames, pairs=M, grid=GRID, hidden=args.hidden, train_us=t_new[0], train_min_us=t_new[1], train_max_us=t_new[2],
                   replicated_us=t_rep[0], replicated_min_us=t_rep[1], replicated_max_us=t_rep[2],
                   replicated_is="forward_ragged_train(input_grads=True) itself" if single else "forward_ragged_train(input_grads=True) on replicated tokens",
                   loop_us=t_loop[0], loop_min_us=t_loop[1], loop_max_us=t_loop[2], replicated_over_train=round(t_rep[0] / t_new[0], 2),
                   loop_over_train=round(t_loop[0] / t_new[0], 2), fastest=best, train_loses=best != "train",
                   max_rel_diff_vs_replicated=dict(zip(("frames_feature", "frames_embed", "guide_embeds"), rel)))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del sets
        m.__dict__.pop("_bwd_graphs", None)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/ragged_multi_guide_train_inputs_bench.py", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       timing="median (min, max) of HIP-event intervals around one stage-3 training step: zero_grad, forward, loss, backward to .grad "
                              "with frames_feature, frames_embed and guide_embeds requiring grad; train = forward_ragged_multi_guide_train("
                              "input_grads=True), replicated = forward_ragged_train(input_grads=True) on tokens replicated Q_i times (the copies "
                              "timed), loop = forward() + backward() per pair with graph_backward at its default; inputs rotate through 3 sets",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
