"""Times one training step -- zero_grad, forward, loss, backward to .grad -- of HIComProjector.forward_ragged_multi_guide_train against the two
things a user can do without it, in the same process:
  replicated  forward_ragged_train on every item's tokens replicated Q_i times, the replication inside the timed region;
  loop        forward() + backward() per (item, guide) pair, `graph_backward` at its default (warmed until its backward graphs are captured
              where the four-entry cache admits them).
A point whose items all have one guide is timed against forward_ragged_train itself (no replication).  HIP events, after warm-up; inputs
rotate through three sets; median and run-to-run range.  All points at 27 x 27, hidden 896.  Also reports the bytes the autograd node saves
per token.  Writes profiles/ragged_multi_guide_train_step.json.

    python tools/ragged_multi_guide_train_bench.py [--iters 20] [--warmup 6] [--out profiles/ragged_multi_guide_train_step.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from batch_bench import recipe_projector, D, GRID, SETS           # noqa: E402
from ragged_train_bench import timed                              # noqa: E402

# name -> (frames per item, guides per item)
POINTS = {
    "8 clips x 8 frames x 3 guides": ([8] * 8, [3] * 8),
    "16 images x 4 guides": ([1] * 16, [4] * 16),
    "4 clips x 64 frames x 3 guides": ([64] * 4, [3] * 4),
    "1 clip x 8 frames x 3 guides": ([8], [3]),
    "8 clips x 8 frames x 1 guide": ([8] * 8, [1] * 8),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--points", default=None, help="comma-separated substrings of the point names to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_multi_guide_train_step.json"))
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
        sets = [tuple(torch.randn(s, device=dev, generator=gen).bfloat16()
                      for s in ((frames, GRID, GRID, D), (frames, GRID, GRID, D), (M, D))) for _ in range(SETS)]

        def new(s):
            m.zero_grad(set_to_none=True)
            sum(o.float().sum() for o in m.forward_ragged_multi_guide_train(s[0], s[1], s[2], splits, counts, modals)).backward()

        def replicated(s):
            m.zero_grad(set_to_none=True)
            if single:
                ff, fe = s[0], s[1]
            else:                                                   # the token-sized copies are part of what this path costs
                ff = torch.cat([s[0][t0[i]:t0[i] + splits[i]] for i, _ in pairs])
                fe = torch.cat([s[1][t0[i]:t0[i] + splits[i]] for i, _ in pairs])
            sum(o.float().sum() for o in m.forward_ragged_train(ff, fe, s[2], rep_splits, rep_modals)).backward()

        def loop(s):
            m.zero_grad(set_to_none=True)
            for i, q in pairs:
                m(s[0][t0[i]:t0[i] + splits[i]], s[1][t0[i]:t0[i] + splits[i]], s[2][pair0[i] + q], modals[i]).float().sum().backward()

        new(sets[0])
        g_new = {n: p.grad.float().clone() for n, p in m.named_parameters() if p.grad is not None}
        replicated(sets[0])
        rel = max(float((p.grad.float() - g_new[n]).abs().max() / (g_new[n].abs().max() + 1e-30)) for n, p in m.named_parameters() if p.grad is not None)
        plan = next(reversed(m.__dict__["_ragged_multi_guide_plans"].values()))
        t = plan.tables
        R = M * plan.io.nh
        saved = sum(q * w for q, w in zip(t.Q, t.windows)) * D * 2 + 16 * sum(p * 32 * n for p, n in zip(t.passes, t.ntiles)) * 4 + R * 2 * 4 + R * D * 4
        t_new, t_rep, t_loop = (timed(f, sets, args.iters, args.warmup) for f in (new, replicated, loop))
        graphs = sum(1 for e in m.__dict__.get("_bwd_graphs", {}).values() if "graph" in e)
        best = min(("train", t_new[0]), ("replicated", t_rep[0]), ("loop", t_loop[0]), key=lambda kv: kv[1])[0]
        row = dict(point=name, B=B, frames=frames, pairs=M, grid=GRID, hidden=args.hidden, train_us=t_new[0], train_min_us=t_new[1], train_max_us=t_new[2],
                   replicated_us=t_rep[0], replicated_min_us=t_rep[1], replicated_max_us=t_rep[2], replicated_is="forward_ragged_train itself" if single
                   else "forward_ragged_train on replicated tokens", loop_us=t_loop[0], loop_min_us=t_loop[1], loop_max_us=t_loop[2],
                   replicated_over_train=round(t_rep[0] / t_new[0], 2), loop_over_train=round(t_loop[0] / t_new[0], 2), fastest=best,
                   loop_backward_graphs=graphs, saved_bytes_per_token=round(saved / (frames * GRID * GRID), 1), max_rel_grad_diff_vs_replicated=rel)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del sets
        m.__dict__.pop("_bwd_graphs", None)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/ragged_multi_guide_train_bench.py", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       timing="median (min, max) of HIP-event intervals around one training step: zero_grad, forward, loss, backward to .grad; "
                              "train = forward_ragged_multi_guide_train, replicated = forward_ragged_train on tokens replicated Q_i times (the copies "
                              "timed), loop = forward() + backward() per pair with graph_backward at its default; inputs rotate through 3 sets",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
