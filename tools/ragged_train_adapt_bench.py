"""Times one training step -- clear the gradients, forward, loss, backward to .grad -- of HIComProjector.forward_ragged_train(adaptors=True)
on the k / v adaptor recipe `local43_adaptkv_global32` against the loop it replaces, forward() + backward() per item on the same module,
both without and with the three inputs requiring grad (input_grads=True).  The points, the timing and the input rotation are
tools/ragged_train_bench.py's (27 x 27, hidden 896, HIP events after warm-up, median and range).  No ratio is fixed in advance: the loop on
the same box is the yardstick, and a point that loses is reported as such (`loop_over_train` < 1).  Writes
profiles/ragged_train_adapt_step.json.

    python tools/ragged_train_adapt_bench.py [--iters 20] [--warmup 6] [--out profiles/ragged_train_adapt_step.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from batch_bench import recipe_projector, D, GRID, SETS           # noqa: E402
from ragged_train_bench import POINTS, backward_launches, timed    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--points", default=None, help="comma-separated substrings of the point names to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_train_adapt_step.json"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    m = recipe_projector("adaptkv", args.hidden, 64, dev).train()
    gen = torch.Generator(device=dev).manual_seed(7)
    rows = []
    for name, splits in POINTS.items():
        if args.points and not any(s in name for s in args.points.split(",")):
            continue
        modals = ["image" if t == 1 else "video" for t in splits]
        B, frames = len(splits), sum(splits)
        t0 = [sum(splits[:i]) for i in range(B)]
        for input_grads in (False, True):
            sets = [tuple(torch.randn(s, device=dev, generator=gen).bfloat16().requires_grad_(input_grads)
                          for s in ((frames, GRID, GRID, D), (frames, GRID, GRID, D), (B, D))) for _ in range(SETS)]

            def clear(s):
                m.zero_grad(set_to_none=True)
                for t in s:
                    t.grad = None

            def new_loss(s):
                return sum(o.float().sum() for o in m.forward_ragged_train(s[0], s[1], s[2], splits, modals, input_grads=input_grads, adaptors=True))

            def new(s):
                clear(s)
                new_loss(s).backward()

            def loop(s):
                clear(s)
                for i in range(B):
                    m(s[0][t0[i]:t0[i] + splits[i]], s[1][t0[i]:t0[i] + splits[i]], s[2][i], modals[i]).float().sum().backward()

            new(sets[0])
            g_new = {n: p.grad.float().clone() for n, p in m.named_parameters() if p.grad is not None}      # (no gradient: the global k_proj.bias)
            loop(sets[0])
            rel = max(float((p.grad.float() - g_new[n]).abs().max() / (g_new[n].abs().max() + 1e-30)) for n, p in m.named_parameters() if n in g_new)
            launches = backward_launches(m, lambda: new_loss(sets[0]))
            t_new, t_loop = timed(new, sets, args.iters, args.warmup), timed(loop, sets, args.iters, args.warmup)
            row = dict(point=name, input_grads=input_grads, B=B, frames=frames, grid=GRID, hidden=args.hidden, train_us=t_new[0], train_min_us=t_new[1],
                       train_max_us=t_new[2], loop_us=t_loop[0], loop_min_us=t_loop[1], loop_max_us=t_loop[2],
                       loop_over_train=round(t_loop[0] / t_new[0], 2), wins=bool(t_loop[0] > t_new[0]), backward_launches=launches,
                       saved_y_bytes_per_token=2 * 2 * D, max_rel_param_grad_diff_vs_loop=rel)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del sets
            m.__dict__.pop("_bwd_graphs", None)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/ragged_train_adapt_bench.py", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       timing="median (min, max) of HIP-event intervals around one training step of local43_adaptkv_global32: clear the gradients, "
                              "forward, loss, backward to .grad; train = forward_ragged_train(adaptors=True), loop = forward() + backward() per item "
                              "(graph_backward at its default; with input_grads the loop's backward is eager); inputs rotate through 3 sets",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
