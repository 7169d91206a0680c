"""Times one training step -- forward + backward to .grad -- of HIComProjector.forward_ragged_train against the loop it replaces: forward()
+ backward() per item, `graph_backward` at its default (the loop is warmed until its backward graphs are captured where the four-entry
cache admits them).  One process, HIP events, after warm-up; inputs rotate through three sets; median and range.  All points at
27 x 27, hidden 896.  Also reports the kernel launches of the backward and the bytes the autograd node saves per token.  Writes
profiles/ragged_train_step.json.

    python tools/ragged_train_bench.py [--iters 20] [--warmup 6] [--out profiles/ragged_train_step.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from batch_bench import recipe_projector, D, GRID, SETS           # noqa: E402

# name -> frames per item ("image" for 1, "video" otherwise)
POINTS = {
    "16 images": [1] * 16,
    "8 clips x 8 frames": [8] * 8,
    "mix (1, 8, 1, 16, 1, 4)": [1, 8, 1, 16, 1, 4],
    "4 clips x 64 frames": [64] * 4,
    "1 image": [1],
    "2 images": [1, 1],
}


def timed(fn, sets, iters, warmup):
    """(median, min, max) in microseconds of HIP-event intervals around fn(set)."""
    for i in range(warmup):
        fn(sets[i % SETS])
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for i, (a, b) in enumerate(evs):
        a.record()
        fn(sets[i % SETS])
        b.record()
    torch.cuda.synchronize()
    us = [a.elapsed_time(b) * 1e3 for a, b in evs]
    return round(statistics.median(us), 1), round(min(us), 1), round(max(us), 1)


def backward_launches(m, make_loss):
    """Device kernels and copies of one backward, counted by the profiler; None where it cannot."""
    try:
        from torch.profiler import ProfilerActivity, profile
        loss = make_loss()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            loss.backward()
            torch.cuda.synchronize()
        m.zero_grad(set_to_none=True)
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    except Exception:  # noqa: BLE001
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--points", default=None, help="comma-separated substrings of the point names to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_train_step.json"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    m = recipe_projector("plain", args.hidden, 64, dev).train()
    gen = torch.Generator(device=dev).manual_seed(7)
    rows = []
    for name, splits in POINTS.items():
        if args.points and not any(s in name for s in args.points.split(",")):
            continue
        modals = ["image" if t == 1 else "video" for t in splits]
        B, frames = len(splits), sum(splits)
        t0 = [sum(splits[:i]) for i in range(B)]
        sets = [tuple(torch.randn(s, device=dev, generator=gen).bfloat16()
                      for s in ((frames, GRID, GRID, D), (frames, GRID, GRID, D), (B, D))) for _ in range(SETS)]

        def new_loss(s):
            return sum(o.float().sum() for o in m.forward_ragged_train(s[0], s[1], s[2], splits, modals))

        def new(s):
            m.zero_grad(set_to_none=True)
            new_loss(s).backward()

        def loop(s):
            m.zero_grad(set_to_none=True)
            for i in range(B):
                m(s[0][t0[i]:t0[i] + splits[i]], s[1][t0[i]:t0[i] + splits[i]], s[2][i], modals[i]).float().sum().backward()

        new(sets[0])
        g_new = {n: p.grad.float().clone() for n, p in m.named_parameters() if p.grad is not None}
        loop(sets[0])
        rel = max(float((p.grad.float() - g_new[n]).abs().max() / (g_new[n].abs().max() + 1e-30)) for n, p in m.named_parameters() if p.grad is not None)
        launches = backward_launches(m, lambda: new_loss(sets[0]))
        plan = next(reversed(m.__dict__["_ragged_plans"].values()))
        t = plan.tables
        R = B * plan.io.nh
        saved = sum(t.windows) * D * 2 + 16 * 16 * sum(t.ntiles) * 4 + R * 2 * 4 + R * D * 4
        t_new, t_loop = timed(new, sets, args.iters, args.warmup), timed(loop, sets, args.iters, args.warmup)
        graphs = sum(1 for e in m.__dict__.get("_bwd_graphs", {}).values() if "graph" in e)
        row = dict(point=name, B=B, frames=frames, grid=GRID, hidden=args.hidden, train_us=t_new[0], train_min_us=t_new[1], train_max_us=t_new[2],
                   loop_us=t_loop[0], loop_min_us=t_loop[1], loop_max_us=t_loop[2], loop_over_train=round(t_loop[0] / t_new[0], 2),
                   loop_backward_graphs=graphs, backward_launches=launches, saved_bytes_per_token=round(saved / (frames * GRID * GRID), 1),
                   max_rel_grad_diff_vs_loop=rel)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del sets
        m.__dict__.pop("_bwd_graphs", None)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/ragged_train_bench.py", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       timing="median (min, max) of HIP-event intervals around one training step: zero_grad, forward, loss, backward to .grad; "
                              "train = forward_ragged_train, loop = forward() + backward() per item with graph_backward at its default; "
                              "inputs rotate through 3 sets",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
