"""Times HIComProjector.forward_multi_guide (one clip, Q instructions, one call) against the two ways the project had before it, on the
same inputs: the loop of Q forward() calls (the baseline), and forward_batch on the Q-fold replicated clip (the replication copy counted).
One process, HIP events, after warm-up; inputs rotate through three sets.  Writes profiles/multi_guide_step.json.

    python tools/multi_guide_bench.py [--frames 64 8] [--guides 1 3 6 16] [--iters 30] [--warmup 5] [--out profiles/multi_guide_step.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--frames", type=int, nargs="+", default=[64, 8])
    ap.add_argument("--guides", type=int, nargs="+", default=[1, 3, 6, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_guide_step.json"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(7)
    rows = []
    with torch.no_grad():
        for T in args.frames:
            m = bench.make_projector(bench.release_config(args.hidden, T), dev)
            clips = [tuple(torch.randn((T, GRID, GRID, D), device=dev, generator=gen).bfloat16() for _ in range(2)) for _ in range(SETS)]
            for Q in args.guides:
                sets = [clip + (torch.randn((Q, D), device=dev, generator=gen).bfloat16(),) for clip in clips]
                multi = lambda s: m.forward_multi_guide(s[0], s[1], s[2], "video")
                loop = lambda s: [m(s[0], s[1], s[2][q], "video") for q in range(Q)]
                # (expand is a view: forward_batch's .contiguous() writes the Q copies, inside the timed interval)
                batch = lambda s: m.forward_batch(s[0].expand(Q, *s[0].shape), s[1].expand(Q, *s[1].shape), s[2], "video")
                want = torch.stack(loop(sets[0])).float()
                dev_abs = float((multi(sets[0]).float() - want).abs().max())
                t_m, t_l, t_b = (timed(fn, sets, args.iters, args.warmup) for fn in (multi, loop, batch))
                rows.append(dict(T=T, Q=Q, grid=GRID, hidden=args.hidden, multi_guide_us=round(t_m, 1), loop_us=round(t_l, 1),
                                 batch_replicated_us=round(t_b, 1), loop_over_multi=round(t_l / t_m, 2), batch_over_multi=round(t_b / t_m, 2),
                                 max_abs_vs_loop=dev_abs))
                print(json.dumps(rows[-1]), flush=True)
                del sets
            del clips, m
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/multi_guide_bench.py", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       timing="median of HIP-event intervals around one forward_multi_guide call, the Q-call forward() loop, or forward_batch on "
                              "the expanded clip (its replication copy included); inputs rotate through 3 sets",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
