"""Times prepared clips on the k / v adaptor recipe (local43_adaptkv_global32): prepare_clip alone, forward_prepared per call, and the
loop of Q forward() calls on the same module -- the only path the project had for this recipe, the baseline -- on the same inputs.  The
protocol of tools/multi_guide_bench.py: one process, HIP events, after warm-up; inputs rotate through three sets (three clips of three
input sets, so a forward_prepared call reads another clip's tokens and planes than the call before it).  Writes
profiles/prepared_clip_step.json.

Per (frames, Q) it reports prepare_us, prepared_us (one forward_prepared call with Q guides), loop_us (Q forward() calls),
single_forward_us (one forward(): against prepared_us at Q = 1 this is the chat pattern) and break_even_calls: the number of calls n of Q
guides from which prepare + n prepared calls beats n loops (None: never, a prepared call is not faster than its loop).

    python tools/prepared_clip_bench.py [--frames 8 64] [--guides 1 3 6 16] [--iters 30] [--warmup 5] [--out profiles/prepared_clip_step.json]"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from batch_bench import D, GRID, SETS, recipe_projector, timed            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--guides", type=int, nargs="+", default=[1, 3, 6, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prepared_clip_step.json"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(7)
    rows = []
    with torch.no_grad():
        for T in args.frames:
            m = recipe_projector("adaptkv", args.hidden, T, dev)
            tokens = [tuple(torch.randn((T, GRID, GRID, D), device=dev, generator=gen).bfloat16() for _ in range(2)) for _ in range(SETS)]
            t_prep = timed(lambda s: m.prepare_clip(s[0], s[1], "video"), tokens, args.iters, args.warmup)
            clips = [m.prepare_clip(ff, fe, "video") for ff, fe in tokens]
            g1 = [tok + (torch.randn((D,), device=dev, generator=gen).bfloat16(),) for tok in tokens]
            t_one = timed(lambda s: m(s[0], s[1], s[2], "video"), g1, args.iters, args.warmup)
            for Q in args.guides:
                sets = [(clip, torch.randn((Q, D), device=dev, generator=gen).bfloat16()) for clip in clips]
                prepared = lambda s: m.forward_prepared(s[0], s[1])
                loop = lambda s: [m(s[0].ff, s[0].fe, s[1][q], "video") for q in range(Q)]
                want = torch.stack(loop(sets[0])).float()
                dev_abs = float((prepared(sets[0]).float() - want).abs().max())
                t_p, t_l = (timed(fn, sets, args.iters, args.warmup) for fn in (prepared, loop))
                even = math.floor(t_prep / (t_l - t_p)) + 1 if t_l > t_p else None
                rows.append(dict(T=T, Q=Q, grid=GRID, hidden=args.hidden, prepare_us=round(t_prep, 1), prepared_us=round(t_p, 1), loop_us=round(t_l, 1),
                                 single_forward_us=round(t_one, 1), loop_over_prepared=round(t_l / t_p, 2), break_even_calls=even,
                                 break_even_questions=None if even is None else even * Q, clip_plane_bytes=clips[0].nbytes, max_abs_vs_loop=dev_abs))
                print(json.dumps(rows[-1]), flush=True)
                del sets
            del clips, tokens, g1, m
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/prepared_clip_bench.py", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       timing="median of HIP-event intervals around one prepare_clip call, one forward_prepared call with Q guides, the Q-call "
                              "forward() loop, or one forward(); inputs rotate through 3 sets (3 clips)",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
