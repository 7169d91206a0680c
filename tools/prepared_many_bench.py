"""Times HIComProjector.forward_prepared_many (B prepared clips, clip i with its own Q_i instructions, one call) on the k / v adaptor recipe
(local43_adaptkv_global32) against the ways a caller had before it, on the same inputs: the loop of forward_prepared per clip,
forward_ragged (adaptor recipe: it reruns the adaptor MLPs) on tokens replicated per guide, the replication copy counted, and the loop of
sum Q_i forward() calls.  The protocol of tools/ragged_multi_guide_bench.py: one process, HIP events, median after warm-up; the clips
rotate through three sets of separately allocated clips, so a call reads other tokens and planes than the call before it and writes its
pointer table.  Writes profiles/prepared_many_step.json.

    python tools/prepared_many_bench.py [--shapes clips8x3_T8 ...] [--iters 30] [--warmup 5] [--out profiles/prepared_many_step.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from batch_bench import D, GRID, SETS, recipe_projector, timed            # noqa: E402

# name -> (frames per clip, guides per clip, what it is compared against)
SHAPES = {
    "clips8x3_T8": ([8] * 8, [3] * 8, "prepared_loop"),
    "images16x4": ([1] * 16, [4] * 16, "ragged_replicated"),
    "clips8x3_T64": ([64] * 8, [3] * 8, "forward_loop"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prepared_many_step.json"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(7)
    rows = []
    with torch.no_grad():
        for name in args.shapes:
            frames, counts, against = SHAPES[name]
            m = recipe_projector("adaptkv", args.hidden, max(frames), dev)
            modals = ["image" if t == 1 else "video" for t in frames]
            pairs = [(i, q) for i, n in enumerate(counts) for q in range(n)]
            rep_frames, rep_modals = [frames[i] for i, _ in pairs], [modals[i] for i, _ in pairs]
            rand = lambda *shape: torch.randn(shape, device=dev, generator=gen).bfloat16()
            sets = []
            for _ in range(SETS):           # every clip from tensors of its own
                clips = [m.prepare_clip(rand(t, GRID, GRID, D), rand(t, GRID, GRID, D), modal) for t, modal in zip(frames, modals)]
                sets.append((clips, rand(sum(counts), D)))

            new = lambda s: m.forward_prepared_many(s[0], s[1], counts)
            prepared_loop = lambda s: [m.forward_prepared(clip, g) for clip, g in zip(s[0], s[1].split(counts))]

            def ragged_replicated(s):       # every clip's tokens written Q_i times, then read by forward_ragged, adaptor MLPs included
                ff = torch.cat([s[0][i].ff for i, _ in pairs])
                fe = torch.cat([s[0][i].fe for i, _ in pairs])
                return m.forward_ragged(ff, fe, s[1], rep_frames, rep_modals)

            forward_loop = lambda s: [m(clip.ff, clip.fe, g[q], clip.modal) for clip, g in zip(s[0], s[1].split(counts)) for q in range(g.shape[0])]
            other = dict(prepared_loop=prepared_loop, ragged_replicated=ragged_replicated, forward_loop=forward_loop)[against]
            want = forward_loop(sets[0])
            got = new(sets[0])
            dev_abs = max(float((got[i][q].float() - want[k].float()).abs().max()) for k, (i, q) in enumerate(pairs))
            t_new, t_other = timed(new, sets, args.iters, args.warmup), timed(other, sets, args.iters, args.warmup)
            rows.append(dict(shape=name, frames=frames, guides=counts, pairs=len(pairs), grid=GRID, hidden=args.hidden, prepared_many_us=round(t_new, 1),
                             against=against, against_us=round(t_other, 1), against_over_new=round(t_other / t_new, 2), max_abs_vs_forward_loop=dev_abs))
            print(json.dumps(rows[-1]), flush=True)
            del sets, want, got, m
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/prepared_many_bench.py", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       timing="median of HIP-event intervals around one forward_prepared_many call, the per-clip forward_prepared loop, forward_ragged "
                              "(adaptor recipe) on the per-guide replicated tokens (its torch.cat copies included), or the sum Q_i forward() loop; "
                              "inputs rotate through 3 sets of separately allocated clips",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
