"""Times one chunk of a clip stream WITHOUT frames_embed against the pipeline it replaces, on the same box and the same
inputs:

    new      L = s.head_scores(x, head)       ->  s.push(x, None, local_logits=L)
    parent   fe = siglip_head_embed(x, head)  ->  s.push(x, fe)

for ClipStream (Q = 1), ClipStreamMulti (Q = 1 / 3 / 16) in chunks of 8 and 16 frames, and for ClipStreamGroupMulti with B = 4 and 16 slots
of 3 guides, 8 frames per slot and tick (g.head_scores(x, head, split_sizes, slots) / g.push(x, fe, split_sizes, slots)).  The tower's
hidden states double as frames_feature, as in tools/multi_guide_logits_bench.py; the head has the so400m widths 1152 -> 4304 -> 1152; 27 x 27,
hidden 896.  Each pipeline pushes into a stream of its own (a clip keeps one form), opened for warmup + iters chunks and reset in front of
every measurement, outside the timed region.  One process, HIP events around one whole chunk's work, after warm-up; inputs rotate through
three sets; every figure is the median of `iters` intervals, measured `repeats` times: the median of those medians is reported, and their
range (max - min) as the run-to-run spread.  `verdict` is "win" / "loss" only if the gap exceeds the two spreads together, "level" otherwise.
The head step and the push of either pipeline are timed on their own as well.  Writes profiles/clip_stream_logits_step.json.

    python tools/clip_stream_logits_bench.py [--chunks 8 16] [--guides 1 3 16] [--slots 4 16] [--iters 20] [--warmup 5] [--repeats 3]"""
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
from hicom_amd import siglip_head_embed                 # noqa: E402
from multi_guide_logits_bench import make_head          # noqa: E402

GROUP_GUIDES, GROUP_FRAMES = 3, 8


def verdict(t_new, sp_new, t_old, sp_old):
    gap = t_old - t_new
    return "win" if gap > sp_new + sp_old else "loss" if -gap > sp_new + sp_old else "level"


def measure(fn, sets, reset, iters, warmup, repeats):
    """(median of the repeats' medians, their range), microseconds; reset() empties the stream in front of every repeat."""
    meds = []
    for _ in range(repeats):
        reset()
        meds.append(timed(fn, sets, iters, warmup))
    return statistics.median(meds), max(meds) - min(meds)


def row_of(kind, shape, pipelines, steps, sets, pre, args):
    """pipelines: {"new" | "parent": (fn, reset)}; steps: {name: (fn, reset, data)}."""
    row = dict(kind=kind, grid=GRID, hidden=args.hidden, **shape)
    for name, (fn, reset) in pipelines.items():
        t, sp = measure(fn, sets, reset, args.iters, args.warmup, args.repeats)
        row[name + "_us"], row[name + "_spread_us"] = round(t, 1), round(sp, 1)
    row["parent_over_new"] = round(row["parent_us"] / row["new_us"], 3)
    row["verdict"] = verdict(row["new_us"], row["new_spread_us"], row["parent_us"], row["parent_spread_us"])
    for name, (fn, reset, data) in steps.items():
        t, sp = measure(fn, data, reset, args.iters, args.warmup, args.repeats)
        row[name + "_us"], row[name + "_spread_us"] = round(t, 1), round(sp, 1)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--chunks", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--guides", type=int, nargs="+", default=[1, 3, 16])
    ap.add_argument("--slots", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_stream_logits_step.json"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(7)
    head = make_head(dev)
    pushes = args.iters + args.warmup
    nothing = lambda: None
    rows = []
    with torch.no_grad():
        for Tc in args.chunks:
            cap = Tc * pushes
            m = bench.make_projector(bench.release_config(args.hidden, cap), dev)
            sets = [torch.randn((Tc, GRID, GRID, D), device=dev, generator=gen).bfloat16() for _ in range(SETS)]
            for kind, Q in [("ClipStream", 1)] + [("ClipStreamMulti", Q) for Q in args.guides]:
                g = torch.randn((Q, D), device=dev, generator=gen).bfloat16()
                opener = (lambda: m.open_stream(g[0], GRID, GRID, cap)) if kind == "ClipStream" else (lambda: m.open_stream_multi(g, GRID, GRID, cap))
                new, old = opener(), opener()
                pre = [(x, new.head_scores(x, head), siglip_head_embed(x, head)) for x in sets]
                rows.append(row_of(kind, dict(Tc=Tc, Q=Q), {
                    "new": (lambda x: new.push(x, None, local_logits=new.head_scores(x, head)), new.reset),
                    "parent": (lambda x: old.push(x, siglip_head_embed(x, head)), old.reset),
                }, {
                    "head_scores": (lambda s: new.head_scores(s[0], head), nothing, pre),
                    "head_embed": (lambda s: siglip_head_embed(s[0], head), nothing, pre),
                    "push_logits": (lambda s: new.push(s[0], None, local_logits=s[1]), new.reset, pre),
                    "push_keyed": (lambda s: old.push(s[0], s[2]), old.reset, pre),
                }, sets, pre, args))
                del new, old, pre
            del m, sets
            torch.cuda.empty_cache()
        Tc, cap = GROUP_FRAMES, GROUP_FRAMES * pushes
        m = bench.make_projector(bench.release_config(args.hidden, cap), dev)
        for B in args.slots:
            counts, sizes, slots = (GROUP_GUIDES,) * B, (Tc,) * B, list(range(B))
            g = torch.randn((GROUP_GUIDES * B, D), device=dev, generator=gen).bfloat16()
            sets = [torch.randn((Tc * B, GRID, GRID, D), device=dev, generator=gen).bfloat16() for _ in range(SETS)]
            new, old = (m.open_stream_group_multi(g, counts, GRID, GRID, cap) for _ in range(2))

            def reset_of(grp):
                return lambda: [grp.reset(s) for s in slots]
            pre = [(x, new.head_scores(x, head, sizes, slots), siglip_head_embed(x, head)) for x in sets]
            rows.append(row_of("ClipStreamGroupMulti", dict(B=B, Q=GROUP_GUIDES, Tc=Tc), {
                "new": (lambda x: new.push(x, None, sizes, slots, local_logits=new.head_scores(x, head, sizes, slots)), reset_of(new)),
                "parent": (lambda x: old.push(x, siglip_head_embed(x, head), sizes, slots), reset_of(old)),
            }, {
                "head_scores": (lambda s: new.head_scores(s[0], head, sizes, slots), nothing, pre),
                "head_embed": (lambda s: siglip_head_embed(s[0], head), nothing, pre),
                "push_logits": (lambda s: new.push(s[0], None, sizes, slots, local_logits=s[1]), reset_of(new), pre),
                "push_keyed": (lambda s: old.push(s[0], s[2], sizes, slots), reset_of(old), pre),
            }, sets, pre, args))
            del new, old, pre, sets
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/clip_stream_logits_bench.py", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       repeats=args.repeats,
                       timing="HIP-event intervals around one whole chunk's work (head step + push) or one step; median of `iters` intervals, "
                              "repeated `repeats` times: median of the medians and their range (the spread); inputs rotate through 3 sets; the "
                              "streams are reset in front of every repeat, outside the timed region; verdict: win / loss only if the gap exceeds "
                              "the two spreads together",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
