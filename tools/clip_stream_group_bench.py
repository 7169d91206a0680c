"""Times one push of a clip stream group (HIComProjector.open_stream_group) against what the project had for B live
videos: a loop of B ClipStream.push calls (open_stream, §3.12) on the same stacked chunk tensor, in the same process.  27 x 27 x 1152,
hidden 896, B = 1, 4, 16, 32 slots, chunks of 8 and 16 frames, 32 frames per slot.  The protocol of tools/clip_stream_bench.py: HIP events,
after warm-up, inputs rotating through resident stacks.  Writes profiles/clip_stream_group_step.json.

Per (chunk, B): push_us of the group (median of one HIP-event interval around a push of all B slots), loop_push_us of the B single streams
(one interval around the B pushes of a tick), the ratio loop / group, the largest difference between the two finished results, and the
peak device bytes each path allocated from open to the last finish (torch.cuda.max_memory_allocated, the stacks excluded).

    python tools/clip_stream_group_bench.py [--frames 32] [--chunks 8 16] [--slots 1 4 16 32] [--iters 6] [--warmup 2] [--out ...]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from batch_bench import D, GRID, recipe_projector            # noqa: E402

SETS = 2


def tick_times(push, reset, stacks, ticks, iters, warmup):
    """Median time of one tick (all B slots pushed) in microseconds; push(ff, fe) acts on the group or on all B single streams."""
    times = []
    for it in range(warmup + iters):
        ff, fe = stacks[it % SETS]
        reset()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(ticks + 1)]
        evs[0].record()
        for i in range(ticks):
            push(ff, fe)
            evs[i + 1].record()
        torch.cuda.synchronize()
        if it >= warmup:
            times += [evs[i].elapsed_time(evs[i + 1]) * 1e3 for i in range(ticks)]
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--chunks", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--slots", type=int, nargs="+", default=[1, 4, 16, 32])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_stream_group_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/clip_stream_group_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(7)
    T = args.frames
    rows = []
    with torch.no_grad():
        m = recipe_projector("plain", args.hidden, T, dev)
        for chunk in args.chunks:
            ticks = T // chunk
            for B in args.slots:
                g = torch.randn((B, D), device=dev, generator=gen).bfloat16()
                stacks = [tuple(torch.randn((B * chunk, GRID, GRID, D), device=dev, generator=gen).bfloat16() for _ in range(2)) for _ in range(SETS)]
                sizes = [chunk] * B
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                group = m.open_stream_group(g, GRID, GRID, T)
                t_group = tick_times(lambda ff, fe: group.push(ff, fe, sizes), lambda: [group.reset(s) for s in range(B)], stacks, ticks, args.iters,
                                     args.warmup)
                got = [group.finish(s).float().clone() for s in range(B)]
                torch.cuda.synchronize()
                peak_group = torch.cuda.max_memory_allocated() - base
                del group
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                singles = [m.open_stream(g[s], GRID, GRID, T) for s in range(B)]
                t_loop = tick_times(lambda ff, fe: [s.push(ff[i * chunk:(i + 1) * chunk], fe[i * chunk:(i + 1) * chunk]) for i, s in enumerate(singles)],
                                    lambda: [s.reset() for s in singles], stacks, ticks, args.iters, args.warmup)
                diff = max(float((got[i] - s.finish().float()).abs().max()) for i, s in enumerate(singles))       # (both sides hold the same stack)
                torch.cuda.synchronize()
                peak_loop = torch.cuda.max_memory_allocated() - base
                row = dict(grid=GRID, hidden=args.hidden, chunk=chunk, B=B, ticks=ticks, push_us=round(t_group, 1), loop_push_us=round(t_loop, 1),
                           loop_over_group=round(t_loop / t_group, 2), max_abs_vs_loop=diff, peak_bytes_group=int(peak_group), peak_bytes_loop=int(peak_loop))
                rows.append(row)
                print(json.dumps(row), flush=True)
                del singles, stacks, got
                torch.cuda.empty_cache()
    wins = {str(c): next((r["B"] for r in rows if r["chunk"] == c and r["loop_over_group"] >= 1.0), None) for c in args.chunks}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/clip_stream_group_bench.py", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       timing="medians of HIP-event intervals around one tick: one push of the group resp. the B pushes of the B single-guide streams "
                              "on slices of the same stack (over every tick of every timed pass); inputs rotate through 2 resident stacks",
                       baseline="B ClipStreams (open_stream) pushed one after the other: the path of the parent commit, untouched",
                       smallest_B_at_which_the_group_does_not_lose=wins, rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
