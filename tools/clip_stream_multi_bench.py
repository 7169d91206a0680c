"""Times the multi-guide clip stream (HIComProjector.open_stream_multi) against what the project had for Q questions about a
streamed video: Q single-guide ClipStreams (open_stream, §3.12) pushed one after the other on the same chunks.  64 frames of 27 x 27 x 1152,
hidden 896, chunks of 8 and 16 frames, Q = 1, 3, 6, 16.  The protocol of tools/clip_stream_bench.py: one process, HIP events, after warm-up,
inputs rotating through three resident clips (a push takes a slice).  Writes profiles/clip_stream_multi_step.json.

Per (chunk, Q): push_us / finish_us of the multi-guide stream (medians of one HIP-event interval around a push, around finish()),
loop_push_us / loop_finish_us of the Q single-guide streams (one interval around the Q pushes of a chunk, around the Q finish() calls), the
ratios loop / multi, and the largest difference between the two results.

    python tools/clip_stream_multi_bench.py [--frames 64] [--chunks 8 16] [--guides 1 3 6 16] [--iters 10] [--warmup 3] [--out ...]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from batch_bench import D, GRID, SETS, recipe_projector            # noqa: E402


def stream_times(push, finish, reset, clips, chunk, iters, warmup):
    """(median push, median finish) in microseconds; push(ff, fe) / finish() / reset() act on one multi-guide stream or on all Q streams."""
    T = clips[0][0].shape[0]
    n = T // chunk
    t_push, t_fin = [], []
    for it in range(warmup + iters):
        ff, fe = clips[it % SETS]
        reset()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 2)]
        evs[0].record()
        for i in range(n):
            push(ff[i * chunk:(i + 1) * chunk], fe[i * chunk:(i + 1) * chunk])
            evs[i + 1].record()
        finish()
        evs[n + 1].record()
        torch.cuda.synchronize()
        if it >= warmup:
            t_push += [evs[i].elapsed_time(evs[i + 1]) * 1e3 for i in range(n)]
            t_fin.append(evs[n].elapsed_time(evs[n + 1]) * 1e3)
    return statistics.median(t_push), statistics.median(t_fin)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--chunks", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--guides", type=int, nargs="+", default=[1, 3, 6, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_stream_multi_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/clip_stream_multi_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(7)
    T = args.frames
    rows = []
    with torch.no_grad():
        m = recipe_projector("plain", args.hidden, T, dev)
        clips = [tuple(torch.randn((T, GRID, GRID, D), device=dev, generator=gen).bfloat16() for _ in range(2)) for _ in range(SETS)]
        for chunk in args.chunks:
            for Q in args.guides:
                g = torch.randn((Q, D), device=dev, generator=gen).bfloat16()
                multi = m.open_stream_multi(g, GRID, GRID, T)
                singles = [m.open_stream(g[q], GRID, GRID, T) for q in range(Q)]
                t_push, t_fin = stream_times(multi.push, multi.finish, multi.reset, clips, chunk, args.iters, args.warmup)
                l_push, l_fin = stream_times(lambda ff, fe: [s.push(ff, fe) for s in singles], lambda: [s.finish() for s in singles],
                                             lambda: [s.reset() for s in singles], clips, chunk, args.iters, args.warmup)
                got = multi.finish().float()                         # (both sides hold clip (warmup + iters - 1) % SETS)
                diff = max(float((got[q] - singles[q].finish().float()).abs().max()) for q in range(Q))
                row = dict(T=T, grid=GRID, hidden=args.hidden, chunk=chunk, Q=Q, pushes=T // chunk, push_us=round(t_push, 1), finish_us=round(t_fin, 1),
                           loop_push_us=round(l_push, 1), loop_finish_us=round(l_fin, 1), push_loop_over_multi=round(l_push / t_push, 2),
                           finish_loop_over_multi=round(l_fin / t_fin, 2), max_abs_vs_loop=diff)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del multi, singles
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/clip_stream_multi_bench.py", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       timing="medians of HIP-event intervals: around one push of the multi-guide stream resp. the Q pushes of the Q single-guide "
                              "streams of a chunk (over every chunk of every timed pass), around finish() resp. the Q finish() calls; inputs rotate "
                              "through 3 resident clips",
                       baseline="Q ClipStreams (open_stream) pushed one after the other on the same chunks: the path of the parent commit",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
