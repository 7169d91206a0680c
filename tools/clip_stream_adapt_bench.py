"""Times the multi-guide clip stream on the k / v adaptor recipe (HIComProjector.open_stream_adapt) against what the project
had for Q questions about a video on that recipe, both of which need the whole clip resident: prepare_clip + ONE forward_prepared (§3.10),
and Q forward() calls.  64 frames of 27 x 27 x 1152, hidden 896, chunks of 8 and 16 frames, Q = 1, 3, 6, 16.  The protocol of
tools/clip_stream_multi_bench.py: one process, HIP events, after warm-up, inputs rotating through three resident clips (a push takes a
slice).  Writes profiles/clip_stream_adapt_step.json.

Per (chunk, Q): push_us / finish_us (medians of one HIP-event interval around a push, around finish()), total_us (one interval around all
pushes + finish()), prepared_us (prepare_clip + forward_prepared on the resident clip), forward_loop_us (Q forward() calls), the largest
difference between the stream's result and forward_prepared's, and the peak device bytes each path allocates on top of the resident inputs
(the stream: everything open_stream_adapt and its plan own; the prepared path: the clip's planes, the prepare plan and the step's plan).

    python tools/clip_stream_adapt_bench.py [--frames 64] [--chunks 8 16] [--guides 1 3 6 16] [--iters 10] [--warmup 3] [--out ...]"""
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
from clip_stream_multi_bench import stream_times                   # noqa: E402

STORES = ("_clip_stream_adapt_plans", "_prepared_plans", "_prepare_plans", "_engine_plans")


def interval_us(fn, clips, iters, warmup):
    """Median of one HIP-event interval around fn(ff, fe), inputs rotating."""
    ts = []
    for it in range(warmup + iters):
        ff, fe = clips[it % SETS]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(ff, fe)
        b.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def peak_bytes(m, fn):
    """Peak device bytes fn() allocates on top of what is resident now, from a module without plans."""
    for s in STORES:
        m.__dict__.pop(s, None)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    keep = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del keep
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--chunks", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--guides", type=int, nargs="+", default=[1, 3, 6, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_stream_adapt_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/clip_stream_adapt_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(7)
    T = args.frames
    rows = []
    with torch.no_grad():
        m = recipe_projector("adaptkv", args.hidden, T, dev)
        clips = [tuple(torch.randn((T, GRID, GRID, D), device=dev, generator=gen).bfloat16() for _ in range(2)) for _ in range(SETS)]
        for chunk in args.chunks:
            n = T // chunk
            for Q in args.guides:
                g = torch.randn((Q, D), device=dev, generator=gen).bfloat16()

                def run_stream(s, ff, fe):
                    s.reset()
                    for i in range(n):
                        s.push(ff[i * chunk:(i + 1) * chunk], fe[i * chunk:(i + 1) * chunk])
                    return s.finish()

                def run_prepared(ff, fe):
                    return m.forward_prepared(m.prepare_clip(ff, fe, "video"), g)

                def run_forward(ff, fe):
                    return [m(ff, fe, g[q], "video") for q in range(Q)]
                stream_peak = peak_bytes(m, lambda: run_stream(m.open_stream_adapt(g, GRID, GRID, T), *clips[0]))
                prepared_peak = peak_bytes(m, lambda: run_prepared(*clips[0]))
                s = m.open_stream_adapt(g, GRID, GRID, T)
                t_push, t_fin = stream_times(s.push, s.finish, s.reset, clips, chunk, args.iters, args.warmup)
                t_total = interval_us(lambda ff, fe: run_stream(s, ff, fe), clips, args.iters, args.warmup)
                t_prep = interval_us(run_prepared, clips, args.iters, args.warmup)
                t_fwd = interval_us(run_forward, clips, args.iters, args.warmup)
                last = clips[(args.warmup + args.iters - 1) % SETS]
                diff = float((run_stream(s, *last).float() - run_prepared(*last).float()).abs().max())
                row = dict(T=T, grid=GRID, hidden=args.hidden, chunk=chunk, Q=Q, pushes=n, push_us=round(t_push, 1), finish_us=round(t_fin, 1),
                           total_us=round(t_total, 1), prepared_us=round(t_prep, 1), forward_loop_us=round(t_fwd, 1),
                           prepared_over_stream=round(t_prep / t_total, 2), forward_loop_over_stream=round(t_fwd / t_total, 2),
                           stream_peak_bytes=stream_peak, prepared_peak_bytes=prepared_peak, max_abs_vs_prepared=diff)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del s
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/clip_stream_adapt_bench.py", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       timing="medians of HIP-event intervals: around one push (over every chunk of every timed pass), around finish(), around all "
                              "pushes + finish(), around prepare_clip + forward_prepared, around the Q forward() calls; inputs rotate through 3 "
                              "resident clips",
                       baseline="prepare_clip + one forward_prepared on the resident clip, and Q forward() calls: the paths of the parent commit",
                       peak="device bytes allocated on top of the resident inputs, from a module without plans",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
