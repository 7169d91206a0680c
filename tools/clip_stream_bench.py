"""Times the clip stream (HIComProjector.open_stream) against forward() on the whole clip, on the same module and inputs:
64 and 512 frames of 27 x 27 x 1152, hidden 896, pushed in chunks of 8, 16 and 64 frames.  forward() is not touched by the stream, so the
yardstick measured here is the one-call step as the parent commit has it, on the same box in the same process.  The protocol of
tools/multi_guide_bench.py: one process, HIP events, after warm-up, inputs rotating through three clips (for timing the clips are resident
and a push takes a slice, so no token is in a cache from the pass before: three clips of 64 frames are 645 MB).  Writes
profiles/clip_stream_step.json.

Per (frames, chunk) it reports push_us (median over all pushes of one HIP-event interval around a push), stream_us (all pushes + finish()),
finish_us, forward_us (one forward() on the whole clip) and the peak device memory of both sides beyond the module: stream_peak_bytes with ONE
chunk pair resident (what a chunked vision tower needs), forward_peak_bytes with the whole pair resident.

    python tools/clip_stream_bench.py [--frames 64 512] [--chunks 8 16 64] [--iters 10] [--warmup 3] [--out profiles/clip_stream_step.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from batch_bench import D, GRID, SETS, recipe_projector, timed            # noqa: E402


def stream_times(s, clips, chunk, iters, warmup):
    """(median push, median whole stream, median finish) in microseconds."""
    T = clips[0][0].shape[0]
    push, whole, fin = [], [], []
    for it in range(warmup + iters):
        ff, fe = clips[it % SETS]
        s.reset()
        n = T // chunk
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 2)]
        evs[0].record()
        for i in range(n):
            s.push(ff[i * chunk:(i + 1) * chunk], fe[i * chunk:(i + 1) * chunk])
            evs[i + 1].record()
        s.finish()
        evs[n + 1].record()
        torch.cuda.synchronize()
        if it >= warmup:
            push += [evs[i].elapsed_time(evs[i + 1]) * 1e3 for i in range(n)]
            fin.append(evs[n].elapsed_time(evs[n + 1]) * 1e3)
            whole.append(evs[0].elapsed_time(evs[n + 1]) * 1e3)
    return statistics.median(push), statistics.median(whole), statistics.median(fin)


def peak_beyond(base, fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    keep = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del keep
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--frames", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--chunks", type=int, nargs="+", default=[8, 16, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_stream_step.json"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(7)
    rows = []
    with torch.no_grad():
        for T in args.frames:
            m = recipe_projector("plain", args.hidden, T, dev)
            g = torch.randn((D,), device=dev, generator=gen).bfloat16()
            m(*(torch.randn((T, GRID, GRID, D), device=dev, generator=gen).bfloat16() for _ in range(2)), g, "video")      # plans and tables
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()

            def whole_clip():
                ff, fe = (torch.randn((T, GRID, GRID, D), device=dev, generator=gen).bfloat16() for _ in range(2))
                return ff, fe, m(ff, fe, g, "video")
            forward_peak = peak_beyond(base, whole_clip)
            for chunk in args.chunks:
                def chunked():
                    s = m.open_stream(g, GRID, GRID, T)
                    ff, fe = (torch.randn((chunk, GRID, GRID, D), device=dev, generator=gen).bfloat16() for _ in range(2))
                    for _ in range(T // chunk):
                        s.push(ff, fe)
                    return s, ff, fe, s.finish()
                rows.append(dict(T=T, chunk=chunk, stream_peak_bytes=peak_beyond(base, chunked), forward_peak_bytes=forward_peak))
            clips = [tuple(torch.randn((T, GRID, GRID, D), device=dev, generator=gen).bfloat16() for _ in range(2)) for _ in range(SETS)]
            t_fwd = timed(lambda c: m(c[0], c[1], g, "video"), clips, args.iters, args.warmup)
            want = m(clips[0][0], clips[0][1], g, "video").float()
            for row in rows[-len(args.chunks):]:
                s = m.open_stream(g, GRID, GRID, T)
                t_push, t_all, t_fin = stream_times(s, clips, row["chunk"], args.iters, args.warmup)
                s.reset()
                for i in range(T // row["chunk"]):
                    s.push(clips[0][0][i * row["chunk"]:(i + 1) * row["chunk"]], clips[0][1][i * row["chunk"]:(i + 1) * row["chunk"]])
                row.update(grid=GRID, hidden=args.hidden, pushes=T // row["chunk"], push_us=round(t_push, 1), finish_us=round(t_fin, 1),
                           stream_us=round(t_all, 1), forward_us=round(t_fwd, 1), stream_over_forward=round(t_all / t_fwd, 2),
                           max_abs_vs_forward=float((s.finish().float() - want).abs().max()))
                print(json.dumps(row), flush=True)
                del s
            del clips, m, want
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/clip_stream_bench.py", device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
                       timing="medians of HIP-event intervals: around one push (over every push of every timed stream), around all pushes + "
                              "finish(), around finish(), around one forward() on the whole clip; inputs rotate through 3 resident clips",
                       memory="torch.cuda.max_memory_allocated beyond the module and its plans: the stream with ONE chunk pair resident, "
                              "forward() with the whole pair resident",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
