"""Times one push and one finish of a clip stream group on the k / v adaptor recipe (HIComProjector.open_stream_group_adapt)
against what the project had for B live videos with Q open questions each on an adaptor module: a loop of B ClipStreamAdapt.push calls
(open_stream_adapt, §3.14) on slices of the same stacked chunk tensor, and a loop of B finish calls, in the same process.  27 x 27 x 1152,
hidden 896, chunks of 8 and 16 frames, 32 frames per slot, B = 1, 4, 16 slots x Q = 1, 3, 6 guides per slot.  HIP events, after warm-up,
inputs rotating through resident stacks.  Writes profiles/clip_stream_group_adapt_step.json.

Every cell of the grid runs in a child process of its own under its own time limit; the parent never opens the GPU, and the first cell that
fails or runs out of time ends the run (nothing further is started on the device).

Per (B, Q): push_us of the group (median of one HIP-event interval around a push of all B slots), loop_push_us of the B adaptor streams
(one interval around the B pushes of a tick), finish_many_us (one interval around finish_many of all slots), loop_finish_us (around the B
finish calls), the ratios loop / group, the largest difference between the finished results of the two paths, and the peak device bytes each
path allocates on top of the resident module and inputs (its objects, plans and workspaces, from a module without plans).

    python tools/clip_stream_group_adapt_bench.py [--frames 32] [--chunks 8 16] [--slots 1 4 16] [--guides 1 3 6] [--iters 6] [--warmup 2] [--out ...]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = 2
CELL_SECONDS = 240


def cell(args, B, Q):
    """One (chunk, B, Q) cell on the GPU; prints its JSON row."""
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from batch_bench import D, GRID, recipe_projector
    if not torch.cuda.is_available():
        raise SystemExit("tools/clip_stream_group_adapt_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(7)
    T, chunk = args.frames, args.chunk
    ticks = T // chunk

    def interval(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    def measure(push, finish, reset, stacks):
        """Medians (push of one tick, finish of all slots) in microseconds."""
        pushes, finishes = [], []
        for it in range(args.warmup + args.iters):
            ff, fe = stacks[it % SETS]
            reset()
            evs = [interval(lambda: push(ff, fe)) for _ in range(ticks)] + [interval(finish) for _ in range(3)]
            torch.cuda.synchronize()
            if it >= args.warmup:
                us = [a.elapsed_time(b) * 1e3 for a, b in evs]
                pushes += us[:ticks]
                finishes += us[ticks:]
        return statistics.median(pushes), statistics.median(finishes)

    def peak_bytes(m, run):
        """Peak device bytes of run() above what is resident before it, from a module without plans."""
        m._invalidate_plans()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        keep = run()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del keep
        return int(peak)

    with torch.no_grad():
        m = recipe_projector("adaptkv", args.hidden, T, dev)
        g = torch.randn((B * Q, D), device=dev, generator=gen).bfloat16()
        stacks = [tuple(torch.randn((B * chunk, GRID, GRID, D), device=dev, generator=gen).bfloat16() for _ in range(2)) for _ in range(SETS)]
        sizes = [chunk] * B
        group = m.open_stream_group_adapt(g, [Q] * B, GRID, GRID, T)
        t_push, t_fin = measure(lambda ff, fe: group.push(ff, fe, sizes), group.finish_many, lambda: [group.reset(s) for s in range(B)], stacks)
        got = {s: o.float().clone() for s, o in group.finish_many().items()}
        singles = [m.open_stream_adapt(g[s * Q:(s + 1) * Q].contiguous(), GRID, GRID, T) for s in range(B)]
        l_push, l_fin = measure(lambda ff, fe: [s.push(ff[i * chunk:(i + 1) * chunk], fe[i * chunk:(i + 1) * chunk]) for i, s in enumerate(singles)],
                                lambda: [s.finish() for s in singles], lambda: [s.reset() for s in singles], stacks)
        diff = max(float((got[i] - s.finish().float()).abs().max()) for i, s in enumerate(singles))       # (both sides hold the same stack)
        torch.cuda.synchronize()
        del group, singles, got
        ff, fe = stacks[0]

        def one_group():
            grp = m.open_stream_group_adapt(g, [Q] * B, GRID, GRID, T)
            grp.push(ff, fe, sizes)
            return grp, grp.finish_many()

        def one_loop():
            ss = [m.open_stream_adapt(g[s * Q:(s + 1) * Q].contiguous(), GRID, GRID, T) for s in range(B)]
            return ss, [s.push(ff[i * chunk:(i + 1) * chunk], fe[i * chunk:(i + 1) * chunk]) for i, s in enumerate(ss)], [s.finish() for s in ss]
        group_peak, loop_peak = peak_bytes(m, one_group), peak_bytes(m, one_loop)
    print("ROW " + json.dumps(dict(grid=GRID, hidden=args.hidden, chunk=chunk, B=B, Q=Q, ticks=ticks, push_us=round(t_push, 1), loop_push_us=round(l_push, 1),
                                   loop_over_group_push=round(l_push / t_push, 2), finish_many_us=round(t_fin, 1), loop_finish_us=round(l_fin, 1),
                                   loop_over_group_finish=round(l_fin / t_fin, 2), max_abs_vs_loop=diff, group_peak_bytes=group_peak, loop_peak_bytes=loop_peak, device=torch.cuda.get_device_name(0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--chunks", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--chunk", type=int, default=8, help="(internal) the chunk length of the cell")
    ap.add_argument("--slots", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--guides", type=int, nargs="+", default=[1, 3, 6])
    ap.add_argument("--cell", type=int, nargs=2, default=None, help="(internal) run one (B, Q) cell in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_stream_group_adapt_step.json"))
    args = ap.parse_args()
    if args.cell:
        return cell(args, *args.cell)
    rows = []
    for chunk, B, Q in ((c, b, q) for c in args.chunks for b in args.slots for q in args.guides):
        cmd = [sys.executable, os.path.abspath(__file__), "--cell", str(B), str(Q), "--iters", str(args.iters), "--warmup", str(args.warmup), "--hidden",
               str(args.hidden), "--frames", str(args.frames), "--chunk", str(chunk)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=CELL_SECONDS)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"chunk={chunk} B={B} Q={Q}: no result within {CELL_SECONDS} s; nothing further is started")
        line = next((ln for ln in out.stdout.splitlines() if ln.startswith("ROW ")), None)
        if out.returncode != 0 or line is None:
            raise SystemExit(f"chunk={chunk} B={B} Q={Q}: exit status {out.returncode}; nothing further is started\n{out.stderr[-2000:]}")
        rows.append(json.loads(line[4:]))
        print(json.dumps(rows[-1]), flush=True)
    device = rows[0].pop("device") if rows else None
    for r in rows[1:]:
        r.pop("device", None)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/clip_stream_group_adapt_bench.py", device=device, iters=args.iters, warmup=args.warmup,
                       timing="medians of HIP-event intervals: around one push of the group resp. the B pushes of the B adaptor streams on slices of "
                              "the same stack (every tick of every timed pass), around finish_many resp. the B finish calls; inputs rotate through 2 "
                              "resident stacks; one child process per cell, each under its own time limit",
                       baseline="B ClipStreamAdapt objects (open_stream_adapt) pushed and finished one after the other: the path of the parent commit, untouched",
                       peak="device bytes allocated on top of the resident module and inputs by opening, one tick and a finish, from a module without plans",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
