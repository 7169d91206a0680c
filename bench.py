"""Headline benchmark: compressed video-tokens / s of the HICom compressor on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]   (N > 1: launched by torchrun)

A "step" = one DROP-IN forward -- HIComProjector.forward(...) as hicom_arch.py:212 calls it, result complete on the
caller's stream -- of the release configuration (mm_projector_type local43_global32_coarse, use_guide=direct,
spatial_unpad/no_token, hidden 896) over synthetic SigLIP features already resident in HBM: 64 frames x 729 tokens x
1152 bf16 PER GPU (BASELINE.json configs[1]; N GPUs => 64*N frames frame-sharded with one RCCL all-gather, configs[2],
weak scaling).  The inputs rotate through 3 distinct buffer sets (645 MB per GPU: HBM, not Infinity Cache).
`python bench.py --gpus N` with N > 1 starts its own N ranks (or run it under torch.distributed.run).

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps and prints the headline
(`ms_per_step` = one timed step).  --dump-outputs DIR writes the compressed tokens of the last timed step as
DIR/compressed_tokens.npy (float32; same arguments -> same inputs).  --full adds everything else, among it:
  roofline     dominant kernel (the fused local+global stream): ALGORITHMIC bytes / its mean launch
               time (HIP events on its own stream, measured here) against the 8 TB/s HBM3E peak
  cpu_baseline the CPU oracle (a port of the reference's PyTorch path) timed on this host's
               cores on the same 64-frame workload (bounded number of repetitions)
  ms_per_step_* spreads and other loop forms, parity, secondary recipes, neighbours, mfma_util, sharded_step.parity
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import hicom_amd                                      # noqa: E402
from hicom_amd import native as nv                    # noqa: E402
from hicom_amd.dist import sharded_forward            # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.3 TB/s measured copy)
D, GRID = 1152, 27


def release_config(hidden: int, frames: int):
    from types import SimpleNamespace
    return SimpleNamespace(mm_projector_type="local43_global32_coarse", use_guide="direct", use_clip_scale="",
                           mm_patch_merge_type="spatial_unpad", mm_newline_position="no_token",
                           mm_vision_tower="google/siglip-so400m-patch14-384", mm_hidden_size=D,
                           hidden_size=hidden, max_num_frames=max(frames, 32))


def make_projector(cfg, device):
    """Random-init weights of the reference's architecture/init law (query ~ N(0,.02) so the branch
    is numerically live), bf16."""
    torch.manual_seed(20250614)
    m = hicom_amd.build_vision_projector(cfg)
    with torch.no_grad():
        m.global_compressor.query.normal_(0, 0.02)
        for name, p in m.named_parameters():
            if p.ndim == 1 and p.numel() > 1:
                p.normal_(0, 0.02)
            elif name.endswith("_alpha"):
                p.fill_(0.5)                         # the reference initialises the blends at 0: numerically dead branches
    return m.to(torch.bfloat16).to(device).eval()


def cpu_baseline(cfg, module, frames: int, budget_s: float = 45.0):
    """SURVEY.md §8(d) "CPU baseline": the CPU oracle (a port of the reference's PyTorch path) on this host's cores -- fp32 AND bf16 (the
    reference's inference dtype), the benchmark shape (`frames` x 729 x 1152) AND BASELINE configs[0] (4 frames), thread count = a MEASURED
    best of {64, 128, all cores} (the sweep is in the line), >= 3 repetitions per leg, min reported.  `value` = the fastest leg on
    the benchmark shape.  Bounded: ~20-30 s of CPU work."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle import hicom_oracle as orc
    host_cores = os.cpu_count() or 1
    t_begin = time.perf_counter()
    sd = {"fp32": {k: v.detach().float().cpu() for k, v in module.state_dict().items()},
          "bf16": {k: v.detach().to(torch.bfloat16).cpu() for k, v in module.state_dict().items()}}
    inputs = {}

    def data(T, dt):
        if T not in inputs:
            g = torch.Generator().manual_seed(1)
            inputs[T] = (torch.randn(T, GRID, GRID, D, generator=g).bfloat16(), torch.randn(T, GRID, GRID, D, generator=g).bfloat16(),
                         torch.randn(D, generator=g).bfloat16())
        ff, fe, gd = inputs[T]
        return (ff.float(), fe.float(), gd.float()) if dt == "fp32" else (ff, fe, gd)

    def leg(T, dt, threads, reps=3):
        torch.set_num_threads(threads)
        ff, fe, gd = data(T, dt)
        c = release_config(cfg.hidden_size, T)
        times = []
        with torch.no_grad():
            out = orc.projector_forward(c, sd[dt], ff, fe, gd, "video", None)      # untimed: the reference builds its pos_embed buffer at construction
            for _ in range(reps):
                t0 = time.perf_counter()
                out = orc.projector_forward(c, sd[dt], ff, fe, gd, "video", None)
                times.append(time.perf_counter() - t0)
                if time.perf_counter() - t_begin > budget_s and len(times) >= 1:
                    break
        n_out = T // 4 * 81 + 32
        assert out.shape[0] == n_out
        return {"frames": T, "dtype": dt, "threads": threads, "ms": round(min(times) * 1e3, 2), "tokens_per_s": round(n_out / min(times), 1),
                "reps": len(times)}

    cands = sorted({c for c in (64, 128, host_cores) if c <= host_cores} or {host_cores})
    # the thread sweep, on the benchmark shape in fp32, in ascending order; it stops at the first count that is SLOWER than the one
    # before it (on the 256-CPU hosts of this pool: 64 -> 0.68 s, 128 -> 1.1 s, 256 -> 13.7 s per forward: oversubscribed OpenMP
    # teams; the last leg alone would be a minute of the run) and says so in the line
    sweep, skipped = [], []
    for c in cands:
        if len(sweep) >= 2 and sweep[-1]["ms"] > sweep[-2]["ms"]:
            skipped.append(c)
            continue
        sweep.append(leg(frames, "fp32", c, reps=2 if sweep else 3))
    best = max(sweep, key=lambda r: r["tokens_per_s"])
    legs = [best if best["reps"] >= 3 else leg(frames, "fp32", best["threads"]), leg(frames, "bf16", best["threads"]),
            leg(4, "fp32", best["threads"]), leg(4, "bf16", best["threads"])]
    head = max(legs[:2], key=lambda r: r["tokens_per_s"])
    return {"value": head["tokens_per_s"], "unit": "tokens/s", "cores": head["threads"], "threads": head["threads"],
            "host_cpu_count": host_cores, "kind": "port", "dtype": head["dtype"],
            "thread_sweep_fp32": [{"threads": r["threads"], "ms": r["ms"]} for r in sweep] +
                                 [{"threads": c, "skipped": "the count before it was already slower than its predecessor"} for c in skipped],
            "legs": legs,
            "sample": f"oracle/hicom_oracle.py on torch-CPU, full {frames}x729x1152 workload and the 4-frame BASELINE configs[0] shape, fp32 and bf16, "
                      f">= 3 forwards per leg (min reported), thread count = best of {cands} measured on the fp32 benchmark shape; "
                      f"{time.perf_counter() - t_begin:.1f} s of CPU work; value = the faster dtype on the benchmark shape"}


def parity_probe(device):
    """max-abs of the HIP path vs the CPU oracle on the reference's CPU-runnable case (configs[0])."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import cases
    from gpu_util import run_native
    from oracle_util import run_oracle
    case = cases.build_case("G11_c1_shape")
    got = run_native(case)["out"].float().cpu()
    want = run_oracle(case)["out"]
    return {"max_abs": float((got - want).abs().max()), "tolerance": 1e-3,
            "workload": "4x729x1152, H=896, direct (BASELINE configs[0]) vs fp32 CPU oracle"}


# Pre-warm-up of a fresh process (reported in the JSON line as `pre_warmup`): untimed windows of EXACTLY the shape of the timed
# region -- [fence | 20 steps | fence] -- until three consecutive windows agree within 2 % (and at least PREWARM_MIN_S have
# passed: clocks, lazily loaded code objects, allocator), capped at PREWARM_CAP_S.  Round 4 ran a fixed 300 steps (25 ms of
# GPU time) and the driver's 20-step region then read 96.8 us against a 82.0-us median of the same process.
PREWARM_WINDOW, PREWARM_TOL, PREWARM_MIN_S, PREWARM_CAP_S = 20, 0.02, 0.30, 2.0
N_INPUT_SETS = 3      # distinct (frames_feature, frames_embed, guide) sets rotated through the timed loop: 3 x 215 MB per
                      # GPU do not fit the 256 MiB Infinity Cache, so every step reads its inputs from HBM


def dist_parity(module, shard_inputs, sharded_out, total_frames, world, device):
    """N > 1 (and the forced world-1 branch): the frame-sharded step against the PLAIN forward of the whole clip on this rank -- every rank's
    shard of the first input set gathered with torch.distributed, one un-sharded call, max-abs difference of the two results.  The reference
    never shards a video; this is what says the sharded step computes the same tokens.  Never fatal: a failure is reported in the line."""
    try:
        import torch.distributed as dist
        ff, fe, g = shard_inputs
        full = []
        for t in (ff, fe):
            buf = torch.empty((world * t.shape[0], *t.shape[1:]), dtype=t.dtype, device=device)
            dist.all_gather_into_tensor(buf, t.contiguous())
            full.append(buf)
        want = module(full[0], full[1], g, "video", None)
        torch.cuda.synchronize()
        d = float((want.float() - sharded_out.float()).abs().max())
        t = torch.tensor([d], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        del full, want
        torch.cuda.empty_cache()
        return {"max_abs_vs_unsharded_forward": float(t.item()), "frames": int(total_frames), "ok": bool(t.item() <= 2e-2),
                "note": "same guide on every rank (the step's first input set); tolerance 2e-2 = the tests' path tolerance for bf16 rows"}
    except Exception as e:                                     # noqa: BLE001
        return {"skipped": f"{type(e).__name__}: {e}"}


def spawn_ranks(args, child_cmd=None, n_devices=None, timeout_s: float = 1500.0) -> int:
    """`python bench.py --gpus N` (N > 1) without a launcher: start N fresh child processes, one per GPU, BEFORE this
    process has touched the GPU (a process that has initialised HIP must not be re-exec'ed; device_count() does not
    initialise it).  Rank 0's JSON line is relayed; any failing child fails the run.
    child_cmd / n_devices / timeout_s: test hooks (tests/test_bench_spawn.py drives the relay and failure paths with a stub child)."""
    import socket
    import subprocess
    n = args.gpus
    have = torch.cuda.device_count() if n_devices is None else n_devices
    if have < n:
        print(f"bench.py: --gpus {n} needs {n} visible devices, this machine has {have}", file=sys.stderr)
        return 3
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = child_cmd if child_cmd is not None else [sys.executable, os.path.abspath(__file__), *sys.argv[1:]]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE if r == 0 else 2, stderr=2))   # (fd 2: the real stderr)
    rc = 0
    out0 = b""
    try:
        out0, _ = procs[0].communicate(timeout=timeout_s)
        for p in procs:
            code = p.wait(timeout=min(300.0, timeout_s))
            rc = rc or code
    except subprocess.TimeoutExpired:
        rc = 4
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()                                   # (exact PIDs of our own children)
                p.wait()
    lines = [ln for ln in out0.decode(errors="replace").splitlines() if ln.startswith("{")]
    if rc == 0 and lines:
        print(lines[-1])
        return 0
    print(f"bench.py: multi-GPU run failed (rc={rc}, {len(lines)} result lines)", file=sys.stderr)
    return rc or 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--frames-per-gpu", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline (spreads, roofline, parity, secondary recipes, CPU baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's output as DIR/compressed_tokens.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true", help="(--full) skip the use_guide=None sweep")
    ap.add_argument("--no-extras", action="store_true", help="(--full) only the timed loop and the roofline (profiling runs)")
    ap.add_argument("--graph", action="store_true", help="hipGraph replay of the cached plan (measured slower than the C launch loop on ROCm 7.2)")
    ap.add_argument("--no-graph", action="store_true", help="(default) eager launches: one C call per step")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    # HICOM_BENCH_FORCE_DIST=1: take the frame-sharded code path at world size 1 (one-GPU check of the N > 1 branch)
    distributed = world > 1 or os.environ.get("HICOM_BENCH_FORCE_DIST") == "1"
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    real_stdout = None
    if distributed:
        import torch.distributed as dist
        # RCCL prints a version banner to the C-level stdout (flushed at exit, i.e. AFTER the JSON line): keep fd 1
        # for the one JSON line and send everything else to stderr
        sys.stdout.flush()
        real_stdout = os.dup(1)
        os.dup2(2, 1)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            import socket
            s = socket.socket()
            s.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(s.getsockname()[1])
            s.close()
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("nccl", device_id=device)      # "nccl" is RCCL on ROCm
        if dist.get_world_size() != world:
            raise SystemExit(f"bench.py: RCCL reports world size {dist.get_world_size()}, launcher said {world}")

    fpg = args.frames_per_gpu
    total_frames = fpg * world
    cfg = release_config(args.hidden, total_frames)
    module = make_projector(cfg, device)
    module.graph_replay = args.graph and not args.no_graph and not distributed
    gen = torch.Generator(device=device).manual_seed(1234 + rank)
    sets = []
    for i in range(N_INPUT_SETS):
        ff = torch.randn(fpg, GRID, GRID, D, device=device, generator=gen).to(torch.bfloat16)
        fe = torch.randn(fpg, GRID, GRID, D, device=device, generator=gen).to(torch.bfloat16)
        guide = torch.randn(D, device=device, generator=torch.Generator(device=device).manual_seed(7 + i)).to(torch.bfloat16)
        sets.append((ff, fe, guide))
    ff, fe, guide = sets[0]
    n_out = total_frames // 4 * 81 + 32
    counter = [0]

    def step():
        """ONE drop-in call, as the reference issues it (hicom_arch.py:212): the result is complete on the caller's
        stream when the call returns.  Inputs rotate through N_INPUT_SETS distinct buffer sets."""
        a, b, g = sets[counter[0] % N_INPUT_SETS]
        counter[0] += 1
        if distributed:
            return sharded_forward(module, a, b, g, total_frames)
        return module(a, b, g, "video", None)

    def step_pipelined():
        """Serving-loop form (not the reference's API): the latency-bound tail of step i (global chain / token exchange)
        overlaps the streaming of step i + 1; fence() waits for every stream."""
        a, b, g = sets[counter[0] % N_INPUT_SETS]
        counter[0] += 1
        if distributed:
            return sharded_forward(module, a, b, g, total_frames, deferred=True)[0]
        return module.forward_deferred(a, b, g, "video", None)[0]

    def fence():
        torch.cuda.synchronize()
        if distributed:
            dist.barrier()
            torch.cuda.synchronize()

    host_marks = []

    def timed(fn, n, marks=None):
        """EXACTLY n steps between two fences (barrier + torch.cuda.synchronize()); marks: host time after each enqueue."""
        fence()
        t0 = time.perf_counter()
        if marks is None:
            for _ in range(n):
                o = fn()
        else:
            for _ in range(n):
                o = fn()
                marks.append(time.perf_counter())
        fence()
        t1 = time.perf_counter()
        if marks is not None:
            marks.insert(0, t0)
            marks.append(t1)
        return (t1 - t0) / n * 1e3, o

    import gc
    with torch.no_grad():
        gc.collect()                       # the collector pass takes tens of ms: BEFORE the warm-up, so that the GPU does not sit idle
        gc.disable()                       # (and drop its clocks) between the warm-up and the timed region; no collector pause inside it
        # N = 1: the drop-in call, joined.  N > 1: there is no reference call to be a drop-in for (the reference never
        # shards a video); the metric is a throughput, so the timed loop is the steady-state serving loop of the frame-
        # sharded path -- sharded_forward(deferred=True), the token exchange of step i under the streaming of step i + 1,
        # same rotating inputs, fence() waits for every stream of every rank -- and the joined latency is reported beside it
        headline = step_pipelined if distributed else step
        dist_guard = None
        if distributed:
            # The sharded step enqueues RCCL's all-gather itself (hicom_amd/dist.py: the process group's own communicator).  First call under a
            # guard every rank agrees on: if that path fails on ANY rank, all of them fall back to torch.distributed's all-gather between two C
            # calls (HICOM_SHARD_DIRECT_AG=0) -- a slower line, not a lost one.
            ok = 1
            try:
                out = step()
                torch.cuda.synchronize()
            except Exception as e:                             # noqa: BLE001
                ok = 0
                print(f"bench.py: rank {rank}: direct all-gather path failed ({type(e).__name__}: {e}); falling back to torch.distributed", file=sys.stderr)
            flag = torch.tensor([ok], device=device)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            dist_guard = {"direct_all_gather": bool(flag.item())}
            if not flag.item():
                os.environ["HICOM_SHARD_DIRECT_AG"] = "0"
                for pl in module.__dict__.pop("_shard_plans", {}).values():
                    pl.release()
        out = step()
        assert out.shape == (n_out, args.hidden)
        if distributed and args.full:
            dist_guard["parity"] = dist_parity(module, sets[0], sharded_forward(module, *sets[0], total_frames), total_frames, world, device)
        # ---- pre-warm-up: convergence rule (PREWARM_* above); every rank follows rank 0's decision ----
        t_pw = time.perf_counter()
        windows = []
        while True:
            windows.append(timed(headline, PREWARM_WINDOW)[0] * 1e3)
            el = time.perf_counter() - t_pw
            last = windows[-3:]
            stop = el >= PREWARM_CAP_S or (el >= PREWARM_MIN_S and len(last) == 3 and (max(last) - min(last)) <= PREWARM_TOL * min(last))
            if distributed:
                flag = torch.tensor([int(stop)], device=device)
                dist.broadcast(flag, 0)
                stop = bool(flag.item())
            if stop:
                break
        pre_warmup = {"rule": f"untimed [fence | {PREWARM_WINDOW} steps | fence] windows until 3 consecutive agree within {PREWARM_TOL:.0%} "
                              f"(at least {PREWARM_MIN_S} s, at most {PREWARM_CAP_S} s)",
                      "windows": len(windows), "steps": len(windows) * PREWARM_WINDOW, "seconds": round(time.perf_counter() - t_pw, 3),
                      "converged": len(windows) >= 3 and (max(windows[-3:]) - min(windows[-3:])) <= PREWARM_TOL * min(windows[-3:]),
                      "first_window_us": round(windows[0], 2), "last_windows_us": [round(w, 2) for w in windows[-3:]]}
        # the rotation restarts at set 0 here, whatever number of pre-warm-up windows ran (at most two more untimed steps reach the
        # boundary, so no set is read twice in a row): the last timed step always reads input set (W + K - 1) mod N_INPUT_SETS, and
        # runs with the same arguments compute the same outputs (--dump-outputs)
        while counter[0] % N_INPUT_SETS:
            headline()
        counter[0] = 0
        for _ in range(args.warmup):       # the W warm-up steps run right in front of the timed region
            out = headline()
        ms_per_step, out = timed(headline, args.steps, host_marks)
        gc.enable()
    if args.dump_outputs and rank == 0:
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "compressed_tokens.npy"), out.float().cpu().numpy())
    if distributed:
        t = torch.tensor([ms_per_step], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ms_per_step = float(t.item())
    # host side of the timed region (rank 0): a stall of the enqueueing thread at the start of a 20-step region is not hidden
    # behind queued GPU work and shows in the headline; the line carries what the host did
    hd = [(host_marks[i + 1] - host_marks[i]) * 1e6 for i in range(len(host_marks) - 1)]
    timed_region_host = {"enqueue_us_mean": round(sum(hd[:-1]) / max(1, len(hd) - 1), 2), "enqueue_us_max": round(max(hd[:-1]), 2),
                         "enqueue_us_first": round(hd[0], 2), "final_fence_us": round(hd[-1], 2)}

    extras = {}
    if args.full and distributed and args.no_extras:
        # the joined latency of the sharded call belongs to every N > 1 line (the headline there is the pipelined loop)
        with torch.no_grad():
            jb = sorted(timed(step, max(5, min(args.steps, 50)))[0] for _ in range(3))
        t = torch.tensor([jb[1]], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        extras["ms_per_step_joined"] = {"median": float(t.item()), "min": jb[0], "api": "sharded_forward(...) with the result joined on the caller's stream"}
    if args.full and not args.no_extras:
        with torch.no_grad():
            gc.disable()
            # spread of the same loop: median over internal batches (the GPU boxes are shared machines)
            nb, per = 7, max(50, min(args.steps, 200))
            batches = sorted(timed(headline, per)[0] for _ in range(nb))
            if distributed:
                jb = sorted(timed(step, per)[0] for _ in range(3))
                extras["ms_per_step_joined"] = {"median": jb[1], "min": jb[0], "api": "sharded_forward(...) with the result joined on the caller's stream"}
            extras["ms_per_step_batches"] = {"median": batches[nb // 2], "min": batches[0], "max": batches[-1], "n": nb,
                                             "steps_per_batch": per}
            if not distributed:             # (both forms on every line, N = 1 included: a scaling curve must compare like with like)
                extras["ms_per_step_joined"] = {"median": batches[nb // 2], "min": batches[0], "api": "HIComProjector.forward(...): the drop-in call (= the headline loop)"}
            # pipelined serving loop (tail of step i under the streaming of step i + 1), same rotating inputs
            for _ in range(20):
                step_pipelined()
            pb = sorted(timed(step_pipelined, per)[0] for _ in range(5))
            extras["ms_per_step_pipelined"] = {"median": pb[2], "min": pb[0], "api": "forward_deferred / sharded_forward(deferred=True)"}
            if not distributed:
                # ONE resident input set: the 215 MB may be served from the Infinity Cache (what round 1 reported)
                def same():
                    return module(ff, fe, guide, "video", None)
                sb = sorted(timed(same, per)[0] for _ in range(5))
                extras["ms_per_step_same_buffers"] = {"median": sb[2], "min": sb[0]}
                # plan miss: every call rebuilds its argument block and workspace (new shape / changed weights)
                def miss():
                    module._invalidate_plans()
                    return step()
                mb = sorted(timed(miss, 20)[0] for _ in range(3))
                extras["ms_per_step_plan_miss"] = {"median": mb[1], "min": mb[0]}
            gc.enable()
        if distributed:
            for k in ("ms_per_step_batches", "ms_per_step_pipelined", "ms_per_step_joined"):
                t = torch.tensor([extras[k]["median"]], device=device, dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                extras[k]["median"] = float(t.item())

    # ---- roofline of the dominant kernel (HIP events on the stream it is launched on) ----------
    roofline = dominant_kernel_roofline(module, sets, args.steps) if args.full else None

    # in-launch hand-offs (query prep granules, the GEMV chain under readout GEMM 2 / in the FINISH phase) whose bounded spin expired
    # during everything above: such a step returns NaN rows and only counts it -- the line carries the counters
    handoff = {"query_prep": 0, "gemv_chain": 0, "checked_workspaces": 0}
    blocks = [p.args for p in module.__dict__.get("_engine_plans", {}).values()]
    for sp in module.__dict__.get("_shard_plans", {}).values():
        blocks += [b for st in sp.sets for b in (st.a_stream, st.a_finish)]
    for blk in blocks:
        qp, ch = nv.compressor_handoff_failures(blk)
        handoff["query_prep"] += qp
        handoff["gemv_chain"] += ch
        handoff["checked_workspaces"] += 1
    assert handoff["query_prep"] == 0 and handoff["gemv_chain"] == 0, f"failed in-launch hand-offs during the bench: {handoff}"

    alg_step = 3359232 * fpg + 18046976 * (args.hidden == 896) + n_out * args.hidden * 2 + 2304
    result = {
        "metric": "compressed_video_tokens_per_sec", "value": n_out / (ms_per_step * 1e-3), "unit": "tokens/s",
        "n_gpus": world, "world_size": (dist.get_world_size() if distributed else 1), "collective_backend": ("rccl (torch.distributed 'nccl')" if distributed else None),
        "steps": args.steps, "warmup": args.warmup, "pre_warmup": pre_warmup, "timed_region_host": timed_region_host, "ms_per_step": ms_per_step,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "config": {"workload": f"{total_frames} frames x 729 SigLIP tokens x 1152 bf16 ({fpg}/GPU), local43+global32, "
                               f"use_guide=direct, hidden {args.hidden} -> {n_out} compressed tokens",
                   "frames": total_frames, "frames_per_gpu": fpg, "hidden": args.hidden,
                   "parallelism": f"frame-shard x{world}" + (" + RCCL all-gather" if distributed else ""),
                   "call": ("sharded_forward(..., deferred=True): steady-state serving loop (exchange of step i under the streaming of "
                            "step i+1); joined latency in ms_per_step_joined" if distributed else
                            "HIComProjector.forward(...): joined drop-in call per step") +
                           f", {N_INPUT_SETS} rotating input sets (HBM-resident, not cache-resident)",
                   "launch": "hipGraph replay" if module.graph_replay else "eager (one C call per step)"},
        "input_visual_tokens_per_sec": total_frames * GRID * GRID / (ms_per_step * 1e-3),
        "whole_step_hbm_frac": (alg_step / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS) if args.hidden == 896 else None,
        **extras,
        **({"sharded_step": dist_guard} if dist_guard is not None else {}),
        "handoff_failures": handoff,
        **({"roofline": roofline} if roofline is not None else {}),
    }
    if args.hidden == 896 and "ms_per_step_batches" in extras:
        result["whole_step_hbm_frac_median"] = alg_step / (extras["ms_per_step_batches"]["median"] * 1e-3) / 1e9 / HBM_PEAK_GBS
    mu = mfma_util_from_profiles() if args.full else None
    if mu is not None:
        result["mfma_util"] = mu
    if rank == 0:
        if world == 1 and args.full and not args.no_extras:
            result["parity"] = parity_probe(device)
            if not distributed and not args.no_secondary:
                result["secondary"] = secondary_sweep(args, device, ff, fe, guide)
                result["neighbours"] = neighbours_sweep(args, device)
            if not args.no_cpu_baseline:
                result["cpu_baseline"] = cpu_baseline(cfg, module, fpg)
                result["speedup_vs_cpu_baseline"] = result["value"] / result["cpu_baseline"]["value"]
        line = json.dumps(result)
        if real_stdout is None:
            print(line)
        else:
            os.write(real_stdout, (line + "\n").encode())
    if distributed:
        dist.destroy_process_group()


def neighbours_sweep(args, device):
    """SURVEY.md §8 rows f2 / f3 next to the path: the SigLIP head projection that produces frames_embed (matrix-core bound,
    925 GFLOP at 64 frames), BASELINE configs[3]'s compressor + splice segment (32 frames, Qwen2.5-7B width 3584) and the whole
    configs[3] pipeline on randomly initialised HF models (c4_first_token)."""
    from hicom_amd.encoder import siglip_head_embed
    from hicom_amd.splice import prepare_inputs_labels_for_multimodal
    out = {}
    gen = torch.Generator(device=device).manual_seed(99)

    def best(fn, n=10, reps=3):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                r = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / n)
        return min(ts), r

    with torch.no_grad():
        # f2: head projection over 64 x 729 tokens, so400m head dimensions (HF config values: 1152 -> 4304 -> 1152, tanh GELU)
        inter = 4304
        head = torch.nn.Module()
        head.layernorm = torch.nn.LayerNorm(D, eps=1e-6)
        head.mlp = torch.nn.Module()
        head.mlp.fc1, head.mlp.fc2 = torch.nn.Linear(D, inter), torch.nn.Linear(inter, D)
        head = head.to(torch.bfloat16).to(device)
        x = torch.randn(args.frames_per_gpu, GRID * GRID, D, device=device, generator=gen).to(torch.bfloat16)
        siglip_head_embed(x, head)
        dt, _ = best(lambda: siglip_head_embed(x, head), n=5)
        flops = 4.0 * x.shape[0] * x.shape[1] * D * inter
        out["siglip_head_projection"] = {"ms": dt * 1e3, "tflops": flops / dt / 1e12, "frac_of_dense_fp16_peak": flops / dt / 2.5e15,
                                         "workload": f"{x.shape[0]}x729 tokens, LayerNorm + 1152->4304->1152 MLP + residual (encoder.py:284-286)",
                                         "kernels": "ln_stream + 2 x dense16_gemm (fp16 operands, fp32 accumulate)"}
        # the known-good reference on this hardware for the two GEMM shapes (cdna_hip_programming.md §5.4 rule 10): the vendor
        # library through torch.mm, plain epilogue (no bias / GELU / residual / fp16 repack), same operand dtype
        def vendor(M, N, K):
            a = (torch.randn(M, K, device=device, generator=gen) * 0.5).to(torch.float16)
            w = (torch.randn(N, K, device=device, generator=gen) * 0.03).to(torch.float16)
            torch.mm(a, w.t())
            dtv, _ = best(lambda: torch.mm(a, w.t()), n=5)
            return 2.0 * M * N * K / dtv / 1e12
        ntok = x.shape[0] * x.shape[1]
        out["siglip_head_projection"]["vendor_gemm_reference_tflops"] = {
            "fc1_shape_plain": vendor(ntok, 4352, D), "fc2_shape_plain": vendor(ntok, D, 4352),
            "note": "torch.mm (hipBLASLt / rocBLAS) on the same shapes with NO epilogue: what the shapes (K = 1152, N = 1152) allow on this chip"}
        # stage 3 of the reference's script trains the head (train.py:717-720): forward under autograd + backward of the projection
        head.train()
        for p_ in head.parameters():
            p_.requires_grad_(True)
        cot_h = torch.randn(x.shape, device=device, generator=gen).to(torch.bfloat16)

        def head_train_step():
            for p_ in head.parameters():
                p_.grad = None
            with torch.enable_grad():
                siglip_head_embed(x, head).backward(cot_h)

        head_train_step()
        dt_h, _ = best(head_train_step, n=3)
        out["siglip_head_projection"]["train_step_ms"] = dt_h * 1e3
        for p_ in head.parameters():
            p_.requires_grad_(False)
            p_.grad = None
        head.eval()
        # f2 completed: head projection + compressor as ONE segment at the benchmark shape.  two_tensor: the head writes
        # frames_embed (bf16) and the compressor streams both visual tensors; logits: the fc2 launch dots its rows with the guide
        # (siglip_head_scores) and the compressor streams frames_feature only.
        from hicom_amd.encoder import siglip_head_scores
        T = args.frames_per_gpu
        mc = make_projector(release_config(args.hidden, T), device)
        hs = x.view(T, GRID, GRID, D)
        gv = torch.randn(D, device=device, generator=gen).to(torch.bfloat16)

        def two_tensor():
            return mc(hs, siglip_head_embed(hs, head), gv, "video", None)

        def with_logits():
            return mc(hs, None, gv, "video", None, local_logits=siglip_head_scores(hs, head, gv))

        for f in (two_tensor, with_logits):
            for _ in range(3):
                f()
        dt2, o2 = best(two_tensor, n=5)
        dtl, ol = best(with_logits, n=5)
        ll = siglip_head_scores(hs, head, gv)
        dt_cl, _ = best(lambda: mc(hs, None, gv, "video", None, local_logits=ll), n=20)
        ntok = T * GRID * GRID
        tensor_b = ntok * D * 2
        out["head_plus_compressor"] = {
            "workload": f"{T} frames: head.layernorm + head.mlp + residual (encoder.py:284-286) -> HIComProjector.forward (release recipe, hidden {args.hidden})",
            "two_tensor_ms": dt2 * 1e3, "logits_ms": dtl * 1e3, "compressor_alone_with_logits_ms": dt_cl * 1e3,
            # algorithmic HBM bytes of the segment behind the hidden layer: fc2 residual read, frames_embed write + re-read,
            # frames_feature read (two_tensor) | fc2 residual read, 18 x 4-byte partials per token + 4-byte logit, frames_feature read
            "bytes_two_tensor": 4 * tensor_b, "bytes_logits": 2 * tensor_b + ntok * (18 * 4 * 2 + 4 * 2),
            "max_abs_diff_between_paths": float((o2.float() - ol.float()).abs().max()),
            "note": "frames_embed enters the direct-mode compressor only through guide . frames_embed_n (projector.py:542-551): "
                    "the logits path never writes it"}
        # C4 segment: compressor at T = 32 / hidden 3584, then the splice into a 2048-token prompt
        cfg = release_config(3584, 32)
        m = make_projector(cfg, device)
        ff = torch.randn(32, GRID, GRID, D, device=device, generator=gen).to(torch.bfloat16)
        fe = torch.randn(32, GRID, GRID, D, device=device, generator=gen).to(torch.bfloat16)
        g = torch.randn(D, device=device, generator=gen).to(torch.bfloat16)
        emb = torch.nn.Embedding(8192, 3584).to(torch.bfloat16).to(device)
        ids = torch.randint(0, 8192, (1, 2048), device=device, generator=gen)
        ids[0, 30] = -201
        mask = torch.ones_like(ids, dtype=torch.bool)
        for _ in range(5):
            m(ff, fe, g, "video", None)
        dt_c, tok = best(lambda: m(ff, fe, g, "video", None), n=20)
        dt_s, res = best(lambda: prepare_inputs_labels_for_multimodal(emb, ids, mask, None, None, [tok]), n=10)
        out["c4_compressor_plus_splice"] = {"compressor_ms": dt_c * 1e3, "splice_ms": dt_s * 1e3, "compressed_tokens": int(tok.shape[0]),
                                            "embeds_shape": list(res[3].shape),
                                            "note": "32 frames, hidden 3584 (Qwen2.5-7B width); SigLIP tower and LLM prefill not included (no weights offline)"}
    out["c4_first_token"] = c4_first_token(device)
    # f4: one training step of the projector at the benchmark shape (forward with a graph + backward), release recipe:
    # projector parameters only (stages 1-2 of the reference's script) and with d frames_embed / d guide_embed (stage 3)
    cfg = release_config(args.hidden, args.frames_per_gpu)
    m = make_projector(cfg, device).train()
    ff = torch.randn(args.frames_per_gpu, GRID, GRID, D, device=device, generator=gen).to(torch.bfloat16)
    fe = torch.randn(args.frames_per_gpu, GRID, GRID, D, device=device, generator=gen).to(torch.bfloat16)
    g = torch.randn(D, device=device, generator=gen).to(torch.bfloat16)
    cot = None

    def train_step(inputs_too):
        nonlocal cot
        fe_, g_ = (fe.detach().requires_grad_(True), g.detach().requires_grad_(True)) if inputs_too else (fe, g)
        m.zero_grad(set_to_none=True)                  # as every training loop does (torch's default since 2.0)
        o = m(ff, fe_, g_, "video", None)
        if cot is None:
            cot = torch.randn(o.shape, device=device, generator=gen).to(o.dtype)
        o.backward(cot)
        return o

    # default: the backward of the plain recipes replays a captured hipGraph over static copies of the inputs (hicom_amd/autograd.py);
    # graph_backward = False: every launch from Python (what rounds 2-3 reported as the eager step)
    for flag, key in ((False, "params_only_ms"), (True, "with_input_grads_ms")):
        for _ in range(3):
            train_step(flag)
        dt, _ = best(lambda: train_step(flag), n=5)
        out.setdefault("train_step", {"workload": f"{args.frames_per_gpu} frames, hidden {args.hidden}, use_guide=direct: forward() under autograd + backward (recompute-based, hicom_amd/autograd.py)"})[key] = dt * 1e3
    ents = list(m.__dict__.get("_bwd_graphs", {}).values())
    out["train_step"]["graph_backward_captured"] = bool(ents) and all("graph" in e for e in ents)
    m.graph_backward = False
    train_step(False)
    dt, _ = best(lambda: train_step(False), n=5)
    out["train_step"]["params_only_eager_backward_ms"] = dt * 1e3
    m.graph_backward = None
    return out


def c4_first_token(device):
    """BASELINE configs[3]: end-to-end prefill on one GPU, 32 frames -- the pipeline of the reference's `mm_infer`
    (hicom/__init__.py:40-124 -> hicom_arch.py:146-214, 271-373): SigLIP-so400m vision tower -> per-patch head projection ->
    HICom compressor -> splice into the prompt embeddings -> Qwen2.5-7B prefill -> first token.  No checkpoints exist
    offline: both HF models are built from typed-in configs (architecture constants of google/siglip-so400m-patch14-384 and
    Qwen/Qwen2.5-7B-Instruct) with RANDOM weights, bf16.  The tower body, the guide (text) tower and the LLM run on stock
    PyTorch (they are outside SURVEY.md §8's hot path); head projection, compressor and splice are this repo's HIP kernels."""
    try:
        from transformers import Qwen2Config, Qwen2ForCausalLM, SiglipTextConfig, SiglipTextModel, SiglipVisionConfig, SiglipVisionModel
    except Exception as e:                                   # transformers not importable on this box
        return {"skipped": f"transformers unavailable: {type(e).__name__}: {e}"}
    from hicom_amd.encoder import siglip_head_embed
    from hicom_amd.splice import prepare_inputs_labels_for_multimodal
    T, S = 32, 2048
    try:
        torch.manual_seed(7)
        prev = torch.get_default_dtype()
        torch.set_default_dtype(torch.bfloat16)
        try:
            with torch.device(device):
                vis = SiglipVisionModel(SiglipVisionConfig(hidden_size=D, intermediate_size=4304, num_hidden_layers=27, num_attention_heads=16,
                                                           image_size=384, patch_size=14)).eval()
                txt = SiglipTextModel(SiglipTextConfig(hidden_size=D, intermediate_size=4304, num_hidden_layers=27, num_attention_heads=16,
                                                       vocab_size=32000, max_position_embeddings=64)).eval()
                llm = Qwen2ForCausalLM(Qwen2Config(vocab_size=152064, hidden_size=3584, intermediate_size=18944, num_hidden_layers=28,
                                                   num_attention_heads=28, num_key_value_heads=4, max_position_embeddings=32768,
                                                   rope_theta=1000000.0, rms_norm_eps=1e-6, tie_word_embeddings=False)).eval()
        finally:
            torch.set_default_dtype(prev)
        proj = make_projector(release_config(3584, T), device)
        gen = torch.Generator(device=device).manual_seed(5)
        frames = torch.randn(T, 3, 384, 384, device=device, generator=gen).to(torch.bfloat16)
        guide_ids = torch.randint(0, 32000, (1, 64), device=device, generator=gen)
        ids = torch.randint(0, 152064, (1, S), device=device, generator=gen)
        ids[0, 30] = -201                                    # <video>
        mask = torch.ones_like(ids)
        emb = llm.get_input_embeddings()
        head = vis.vision_model.head if hasattr(vis, "vision_model") else vis.head

        def stage(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, r

        def run():
            ms = {}
            # encoder.py:277-283: the tower's hidden states (select_layer -2) are frames_feature ...
            ms["vision_tower"], o = stage(lambda: vis(pixel_values=frames, output_hidden_states=True))
            ff = o.hidden_states[-2].view(T, GRID, GRID, D)
            # ... and last_hidden_state + head.mlp(head.layernorm(.)) is frames_embed (encoder.py:284-286); the guide is the text
            # tower's pooled output (:279-283)
            ms["head_projection"], fe = stage(lambda: siglip_head_embed(o.last_hidden_state, head).view(T, GRID, GRID, D))
            ms["guide_tower"], g = stage(lambda: txt(input_ids=guide_ids).pooler_output[0].contiguous())
            ms["compressor"], tok = stage(lambda: proj(ff.contiguous(), fe, g, "video", None))
            ms["splice"], sp = stage(lambda: prepare_inputs_labels_for_multimodal(emb, ids, mask, None, None, [tok]))
            ms["llm_prefill"], lo = stage(lambda: llm(inputs_embeds=sp[3], attention_mask=sp[1], use_cache=True).logits[0, -1].argmax())
            ms["total"] = sum(ms.values())
            return ms, int(lo), tuple(sp[3].shape), (o, ff, fe, g, tok)

        def steady(fn, n=10):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3

        with torch.no_grad():
            first = run()                                    # first sight of every shape: plan builds, table builds, lazy code loads
            runs = [run() for _ in range(3)]
            best = min(runs, key=lambda r: r[0]["total"])
            o, ff, fe, g, tok = best[3]
            ffc = ff.contiguous()
            # the three HIP stages back to back (a serving loop: the second video of a shape hits the compressor plan, the same
            # prompt template hits the splice plan): `ms` above is ONE call between two device synchronisations, from idle clocks
            steady_ms = {"head_projection": steady(lambda: siglip_head_embed(o.last_hidden_state, head)),
                         "compressor": steady(lambda: proj(ffc, fe, g, "video", None)),
                         "splice": steady(lambda: prepare_inputs_labels_for_multimodal(emb, ids, mask, None, None, [tok]))}
        hip = ("head_projection", "compressor", "splice")
        return {"ms": {k: round(v, 3) for k, v in best[0].items()}, "first_token_id": best[1], "prompt_embeds_shape": list(best[2]),
                "first_call_ms": {k: round(first[0][k], 3) for k in hip}, "steady_ms": {k: round(v, 3) for k, v in steady_ms.items()},
                "note": "ms: best of 3 single-shot pipelines (each stage between two device synchronisations); first_call_ms: the very first "
                        "call of each HIP stage (plan / table builds); steady_ms: the stage called back to back (plan hits)",
                "workload": f"{T} frames 384x384 -> SigLIP-so400m (27 layers, random init) -> head projection -> HICom compressor (680 tokens) -> "
                            f"splice into a {S}-token prompt -> Qwen2.5-7B (28 layers, random init) prefill, bf16, batch 1",
                "hip_stages": ["head_projection", "compressor", "splice"], "torch_stages": ["vision_tower", "guide_tower", "llm_prefill"]}
    except Exception as e:                                   # never take the headline down with a neighbour
        return {"skipped": f"{type(e).__name__}: {e}"}
    finally:
        torch.cuda.empty_cache()


def mfma_util_from_profiles():
    """MFMA utilisation per kernel from the committed rocprofv3 PMC pass of this workload (profiles/*_mfma_util.json,
    made by tools/pmc_mfma.py: SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE per XCD x CUs x 4 SIMDs))."""
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_mfma_util.json")))
    if not cands:
        return None
    try:
        prof = json.load(open(cands[-1]))
        return {"source": os.path.relpath(cands[-1], ROOT), "definition": prof.get("definition"),
                "kernels": {k: {"mfma_busy_frac": v.get("mfma_busy_frac"), "insts_mfma": v.get("SQ_INSTS_MFMA")}
                            for k, v in prof.get("kernels", {}).items()}}
    except Exception:
        return None


def secondary_sweep(args, device, ff, fe, guide):
    """SURVEY.md §8(d) secondary sweep, same shapes, plain joined forwards: the generic mode (use_guide=None: 32 distinct learnable
    queries x 9 heads = 288 folded rows, where the global QK^T / PV contraction is dense MFMA work) and the §8 f1 recipes (k / v
    adaptors, coarse and fine injection), with the training step of the recipes the backward covers."""
    def best_of(fn, n=10, reps=3):
        for _ in range(3):
            out = fn()
        dts = []
        for _ in range(reps):                   # best of three batches: a shared box throws the odd 20-ms stall
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                out = fn()
            torch.cuda.synchronize()
            dts.append((time.perf_counter() - t0) / n)
        return min(dts), out

    res = {}
    gen = torch.Generator(device=device).manual_seed(123)
    guide_tokens = torch.randn(64, D, device=device, generator=gen).to(torch.bfloat16)       # "fine": the 64 SigLIP text tokens
    recipes = (("use_guide=None (32 distinct queries)", "local43_global32", None, guide,
                "two-kernel path (local windows || wide global stream kernel)"),
               ("local43_adaptkv_global32 (second released recipe)", "local43_adaptkv_global32", "direct", guide,
                "k / v adaptors over all tokens: 4 dense16 GEMMs + 2 LayerNorm blends in front of the window attention"),
               ("use_guide=coarse", "local43_global32", "coarse", guide, "FiLM injection of the pooled / learnable queries"),
               ("use_guide=fine", "local43_global32", "fine", guide_tokens, "64-token cross-attention injection"))
    for label, ptype, ug, gd, note in recipes:
        cfg = release_config(args.hidden, args.frames_per_gpu)
        cfg.mm_projector_type, cfg.use_guide = ptype, ug
        m = make_projector(cfg, device)
        with torch.no_grad():
            dt, out = best_of(lambda: m(ff, fe, gd, "video", None))
        res[label] = {"ms_per_forward": dt * 1e3, "tokens_per_sec": out.shape[0] / dt, "note": "joined forwards, best of 3 batches of 10; " + note}
        if True:
            # f4: one training step of this recipe (forward under autograd + recompute-based backward, hicom_amd/autograd.py)
            m.train()
            cot = torch.randn(out.shape, device=device, generator=gen).to(out.dtype)

            def train_step():
                m.zero_grad(set_to_none=True)
                o = m(ff, fe, gd, "video", None)
                o.backward(cot)
                return o
            dt_t, _ = best_of(train_step, n=3)
            res[label]["train_step_ms"] = dt_t * 1e3
        del m
    return res


def dominant_kernel_roofline(module, sets, iters):
    """fused_ring_kernel reads both visual tensors (frames_embed + frames_feature) exactly once and
    produces the local contexts and the global partial state: its algorithmic bytes are SURVEY.md
    §8(d)'s 3,359,232 B per frame x frames (+ the fp16 local contexts it writes).  Launched EXACTLY as the release step launches it
    (fp16 window contexts, normalised fp16 partial contexts, the zeroed fixed-point accumulators, value-side pos-emb); the launches
    rotate through the same distinct input sets as the timed loop: the kernel is measured reading HBM, as it runs in the step, not
    re-reading one Infinity-Cache-resident set."""
    ff, fe, guide = sets[0]
    lc, gc = module.local_compressor, module.global_compressor
    T, H, W, _ = ff.shape
    dev = ff.device
    at, ay, ax = lc.tilings(T, H, W, "video")
    nw = at.nwin * ay.nwin * ax.nwin
    R = gc.attn_layer.num_heads
    qhi = (torch.randn(16, D, device=dev) * 0.05).to(torch.bfloat16)
    qlo = (torch.randn(16, D, device=dev) * 1e-4).to(torch.bfloat16)
    qhi[R:] = guide
    qlo[R:] = 0
    pos_a = torch.randn(16, T + H + W, device=dev) * 0.1
    nparts = nv.fused_stream_nparts(nw)
    pe = torch.randn(T + H + W, D, device=dev)
    pe_hi = pe.to(torch.bfloat16)
    pe_lo = (pe - pe_hi.float()).to(torch.bfloat16)
    pm, pl = torch.empty(nparts, 16, device=dev), torch.empty(nparts, 16, device=dev)
    p16 = torch.empty(nparts, 16, D, device=dev, dtype=torch.float16)
    c16 = torch.empty(nw, D, device=dev, dtype=torch.float16)
    zero = torch.zeros(D, dtype=torch.int64, device=dev)
    turn = [0]
    # round 6: with HICOM_RING_MARG=1 the release step takes the value-side pos-emb out of this kernel (its marginals leave it, the merge
    # role applies v_proj . pe^T; opt-in: measured a net loss, executor.hip: marg_out) -- the kernel is then timed in that form
    marg_form = gc.vpe_f16(T, H, W, dev) is not None and os.environ.get("HICOM_RING_MARG", "0") == "1" \
        and os.environ.get("HICOM_TAIL_LAUNCHES", "4") in ("3", "4")
    mg16 = torch.empty(nparts, R, 8 * (D // 64), device=dev, dtype=torch.float16) if marg_form else None

    def launch():
        a, b, _ = sets[turn[0] % len(sets)]
        turn[0] += 1
        nv.fused_stream(a, b, at.k, ay.k, qhi, qlo, R, 1.0 / D ** 0.5, 0.0, pos_a, None if marg_form else pe_hi, None if marg_form else pe_lo,
                        0, T, T + H, pm, pl, None, None, ctx_f16=c16, zero=zero, part_ctx_f16=p16, part_marg=mg16)

    # HIP events on the stream the kernel is launched on (torch's current stream).  The launches are queued
    # back to back in batches, so the host's per-launch cost (ctypes, ~10 us) hides behind the running kernel
    # and a batch's elapsed time / batch size is the kernel's average duration (agrees with rocprofv3 --stats).
    stream = torch.cuda.current_stream()
    batch = 10
    nb = max(10, min(40, iters // batch))
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(nb)]
    # warm-up by the same convergence rule as the step loop: after any idle moment (the allocations above) the chip's power management
    # overshoots for ~15 ms -- ring-only batches read 46 -> 53 -> 45.4 us over thirty batches of ten (tools/ring_bench2.py); batches of
    # ten until five in a row agree within 2 % (at most 300 batches)
    hist = []
    for _ in range(300):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(batch):
            launch()
        b.record(stream)
        b.synchronize()
        hist.append(a.elapsed_time(b))
        # (at least 30 batches = ~14 ms: the overshoot CRESTS around batch 10-15 and five batches on the crest agree within 2 % too --
        # a run that stopped there after 10 batches read 49.2 us where the kernel trace of the same build shows 43.9, round 6)
        if len(hist) >= 30 and max(hist[-5:]) - min(hist[-5:]) <= 0.02 * min(hist[-5:]):
            break
    for a, b in evs:
        a.record(stream)
        for _ in range(batch):
            launch()
        b.record(stream)
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) / batch for a, b in evs)
    mean_ms = sum(ms) / len(ms)
    alg_bytes = 3359232 * T            # bytes per frame x frames of one launch (the 3 MB of fp16 window contexts
    achieved = alg_bytes / (mean_ms * 1e-3) / 1e9   # and 4.5 MB of partial contexts the kernel also WRITES are not counted)
    traffic = traffic_source = None
    try:   # HBM bytes per launch from the newest committed PMC pass of this same workload (profiles/): counters cannot be read from
        # inside an un-profiled run, so the value is REPLAYED from that file (named in `traffic_source`), not measured by this process
        import glob
        src = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_hbm_traffic.json")))[-1]
        prof = json.load(open(src))
        if prof.get("frames") == T:
            traffic = prof["kernels"]["fused_ring_kernel"]["hbm_bytes_per_launch_corrected"]
            traffic_source = os.path.relpath(src, ROOT) + " (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, own passes; replayed, not measured in this run)"
    except Exception:
        pass
    return {"kernel": "hicom::fused_ring_kernel<9, false>", "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS,
            "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
            "algorithmic_bytes_per_launch": alg_bytes, "bytes_per_frame": 3359232, "frames_per_launch": T,
            "mean_launch_ms": mean_ms, "min_launch_ms": ms[0], "median_launch_ms": ms[len(ms) // 2],
            "warmup_batches": len(hist),
            "launch_form": "as in the release step: fp16 window contexts + normalised fp16 partial contexts + " +
                           ("the value-side pos-emb's marginals (applied by the merge role)" if marg_form else "value-side pos-emb in the kernel")}


if __name__ == "__main__":
    main()
