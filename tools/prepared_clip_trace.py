"""Dev tool: the launches of one forward_prepared call on the k / v adaptor recipe, for a kernel-trace run of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/prepared_clip_trace.py [frames] [Q] [calls]

One prepare_clip (three clips), 5 warm-up calls, then `calls` forward_prepared calls rotating through the clips; the per-kernel averages of
the stats file divided by `calls` are the per-launch times (the prepare's GEMMs appear with 3 + their plan's first use)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from batch_bench import D, GRID, recipe_projector            # noqa: E402


def main():
    T, Q, calls = (int(v) for v in (sys.argv[1:4] + ["64", "4", "30"][len(sys.argv) - 1:]))
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(7)
    with torch.no_grad():
        m = recipe_projector("adaptkv", 896, T, dev)
        clips = [m.prepare_clip(*(torch.randn((T, GRID, GRID, D), device=dev, generator=gen).bfloat16() for _ in range(2)), "video") for _ in range(3)]
        g = torch.randn((Q, D), device=dev, generator=gen).bfloat16()
        for i in range(5 + calls):
            m.forward_prepared(clips[i % 3], g)
    torch.cuda.synchronize()
    print(f"T={T} Q={Q}: 3 prepare_clip, {5 + calls} forward_prepared calls")


if __name__ == "__main__":
    main()
