"""HIComProjector.forward_batch: B items of one shape through hicom_compressor_batch_fwd (csrc/batch.hip).

The reference runs its projector once per item of a batch (hicom_arch.py:166-178).  For single images and short clips an item is a
few dozen windows and every forward() is launch latency on an idle chip; here a batch of equal-shaped items is ONE C call and twelve
launches whatever B is (fourteen for `local43_adaptkv_global32`).  The module's recipe alone decides which entry point runs; scope,
plan and plan cache are segments.py's, shared with forward_ragged.  Plans are keyed by shape, B included."""
from __future__ import annotations

import torch

from . import native as nv
from . import segments as seg
from .segments import seg_recipe          # noqa: F401  (the scope rule, under the name it had here)


def _scope(proj, ff, fe, guides, modal, nl):
    """Raises for everything outside the batched step's scope; returns (B, T, H, W, E, tilings)."""
    B, E = seg.check_inputs("forward_batch", "batched", proj, ff, fe, guides, nl, 5, "[B, T, H, W, E]", lambda: ff.shape[0])
    _, T, H, W, _ = ff.shape
    if modal == "image" and T != 1:
        raise ValueError("forward_batch: image modality expects single-frame items [B, 1, H, W, E]")
    return B, T, H, W, E, seg.exact_tilings("forward_batch", proj, T, H, W, modal)


def run_batch(proj, ff, fe, guides, modal, nl, chunks=None):
    B, T, H, W, E, tiles = _scope(proj, ff, fe, guides, modal, nl)
    dev, ff, fe, guides, nl, out_dtype, stream = seg.call_inputs(proj, "forward_batch", ff, fe, guides, nl)
    key = (B, T, H, W, E, fe is not None, modal, None if nl is None else tuple(nl.shape), out_dtype, stream, int(chunks or 0),
           seg_recipe(proj), proj.local_compressor.adapt_k, proj.local_compressor.adapt_v)
    plan = seg.cached_plan(proj, "_batch_plans", key, lambda: seg.build_equal_plan(
        proj, "forward_batch", nv.CompressorBatchArgs, nv.CompressorBatchAdaptArgs, "B", (B, T, H, W, E), tiles, modal, nl, out_dtype, chunks, dev,
        nv.compressor_batch_workspace))                                              # (B is among the kernels' limits)
    a = plan.io
    out = torch.empty((B, plan.rows, plan.hidden), dtype=out_dtype, device=dev)
    seg.patch_io(a, ff, fe, guides, nl if a.nl_count > 0 else None, out, stream)
    nv.compressor_batch_fwd(plan.args)
    return out
