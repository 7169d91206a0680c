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


def _build(proj, B, T, H, W, E, tiles, modal, nl, out_dtype, chunks, dev):
    gc = proj.global_compressor
    at, ay, ax = tiles
    lay = proj._layout((at.nwin, ay.nwin, ax.nwin), modal, nl is not None, False)
    args, a, keep, ptr = seg.new_args(proj, nv.CompressorBatchArgs, nv.CompressorBatchAdaptArgs)
    a.B, a.T, a.E, a.kt, a.ks = B, T, E, at.k, ay.k
    refresh = seg.fill_common(a, proj, T, H, W, dev, out_dtype, chunks, ptr)
    a.global_row0 = lay.n_rows
    a.n_global_rows = gc.num_queries
    a.item_rows = lay.n_rows + gc.num_queries
    a.nl_group = lay.nl_group
    a.nl_count = len(lay.newline_rows)
    if lay.newline_rows:
        a.nl_first = lay.newline_rows[0]
        a.nl_step = lay.newline_rows[1] - lay.newline_rows[0] if len(lay.newline_rows) > 1 else 1
    if args is not a:
        seg.fill_adaptors(args, proj.local_compressor, "forward_batch", ptr)
    ws, adapt_bytes = seg.alloc_workspace(args, a, nv.compressor_batch_workspace, dev)     # (B is among the kernels' limits)
    plan = seg.SegPlan(args, ws, a.item_rows, a.hidden)
    plan.keep, plan.adapt_bytes, plan.refresh = keep, adapt_bytes, refresh
    return plan


def run_batch(proj, ff, fe, guides, modal, nl, chunks=None):
    from .projector import _out_dtype, _refuse_grad
    B, T, H, W, E, tiles = _scope(proj, ff, fe, guides, modal, nl)
    _refuse_grad(proj, "HIComProjector.forward_batch")
    dev = ff.device
    ff = ff.contiguous()
    fe = fe.contiguous() if fe is not None else None
    guides = guides.contiguous()
    nl = nl.contiguous() if nl is not None else None
    out_dtype = _out_dtype(proj)
    stream = torch.cuda.current_stream(dev).cuda_stream
    key = (B, T, H, W, E, fe is not None, modal, None if nl is None else tuple(nl.shape), out_dtype, stream, int(chunks or 0),
           seg_recipe(proj), proj.local_compressor.adapt_k, proj.local_compressor.adapt_v)
    plan = seg.cached_plan(proj, "_batch_plans", key, lambda: _build(proj, B, T, H, W, E, tiles, modal, nl, out_dtype, chunks, dev))
    a = plan.io
    out = torch.empty((B, plan.rows, plan.hidden), dtype=out_dtype, device=dev)
    a.ff = ff.data_ptr()
    a.fe = fe.data_ptr() if fe is not None else None
    a.guide = guides.data_ptr()
    a.newline = nl.data_ptr() if (nl is not None and a.nl_count > 0) else None
    a.out = out.data_ptr()
    a.stream = stream
    nv.compressor_batch_fwd(plan.args)
    return out
