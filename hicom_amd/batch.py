"""HIComProjector.forward_batch: B items of one shape through hicom_compressor_batch_fwd (csrc/batch.hip).

The reference runs its projector once per item of a batch (hicom_arch.py:166-178).  For single images and short clips an item is a
few dozen windows and every forward() is launch latency on an idle chip; here a batch of equal-shaped items is ONE C call and twelve
launches whatever B is.  The two released recipes only -- `local43_global32` and, with the k / v adaptor MLPs as two more launches
over all tokens of the call and the LayerNorm blend fused into the local stage's row loads, `local43_adaptkv_global32` (fourteen
launches); everything else raises NotImplementedError.  The module's recipe alone decides which entry point runs.

Plans (filled argument block + the workspace it owns) are cached on the module by shape, B included, like engine.run_dense's; the
input / output pointers are patched per call."""
from __future__ import annotations

import math

import torch

from . import engine
from . import native as nv

_MAX_PLANS = 16


class _BatchPlan:
    __slots__ = ("args", "io", "ws", "rows", "hidden", "sig", "fresh", "refresh", "hits", "keep", "adapt_bytes")

    def __init__(self, args, ws, rows, hidden, sig):
        # args: the block the entry point takes; io: the plain block inside it (args itself for the plain recipe), whose input / output
        # pointers are patched per call; adapt_bytes: the adaptor regions behind the plain workspace layout (0 for the plain recipe)
        self.args, self.ws, self.rows, self.hidden, self.sig = args, ws, rows, hidden, sig
        self.io = getattr(args, "base", args)
        self.fresh = self.refresh = self.keep = None
        self.hits = self.adapt_bytes = 0


def seg_recipe(proj):
    """The recipe of the batched / ragged step a projector runs: "plain" (local43_global32), "adaptkv" (adapt_k and / or adapt_v on the
    local compressor), or None for everything outside their scope."""
    lc, gc = proj.local_compressor, proj.global_compressor
    if (lc is None or gc is None or lc.use_guide != "direct" or gc.use_guide != "direct" or not lc.queries_native or not gc.is_plain
            or proj.local_use_clip_scale or proj.global_use_clip_scale):
        return None
    return "adaptkv" if (lc.adapt_k or lc.adapt_v) else "plain"


def adaptor_streams(lc):
    """(field of the argument block, MLP, LayerNorm, alpha) per adapted stream of the local compressor."""
    return [s for on, s in ((lc.adapt_k, ("ak", lc.k_proj, lc.k_norm, lc.k_alpha)), (lc.adapt_v, ("av", lc.v_proj, lc.v_norm, lc.v_alpha))) if on]


def fill_adaptors(a, lc, what, ptr):
    """The adaptor descriptors of a Compressor{Batch,Ragged}AdaptArgs block from the local compressor's parameters; `ptr` registers a
    tensor with the plan and returns its address.  The fp16 copy of the second layer's weight is the cached one of
    injector._f16_weight (range-checked when first built, refreshed in place: the plan holds its address)."""
    from . import injector as inj
    from .projector import _linear_params, _require_bf16_cuda
    for field, mlp, norm, alpha in adaptor_streams(lc):
        d = getattr(a, field)
        (w0, b0), (w2, b2) = _linear_params(mlp[0]), _linear_params(mlp[2])
        if w0.shape[0] % 64 or w0.shape[1] % 64 or w2.shape[0] % 64 or w0.shape != w2.shape:
            raise NotImplementedError(f"{what}: adaptor widths must be multiples of 64")
        _require_bf16_cuda("adaptor norm", norm.weight)
        d.w0, d.b0 = ptr(w0), ptr(b0)
        d.w2_f16, d.b2 = ptr(inj._f16_weight(mlp[2])), ptr(b2)
        d.gamma, d.beta, d.alpha = ptr(norm.weight.detach()), ptr(norm.bias.detach()), ptr(alpha.detach())
        a.alpha_dt, a.eps = nv._dt(alpha), norm.eps


def refresh_adaptors(lc):
    """Rebuilds, in place, the cached fp16 weight copies the adaptor descriptors point at (a no-op while the weights have not moved)."""
    from . import injector as inj
    for _, mlp, _, _ in adaptor_streams(lc):
        inj._f16_weight(mlp[2])


def _scope(proj, ff, fe, guides, modal, nl):
    """Raises for everything outside the batched step's scope; returns (B, T, H, W, E, tilings)."""
    from .projector import _require_bf16_cuda
    lc, gc = proj.local_compressor, proj.global_compressor
    if isinstance(ff, dict) or isinstance(fe, dict):
        raise NotImplementedError("forward_batch: anyres dict inputs have no batched path (call forward() per image)")
    if seg_recipe(proj) is None:
        raise NotImplementedError("forward_batch is built for the two release recipes only (local + global compressor, "
                                  "use_guide='direct', no adaptors but adapt_k / adapt_v on the local stage, no clip scale)")
    wdt = lc.readout[0].weight.dtype
    if wdt != torch.bfloat16:
        raise NotImplementedError(f"forward_batch: a {wdt} projector; the batched step takes a bfloat16 module and bfloat16 inputs")
    if not isinstance(ff, torch.Tensor) or ff.ndim != 5:
        raise ValueError("forward_batch: frames_feature is [B, T, H, W, E]")
    _require_bf16_cuda("frames_feature", ff)
    B, T, H, W, E = ff.shape
    if fe is not None:
        _require_bf16_cuda("frames_embed", fe)
        if tuple(fe.shape) != tuple(ff.shape):
            raise ValueError(f"forward_batch: frames_embed {tuple(fe.shape)} vs frames_feature {tuple(ff.shape)}")
    if not isinstance(guides, torch.Tensor) or tuple(guides.shape) != (B, E):
        raise ValueError(f"forward_batch: guide_embeds is [B, E] = [{B}, {E}], one instruction per item "
                         f"(got {None if guides is None else tuple(guides.shape)})")
    _require_bf16_cuda("guide_embeds", guides)
    if nl is not None:
        _require_bf16_cuda("image_newline", nl)
    if modal == "image" and T != 1:
        raise ValueError("forward_batch: image modality expects single-frame items [B, 1, H, W, E]")
    try:
        tiles = lc.tilings(T, H, W, modal)
    except RuntimeError as e:
        raise NotImplementedError(f"forward_batch: the windows must partition the grid exactly ({e})") from None
    if any(a.nwin * a.k != a.n or a.nfull != a.nwin for a in tiles):
        raise NotImplementedError(f"forward_batch: the windows must partition the grid exactly (T={T} H={H} W={W}, windows "
                                  f"{tiles[0].k}x{tiles[1].k}x{tiles[2].k}); such items go through forward()")
    if tiles[1].k != tiles[2].k:
        raise NotImplementedError("forward_batch: square spatial windows only")
    return B, T, H, W, E, tiles


def _build(proj, B, T, H, W, E, tiles, has_fe, modal, nl, out_dtype, chunks, dev):
    from .projector import _linear_params
    lc, gc = proj.local_compressor, proj.global_compressor
    at, ay, ax = tiles
    lay = proj._layout((at.nwin, ay.nwin, ax.nwin), modal, nl is not None, False)
    att = gc.attn_layer
    hidden = lc.readout[2].out_features
    adapt = seg_recipe(proj) == "adaptkv"
    args = nv.CompressorBatchAdaptArgs() if adapt else nv.CompressorBatchArgs()
    a = args.base if adapt else args
    a.B, a.T, a.H, a.W, a.E, a.hidden = B, T, H, W, E, hidden
    a.kt, a.ks, a.nh = at.k, ay.k, att.num_heads
    a.l_scale = 1.0 / math.sqrt(lc.qk_dim)
    a.chunks = int(chunks or 0)
    keep = []

    def ptr(t):
        if t is None:
            return None
        keep.append(t)
        return t.data_ptr()
    w0h, w2h = lc.readout_f16()
    a.lw0_f16, a.lw2_f16 = ptr(w0h), ptr(w2h)
    a.lb0, a.lb2 = ptr(_linear_params(lc.readout[0])[1]), ptr(_linear_params(lc.readout[2])[1])
    for name, lin in (("q", att.q_proj), ("k", att.k_proj), ("v", att.v_proj), ("o", att.out_proj)):
        w, b = _linear_params(lin)
        setattr(a, "w" + name, ptr(w))
        if name != "k":                      # b_k shifts every logit of a row: softmax cancels it
            setattr(a, "b" + name, ptr(b))
    for name, lin in (("0", gc.readout[0]), ("2", gc.readout[2])):
        w, b = _linear_params(lin)
        setattr(a, "gw" + name, ptr(w))
        setattr(a, "gb" + name, ptr(b))
    if gc.use_pos_emb:
        pe, kpe, cap = gc.pos_and_kpe(T, H, W, dev)
        a.pe, a.kpe, a.P = ptr(pe), ptr(kpe), pe.shape[0]
        a.t_index0, a.y_index0, a.x_index0 = 0, cap, cap + H
    a.out_dt = nv.DT_F32 if out_dtype == torch.float32 else nv.DT_BF16
    a.ldo = hidden
    a.global_row0 = lay.n_rows
    a.n_global_rows = gc.num_queries
    a.item_rows = lay.n_rows + gc.num_queries
    a.nl_group = lay.nl_group
    a.nl_count = len(lay.newline_rows)
    if lay.newline_rows:
        a.nl_first = lay.newline_rows[0]
        a.nl_step = lay.newline_rows[1] - lay.newline_rows[0] if len(lay.newline_rows) > 1 else 1
    if adapt:
        fill_adaptors(args, lc, "forward_batch", ptr)
    nbytes = nv.compressor_batch_workspace(args)       # (NotImplementedError for a limit of the kernels, B among them)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    a.ws, a.ws_bytes = ws.data_ptr(), nbytes
    plan = _BatchPlan(args, ws, a.item_rows, hidden, None)
    plan.keep = keep
    plan.adapt_bytes = nbytes - nv.compressor_batch_workspace(a) if adapt else 0

    def refresh():
        lc.readout_f16()
        refresh_adaptors(lc)
        if gc.use_pos_emb:
            gc.pos_and_kpe(T, H, W, dev)
    plan.refresh = refresh
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
    plans = proj.__dict__.setdefault("_batch_plans", {})
    plan = plans.get(key)
    sig = engine.plan_sig(proj)
    if plan is not None and plan.sig == sig:
        fresh = engine.content_sig(proj)
        if plan.fresh != fresh:              # the weights changed in place: rebuild the weight-derived tables into their buffers
            plan.refresh()
            sig = engine.plan_sig(proj)
            plan.fresh = fresh
    if plan is not None and plan.sig != sig:
        plans.pop(key)
        plan = None
    if plan is None:
        plan = _build(proj, B, T, H, W, E, tiles, fe is not None, modal, nl, out_dtype, chunks, dev)
        plan.sig = engine.plan_sig(proj)     # (building may have (re)built the cached positional tables)
        plan.fresh = engine.content_sig(proj)
        if len(plans) >= _MAX_PLANS:
            plans.pop(next(iter(plans)))
        plans[key] = plan
    plan.hits += 1
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
