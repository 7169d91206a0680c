"""HIComProjector.forward_ragged: B items of unequal length and mixed modality through hicom_compressor_ragged_fwd (csrc/ragged.hip).

The reference stacks whatever a batch holds -- single images, clips of 4, 8 or 16 frames, the odd 1-frame "video" -- into one
[(b t), H, W, E] tensor, splits it by image_video_split_size and runs its projector once per item (hicom_arch.py:146-180).  Here the
stacked tensor is read in place by ONE C call and the twelve launches of the batched step (batch.py), whatever B and the mix are.
The two released recipes only, as there: `local43_global32`, and `local43_adaptkv_global32` with the adaptor MLPs as two more launches
over the whole stack (fourteen); everything else raises NotImplementedError.

Plans (filled argument block, the host item descriptors and the workspace, whose head holds the device tables) are cached on the
module by (split_sizes, modals, grid, ...), like batch.py's; the input / output pointers are patched per call.

`plan_tables` restates the table arithmetic of hicom_compressor_ragged_prepare in Python: forward_ragged takes the items' row counts
from it, and the tests hold the device's table region against it."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

from . import engine
from . import native as nv
from .batch import fill_adaptors, refresh_adaptors, seg_recipe

_MAX_PLANS = 16
MAX_CHUNKS = 64          # work units per item (csrc/segment_item.hpp: kSegMaxChunks)


class _RaggedPlan:
    __slots__ = ("args", "io", "items", "ws", "rows", "hidden", "sig", "fresh", "refresh", "hits", "keep", "tables", "adapt_bytes")

    def __init__(self, args, items, ws, rows, hidden):
        # args / io / adapt_bytes: as batch._BatchPlan's
        self.args, self.items, self.ws, self.rows, self.hidden = args, items, ws, rows, hidden
        self.io = getattr(args, "base", args)
        self.sig = self.fresh = self.refresh = self.keep = self.tables = None
        self.hits = self.adapt_bytes = 0


# ------------------------------------------------------------------------------------------------------------------------------------
# table arithmetic (host, no device): mirrors csrc/ragged.hip
# ------------------------------------------------------------------------------------------------------------------------------------
def item_chunks(ntiles: int, ntiles_sum: int, chunks: int, n_cus: int) -> int:
    """Work units of an item of `ntiles` 16-token tiles: its share of 2 * n_cus by tile count, rounded to nearest -- or the `chunks`
    override -- clamped to [1, min(ntiles, 64)]."""
    c = chunks if chunks and chunks > 0 else (2 * n_cus * ntiles + ntiles_sum // 2) // ntiles_sum
    return max(1, min(c, ntiles, MAX_CHUNKS))


def plan_tables(items, H: int, W: int, ks: int, n_cus: int, chunks: int = 0):
    """items: sequences (T, kt, nl_group, nl_count, nl_first, nl_step, n_global_rows), the fields of hicom_ragged_item.
    Returns the per-item offsets (tokens, windows, rows, logits, partial-state slots), the work units (item, first tile, last tile,
    slot) and the window -> item / row -> item lookups, as hicom_compressor_ragged_prepare lays them out."""
    wps = (H // ks) * (W // ks)
    N = [it[0] * H * W for it in items]
    ntiles = [(n + 15) // 16 for n in N]
    windows = [(it[0] // it[1]) * wps for it in items]
    rows = [w + it[3] + it[6] for w, it in zip(windows, items)]
    nchunks = [item_chunks(t, sum(ntiles), chunks, n_cus) for t in ntiles]

    def prefix(v):
        return [int(x) for x in np.concatenate([[0], np.cumsum(v)[:-1]])] if v else []
    t = SimpleNamespace(N=N, ntiles=ntiles, windows=windows, rows=rows, chunks=nchunks, tok0=prefix(N), win0=prefix(windows), row0=prefix(rows),
                        score_off=prefix([16 * x for x in ntiles]), slot0=prefix(nchunks),
                        global_row0=[w + it[3] for w, it in zip(windows, items)])
    t.units = [(i, nt * c // nc, nt * (c + 1) // nc, s0 + c) for i, (nt, nc, s0) in enumerate(zip(ntiles, nchunks, t.slot0)) for c in range(nc)]
    t.win_item = np.repeat(np.arange(len(items), dtype=np.int32), windows)
    t.row_item = np.repeat(np.arange(len(items), dtype=np.int32), rows)
    t.items = items
    return t


def table_image(t) -> np.ndarray:
    """int32 image of the workspace's table region (each table padded to 256 bytes): item table, work units, window -> item,
    row -> item."""
    def pad(a):
        a = np.asarray(a, np.int32).reshape(-1)
        return np.concatenate([a, np.zeros((-a.size) % 64, np.int32)])
    it = [[t.tok0[i], t.N[i], x[0], x[1], t.win0[i], t.slot0[i], t.chunks[i], t.score_off[i], t.row0[i], t.global_row0[i], x[2], x[3], x[4],
           x[5] if x[5] > 0 else 1, 0, 0] for i, x in enumerate(t.items)]
    return np.concatenate([pad(it), pad(t.units), pad(t.win_item), pad(t.row_item)])


# ------------------------------------------------------------------------------------------------------------------------------------
def _scope(proj, ff, fe, guides, split_sizes, modals, nl):
    """Raises for everything outside the ragged step's scope that does not need the per-item geometry; returns (B, H, W, E,
    split_sizes, modals) with the last two as tuples."""
    from .projector import _require_bf16_cuda
    lc, gc = proj.local_compressor, proj.global_compressor
    if isinstance(ff, dict) or isinstance(fe, dict):
        raise NotImplementedError("forward_ragged: anyres dict inputs have no ragged path (call forward() per image)")
    if seg_recipe(proj) is None:
        raise NotImplementedError("forward_ragged is built for the two release recipes only (local + global compressor, "
                                  "use_guide='direct', no adaptors but adapt_k / adapt_v on the local stage, no clip scale)")
    wdt = lc.readout[0].weight.dtype
    if wdt != torch.bfloat16:
        raise NotImplementedError(f"forward_ragged: a {wdt} projector; the ragged step takes a bfloat16 module and bfloat16 inputs")
    if not isinstance(ff, torch.Tensor) or ff.ndim != 4:
        raise ValueError("forward_ragged: frames_feature is the stacked [sum T_i, H, W, E] tensor")
    _require_bf16_cuda("frames_feature", ff)
    Tsum, H, W, E = ff.shape
    if fe is not None:
        _require_bf16_cuda("frames_embed", fe)
        if tuple(fe.shape) != tuple(ff.shape):
            raise ValueError(f"forward_ragged: frames_embed {tuple(fe.shape)} vs frames_feature {tuple(ff.shape)}")
    try:
        split_sizes = tuple(int(t) for t in split_sizes)
    except TypeError:
        raise ValueError("forward_ragged: split_sizes is a sequence of positive ints, one per item") from None
    B = len(split_sizes)
    if B == 0 or any(t <= 0 for t in split_sizes):
        raise ValueError(f"forward_ragged: split_sizes is a sequence of positive ints, one per item (got {split_sizes})")
    if sum(split_sizes) != Tsum:
        raise ValueError(f"forward_ragged: sum(split_sizes) = {sum(split_sizes)} vs {Tsum} stacked frames")
    modals = (modals,) * B if isinstance(modals, str) else tuple(modals)
    if len(modals) != B:
        raise ValueError(f"forward_ragged: {len(modals)} modals for {B} items (one string, or one per item)")
    if any(m not in ("image", "video") for m in modals):
        raise ValueError(f"forward_ragged: modals are 'image' or 'video' (got {modals})")
    if not isinstance(guides, torch.Tensor) or tuple(guides.shape) != (B, E):
        raise ValueError(f"forward_ragged: guide_embeds is [B, E] = [{B}, {E}], one instruction per item "
                         f"(got {None if guides is None else tuple(guides.shape)})")
    _require_bf16_cuda("guide_embeds", guides)
    if nl is not None:
        _require_bf16_cuda("image_newline", nl)
    for i, (t, m) in enumerate(zip(split_sizes, modals)):
        if m == "image" and t != 1:
            raise ValueError(f"forward_ragged: item {i}: image modality expects a single frame (T = {t})")
    return B, H, W, E, split_sizes, modals


def item_descriptors(proj, split_sizes, modals, H, W, has_newline):
    """The fields of hicom_ragged_item per item, (T, kt, nl_group, nl_count, nl_first, nl_step, n_global_rows), and the spatial
    window ks: LocalCompressor.tilings and HIComProjector._layout on every item alone."""
    lc, gc = proj.local_compressor, proj.global_compressor
    items, ks = [], None
    for i, (T, modal) in enumerate(zip(split_sizes, modals)):
        try:
            tiles = lc.tilings(T, H, W, modal)
        except RuntimeError as e:
            raise NotImplementedError(f"forward_ragged: item {i}: the windows must partition the grid exactly ({e})") from None
        if any(a.nwin * a.k != a.n or a.nfull != a.nwin for a in tiles):
            raise NotImplementedError(f"forward_ragged: item {i}: the windows must partition the grid exactly (T={T} H={H} W={W}, windows "
                                      f"{tiles[0].k}x{tiles[1].k}x{tiles[2].k}); such items go through forward()")
        if tiles[1].k != tiles[2].k:
            raise NotImplementedError("forward_ragged: square spatial windows only")
        at, ay, ax = tiles
        ks = ay.k
        lay = proj._layout((at.nwin, ay.nwin, ax.nwin), modal, has_newline, False)
        nlr = lay.newline_rows
        items.append((T, at.k, lay.nl_group, len(nlr), nlr[0] if nlr else 0, (nlr[1] - nlr[0]) if len(nlr) > 1 else 1, gc.num_queries))
    return items, ks


def _build(proj, H, W, E, split_sizes, modals, nl, out_dtype, chunks, dev, stream):
    from .projector import _linear_params
    lc, gc = proj.local_compressor, proj.global_compressor
    desc, ks = item_descriptors(proj, split_sizes, modals, H, W, nl is not None)
    B = len(desc)
    att = gc.attn_layer
    hidden = lc.readout[2].out_features
    items = (nv.RaggedItem * B)(*[nv.RaggedItem(*d) for d in desc])
    adapt = seg_recipe(proj) == "adaptkv"
    args = nv.CompressorRaggedAdaptArgs() if adapt else nv.CompressorRaggedArgs()
    a = args.base if adapt else args
    a.B, a.H, a.W, a.E, a.hidden = B, H, W, E, hidden
    a.ks, a.nh = ks, att.num_heads
    a.l_scale = 1.0 / math.sqrt(lc.qk_dim)
    a.chunks = int(chunks or 0)
    a.items = items
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
    t_max = max(split_sizes)
    if gc.use_pos_emb:
        pe, kpe, cap = gc.pos_and_kpe(t_max, H, W, dev)
        a.pe, a.kpe, a.P = ptr(pe), ptr(kpe), pe.shape[0]
        a.t_index0, a.y_index0, a.x_index0 = 0, cap, cap + H
    a.out_dt = nv.DT_F32 if out_dtype == torch.float32 else nv.DT_BF16
    a.ldo = hidden
    a.stream = stream
    if adapt:
        fill_adaptors(args, lc, "forward_ragged", ptr)
    nbytes = nv.compressor_ragged_workspace(args)      # (NotImplementedError for a limit of the kernels)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    a.ws, a.ws_bytes = ws.data_ptr(), nbytes
    nv.compressor_ragged_prepare(args)                 # the device tables, once per plan (synchronises the stream)
    tables = plan_tables(desc, H, W, ks, torch.cuda.get_device_properties(dev).multi_processor_count, a.chunks)
    plan = _RaggedPlan(args, items, ws, tables.rows, hidden)
    plan.keep, plan.tables = keep, tables
    plan.adapt_bytes = nbytes - nv.compressor_ragged_workspace(a) if adapt else 0

    def refresh():
        lc.readout_f16()
        refresh_adaptors(lc)
        if gc.use_pos_emb:
            gc.pos_and_kpe(t_max, H, W, dev)
    plan.refresh = refresh
    return plan


def run_ragged(proj, ff, fe, guides, split_sizes, modals, nl, chunks=None):
    from .projector import _out_dtype, _refuse_grad
    B, H, W, E, split_sizes, modals = _scope(proj, ff, fe, guides, split_sizes, modals, nl)
    _refuse_grad(proj, "HIComProjector.forward_ragged")
    dev = ff.device
    ff = ff.contiguous()
    fe = fe.contiguous() if fe is not None else None
    guides = guides.contiguous()
    nl = nl.contiguous() if nl is not None else None
    out_dtype = _out_dtype(proj)
    stream = torch.cuda.current_stream(dev).cuda_stream
    key = (split_sizes, modals, H, W, E, fe is not None, None if nl is None else tuple(nl.shape), out_dtype, stream, int(chunks or 0),
           seg_recipe(proj), proj.local_compressor.adapt_k, proj.local_compressor.adapt_v)
    plans = proj.__dict__.setdefault("_ragged_plans", {})
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
        plan = _build(proj, H, W, E, split_sizes, modals, nl, out_dtype, chunks, dev, stream)
        plan.sig = engine.plan_sig(proj)     # (building may have (re)built the cached positional tables)
        plan.fresh = engine.content_sig(proj)
        if len(plans) >= _MAX_PLANS:
            plans.pop(next(iter(plans)))
        plans[key] = plan
    plan.hits += 1
    a = plan.io
    out = torch.empty((sum(plan.rows), plan.hidden), dtype=out_dtype, device=dev)
    a.ff = ff.data_ptr()
    a.fe = fe.data_ptr() if fe is not None else None
    a.guide = guides.data_ptr()
    a.newline = nl.data_ptr() if nl is not None else None
    a.out = out.data_ptr()
    a.stream = stream
    nv.compressor_ragged_fwd(plan.args)
    return list(out.split(plan.rows))
