"""HIComProjector.forward_ragged: B items of unequal length and mixed modality through hicom_compressor_ragged_fwd (csrc/ragged.hip).

The reference stacks whatever a batch holds -- single images, clips of 4, 8 or 16 frames, the odd 1-frame "video" -- into one
[(b t), H, W, E] tensor, splits it by image_video_split_size and runs its projector once per item (hicom_arch.py:146-180).  Here the
stacked tensor is read in place by ONE C call and the twelve launches of the batched step (fourteen for `local43_adaptkv_global32`),
whatever B and the mix are.  Scope, plan and plan cache are segments.py's, shared with forward_batch.  Plans are keyed by (split_sizes,
modals, grid, ...); a ragged plan also holds the host item descriptors, and the head of its workspace holds the device tables.

Logits form: with `local_logits` = fp32 [sum T_i, H, W] from `siglip_head_scores_ragged` (one guide per item) the local
stage takes its scores from it and reads value rows only (hicom_compressor_ragged_logits_fwd); frames_embed is None, the plan is the one of
the call without frames_embed.

`plan_tables` restates the table arithmetic of hicom_compressor_ragged_prepare in Python: forward_ragged takes the items' row counts
from it, and the tests hold the device's table region against it."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import native as nv
from . import segments as seg

MAX_CHUNKS = 64          # work units per item (csrc/segment_host.hpp: kSegMaxChunks)


# ------------------------------------------------------------------------------------------------------------------------------------
# table arithmetic (host, no device): mirrors csrc/ragged.hip
# ------------------------------------------------------------------------------------------------------------------------------------
def item_chunks(ntiles: int, ntiles_sum: int, chunks: int, n_cus: int) -> int:
    """Work units of an item of `ntiles` 16-token tiles: its share of 2 * n_cus by tile count, rounded to nearest -- or the `chunks`
    override -- clamped to [1, min(ntiles, 64)]."""
    c = chunks if chunks and chunks > 0 else (2 * n_cus * ntiles + ntiles_sum // 2) // ntiles_sum
    return max(1, min(c, ntiles, MAX_CHUNKS))


def prefix(v):
    """Exclusive prefix sums of a list of ints."""
    return [int(x) for x in np.concatenate([[0], np.cumsum(v)[:-1]])] if v else []


def item_geometry(items, H: int, W: int, ks: int):
    """What the item descriptors and the grid alone decide, per item: tokens N, 16-token tiles, windows, packed rows (of one guide),
    the rows in front of the global rows, the first token and the first window in the stack."""
    wps = (H // ks) * (W // ks)
    N = [it[0] * H * W for it in items]
    windows = [(it[0] // it[1]) * wps for it in items]
    return SimpleNamespace(N=N, ntiles=[(n + 15) // 16 for n in N], windows=windows, rows=[w + it[3] + it[6] for w, it in zip(windows, items)],
                           global_row0=[w + it[3] for w, it in zip(windows, items)], tok0=prefix(N), win0=prefix(windows), items=items)


def plan_tables(items, H: int, W: int, ks: int, n_cus: int, chunks: int = 0):
    """items: sequences (T, kt, nl_group, nl_count, nl_first, nl_step, n_global_rows), the fields of hicom_ragged_item.
    Returns the per-item offsets (tokens, windows, rows, logits, partial-state slots), the work units (item, first tile, last tile,
    slot) and the window -> item / row -> item lookups, as hicom_compressor_ragged_prepare lays them out."""
    t = item_geometry(items, H, W, ks)
    t.chunks = [item_chunks(n, sum(t.ntiles), chunks, n_cus) for n in t.ntiles]
    t.row0, t.score_off, t.slot0 = prefix(t.rows), prefix([16 * x for x in t.ntiles]), prefix(t.chunks)
    t.units = [(i, nt * c // nc, nt * (c + 1) // nc, s0 + c) for i, (nt, nc, s0) in enumerate(zip(t.ntiles, t.chunks, t.slot0)) for c in range(nc)]
    t.win_item = np.repeat(np.arange(len(items), dtype=np.int32), t.windows)
    t.row_item = np.repeat(np.arange(len(items), dtype=np.int32), t.rows)
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
def check_splits(what, ff, split_sizes, modals, guide_counts=None, check_counts=None):
    """Raises unless split_sizes are positive ints that add up to the stacked frames and modals name a modality per item (one string
    stands for all).  guide_counts (forward_ragged_multi_guide) are converted with the sizes and handed to check_counts(B, guide_counts)
    between the two.  Returns (split_sizes, modals, guide_counts) as tuples."""
    try:
        split_sizes = tuple(int(t) for t in split_sizes)
        if guide_counts is not None:
            guide_counts = tuple(int(q) for q in guide_counts)
    except TypeError:
        seqs = "split_sizes is a sequence" if guide_counts is None else "split_sizes and guide_counts are sequences"
        raise ValueError(f"{what}: {seqs} of positive ints, one per item") from None
    B = len(split_sizes)
    if B == 0 or any(t <= 0 for t in split_sizes):
        raise ValueError(f"{what}: split_sizes is a sequence of positive ints, one per item (got {split_sizes})")
    if sum(split_sizes) != ff.shape[0]:
        raise ValueError(f"{what}: sum(split_sizes) = {sum(split_sizes)} vs {ff.shape[0]} stacked frames")
    if check_counts is not None:
        check_counts(B, guide_counts)
    modals = (modals,) * B if isinstance(modals, str) else tuple(modals)
    if len(modals) != B:
        raise ValueError(f"{what}: {len(modals)} modals for {B} items (one string, or one per item)")
    if any(m not in ("image", "video") for m in modals):
        raise ValueError(f"{what}: modals are 'image' or 'video' (got {modals})")
    return split_sizes, modals, guide_counts


def train_row_maps(t):
    """Where the rows of the packed output come from, for the backward of the call (ragged_train.py), from plan_tables' result alone:
    (local, newline, glob) int64 arrays of output rows -- local[w] the row of window w of the concatenated window list (the packing's
    row map: a newline gap after every nl_group local tokens), newline the newline rows of all items, glob [B, n_global_rows] the copies
    of each item's global token."""
    local, newline, glob = [], [], []
    for i, it in enumerate(t.items):
        _, _, nl_group, nl_count, nl_first, nl_step, n_global = it
        m = np.arange(t.windows[i], dtype=np.int64)
        local.append(t.row0[i] + m + (m // nl_group if nl_group else 0))
        newline.append(t.row0[i] + nl_first + np.arange(nl_count, dtype=np.int64) * (nl_step if nl_step > 0 else 1))
        glob.append(t.row0[i] + t.global_row0[i] + np.arange(n_global, dtype=np.int64))
    return np.concatenate(local), np.concatenate(newline), np.stack(glob)


DX_TILE = 64             # tokens per workgroup of ragged_global_dx_kernel (csrc/ragged_train.hip)


def dx_tile_table(t) -> np.ndarray:
    """The tile -> item table of hicom_compressor_ragged_global_dx from plan_tables' result alone: int32 [sum ceil(N_i / 64), 2] rows
    (item, first token of the tile inside the item).  Tiles are counted from each item's first token, so no tile spans two items; an
    item's last tile ends at the item's end (the kernel masks it there)."""
    return np.array([(i, n0) for i, N in enumerate(t.N) for n0 in range(0, N, DX_TILE)], dtype=np.int32).reshape(-1, 2)


def token_item_window(t, H: int, W: int, ks: int):
    """(item, window) int64 arrays over all sum N_i stacked tokens, found as ragged_adapt_dy_kernel (csrc/ragged_train.hip) finds them, from
    plan_tables' result alone: the item is the last one whose first token is <= the token (a search of tok0, no table of token size), the
    window WindowGeom::window_of on the item's own (T, kt) axes plus the item's first window."""
    tok = np.arange(sum(t.N), dtype=np.int64)
    tok0, win0 = np.asarray(t.tok0, np.int64), np.asarray(t.win0, np.int64)
    item = np.searchsorted(tok0, tok, side="right") - 1
    kt = np.asarray([it[1] for it in t.items], np.int64)[item]
    loc = tok - tok0[item]
    frame, rem = loc // (H * W), loc % (H * W)
    win = ((frame // kt) * (H // ks) + (rem // W) // ks) * (W // ks) + (rem % W) // ks
    return item, win0[item] + win


def _scope(proj, ff, fe, guides, split_sizes, modals, nl, what="forward_ragged"):
    """Raises for everything outside the ragged step's scope that does not need the per-item geometry; returns (B, H, W, E,
    split_sizes, modals) with the last two as tuples."""
    def count_items():
        nonlocal split_sizes, modals
        split_sizes, modals, _ = check_splits(what, ff, split_sizes, modals)
        return len(split_sizes)
    B, E = seg.check_inputs(what, "ragged", proj, ff, fe, guides, nl, 4, "the stacked [sum T_i, H, W, E] tensor", count_items)
    for i, (t, m) in enumerate(zip(split_sizes, modals)):
        if m == "image" and t != 1:
            raise ValueError(f"{what}: item {i}: image modality expects a single frame (T = {t})")
    return B, ff.shape[1], ff.shape[2], E, split_sizes, modals


def item_descriptors(proj, split_sizes, modals, H, W, has_newline, what="forward_ragged"):
    """The fields of hicom_ragged_item per item, (T, kt, nl_group, nl_count, nl_first, nl_step, n_global_rows), and the spatial
    window ks: LocalCompressor.tilings and HIComProjector._layout on every item alone.  Raises, under the name `what`, unless every
    item's windows partition its grid exactly, with square spatial windows."""
    items, ks = [], None
    for i, (T, modal) in enumerate(zip(split_sizes, modals)):
        at, ay, ax = seg.exact_tilings(what, proj, T, H, W, modal, f"item {i}: ")
        ks = ay.k
        lay = proj._layout((at.nwin, ay.nwin, ax.nwin), modal, has_newline, False)
        nlr = lay.newline_rows
        items.append((T, at.k, lay.nl_group, len(nlr), nlr[0] if nlr else 0, (nlr[1] - nlr[0]) if len(nlr) > 1 else 1,
                      proj.global_compressor.num_queries))
    return items, ks


def _build(proj, H, W, E, split_sizes, modals, nl, out_dtype, chunks, dev, stream):
    desc, ks = item_descriptors(proj, split_sizes, modals, H, W, nl is not None)
    items = (nv.RaggedItem * len(desc))(*[nv.RaggedItem(*d) for d in desc])
    args, a, keep, ptr = seg.new_args(proj, nv.CompressorRaggedArgs, nv.CompressorRaggedAdaptArgs)
    a.B, a.E, a.ks, a.items = len(desc), E, ks, items
    refresh = seg.fill_common(a, proj, max(split_sizes), H, W, dev, out_dtype, chunks, ptr)
    a.stream = stream
    if args is not a:
        seg.fill_adaptors(args, proj.local_compressor, "forward_ragged", ptr)
    ws, adapt_bytes = seg.alloc_workspace(args, a, nv.compressor_ragged_workspace, dev)
    nv.compressor_ragged_prepare(args)                 # the device tables, once per plan (synchronises the stream)
    tables = plan_tables(desc, H, W, ks, torch.cuda.get_device_properties(dev).multi_processor_count, a.chunks)
    plan = seg.SegPlan(args, ws, tables.rows, a.hidden, items, tables)
    plan.keep, plan.adapt_bytes, plan.refresh = keep, adapt_bytes, refresh
    return plan


NOT_LINEAR = ("local_logits has no form on the k / v adaptor recipe: the keys pass an MLP and a LayerNorm blend in front of the score, so it is "
              "not linear in frames_embed; pass frames_embed")


def check_logits(what, proj, ll, fe, ff):
    """The checks of local_logits behind the scope checks of the keyed call and in front of any device work: frames_embed must be None (the
    rule of forward(..., local_logits=)), the plain recipe, fp32 device [sum T_i, H, W] -- or [1, sum T_i, H, W], what
    siglip_head_scores_ragged returns for one guide per item.  Returns the [sum T_i, H, W] view."""
    from .multi_guide import _require_f32_cuda
    if fe is not None:
        raise ValueError(f"{what}: local_logits replaces frames_embed: pass frames_embed=None")
    if seg.seg_recipe(proj) != "plain":
        raise NotImplementedError(f"{what}: {NOT_LINEAR}")
    want = tuple(ff.shape[:3])
    if not isinstance(ll, torch.Tensor) or tuple(ll.shape) not in (want, (1,) + want):
        raise ValueError(f"{what}: local_logits is [sum T_i, H, W] = [{', '.join(map(str, want))}] (or [1, sum T_i, H, W], as siglip_head_scores_ragged "
                         f"returns it for one guide per item), the raw dot products frames_embed_n . guide of the token's item "
                         f"(got {tuple(ll.shape) if isinstance(ll, torch.Tensor) else None})")
    _require_f32_cuda("local_logits", ll)
    return ll.view(want) if ll.is_contiguous() else ll.reshape(want)


def call_ragged(proj, ff, fe, guides, split_sizes, modals, nl, chunks=None, what="forward_ragged", refuse_grad=True, local_logits=None):
    """The one C call of forward_ragged and of forward_ragged_train (ragged_train.py: refuse_grad False): returns (the [sum rows_i,
    hidden] output, the plan, the contiguous frames_feature and guides the call read).  local_logits (frames_embed None):
    the logits form of the call, on the plan of the call without frames_embed."""
    B, H, W, E, split_sizes, modals = _scope(proj, ff, fe, guides, split_sizes, modals, nl, what)
    if local_logits is not None:
        local_logits = check_logits(what, proj, local_logits, fe, ff)
        if refuse_grad and local_logits.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"{what} builds no autograd graph: local_logits requires grad (compute it under torch.no_grad(), or train through "
                               "forward_ragged_train(local_logits=))")
    dev, ff, fe, guides, nl, out_dtype, stream = seg.call_inputs(proj, what, ff, fe, guides, nl, refuse_grad=refuse_grad)
    key = (split_sizes, modals, H, W, E, fe is not None, None if nl is None else tuple(nl.shape), out_dtype, stream, int(chunks or 0),
           seg.seg_recipe(proj), proj.local_compressor.adapt_k, proj.local_compressor.adapt_v)
    plan = seg.cached_plan(proj, "_ragged_plans", key, lambda: _build(proj, H, W, E, split_sizes, modals, nl, out_dtype, chunks, dev, stream))
    a = plan.io
    out = torch.empty((sum(plan.rows), plan.hidden), dtype=out_dtype, device=dev)
    seg.patch_io(a, ff, fe, guides, nl, out, stream)         # (the newline pointer whenever given: items differ in their newline rows)
    if local_logits is not None:
        nv.compressor_ragged_logits_fwd(plan.io, local_logits.detach().contiguous())
    else:
        nv.compressor_ragged_fwd(plan.args)
    return out, plan, ff, guides


def run_ragged(proj, ff, fe, guides, split_sizes, modals, nl, chunks=None, local_logits=None):
    out, plan, _, _ = call_ragged(proj, ff, fe, guides, split_sizes, modals, nl, chunks, local_logits=local_logits)
    return list(out.split(plan.rows))
