"""HIComProjector.forward_ragged_multi_guide: B items of unequal length and mixed modality, item i with its own Q_i instructions, through
hicom_compressor_ragged_multiguide_fwd (csrc/ragged_multi_guide.hip).

The product of forward_ragged and forward_multi_guide: a Video-MME evaluation batch (several videos x 3 questions,
hicom/eval/video/inference_video_mcqa_videomme.py:268-303), or multi-question items through hicom_arch.py:146-180.  A *pair* is one (item,
guide).  The stacked [sum T_i, H, W, E] tensor is read in place; every item's tokens are read once by the local stage and once per pass of
32 folded rows by the global stream, in the twelve launches of the ragged step whatever B, the Q_i and the mix are.  Scope rule, input
checks, plan and plan cache are segments.py's; the plain release recipe only.  Plans are keyed by ragged.py's key plus `guide_counts`; a
plan holds the host item descriptors and guide counts, and the head of its workspace holds the device tables.

`plan_tables` / `table_image` restate the table arithmetic of hicom_compressor_ragged_multiguide_prepare in Python: the call takes the
pairs' row counts from it, and the tests hold the device's table region against it."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import native as nv
from . import ragged
from . import segments as seg

MAX_GUIDES = 32          # per item, as in forward_multi_guide
PASS_ROWS = 32           # folded rows one workgroup of the stream carries (two row groups of 16)
STORE = "_ragged_multi_guide_plans"
WHAT = "forward_ragged_multi_guide"


# ------------------------------------------------------------------------------------------------------------------------------------
# table arithmetic (host, no device): mirrors csrc/ragged_multi_guide.hip
# ------------------------------------------------------------------------------------------------------------------------------------
def item_passes(nh: int, q: int) -> int:
    """Passes of the stream over an item's tokens: its nh * q folded rows in passes of 32."""
    return (nh * q + PASS_ROWS - 1) // PASS_ROWS


def item_chunks(ntiles: int, work_sum: int, chunks: int, n_cus: int) -> int:
    """Token chunks per pass of an item of `ntiles` 16-token tiles: its share of 2 * n_cus work units by tiles x passes (work_sum: that
    product summed over the call), rounded to nearest -- or the `chunks` override -- clamped to [1, min(ntiles, 64)].  With one guide per
    item this is ragged.item_chunks."""
    return ragged.item_chunks(ntiles, work_sum, chunks, n_cus)


def plan_tables(items, guide_counts, H: int, W: int, ks: int, nh: int, n_cus: int, chunks: int = 0):
    """items: the fields of hicom_ragged_item per item (ragged.item_descriptors); guide_counts: Q_i.  Returns the per-item offsets, the
    work units (item, first tile, last tile, pass, slot of row group 0), the pair table (item, guide, first context row, first output
    row) and the window -> item / row -> pair lookups, as hicom_compressor_ragged_multiguide_prepare lays them out.  Partial-state
    slots are ordered [item][pass][row group][chunk]."""
    Q = [int(q) for q in guide_counts]
    wps = (H // ks) * (W // ks)
    N = [it[0] * H * W for it in items]
    ntiles = [(n + 15) // 16 for n in N]
    windows = [(it[0] // it[1]) * wps for it in items]
    rows = [w + it[3] + it[6] for w, it in zip(windows, items)]                  # of ONE pair of the item
    passes = [item_passes(nh, q) for q in Q]
    work_sum = sum(t * p for t, p in zip(ntiles, passes))
    nchunks = [item_chunks(t, work_sum, chunks, n_cus) for t in ntiles]

    def prefix(v):
        return [int(x) for x in np.concatenate([[0], np.cumsum(v)[:-1]])] if v else []
    t = SimpleNamespace(N=N, ntiles=ntiles, windows=windows, rows=rows, Q=Q, passes=passes, chunks=nchunks, tok0=prefix(N), win0=prefix(windows),
                        pair0=prefix(Q), ctx_row0=prefix([q * w for q, w in zip(Q, windows)]), row0=prefix([q * r for q, r in zip(Q, rows)]),
                        score_off=prefix([p * PASS_ROWS * x for p, x in zip(passes, ntiles)]),
                        slot0=prefix([2 * p * c for p, c in zip(passes, nchunks)]),
                        global_row0=[w + it[3] for w, it in zip(windows, items)])
    t.units = [(i, nt * c // nc, nt * (c + 1) // nc, p, s0 + 2 * p * nc + c)
               for i, (nt, nc, s0, np_) in enumerate(zip(ntiles, nchunks, t.slot0, passes)) for p in range(np_) for c in range(nc)]
    t.pairs = [(i, q, t.ctx_row0[i] + q * windows[i], t.row0[i] + q * rows[i]) for i in range(len(items)) for q in range(Q[i])]
    t.pair_rows = [rows[i] for i, _, _, _ in t.pairs]
    t.win_item = np.repeat(np.arange(len(items), dtype=np.int32), windows)
    t.row_pair = np.repeat(np.arange(len(t.pairs), dtype=np.int32), t.pair_rows)
    t.slots = sum(2 * p * c for p, c in zip(passes, nchunks))
    t.items = items
    return t


def table_image(t) -> np.ndarray:
    """int32 image of the workspace's table region (each table padded to 256 bytes): item table (16 ints per item), work units (8 ints
    each), window -> item, pair table (4 ints per pair), row -> pair."""
    def pad(a):
        a = np.asarray(a, np.int32).reshape(-1)
        return np.concatenate([a, np.zeros((-a.size) % 64, np.int32)])
    it = [[t.tok0[i], t.N[i], x[0], x[1], t.win0[i], t.slot0[i], t.chunks[i], t.score_off[i], t.pair0[i], t.Q[i], t.ctx_row0[i], t.global_row0[i],
           x[2], x[3], x[4], x[5] if x[5] > 0 else 1] for i, x in enumerate(t.items)]
    units = [list(u) + [0, 0, 0] for u in t.units]
    return np.concatenate([pad(it), pad(units), pad(t.win_item), pad(t.pairs), pad(t.row_pair)])


# ------------------------------------------------------------------------------------------------------------------------------------
def check_inputs(proj, ff, fe, guides, split_sizes, guide_counts, modals, nl):
    """Raises for everything outside the step's scope that does not need the per-item geometry; returns (B, H, W, E, split_sizes,
    guide_counts, modals) with the last three as tuples."""
    if not isinstance(ff, dict) and not isinstance(fe, dict) and seg.seg_recipe(proj) != "plain":
        raise NotImplementedError(f"{WHAT} is built for the plain release recipe only (local + global compressor, use_guide='direct', no "
                                  "adaptors, no clip scale); the adaptor recipe and everything else go through forward() per pair")
    # the items are described as forward_ragged's; the guide rows are counted here, so the shared check sees M = sum Q_i rows
    counted = {}

    def count_pairs():
        nonlocal split_sizes, modals, guide_counts
        try:
            split_sizes = tuple(int(t) for t in split_sizes)
            guide_counts = tuple(int(q) for q in guide_counts)
        except TypeError:
            raise ValueError(f"{WHAT}: split_sizes and guide_counts are sequences of positive ints, one per item") from None
        B = len(split_sizes)
        if B == 0 or any(t <= 0 for t in split_sizes):
            raise ValueError(f"{WHAT}: split_sizes is a sequence of positive ints, one per item (got {split_sizes})")
        if sum(split_sizes) != ff.shape[0]:
            raise ValueError(f"{WHAT}: sum(split_sizes) = {sum(split_sizes)} vs {ff.shape[0]} stacked frames")
        if len(guide_counts) != B:
            raise ValueError(f"{WHAT}: {len(guide_counts)} guide counts for {B} items (one per item)")
        if any(not 1 <= q <= MAX_GUIDES for q in guide_counts):
            raise ValueError(f"{WHAT}: guide_counts {guide_counts}: 1 <= Q_i <= {MAX_GUIDES} guides per item")
        modals = (modals,) * B if isinstance(modals, str) else tuple(modals)
        if len(modals) != B:
            raise ValueError(f"{WHAT}: {len(modals)} modals for {B} items (one string, or one per item)")
        if any(m not in ("image", "video") for m in modals):
            raise ValueError(f"{WHAT}: modals are 'image' or 'video' (got {modals})")
        E = ff.shape[-1]
        if not isinstance(guides, torch.Tensor) or guides.ndim != 2 or guides.shape[1] != E or guides.shape[0] != sum(guide_counts):
            raise ValueError(f"{WHAT}: guide_embeds is [sum Q_i, E] = [{sum(guide_counts)}, {E}], the guides of item i in the rows "
                             f"[sum_(j<i) Q_j, + Q_i) (got {tuple(guides.shape) if isinstance(guides, torch.Tensor) else None})")
        counted["B"] = B
        return sum(guide_counts)
    _, E = seg.check_inputs(WHAT, "ragged multi-guide", proj, ff, fe, guides, nl, 4, "the stacked [sum T_i, H, W, E] tensor", count_pairs)
    for i, (t, m) in enumerate(zip(split_sizes, modals)):
        if m == "image" and t != 1:
            raise ValueError(f"{WHAT}: item {i}: image modality expects a single frame (T = {t})")
    return counted["B"], ff.shape[1], ff.shape[2], E, split_sizes, guide_counts, modals


def exact_tilings(proj, split_sizes, modals, H, W, has_newline):
    """ragged.item_descriptors under this step's name: the fields of hicom_ragged_item per item and the spatial window ks; raises unless
    every item's windows partition its grid exactly, with square spatial windows."""
    items, ks = [], None
    for i, (T, modal) in enumerate(zip(split_sizes, modals)):
        at, ay, ax = seg.exact_tilings(WHAT, proj, T, H, W, modal, f"item {i}: ")
        ks = ay.k
        lay = proj._layout((at.nwin, ay.nwin, ax.nwin), modal, has_newline, False)
        nlr = lay.newline_rows
        items.append((T, at.k, lay.nl_group, len(nlr), nlr[0] if nlr else 0, (nlr[1] - nlr[0]) if len(nlr) > 1 else 1,
                      proj.global_compressor.num_queries))
    return items, ks


def new_args(proj):
    return seg.new_args(proj, nv.CompressorRaggedMultiGuideArgs, None)          # (no adaptor recipe: check_inputs refuses it)


def fill_common(a, proj, split_sizes, H, W, dev, out_dtype, chunks, ptr):
    return seg.fill_common(a, proj, max(split_sizes), H, W, dev, out_dtype, chunks, ptr)


def alloc_workspace(args, a, dev):
    return seg.alloc_workspace(args, a, nv.compressor_ragged_multiguide_workspace, dev)


def _build(proj, H, W, E, split_sizes, guide_counts, modals, nl, out_dtype, chunks, dev, stream):
    desc, ks = exact_tilings(proj, split_sizes, modals, H, W, nl is not None)
    items = (nv.RaggedItem * len(desc))(*[nv.RaggedItem(*d) for d in desc])
    counts = (C.c_int32 * len(guide_counts))(*guide_counts)
    args, a, keep, ptr = new_args(proj)
    a.B, a.E, a.ks, a.items = len(desc), E, ks, items
    a.guide_counts, a.n_guide_counts = counts, len(guide_counts)
    refresh = fill_common(a, proj, split_sizes, H, W, dev, out_dtype, chunks, ptr)
    a.stream = stream
    ws, _ = alloc_workspace(args, a, dev)                       # (the kernels' limits raise here, in front of any launch)
    nv.compressor_ragged_multiguide_prepare(args)               # the device tables, once per plan (synchronises the stream)
    tables = plan_tables(desc, guide_counts, H, W, ks, a.nh, torch.cuda.get_device_properties(dev).multi_processor_count, a.chunks)
    plan = seg.SegPlan(args, ws, tables.pair_rows, a.hidden, (items, counts), tables)
    plan.keep, plan.refresh = keep, refresh
    return plan


def call_inputs(proj, ff, fe, guides, nl):
    return seg.call_inputs(proj, WHAT, ff, fe, guides, nl)


def patch_io(a, ff, fe, guides, nl, out, stream):
    seg.patch_io(a, ff, fe, guides, nl, out, stream)            # (the newline pointer whenever given: items differ in their newline rows)


def cached_plan(proj, key, build):
    return seg.cached_plan(proj, STORE, key, build)


def run_ragged_multi_guide(proj, ff, fe, guides, split_sizes, guide_counts, modals, nl, chunks=None):
    B, H, W, E, split_sizes, guide_counts, modals = check_inputs(proj, ff, fe, guides, split_sizes, guide_counts, modals, nl)
    dev, ff, fe, guides, nl, out_dtype, stream = call_inputs(proj, ff, fe, guides, nl)
    key = (split_sizes, modals, H, W, E, fe is not None, None if nl is None else tuple(nl.shape), out_dtype, stream, int(chunks or 0),
           seg.seg_recipe(proj), proj.local_compressor.adapt_k, proj.local_compressor.adapt_v, guide_counts)
    plan = cached_plan(proj, key, lambda: _build(proj, H, W, E, split_sizes, guide_counts, modals, nl, out_dtype, chunks, dev, stream))
    t = plan.tables
    out = torch.empty((sum(plan.rows), plan.hidden), dtype=out_dtype, device=dev)
    patch_io(plan.io, ff, fe, guides, nl, out, stream)
    nv.compressor_ragged_multiguide_fwd(plan.args)
    # item i: its Q_i pairs' rows follow each other, all of one length -- a [Q_i, rows_i, hidden] view of the one storage
    return [v.view(q, r, plan.hidden) for v, q, r in zip(out.split([q * r for q, r in zip(t.Q, t.rows)]), t.Q, t.rows)]
