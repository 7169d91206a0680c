"""HIComProjector.forward_ragged_multi_guide: B items of unequal length and mixed modality, item i with its own Q_i instructions, through
hicom_compressor_ragged_multiguide_fwd (csrc/ragged_multi_guide.hip).

The product of forward_ragged and forward_multi_guide: a Video-MME evaluation batch (several videos x 3 questions,
hicom/eval/video/inference_video_mcqa_videomme.py:268-303), or multi-question items through hicom_arch.py:146-180.  A *pair* is one (item,
guide).  The stacked [sum T_i, H, W, E] tensor is read in place; every item's tokens are read once by the local stage and once per pass of
32 folded rows by the global stream, in the twelve launches of the ragged step whatever B, the Q_i and the mix are.  Scope rule, input
checks, plan and plan cache are segments.py's; the plain release recipe only.  Plans are keyed by ragged.py's key plus `guide_counts`; a
plan holds the host item descriptors and guide counts, and the head of its workspace holds the device tables.

`plan_tables` / `table_image` restate the table arithmetic of hicom_compressor_ragged_multiguide_prepare in Python: the call takes the
pairs' row counts from it, and the tests hold the device's table region against it.

Logits form: with `local_logits` = fp32 [max Q_i, sum T_i, H, W] from `siglip_head_scores_ragged` the local stage takes
its scores from that tensor and reads the value rows only (hicom_compressor_ragged_multiguide_logits_fwd: the same sequence, workspace and
tables, another launch 3); frames_embed is None.  The two forms do not share a plan: the key carries the form."""
from __future__ import annotations

import ctypes as C

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
    prefix = ragged.prefix
    t = ragged.item_geometry(items, H, W, ks)                   # (t.rows: of ONE pair of the item)
    t.Q = [int(q) for q in guide_counts]
    t.passes = [item_passes(nh, q) for q in t.Q]
    work_sum = sum(n * p for n, p in zip(t.ntiles, t.passes))
    t.chunks = [item_chunks(n, work_sum, chunks, n_cus) for n in t.ntiles]
    t.pair0, t.ctx_row0, t.row0 = prefix(t.Q), prefix([q * w for q, w in zip(t.Q, t.windows)]), prefix([q * r for q, r in zip(t.Q, t.rows)])
    t.score_off = prefix([p * PASS_ROWS * x for p, x in zip(t.passes, t.ntiles)])
    t.slot0 = prefix([2 * p * c for p, c in zip(t.passes, t.chunks)])
    t.units = [(i, nt * c // nc, nt * (c + 1) // nc, p, s0 + 2 * p * nc + c)
               for i, (nt, nc, s0, np_) in enumerate(zip(t.ntiles, t.chunks, t.slot0, t.passes)) for p in range(np_) for c in range(nc)]
    t.pairs = [(i, q, t.ctx_row0[i] + q * t.windows[i], t.row0[i] + q * t.rows[i]) for i in range(len(items)) for q in range(t.Q[i])]
    t.pair_rows = [t.rows[i] for i, _, _, _ in t.pairs]
    t.win_item = np.repeat(np.arange(len(items), dtype=np.int32), t.windows)
    t.row_pair = np.repeat(np.arange(len(t.pairs), dtype=np.int32), t.pair_rows)
    t.slots = sum(2 * p * c for p, c in zip(t.passes, t.chunks))
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

    def check_counts(B, counts):
        if len(counts) != B:
            raise ValueError(f"{WHAT}: {len(counts)} guide counts for {B} items (one per item)")
        if any(not 1 <= q <= MAX_GUIDES for q in counts):
            raise ValueError(f"{WHAT}: guide_counts {counts}: 1 <= Q_i <= {MAX_GUIDES} guides per item")

    def count_pairs():
        nonlocal split_sizes, modals, guide_counts
        split_sizes, modals, guide_counts = ragged.check_splits(WHAT, ff, split_sizes, modals, guide_counts, check_counts)
        E = ff.shape[-1]
        if not isinstance(guides, torch.Tensor) or guides.ndim != 2 or guides.shape[1] != E or guides.shape[0] != sum(guide_counts):
            raise ValueError(f"{WHAT}: guide_embeds is [sum Q_i, E] = [{sum(guide_counts)}, {E}], the guides of item i in the rows "
                             f"[sum_(j<i) Q_j, + Q_i) (got {tuple(guides.shape) if isinstance(guides, torch.Tensor) else None})")
        counted["B"] = len(split_sizes)
        return sum(guide_counts)
    _, E = seg.check_inputs(WHAT, "ragged multi-guide", proj, ff, fe, guides, nl, 4, "the stacked [sum T_i, H, W, E] tensor", count_pairs)
    for i, (t, m) in enumerate(zip(split_sizes, modals)):
        if m == "image" and t != 1:
            raise ValueError(f"{WHAT}: item {i}: image modality expects a single frame (T = {t})")
    return counted["B"], ff.shape[1], ff.shape[2], E, split_sizes, guide_counts, modals


def build_plan(proj, what, H, W, E, split_sizes, guide_counts, modals, nl, out_dtype, chunks, dev, stream, block=nv.CompressorRaggedMultiGuideArgs,
               workspace=nv.compressor_ragged_multiguide_workspace, prepare=nv.compressor_ragged_multiguide_prepare, fill=None):
    """The plan of a step over B items with Q_i guides each: this module's, or forward_prepared_many's (prepared_many.py: `block` holds the
    ragged multi-guide block as `base`; fill(args, ptr) enters what it adds in front of the workspace call).  The item walk, the common
    fields, the workspace, the device tables (once per plan) and their Python restatement are one function for both."""
    desc, ks = ragged.item_descriptors(proj, split_sizes, modals, H, W, nl is not None, what)
    items = (nv.RaggedItem * len(desc))(*[nv.RaggedItem(*d) for d in desc])
    counts = (C.c_int32 * len(guide_counts))(*guide_counts)
    args, a, keep, ptr = seg.new_args(proj, block, block)
    a.B, a.E, a.ks, a.items = len(desc), E, ks, items
    a.guide_counts, a.n_guide_counts = counts, len(guide_counts)
    refresh = seg.fill_common(a, proj, max(split_sizes), H, W, dev, out_dtype, chunks, ptr)
    a.stream = stream
    if fill is not None:
        fill(args, ptr)
    nbytes = workspace(args)                                    # (the kernels' limits raise here, in front of any launch)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    a.ws, a.ws_bytes = ws.data_ptr(), nbytes
    prepare(args)                                               # the device tables, once per plan (synchronises the stream)
    tables = plan_tables(desc, guide_counts, H, W, ks, a.nh, torch.cuda.get_device_properties(dev).multi_processor_count, a.chunks)
    plan = seg.SegPlan(args, ws, tables.pair_rows, a.hidden, (items, counts), tables)
    plan.keep, plan.refresh = keep, refresh
    return plan


def pair_views(plan, out):
    """Item i's Q_i pairs' rows follow each other, all of one length: a [Q_i, rows_i, hidden] view of the one storage per item."""
    t = plan.tables
    return [v.view(q, r, plan.hidden) for v, q, r in zip(out.split([q * r for q, r in zip(t.Q, t.rows)]), t.Q, t.rows)]


def check_logits(ll, fe, ff, guide_counts):
    """The checks of local_logits behind the scope checks of the keyed call and in front of any device work (multi_guide.check_logits for
    the stack): frames_embed must be None, fp32 device [max Q_i, sum T_i, H, W]."""
    from .multi_guide import _require_f32_cuda
    if fe is not None:
        raise ValueError(f"{WHAT}: local_logits replaces frames_embed: pass frames_embed=None")
    want = (max(guide_counts),) + tuple(ff.shape[:3])
    if not isinstance(ll, torch.Tensor) or tuple(ll.shape) != want:
        raise ValueError(f"{WHAT}: local_logits is [max Q_i, sum T_i, H, W] = [{', '.join(map(str, want))}], plane q holding guide q of every item on "
                         f"the item's frames (got {tuple(ll.shape) if isinstance(ll, torch.Tensor) else None})")
    _require_f32_cuda("local_logits", ll)


def plan_key(split_sizes, modals, H, W, E, has_fe, nl, out_dtype, stream, chunks, recipe, adapt_k, adapt_v, guide_counts, logits=False):
    """The key of a plan; the keyed form's is what it was before the logits form (so its plans and their order in the store do not change)."""
    key = (split_sizes, modals, H, W, E, has_fe, None if nl is None else tuple(nl.shape), out_dtype, stream, int(chunks or 0), recipe, adapt_k, adapt_v,
           guide_counts)
    return key + ("logits",) if logits else key


def call_ragged_multi_guide(proj, ff, fe, guides, split_sizes, guide_counts, modals, nl, chunks=None, local_logits=None, refuse_grad=True):
    """The one C call of forward_ragged_multi_guide and of forward_ragged_multi_guide_train (ragged_multi_guide_train.py: refuse_grad
    False): returns (the [sum Q_i rows_i, hidden] output, the plan, the contiguous frames_feature and guides the call read)."""
    B, H, W, E, split_sizes, guide_counts, modals = check_inputs(proj, ff, fe, guides, split_sizes, guide_counts, modals, nl)
    if local_logits is not None:
        check_logits(local_logits, fe, ff, guide_counts)
    grad_kw = {} if refuse_grad else {"refuse_grad": False}     # (the inference call is made as it always was)
    dev, ff, fe, guides, nl, out_dtype, stream = seg.call_inputs(proj, WHAT, ff, fe, guides, nl, **grad_kw)
    key = plan_key(split_sizes, modals, H, W, E, fe is not None, nl, out_dtype, stream, chunks, seg.seg_recipe(proj), proj.local_compressor.adapt_k,
                   proj.local_compressor.adapt_v, guide_counts, local_logits is not None)
    plan = seg.cached_plan(proj, STORE, key, lambda: build_plan(proj, WHAT, H, W, E, split_sizes, guide_counts, modals, nl, out_dtype, chunks, dev,
                                                                stream))       # (no adaptor recipe: check_inputs refuses it)
    out = torch.empty((sum(plan.rows), plan.hidden), dtype=out_dtype, device=dev)
    seg.patch_io(plan.io, ff, fe, guides, nl, out, stream)      # (the newline pointer whenever given: items differ in their newline rows)
    if local_logits is not None:
        ll = local_logits.contiguous()
        nv.compressor_ragged_multiguide_logits_fwd(plan.args, ll.data_ptr(), ff.shape[0] * H * W)
    else:
        nv.compressor_ragged_multiguide_fwd(plan.args)
    return out, plan, ff, guides


def run_ragged_multi_guide(proj, ff, fe, guides, split_sizes, guide_counts, modals, nl, chunks=None, local_logits=None):
    out, plan, _, _ = call_ragged_multi_guide(proj, ff, fe, guides, split_sizes, guide_counts, modals, nl, chunks, local_logits)
    return pair_views(plan, out)


def dx_tile_table(t) -> np.ndarray:
    """The tile -> item table of hicom_compressor_ragged_multiguide_global_dx from plan_tables' result alone: ragged.dx_tile_table -- int32
    [sum ceil(N_i / 64), 2] rows (item, first token of the tile inside the item).  A tile belongs to an ITEM, not to a pair: its workgroup
    adds all nh Q_i rows of the item's row space."""
    return ragged.dx_tile_table(t)


def pair_dq_table(t) -> np.ndarray:
    """The (first row, count) table hicom_compressor_ragged_multiguide_dq_pair sums by, from plan_tables' result alone: int64 [M, 2], pair p's
    rows of the pair-major dq [sum Q_i windows_i, E] (its window contexts' rows)."""
    return np.array([(ctx_row0, t.windows[i]) for i, _, ctx_row0, _ in t.pairs], dtype=np.int64).reshape(-1, 2)


def train_row_maps(t):
    """Where the rows of the pair-major packed output come from, for the backward of the call (ragged_multi_guide_train.py), from
    plan_tables' result alone: (local, newline, glob) int64 arrays of output rows -- local[c] the row of context row c (pair p owns the
    context rows [ctx_row0_p, + windows_i) in window order; the packing's row map: a newline gap after every nl_group local tokens),
    newline the newline rows of all pairs, glob [M, n_global_rows] the copies of each pair's global token.  With one guide per item these
    are ragged.train_row_maps."""
    local, newline, glob = [], [], []
    for i, _, _, row0 in t.pairs:
        _, _, nl_group, nl_count, nl_first, nl_step, n_global = t.items[i]
        m = np.arange(t.windows[i], dtype=np.int64)
        local.append(row0 + m + (m // nl_group if nl_group else 0))
        newline.append(row0 + nl_first + np.arange(nl_count, dtype=np.int64) * (nl_step if nl_step > 0 else 1))
        glob.append(row0 + t.global_row0[i] + np.arange(n_global, dtype=np.int64))
    return np.concatenate(local), np.concatenate(newline), np.stack(glob)
