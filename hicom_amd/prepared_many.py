"""HIComProjector.forward_prepared_many: B prepared clips (prepared.py: prepare_clip), item i with its own Q_i instructions, in one native
call through hicom_compressor_clips_multiguide_fwd (csrc/ragged_multi_guide.hip).

The product of forward_prepared and forward_ragged_multi_guide: a server with B videos in flight, each with a few pending questions.  The
clips were made at different times, so every clip lives at its own addresses, each with its own y planes; nothing is stacked: the two
launches that read tokens (local windows, segmented stream) take an item's base pointers from a [B, 4] device table.  No adaptor MLP
runs, nothing token-sized is allocated or copied.  A plain-recipe module's clips carry no planes and the same call runs the plain window:
forward_ragged_multi_guide over separately allocated tensors, bit for bit.

Scope rule, plan cache and the common fields are segments.py's, the item walk, the plan builder and the table arithmetic
ragged_multi_guide.py's; clips, staleness and the stream protocol prepared.py's.  Plans live in `proj._prepared_many_plans`, keyed by the
mix of shapes, modalities and guide counts -- NOT by the clips' addresses: two calls with the same mix and other clips share a plan.

The pointer table: one int64 [B, 4] device tensor per plan, rows {key_x, value_x, ky, vy}.  The C call only launches, so the table is
filled here, per call, on the call's stream: stream order puts the copy behind the previous call's kernels, which still read the old
rows.  Its source is a fresh pageable CPU tensor and a plain copy_: the copy has consumed the source when copy_ returns (the runtime stages
pageable memory, and may wait for the stream to do so), which a reused pinned buffer would not guarantee.  A call whose rows are those the
table already holds -- the same clips asked again -- writes nothing."""
from __future__ import annotations

import torch

from . import native as nv
from . import prepared
from . import ragged_multi_guide as rmg
from . import segments as seg

STORE = "_prepared_many_plans"
WHAT = "forward_prepared_many"
MAX_GUIDES = rmg.MAX_GUIDES


class ClipsPlan(seg.SegPlan):
    """A ragged multi-guide plan plus the device pointer table and the rows it holds (None: not written yet)."""
    __slots__ = ("ptrs", "held")


def check_clips(proj, clips):
    """Raises for what the clips themselves decide and no device is needed for; returns (clips as a list, H, W, E, has_fe)."""
    try:
        clips = list(clips)
    except TypeError:
        raise ValueError(f"{WHAT}: clips is a sequence of what prepare_clip returned") from None
    if not clips:
        raise ValueError(f"{WHAT}: clips is a non-empty sequence of what prepare_clip returned")
    lc = proj.local_compressor
    recipe = seg.seg_recipe(proj)
    for i, c in enumerate(clips):
        if not isinstance(c, prepared.PreparedClip):
            raise ValueError(f"{WHAT}: clip {i} is not what prepare_clip returned (got {type(c).__name__})")
        if c.proj is not proj:
            raise ValueError(f"{WHAT}: clip {i} was prepared by another module")
    _, H, W, E = clips[0].shape
    has_fe = clips[0].fe is not None
    for i, c in enumerate(clips):
        if c.shape[1:] != (H, W, E):
            raise ValueError(f"{WHAT}: clip {i} is {c.shape[1]} x {c.shape[2]} x {c.shape[3]} (H x W x E), clip 0 {H} x {W} x {E}: one grid and width per call")
        if (c.fe is not None) != has_fe:
            raise ValueError(f"{WHAT}: clip {i} {'has' if c.fe is not None else 'has no'} frames_embed, clip 0 {'has' if has_fe else 'has none'}: "
                             "all clips of a call or none")
        if recipe is not None and ((c.y_k is not None) != (recipe == "adaptkv" and bool(lc.adapt_k))
                                   or (c.y_v is not None) != (recipe == "adaptkv" and bool(lc.adapt_v))):
            raise ValueError(f"{WHAT}: clip {i}: the module's adaptors changed since prepare_clip")
    return clips, H, W, E, has_fe


def check_guides(B, E, guides, guide_counts):
    from .projector import _require_bf16_cuda
    try:
        counts = tuple(int(q) for q in guide_counts)
    except TypeError:
        raise ValueError(f"{WHAT}: guide_counts is a sequence of positive ints, one per clip") from None
    if len(counts) != B:
        raise ValueError(f"{WHAT}: {len(counts)} guide counts for {B} clips (one per clip)")
    if any(not 1 <= q <= MAX_GUIDES for q in counts):
        raise ValueError(f"{WHAT}: guide_counts {counts}: 1 <= Q_i <= {MAX_GUIDES} guides per clip")
    if not isinstance(guides, torch.Tensor) or guides.ndim != 2 or tuple(guides.shape) != (sum(counts), E):
        raise ValueError(f"{WHAT}: guide_embeds is [sum Q_i, E] = [{sum(counts)}, {E}], the guides of clip i in the rows [sum_(j<i) Q_j, + Q_i) "
                         f"(got {tuple(guides.shape) if isinstance(guides, torch.Tensor) else None})")
    _require_bf16_cuda("guide_embeds", guides)
    return counts


def pointer_rows(clips):
    """The table's rows {key_x, value_x, ky, vy} per clip, checked: the host side of the C call cannot look at device-resident addresses."""
    rows = []
    for i, c in enumerate(clips):
        row = ((c.fe if c.fe is not None else c.ff).data_ptr(), c.ff.data_ptr(), 0 if c.y_k is None else c.y_k.data_ptr(),
               0 if c.y_v is None else c.y_v.data_ptr())
        if not row[0] or not row[1] or (c.y_k is not None and not row[2]) or (c.y_v is not None and not row[3]) or any(p % 16 for p in row):
            raise ValueError(f"{WHAT}: clip {i}: tokens and planes are non-NULL and 16-byte aligned")
        rows.append(row)
    return tuple(rows)


def _build(proj, H, W, E, Ts, counts, modals, nl, out_dtype, chunks, dev, stream):
    def fill(args, ptr):
        if seg.seg_recipe(proj) == "adaptkv":
            seg.fill_adaptors(args, proj.local_compressor, WHAT, ptr)
    base = rmg.build_plan(proj, WHAT, H, W, E, Ts, counts, modals, nl, out_dtype, chunks, dev, stream, nv.CompressorClipsMultiGuideArgs,
                          nv.compressor_clips_multiguide_workspace, nv.compressor_clips_multiguide_prepare, fill)
    plan = ClipsPlan(base.args, base.ws, base.rows, base.hidden, base.items, base.tables)
    plan.keep, plan.refresh = base.keep, base.refresh
    plan.ptrs = torch.empty((len(Ts), 4), dtype=torch.int64, device=dev)
    plan.held = None
    plan.args.item_ptrs = plan.ptrs.data_ptr()
    return plan


def run_prepared_many(proj, clips, guides, guide_counts, nl=None, chunks=None):
    from .projector import _require_bf16_cuda
    clips, H, W, E, has_fe = check_clips(proj, clips)
    first = clips[0]
    seg.check_tokens(WHAT, "prepared-many", proj, first.ff, first.fe, 4, "[T, H, W, E]")     # (the module's scope; the tokens passed prepare_clip)
    counts = check_guides(len(clips), E, guides, guide_counts)
    if nl is not None:
        _require_bf16_cuda("image_newline", nl)
    dev, _, _, guides, nl, out_dtype, stream = seg.call_inputs(proj, WHAT, first.ff, None, guides, nl)
    if any(c.ff.device != dev for c in clips):
        raise ValueError(f"{WHAT}: the clips live on one device")
    lc = proj.local_compressor
    state = prepared.adaptor_sig(proj) if seg.seg_recipe(proj) == "adaptkv" else None
    for i, c in enumerate(clips):           # (free while the weight state stands; a moved epoch alone compares the checksums once per clip)
        if state is not None and (c.sig, c.epoch) != state and c.is_stale():
            raise RuntimeError(f"{WHAT}: clip {i} is stale: the adaptor MLP weights moved since prepare_clip (clip.refresh() recomputes its planes)")
    rows = pointer_rows(clips)
    Ts, modals = tuple(c.shape[0] for c in clips), tuple(c.modal for c in clips)
    key = (Ts, modals, counts, H, W, E, has_fe, None if nl is None else tuple(nl.shape), out_dtype, stream, int(chunks or 0),
           seg.seg_recipe(proj), lc.adapt_k, lc.adapt_v)
    plan = seg.cached_plan(proj, STORE, key, lambda: _build(proj, H, W, E, Ts, counts, modals, nl, out_dtype, chunks, dev, stream))
    cur = torch.cuda.current_stream(dev)
    waited = set()
    for c in clips:                          # on the device: no host wait
        if c.event is not None and c.stream != cur and id(c) not in waited:
            waited.add(id(c))
            cur.wait_event(c.event)
            for y in (c.y_k, c.y_v):
                if y is not None:
                    y.record_stream(cur)
    if plan.held != rows:
        plan.held = None                     # (a copy that raises leaves no claim on what the table holds)
        plan.ptrs.copy_(torch.tensor(rows, dtype=torch.int64))
        plan.held = rows
    a = plan.io
    out = torch.empty((sum(plan.rows), plan.hidden), dtype=out_dtype, device=dev)
    a.ff = a.fe = None
    a.guide, a.newline, a.out, a.stream = guides.data_ptr(), (nl.data_ptr() if nl is not None else None), out.data_ptr(), stream
    nv.compressor_clips_multiguide_fwd(plan.args)
    return rmg.pair_views(plan, out)
