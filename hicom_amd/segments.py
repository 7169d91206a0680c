"""What HIComProjector.forward_batch (batch.py), forward_ragged (ragged.py) and forward_multi_guide (multi_guide.py) share on the Python
side: the scope rule, the input checks, the plan (filled argument block + the workspace it owns), the fields of the argument block that
come from the module alone, the plan builder of the two steps whose items share one shape, the call prologue and the per-call pointer
patch.  The modules keep what depends on how items are described: one (T, H, W) shape and B or Q, or split sizes, modals and the table
arithmetic.

Plans are cached on the module by shape (`proj._batch_plans`, `proj._ragged_plans`, `proj._multi_guide_plans`: at most MAX_PLANS each)
through engine.cached_plan, the ONE plan-cache protocol of the package: engine.run_dense's plans go through the same function.  The input /
output pointers are patched per call.  forward_ragged_multi_guide (ragged_multi_guide.py: the product of the last two,
`proj._ragged_multi_guide_plans`) is built on the same functions, and so are prepare_clip / forward_prepared (prepared.py:
`proj._prepare_plans`, `proj._prepared_plans`).  No list of the stores is kept by hand: cached_plan records each store's name on the module,
and HIComProjector._invalidate_plans drops what is recorded."""
from __future__ import annotations

import math

import torch

from . import engine
from . import native as nv

cached_plan, MAX_PLANS = engine.cached_plan, engine.MAX_PLANS       # (the steps' modules and the tests reach them here)


class SegPlan:
    __slots__ = ("args", "io", "items", "ws", "rows", "hidden", "sig", "fresh", "refresh", "hits", "keep", "tables", "adapt_bytes", "train")

    def __init__(self, args, ws, rows, hidden, items=None, tables=None):
        # args: the block the entry point takes; io: the plain block inside it (args itself for the plain recipe), whose input / output
        # pointers are patched per call; adapt_bytes: the adaptor regions behind the plain workspace layout (0 for the plain recipe);
        # items / tables: the host item descriptors and the table arithmetic of a ragged plan, None for a batch plan
        self.args, self.ws, self.rows, self.hidden, self.items, self.tables = args, ws, rows, hidden, items, tables
        self.io = getattr(args, "base", args)
        self.sig = self.fresh = self.refresh = self.keep = self.train = None   # (train: what ragged_train.py derives from the plan once, made there)
        self.hits = self.adapt_bytes = 0


def seg_recipe(proj):
    """The recipe of the batched / ragged step a projector runs: "plain" (local43_global32), "adaptkv" (adapt_k and / or adapt_v on the
    local compressor), or None for everything outside their scope."""
    lc, gc = proj.local_compressor, proj.global_compressor
    if (lc is None or gc is None or lc.use_guide != "direct" or gc.use_guide != "direct" or not lc.queries_native or not gc.is_plain
            or proj.local_use_clip_scale or proj.global_use_clip_scale):
        return None
    return "adaptkv" if (lc.adapt_k or lc.adapt_v) else "plain"


def fill_adaptors(a, lc, what, ptr):
    """The adaptor descriptors of a Compressor{Batch,Ragged}AdaptArgs block from the local compressor's parameters; `ptr` registers a
    tensor with the plan and returns its address.  The fp16 copy of the second layer's weight is the cached one of
    injector._f16_weight (range-checked when first built, refreshed in place: the plan holds its address)."""
    from . import injector as inj
    from .projector import _linear_params, _require_bf16_cuda
    for field, mlp, norm, alpha in engine.adaptor_streams(lc):
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
    for _, mlp, _, _ in engine.adaptor_streams(lc):
        inj._f16_weight(mlp[2])


def check_tokens(what, step, proj, ff, fe, ndim, ff_layout):
    """The part of check_inputs that knows no guide: the module's scope and dtype, frames_feature and frames_embed.  Returns E."""
    from .projector import _require_bf16_cuda
    if isinstance(ff, dict) or isinstance(fe, dict):
        raise NotImplementedError(f"{what}: anyres dict inputs have no {step} path (call forward() per image)")
    if seg_recipe(proj) is None:
        raise NotImplementedError(f"{what} is built for the two release recipes only (local + global compressor, "
                                  "use_guide='direct', no adaptors but adapt_k / adapt_v on the local stage, no clip scale)")
    wdt = proj.local_compressor.readout[0].weight.dtype
    if wdt != torch.bfloat16:
        raise NotImplementedError(f"{what}: a {wdt} projector; the {step} step takes a bfloat16 module and bfloat16 inputs")
    if not isinstance(ff, torch.Tensor) or ff.ndim != ndim:
        raise ValueError(f"{what}: frames_feature is {ff_layout}")
    _require_bf16_cuda("frames_feature", ff)
    E = ff.shape[-1]
    if fe is not None:
        _require_bf16_cuda("frames_embed", fe)
        if tuple(fe.shape) != tuple(ff.shape):
            raise ValueError(f"{what}: frames_embed {tuple(fe.shape)} vs frames_feature {tuple(ff.shape)}")
    return E


def check_inputs(what, step, proj, ff, fe, guides, nl, ndim, ff_layout, count_items):
    """The input checks of `what` ("forward_batch" / "forward_ragged", the `step` "batched" / "ragged"): raises for a module or tensors
    outside the step's scope.  frames_feature has `ndim` axes (`ff_layout` says which); count_items() is called once frames_feature and
    frames_embed have passed, checks what describes the items and returns B.  Returns (B, E)."""
    from .projector import _require_bf16_cuda
    E = check_tokens(what, step, proj, ff, fe, ndim, ff_layout)
    B = count_items()
    if not isinstance(guides, torch.Tensor) or tuple(guides.shape) != (B, E):
        raise ValueError(f"{what}: guide_embeds is [B, E] = [{B}, {E}], one instruction per item "
                         f"(got {None if guides is None else tuple(guides.shape)})")
    _require_bf16_cuda("guide_embeds", guides)
    if nl is not None:
        _require_bf16_cuda("image_newline", nl)
    return B, E


def exact_tilings(what, proj, T, H, W, modal, item=""):
    """LocalCompressor.tilings of one item shape; raises unless the windows partition the grid exactly, with square spatial windows."""
    try:
        tiles = proj.local_compressor.tilings(T, H, W, modal)
    except RuntimeError as e:
        raise NotImplementedError(f"{what}: {item}the windows must partition the grid exactly ({e})") from None
    if any(a.nwin * a.k != a.n or a.nfull != a.nwin for a in tiles):
        raise NotImplementedError(f"{what}: {item}the windows must partition the grid exactly (T={T} H={H} W={W}, windows "
                                  f"{tiles[0].k}x{tiles[1].k}x{tiles[2].k}); such items go through forward()")
    if tiles[1].k != tiles[2].k:
        raise NotImplementedError(f"{what}: square spatial windows only")
    return tiles


def new_args(proj, plain, adapt):
    """(the block the entry point takes, the plain block inside it, keep, ptr) for the module's recipe: an instance of `adapt` (plain block
    first) for the adaptor recipe, of `plain` otherwise (adapt None: a step without adaptor recipe).  ptr(t) registers a tensor with the
    plan (`keep`) and returns its address."""
    args = adapt() if adapt is not None and seg_recipe(proj) == "adaptkv" else plain()
    keep = []

    def ptr(t):
        if t is None:
            return None
        keep.append(t)
        return t.data_ptr()
    return args, getattr(args, "base", args), keep, ptr


def fill_common(a, proj, T_for_pos, H, W, dev, out_dtype, chunks, ptr):
    """The fields of a plain argument block that the module alone decides (everything but the items' shapes, their packed-row layout, the
    workspace and the per-call pointers); T_for_pos: the frames the positional tables must cover.  Returns the plan's refresh(): rebuilds,
    in place, the weight-derived tables whose addresses the block holds."""
    from .projector import _linear_params
    lc, gc = proj.local_compressor, proj.global_compressor
    att = gc.attn_layer
    a.H, a.W, a.hidden, a.nh = H, W, lc.readout[2].out_features, att.num_heads
    a.l_scale = 1.0 / math.sqrt(lc.qk_dim)
    a.chunks = int(chunks or 0)
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
        pe, kpe, cap = gc.pos_and_kpe(T_for_pos, H, W, dev)
        a.pe, a.kpe, a.P = ptr(pe), ptr(kpe), pe.shape[0]
        a.t_index0, a.y_index0, a.x_index0 = 0, cap, cap + H
    a.out_dt = nv.DT_F32 if out_dtype == torch.float32 else nv.DT_BF16
    a.ldo = a.hidden

    def refresh():
        lc.readout_f16()
        refresh_adaptors(lc)
        if gc.use_pos_emb:
            gc.pos_and_kpe(T_for_pos, H, W, dev)
    return refresh


def alloc_workspace(args, a, workspace_bytes, dev):
    """Allocates the workspace `workspace_bytes(args)` asks for (NotImplementedError for a limit of the kernels) and enters it into the plain
    block `a`; returns (workspace, bytes of the adaptor regions behind the plain layout)."""
    nbytes = workspace_bytes(args)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    a.ws, a.ws_bytes = ws.data_ptr(), nbytes
    return ws, (nbytes - workspace_bytes(a) if args is not a else 0)


def build_equal_plan(proj, what, plain, adapt, count, shape, tiles, modal, nl, out_dtype, chunks, dev, workspace_bytes):
    """The plan of a step whose items share one shape (T, H, W, E) and so one packed-row layout (HIComProjector._layout): `shape` =
    (items, T, H, W, E), `count` the field of the block that takes the item count ("B" / "Q")."""
    n, T, H, W, E = shape
    at, ay, ax = tiles
    lay = proj._layout((at.nwin, ay.nwin, ax.nwin), modal, nl is not None, False)
    args, a, keep, ptr = new_args(proj, plain, adapt)
    setattr(a, count, n)
    a.T, a.E, a.kt, a.ks = T, E, at.k, ay.k
    refresh = fill_common(a, proj, T, H, W, dev, out_dtype, chunks, ptr)
    a.global_row0 = lay.n_rows
    a.n_global_rows = proj.global_compressor.num_queries
    a.item_rows = lay.n_rows + a.n_global_rows
    a.nl_group = lay.nl_group
    a.nl_count = len(lay.newline_rows)
    if lay.newline_rows:
        a.nl_first = lay.newline_rows[0]
        a.nl_step = lay.newline_rows[1] - lay.newline_rows[0] if len(lay.newline_rows) > 1 else 1
    if args is not a:
        fill_adaptors(args, proj.local_compressor, what, ptr)
    ws, adapt_bytes = alloc_workspace(args, a, workspace_bytes, dev)      # (the kernels' limits raise here, in front of any launch)
    plan = SegPlan(args, ws, a.item_rows, a.hidden)
    plan.keep, plan.adapt_bytes, plan.refresh = keep, adapt_bytes, refresh
    return plan


def call_inputs(proj, what, ff, fe, guides, nl, refuse_grad=True):
    """The prologue of a call behind its scope checks: (device, the four inputs made contiguous, output dtype, stream).  refuse_grad
    False: the caller builds the autograd graph itself (forward_ragged_train) and has told native.py which kind of forward this is."""
    from .projector import _out_dtype, _refuse_grad
    if refuse_grad:
        _refuse_grad(proj, f"HIComProjector.{what}")
    dev = ff.device

    def dense(t):
        return t.contiguous() if t is not None else None
    return dev, ff.contiguous(), dense(fe), guides.contiguous(), dense(nl), _out_dtype(proj), torch.cuda.current_stream(dev).cuda_stream


def patch_io(a, ff, fe, guides, nl, out, stream):
    """The per-call fields of a plan's plain block; nl None: no newline pointer."""
    a.ff = ff.data_ptr()
    a.fe = fe.data_ptr() if fe is not None else None
    a.guide = guides.data_ptr()
    a.newline = nl.data_ptr() if nl is not None else None
    a.out = out.data_ptr()
    a.stream = stream
