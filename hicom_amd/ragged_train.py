"""HIComProjector.forward_ragged_train: the training step of a mixed batch -- forward_ragged's one C call under autograd.

The reference trains on exactly the shape forward_ragged reads (hicom_arch.py:146-180 with mm_tunable_parts="mm_projector",
train.py:709-713): one projector call and one backward per item.  Here the forward is the C call of forward_ragged (same plan cache,
same bits) and the backward is ONE eager pass over all items: the same call sequence, four HIP launches among it, whatever B and the mix are:

  local stage    dY gathered from the cotangent through the packing's row maps (ragged.train_row_maps), the readout backward
                 (autograd._readout_backward) over the sum of all items' windows; d image_newline = the sum of all newline rows.
                 The window backward never runs in this scope (autograd._window_backward_runs is false for it).
  global stage   rows item-major (item nh + head): autograd._global_tail_backward with the B guides as the B queries, then
                 hicom_compressor_ragged_global_bwd (csrc/ragged_train.hip: the segmented backward stream + the dq merge, four launches),
                 then autograd._global_fold_backward and the q_proj gradients.

The autograd node owns what its backward reads (window contexts, logits, softmax state, merged contexts: copied out of the plan's
workspace by hicom_compressor_ragged_train_state), so forward, forward, backward, backward on one plan works.

Input gradients (stage 3 of the reference's script, train.py:712-726; `input_grads=True`): every one of frames_feature,
frames_embed and guide_embeds that requires grad gets its gradient, from two more native calls over all items:

  local stage    hicom_compressor_ragged_local_bwd: the window backward over the concatenated window list (dq per window, d frames_embed,
                 the value-side share of d frames_feature -- with the key-side term where frames_embed is None), and dq summed per item;
  global stage   hicom_compressor_ragged_global_dx: dS^T qt + P^T dctx per item, added into the rows the window backward left.

d guide_embeds[i] = dq_item[i] + row i of (dqp Wq + dpre): the injected query of the direct recipe is the guide, one row per item.  A stage
whose parameters are all frozen runs only where an input gradient needs it (d frames_feature and d guide_embeds: both; d frames_embed: local).

The k / v adaptor recipe `local43_adaptkv_global32` (`adaptors=True`): the forward is forward_ragged's adaptor C call; the
node also keeps the fp16 y planes of the adapted streams (the MLPs' outputs over all sum N_i tokens, the forward's own bits, copied out of
the workspace by hicom_compressor_ragged_adapt_train_state; the hidden planes are recomputed in the backward, one layer-1 GEMM per stream).
The local stage of the backward is then

  window backward  hicom_compressor_ragged_local_adapt_bwd over the concatenated window list (ds, pw per token; the four sums per window);
                   d alpha, d norm.weight, d norm.bias of both adaptors are reductions of those (autograd._adaptor_streams_backward, the
                   single-item code: the query row of a window is its item's guide, gathered through a cached window -> item index);
  adaptor MLPs     autograd._adaptor_mlp_backward over the stacked [sum N_i, E] tokens -- the per-token GEMMs do not care where an item
                   ends, so B chains of small GEMMs are one chain of large ones -- with hicom_compressor_ragged_adapt_dy as its dy step;
  input gradients  d frames_embed = d_kx, d frames_feature = d_vx (+ d_kx without frames_embed) and then the global share as above,
                   d guide's local share = hicom_compressor_ragged_dq_item of dq = (1 - a_k) sxk + a_k gamma_k syk.

The logits form (`local_logits=`; the plain recipe, frames_embed None): the forward is hicom_compressor_ragged_logits_fwd, the
local scores given in the place of frames_embed.  A parameters-only step (stages 1 and 2: the head is frozen) has the backward above with no
further launch.  With input_grads=True the local stage of the backward is ONE launch, hicom_compressor_ragged_local_logits_bwd: d local_logits
(fp32) and the value-side share of d frames_feature; there is no dq, so d guide_embeds is the global share alone -- the local share flows
through the scores into the caller's graph.  The node keeps the scores by reference only where that launch will run.

Frozen adaptors with no input gradient asked for: neither the window call nor the MLP backward runs, and no y plane is kept.

Scope: the two release recipes `local43_global32` and, with adaptors=True, `local43_adaptkv_global32` (use_guide="direct", no other
adaptors, no clip-scale, bf16 module and inputs, exact window partition per item); gradients of every projector parameter that requires
grad and of image_newline.  Everything else raises NotImplementedError naming the loop of forward(): nothing is detached silently."""
from __future__ import annotations

import functools
import types

import torch

from . import autograd as ag
from . import native as nv
from . import ragged
from . import segments as seg

WHAT = "forward_ragged_train"
_LOOP = "run the loop of forward() per item instead"


def check_scope(proj, ff, fe, guides, input_grads=False, adaptors=False, local_logits=None):
    """The refusals of forward_ragged_train that forward_ragged does not make; no device is touched."""
    if isinstance(ff, dict) or isinstance(fe, dict):
        raise NotImplementedError(f"{WHAT}: anyres dict inputs have no ragged training step; {_LOOP}")
    if proj.local_use_clip_scale or proj.global_use_clip_scale:
        raise NotImplementedError(f"{WHAT}: clip-scale is not built for the ragged training step; {_LOOP}")
    recipe = seg.seg_recipe(proj)
    if recipe == "adaptkv" and not adaptors:
        raise NotImplementedError(f"{WHAT}: the k / v adaptor recipe (local43_adaptkv_global32) trains through the ragged training step with "
                                  f"adaptors=True only; pass adaptors=True or {_LOOP}")
    if recipe is None:
        raise NotImplementedError(f"{WHAT} is built for the release recipes local43_global32 and (adaptors=True) local43_adaptkv_global32 only "
                                  f"(local + global compressor, use_guide='direct', no adaptors but adapt_k / adapt_v, no clip scale); {_LOOP}")
    if local_logits is not None and fe is not None:
        raise ValueError(f"{WHAT}: local_logits replaces frames_embed: pass frames_embed=None")
    if local_logits is not None and recipe != "plain":
        raise NotImplementedError(f"{WHAT}: {ragged.NOT_LINEAR}")
    for name, t in (("frames_feature", ff), ("frames_embed", fe), ("guide_embeds", guides), ("local_logits", local_logits)):
        if not input_grads and isinstance(t, torch.Tensor) and t.requires_grad:
            raise NotImplementedError(f"{WHAT}: the gradient w.r.t. {name} (stage 3) is not built for the ragged training step without "
                                      f"input_grads=True; pass it, detach {name}, or {_LOOP}")


class _PlanTrain:
    """What the backward derives from a ragged plan (SegPlan.train): each field is made when first asked for and kept with the plan."""

    def __init__(self, plan, dev):
        self._tables, self._io, self._dev = plan.tables, plan.io, dev

    # ragged.train_row_maps as device index tensors: (local rows, newline rows, global rows)
    row_maps = functools.cached_property(lambda s: tuple(torch.from_numpy(m).to(s._dev) for m in ragged.train_row_maps(s._tables)))
    # ragged.dx_tile_table as a device int32 [ntiles, 2] tensor
    dx_tiles = functools.cached_property(lambda s: torch.from_numpy(ragged.dx_tile_table(s._tables)).to(s._dev))
    # the window -> item index (plan_tables' win_item) as a device int64 tensor: the query row of a window is its item's guide
    win_item = functools.cached_property(lambda s: torch.from_numpy(s._tables.win_item.astype("int64")).to(s._dev))
    bwd_ws_bytes = functools.cached_property(lambda s: nv.compressor_ragged_global_bwd_workspace(s._io))
    # the native calls of the backward over the plan's rows (looked up per call): the global stage's attention backward and, for the input
    # gradients, the window backward and the global stage's d x.  ragged_backward reads row_maps, dx_tiles, bwd_ws_bytes and these three
    # only: a plan whose rows are (item, guide) pairs brings its own (ragged_multi_guide_train.py), with the same arguments
    global_bwd = property(lambda s: nv.compressor_ragged_global_bwd)
    local_bwd = property(lambda s: nv.compressor_ragged_local_bwd)
    global_dx = property(lambda s: nv.compressor_ragged_global_dx)


_ADAPTOR_PARAMS = tuple(f"local_compressor.{s}_{part}" for s in "kv" for part in ("proj.", "norm.", "alpha"))


def _adaptor_wanted(names):
    return any(n.startswith(_ADAPTOR_PARAMS) for n in names)


class _RaggedTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, proj, ff, fe, guides, nl, ll, meta, names, *params):
        split_sizes, modals, chunks, rows = meta
        with torch.no_grad():
            out, plan, x, g = ragged.call_ragged(proj, ff, fe, guides, split_sizes, modals, nl, chunks, what=WHAT, refuse_grad=False, local_logits=ll)
            t, a, dev = plan.tables, plan.io, x.device
            plan.train = plan.train or _PlanTrain(plan, dev)
            # frames_embed, by reference, only where the window backward will run (an input gradient is asked for, or an adaptor trains)
            lc = proj.local_compressor
            adapt = lc.adapt_k or lc.adapt_v
            window = any(ctx.needs_input_grad[1:4]) or (adapt and _adaptor_wanted(n for k, n in enumerate(names) if ctx.needs_input_grad[8 + k]))
            keys = fe.contiguous() if (fe is not None and window) else None
            # the logits form: the scores, by reference, only where its window backward will run (d frames_feature or d local_logits)
            needs_scores = ll is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[5])
            lsaved = ll.detach().reshape(x.shape[:3]).contiguous() if needs_scores else None
            R, E = a.B * a.nh, a.E
            f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
            ctx16 = torch.empty((sum(t.windows), E), dtype=torch.float16, device=dev)
            scores, ml, ctxg = f(16 * 16 * sum(t.ntiles)), f(R, 2), f(R, E)
            nv.compressor_ragged_train_state(a, ctx16, scores, ml, ctxg)      # (the workspace belongs to the plan's next call)
            ky = vy = None
            if adapt and window:                                   # the y planes of the adapted streams, the forward's own bits
                N = x.numel() // E
                ky = torch.empty((N, E), dtype=torch.float16, device=dev) if lc.adapt_k else None
                vy = torch.empty((N, E), dtype=torch.float16, device=dev) if lc.adapt_v else None
                nv.compressor_ragged_adapt_train_state(plan.args, ky, vy)
        rows.extend(plan.rows)                                 # (for the caller: how to split the output)
        ctx.proj, ctx.plan, ctx.names = proj, plan, names
        ctx.nl_meta = None if nl is None else nl.dtype
        ctx.logits_form, ctx.ll_shape = ll is not None, None if ll is None else ll.shape
        ctx.save_for_backward(x, g, ctx16, scores, ml, ctxg, keys, ky, vy, lsaved)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, guides, ctx16, scores, ml, ctxg, keys, ky, vy, ll = ctx.saved_tensors
        proj, plan, names = ctx.proj, ctx.plan, ctx.names
        need = ctx.needs_input_grad            # (proj, ff, fe, guides, nl, ll, meta, names, *params)
        want = {n for k, n in enumerate(names) if need[8 + k]}
        inputs = types.SimpleNamespace(want_ff=bool(need[1]), want_fe=bool(need[2]), want_guide=bool(need[3]), fe=keys, d_ff=None, d_fe=None, d_guide=None,
                                       logits_form=ctx.logits_form, ll=ll, want_ll=bool(need[5]), d_ll=None)
        with torch.no_grad():
            grads, d_nl = ragged_backward(proj, plan, x, guides, ctx16, scores, ml, ctxg, dout, want, bool(need[4]), inputs, adapt=(ky, vy))
        ag.LAST_FP32_GRADS = dict(grads)               # (test hook, as the single-item backward leaves it; here with d image_newline)
        if d_nl is not None:
            ag.LAST_FP32_GRADS["image_newline"] = d_nl
        d_g = None
        if inputs.d_guide is not None:
            ag.LAST_FP32_GRADS["__guide_embeds__"] = inputs.d_guide        # (fp32 [B, E], as the single-item path leaves "__guide_embed__")
            d_g = inputs.d_guide.to(guides.dtype)
        plist = dict(proj.named_parameters())
        out = [None] * len(names)
        by_dtype = {}
        for k, n in enumerate(names):
            if n in want and grads.get(n) is not None:
                by_dtype.setdefault(plist[n].dtype, []).append((k, n))
        for dt, group in by_dtype.items():                     # views of ONE buffer per parameter dtype, cast once
            flat, o = torch.cat([grads[n].reshape(-1) for _, n in group]).to(dt), 0
            for k, n in group:
                cnt = plist[n].numel()
                out[k] = flat[o:o + cnt].view(plist[n].shape)
                o += cnt
        d_ll = None if inputs.d_ll is None else inputs.d_ll.view(ctx.ll_shape)
        return (None, inputs.d_ff, inputs.d_fe, d_g, None if d_nl is None else d_nl.to(ctx.nl_meta), d_ll, None, None, *out)


def _local_adapt_backward(st, lc, plan, guides, dctx_l, fe, ky, vy, want_kx, want_vx, want_guide):
    """The local stage behind the readout for the k / v adaptor recipe: the window backward through the blends over all items, the adaptors'
    reductions and the MLPs' backward over the stacked tokens.  Fills st.grads; returns (dq_w or None, d_kx, d_vx), bf16 [sum N_i, E] each."""
    a, x, dev, E = plan.io, st.ff, st.dev, plan.io.E
    kx2, vx2 = (fe if fe is not None else x).view(-1, E), x.view(-1, E)
    N, nw = vx2.shape[0], dctx_l.shape[0]
    f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
    ds, pw = f(N), f(N)
    sxk = f(nw, E) if (lc.adapt_k or want_guide) else None
    syk = f(nw, E) if lc.adapt_k else None
    sxv, syv = (f(nw, E), f(nw, E)) if lc.adapt_v else (None, None)
    nv.compressor_ragged_local_adapt_bwd(a, kx2, ky, lc.k_norm, lc.k_alpha, vx2, vy, lc.v_norm, lc.v_alpha, guides, dctx_l, ds, pw, sxk, syk, sxv, syv,
                                         eps=(lc.k_norm if lc.adapt_k else lc.v_norm).eps)
    # the hidden planes, recomputed: one layer-1 GEMM per adapted stream, in the forward's arithmetic
    rec_k = (ag._adaptor_hidden(kx2, lc.k_proj)[0], None, ky) if lc.adapt_k else None
    rec_v = (ag._adaptor_hidden(vx2, lc.v_proj)[0], None, vy) if lc.adapt_v else None
    qf = guides.float()[plan.train.win_item] if lc.adapt_k else None           # the query row of every window: its item's guide
    dy_of = lambda per_item: lambda y, gamma, vec, coef, alpha, dy, r1, **kw: nv.compressor_ragged_adapt_dy(a, y, gamma, vec, per_item, coef, alpha, dy, r1, **kw)
    return ag._adaptor_streams_backward(lc, st.f32, st.grads, kx2, vx2, rec_k, rec_v, qf, guides, dctx_l, (ds, pw, sxk, syk, sxv, syv), want_kx, want_vx,
                                        dy_of(True), dy_of(False), want_dq=want_guide)


def _local_backward(st, ctx16, dout, local_rows, window, adapt):
    """The local stage: the readout backward over the sum of all items' windows and, where `window`, the window backward of the module's
    recipe behind it, which leaves d frames_embed and the local share of d frames_feature in st.inputs.  Returns dq_item (fp32 [B, E], the
    local share of d guide) or None."""
    lc, plan, x, guides, inputs, f32 = st.proj.local_compressor, st.plan, st.ff, st.guides, st.inputs, st.f32
    a, fe, L = plan.io, inputs.fe, "local_compressor.readout."
    adaptors = lc.adapt_k or lc.adapt_v
    assert adaptors or inputs.logits_form or ag._window_backward_runs(lc, st.want_fe, st.want_guide, st.proj.local_logit, st.want_ff) == window
    ctx_l = ctx16.float()
    W0, b0 = f32[L + "0.weight"], f32[L + "0.bias"]
    dpre = ag._readout_backward(ctx_l, torch.addmm(b0, ctx_l, W0.t()), f32[L + "2.weight"], dout[local_rows], L, st.grads)
    if not window:
        return None
    dctx_l = (dpre @ W0).contiguous()
    if inputs.logits_form:
        # the scores were given: d local_logits and the value-side share of d frames_feature from one launch; the guide does not enter this stage
        inputs.d_ll = torch.empty_like(inputs.ll)
        inputs.d_ff = torch.empty_like(x) if st.want_ff else None
        nv.compressor_ragged_local_logits_bwd(a, x, inputs.ll, dctx_l, inputs.d_ll, inputs.d_ff)
        if not inputs.want_ll:
            inputs.d_ll = None
        return None
    dq_item = torch.empty((guides.shape[0], a.E), dtype=torch.float32, device=st.dev) if st.want_guide else None     # (a row per item, or per pair)
    if adaptors:
        dq_w, d_kx, d_vx = _local_adapt_backward(st, lc, plan, guides, dctx_l, fe, *adapt, st.want_fe or (st.want_ff and fe is None), st.want_ff, st.want_guide)
        if st.want_guide:
            nv.compressor_ragged_dq_item(a, dq_w.contiguous(), dq_item)
        d_fe = d_kx.view(fe.shape) if st.want_fe else None
        # the value stream's input gradient and, without frames_embed, the key's
        d_ff = (d_vx if fe is not None else (d_vx.float() + d_kx.float()).to(x.dtype)).view(x.shape) if st.want_ff else None
    else:
        dq_w = torch.empty_like(dctx_l)
        d_fe = torch.empty_like(fe) if st.want_fe else None
        d_ff = torch.empty_like(x) if st.want_ff else None      # (value-side share; without frames_embed the key-side term is added in)
        plan.train.local_bwd(a, fe if fe is not None else x, x, guides, dctx_l, dq_w, dq_item, d_fe, d_ff, value_is_key=st.want_ff and fe is None)
    inputs.d_fe, inputs.d_ff = d_fe, d_ff
    return dq_item


def _global_backward(st, scores, ml, ctxg, dout, glob_rows, dq_item):
    """The global stage, rows item-major (pair-major where the plan's rows are (item, guide) pairs: the M guides are then the M queries): the
    tail, the attention backward over all rows in one native call (plan.train.global_bwd), the fold and q_proj; then the
    global shares of d frames_feature (added into st.inputs.d_ff) and of d guide (st.inputs.d_guide = dq_item + it)."""
    plan, x, inputs, f32 = st.plan, st.ff, st.inputs, st.f32
    a, dev = plan.io, st.dev
    att = st.proj.global_compressor.attn_layer
    nh, hd = att.num_heads, att.head_dim
    q32 = st.guides.float()
    dtok = dout[glob_rows].sum(1)                              # [B, hidden]: an item's global rows are copies of one row
    dpre_g, dctx, delta = ag._global_tail_backward(st, nh, hd, ml, None, q32, dtok, ctxg=ctxg)
    ds, dqt = torch.empty_like(scores), torch.empty_like(ctxg)
    ws = torch.empty((plan.train.bwd_ws_bytes,), dtype=torch.uint8, device=dev)
    plan.train.global_bwd(a, x, dctx, delta, scores, ml, ds, dqt, ws)
    A = "global_compressor.attn_layer."
    Wq, bq, Wk = f32[A + "q_proj.weight"], f32[A + "q_proj.bias"], f32[A + "k_proj.weight"]
    dqp = ag._global_fold_backward(st, att, None, None, None, None, q32, Wq, bq, Wk, dqt=dqt)
    ag._q_proj_backward(st.grads, dqp, q32)
    if st.want_ff:
        # d frames_feature, global share (the algebra of autograd._global_dff with the B guides as the B queries): qt for all B nh rows,
        # then one call over all items, added to the rows the window backward left
        E = q32.shape[1]
        qp_ = (q32 @ Wq.t() + bq).view(-1, nh, hd)
        qt_ = (att.scale * torch.einsum("hje,qhj->qhe", Wk.view(nh, hd, E), qp_)).reshape(-1, E).contiguous()
        plan.train.global_dx(a, scores, ds, ml, qt_, dctx, plan.train.dx_tiles, inputs.d_ff.view(-1, E), accumulate=True)
    if st.want_guide:
        # direct recipe: the injected query IS the guide, one row per item (autograd._global_query_backward) + the local stage's share
        glob = dqp @ Wq + dpre_g
        inputs.d_guide = glob if dq_item is None else dq_item + glob       # (the logits form: the global share only)


def ragged_backward(proj, plan, x, guides, ctx16, scores, ml, ctxg, dout, want, want_nl, inputs, adapt=(None, None)):
    """(fp32 gradients {parameter name: tensor} of sum(out * dout) over all items, d image_newline or None): _local_backward, then
    _global_backward, over one shared state `st`.  `want`: the names of the parameters whose gradient is asked for; a stage none of whose
    parameters is wanted does not run unless an input gradient needs it.
    inputs: want_ff / want_fe / want_guide (the input gradients asked for) and the contiguous frames_embed (or None) in, d_ff / d_fe (bf16,
    the inputs' shapes) and d_guide (fp32 [B, E]) out.  adapt: (ky, vy) of the adaptor recipe, the y planes the forward kept (None for a
    stream without adaptor; both None for the plain recipe)."""
    lc, dev = proj.local_compressor, x.device
    local_rows, nl_rows, glob_rows = plan.train.row_maps
    dout = dout.float()
    st = types.SimpleNamespace(proj=proj, plan=plan, ff=x, guides=guides, dev=dev, f32=ag._f32_params(proj), grads={}, inputs=inputs,
                               want_ff=inputs.want_ff, want_fe=inputs.want_fe and inputs.fe is not None, want_guide=inputs.want_guide)
    d_nl = dout[nl_rows].sum(0) if (want_nl and nl_rows.numel()) else None
    # the window backward: every input gradient has a local share; with adaptors, also where one of them trains
    window = st.want_ff or st.want_fe or st.want_guide or ((lc.adapt_k or lc.adapt_v) and _adaptor_wanted(want))
    if inputs.logits_form:                                     # the guide has no local share there; the scores have
        window = st.want_ff or inputs.want_ll
    dq_item = None
    if window or any(n.startswith("local_compressor.") for n in want):
        dq_item = _local_backward(st, ctx16, dout, local_rows, window, adapt)
    if st.want_ff or st.want_guide or any(n.startswith("global_compressor.") for n in want):
        _global_backward(st, scores, ml, ctxg, dout, glob_rows, dq_item)
    return st.grads, d_nl


def run_ragged_train(proj, ff, fe, guides, split_sizes, modals, nl, chunks=None, input_grads=False, adaptors=False, local_logits=None):
    check_scope(proj, ff, fe, guides, input_grads, adaptors, local_logits)
    if local_logits is not None:                               # shape, dtype and device in front of any device work
        ragged._scope(proj, ff, fe, guides, split_sizes, modals, nl, WHAT)
        ragged.check_logits(WHAT, proj, local_logits, fe, ff)
    params = [(n, p) for n, p in proj.named_parameters()]
    trainable = torch.is_grad_enabled() and (any(p.requires_grad for _, p in params) or (isinstance(nl, torch.Tensor) and nl.requires_grad)
                                             or (input_grads and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (ff, fe, guides, local_logits))))
    if not trainable:                                          # nothing to differentiate: forward_ragged's call, no graph
        nv.begin_inference()
        out, plan, _, _ = ragged.call_ragged(proj, ff, fe, guides, split_sizes, modals, nl, chunks, what=WHAT, refuse_grad=False, local_logits=local_logits)
        return list(out.split(plan.rows))
    nv.note_training_forward()                                 # (the plan's refresh() then rebuilds the weight-derived tables from the live weights)
    names, ps = zip(*params)
    rows = []
    out = _RaggedTrainFn.apply(proj, ff, fe, guides, nl, local_logits, (split_sizes, modals, chunks, rows), names, *ps)
    return list(out.split(rows))
