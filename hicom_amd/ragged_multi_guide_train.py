"""HIComProjector.forward_ragged_multi_guide_train: the training step of a mixed batch whose item i has Q_i instructions -- the one C call
of forward_ragged_multi_guide under autograd.

A multi-turn item (one clip, one instruction per turn), or a batch of them, otherwise trains through forward_ragged_train on the clip's
tokens replicated Q_i times (a token-sized copy, and both stages read the tokens Q_i times) or through the loop of forward() + backward
per (item, guide) pair.  Here the forward is forward_ragged_multi_guide's call on its plan (same plan cache, same bits:
hicom_compressor_ragged_multiguide_fwd, or _logits_fwd with local_logits) and the backward is ONE eager pass over all M = sum Q_i pairs.
Behind the two native launches that read tokens a pair is an item, so the backward is ragged_train.ragged_backward with M rows -- the
readout backward over all pairs' window contexts, the global tail with the M guides as the M queries, the fold and q_proj -- on three
things this module's plans bring:

  row maps     ragged_multi_guide.train_row_maps: the local, newline and global rows of every pair in the pair-major packed output;
               d image_newline = the sum of all pairs' newline rows
  native call  hicom_compressor_ragged_multiguide_global_bwd (csrc/ragged_multi_guide_train.hip): the two-row-group backward stream on the
               forward's work units -- an item's tokens are read once per 32 folded rows, not once per guide -- and the dq merge per
               (pair, head); four launches whatever B, the Q_i and the mix are
  state        hicom_compressor_ragged_multiguide_train_state: window contexts, scores, (M, L) and merged contexts, pair-major, copied out
               of the plan's workspace into tensors the autograd node owns, so forward, forward, backward, backward on one plan works.

Input gradients (stage 3 of the release script, train.py:712-726; `input_grads=True`): every one of frames_feature,
frames_embed and guide_embeds that requires grad gets its gradient from the same one backward, through three more native calls that
ragged_backward reaches through the plan (csrc/ragged_multi_guide_train.hip):

  local stage    hicom_compressor_ragged_multiguide_local_bwd: the window backward over the sum windows_i windows of the stacked tensor, every
                 window for all Q_i guides of its item: dq per (pair, window), d frames_embed and the value-side share of d frames_feature
                 (with the key-side term where frames_embed is None) -- a token's sum over the guides is formed in fp32 in the order
                 q = 0 .. Q_i - 1 and written once; hicom_compressor_ragged_multiguide_dq_pair sums dq per pair, only where d guide is asked for;
  global stage   hicom_compressor_ragged_multiguide_global_dx: dS^T qt + P^T dctx over all nh Q_i rows of the token's item, one fp32 chain
                 from the row the window backward left, one bf16 store: a token of d frames_feature is rounded twice whatever Q_i is.

d guide_embeds[pair] = dq_pair[pair] + row pair of (dqp Wq + dpre): fp32 [M, E] in autograd.LAST_FP32_GRADS["__guide_embeds__"].  An input that
does not require grad costs nothing (NULL output pointer, or no launch); a step with every parameter frozen and an input requiring grad is
trainable; parameter gradients and d image_newline are bit-equal to the same step with the inputs detached.  frames_embed is kept by
reference, and only where the window backward will run.  With every Q_i = 1 the three input gradients are forward_ragged_train's, bit for bit.

Scope: the plain release recipe local43_global32, bf16 module and inputs, exact window partition per item, 1 <= Q_i <= 32; gradients of
every projector parameter that requires grad and of image_newline (stages 1 and 2 of the release script) and, with input_grads=True, of
the three inputs.  The logits form (`local_logits`, frames_embed None) has the head frozen: the backward is the keyed one with no further
launch, and with input_grads=True the local share of its input gradients is not built -- local_logits that requires grad raises.
Everything else -- the k / v adaptor recipe, clip-scale, anyres dicts, fp16 / fp32, an input that requires grad without input_grads=True
-- raises in front of any device work and names the loop of forward() per pair; nothing is detached silently.  A stage none of whose
parameters requires grad runs only where an input gradient needs it.

Which path when (tools/ragged_multi_guide_train_bench.py, DESIGN.md §3.26 has the table): a batch in which every Q_i = 1 is
forward_ragged_train's -- this step runs the same arithmetic there (the fp32 gradients are bit-equal) behind a 512-thread stream whose
second row group idles."""
from __future__ import annotations

import functools
import types

import torch

from . import autograd as ag
from . import native as nv
from . import ragged_multi_guide as rmg
from . import ragged_train
from . import segments as seg

WHAT = "forward_ragged_multi_guide_train"
_LOOP = "run the loop of forward() per (item, guide) pair instead"


def check_scope(proj, ff, fe, guides, local_logits=None, input_grads=False):
    """The refusals of the training step that forward_ragged_multi_guide does not make, or makes without naming the loop; no device is
    touched."""
    if isinstance(ff, dict) or isinstance(fe, dict):
        raise NotImplementedError(f"{WHAT}: anyres dict inputs have no ragged multi-guide training step; {_LOOP}")
    if proj.local_use_clip_scale or proj.global_use_clip_scale:
        raise NotImplementedError(f"{WHAT}: clip-scale is not built for the ragged multi-guide training step; {_LOOP}")
    recipe = seg.seg_recipe(proj)
    if recipe == "adaptkv":
        raise NotImplementedError(f"{WHAT}: the k / v adaptor recipe (local43_adaptkv_global32) is not built for the ragged multi-guide training "
                                  f"step; {_LOOP}")
    if recipe is None:
        raise NotImplementedError(f"{WHAT} is built for the plain release recipe local43_global32 only (local + global compressor, "
                                  f"use_guide='direct', no adaptors, no clip scale); {_LOOP}")
    wdt = proj.local_compressor.readout[0].weight.dtype
    if wdt != torch.bfloat16:
        raise NotImplementedError(f"{WHAT}: a {wdt} projector; the step takes a bfloat16 module and bfloat16 inputs; cast them or {_LOOP}")
    for name, t in (("frames_feature", ff), ("frames_embed", fe), ("guide_embeds", guides)):
        if isinstance(t, torch.Tensor) and t.dtype != torch.bfloat16:
            raise NotImplementedError(f"{WHAT}: {name} is {t.dtype}; the step takes bfloat16 inputs; cast it or {_LOOP}")
    if local_logits is not None and fe is not None:
        raise ValueError(f"{WHAT}: local_logits replaces frames_embed: pass frames_embed=None (or {_LOOP})")
    if input_grads:
        if isinstance(local_logits, torch.Tensor) and local_logits.requires_grad:
            raise NotImplementedError(f"{WHAT}: the gradient w.r.t. local_logits is not built for the ragged multi-guide training step, with "
                                      f"input_grads=True either (the logits form with input gradients); detach local_logits or {_LOOP}")
        if local_logits is not None and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (ff, guides)):
            raise NotImplementedError(f"{WHAT}: input gradients of the logits form (local_logits with frames_feature or guide_embeds requiring grad) "
                                      f"are not built for the ragged multi-guide training step; detach them or {_LOOP}")
        return
    for name, t in (("frames_feature", ff), ("frames_embed", fe), ("guide_embeds", guides), ("local_logits", local_logits)):
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise NotImplementedError(f"{WHAT}: the gradient w.r.t. {name} (stage 3) is not built for the ragged multi-guide training step "
                                      f"without input_grads=True; pass it, detach {name} or {_LOOP}")


class _PairPlanTrain:
    """What ragged_train.ragged_backward reads from a plan (SegPlan.train), for a plan whose rows are (item, guide) pairs: each field is made
    when first asked for and kept with the plan."""

    def __init__(self, plan, dev):
        self._tables, self._io, self._dev = plan.tables, plan.io, dev

    # ragged_multi_guide.train_row_maps as device index tensors: (local rows, newline rows, global rows [M, n_global_rows])
    row_maps = functools.cached_property(lambda s: tuple(torch.from_numpy(m).to(s._dev) for m in rmg.train_row_maps(s._tables)))
    # ragged.dx_tile_table on the step's tables as a device int32 [ntiles, 2] tensor: 64 tokens of one ITEM per tile, whatever its Q_i
    dx_tiles = functools.cached_property(lambda s: torch.from_numpy(rmg.dx_tile_table(s._tables)).to(s._dev))
    bwd_ws_bytes = functools.cached_property(lambda s: nv.compressor_ragged_multiguide_global_bwd_workspace(s._io))
    global_bwd = property(lambda s: nv.compressor_ragged_multiguide_global_bwd)      # (looked up per call)
    local_bwd = property(lambda s: nv.compressor_ragged_multiguide_local_bwd)        # (dq_item: a row per pair)
    global_dx = property(lambda s: nv.compressor_ragged_multiguide_global_dx)


class _RaggedMultiGuideTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, proj, ff, fe, guides, nl, ll, meta, names, *params):
        split_sizes, guide_counts, modals, chunks, plans = meta
        with torch.no_grad():
            out, plan, x, g = rmg.call_ragged_multi_guide(proj, ff, fe, guides, split_sizes, guide_counts, modals, nl, chunks, ll, refuse_grad=False)
            t, a, dev = plan.tables, plan.io, x.device
            plan.train = plan.train or _PairPlanTrain(plan, dev)
            R, E = len(t.pairs) * a.nh, a.E
            f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
            ctx16 = torch.empty((sum(q * w for q, w in zip(t.Q, t.windows)), E), dtype=torch.float16, device=dev)
            scores, ml, ctxg = f(16 * sum(p * rmg.PASS_ROWS * n for p, n in zip(t.passes, t.ntiles))), f(R, 2), f(R, E)
            nv.compressor_ragged_multiguide_train_state(a, ctx16, scores, ml, ctxg)      # (the workspace belongs to the plan's next call)
            # frames_embed, by reference, only where the window backward will run (an input gradient is asked for)
            keys = fe.contiguous() if (fe is not None and any(ctx.needs_input_grad[1:4])) else None
        plans.append(plan)                                     # (for the caller: how to split the output)
        ctx.proj, ctx.plan, ctx.names = proj, plan, names
        ctx.nl_meta, ctx.logits_form = None if nl is None else nl.dtype, ll is not None
        ctx.save_for_backward(x, g, ctx16, scores, ml, ctxg, keys)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, guides, ctx16, scores, ml, ctxg, keys = ctx.saved_tensors
        proj, plan, names = ctx.proj, ctx.plan, ctx.names
        need = ctx.needs_input_grad            # (proj, ff, fe, guides, nl, ll, meta, names, *params)
        want = {n for k, n in enumerate(names) if need[8 + k]}
        # (without input_grads=True no input requires grad here: the window backward never runs and frames_embed is not kept; the logits form
        # has no input gradient in this scope: its scores are not kept)
        inputs = types.SimpleNamespace(want_ff=bool(need[1]), want_fe=bool(need[2]), want_guide=bool(need[3]), fe=keys, d_ff=None, d_fe=None, d_guide=None,
                                       logits_form=ctx.logits_form, ll=None, want_ll=False, d_ll=None)
        with torch.no_grad():
            grads, d_nl = ragged_train.ragged_backward(proj, plan, x, guides, ctx16, scores, ml, ctxg, dout, want, bool(need[4]), inputs)
        ag.LAST_FP32_GRADS = dict(grads)               # (test hook, as forward_ragged_train leaves it; here with d image_newline)
        if d_nl is not None:
            ag.LAST_FP32_GRADS["image_newline"] = d_nl
        d_g = None
        if inputs.d_guide is not None:
            ag.LAST_FP32_GRADS["__guide_embeds__"] = inputs.d_guide        # (fp32 [M, E], as forward_ragged_train leaves its [B, E])
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
        return (None, inputs.d_ff, inputs.d_fe, d_g, None if d_nl is None else d_nl.to(ctx.nl_meta), None, None, None, *out)


def run_ragged_multi_guide_train(proj, ff, fe, guides, split_sizes, guide_counts, modals, nl, chunks=None, local_logits=None, input_grads=False):
    check_scope(proj, ff, fe, guides, local_logits, input_grads)
    params = [(n, p) for n, p in proj.named_parameters()]
    trainable = torch.is_grad_enabled() and (any(p.requires_grad for _, p in params) or (isinstance(nl, torch.Tensor) and nl.requires_grad)
                                             or (input_grads and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (ff, fe, guides))))
    if not trainable:                                          # nothing to differentiate: forward_ragged_multi_guide's call, no graph
        nv.begin_inference()
        out, plan, _, _ = rmg.call_ragged_multi_guide(proj, ff, fe, guides, split_sizes, guide_counts, modals, nl, chunks, local_logits, refuse_grad=False)
        return rmg.pair_views(plan, out)
    # every input check in front of the graph and of any device work (they run again inside the call)
    _, _, _, _, _, counts, _ = rmg.check_inputs(proj, ff, fe, guides, split_sizes, guide_counts, modals, nl)
    if local_logits is not None:
        rmg.check_logits(local_logits, fe, ff, counts)
    nv.note_training_forward()                                 # (the plan's refresh() then rebuilds the weight-derived tables from the live weights)
    names, ps = zip(*params)
    plans = []
    out = _RaggedMultiGuideTrainFn.apply(proj, ff, fe, guides, nl, local_logits, (split_sizes, guide_counts, modals, chunks, plans), names, *ps)
    return rmg.pair_views(plans[0], out)
