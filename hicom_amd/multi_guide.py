"""HIComProjector.forward_multi_guide: ONE clip, Q instructions through hicom_compressor_multiguide_fwd (csrc/multi_guide.hip).

The reference's Video-MME driver asks every question of a video with its own projector run over the same video tensor
(hicom/eval/video/inference_video_mcqa_videomme.py:268-303).  The guide is only the query of the two stages, so here the visual tokens
are streamed once for all Q guides: the local stage loads each window row once per group of guides, the global stage runs the 9 Q folded
rows through the many-row stream kernel of the guide-off recipe.  Scope rule, input checks, plan and plan cache are segments.py's, shared
with forward_batch and forward_ragged; the plain release recipe only.  Plans are keyed by shape, Q included.

Logits form: with `local_logits` = fp32 [Q, T, H, W] from `siglip_head_scores_multi` the local stage takes its scores
from that tensor and reads the value rows only (hicom_compressor_multiguide_logits_fwd: the same sequence, another launch 3); frames_embed
is None, as for forward(..., local_logits=).  The two forms do not share a plan: the key carries the form."""
from __future__ import annotations

import torch

from . import native as nv
from . import segments as seg

MAX_GUIDES = 32         # 9 heads x 32 guides = 288 folded rows, the row count the many-row stream kernel is proven at
STORE = "_multi_guide_plans"


def count_guides(what, guides, E):
    """Q of guide_embeds [Q, E]; raises unless 1 <= Q <= MAX_GUIDES."""
    if not isinstance(guides, torch.Tensor) or guides.ndim != 2 or guides.shape[1] != E:
        raise ValueError(f"{what}: guide_embeds is [Q, E] = [Q, {E}], one instruction per row "
                         f"(got {tuple(guides.shape) if isinstance(guides, torch.Tensor) else None})")
    if not 1 <= guides.shape[0] <= MAX_GUIDES:
        raise ValueError(f"{what}: Q={guides.shape[0]} guides (1 <= Q <= {MAX_GUIDES} per call)")
    return guides.shape[0]


def clip_scope(what, step, proj, ff, fe, guides, modal, nl):
    """The checks of a step on ONE clip with Q guides (this one and forward_prepared, prepared.py) behind the caller's rule on the recipe;
    returns (Q, T, H, W, E, tilings)."""
    Q, E = seg.check_inputs(what, step, proj, ff, fe, guides, nl, 4, "[T, H, W, E]", lambda: count_guides(what, guides, ff.shape[-1]))
    T, H, W, _ = ff.shape
    if modal == "image" and T != 1:
        raise ValueError(f"{what}: image modality expects a single frame [1, H, W, E]")
    return Q, T, H, W, E, seg.exact_tilings(what, proj, T, H, W, modal)


def _scope(proj, ff, fe, guides, modal, nl):
    """Raises for everything outside the step's scope; returns (Q, T, H, W, E, tilings)."""
    what = "forward_multi_guide"
    if not isinstance(ff, dict) and not isinstance(fe, dict) and seg.seg_recipe(proj) != "plain":
        raise NotImplementedError(f"{what} is built for the plain release recipe only (local + global compressor, use_guide='direct', no "
                                  "adaptors, no clip scale); the adaptor recipe and everything else go through forward() per guide")
    return clip_scope(what, "multi-guide", proj, ff, fe, guides, modal, nl)


def _require_f32_cuda(name, t):
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: float32 expected, got {t.dtype} (siglip_head_scores_multi returns it)")
    if not t.is_cuda:
        raise ValueError(f"{name}: a device tensor expected (got {t.device})")


def check_logits(what, ll, fe, Q, grid):
    """The checks of local_logits behind the scope checks of the keyed call and in front of any device work: frames_embed must be None
    (forward(..., local_logits=) has the same rule), fp32 device [Q, T, H, W]."""
    if fe is not None:
        raise ValueError(f"{what}: local_logits replaces frames_embed: pass frames_embed=None")
    if not isinstance(ll, torch.Tensor) or ll.ndim != 4 or tuple(ll.shape[1:]) != tuple(grid):
        raise ValueError(f"{what}: local_logits is [Q, T, H, W] = [{Q}, {', '.join(map(str, grid))}], one plane of raw dot products per guide "
                         f"(got {tuple(ll.shape) if isinstance(ll, torch.Tensor) else None})")
    if ll.shape[0] != Q:
        raise ValueError(f"{what}: local_logits holds {ll.shape[0]} guides, guide_embeds {Q}")
    _require_f32_cuda("local_logits", ll)


def plan_key(Q, T, H, W, E, has_fe, modal, nl, out_dtype, stream, chunks, logits=False):
    """The key of a plan; the keyed form's is what it was before the logits form (so its plans and their order in the store do not change)."""
    key = (Q, T, H, W, E, has_fe, modal, None if nl is None else tuple(nl.shape), out_dtype, stream, int(chunks or 0))
    return key + ("logits",) if logits else key


def run_multi_guide(proj, ff, fe, guides, modal, nl, chunks=None, local_logits=None):
    Q, T, H, W, E, tiles = _scope(proj, ff, fe, guides, modal, nl)
    if local_logits is not None:
        check_logits("forward_multi_guide", local_logits, fe, Q, (T, H, W))
    dev, ff, fe, guides, nl, out_dtype, stream = seg.call_inputs(proj, "forward_multi_guide", ff, fe, guides, nl)
    key = plan_key(Q, T, H, W, E, fe is not None, modal, nl, out_dtype, stream, chunks, local_logits is not None)
    plan = seg.cached_plan(proj, STORE, key, lambda: seg.build_equal_plan(
        proj, "forward_multi_guide", nv.CompressorMultiGuideArgs, None, "Q", (Q, T, H, W, E), tiles, modal, nl, out_dtype, chunks, dev,
        nv.compressor_multiguide_workspace))                                         # (no adaptor recipe: _scope refuses it)
    a = plan.io
    out = torch.empty((Q, plan.rows, plan.hidden), dtype=out_dtype, device=dev)
    seg.patch_io(a, ff, fe, guides, nl if a.nl_count > 0 else None, out, stream)
    if local_logits is not None:
        ll = local_logits.contiguous()
        nv.compressor_multiguide_logits_fwd(plan.args, ll.data_ptr(), T * H * W)
    else:
        nv.compressor_multiguide_fwd(plan.args)
    return out
