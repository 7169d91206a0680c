"""HIComProjector.open_stream_group_adapt: the clip stream group with several guides per slot (clip_stream_group_multi.py) for a module of
the k / v adaptor recipe (`local43_adaptkv_global32`: adapt_k and / or adapt_v on the local compressor), the adaptor MLPs run ONCE per
tick over the stacked tokens of all B videos (csrc/clip_stream_group_multi.hip: the flavour Adapt).

    g = proj.open_stream_group_adapt(guide_embeds[sum Q_s, E], guide_counts, H, W, max_frames, image_newline)
    views = g.push(frames_feature[sum Tc_i, H, W, E], frames_embed or None, split_sizes, slots=None)    # views[i]: [Q_slot_i, chunk rows, hidden]
    out   = g.finish(slot);  outs = g.finish_many(slots=None);  g.reset(slot, guides=None)
    g.frames[slot], g.rows(slot), g.guide_counts

guide_counts == (1,) * B is the case of one guide per slot.  The surface, the state layout, the output storage [M, cap_rows + 32, hidden],
finish, finish_many, reset, the slot rules and the errors are ClipStreamGroupMulti's: the adaptors sit on the local stage only and the
global stage of the recipe is the plain one.  Only the front of a push differs (hicom_compressor_stream_group_adapt_push, eight launches
whatever B, the Q_s and the chunk lengths are): both layers of each adaptor MLP over the tick's sum N_i stacked tokens -- they know neither
the guide nor the slot, so ONE GEMM pair per layer serves every video -- into fp16 planes ky / vy [sum N_i, E] that live for that push; the
adaptor local stage, one wave per window of the stack, which reads an item's tokens and its rows of the planes and walks the guides of the
item's slot in groups of 4; then launches 2-6 of the plain group push.  Without frames_embed the k adaptor reads frames_feature, as the
keys do.

Per plan -- ClipStreamGroupMulti's key plus the adaptor set, cached on the module as `proj._clip_stream_group_adapt_plans` -- the ONE
workspace: the parent's regions and, behind them, the two planes and the hidden planes of layer 1 (4 x 2304 bytes per token of a TICK with
both adaptors).  The planes are written and read inside one push, in stream order, so the groups of one module share a plan.  push
allocates nothing.  The plan follows the weights as every plan does: its refresh rebuilds the cached fp16 copies of the readout and of the
adaptors' second layers.

Scope: that of open_stream_group_multi with the adaptor recipe in the place of the plain one, adaptor widths % 64 == 0 and
(sum Tc_i) H W E < 2^32 per push (the dense GEMM's operand limit over the stack)."""
from __future__ import annotations

from . import clip_stream as cs
from . import clip_stream_group_multi as cgm
from . import native as nv
from . import segments as seg

STORE_GROUP_ADAPT = "_clip_stream_group_adapt_plans"


class _SlotGuides:
    """cgm._SlotGuides for the adaptor recipe: what stream_scope is told when reset(slot, guides) checks ONE slot's new guides."""
    WHAT, RECIPE, MULTI = "ClipStreamGroupAdapt.reset", "adaptkv", True


class ClipStreamGroupAdapt(cgm.ClipStreamGroupMulti):
    """The object HIComProjector.open_stream_group_adapt returns for a module of the k / v adaptor recipe (module docstring)."""
    NAME, WHAT, STORE = "ClipStreamGroupAdapt", "open_stream_group_adapt", STORE_GROUP_ADAPT
    RECIPE, RECIPE_WORDS = "adaptkv", "the k / v adaptor release recipe"
    SLOT_GUIDES = _SlotGuides
    NO_LOGITS = cs.NOT_LINEAR                    # (push is the base's: its local_logits keyword raises NotImplementedError here)

    def head_scores(self, last_hidden_state, head, split_sizes, slots=None, hidden_act=None):
        raise NotImplementedError(f"{self.NAME}.head_scores: {cs.NOT_LINEAR}")

    def _scope(self, proj, guide_embeds, H, W, max_frames, image_newline):
        dims = super()._scope(proj, guide_embeds, H, W, max_frames, image_newline)
        cs.adaptor_widths(self.WHAT, proj.local_compressor)
        return dims

    def _chunk_limits(self, what, proj, Tc, H, W, E):
        super()._chunk_limits(what, proj, Tc, H, W, E)
        cs.adapt_chunk_limit(what, Tc, H, W, E)

    def _check_push(self, ff, fe, split_sizes, slots):
        """The parent's refusals, then the operand limit of the adaptor GEMMs on the STACK (the C entry checks the same)."""
        tcs, slots = super()._check_push(ff, fe, split_sizes, slots)
        if sum(tcs) * self.H * self.W * self.E >= 1 << 32:
            raise NotImplementedError(f"{self.NAME}.push: {sum(tcs)} stacked frames of {self.H}x{self.W}: the adaptor GEMMs take operands below 2^32 "
                                      "elements over the whole stack; push fewer or shorter chunks per call")
        return tcs, slots

    def _plan_key(self, tcqs, has_fe, stream):
        lc = self.proj.local_compressor
        return super()._plan_key(tcqs, has_fe, stream) + (bool(lc.adapt_k), bool(lc.adapt_v))

    def _native(self):
        return (nv.StreamGroupAdaptPushArgs, nv.compressor_stream_group_adapt_workspace, nv.compressor_stream_group_adapt_prepare,
                nv.compressor_stream_group_adapt_push)

    def _fill_front(self, args):
        """The adaptor descriptors (the workspace query reads them: the planes are regions of the plan's workspace) and the refresh that
        follows the adaptors' second layers as well."""
        lc = self.proj.local_compressor
        keep = []

        def ptr(t):
            if t is None:
                return None
            keep.append(t)
            return t.data_ptr()
        seg.fill_adaptors(args, lc, self.WHAT, ptr)

        def refresh():
            lc.readout_f16()
            seg.refresh_adaptors(lc)
        return keep, refresh
