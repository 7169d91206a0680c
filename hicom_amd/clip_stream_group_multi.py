"""HIComProjector.open_stream_group_multi: B live videos, slot s with its own Q_s guides, pushed in ONE call per tick and finished in ONE
launch sequence (csrc/clip_stream_group_multi.hip).

A server that follows B videos and holds a few open questions about each had a ClipStreamMulti per video (one launch sequence per video and
tick) or a ClipStreamGroup slot per (video, guide) (every video's tokens stacked and streamed Q times).  Here:

    g = proj.open_stream_group_multi(guide_embeds[sum Q_s, E], guide_counts, H, W, max_frames, image_newline)
    views = g.push(frames_feature[sum Tc_i, H, W, E], frames_embed or None, split_sizes, slots=None)    # views[i]: [Q_slot_i, chunk rows, hidden]
    out   = g.finish(slot)              # [Q_s, local rows of the slot so far + 32, hidden]; the state is not consumed
    outs  = g.finish_many(slots=None)   # the same for several slots (default: every slot with frames), ONE launch sequence
    g.reset(slot, guides=None)          # guides bf16 [Q_s, E]: the count of a slot is fixed at open
    g.frames[slot], g.rows(slot), g.guide_counts

guide_counts holds the B ints Q_s (1 <= B <= 32, 1 <= Q_s <= 32); the guides of slot s are the rows [pair0_s, pair0_s + Q_s) of guide_embeds,
pair0_s = sum_{j<s} Q_j (forward_ragged_multi_guide's convention).  A PAIR is one (slot, guide), M = sum Q_s of them, and everything the
group holds is pair-major: the output storage [M, cap_rows + 32, hidden], state_ml [M nh, 2] and state_acc [M nh, E] (slot s's rows are
contiguous: the one set GlobalCompressor.finish_guides reads), the query operands with row pair nh + h, padded to whole 32-row passes.
finish(slot)[q] is forward() on the concatenation of everything pushed into the slot with the slot's guide q, to the kernels' rounding;
`slots` of a push as for ClipStreamGroup: a slot at most once, an absent slot is not touched.

Who holds what.  ClipStreamGroup has the checks of a push, the per-slot counters, the spans and the pair-major device side (allocation,
query preparation, plan, launch and push: one body, of which ClipStreamGroup itself is the case of one pair per slot); ClipStreamBase the
scope, the layout and the readout fields of the push block.  This class has the counts, the plan key, what the body asks a class for (the
native entry points, the rows of the planes, the names of two fields) and the batched finish.  The query preparation runs at open and per reset(slot),
always over all M guides into staging planes -- only the prepared slot's rows are copied into the planes a push reads (ClipStreamGroup's
rule: the kernels pick their instantiation by the row count, and a replay must be bit-equal to the first run).  Per plan, keyed by the
TUPLE of (Tc_i, Q_i) of the call: the workspace and the static device tables.  Per push, by value in the kernel arguments: every item's
first pair, frame offset and first output row.  A push is six launches; it allocates nothing, copies nothing to the device and never
synchronises.

finish_many is one launch sequence for any set of slots: hicom_global_combine_fwd over the whole state, the four hicom_linear_fwd of
finish_guides with M rows into work buffers allocated at open, one placement that writes the whole-clip newline rows and the 32 global
rows of the NAMED slots' pairs.  Rows of slots that are not named, or empty, are computed (an empty state gives NaN) and never placed;
every launch is row-wise, so they reach no other row.  finish(slot) is finish_many([slot]): a slot's result does not depend on which
other slots are finished with it.

Scope: that of open_stream_group."""
from __future__ import annotations

import operator

import torch

from . import clip_stream as cs
from . import clip_stream_group as csg
from . import native as nv

STORE_GROUP_MULTI = "_clip_stream_group_multi_plans"
MAX_SLOTS = MAX_GUIDES = nv.GROUP_MAX


class _SlotGuides:
    """What stream_scope is told when reset(slot, guides) checks ONE slot's new guides: the [Q, E] block of a multi-guide stream."""
    WHAT, RECIPE, MULTI = "ClipStreamGroupMulti.reset", "plain", True


def check_counts(what, guide_counts):
    """The B guide counts as a tuple of ints; ValueError unless 1 <= B <= 32 and 1 <= Q_s <= 32."""
    try:                                         # (anything with __index__: Python, numpy and torch integers; no bools, no floats)
        counts = tuple(guide_counts)
        counts = None if any(isinstance(q, bool) for q in counts) else tuple(operator.index(q) for q in counts)
    except TypeError:
        counts = None
    if counts is None:
        raise ValueError(f"{what}: guide_counts is the list of the B ints Q_s, one per slot (got {guide_counts!r})")
    if not 1 <= len(counts) <= MAX_SLOTS:
        raise ValueError(f"{what}: B={len(counts)} slots (1 <= B <= {MAX_SLOTS} per group)")
    for s, q in enumerate(counts):
        if not 1 <= q <= MAX_GUIDES:
            raise ValueError(f"{what}: slot {s}: Q={q} guides (1 <= Q <= {MAX_GUIDES} per slot)")
    return counts


class ClipStreamGroupMulti(csg.ClipStreamGroup):
    """The object HIComProjector.open_stream_group_multi returns (module docstring).  `frames` and `has_fe` are per-slot lists; `out` is
    [M, cap_rows + 32, hidden], pair-major; `guides` the [M, E] block; `pair0[s]` the first pair of slot s."""
    NAME, WHAT, STORE = "ClipStreamGroupMulti", "open_stream_group_multi", STORE_GROUP_MULTI
    PAIRS, STRIDE, ROWS = True, "pair_stride", "pair_rows"
    SLOT_GUIDES = _SlotGuides                    # what reset(slot, guides) tells stream_scope: the entry's name and the class's recipe
    NO_LOGITS = None                             # push(local_logits=) is built for this class

    def __init__(self, proj, guide_embeds, guide_counts, H, W, max_frames, image_newline=None):
        # the open sequence is ClipStreamBase's (scope, allocate, prepare); _scope takes the counts from here and sets B (the slots, what
        # ClipStreamGroup's checks read), M (the pairs; the base's Q, the guide rows, equals it) and pair0
        self._counts_arg = guide_counts
        super().__init__(proj, guide_embeds, H, W, max_frames, image_newline)
        del self._counts_arg
        assert self.Q == self.M

    def _scope(self, proj, guide_embeds, H, W, max_frames, image_newline):
        """stream_scope on the guide block (its count is checked per slot here, not per call) and the counts: (E, kt, ks, hidden, heads)."""
        what = self.WHAT
        probe = guide_embeds[:1] if isinstance(guide_embeds, torch.Tensor) and guide_embeds.ndim == 2 and guide_embeds.shape[0] else guide_embeds
        dims = cs.stream_scope(proj, probe, H, W, max_frames, image_newline, type(self))
        self._chunk_limits(self.WHAT, proj, dims[1], H, W, dims[0])
        counts = check_counts(what, self._counts_arg)
        if guide_embeds.shape[0] != sum(counts):
            raise ValueError(f"{what}: guide_embeds has {guide_embeds.shape[0]} rows, guide_counts {list(counts)} add up to {sum(counts)} "
                             "(the guides of slot s are the rows [sum of the counts in front of s, + Q_s))")
        self.guide_counts, self.B, self.M = counts, len(counts), sum(counts)
        self.pair0 = [sum(counts[:s]) for s in range(self.B)]
        return dims

    def _plan_key(self, tcqs, has_fe, stream):
        """The tuple of (Tc_i, Q_i) and the base's fields, with the slots B where the base has its guide count.  Not M: a plan holds the
        workspace and the tables of the tuple, and everything that belongs to a group -- B and M among it -- is set per push (_launch),
        so groups of one module with other guide counts share plans."""
        return (self.B, tcqs, self.H, self.W, self.E, has_fe, None if self.newline is None else tuple(self.newline.shape), self.out_dtype, stream)

    # -- what the class says of itself; the device work and push are ClipStreamGroup's -------------------------------------------------------
    def _native(self):
        return (nv.StreamGroupMultiPushArgs, nv.compressor_stream_group_multi_workspace, nv.compressor_stream_group_multi_prepare,
                nv.compressor_stream_group_multi_push)

    def _row_shapes(self, M, nh):
        return (M * nh,), (M * nh + 31) // 32 * 32       # whole 32-row passes, as the ragged multi-guide step pads its planes

    def _push_logits(self, args, local_logits, tokens, q_max):
        """The logits form of the native push: the same block, workspace and tables, launch 1 on the tick's logits."""
        q_stride = cs.logits_stride(f"{self.NAME}.push", local_logits, q_max, tokens)
        nv.compressor_stream_group_multi_push_logits(args, local_logits.data_ptr(), q_stride)

    def head_scores(self, last_hidden_state, head, split_sizes, slots=None, hidden_act=None):
        """fp32 [max Q over the tick's slots, sum Tc_i, H, W]: what push(frames_feature, None, split_sizes, slots, local_logits=) takes for the
        same split_sizes and slots -- siglip_head_scores_ragged with the guides of the tick's slots gathered item after item (the order of
        `slots`, not of the group) and those slots' guide counts.  U and c are folded from the live weights on every call: nothing is kept."""
        from .encoder import siglip_head_scores_ragged
        what = f"{self.NAME}.head_scores"
        tcs = tuple(int(n) for n in split_sizes)
        slots = tuple(range(self.B)) if slots is None and len(tcs) == self.B else slots
        if slots is None or len(slots) != len(tcs):
            raise ValueError(f"{what}: slots names the slot of each of the {len(tcs)} items (the default is range(B) for B = {self.B} items)")
        slots = tuple(self._slot(what, s) for s in slots)
        guides = torch.cat([self.guides[self._pairs(s)] for s in slots])
        return siglip_head_scores_ragged(last_hidden_state, head, guides, tcs, [self.guide_counts[s] for s in slots], hidden_act)

    def _allocate(self, rows):
        super()._allocate(rows)
        M, E, gc = self.M, self.E, self.proj.global_compressor
        # finish_many: the combined contexts and the global tail with M rows
        self.fin = tuple(torch.empty(shape, dtype=torch.float32, device=self.device)
                         for shape in ((M * self.nh, E), (M, E), (M, E), (M, gc.readout[0].out_features), (M, gc.readout[2].out_features)))

    def finish_many(self, slots=None):
        """{slot: [Q_s, local rows of the slot so far + 32, hidden]} for the slots named (default: every slot that holds frames), in ONE
        launch sequence whatever the set is (module docstring).  Views of the output storage; the state is not consumed."""
        from .projector import _refuse_grad
        what = f"{self.NAME}.finish_many"
        if slots is None:
            slots = [s for s in range(self.B) if self.frames[s]]
            if not slots:
                raise ValueError(f"{what}: nothing has been pushed into any slot")
        else:
            slots = [self._slot(what, s) for s in slots]
            if not slots or len(set(slots)) != len(slots):
                raise ValueError(f"{what}: slots {list(slots)}: a non-empty list of distinct slots")
            for s in slots:
                if self.frames[s] == 0:
                    raise ValueError(f"{what}: nothing has been pushed into slot {s}")
        _refuse_grad(self.proj, what)
        row0s, ends, tails = [0] * self.B, {}, set()
        for s in slots:
            row0, lay = cs.prefix_layout(self.proj, self.frames[s] // self.kt, self.gh, self.gw, self.newline is not None)
            row0s[s], ends[s] = row0, lay.n_rows + self.n_global
            tails.add(lay.n_rows - row0)
        if len(tails) != 1:                      # the whole-clip newline rows follow the packing mode, not the frame count: one value for the launch
            raise RuntimeError(f"{what}: the slots disagree on the whole-clip newline rows ({sorted(tails)})")
        self._finish_device(slots, row0s, tails.pop())
        return {s: self.out[self._pairs(s), :ends[s]] for s in slots}

    def _finish_device(self, slots, row0s, tail):
        nh = self.nh
        tok = self.proj.global_compressor.finish_guides(self.state_ml.view(1, self.M * nh, 2), self.state_acc.view(1, self.M * nh, self.E), self.guides,
                                                        self.fin)
        nv.stream_group_place_global(tok, self.newline, self.guide_counts, row0s, slots, tail, self.n_global, self.out)

    def finish(self, slot):
        """[Q_s, local rows of `slot` so far + 32, hidden]: finish_many([slot])."""
        what = f"{self.NAME}.finish"
        slot = self._slot(what, slot)
        if self.frames[slot] == 0:
            raise ValueError(f"{what}: nothing has been pushed into slot {slot}")
        return self.finish_many([slot])[slot]

    def reset(self, slot, guides=None):
        """A new clip in `slot` on the same buffers, with the same or new guides (bf16 [Q_s, E]: the count of a slot is fixed at open): the
        slot's query rows are prepared again and its pairs' states are emptied on the caller's stream.  The other slots are not touched."""
        from .projector import _refuse_grad
        what = f"{self.NAME}.reset"
        slot = self._slot(what, slot)
        if guides is not None:
            cs.stream_scope(self.proj, guides, self.H, self.W, self.max_frames, self.newline, self.SLOT_GUIDES)
            if guides.shape[0] != self.guide_counts[slot]:
                raise ValueError(f"{what}: {guides.shape[0]} guides for slot {slot}, which was opened with Q={self.guide_counts[slot]} (the buffers are "
                                 "sized by the counts: open another group)")
            cs._require_bf16_cuda("guide_embeds", guides)
        _refuse_grad(self.proj, what)
        self.frames[slot], self.has_fe[slot], self.has_logits[slot] = 0, None, None
        self._prepare(guides, slot)
