"""HIComProjector.open_stream_group: B live videos, each with its own guide, pushed in ONE call per tick (csrc/clip_stream_group.hip,
DESIGN.md §3.15).

A server that follows B videos gets one stacked [sum Tc_i, H, W, E] tensor per tick from its vision tower -- the tensor forward_ragged
reads in place.  A loop of B ClipStream.push calls costs B launch sequences; a group push is six launches whatever B and the mix of chunk
lengths are:

    g = proj.open_stream_group(guide_embeds[B, E], H, W, max_frames, image_newline)       # 1 <= B <= 32 slots, one guide per slot
    views = g.push(frames_feature[sum Tc, H, W, E], frames_embed or None, split_sizes, slots=None)
    out_i = g.finish(slot)                # [local rows of the slot so far + 32, hidden]; the state is not consumed
    g.reset(slot, guide=None)             # a new clip (and optionally a new guide) in that slot; the other slots untouched
    g.frames[slot], g.rows(slot)

`slots` names the slot of every item of the push (default: range(B) when there are B items): any non-empty subset in any order, a slot at
most once -- its state is updated in place by the one workgroup that owns the row.  A slot that is absent from a push is not touched.
finish(slot) is ClipStream.finish's contract per slot: forward() on the concatenation of everything pushed into the slot with the slot's
guide, to the kernels' rounding.

Who holds what.  ClipStreamBase has the open sequence, the scope (stream_scope), the chunk checks (_check_chunk, with the slot's counters),
the layout (prefix_layout, chunk_rows), the plan key and store (cached_plan with a store of its own) and the readout fields of the push
block (_fill_common); this class has per-slot counters in the place of the base's single ones and the device side.  The device side is
written pair-major, for slots of several guides (clip_stream_group_multi.py: ClipStreamGroupMulti supplies only its native entry points,
its plane rows and field names); this class is its case guide_counts == (1,) * B, pair0 == range(B), M == B.  Per group, at open:
the output storage [B, cap_rows + 32, hidden], state_ml [B, nh, 2] and state_acc [B, nh, E] (slot s's slices are the ONE set
GlobalCompressor.finish reads), the slot-major query operands q_hi / q_lo [B nh, E] and pos_a [B nh, P], the positional tables for
max_frames.  The query preparation (hicom_linear_fwd + hicom_fold_query_split_fwd) runs at open and per reset(slot) -- then only that
slot's rows are replaced -- never per push.  Per plan, keyed by the TUPLE of chunk lengths of the call: the workspace and the static device tables
(uploaded once).  Per push, by value in the kernel arguments: every item's slot, frame offset and first output row -- so B streams pushing
equal chunks every tick build one plan, and a push allocates nothing, copies nothing to the device and never synchronises.

Scope: that of open_stream (the plain release recipe, a bf16 module with bf16 CUDA inputs, H % ks == W % ks == 0, windows of <= 64
tokens, E == 1152, hidden % 64 == 0, the packing modes ClipStream takes, inference only) with 1 <= B <= 32 slots and the merge's LDS
limit on a chunk."""
from __future__ import annotations

import torch

from . import clip_stream as cs
from . import native as nv
from . import segments as seg

STORE_GROUP = "_clip_stream_group_plans"
MAX_SLOTS = nv.GROUP_MAX


class _SlotGuide:
    """What stream_scope is told when reset(slot, guide) checks ONE slot's new guide: the [E] row of a single stream."""
    WHAT, RECIPE, MULTI = "ClipStreamGroup.reset", "plain", False


class ClipStreamGroup(cs.ClipStreamBase):
    """The object HIComProjector.open_stream_group returns (module docstring).  `frames` and `has_fe` are per-slot lists; `out` is
    [B, cap_rows + 32, hidden]; `guides` the [B, E] block, one row per slot."""
    NAME, WHAT, STORE = "ClipStreamGroup", "open_stream_group", STORE_GROUP
    MULTI, GUIDE = True, "guide_embeds"          # the guides come as one [sum Q_s, E] block: Q of the base is M, the pairs
    PAIRS = False                                # the push block has M, q and pair0 (ClipStreamGroupMulti); here a slot is its one pair
    STRIDE, ROWS = "slot_stride", "slot_rows"    # the push block's fields for the output's stride and rows per slot / pair
    NO_LOGITS = ("local_logits has no form on the group of one guide per slot (its local stage is fused into a kernel of its own); open the group "
                 "with open_stream_group_multi(guide_counts=(1,) * B), which takes them")

    def __init__(self, proj, guide_embeds, H, W, max_frames, image_newline=None):
        super().__init__(proj, guide_embeds, H, W, max_frames, image_newline)
        if not self.PAIRS:
            self.B = self.M = self.Q
            self.guide_counts, self.pair0 = (1,) * self.B, list(range(self.B))
        self.frames = [0] * self.B
        self.has_fe = [None] * self.B            # per slot, decided by the slot's first push; every chunk of a clip agrees
        self.has_logits = [None] * self.B        # per slot: the clip's chunks come with local_logits (has_fe is then False)
        self._spans = {}

    def _chunk_limits(self, what, proj, Tc, H, W, E):
        if proj.global_compressor.use_pos_emb and (Tc * (H + W) + Tc + H + W) * 4 > 48 * 1024:
            raise NotImplementedError(f"{what}: Tc={Tc} frames of {H}x{W}: the merge keeps Tc (H + W) marginal sums in LDS; push shorter chunks")

    # -- what the two classes say of themselves ------------------------------------------------------------------------------------------
    def _native(self):
        """(the push block's class, workspace_bytes, prepare, push) of `nv` as the class's module sees it."""
        return nv.StreamGroupPushArgs, nv.compressor_stream_group_workspace, nv.compressor_stream_group_prepare, nv.compressor_stream_group_push

    def _row_shapes(self, M, nh):
        """(the leading dimensions of state_ml / state_acc, the rows of the query planes) for M pairs."""
        return (M, nh), M * nh

    # -- device work, pair-major: pair p = pair0[slot] + q owns out[p], the state rows and the query rows [p nh, (p + 1) nh) ---------------------
    def _allocate(self, rows):
        dev, E, M, nh, gc = self.device, self.E, self.Q, self.nh, self.proj.global_compressor
        state, RP = self._row_shapes(M, nh)

        def f32(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)
        self.out = torch.empty((M, rows, self.hidden), dtype=self.out_dtype, device=dev)
        self.state_ml, self.state_acc = f32(*state, 2), f32(*state, E)         # in place: one workgroup owns a row, no ping-pong
        self.qp = f32(M, E)
        self.q_hi = torch.zeros((RP, E), dtype=torch.bfloat16, device=dev)     # (rows >= M nh stay zero)
        self.q_lo = torch.zeros_like(self.q_hi)
        self.pos_a = self.pe = self.kpe = None
        self.P = self.y0 = self.x0 = 0
        if gc.use_pos_emb:
            # sized for max_frames: the y / x table offsets (cap, cap + H) never move while the group lives; one set for all slots
            self.pe, self.kpe, cap = gc.pos_and_kpe(self.max_frames, self.H, self.W, dev)
            self.P, self.y0, self.x0 = self.pe.shape[0], cap, cap + self.H
            self.pos_a = torch.zeros((RP, self.P), dtype=torch.float32, device=dev)
        # staging planes of the query preparation (_prepare)
        self.stage = (torch.zeros_like(self.q_hi), torch.zeros_like(self.q_hi), None if self.pos_a is None else torch.zeros_like(self.pos_a))

    def _pairs(self, slot):
        return slice(self.pair0[slot], self.pair0[slot] + self.guide_counts[slot])

    def _prepare(self, guides, slot=None):
        """Everything that depends on the guides alone, for every slot (open) or for `slot`'s pairs only (reset): q_proj, the fold into the
        query planes and the score-side positional table, the empty state."""
        from .projector import _linear_params
        gc = self.proj.global_compressor
        att, nh = gc.attn_layer, self.nh
        if slot is None:
            self.guides = guides.contiguous().clone()                          # the group's own block: reset(slot, guides) writes rows
            pairs = slice(0, self.Q)
        else:
            pairs = self._pairs(slot)
            if guides is not None:
                self.guides[pairs].copy_(guides)
        wq, bq = _linear_params(att.q_proj)
        wk, _ = _linear_params(att.k_proj)
        if gc.use_pos_emb:
            gc.pos_and_kpe(self.max_frames, self.H, self.W, self.device)       # (follows k_proj.weight in place)
        # The launch pair always runs over all M guides, into staging planes: both kernels choose their instantiation by the row count
        # (one row takes another path and rounds differently), and a replay behind reset(slot) must be bit-equal to the slot's first
        # run.  Only the rows of the pairs being prepared are copied into the planes a push reads: the other slots keep theirs.
        hi, lo, pos = self.stage
        nv.linear(self.guides, wq, bq, self.qp)
        nv.fold_query_split(self.qp, wk, self.kpe, nh, att.scale, hi, lo, pos)
        rows = slice(pairs.start * nh, pairs.stop * nh)
        self.q_hi[rows].copy_(hi[rows])
        self.q_lo[rows].copy_(lo[rows])
        if pos is not None:
            self.pos_a[rows].copy_(pos[rows])
        nv.stream_state_clear(self.state_ml.view(-1, 2)[rows], self.state_acc.view(-1, self.E)[rows])

    def _build_plan(self, items, has_fe, stream=None):
        """The plan of one tuple of chunk lengths (PAIRS: of (chunk length, guide count)): the block with everything but the per-push fields,
        the workspace and its static tables."""
        Args, workspace, prepare, _ = self._native()
        args = Args()
        a = getattr(args, "base", args)              # (the block of the k / v adaptor recipe has the plain block first: clip_stream_group_adapt.py)
        a.B, a.items, a.H, a.W, a.E, a.kt, a.ks, a.nh, a.hidden, a.chunks = self.B, len(items), self.H, self.W, self.E, self.kt, self.ks, self.nh, self.hidden, 0
        a.out_dt = nv.DT_F32 if self.out_dtype == torch.float32 else nv.DT_BF16
        a.nl_group = self.proj._layout((self.max_frames // self.kt, self.gh, self.gw), "video", self.newline is not None, False).nl_group
        if self.PAIRS:
            a.M, a.q[:len(items)], items = self.M, [q for _, q in items], [n for n, _ in items]
        a.tc[:len(items)] = items
        more, refresh = self._fill_front(args)
        ws, (a.ws,), keep = self._fill_common(a, max(items), 0, [workspace(args)])
        a.ws_bytes, a.stream = ws.numel(), stream
        prepare(args)
        return cs.StreamPlan(args, ws, keep + more, refresh)

    def _fill_front(self, args):
        """Hook: what the block has beyond the plain fields, entered in front of the workspace query: (the tensors those fields point at, the
        plan's refresh).  Here nothing, and the plan follows the readout weights."""
        return [], self.proj.local_compressor.readout_f16

    def _launch(self, plan, ff, fe, slots, t0s, row0s, stream, local_logits=None):
        a = getattr(plan.args, "base", plan.args)
        a.B = self.B                             # of THIS group, as M and pair0: plans are shared by the groups of a module, and the C checks use them
        a.ff, a.fe, a.guide = ff.data_ptr(), (fe.data_ptr() if fe is not None else None), self.guides.data_ptr()
        a.q_hi, a.q_lo = self.q_hi.data_ptr(), self.q_lo.data_ptr()
        a.pos_a = self.pos_a.data_ptr() if self.pos_a is not None else None
        a.pe = self.pe.data_ptr() if self.pe is not None else None
        a.P, a.y_index0, a.x_index0 = self.P, self.y0, self.x0
        a.state_ml, a.state_acc = self.state_ml.data_ptr(), self.state_acc.data_ptr()
        a.out = self.out.data_ptr()
        setattr(a, self.STRIDE, self.out.stride(0))
        setattr(a, self.ROWS, self.out.shape[1])
        a.newline = self.newline.data_ptr() if (self.newline is not None and a.nl_group) else None
        for i, (s, t0, row0) in enumerate(zip(slots, t0s, row0s)):
            a.slot[i], a.t0[i], a.row0[i] = s, t0, row0
        if self.PAIRS:
            a.M, a.pair0[:len(slots)] = self.M, [self.pair0[s] for s in slots]
        a.stream = stream
        if local_logits is None:
            self._native()[3](plan.args)
        else:
            self._push_logits(plan.args, local_logits, ff.shape[0] * self.H * self.W, max(self.guide_counts[s] for s in slots))

    # -- the public surface ---------------------------------------------------------------------------------------------------------------
    def _slot(self, what, slot):
        if not isinstance(slot, int) or isinstance(slot, bool) or not 0 <= slot < self.B:
            raise ValueError(f"{what}: slot {slot!r} (0 <= slot < B = {self.B})")
        return slot

    def rows(self, slot):
        """Local rows of the frames pushed into `slot` so far, as forward() on them would lay them out."""
        slot = self._slot(f"{self.NAME}.rows", slot)
        return self.proj._layout((self.frames[slot] // self.kt, self.gh, self.gw), "video", self.newline is not None, False).n_rows

    def _check_logits(self, what, ll, fe, Tc):
        """(the base's per-chunk hook: a group checks the logits of the whole stack once, in _check_stack_logits)"""

    def _check_stack_logits(self, what, ll, fe, ff, slots):
        """The refusals of local_logits for the stack of a tick: beside frames_embed, shape, dtype, device, autograd, layout."""
        if fe is not None:
            raise ValueError(f"{what}: local_logits replaces frames_embed: pass frames_embed=None")
        want = (max(self.guide_counts[s] for s in slots),) + tuple(ff.shape[:3])
        if not isinstance(ll, torch.Tensor) or tuple(ll.shape) != want:
            raise ValueError(f"{what}: local_logits is [max Q over the tick's slots, sum Tc, H, W] = [{', '.join(map(str, want))}], plane q holding guide "
                             f"q of every item's slot on the item's frames (got {tuple(ll.shape) if isinstance(ll, torch.Tensor) else None})")
        cs._require_f32_cuda("local_logits", ll)
        if ll.requires_grad:
            raise RuntimeError(f"{what} builds no autograd graph: local_logits requires grad (compute it under torch.no_grad())")
        cs.logits_stride(what, ll, want[0], ff.shape[0] * self.H * self.W)

    def _check_push(self, ff, fe, split_sizes, slots, ll=None):
        """Every refusal of a push, in front of any device work: (chunk lengths, slots).  ll: the tick's local_logits, or None."""
        what = f"{self.NAME}.push"
        if isinstance(ff, dict) or isinstance(fe, dict):
            raise NotImplementedError(f"{what}: anyres dict inputs have no clip-stream path (call forward() per image)")
        if not isinstance(ff, torch.Tensor) or ff.ndim != 4:
            raise ValueError(f"{what}: frames_feature is [sum Tc, H, W, E], the stacked chunks of the call")
        tcs = tuple(int(n) for n in split_sizes)
        if not 1 <= len(tcs) <= self.B:
            raise ValueError(f"{what}: {len(tcs)} items (1 .. B = {self.B}: a slot appears at most once per push)")
        slots = tuple(range(self.B)) if slots is None and len(tcs) == self.B else slots
        if slots is None or len(slots) != len(tcs):
            raise ValueError(f"{what}: slots names the slot of each of the {len(tcs)} items (the default is range(B) for B = {self.B} items)")
        slots = tuple(self._slot(what, s) for s in slots)
        if len(set(slots)) != len(slots):
            raise ValueError(f"{what}: slots {list(slots)}: a slot appears at most once per push (its state is updated in place)")
        if sum(tcs) != ff.shape[0]:
            raise ValueError(f"{what}: split_sizes {list(tcs)} add up to {sum(tcs)} frames, frames_feature has {ff.shape[0]}")
        if fe is not None and (not isinstance(fe, torch.Tensor) or tuple(fe.shape) != tuple(ff.shape)):
            raise ValueError(f"{what}: frames_embed {tuple(getattr(fe, 'shape', ()))} vs frames_feature {tuple(ff.shape)}")
        if ll is not None:
            self._check_stack_logits(what, ll, fe, ff, slots)
        # the base's chunk check per item, with the slot's counters; items that agree in length and counters (B streams in lock step) are
        # slices of one stack and share one check
        t, seen = 0, set()
        for n, s in zip(tcs, slots):
            case = (n, self.frames[s], self.has_fe[s], self.has_logits[s])
            if case not in seen:
                seen.add(case)
                self._check_chunk(ff[t:t + max(n, 0)], None if fe is None else fe[t:t + max(n, 0)], case[1:], ll)
            t += n
        return tcs, slots

    def _span(self, frames, Tc):
        """chunk_rows of a chunk of Tc frames behind `frames`: (row0, nl_group, newline rows, the row behind it); a function of the pair."""
        hit = self._spans.get((frames, Tc))
        if hit is None:
            hit = self._spans[(frames, Tc)] = cs.chunk_rows(self.proj, frames // self.kt, Tc // self.kt, self.gh, self.gw, self.newline is not None)
        return hit

    def push(self, frames_feature, frames_embed=None, split_sizes=(), slots=None, local_logits=None):
        """The next chunks of the slots named: frames_feature bf16 [sum Tc_i, H, W, E] (frames_embed None: the keys are frames_feature; all or
        none within a call), split_sizes the chunk lengths Tc_i (positive multiples of kt), slots the slot of each item (module docstring).
        local_logits (ClipStreamGroupMulti only; frames_embed None): fp32 [max Q over the tick's slots, sum Tc_i, H, W] from
        head_scores for the same split_sizes and slots; a slot's clip keeps one of the three forms.
        Returns one view per item: that chunk's local rows ([chunk rows, hidden]; PAIRS: of every guide of the slot, [Q_slot, chunk rows,
        hidden]) in their final place in the output storage, complete on the caller's stream; the stack is not referenced afterwards."""
        if local_logits is None:
            tcs, slots = self._check_push(frames_feature, frames_embed, split_sizes, slots)
        elif self.NO_LOGITS:
            raise NotImplementedError(f"{self.NAME}.push: {self.NO_LOGITS}")
        else:
            tcs, slots = self._check_push(frames_feature, frames_embed, split_sizes, slots, local_logits)
        ff = frames_feature.contiguous()
        fe = frames_embed.contiguous() if frames_embed is not None else None
        stream = torch.cuda.current_stream(self.device).cuda_stream
        # what an item gives the plan key: its length and, PAIRS, its guide count, which decides its work units
        items = tuple((n, self.guide_counts[s]) for n, s in zip(tcs, slots)) if self.PAIRS else tcs
        key = self._plan_key(items, fe is not None, stream) + (cs.LOGITS_KEY if local_logits is not None else ())
        plan = seg.cached_plan(self.proj, self.STORE, key, lambda: self._build_plan(items, fe is not None, stream))
        spans = [self._span(self.frames[s], n) for n, s in zip(tcs, slots)]
        if local_logits is None:                  # (the keyed call as it always was: a class outside the feature may keep _launch's old signature)
            self._launch(plan, ff, fe, slots, [self.frames[s] for s in slots], [sp[0] for sp in spans], stream)
        else:
            self._launch(plan, ff, fe, slots, [self.frames[s] for s in slots], [sp[0] for sp in spans], stream, local_logits=local_logits)
        for n, s in zip(tcs, slots):
            self.frames[s] += n
            self.has_fe[s], self.has_logits[s] = fe is not None, local_logits is not None
        self.n_pushes += 1
        return [self.out[self._pairs(s) if self.PAIRS else s, sp[0]:sp[3]] for s, sp in zip(slots, spans)]

    def finish(self, slot):
        """[local rows of `slot` so far + 32, hidden]: the rows that depend on the whole clip (a `one_token` newline row, the 32 global rows)
        written behind the slot's local rows.  A view of the slot's part of the output storage; the state is not consumed."""
        from .projector import _refuse_grad
        slot = self._slot(f"{self.NAME}.finish", slot)
        if self.frames[slot] == 0:
            raise ValueError(f"{self.NAME}.finish: nothing has been pushed into slot {slot}")
        _refuse_grad(self.proj, f"{self.NAME}.finish")
        row0, lay = cs.prefix_layout(self.proj, self.frames[slot] // self.kt, self.gh, self.gw, self.newline is not None)
        tail = lay.n_rows - row0
        out = self.out[slot]
        if tail:                                                                           # whole-clip newline rows (`one_token`)
            nv.scatter_rows(self.newline.view(1, -1), out, row0, tail)
        self.proj.global_compressor.finish(self.state_ml[slot:slot + 1], self.state_acc[slot:slot + 1], self.guides[slot:slot + 1], out, row0 + tail,
                                           self.n_global)
        return out[:lay.n_rows + self.n_global]

    def reset(self, slot, guide=None):
        """A new clip in `slot` on the same buffers, with the same or a new guide (bf16 [E]): the slot's query rows are prepared again (they
        follow the weights) and its state is emptied on the caller's stream.  The other slots are not touched."""
        from .projector import _refuse_grad
        what = f"{self.NAME}.reset"
        slot = self._slot(what, slot)
        if guide is not None:
            cs.stream_scope(self.proj, guide, self.H, self.W, self.max_frames, self.newline, _SlotGuide)
            cs._require_bf16_cuda("guide_embed", guide)
        _refuse_grad(self.proj, what)
        self.frames[slot], self.has_fe[slot], self.has_logits[slot] = 0, None, None
        self._prepare(guide, slot)
