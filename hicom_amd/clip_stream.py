"""HIComProjector.open_stream: ONE video that arrives in chunks, compressed as it arrives (csrc/clip_stream.hip).

The vision tower runs over a few frames at a time; forward() and every many-item step want the whole [T, H, W, E] pair resident before
the first launch.  A ClipStream takes the guide up front and the frames in pieces of whole window groups (Tc % kt == 0):

    s = proj.open_stream(guide_embed, H, W, max_frames, image_newline)
    rows = s.push(frames_feature[Tc, H, W, E], frames_embed or None)      # any number of times; the chunk may be freed afterwards
    out = s.finish()                                                      # [local rows so far + 32, hidden]

Why it is exact (hicom_amd/dist.py has the same split over GPUs): local windows never straddle a group of kt frames, so a chunk's local rows
are final when the chunk has been read; the global softmax state (M, L, ACC[rows, E]) of disjoint frame ranges merges exactly when the
positional terms use absolute frame numbers, and the positional tables are indexed by absolute frame (sized for max_frames at open, so the
y / x offsets never move); in `direct` mode both stages' queries are the guide, so nothing depends on the final T.

One push is one host call (hicom_compressor_stream_push): the fused ring kernel on the chunk with t_index0 = frames pushed so far, the fold of
its partials into the carried state (hicom_stream_state_fold_fwd), the two readout GEMMs writing the chunk's rows at their packed offset in the
stream's output buffer (+ the chunk's `grid` / `frame` newline rows).  finish() runs GlobalCompressor.finish on the carried state as one set
and does not consume it: more pushes and another finish() give the longer clip's result.

Nothing token-sized is allocated: the output buffer (for max_frames), the state, the query operands and the positional tables at open; the
per-chunk workspace (partials, the fp16 context and hidden planes of ONE chunk) with the plan, on first use of a chunk length.  Plans are cached
on the module (`proj._clip_stream_plans`) per (Q, Tc, H, W, E, has frames_embed, newline, out dtype, stream) through segments.cached_plan; the
frame offset, the row offset and everything that belongs to a stream (queries, tables, state, output) are patched per push, so a stream of
equal chunks builds one plan and two streams of one module share it.  Everything runs on the caller's current stream.

Scope: that of forward_multi_guide (the plain release recipe, a bf16 module with bf16 CUDA inputs, inference only) on the geometry the fused
ring kernel takes (H % ks == W % ks == 0, 16 <= kt ks ks <= 64, E == 1152, at most 12 folded rows, hidden % 64 == 0).

HIComProjector.open_stream_multi (ClipStreamMulti) is the same stream for Q guides known up front: every chunk is read once
for all of them.  HIComProjector.open_stream_adapt (ClipStreamAdapt, at the end of this file) is that stream for the
k / v adaptor recipe: the adaptor MLPs run once per chunk for all Q guides.

Who holds what: ClipStreamBase has the host side of all three once -- the open sequence, the chunk checks, push, finish, reset, `rows`,
the plan key and store, and the fields of the push block that every native push takes (_fill_common per plan, _patch_common per push).
A class names itself (NAME, WHAT, STORE, RECIPE, RECIPE_WORDS, MULTI, GUIDE) and holds its device side: _allocate, _prepare, _build_plan,
_launch, _finish_device, and the limits of a chunk (_chunk_limits)."""
from __future__ import annotations

import math

import torch

from . import native as nv
from . import segments as seg

STORE = "_clip_stream_plans"
STORE_MULTI = "_clip_stream_multi_plans"
STORE_ADAPT = "_clip_stream_adapt_plans"
MAX_PARTS = 256                                  # token chunks of the many-row global stream (csrc/clip_stream.hip: kMaxStreamParts)


def _require_bf16_cuda(name, t):
    from .projector import _require_bf16_cuda as check
    check(name, t)


def _require_f32_cuda(name, t):
    from .multi_guide import _require_f32_cuda as check
    check(name, t)


LOGITS_KEY = ("logits",)                         # what the plan key of a logits push has behind the keyed push's fields
NOT_LINEAR = ("local_logits has no form on the k / v adaptor recipe: the keys pass an MLP and a LayerNorm blend in front of the score, so it is "
              "not linear in frames_embed; push frames_embed")


def logits_stride(what, ll, planes, tokens):
    """The leading stride of local_logits [planes, ...tokens] as q_stride, behind the check that the planes are contiguous and `tokens`
    floats or more apart (one plane: its stride is never used)."""
    if not ll[0].is_contiguous():
        raise ValueError(f"{what}: local_logits must be contiguous in its last three dimensions [T, H, W] (the leading stride travels as q_stride)")
    if planes > 1 and ll.stride(0) < tokens:
        raise ValueError(f"{what}: local_logits: the guides' planes are {ll.stride(0)} floats apart, a plane holds {tokens}")
    return ll.stride(0) if planes > 1 else tokens


def prefix_layout(proj, groups, gh, gw, has_newline):
    """(row at which a chunk behind `groups` window groups starts, HIComProjector._layout of that prefix).  The rows of a prefix that depend
    on the whole clip -- the `one_token` newline row behind the last token: a layout with newline rows but no interleaving -- belong to
    finish(), so they do not count."""
    lay = proj._layout((groups, gh, gw), "video", has_newline, False)
    tail = len(lay.newline_rows) if lay.nl_group == 0 else 0
    return lay.n_rows - tail, lay


def chunk_rows(proj, groups0, groups, gh, gw, has_newline):
    """Where the chunk of `groups` window groups behind `groups0` lands: (row0, nl_group, its chunk-local newline rows as absolute rows, the
    row behind it).  All of it from _layout of the two prefixes."""
    row0, _ = prefix_layout(proj, groups0, gh, gw, has_newline)
    row1, lay = prefix_layout(proj, groups0 + groups, gh, gw, has_newline)
    newline = [r for r in lay.newline_rows if row0 <= r < row1] if lay.nl_group else []
    return row0, lay.nl_group, newline, row1


def stream_scope(proj, guide, H, W, max_frames, nl, cls=None):
    """Raises for everything outside the scope of a clip stream, in front of any device work; returns (E, kt, ks, hidden, heads).  cls: the
    stream class (None: ClipStream) -- its WHAT names the entry in the messages, MULTI says that the guide is the [Q, E] block of
    open_stream_multi, RECIPE is the segments.seg_recipe the entry is built for ("adaptkv": open_stream_adapt)."""
    cls = cls or ClipStream
    WHAT = cls.WHAT
    if seg.seg_recipe(proj) != cls.RECIPE:
        if cls.RECIPE == "adaptkv":
            raise NotImplementedError(f"{WHAT} is built for the two release recipes only (local + global compressor, use_guide='direct', no "
                                      "adaptors but adapt_k / adapt_v on the local stage, no clip scale); everything else goes through "
                                      "forward() on the whole clip")
        raise NotImplementedError(f"{WHAT} is built for the plain release recipe only (local + global compressor, use_guide='direct', no "
                                  "adaptors, no clip scale); everything else goes through forward() on the whole clip")
    lc, gc = proj.local_compressor, proj.global_compressor
    wdt = lc.readout[0].weight.dtype
    if wdt != torch.bfloat16:
        raise NotImplementedError(f"{WHAT}: a {wdt} projector; the clip stream takes a bfloat16 module and bfloat16 inputs")
    E, hidden, nh = gc.embed_dim, lc.readout[2].out_features, gc.attn_layer.num_heads
    if cls.MULTI:
        from .multi_guide import count_guides
        count_guides(WHAT, guide, E)
    elif not isinstance(guide, torch.Tensor) or tuple(guide.shape) != (E,):
        raise ValueError(f"{WHAT}: guide_embed is [E] = [{E}], the one instruction of the stream "
                         f"(got {tuple(guide.shape) if isinstance(guide, torch.Tensor) else None})")
    if guide.dtype != torch.bfloat16:
        raise NotImplementedError(f"{WHAT}: guide_embed dtype {guide.dtype}; the clip stream takes bfloat16 inputs")
    kt, ks = lc.temporal_kernel_size, lc.spatial_kernel_size
    if E != 1152 or nh > 12 or hidden % 64:
        raise NotImplementedError(f"{WHAT}: E={E}, {nh} heads, hidden={hidden} (the fused ring kernel takes E == 1152 and <= 12 folded rows, "
                                  "the fp16 readout planes hidden % 64 == 0)")
    if not all(isinstance(v, int) and v > 0 for v in (H, W, max_frames)):
        raise ValueError(f"{WHAT}: H, W and max_frames are positive ints (got {H}, {W}, {max_frames})")
    if H % ks or W % ks or not 16 <= kt * ks * ks <= 64:
        raise NotImplementedError(f"{WHAT}: the windows must partition the grid exactly, 16 .. 64 tokens each (H={H} W={W}, windows "
                                  f"{kt}x{ks}x{ks}); such clips go through forward()")
    if max_frames % kt:
        raise ValueError(f"{WHAT}: max_frames={max_frames} (a multiple of the temporal window, {kt} frames)")
    if nl is not None:
        if not isinstance(nl, torch.Tensor) or tuple(nl.shape) != (hidden,):
            raise ValueError(f"{WHAT}: image_newline is [hidden] = [{hidden}]")
        if nl.dtype != torch.bfloat16:
            raise NotImplementedError(f"{WHAT}: image_newline dtype {nl.dtype}; the clip stream takes bfloat16 inputs")
    proj._layout((max_frames // kt, H // ks, W // ks), "video", nl is not None, False)       # (ValueError: a packing that needs image_newline)
    return E, kt, ks, hidden, nh


def multi_chunk_limits(what, Tc, H, W, use_pos_emb):
    """The LDS limits of the merge kernels (csrc/merge.hip) applied to ONE chunk of Tc frames, with the largest number of token chunks a plan
    may choose: NotImplementedError in front of any device work (hicom_compressor_stream_push_multi checks the same with the plan's own)."""
    if not use_pos_emb:
        return
    if H + W > 1024 or not ((H <= 32 and W <= 32) or (H * W + H + 4) * 4 <= 60000):
        raise NotImplementedError(f"{what}: a {H}x{W} grid: the merge keeps a frame of logits in LDS")
    if (MAX_PARTS + 2 * Tc + H + W + 64 * (H + W + 2) + 16 * 64 + 4) * 4 > 60000:
        raise NotImplementedError(f"{what}: Tc={Tc} frames of {H}x{W}: the merge keeps the row's Tc + H + W weights and 64 frames of "
                                  "marginals in LDS; push shorter chunks")


def adaptor_widths(what, lc):
    """The width condition of segments.fill_adaptors, from the parameters' shapes alone: in front of any device work."""
    from . import engine
    for _, mlp, _, _ in engine.adaptor_streams(lc):
        w0, w2 = mlp[0].weight, mlp[2].weight
        if w0.shape[0] % 64 or w0.shape[1] % 64 or w2.shape[0] % 64 or w0.shape != w2.shape:
            raise NotImplementedError(f"{what}: adaptor widths must be multiples of 64")


def adapt_chunk_limit(what, Tc, H, W, E):
    """The operand limit of the adaptor MLPs' dense GEMMs on ONE chunk (hicom_clip_adapt_prepare_fwd checks the same)."""
    if Tc * H * W * E >= 1 << 32:
        raise NotImplementedError(f"{what}: Tc={Tc} frames of {H}x{W}: the adaptor GEMMs take operands below 2^32 elements; push shorter chunks")


class StreamPlan:
    """What one chunk shape needs: the argument block with the module's fields filled and the workspace of ONE chunk."""
    __slots__ = ("args", "ws", "sig", "fresh", "refresh", "hits", "keep")

    def __init__(self, args, ws, keep, refresh):
        self.args, self.ws, self.keep, self.refresh = args, ws, keep, refresh
        self.sig = self.fresh = None
        self.hits = 0


class ClipStreamBase:
    """The host side of the three clip streams (module docstring: who holds what).  Attributes: `frames` pushed so far, `rows` local rows so
    far (the whole-clip newline row of `one_token` included once finish() has written it), `out` the output buffer for `cap_rows` local
    rows + the global rows, `Q` guides (1: ClipStream), `guide` / `guides`, `n_pushes`, `has_fe`, `cur` (the (M, L) block a push reads)."""
    NAME = WHAT = STORE = None                       # what the messages call the object and the entry that opens it; the plan store
    RECIPE, RECIPE_WORDS = "plain", "the plain release recipe"       # segments.seg_recipe of the modules the stream takes
    MULTI, GUIDE = False, "guide_embed"              # the guide is [E] (kept as `guide`) / the [Q, E] block (`guides`); the argument's name
    NO_LOGITS = None                                 # why push(local_logits=) is refused by the class (None: it takes them)

    def __init__(self, proj, guide, H, W, max_frames, image_newline=None):
        from .projector import _out_dtype, _refuse_grad
        self.E, self.kt, self.ks, self.hidden, self.nh = self._scope(proj, guide, H, W, max_frames, image_newline)
        _refuse_grad(proj, f"HIComProjector.{self.WHAT}")
        _require_bf16_cuda(self.GUIDE, guide)
        if image_newline is not None:
            _require_bf16_cuda("image_newline", image_newline)
        self.proj, self.H, self.W, self.max_frames = proj, H, W, max_frames
        self.Q = guide.shape[0] if self.MULTI else 1
        self.gh, self.gw = H // self.ks, W // self.ks
        self.newline = None if image_newline is None else image_newline.contiguous()
        self.device, self.out_dtype = guide.device, _out_dtype(proj)
        self.has_fe = None                        # decided by the first push; every chunk of a clip agrees
        self.has_logits = None                    # the third form: the chunks come with local_logits (has_fe is then False)
        self.frames = 0
        self.n_pushes = 0
        self.cap_rows = proj._layout((max_frames // self.kt, self.gh, self.gw), "video", image_newline is not None, False).n_rows
        self.n_global = proj.global_compressor.num_queries
        self._allocate(self.cap_rows + self.n_global)
        self._prepare(guide)

    def _scope(self, proj, guide, H, W, max_frames, image_newline):
        """stream_scope of the class and the limits of the shortest chunk: (E, kt, ks, hidden, heads)."""
        dims = stream_scope(proj, guide, H, W, max_frames, image_newline, type(self))
        self._chunk_limits(self.WHAT, proj, dims[1], H, W, dims[0])
        return dims

    def _chunk_limits(self, what, proj, Tc, H, W, E):
        """Hook: NotImplementedError for a chunk of Tc frames that the class's kernels do not take (at open: the shortest chunk)."""

    def _plan_key(self, Tc, has_fe, stream):
        return (self.Q, Tc, self.H, self.W, self.E, has_fe, None if self.newline is None else tuple(self.newline.shape), self.out_dtype, stream)

    def _fill_common(self, a, Tc, nparts, sizes):
        """The fields that every push block has and the module and the chunk shape decide -- the geometry, the local scale, the readout
        and the output's form -- and the workspace of ONE chunk: regions of `sizes` bytes, each rounded up to 256.  Returns (workspace, the
        regions' addresses, the tensors the block points at)."""
        from .projector import _linear_params
        lc = self.proj.local_compressor
        offs, at = [], 0
        for n in sizes:
            offs.append(at)
            at += (n + 255) // 256 * 256
        ws = torch.empty((at,), dtype=torch.uint8, device=self.device)
        a.Tc, a.H, a.W, a.E, a.kt, a.ks, a.hidden, a.nparts = Tc, self.H, self.W, self.E, self.kt, self.ks, self.hidden, nparts
        a.l_scale = 1.0 / math.sqrt(lc.qk_dim)
        w0h, w2h = lc.readout_f16()
        b0, b2 = _linear_params(lc.readout[0])[1], _linear_params(lc.readout[2])[1]
        a.lw0_f16, a.lw2_f16, a.lb0, a.lb2 = w0h.data_ptr(), w2h.data_ptr(), b0.data_ptr(), b2.data_ptr()
        a.out_dt = nv.DT_F32 if self.out_dtype == torch.float32 else nv.DT_BF16
        a.ldo = self.hidden
        return ws, [ws.data_ptr() + o for o in offs], [w0h, w2h, b0, b2]

    def _patch_common(self, a, ff, fe, t0, row0, nl_group, newline_rows, stream):
        """What changes from push to push in every push block: the chunk, its frame and row offsets, its newline rows and what belongs to
        this stream (a plan serves every stream of the module)."""
        a.ff, a.fe, a.t0 = ff.data_ptr(), (fe.data_ptr() if fe is not None else None), t0
        a.q_hi, a.q_lo = self.q_hi.data_ptr(), self.q_lo.data_ptr()
        a.pos_a = self.pos_a.data_ptr() if self.pos_a is not None else None
        a.P, a.y_index0, a.x_index0 = self.P, self.y0, self.x0
        a.state_ml_in, a.state_ml_out = self.state_ml[self.cur].data_ptr(), self.state_ml[self.cur ^ 1].data_ptr()
        a.state_acc = self.state_acc.data_ptr()
        a.out, a.row0, a.nl_group = self.out.data_ptr(), row0, nl_group
        a.nl_count = len(newline_rows)
        a.newline = self.newline.data_ptr() if newline_rows else None
        # Plans are shared, so both fields are set on every push.  Without newline rows nothing reads them: hicom_compressor_stream_push
        # returns in front of hicom_scatter_rows_fwd and place_check / place_row stop at nl_count == 0.  With ONE row the step is
        # nl_group + 1, which place_check asks for; the scatter kernel multiplies it by the row's index, 0, and its check wants it > 0.
        a.nl_first, a.nl_step = 0, 1
        if newline_rows:
            a.nl_first = newline_rows[0]
            a.nl_step = newline_rows[1] - newline_rows[0] if len(newline_rows) > 1 else nl_group + 1
        a.stream = stream

    # -- the public surface ---------------------------------------------------------------------------------------------------------------
    @property
    def rows(self):
        """Local rows of the frames pushed so far, as forward() on them would lay them out."""
        return self.proj._layout((self.frames // self.kt, self.gh, self.gw), "video", self.newline is not None, False).n_rows

    def _check_logits(self, what, ll, fe, Tc):
        """The refusals of local_logits for one chunk of Tc frames: beside frames_embed, shape, dtype, device, autograd, layout."""
        if fe is not None:
            raise ValueError(f"{what}: local_logits replaces frames_embed: pass frames_embed=None")
        want = ((self.Q,) if self.MULTI else ()) + (Tc, self.H, self.W)
        if not isinstance(ll, torch.Tensor) or tuple(ll.shape) != want:
            raise ValueError(f"{what}: local_logits is {'[Q, Tc, H, W]' if self.MULTI else '[Tc, H, W]'} = [{', '.join(map(str, want))}], the raw dot "
                             f"products of the chunk's own tokens (got {tuple(ll.shape) if isinstance(ll, torch.Tensor) else None})")
        _require_f32_cuda("local_logits", ll)
        if ll.requires_grad:
            raise RuntimeError(f"{what} builds no autograd graph: local_logits requires grad (compute it under torch.no_grad())")
        logits_stride(what, ll if self.MULTI else ll.unsqueeze(0), self.Q, Tc * self.H * self.W)

    def _check_chunk(self, ff, fe, counters=None, ll=None):
        """The chunk against the stream's scope and the clip's counters, in front of any device work; returns Tc.  counters: the (frames,
        has_fe, has_logits) triple the chunk continues (None: the stream's own; a ClipStreamGroup passes those of the chunk's slot).  ll: the
        chunk's local_logits, or None."""
        from .projector import _refuse_grad
        what, WHAT = f"{self.NAME}.push", self.WHAT
        frames, has_fe, has_logits = (self.frames, self.has_fe, self.has_logits) if counters is None else (tuple(counters) + (None,))[:3]
        if isinstance(ff, dict) or isinstance(fe, dict):
            raise NotImplementedError(f"{what}: anyres dict inputs have no clip-stream path (call forward() per image)")
        if seg.seg_recipe(self.proj) != self.RECIPE or self.proj.local_compressor.readout[0].weight.dtype != torch.bfloat16:
            raise NotImplementedError(f"{what}: the module left the scope of {WHAT} ({self.RECIPE_WORDS}, bfloat16) since the stream was opened")
        if not isinstance(ff, torch.Tensor) or ff.ndim != 4:
            raise ValueError(f"{what}: frames_feature is [Tc, H, W, E]")
        Tc = ff.shape[0]
        if tuple(ff.shape[1:]) != (self.H, self.W, self.E):
            raise ValueError(f"{what}: a chunk of {tuple(ff.shape)}; the stream was opened for [Tc, {self.H}, {self.W}, {self.E}]")
        if Tc <= 0 or Tc % self.kt:
            raise ValueError(f"{what}: Tc={Tc} frames; a chunk is a positive number of whole window groups of {self.kt} frames")
        if frames + Tc > self.max_frames:
            raise ValueError(f"{what}: {frames} + {Tc} frames exceed max_frames={self.max_frames} of {WHAT}")
        for name, t in (("frames_feature", ff), ("frames_embed", fe)):
            if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.bfloat16):
                raise NotImplementedError(f"{what}: {name} dtype {getattr(t, 'dtype', type(t))}; the clip stream takes bfloat16 tokens")
        if fe is not None and tuple(fe.shape) != tuple(ff.shape):
            raise ValueError(f"{what}: frames_embed {tuple(fe.shape)} vs frames_feature {tuple(ff.shape)}")
        if ll is not None:
            self._check_logits(what, ll, fe, Tc)
        # the form of a clip: with frames_embed, without it, or with local_logits; every chunk agrees
        if has_fe is not None and (bool(has_logits) != (ll is not None) or (ll is None and (fe is not None) != has_fe)):
            was = "with local_logits" if has_logits else f"{'with' if has_fe else 'without'} frames_embed"
            raise ValueError(f"{what}: this clip's chunks came {was} so far")
        _refuse_grad(self.proj, what)
        _require_bf16_cuda("frames_feature", ff)
        if fe is not None:
            _require_bf16_cuda("frames_embed", fe)
        self._chunk_limits(what, self.proj, Tc, self.H, self.W, self.E)
        return Tc

    def push(self, frames_feature, frames_embed=None, local_logits=None):
        """The next Tc frames of the clip (bf16 [Tc, H, W, E], Tc a positive multiple of kt; frames_embed None: the keys are
        frames_feature).  local_logits (frames_embed None): fp32 [Tc, H, W] ([Q, Tc, H, W] for Q guides) from head_scores --
        the local stage takes its scores from it and reads the value rows only; a clip keeps one of the three forms.  Returns a view of this
        chunk's local output rows in their final place in the stream's output buffer ([chunk rows, hidden]; [Q, chunk rows, hidden], strided
        over q, for Q guides), complete on the caller's stream; the chunk is not referenced afterwards."""
        if local_logits is not None and self.NO_LOGITS:
            raise NotImplementedError(f"{self.NAME}.push: {self.NO_LOGITS}")
        Tc = self._check_chunk(frames_feature, frames_embed, None, local_logits)
        ff = frames_feature.contiguous()
        fe = frames_embed.contiguous() if frames_embed is not None else None
        stream = torch.cuda.current_stream(self.device).cuda_stream
        key = self._plan_key(Tc, fe is not None, stream) + (LOGITS_KEY if local_logits is not None else ())
        plan = seg.cached_plan(self.proj, self.STORE, key, lambda: self._build_plan(Tc, fe is not None))
        row0, nl_group, newline_rows, row1 = chunk_rows(self.proj, self.frames // self.kt, Tc // self.kt, self.gh, self.gw, self.newline is not None)
        if local_logits is None:                  # (the keyed call as it always was: ClipStreamAdapt._launch has no local_logits keyword)
            self._launch(plan, ff, fe, self.frames, row0, nl_group, newline_rows, stream)
        else:
            self._launch(plan, ff, fe, self.frames, row0, nl_group, newline_rows, stream, local_logits=local_logits)
        self.cur ^= 1
        self.has_fe, self.has_logits = fe is not None, local_logits is not None
        self.frames += Tc
        self.n_pushes += 1
        return self.out[:, row0:row1] if self.MULTI else self.out[row0:row1]

    def finish(self):
        """[local rows so far + 32, hidden] ([Q, ...] for Q guides): the rows that depend on the whole clip (a `one_token` newline row, the
        32 global rows of every guide) written behind the local rows pushed so far.  A view of the stream's buffer (strided over q); the
        state is not consumed."""
        from .projector import _refuse_grad
        if self.frames == 0:
            raise ValueError(f"{self.NAME}.finish: nothing has been pushed")
        _refuse_grad(self.proj, f"{self.NAME}.finish")
        row0, lay = prefix_layout(self.proj, self.frames // self.kt, self.gh, self.gw, self.newline is not None)
        self._finish_device(row0, lay.n_rows - row0)
        n = lay.n_rows + self.n_global
        return self.out[:, :n] if self.MULTI else self.out[:n]

    def reset(self, guide=None):
        """A new clip on the same buffers, with the same or a new guide (Q new guides; another Q: ValueError -- open another stream): the
        query preparation runs again (it follows the weights) and the state is emptied on the caller's stream."""
        from .projector import _refuse_grad
        new = guide if guide is not None else self.guides if self.MULTI else self.guide
        if guide is not None:
            self._scope(self.proj, new, self.H, self.W, self.max_frames, self.newline)
            if self.MULTI and new.shape[0] != self.Q:
                raise ValueError(f"{self.NAME}.reset: {new.shape[0]} guides on a stream opened for Q={self.Q} (the buffers are sized by Q)")
            _require_bf16_cuda(self.GUIDE, new)
        _refuse_grad(self.proj, f"{self.NAME}.reset")
        self.frames, self.n_pushes, self.has_fe, self.has_logits = 0, 0, None, None
        self._prepare(new)


class ClipStream(ClipStreamBase):
    """The object HIComProjector.open_stream returns (module docstring): one guide, the fused ring kernel per chunk."""
    NAME, WHAT, STORE = "ClipStream", "open_stream", STORE

    # -- device work: methods of their own, so that the host logic around them can be exercised without a device ---------------------------
    def _allocate(self, rows):
        dev, E, gc = self.device, self.E, self.proj.global_compressor
        self.out = torch.empty((rows, self.hidden), dtype=self.out_dtype, device=dev)
        self.state_ml = torch.empty((2, self.nh, 2), dtype=torch.float32, device=dev)      # (M, L) ping-pong: read one, write the other
        self.state_acc = torch.empty((1, self.nh, E), dtype=torch.float32, device=dev)
        self.q_hi = torch.zeros((16, E), dtype=torch.bfloat16, device=dev)
        self.q_lo = torch.zeros_like(self.q_hi)
        self.qp_state = nv.query_prep_state(E, dev)
        self.pos_a = self.pe_hi = self.pe_lo = None
        self.P = self.y0 = self.x0 = 0
        if gc.use_pos_emb:
            # sized for max_frames: the y / x table offsets (cap, cap + H) never move while the stream lives; the stream keeps the tables
            _, self.kpe, cap = gc.pos_and_kpe(self.max_frames, self.H, self.W, dev)
            self.pe_hi, self.pe_lo = gc.pos_planes(self.max_frames, self.H, self.W, dev)
            self.P, self.y0, self.x0 = self.pe_hi.shape[0], cap, cap + self.H
            self.pos_a = torch.zeros((16, self.P), dtype=torch.float32, device=dev)

    def _prepare(self, guide):
        """Everything that depends on the guide alone: q_proj, the fold, the score-side positional table and the local query rows in one
        launch (hicom_query_prep_fwd), and the empty state.  Once per open_stream / reset, not per push."""
        from .projector import _linear_params
        gc = self.proj.global_compressor
        att = gc.attn_layer
        self.guide = guide.contiguous()
        wq, bq = _linear_params(att.q_proj)
        wk, _ = _linear_params(att.k_proj)
        if gc.use_pos_emb:
            gc.pos_and_kpe(self.max_frames, self.H, self.W, self.device)                   # (follows k_proj.weight in place)
        nv.query_prep(self.guide, self.guide, wq, bq, wk, self.kpe if gc.use_pos_emb else None, self.nh, att.scale, self.q_hi, self.q_lo,
                      self.pos_a, self.qp_state)
        nv.stream_state_clear(self.state_ml, self.state_acc)
        self.cur = 0

    def _build_plan(self, Tc, has_fe):
        nw = (Tc // self.kt) * self.gh * self.gw
        nparts = nv.fused_stream_nparts(nw)
        a = nv.StreamPushArgs()
        ws, (a.part_m, a.part_l, a.part_acc, a.ctx_f16, a.hid_f16), keep = self._fill_common(
            a, Tc, nparts, [nparts * 16 * 4, nparts * 16 * 4, nparts * 16 * self.E * 4, nw * self.E * 2, nw * self.hidden * 2])
        a.rows = self.nh
        return StreamPlan(a, ws, keep, self.proj.local_compressor.readout_f16)

    def _launch(self, plan, ff, fe, t0, row0, nl_group, newline_rows, stream, local_logits=None):
        a = plan.args
        self._patch_common(a, ff, fe, t0, row0, nl_group, newline_rows, stream)
        a.pe_hi = self.pe_hi.data_ptr() if self.pe_hi is not None else None
        a.pe_lo = self.pe_lo.data_ptr() if self.pe_lo is not None else None
        if local_logits is None:
            nv.compressor_stream_push(a)
        else:
            nv.compressor_stream_push_logits(a, local_logits.data_ptr())

    def head_scores(self, last_hidden_state, head, hidden_act=None):
        """fp32 [Tc, H, W]: what push(frames_feature, None, local_logits=) takes for the chunk whose tower output is last_hidden_state --
        siglip_head_scores with the stream's guide.  U and c are folded from the live weights on every call: nothing is kept."""
        from .encoder import siglip_head_scores
        return siglip_head_scores(last_hidden_state, head, self.guide, hidden_act)

    def _finish_device(self, row0, tail):
        if tail:                                                                           # whole-clip newline rows (`one_token`)
            nv.scatter_rows(self.newline.view(1, -1), self.out, row0, tail)
        gc = self.proj.global_compressor
        gc.finish(self.state_ml[self.cur:self.cur + 1], self.state_acc, self.guide.view(1, -1), self.out, row0 + tail, self.n_global)


# =================================================================================================================================
# several guides per stream (HIComProjector.open_stream_multi)
# =================================================================================================================================
class ClipStreamMulti(ClipStreamBase):
    """The object HIComProjector.open_stream_multi returns: ONE video that arrives in chunks, Q guides known up front.

        s = proj.open_stream_multi(guide_embeds[Q, E], H, W, max_frames, image_newline)        # 1 <= Q <= 32
        rows = s.push(frames_feature[Tc, H, W, E], frames_embed or None)     # [Q, chunk rows, hidden]; the chunk may be freed afterwards
        out = s.finish()                                                     # [Q, local rows so far + 32, hidden]

    out[q] is what forward() gives for the concatenation of everything pushed with guide q (to the kernels' rounding).  finish() does not
    consume the state.  The output buffer `out` is [Q, cap_rows + 32, hidden] with cap_rows = the local rows of max_frames frames: the
    views push() and finish() return are STRIDED over q (a row range of every guide's block; `.contiguous()` copies), valid until the rows
    are written again (reset, or a later finish() for the rows behind the local ones).

    One push is one host call (hicom_compressor_stream_push_multi): the multi-guide local kernel on the chunk's windows, the many-row
    global stream over the chunk's tokens at the absolute frame offset, its merge into ONE un-normalised set of R = heads x Q rows, the fold
    of that set into the carried state (hicom_stream_state_fold_set_fwd), the readout GEMM pair over Q x windows rows and the placement.
    The tokens of a chunk are read once for all Q guides by the local stage and once per 32 folded rows by the global stage.

    Per stream (open and reset): q_proj over the Q guides, the fold into the hi / lo query planes and the score-side positional table (sized
    for max_frames: the y / x offsets never move), the empty state.  Per plan -- (Q, Tc, H, W, E, has frames_embed, newline, out dtype,
    stream), cached on the module as `proj._clip_stream_multi_plans` -- the workspace of ONE chunk; push allocates nothing.

    Scope: that of open_stream (plain release recipe, bf16 module and inputs, inference only, exact window partition, E == 1152,
    hidden % 64 == 0; windows of <= 64 tokens) with 1 <= Q <= 32 and the merge kernels' LDS limits on a chunk (multi_chunk_limits)."""
    NAME, WHAT, STORE = "ClipStreamMulti", "open_stream_multi", STORE_MULTI
    MULTI, GUIDE = True, "guide_embeds"
    R = property(lambda self: self.Q * self.nh)                     # folded rows: guide q's heads are rows nh q .. nh q + nh - 1
    rows_pad = property(lambda self: (self.R + 31) // 32 * 32)      # whole 32-row passes of the many-row stream kernel

    def _chunk_limits(self, what, proj, Tc, H, W, E):
        multi_chunk_limits(what, Tc, H, W, proj.global_compressor.use_pos_emb)

    # -- device work ------------------------------------------------------------------------------------------------------------------------
    def _allocate(self, rows):
        dev, E, Q, R, RP, gc = self.device, self.E, self.Q, self.R, self.rows_pad, self.proj.global_compressor

        def f32(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)
        self.out = torch.empty((Q, rows, self.hidden), dtype=self.out_dtype, device=dev)
        self.state_ml = f32(2, R, 2)                                         # (M, L) ping-pong: read one block, write the other
        self.state_acc = f32(1, R, E)
        self.qp = f32(Q, E)
        self.q_hi = torch.zeros((RP, E), dtype=torch.bfloat16, device=dev)   # rows >= R stay zero (the fold does not write them)
        self.q_lo = torch.zeros_like(self.q_hi)
        # finish(): the combined contexts and the global tail with M = Q
        self.fin = (f32(R, E), f32(Q, E), f32(Q, E), f32(Q, gc.readout[0].out_features), f32(Q, gc.readout[2].out_features))
        self.pos_a = self.pe = self.kpe = None
        self.P = self.y0 = self.x0 = 0
        if gc.use_pos_emb:
            # sized for max_frames: the y / x table offsets (cap, cap + H) never move while the stream lives; the stream keeps the tables
            self.pe, self.kpe, cap = gc.pos_and_kpe(self.max_frames, self.H, self.W, dev)
            self.P, self.y0, self.x0 = self.pe.shape[0], cap, cap + self.H
            self.pos_a = torch.zeros((RP, self.P), dtype=torch.float32, device=dev)

    def _prepare(self, guides):
        """Everything that depends on the guides alone: q_proj with M = Q, the fold into the query planes and the score-side positional
        table, the empty state.  Once per open_stream_multi / reset, not per push."""
        from .projector import _linear_params
        gc = self.proj.global_compressor
        att = gc.attn_layer
        self.guides = guides.contiguous()
        wq, bq = _linear_params(att.q_proj)
        wk, _ = _linear_params(att.k_proj)
        if gc.use_pos_emb:
            gc.pos_and_kpe(self.max_frames, self.H, self.W, self.device)                   # (follows k_proj.weight in place)
        nv.linear(self.guides, wq, bq, self.qp)
        nv.fold_query_split(self.qp, wk, self.kpe, self.nh, att.scale, self.q_hi, self.q_lo, self.pos_a)
        nv.stream_state_clear(self.state_ml, self.state_acc)
        self.cur = 0

    def _build_plan(self, Tc, has_fe):
        a = nv.StreamPushMultiArgs()
        ws, _, keep = self._fill_block(a, Tc)
        return StreamPlan(a, ws, keep, self.proj.local_compressor.readout_f16)

    def _fill_block(self, a, Tc, extra=()):
        """The fields of the push block `a` that the module and the chunk shape decide, and the workspace of ONE chunk with its regions
        entered into `a`.  extra: byte sizes of further regions behind them (0: none).  Returns (workspace, the addresses of the extra
        regions -- None for an empty one --, the tensors the block points at)."""
        gc = self.proj.global_compressor
        E, hidden, H, W, Q, R, RP = self.E, self.hidden, self.H, self.W, self.Q, self.R, self.rows_pad
        nw = (Tc // self.kt) * self.gh * self.gw
        N = Tc * H * W
        ntiles = (N + 15) // 16
        nparts = max(1, min(nv.global_stream_nparts(N, RP), ntiles, MAX_PARTS))
        marg = bool(gc.use_pos_emb) and nv.global_stream_has_marg(N, E, RP, H, W, nparts)      # the form, once per plan
        stride = ntiles * 16
        odt = 4 if self.out_dtype == torch.float32 else 2
        scores = max(RP * stride, nparts * RP * nv.global_stream_marg_width(H, W))
        ws, at, keep = self._fill_common(a, Tc, nparts, [nparts * RP * 4, nparts * RP * 4, nparts * RP * E * 4, scores * 4, RP * Tc * (H + W + 2) * 4, R * 2 * 4,
                                                         R * E * 4, Q * nw * E * 2, Q * nw * hidden * 2, Q * nw * hidden * odt, *extra])
        a.Q, a.nh, a.marg, a.score_stride = Q, self.nh, int(marg), stride
        (a.part_m, a.part_l, a.part_acc, a.scores, a.scratch, a.set_ml, a.set_acc, a.ctx_f16, a.hid_f16, a.loc) = at[:10]
        return ws, [p if n else None for p, n in zip(at[10:], extra)], keep

    def _launch(self, plan, ff, fe, t0, row0, nl_group, newline_rows, stream, local_logits=None):
        self._patch(plan.args, ff, fe, t0, row0, nl_group, newline_rows, stream)
        if local_logits is None:
            nv.compressor_stream_push_multi(plan.args)
        else:
            q_stride = logits_stride(f"{self.NAME}.push", local_logits, self.Q, ff.shape[0] * self.H * self.W)
            nv.compressor_stream_push_multi_logits(plan.args, local_logits.data_ptr(), q_stride)

    def head_scores(self, last_hidden_state, head, hidden_act=None):
        """fp32 [Q, Tc, H, W]: what push(frames_feature, None, local_logits=) takes for the chunk whose tower output is last_hidden_state --
        siglip_head_scores_multi with the stream's guides.  U and c are folded from the live weights on every call: nothing is kept."""
        from .encoder import siglip_head_scores_multi
        return siglip_head_scores_multi(last_hidden_state, head, self.guides, hidden_act)

    def _patch(self, a, ff, fe, t0, row0, nl_group, newline_rows, stream):
        """_patch_common on the plain push block `a`, and what only the multi-guide block has."""
        self._patch_common(a, ff, fe, t0, row0, nl_group, newline_rows, stream)
        a.guide, a.q_stride = self.guides.data_ptr(), self.out.stride(0)
        a.pe = self.pe.data_ptr() if self.pe is not None else None

    def _finish_device(self, row0, tail):
        self.proj.global_compressor.finish_guides(self.state_ml[self.cur:self.cur + 1], self.state_acc, self.guides, self.fin)
        nv.stream_place_global(self.fin[4], self.newline, tail, self.n_global, self.out, row0)


# =================================================================================================================================
# several guides per stream on the k / v adaptor recipe (HIComProjector.open_stream_adapt)
# =================================================================================================================================
class ClipStreamAdapt(ClipStreamMulti):
    """The object HIComProjector.open_stream_adapt returns for a module of the k / v adaptor recipe (`local43_adaptkv_global32`; adapt_k
    and / or adapt_v on the local compressor): ClipStreamMulti's surface, state, output buffer, finish() and reset().

    The adaptors sit on the local stage only and the adaptor MLPs do not know the guide, so only the local stage of a push differs
    (hicom_compressor_stream_push_multi_adapt): both layers of each adaptor MLP over the chunk's Tc H W tokens ONCE for all Q guides, into
    fp16 planes ky / vy [Tc H W, E] that live for that push; the multi-guide local kernel that blends LayerNorm of those planes into the
    rows it loads (the kernel of forward_prepared); then the launches of the plain push.  Without frames_embed the k adaptor reads
    frames_feature, as the keys do.

    Per plan -- ClipStreamMulti's key plus the adaptor set, cached on the module as `proj._clip_stream_adapt_plans` -- the workspace of ONE
    chunk: the parent's regions, the two planes and the hidden planes of layer 1 (4 x 2304 bytes per token of a chunk with both adaptors).
    The planes are written and read inside one push, in stream order, so two streams of one module share a plan.  push allocates nothing.
    The plan follows the weights as every plan does: its refresh rebuilds the cached fp16 copies of the adaptors' second layers.

    Scope: that of open_stream_multi with the adaptor recipe in the place of the plain one, adaptor widths % 64 == 0 and Tc H W E < 2^32
    per chunk."""
    NAME, WHAT, STORE = "ClipStreamAdapt", "open_stream_adapt", STORE_ADAPT
    RECIPE, RECIPE_WORDS = "adaptkv", "the k / v adaptor release recipe"
    NO_LOGITS = NOT_LINEAR                           # (push is the base's: its local_logits keyword raises NotImplementedError here)

    def head_scores(self, last_hidden_state, head, hidden_act=None):
        raise NotImplementedError(f"{self.NAME}.head_scores: {NOT_LINEAR}")

    def _scope(self, proj, guide_embeds, H, W, max_frames, image_newline):
        dims = super()._scope(proj, guide_embeds, H, W, max_frames, image_newline)
        adaptor_widths(self.WHAT, proj.local_compressor)
        return dims

    def _chunk_limits(self, what, proj, Tc, H, W, E):
        super()._chunk_limits(what, proj, Tc, H, W, E)
        adapt_chunk_limit(what, Tc, H, W, E)

    def _plan_key(self, Tc, has_fe, stream):
        lc = self.proj.local_compressor
        return super()._plan_key(Tc, has_fe, stream) + (bool(lc.adapt_k), bool(lc.adapt_v))

    def _build_plan(self, Tc, has_fe):
        lc = self.proj.local_compressor
        args = nv.StreamPushMultiAdaptArgs()
        keep = []

        def ptr(t):
            if t is None:
                return None
            keep.append(t)
            return t.data_ptr()
        seg.fill_adaptors(args, lc, self.WHAT, ptr)
        N = Tc * self.H * self.W
        hid_bytes = nv.clip_adapt_prepare_workspace(N, self.E, args.ak, args.av, self.WHAT)     # (the GEMM's operand limit raises here)
        plane = N * self.E * 2
        ws, (args.ky, args.vy, args.adapt_ws), readout = self._fill_block(args.base, Tc, (plane if lc.adapt_k else 0, plane if lc.adapt_v else 0,
                                                                                         hid_bytes))
        args.adapt_ws_bytes = hid_bytes

        def refresh():
            lc.readout_f16()
            seg.refresh_adaptors(lc)
        return StreamPlan(args, ws, keep + readout, refresh)

    def _launch(self, plan, ff, fe, t0, row0, nl_group, newline_rows, stream):
        self._patch(plan.args.base, ff, fe, t0, row0, nl_group, newline_rows, stream)
        nv.compressor_stream_push_multi_adapt(plan.args)
