"""HIComProjector.prepare_clip / forward_prepared: the k / v adaptor recipe with the adaptor MLPs run ONCE per video, Q guides per call
(csrc/multi_guide.hip: hicom_clip_adapt_prepare_fwd, hicom_compressor_multiguide_adapt_fwd).

key = (1 - a_k) x + a_k LN(MLP_k(x)) and the values likewise depend on the tokens alone; the guide is only the query of the two stages.
The reference's Video-MME driver asks several questions about one video tensor (hicom/eval/video/inference_video_mcqa_videomme.py:268-303),
a chat asks them one after another: with `local43_adaptkv_global32` each of them was a full forward(), the two D -> D -> D GEMM pairs over
every token included.  Here a PreparedClip keeps y = MLP(x) as fp16 planes and every later call is the multi-guide step (§3.8) with a local
kernel that blends LayerNorm(y) into the rows it loads.  Scope rule, input checks, plans and plan cache are segments.py's and
multi_guide.py's; a plain-recipe module gets a clip without planes and its calls are forward_multi_guide."""
from __future__ import annotations

import torch

from . import engine
from . import multi_guide
from . import native as nv
from . import segments as seg

STORE = "_prepared_plans"               # forward_prepared: keyed like forward_multi_guide's, plus the recipe
PREPARE_STORE = "_prepare_plans"        # prepare_clip: the adaptor descriptors and the hidden planes of layer 1, keyed by token count


def _adaptor_params(proj):
    return [p for _, mlp, _, _ in engine.adaptor_streams(proj.local_compressor) for p in mlp.parameters()]


def adaptor_sig(proj):
    """engine.plan_sig + engine.content_sig restricted to the parameters of the adaptor MLPs: the module, their storage addresses, their
    in-place version counters and the process-wide weights epoch (writes through `.data`, which no version counter sees)."""
    ps = _adaptor_params(proj)
    return (id(proj), sum(p.data_ptr() for p in ps), sum(p._version for p in ps)), nv.weights_epoch()


def _fingerprint(proj):
    """An int64 checksum per adaptor MLP parameter, on the device (position-weighted sum of the bf16 bit patterns).  The weights epoch is
    one number per process: when it moves while the adaptor parameters' own addresses and counters stand, this tells whether THEIR content
    moved or somebody else's."""
    sums = []
    for p in _adaptor_params(proj):
        bits = p.detach().contiguous().view(torch.int16).flatten().to(torch.int64)
        ramp = torch.arange(bits.numel(), device=bits.device, dtype=torch.int64) % 8191 + 1
        sums.append((bits * ramp).sum())
    return torch.stack(sums)


class PreparedClip:
    """What HIComProjector.prepare_clip returns.  Owns the fp16 planes y_k / y_v [T H W, E] (None for a stream without adaptor; both None
    for a plain-recipe module); keeps REFERENCES to the caller's frames_feature / frames_embed, which every later call reads in place: the
    caller must not overwrite them while the clip is in use.  Records the modality and shape, the weight state of the adaptor MLPs the
    planes were computed from, and an event on the stream it was made on."""
    __slots__ = ("proj", "ff", "fe", "modal", "shape", "y_k", "y_v", "sig", "epoch", "mark", "event", "stream")

    def __init__(self, proj, ff, fe, modal):
        self.proj, self.ff, self.fe, self.modal, self.shape = proj, ff, fe, modal, tuple(ff.shape)
        self.y_k = self.y_v = self.sig = self.epoch = self.mark = self.event = self.stream = None

    @property
    def nbytes(self) -> int:
        """Bytes of the planes: 2 E = 2304 per token and adapted stream."""
        return sum(y.numel() * 2 for y in (self.y_k, self.y_v) if y is not None)

    def refresh(self):
        """Recomputes the planes IN PLACE from the module's present adaptor weights, on the current stream (the caller orders it behind
        calls still running on other streams), and takes their weight state as the clip's."""
        _fill_planes(self)
        return self

    def is_stale(self) -> bool:
        """True when the adaptor MLP weights moved since the planes were computed.  Free while the weight state stands (addresses, version
        counters, weights epoch: what the plans look at); when only the process-wide epoch moved -- a write through `.data` somewhere -- the
        checksums of the adaptor parameters are compared once, which reads the device."""
        if self.y_k is None and self.y_v is None:
            return False
        sig, epoch = adaptor_sig(self.proj)
        if sig != self.sig:
            return True
        if epoch != self.epoch:
            if not torch.equal(_fingerprint(self.proj), self.mark):
                return True
            self.epoch = epoch
        return False


class _PreparePlan:
    __slots__ = ("args", "ws", "ws_bytes", "keep", "sig", "fresh", "refresh", "hits")

    def __init__(self, args, ws, ws_bytes, keep, refresh):
        self.args, self.ws, self.ws_bytes, self.keep, self.refresh = args, ws, ws_bytes, keep, refresh
        self.sig = self.fresh = None
        self.hits = 0


def _prepare_plan(proj, N, E, dev, stream):
    lc = proj.local_compressor

    def build():
        args = nv.CompressorMultiGuideAdaptArgs()          # (the holder of the two descriptors: what fill_adaptors fills)
        keep = []

        def ptr(t):
            if t is None:
                return None
            keep.append(t)
            return t.data_ptr()
        seg.fill_adaptors(args, lc, "prepare_clip", ptr)
        nbytes = nv.clip_adapt_prepare_workspace(N, E, args.ak, args.av)       # (the GEMM's operand limit raises here, in front of any launch)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        return _PreparePlan(args, ws, nbytes, keep, lambda: seg.refresh_adaptors(lc))
    return seg.cached_plan(proj, PREPARE_STORE, (N, E, lc.adapt_k, lc.adapt_v, stream), build)


def _fill_planes(clip):
    """Both layers of each adaptor MLP over the clip's tokens into its planes, on the current stream."""
    proj, ff, fe = clip.proj, clip.ff, clip.fe
    if clip.y_k is None and clip.y_v is None:
        return
    dev = ff.device
    N, E = ff.numel() // ff.shape[-1], ff.shape[-1]
    cur = torch.cuda.current_stream(dev)
    plan = _prepare_plan(proj, N, E, dev, cur.cuda_stream)
    a = plan.args
    nv.clip_adapt_prepare_fwd((fe if fe is not None else ff).data_ptr(), ff.data_ptr(), N, E, a.ak, a.av,
                              None if clip.y_k is None else clip.y_k.data_ptr(), None if clip.y_v is None else clip.y_v.data_ptr(),
                              plan.ws.data_ptr(), plan.ws_bytes, cur.cuda_stream)
    clip.sig, clip.epoch = adaptor_sig(proj)
    clip.mark = _fingerprint(proj)
    clip.stream = cur
    clip.event = torch.cuda.Event()
    clip.event.record(cur)


def prepare_clip(proj, ff, fe, modal):
    from .projector import _refuse_grad
    what = "prepare_clip"
    E = seg.check_tokens(what, "prepared-clip", proj, ff, fe, 4, "[T, H, W, E]")
    T, H, W, _ = ff.shape
    if modal == "image" and T != 1:
        raise ValueError(f"{what}: image modality expects a single frame [1, H, W, E]")
    seg.exact_tilings(what, proj, T, H, W, modal)
    _refuse_grad(proj, f"HIComProjector.{what}")
    ff = ff.contiguous()
    fe = fe.contiguous() if fe is not None else None
    clip = PreparedClip(proj, ff, fe, modal)
    if seg.seg_recipe(proj) == "adaptkv":
        lc = proj.local_compressor
        plane = lambda: torch.empty((T * H * W, E), dtype=torch.float16, device=ff.device)
        clip.y_k = plane() if lc.adapt_k else None
        clip.y_v = plane() if lc.adapt_v else None
        _fill_planes(clip)
    return clip


def run_prepared(proj, clip, guides, nl=None, chunks=None):
    what = "forward_prepared"
    if not isinstance(clip, PreparedClip):
        raise ValueError(f"{what}: the first argument is what prepare_clip returned (got {type(clip).__name__})")
    if clip.proj is not proj:
        raise ValueError(f"{what}: the clip was prepared by another module")
    if clip.y_k is None and clip.y_v is None:              # a plain-recipe module: one code path in the caller serves both recipes
        return proj.forward_multi_guide(clip.ff, clip.fe, guides, clip.modal, nl, chunks=chunks)
    Q, T, H, W, E, tiles = multi_guide.clip_scope(what, "prepared-clip", proj, clip.ff, clip.fe, guides, clip.modal, nl)
    lc = proj.local_compressor
    if (clip.y_k is not None) != bool(lc.adapt_k) or (clip.y_v is not None) != bool(lc.adapt_v):
        raise ValueError(f"{what}: the module's adaptors changed since prepare_clip")
    dev, ff, fe, guides, nl, out_dtype, stream = seg.call_inputs(proj, what, clip.ff, clip.fe, guides, nl)
    if clip.is_stale():
        raise RuntimeError(f"{what}: the clip is stale: the adaptor MLP weights moved since prepare_clip (clip.refresh() recomputes its planes)")
    modal = clip.modal
    key = (Q, T, H, W, E, fe is not None, modal, None if nl is None else tuple(nl.shape), out_dtype, stream, int(chunks or 0),
           seg.seg_recipe(proj), lc.adapt_k, lc.adapt_v)
    plan = seg.cached_plan(proj, STORE, key, lambda: seg.build_equal_plan(
        proj, what, nv.CompressorMultiGuideArgs, nv.CompressorMultiGuideAdaptArgs, "Q", (Q, T, H, W, E), tiles, modal, nl, out_dtype, chunks, dev,
        nv.compressor_multiguide_workspace))
    cur = torch.cuda.current_stream(dev)
    if cur != clip.stream:                                  # on the device: no host wait
        cur.wait_event(clip.event)
        for y in (clip.y_k, clip.y_v):
            if y is not None:
                y.record_stream(cur)
    args, a = plan.args, plan.io
    args.ky = None if clip.y_k is None else clip.y_k.data_ptr()
    args.vy = None if clip.y_v is None else clip.y_v.data_ptr()
    out = torch.empty((Q, plan.rows, plan.hidden), dtype=out_dtype, device=dev)
    seg.patch_io(a, ff, fe, guides, nl if a.nl_count > 0 else None, out, stream)
    nv.compressor_multiguide_fwd(args)
    return out
