"""CPU checks of the host side of forward_prepared_many (csrc/ragged_multi_guide.hip: hicom_compressor_clips_multiguide_*;
hicom_amd/native.py, hicom_amd/prepared_many.py): the new symbols, the new argument struct as the host C compiler lays it out against its
ctypes mirror, the workspace rule (tokens and planes are the caller's: the entry point asks for what the ragged multi-guide step asks for
on the base block), the refusals of the C entry points in front of any device call, and the Python refusals that need no device.

As in tests/test_ragged_multi_guide_host.py: with chunks > 0 the workspace function and every check in front of the first launch are pure
host code, pointer fields are made-up aligned addresses that nothing reads before a launch, and every *_fwd / *_prepare case breaks one
rule, so none launches or copies."""
import ctypes

import pytest
import torch

import cases
import host_util
from hicom_amd import native as nv
from hicom_amd import prepared, prepared_many
from host_util import ADDR, EINVAL, EUNSUP

POINTERS = ("guide", "out", "newline", "lw0_f16", "lb0", "lw2_f16", "lb2", "wq", "bq", "wk", "wv", "bv", "wo", "bo", "gw0", "gb0", "gw2", "gb2", "pe", "kpe")
STORE = "_prepared_many_plans"
IMAGE, CLIP4, CLIP8 = (1, 1, 0, 0, 0, 1, 32), (4, 4, 0, 0, 0, 1, 32), (8, 4, 0, 0, 0, 1, 32)
MIX6 = ([IMAGE, CLIP4, IMAGE, CLIP8, IMAGE], (1, 3, 5, 2, 4), 6)
MIX9 = ([IMAGE, CLIP4], (4, 8), 9)


def block(mix=MIX6, fwd=False, adapt=(True, True), item_ptrs=ADDR, **over):
    """A valid block: a mix on its grid, windows of 3 x 3, hidden 896, fp32 rows, 3 token chunks, the adaptors of `adapt` (k, v)."""
    items, counts, grid = mix
    args = nv.CompressorClipsMultiGuideArgs()
    a = args.base
    args._items = (nv.RaggedItem * len(items))(*[nv.RaggedItem(*d) for d in items])
    args._counts = (ctypes.c_int32 * len(counts))(*counts)
    a.B, a.H, a.W, a.E, a.hidden, a.ks, a.nh, a.P = len(items), grid, grid, 1152, 896, 3, 9, 0
    a.chunks, a.out_dt, a.l_scale = 3, nv.DT_F32, 0.125
    a.items, a.guide_counts, a.n_guide_counts = args._items, args._counts, len(counts)
    for d, on in zip((args.ak, args.av), adapt):
        if on:
            d.w0 = d.gamma = d.beta = d.alpha = ADDR
    args.alpha_dt, args.eps = nv.DT_BF16, 1e-5
    if fwd:
        for f in POINTERS:
            setattr(a, f, ADDR)
        a.P, a.t_index0, a.y_index0, a.x_index0 = 28, 0, 16, 22
        a.ldo, a.ws, a.ws_bytes = a.hidden, ADDR, 1 << 40
    args.item_ptrs = item_ptrs
    for k, v in over.items():
        setattr(a, k, v)
    return args


def call(fn, args):
    r = getattr(nv.lib(), f"hicom_compressor_clips_multiguide_{fn}")(None if args is None else ctypes.byref(args))
    return int(r), nv.lib().hicom_last_error().decode()


@pytest.mark.parametrize("mix", [MIX6, MIX9], ids=["mix6", "mix9"])
@pytest.mark.parametrize("over", [dict(), dict(out_dt=nv.DT_BF16, P=28), dict(chunks=18)], ids=["f32", "bf16_pos", "chunks18"])
def test_workspace_is_the_ragged_multi_guide_steps_on_the_base_block(mix, over):
    """Tokens and planes are the caller's: nothing is added, whichever streams are adapted."""
    want = None
    for adapt in ((True, True), (True, False), (False, True), (False, False)):
        args = block(mix, adapt=adapt, **over)
        base = nv.lib().hicom_compressor_ragged_multiguide_workspace_bytes(ctypes.byref(args.base))
        assert base > 0 and (want is None or base == want)
        want = base
        assert call("workspace_bytes", args)[0] == base == nv.compressor_clips_multiguide_workspace(args)


def with_counts(*counts):
    return ([CLIP4] * len(counts), counts, 6)


REFUSALS = {
    "NULL block": ("fwd", None, EINVAL, "compressor_clips_multiguide: NULL arguments"),
    "NULL block, workspace": ("workspace_bytes", None, EINVAL, "compressor_clips_multiguide: NULL arguments"),
    "NULL block, prepare": ("prepare", None, EINVAL, "compressor_clips_multiguide: NULL arguments"),
    "non-NULL ff": ("fwd", dict(fwd=True, ff=ADDR), EINVAL, "compressor_clips_multiguide: the clips' tokens come through item_ptrs: base.ff and base.fe must be NULL"),
    "non-NULL fe": ("fwd", dict(fwd=True, fe=ADDR), EINVAL, "compressor_clips_multiguide: the clips' tokens come through item_ptrs: base.ff and base.fe must be NULL"),
    "non-NULL ff, workspace": ("workspace_bytes", dict(ff=ADDR), EINVAL, "base.ff and base.fe must be NULL"),
    "non-NULL ff, prepare": ("prepare", dict(fwd=True, ff=ADDR), EINVAL, "base.ff and base.fe must be NULL"),
    "NULL item_ptrs": ("fwd", dict(fwd=True, item_ptrs=None), EINVAL, "compressor_clips_multiguide: item_ptrs is a 16-byte aligned DEVICE table [B][4]"),
    "item_ptrs not 16-byte aligned": ("fwd", dict(fwd=True, item_ptrs=ADDR + 8), EINVAL, "item_ptrs is a 16-byte aligned DEVICE table"),
    "Q_i = 0": ("fwd", dict(fwd=True, mix=with_counts(3, 0)), EUNSUP, "compressor_ragged_multiguide: item 1: Q=0 guides (1 <= Q <= 32 per item)"),
    "Q_i = 33": ("fwd", dict(fwd=True, mix=with_counts(33, 1)), EUNSUP, "compressor_ragged_multiguide: item 0: Q=33 guides (1 <= Q <= 32 per item)"),
    "workspace: Q_i = 0": ("workspace_bytes", dict(mix=with_counts(0)), EUNSUP, "item 0: Q=0 guides (1 <= Q <= 32 per item)"),
    "workspace: Q_i = 33": ("workspace_bytes", dict(mix=with_counts(1, 33)), EUNSUP, "item 1: Q=33 guides (1 <= Q <= 32 per item)"),
    "prepare: Q_i = 33": ("prepare", dict(fwd=True, mix=with_counts(1, 33)), EUNSUP, "item 1: Q=33 guides (1 <= Q <= 32 per item)"),
    "T not a multiple of kt": ("fwd", dict(fwd=True, mix=([CLIP4, (6, 4, 0, 0, 0, 1, 32)], (1, 2), 6)), EUNSUP,
                               "compressor_ragged_multiguide: item 1 needs an exact window partition (T=6, temporal window 4)"),
    "workspace: T not a multiple of kt": ("workspace_bytes", dict(mix=([(6, 4, 0, 0, 0, 1, 32)], (2,), 6)), EUNSUP,
                                          "item 0 needs an exact window partition (T=6, temporal window 4)"),
    "hidden not a multiple of 64": ("fwd", dict(fwd=True, hidden=100, ldo=100), EUNSUP, "hidden=100 (multiple of 64"),
    "NULL guide": ("fwd", dict(fwd=True, guide=None), EINVAL, "compressor_ragged_multiguide: NULL pointer"),
    "workspace too small": ("fwd", dict(fwd=True, ws_bytes=4096), EINVAL, "256-byte aligned"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_c_refusals_in_front_of_any_device_call(name):
    fn, kw, code, needle = REFUSALS[name]
    got, msg = call(fn, None if kw is None else block(**kw))
    assert got == code, (got, msg)
    assert needle in msg, msg


def test_c_refusals_alpha_dtype_and_adaptor_weights():
    args = block(fwd=True)
    args.alpha_dt = nv.DT_F16
    for fn in ("fwd", "workspace_bytes", "prepare"):
        assert call(fn, args) == (EINVAL, "compressor_clips_multiguide: alpha dtype 2 (bf16 | f32)")
    with pytest.raises(nv.HicomNativeError, match="alpha dtype 2"):
        nv.compressor_clips_multiguide_workspace(args)
    plain = block(adapt=(False, False))                # the plain recipe: the adaptor fields are not looked at
    plain.alpha_dt = nv.DT_F16
    assert call("workspace_bytes", plain)[0] > 0
    args = block(fwd=True)
    args.av.gamma = None
    assert call("fwd", args) == (EINVAL, "compressor_clips_multiguide: adaptor weights")
    args = block(fwd=True, adapt=(False, True))        # the key stream is not adapted: its descriptor is not looked at
    args.ak.gamma = args.ak.beta = args.ak.alpha = None
    args.base.ws_bytes = 4096                          # (... and the call still ends in front of a launch)
    code, msg = call("fwd", args)
    assert code == EINVAL and "256-byte aligned" in msg


def test_a_limit_of_the_kernels_is_not_implemented_error_under_the_python_name():
    with pytest.raises(NotImplementedError, match=r"forward_prepared_many: .*Q=33 guides"):
        nv.compressor_clips_multiguide_workspace(block(mix=with_counts(33)))


# ---- Python refusals that need no device ------------------------------------------------------------------------------------------------
def module(ptype="local43_adaptkv_global32", use_guide="direct", dtype=torch.bfloat16):
    return host_util.module(ptype, use_guide, dtype, hidden_size=896)


def cpu_clip(m, T=4, h=6, w=6, fe=True, modal="video", planes=(True, True)):
    """A PreparedClip as prepare_clip would leave it, on CPU tensors: what the checks in front of any device call look at."""
    ff = torch.zeros((T, h, w, cases.D), dtype=torch.bfloat16)
    c = prepared.PreparedClip(m, ff, ff.clone() if fe else None, modal)
    plane = lambda: torch.zeros((T * h * w, cases.D), dtype=torch.float16)
    c.y_k, c.y_v = (plane() if planes[0] else None), (plane() if planes[1] else None)
    return c


def test_python_refusals_without_a_device_leave_no_plan():
    m, other = module(), module()
    g = torch.zeros((3, cases.D), dtype=torch.bfloat16)
    a, b = cpu_clip(m), cpu_clip(m, T=8)
    refused = [
        (ValueError, "clip 1 was prepared by another module", [a, cpu_clip(other)], [2, 1]),
        (ValueError, "clip 2 has no frames_embed, clip 0 has", [a, b, cpu_clip(m, fe=False)], [1, 1, 1]),
        (ValueError, "clip 0 has none", [cpu_clip(m, fe=False), a], [2, 1]),
        (ValueError, r"clip 1 is 9 x 9 x 1152 \(H x W x E\), clip 0 6 x 6 x 1152", [a, cpu_clip(m, T=1, h=9, w=9, modal="image")], [2, 1]),
        (ValueError, r"clip 1 is 6 x 9 x 1152", [a, cpu_clip(m, h=6, w=9)], [2, 1]),
        (ValueError, "clip 1: the module's adaptors changed since prepare_clip", [a, cpu_clip(m, planes=(True, False))], [2, 1]),
        (ValueError, "clip 0: the module's adaptors changed since prepare_clip", [cpu_clip(m, planes=(False, False))], [3]),
        (ValueError, "clip 1 is not what prepare_clip returned", [a, a.ff], [2, 1]),
        (ValueError, "non-empty sequence", [], []),
        (ValueError, "sequence of what prepare_clip returned", a, [3]),
    ]
    with torch.no_grad():
        for exc, match, clips, counts in refused:
            with pytest.raises(exc, match=match):
                m.forward_prepared_many(clips, g, counts)
        with pytest.raises(nv.HicomNativeError, match="GPU only"):        # (everything a CPU can decide has passed)
            m.forward_prepared_many([a, b, a], g, [1, 1, 1])
        plain = module("local43_global32")
        with pytest.raises(ValueError, match="clip 0: the module's adaptors changed"):
            plain.forward_prepared_many([cpu_clip(plain)], g, [3])
        with pytest.raises(nv.HicomNativeError, match="GPU only"):
            plain.forward_prepared_many([cpu_clip(plain, planes=(False, False))], g, [3])
        coarse = module(use_guide="coarse")
        with pytest.raises(NotImplementedError, match="two release recipes"):
            coarse.forward_prepared_many([cpu_clip(coarse)], g, [3])
        half = module(dtype=torch.float16)
        with pytest.raises(NotImplementedError, match="float16"):
            half.forward_prepared_many([cpu_clip(half)], g, [3])
    for mod in (m, other, plain, coarse, half):
        assert not mod.__dict__.get(STORE) and not mod.__dict__.get("_ragged_multi_guide_plans")


def test_guide_checks_need_no_device():
    E = cases.D
    g = torch.zeros((6, E), dtype=torch.bfloat16)
    for counts, match in (([3], "2 clips"), ([0, 6], "Q_i <= 32"), ([33, 1], "Q_i <= 32"), (3, "sequence of positive ints")):
        with pytest.raises(ValueError, match=match):
            prepared_many.check_guides(2, E, g, counts)
    for bad in (g[:5], g[:, :-1], g[0], None):
        with pytest.raises(ValueError, match=r"\[sum Q_i, E\]"):
            prepared_many.check_guides(2, E, bad, [2, 4])
    with pytest.raises(nv.HicomNativeError, match="GPU only"):
        prepared_many.check_guides(2, E, g, [2, 4])


def test_pointer_rows_are_checked_on_the_host():
    m = module()
    a, b = cpu_clip(m), cpu_clip(m, fe=False, planes=(False, True))
    rows = prepared_many.pointer_rows([a, b])
    assert rows[0] == (a.fe.data_ptr(), a.ff.data_ptr(), a.y_k.data_ptr(), a.y_v.data_ptr())
    assert rows[1] == (b.ff.data_ptr(), b.ff.data_ptr(), 0, b.y_v.data_ptr())           # keys from frames_feature; no k plane: 0
    odd = cpu_clip(m)
    odd.y_v = torch.zeros((4 * 36 * cases.D + 1,), dtype=torch.float16)[1:].view(4 * 36, cases.D)     # 2 bytes off
    with pytest.raises(ValueError, match="clip 1: tokens and planes are non-NULL and 16-byte aligned"):
        prepared_many.pointer_rows([a, odd])
