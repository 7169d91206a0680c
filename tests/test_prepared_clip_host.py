"""CPU checks of the host side of prepared clips (csrc/multi_guide.hip: hicom_clip_adapt_prepare_*, hicom_compressor_multiguide_adapt_*;
hicom_amd/prepared.py): the new symbols, the new argument struct as the host C compiler lays it out against its ctypes mirror, the
workspace rule (the planes are the caller's: the adapt entry point asks for what the plain one asks for), the refusals of the C entry
points in front of any device call, and the Python refusals that need no device.

As in tests/test_multi_guide_host.py: with chunks > 0 the workspace functions and every check in front of the first launch are pure host
code, pointer fields are made-up aligned addresses that nothing reads before a launch, and every *_fwd case breaks one rule, so none
launches."""
import ctypes

import pytest
import torch

import cases
import host_util
from hicom_amd import native as nv
from host_util import ADDR, EINVAL, EUNSUP

POINTERS = ("ff", "fe", "guide", "out", "newline", "lw0_f16", "lb0", "lw2_f16", "lb2", "wq", "bq", "wk", "wv", "bv", "wo", "bo", "gw0", "gb0", "gw2", "gb2",
            "pe", "kpe")
STORES = ("_prepared_plans", "_prepare_plans", "_multi_guide_plans")


def block(fwd=False, ky=ADDR, vy=ADDR, **over):
    """A valid block: Q = 3 guides on a 4 x 6 x 6 clip, windows 4 x 3 x 3, hidden 896, fp32 rows, 3 token chunks, both planes given."""
    args = nv.CompressorMultiGuideAdaptArgs()
    a = args.base
    a.Q, a.T, a.H, a.W, a.E, a.hidden, a.kt, a.ks, a.nh, a.P = 3, 4, 6, 6, 1152, 896, 4, 3, 9, 0
    a.chunks, a.out_dt, a.l_scale = 3, nv.DT_F32, 0.125
    if fwd:
        for f in POINTERS:
            setattr(a, f, ADDR)
        a.P, a.t_index0, a.y_index0, a.x_index0 = 28, 0, 16, 22
        a.ldo, a.ws, a.ws_bytes = a.hidden, ADDR, 1 << 40
        a.global_row0, a.n_global_rows, a.item_rows = 4, 32, 36
        for d in (args.ak, args.av):
            d.gamma = d.beta = d.alpha = ADDR
        args.alpha_dt, args.eps = nv.DT_BF16, 1e-5
    args.ky, args.vy = ky, vy
    for k, v in over.items():
        setattr(a, k, v)
    return args


def call(fn, args):
    r = getattr(nv.lib(), f"hicom_compressor_multiguide_adapt_{fn}")(None if args is None else ctypes.byref(args))
    return int(r), nv.lib().hicom_last_error().decode()


@pytest.mark.parametrize("over", [dict(), dict(out_dt=nv.DT_BF16, P=28), dict(T=1, kt=1, H=9, W=9), dict(T=8, chunks=9)],
                         ids=["clip_f32", "clip_bf16_pos", "image_9x9", "clip_T8_chunks9"])
def test_workspace_is_the_plain_entry_points(over):
    """The planes are the caller's: nothing token-sized is added, whichever planes are given."""
    for q in (1, 2, 3, 4, 5, 8, 32):
        args = block(Q=q, **over)
        plain = nv.lib().hicom_compressor_multiguide_workspace_bytes(ctypes.byref(args.base))
        assert plain > 0
        for ky, vy in ((ADDR, ADDR), (ADDR, None), (None, ADDR)):
            args.ky, args.vy = ky, vy
            assert call("workspace_bytes", args)[0] == plain == nv.compressor_multiguide_workspace(args)


REFUSALS = {
    "both planes NULL": ("fwd", dict(fwd=True, ky=None, vy=None), EINVAL, "neither stream has a prepared plane"),
    "Q = 0": ("fwd", dict(fwd=True, Q=0), EUNSUP, "Q=0 guides (1 <= Q <= 32 per call)"),
    "Q = 33": ("fwd", dict(fwd=True, Q=33), EUNSUP, "Q=33 guides (1 <= Q <= 32 per call)"),
    "workspace: Q = 0": ("workspace_bytes", dict(Q=0), EUNSUP, "Q=0 guides (1 <= Q <= 32 per call)"),
    "workspace: Q = 33": ("workspace_bytes", dict(Q=33), EUNSUP, "Q=33 guides (1 <= Q <= 32 per call)"),
    "ky not 16-byte aligned": ("fwd", dict(fwd=True, ky=ADDR + 8), EINVAL, "16-byte aligned planes"),
    "vy not 16-byte aligned": ("fwd", dict(fwd=True, vy=ADDR + 2), EINVAL, "16-byte aligned planes"),
    "NULL block": ("fwd", None, EINVAL, "NULL arguments"),
    "NULL block, workspace": ("workspace_bytes", None, EINVAL, "NULL arguments"),
    "the plain checks come first": ("fwd", dict(fwd=True, ky=None, vy=None, hidden=100, ldo=100), EUNSUP, "hidden=100 (multiple of 64"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_c_refusals_in_front_of_any_device_call(name):
    fn, kw, code, needle = REFUSALS[name]
    got, msg = call(fn, None if kw is None else block(**kw))
    assert got == code, (got, msg)
    assert msg.startswith("compressor_multiguide: ") and needle in msg, msg


def test_c_refusals_missing_adaptor_weights_and_alpha_dtype():
    args = block(fwd=True)
    args.av.gamma = None
    assert call("fwd", args) == (EINVAL, "compressor_multiguide: adaptor weights")
    args = block(fwd=True, ky=None)                  # the key stream is not adapted: its descriptor is not looked at
    args.ak.gamma = args.ak.beta = args.ak.alpha = None
    args.alpha_dt = nv.DT_F16
    assert call("fwd", args) == (EINVAL, "compressor_multiguide: alpha dtype 2 (bf16 | f32)")


def adaptors(k=True, v=True):
    ak, av = nv.SegAdaptor(), nv.SegAdaptor()
    for d, on in ((ak, k), (av, v)):
        if on:
            d.w0 = d.w2_f16 = ADDR
    return ak, av


def prepare_ws(N, E, ak, av):
    r = nv.lib().hicom_clip_adapt_prepare_workspace_bytes(N, E, ctypes.byref(ak), ctypes.byref(av))
    return int(r), nv.lib().hicom_last_error().decode()


def prepare_fwd(N, E, ak, av, key_x=ADDR, ff=ADDR, ky=ADDR, vy=ADDR, ws=ADDR, ws_bytes=1 << 40):
    r = nv.lib().hicom_clip_adapt_prepare_fwd(key_x, ff, N, E, ctypes.byref(ak), ctypes.byref(av), ky, vy, ws, ws_bytes, None)
    return int(r), nv.lib().hicom_last_error().decode()


def test_prepare_workspace_is_one_hidden_plane_per_adapted_stream():
    N, E = 4 * 36, 1152
    plane = N * E * 2
    assert plane % 256 == 0
    assert prepare_ws(N, E, *adaptors())[0] == 2 * plane
    assert prepare_ws(N, E, *adaptors(v=False))[0] == plane == prepare_ws(N, E, *adaptors(k=False))[0]
    assert prepare_ws(81, E, *adaptors())[0] == 2 * ((81 * E * 2 + 255) // 256 * 256)
    assert nv.clip_adapt_prepare_workspace(N, E, *adaptors()) == 2 * plane


def test_prepare_refusals_in_front_of_any_device_call():
    ak, av = adaptors()
    for f in (prepare_ws, prepare_fwd):
        assert f(144, 100, ak, av) == (EUNSUP, "clip_adapt_prepare: adaptor width 100 (multiple of 64)")
        assert f(144, 1152, *adaptors(k=False, v=False)) == (
            EINVAL, "clip_adapt_prepare: neither stream has an adaptor (the plain entry point runs that recipe)")
        assert f(0, 1152, ak, av) == (EINVAL, "clip_adapt_prepare: bad shape")
        code, msg = f(1 << 22, 1152, ak, av)            # 2^22 x 1152 >= 2^32: the dense GEMM's operand limit
        assert code == EUNSUP and "below 2^32 elements" in msg
    with pytest.raises(NotImplementedError, match="prepare_clip: .*adaptor width 100"):
        nv.clip_adapt_prepare_workspace(144, 100, ak, av)
    assert prepare_fwd(144, 1152, ak, av, ky=None) == (EINVAL, "clip_adapt_prepare: NULL pointer")
    assert prepare_fwd(144, 1152, ak, av, ff=None) == (EINVAL, "clip_adapt_prepare: NULL pointer")
    assert prepare_fwd(144, 1152, ak, av, ky=ADDR + 8) == (EINVAL, "clip_adapt_prepare: 16-byte aligned tokens and planes")
    assert prepare_fwd(144, 1152, ak, av, ws_bytes=4096) == (EINVAL, f"clip_adapt_prepare: workspace of {2 * 144 * 1152 * 2} bytes, 256-byte aligned")
    ak.w2_f16 = None
    assert prepare_fwd(144, 1152, ak, av) == (EINVAL, "clip_adapt_prepare: adaptor weights")


# ---- Python refusals that need no device ------------------------------------------------------------------------------------------------
def module(ptype="local43_adaptkv_global32", use_guide="direct", dtype=torch.bfloat16):
    return host_util.module(ptype, use_guide, dtype, hidden_size=896)


def no_plans(m):
    return not any(m.__dict__.get(s) for s in STORES)


def test_python_refusals_without_a_device_leave_no_plan():
    ff = torch.zeros((4, 6, 6, cases.D), dtype=torch.bfloat16)
    g = torch.zeros((3, cases.D), dtype=torch.bfloat16)
    with torch.no_grad():
        for m in (module(use_guide="coarse"), module("local43_adaptqkv_global32", "fine"), module("local43_adaptkv_global32_adaptg")):
            with pytest.raises(NotImplementedError, match="two release recipes"):
                m.prepare_clip(ff, ff, "video")
            assert no_plans(m)
        half = module(dtype=torch.float16)
        with pytest.raises(NotImplementedError, match="float16"):
            half.prepare_clip(ff.half(), ff.half(), "video")
        assert no_plans(half)
        m = module()
        with pytest.raises(NotImplementedError, match="anyres"):
            m.prepare_clip({"base": None, "patch": ff[0]}, None, "image")
        with pytest.raises(nv.HicomNativeError, match="GPU only"):
            m.prepare_clip(ff, ff, "video")
        with pytest.raises(nv.HicomNativeError, match="GPU only"):
            m.prepare_clip(ff, None, "video")
        with pytest.raises(ValueError, match="prepare_clip returned"):
            m.forward_prepared(ff, g)
        assert no_plans(m)
        plain = module("local43_global32")
        with pytest.raises(nv.HicomNativeError, match="GPU only"):
            plain.prepare_clip(ff, ff, "video")
        assert no_plans(plain)
