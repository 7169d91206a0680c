"""CPU checks of the logits form of the ragged step and its training step: the two new entry points in the header, the
binding and the library, the `local_logits` keyword of HIComProjector.forward_ragged / forward_ragged_train, and its refusals in front of
any device work (fake devices: the tensors live on the CPU, the device checks and the native module are replaced, so nothing can launch),
and the refusals of the C entry points in front of their launches (made-up aligned addresses that nothing reads before a launch).
Every test here fails without the feature."""
import ctypes
import inspect
import re
from types import SimpleNamespace

import pytest
import torch

import cases
import hicom_amd
from hicom_amd import native as nv
from hicom_amd import ragged, ragged_train
from hicom_amd import segments as seg
from hicom_amd.projector import HIComProjector
from host_util import ADDR, EINVAL, HEADER

NEW = {"hicom_compressor_ragged_logits_fwd": 2, "hicom_compressor_ragged_local_logits_bwd": 6}
D = cases.D
SPLITS, MODALS = (1, 4, 1, 8, 1), ("image", "video", "video", "video", "image")


def test_entry_points_are_declared_exported_and_bound():
    raw = ctypes.CDLL(nv.LIB_PATH)                        # loading needs no GPU; no compute call is made
    for name, n_args in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", HEADER)
        assert m, f"{name} is not declared in include/hicom_hip.h"
        assert name in nv.EXPORTS and hasattr(raw, name)
        fn = getattr(nv.lib(), name)
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args == len(fn.argtypes) and fn.restype is ctypes.c_int
        assert fn.argtypes[0] == ctypes.POINTER(nv.CompressorRaggedArgs)
    assert nv.ABI_VERSION == 16 and "#define HICOM_ABI_VERSION 16" in HEADER


def test_the_python_surface_takes_local_logits():
    for entry in (HIComProjector.forward_ragged, HIComProjector.forward_ragged_train):
        p = inspect.signature(entry).parameters["local_logits"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert "global share" in HIComProjector.forward_ragged_train.__doc__.lower()


class NoNative:
    """Stands in for hicom_amd.native: any use is a device call in front of a refusal."""
    def __getattr__(self, name):
        raise AssertionError(f"native.{name} reached before the refusal")


def module(recipe="local43_global32", **over):
    return hicom_amd.build_vision_projector(SimpleNamespace(**{**cases.DEFAULT_CFG, "hidden_size": 64, "mm_projector_type": recipe, **over})).to(torch.bfloat16)


@pytest.fixture
def host(monkeypatch):
    """CPU tensors pass for device tensors; no native call may happen."""
    import hicom_amd.projector as pj
    monkeypatch.setattr(pj, "_require_bf16_cuda", lambda name, t: None if t.dtype == torch.bfloat16 else (_ for _ in ()).throw(
        NotImplementedError(f"{name}: {t.dtype}")))
    for mod in (seg, ragged, ragged_train):
        monkeypatch.setattr(mod, "nv", NoNative())
    T = sum(SPLITS)
    return SimpleNamespace(ff=torch.zeros(T, 6, 6, D, dtype=torch.bfloat16), g=torch.zeros(len(SPLITS), D, dtype=torch.bfloat16),
                           ll=torch.zeros(T, 6, 6, dtype=torch.float32))


def infer(m, h, ll, fe=None):
    with torch.no_grad():
        return m.forward_ragged(h.ff, fe, h.g, SPLITS, MODALS, None, local_logits=ll)


def train(m, h, ll, fe=None, **kw):
    return m.forward_ragged_train(h.ff, fe, h.g, SPLITS, MODALS, None, local_logits=ll, **kw)


CALLS = {"forward_ragged": infer, "forward_ragged_train": train}


@pytest.mark.parametrize("entry", list(CALLS))
def test_frames_embed_must_be_none_with_logits(host, entry):
    with pytest.raises(ValueError, match="local_logits replaces frames_embed: pass frames_embed=None"):
        CALLS[entry](module(), host, host.ll, fe=host.ff)


@pytest.mark.parametrize("entry", list(CALLS))
def test_shape_dtype_and_device_are_checked_in_front_of_any_device_work(host, entry):
    m, T = module(), sum(SPLITS)
    for bad in (host.ll[:3], host.ll[:, :3], host.ll.view(T, 36), host.ll.view(1, 1, T, 6, 6), torch.zeros(2, T, 6, 6), torch.zeros(6, T, 6), "logits"):
        with pytest.raises(ValueError, match=r"local_logits is \[sum T_i, H, W\] = \[15, 6, 6\]"):
            CALLS[entry](m, host, bad)
    for dt in (torch.float64, torch.bfloat16, torch.float16):
        with pytest.raises(ValueError, match="float32"):
            CALLS[entry](m, host, host.ll.to(dt))
    for ll in (host.ll, host.ll[None]):                    # CPU tensors of the right shape, and the real device check of the logits
        with pytest.raises(ValueError, match="device tensor"):
            CALLS[entry](m, host, ll)
    assert "_ragged_plans" not in m.__dict__


@pytest.mark.parametrize("entry", list(CALLS))
def test_the_adaptor_recipe_refuses_local_logits(host, entry):
    m = module("local43_adaptkv_global32")
    kw = {"adaptors": True} if entry == "forward_ragged_train" else {}
    with pytest.raises(NotImplementedError, match="local_logits has no form on the k / v adaptor recipe.*not linear in frames_embed"):
        CALLS[entry](m, host, host.ll, **kw)
    assert "_ragged_plans" not in m.__dict__


def test_scores_requiring_grad_without_input_grads_raise_like_the_other_inputs(host):
    m = module()
    for extra in ({}, {"input_grads": False}):
        with pytest.raises(NotImplementedError, match=r"local_logits.*input_grads=True") as e:
            train(m, host, host.ll.clone().requires_grad_(True), **extra)
        assert "forward()" in str(e.value) and "_ragged_plans" not in m.__dict__


def test_the_inference_call_builds_no_graph_through_the_scores(host, monkeypatch):
    from hicom_amd import multi_guide as mg
    monkeypatch.setattr(mg, "_require_f32_cuda", lambda name, t: None)
    m = module().requires_grad_(False)
    with pytest.raises(RuntimeError, match="local_logits requires grad"):
        m.forward_ragged(host.ff, None, host.g, SPLITS, MODALS, None, local_logits=host.ll.clone().requires_grad_(True))


def test_the_refusals_of_the_keyed_call_hold_on_the_new_keyword(host):
    m = module()
    with pytest.raises(ValueError, match=r"sum\(split_sizes\)"):
        with torch.no_grad():
            m.forward_ragged(host.ff, None, host.g, (1, 4, 1, 8), MODALS[:4], None, local_logits=host.ll)
    with pytest.raises(NotImplementedError, match="clip-scale"):
        train(module(use_clip_scale="local"), host, host.ll)


# ---- the C entry points refuse in front of their launches -----------------------------------------------------------------------------------
def block(T1=8, **over):
    a = nv.CompressorRaggedArgs()
    a._items = (nv.RaggedItem * 2)(nv.RaggedItem(1, 1, 0, 0, 0, 1, 32), nv.RaggedItem(T1, 4, 0, 0, 0, 1, 32))
    a.B, a.H, a.W, a.E, a.hidden, a.ks, a.nh, a.chunks, a.items = 2, 6, 6, D, 64, 3, 9, 1, a._items
    a.l_scale = D ** -0.5
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_the_c_entry_points_refuse_without_a_device():
    """chunks = 1: the layout needs no CU count, so nothing here can have asked for a device."""
    lib = nv.lib()
    err = lambda: lib.hicom_last_error().decode()
    a = block()
    assert lib.hicom_compressor_ragged_logits_fwd(None, ADDR) == EINVAL and "NULL arguments" in err()
    assert lib.hicom_compressor_ragged_logits_fwd(ctypes.byref(a), None) == EINVAL and "local_logits" in err()
    assert lib.hicom_compressor_ragged_logits_fwd(ctypes.byref(a), ADDR + 2) == EINVAL and "local_logits" in err()
    # a stale, misaligned frames_embed is not looked at: the next refusal is the NULL frames_feature
    assert lib.hicom_compressor_ragged_logits_fwd(ctypes.byref(block(fe=ADDR + 2)), ADDR) == EINVAL and "NULL pointer" in err()
    bwd = lib.hicom_compressor_ragged_local_logits_bwd
    assert bwd(ctypes.byref(a), None, None, None, None, None) == EINVAL and "compressor_ragged_local_logits_bwd: NULL pointer" in err()
    assert bwd(ctypes.byref(a), ADDR, ADDR, ADDR, None, ADDR) == EINVAL and "NULL pointer" in err()          # (dlogits is not optional)
    assert bwd(ctypes.byref(a), ADDR, ADDR, ADDR + 4, 2 * ADDR, None) == EINVAL and "aligned" in err()
    assert bwd(ctypes.byref(a), ADDR, ADDR, ADDR, ADDR, None) == EINVAL and "overwrite" in err()
    assert bwd(ctypes.byref(a), ADDR, ADDR, ADDR, 2 * ADDR, None) == EINVAL and "workspace" in err()         # all given, no workspace
    b = block(T1=6)                                        # 6 frames under a temporal window of 4: no exact partition
    assert bwd(ctypes.byref(b), ADDR, ADDR, ADDR, 2 * ADDR, None) < 0 and re.search("item 1.*partition", err())
    assert lib.hicom_compressor_ragged_logits_fwd(ctypes.byref(b), ADDR) < 0 and re.search("item 1.*partition", err())
