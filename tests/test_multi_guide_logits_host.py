"""CPU checks of the logits form of the multi-guide step: the four new entry points in the binding and the library,
the `local_logits` keyword of HIComProjector.forward_multi_guide, its checks in front of any device work (fake devices: the tensors live
on the CPU, the device checks and the native module are replaced, so nothing can launch), the plan key that separates the two forms, and
the refusals of the C entry points in front of their launches."""
import ctypes
import inspect
from types import SimpleNamespace

import pytest
import torch

import cases
import hicom_amd
from hicom_amd import multi_guide as mg
from hicom_amd import native as nv
from hicom_amd import segments as seg
from hicom_amd.projector import HIComProjector
from host_util import ADDR, EINVAL, EUNSUP

NEW = ("hicom_head_guide_fold_fwd", "hicom_head_scores_multi_fwd", "hicom_multi_guide_local_logits_fwd", "hicom_compressor_multiguide_logits_fwd")
D = 1152


def test_the_four_entry_points_are_bound_and_exported():
    raw = ctypes.CDLL(nv.LIB_PATH)
    for name in NEW:
        assert name in nv.SIGNATURES, name
        assert hasattr(raw, name), name
    assert nv.ABI_VERSION == 16
    assert nv.SIGNATURES["hicom_compressor_multiguide_logits_fwd"][1][0] == ctypes.POINTER(nv.CompressorMultiGuideArgs)
    assert nv.SIGNATURES["hicom_multi_guide_local_logits_fwd"][1][3:6] == [nv.Axis] * 3


def test_the_python_surface_takes_local_logits():
    sig = inspect.signature(HIComProjector.forward_multi_guide)
    assert sig.parameters["local_logits"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["local_logits"].default is None
    assert callable(hicom_amd.siglip_head_scores_multi) and "siglip_head_scores_multi" in hicom_amd.__all__


class NoNative:
    """Stands in for hicom_amd.native: any use is a device call in front of a refusal."""
    def __getattr__(self, name):
        raise AssertionError(f"native.{name} reached before the refusal")


def module(**over):
    cfg = SimpleNamespace(**{**cases.DEFAULT_CFG, **over})
    return hicom_amd.build_vision_projector(cfg).to(torch.bfloat16).eval()


@pytest.fixture
def host(monkeypatch):
    """CPU tensors pass for device tensors; no native call may happen."""
    import hicom_amd.projector as pj
    monkeypatch.setattr(pj, "_require_bf16_cuda", lambda name, t: None if t.dtype == torch.bfloat16 else (_ for _ in ()).throw(
        NotImplementedError(f"{name}: {t.dtype}")))
    monkeypatch.setattr(mg, "nv", NoNative())
    monkeypatch.setattr(seg, "nv", NoNative())
    return SimpleNamespace(ff=torch.zeros(4, 6, 6, D, dtype=torch.bfloat16), g=torch.zeros(3, D, dtype=torch.bfloat16),
                           ll=torch.zeros(3, 4, 6, 6, dtype=torch.float32))


def call(m, h, ll, fe=None, g=None):
    with torch.no_grad():
        return m.forward_multi_guide(h.ff, fe, h.g if g is None else g, "video", None, local_logits=ll)


def test_logits_shape_is_checked_in_front_of_any_device_work(host):
    m = module()
    for bad in (host.ll[:, :3], host.ll.view(3, 4, 36), host.ll[0], host.ll.view(3, 6, 4, 6), "logits"):
        with pytest.raises(ValueError, match=r"local_logits is \[Q, T, H, W\]"):
            call(m, host, bad)


def test_logits_dtype_is_checked_in_front_of_any_device_work(host):
    m = module()
    for dt in (torch.float64, torch.bfloat16, torch.float16):
        with pytest.raises(ValueError, match="float32"):
            call(m, host, host.ll.to(dt))


def test_logits_device_is_checked_in_front_of_any_device_work(host):
    with pytest.raises(ValueError, match="device tensor"):
        call(module(), host, host.ll)                      # a CPU tensor, and the real device check of the logits


def test_guide_count_of_guides_and_logits_must_agree(host):
    m = module()
    with pytest.raises(ValueError, match="holds 2 guides, guide_embeds 3"):
        call(m, host, host.ll[:2])
    with pytest.raises(ValueError, match="holds 3 guides, guide_embeds 5"):
        call(m, host, host.ll, g=torch.zeros(5, D, dtype=torch.bfloat16))


def test_frames_embed_must_be_none_with_logits(host):
    with pytest.raises(ValueError, match="pass frames_embed=None"):
        call(module(), host, host.ll, fe=host.ff)


def test_the_adaptor_recipe_is_refused(host):
    m = module(mm_local_adapt_k=True) if "mm_local_adapt_k" in cases.DEFAULT_CFG else None
    if m is None:
        m = module()
        m.local_compressor.adapt_k = True                  # what seg_recipe reads
    assert seg.seg_recipe(m) == "adaptkv"
    with pytest.raises(NotImplementedError, match="plain release recipe only"):
        call(m, host, host.ll)


def test_the_refusals_of_the_keyed_call_hold_on_the_new_keyword(host):
    m = module()
    with pytest.raises(NotImplementedError, match="float16"):
        call(m, SimpleNamespace(ff=host.ff.half(), g=host.g), host.ll)
    with pytest.raises(NotImplementedError, match="float16"):
        call(m.half(), host, host.ll)


def test_the_plan_key_separates_the_two_forms():
    args = (3, 4, 6, 6, D, False, "video", None, torch.float32, 0, None)
    keyed, logits = mg.plan_key(*args), mg.plan_key(*args, logits=True)
    assert keyed != logits and logits[:len(keyed)] == keyed and logits[-1] == "logits"
    # the keyed form's key is what it was before the logits form: its plans are found again
    assert keyed == (3, 4, 6, 6, D, False, "video", None, torch.float32, 0, 0)


def test_the_two_forms_build_their_own_plans(host, monkeypatch):
    """Past the checks (the logits' device check replaced as well): one plan per form in the step's store, the keyed form's first."""
    built = []

    def fake_plan(proj, store, key, build):
        built.append(key)
        raise StopIteration                                 # (nothing behind the plan lookup runs on a CPU)
    monkeypatch.setattr(mg, "_require_f32_cuda", lambda name, t: None)
    monkeypatch.setattr(seg, "call_inputs", lambda proj, what, ff, fe, g, nl: ("cpu", ff, fe, g, nl, torch.float32, 0))
    monkeypatch.setattr(seg, "cached_plan", fake_plan)
    m = module()
    for ll in (None, host.ll):
        with pytest.raises(StopIteration):
            call(m, host, ll)
    assert len(built) == 2 and built[0] != built[1] and built[1][-1] == "logits" and built[0][-1] != "logits"


# ---- the C entry points refuse in front of their launches -----------------------------------------------------------------------------------
def axis(n, k):
    return nv.Axis(n, k, n // k, n // k)


def local(Q=3, nwin=4, q_stride=144, at=None, ay=None, ax=None, value=ADDR, logits=ADDR, out=ADDR):
    r = nv.lib().hicom_multi_guide_local_logits_fwd(value, logits, q_stride, at or axis(4, 4), ay or axis(6, 3), ax or axis(6, 3), Q, nwin, 0.03, out, None)
    return int(r), nv.lib().hicom_last_error().decode()


def scores(M=144, D_=D, kpad=256, ld=256, ldu=256, Q=3, q_stride=144, x=ADDR):
    r = nv.lib().hicom_head_scores_multi_fwd(x, ADDR, ld, M, D_, kpad, ADDR, ADDR, ADDR, ldu, ADDR, ADDR, Q, ADDR, q_stride, None)
    return int(r), nv.lib().hicom_last_error().decode()


REFUSALS = {
    "local: Q = 0": (lambda: local(Q=0), EUNSUP, "1 <= Q <= 32"),
    "local: Q = 33": (lambda: local(Q=33), EUNSUP, "1 <= Q <= 32"),
    "local: inexact partition": (lambda: local(ay=nv.Axis(7, 3, 2, 2)), EUNSUP, "exact window partition"),
    "local: window of 100 tokens": (lambda: local(at=axis(4, 4), ay=axis(10, 5), ax=axis(10, 5), q_stride=400), EUNSUP, "<= 64 tokens"),
    "local: wrong window count": (lambda: local(nwin=5), EINVAL, "nwin=5"),
    "local: planes overlap": (lambda: local(q_stride=100), EINVAL, "q_stride=100"),
    "local: NULL logits": (lambda: local(logits=None), EINVAL, "NULL pointer"),
    "local: misaligned value": (lambda: local(value=ADDR + 8), EINVAL, "aligned"),
    "scores: Q = 33": (lambda: scores(Q=33), EUNSUP, "1 <= Q <= 32"),
    "scores: D = 1100": (lambda: scores(D_=1100), EUNSUP, "multiple of 128"),
    "scores: kpad = 200": (lambda: scores(kpad=200), EINVAL, "multiple of 64"),
    "scores: ld < kpad": (lambda: scores(kpad=320, ld=256, ldu=384), EINVAL, ">= kpad"),
    "scores: narrow U planes": (lambda: scores(kpad=320, ld=320, ldu=320), EINVAL, "rounded up to 128"),
    "scores: rows overlap": (lambda: scores(q_stride=100), EINVAL, "q_stride=100"),
    "scores: M = 0": (lambda: scores(M=0), EUNSUP, "M=0"),
    "scores: misaligned x": (lambda: scores(x=ADDR + 8), EINVAL, "aligned"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_c_entry_points_refuse_in_front_of_the_launch(name):
    fn, code, text = REFUSALS[name]
    got, msg = fn()
    assert got == code and text in msg, (got, msg)


def test_the_step_refuses_missing_logits_and_overlapping_planes():
    a = nv.CompressorMultiGuideArgs()
    a.Q, a.T, a.H, a.W, a.E, a.hidden, a.kt, a.ks, a.nh = 3, 4, 6, 6, D, 896, 4, 3, 9
    L = nv.lib()
    assert L.hicom_compressor_multiguide_logits_fwd(ctypes.byref(a), None, 144) == EINVAL and "local_logits" in L.hicom_last_error().decode()
    assert L.hicom_compressor_multiguide_logits_fwd(ctypes.byref(a), ADDR, 100) == EINVAL and "q_stride=100" in L.hicom_last_error().decode()
    assert L.hicom_compressor_multiguide_logits_fwd(None, ADDR, 144) == EINVAL
    a.Q = 33
    assert L.hicom_compressor_multiguide_logits_fwd(ctypes.byref(a), ADDR, 144) == EUNSUP and "1 <= Q <= 32" in L.hicom_last_error().decode()
