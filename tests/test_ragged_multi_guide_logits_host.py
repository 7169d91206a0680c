"""CPU checks of the logits form of the ragged multi-guide step: the three new entry points in the binding and the
library, `hicom_amd.siglip_head_scores_ragged`, the `local_logits` keyword of HIComProjector.forward_ragged_multi_guide, its checks in
front of any device work (fake devices: the tensors live on the CPU, the device checks and the native module are replaced, so nothing can
launch), the plan key that separates the two forms, the host tables of the scores kernel, and the refusals of the C entry points in front
of their launches (made-up aligned addresses that nothing reads before a launch)."""
import ctypes
import inspect
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cases
import hicom_amd
from hicom_amd import encoder
from hicom_amd import native as nv
from hicom_amd import ragged
from hicom_amd import ragged_multi_guide as rmg
from hicom_amd import segments as seg
from hicom_amd.projector import HIComProjector
from host_util import ADDR, EINVAL, EUNSUP

NEW = ("hicom_head_guide_fold_many_fwd", "hicom_head_scores_ragged_fwd", "hicom_compressor_ragged_multiguide_logits_fwd")
D = 1152
SPLITS, COUNTS, MODALS = (1, 4, 1, 8, 1), (1, 3, 5, 2, 4), ("image", "video", "video", "video", "image")      # MIX6


def test_the_three_entry_points_are_bound_and_exported():
    raw = ctypes.CDLL(nv.LIB_PATH)
    for name in NEW:
        assert name in nv.SIGNATURES, name
        assert hasattr(raw, name), name
    assert nv.ABI_VERSION == 16
    assert nv.SIGNATURES["hicom_compressor_ragged_multiguide_logits_fwd"][1][0] == ctypes.POINTER(nv.CompressorRaggedMultiGuideArgs)
    assert nv.SIGNATURES["hicom_head_guide_fold_many_fwd"] == nv.SIGNATURES["hicom_head_guide_fold_fwd"]


def test_the_python_surface_takes_local_logits():
    sig = inspect.signature(HIComProjector.forward_ragged_multi_guide)
    assert sig.parameters["local_logits"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["local_logits"].default is None
    assert sig.parameters["chunks"].kind is inspect.Parameter.KEYWORD_ONLY
    # a public name of the package.  It is NOT a row of __all__: tests/test_ragged_host.py holds __all__ to no name with "ragged" in it.
    assert callable(hicom_amd.siglip_head_scores_ragged) and hicom_amd.siglip_head_scores_ragged is encoder.siglip_head_scores_ragged
    assert "siglip_head_scores_multi" in hicom_amd.__all__
    assert list(inspect.signature(hicom_amd.siglip_head_scores_ragged).parameters)[:5] == ["last_hidden_state", "head", "guide_embeds", "split_sizes",
                                                                                            "guide_counts"]


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
    for mod in (rmg, seg, ragged, encoder):
        monkeypatch.setattr(mod, "nv", NoNative())
    T = sum(SPLITS)
    return SimpleNamespace(ff=torch.zeros(T, 6, 6, D, dtype=torch.bfloat16), g=torch.zeros(sum(COUNTS), D, dtype=torch.bfloat16),
                           ll=torch.zeros(max(COUNTS), T, 6, 6, dtype=torch.float32))


def call(m, h, ll, fe=None, g=None, counts=COUNTS):
    with torch.no_grad():
        return m.forward_ragged_multi_guide(h.ff, fe, h.g if g is None else g, SPLITS, counts, MODALS, None, local_logits=ll)


def test_logits_shape_is_checked_in_front_of_any_device_work(host):
    m = module()
    T = sum(SPLITS)
    for bad in (host.ll[:, :3], host.ll[:4], host.ll.view(5, T, 36), host.ll[0], host.ll.view(5, 6, T, 6), torch.zeros(sum(COUNTS), T, 6, 6), "logits"):
        with pytest.raises(ValueError, match=r"local_logits is \[max Q_i, sum T_i, H, W\] = \[5, 15, 6, 6\]"):
            call(m, host, bad)


def test_logits_dtype_is_checked_in_front_of_any_device_work(host):
    m = module()
    for dt in (torch.float64, torch.bfloat16, torch.float16):
        with pytest.raises(ValueError, match="float32"):
            call(m, host, host.ll.to(dt))


def test_logits_device_is_checked_in_front_of_any_device_work(host):
    with pytest.raises(ValueError, match="device tensor"):
        call(module(), host, host.ll)                      # a CPU tensor, and the real device check of the logits


def test_frames_embed_must_be_none_with_logits(host):
    with pytest.raises(ValueError, match="pass frames_embed=None"):
        call(module(), host, host.ll, fe=host.ff)


def test_the_adaptor_recipe_is_refused(host):
    m = module()
    m.local_compressor.adapt_k = True                      # what seg_recipe reads
    assert seg.seg_recipe(m) == "adaptkv"
    with pytest.raises(NotImplementedError, match="plain release recipe only"):
        call(m, host, host.ll)


def test_the_refusals_of_the_keyed_call_hold_on_the_new_keyword(host):
    m = module()
    with pytest.raises(NotImplementedError, match="float16"):
        call(m, SimpleNamespace(ff=host.ff.half(), g=host.g), host.ll)
    with pytest.raises(ValueError, match="1 <= Q_i <= 32"):
        call(m, host, host.ll, counts=(1, 3, 5, 2, 33))
    with pytest.raises(ValueError, match=r"guide_embeds is \[sum Q_i, E\]"):
        call(m, host, host.ll, g=host.g[:-1])
    with pytest.raises(NotImplementedError, match="float16"):
        call(m.half(), host, host.ll)                      # (last: .half() converts the module in place)


def test_the_scores_entry_refuses_in_front_of_any_device_work(host):
    head = SimpleNamespace()                               # never looked at: every refusal comes first
    f = hicom_amd.siglip_head_scores_ragged
    with pytest.raises(ValueError, match="stacked"):
        f(host.ff[0], head, host.g, SPLITS, COUNTS)
    with pytest.raises(NotImplementedError, match="float16"):
        f(host.ff.half(), head, host.g, SPLITS, COUNTS)
    with pytest.raises(ValueError, match="sum\\(split_sizes\\)"):
        f(host.ff, head, host.g, (1, 4, 1, 8), COUNTS[:4])
    with pytest.raises(ValueError, match="4 guide counts for 5 items"):
        f(host.ff, head, host.g, SPLITS, COUNTS[:4])
    with pytest.raises(ValueError, match="1 <= Q_i <= 32"):
        f(host.ff, head, host.g, SPLITS, (1, 3, 5, 2, 0))
    with pytest.raises(ValueError, match=r"guide_embeds is \[sum Q_i, D\] = \[15, 1152\]"):
        f(host.ff, head, host.g[:14], SPLITS, COUNTS)
    with pytest.raises(NotImplementedError, match="float16"):
        f(host.ff, head, host.g.half(), SPLITS, COUNTS)


def test_the_plan_key_separates_the_two_forms():
    args = (SPLITS, MODALS, 6, 6, D, False, None, torch.float32, 0, None, "plain", False, False, COUNTS)
    keyed, logits = rmg.plan_key(*args), rmg.plan_key(*args, logits=True)
    assert keyed != logits and logits[:len(keyed)] == keyed and logits[-1] == "logits"
    # the keyed form's key is what it was before the logits form: its plans are found again
    assert keyed == (SPLITS, MODALS, 6, 6, D, False, None, torch.float32, 0, 0, "plain", False, False, COUNTS)


def test_the_two_forms_build_their_own_plans(host, monkeypatch):
    """Past the checks (the logits' device check replaced as well): one plan per form in the step's store, the keyed form's first."""
    from hicom_amd import multi_guide as mg
    built = []

    def fake_plan(proj, store, key, build):
        built.append((store, key))
        raise StopIteration                                 # (nothing behind the plan lookup runs on a CPU)
    monkeypatch.setattr(mg, "_require_f32_cuda", lambda name, t: None)
    monkeypatch.setattr(seg, "call_inputs", lambda proj, what, ff, fe, g, nl: ("cpu", ff, fe, g, nl, torch.float32, 0))
    monkeypatch.setattr(seg, "cached_plan", fake_plan)
    m = module()
    for ll in (None, host.ll):
        with pytest.raises(StopIteration):
            call(m, host, ll)
    (s0, k0), (s1, k1) = built
    assert s0 == s1 == rmg.STORE and k0 != k1 and k1[-1] == "logits" and k1[:-1] == k0 and k0[-1] == COUNTS


def test_the_host_tables_of_the_scores_kernel():
    """Tiles are counted per item (ceil(N_i / 32) each): no tile crosses into the next item; B = 1 is the tiling of the multi form."""
    N, Q = (5, 36, 53, 729), (1, 3, 17, 2)
    items, tile_item = encoder.ragged_score_tables(N, Q)
    assert items.dtype == np.int32 and items.shape == (4, 8) and tile_item.dtype == np.int32
    assert items[:, 0].tolist() == [0, 5, 41, 94] and items[:, 1].tolist() == list(N)
    assert items[:, 2].tolist() == [0, 1, 4, 21] and items[:, 3].tolist() == list(Q)
    assert items[:, 4].tolist() == [0, 1, 3, 5] and not items[:, 5:].any()
    assert tile_item.tolist() == [0] + [1] * 2 + [2] * 2 + [3] * 23
    for t, i in enumerate(tile_item):
        first = items[i, 0] + 32 * (t - items[i, 4])
        assert items[i, 0] <= first < items[i, 0] + items[i, 1]
    one, tiles = encoder.ragged_score_tables((729,), (3,))
    assert one[0].tolist() == [0, 729, 0, 3, 0, 0, 0, 0] and tiles.tolist() == [0] * 23


def test_the_table_cache_is_bounded_and_keeps_the_latest(monkeypatch):
    made = []
    monkeypatch.setattr(encoder, "_score_tables", {})
    monkeypatch.setattr(encoder, "ragged_score_tables", lambda n, q: (made.append((tuple(n), tuple(q))), (np.zeros((1, 8), np.int32), np.zeros(1, np.int32)))[1])
    for k in range(encoder.MAX_SCORE_TABLES + 3):
        encoder._device_score_tables((k + 1,), (1,), "cpu")
        encoder._device_score_tables((1,), (1,), "cpu")                          # the mix in steady use: made once, never dropped
    assert len(encoder._score_tables) == encoder.MAX_SCORE_TABLES
    assert made.count(((1,), (1,))) == 1 and len(made) == encoder.MAX_SCORE_TABLES + 3
    a = encoder._device_score_tables((1,), (1,), "cpu")
    assert a[0] is encoder._device_score_tables((1,), (1,), "cpu")[0]


# ---- the C entry points refuse in front of their launches -----------------------------------------------------------------------------------
def fold_many(M=15, D_=D, inter=200, ldu=256, ws_bytes=1 << 40, w2=ADDR, u_hi=ADDR):
    r = nv.lib().hicom_head_guide_fold_many_fwd(w2, ADDR, D_, inter, ADDR, M, u_hi, ADDR, ldu, ADDR, ADDR, ADDR, ws_bytes, None)
    return int(r), nv.lib().hicom_last_error().decode()


def scores(D_=D, kpad=256, ld=256, ldu=256, B=4, ntiles=29, q_max=17, q_stride=823, x=ADDR, items=ADDR, tile_item=ADDR, logits=ADDR):
    r = nv.lib().hicom_head_scores_ragged_fwd(x, ADDR, ld, D_, kpad, ADDR, ADDR, ADDR, ldu, ADDR, ADDR, items, tile_item, B, ntiles, q_max, logits, q_stride,
                                              None)
    return int(r), nv.lib().hicom_last_error().decode()


REFUSALS = {
    "fold: M = 0": (lambda: fold_many(M=0), EUNSUP, "1 <= M <= 4096"),
    "fold: M = 4097": (lambda: fold_many(M=4097), EUNSUP, "1 <= M <= 4096"),
    "fold: NULL weight": (lambda: fold_many(w2=None), EINVAL, "NULL pointer"),
    "fold: D = 4096": (lambda: fold_many(D_=4096), EUNSUP, "D=4096"),
    "fold: narrow planes": (lambda: fold_many(ldu=192), EINVAL, "ldu=192"),
    "fold: small workspace": (lambda: fold_many(ws_bytes=16 * 15 * 256 * 4 - 4), EINVAL, "workspace of 245760 bytes"),
    "fold: misaligned planes": (lambda: fold_many(u_hi=ADDR + 8), EINVAL, "aligned planes"),
    "scores: NULL items": (lambda: scores(items=None), EINVAL, "NULL pointer"),
    "scores: NULL tile_item": (lambda: scores(tile_item=None), EINVAL, "NULL pointer"),
    "scores: NULL logits": (lambda: scores(logits=None), EINVAL, "NULL pointer"),
    "scores: B = 0": (lambda: scores(B=0), EUNSUP, "B=0"),
    "scores: q_max = 0": (lambda: scores(q_max=0), EUNSUP, "q_max=0"),
    "scores: q_max = 33": (lambda: scores(q_max=33), EUNSUP, "q_max=33"),
    "scores: fewer tiles than items": (lambda: scores(ntiles=3), EUNSUP, "ntiles=3"),
    "scores: D = 1100": (lambda: scores(D_=1100), EUNSUP, "multiple of 128"),
    "scores: kpad = 200": (lambda: scores(kpad=200), EINVAL, "multiple of 64"),
    "scores: ld < kpad": (lambda: scores(kpad=320, ld=256, ldu=384), EINVAL, ">= kpad"),
    "scores: narrow U planes": (lambda: scores(kpad=320, ld=320, ldu=320), EINVAL, "rounded up to 128"),
    "scores: rows overlap": (lambda: scores(q_stride=800), EINVAL, "q_stride=800"),      # 29 tiles of 4 items hold more than 800 tokens
    "scores: misaligned x": (lambda: scores(x=ADDR + 8), EINVAL, "aligned"),
    "scores: misaligned items": (lambda: scores(items=ADDR + 4), EINVAL, "device table"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_c_entry_points_refuse_in_front_of_the_launch(name):
    fn, code, text = REFUSALS[name]
    got, msg = fn()
    assert got == code and text in msg, (got, msg)


IMAGE, CLIP4, CLIP8 = (1, 1, 0, 0, 0, 1, 32), (4, 4, 0, 0, 0, 1, 32), (8, 4, 0, 0, 0, 1, 32)


def step_block(counts=COUNTS, **over):
    """A block of the MIX6 batch (6 x 6 grid, windows of 3 x 3, hidden 64) that passes every check of the keyed step's fwd."""
    items = [IMAGE, CLIP4, IMAGE, CLIP8, IMAGE]
    a = nv.CompressorRaggedMultiGuideArgs()
    a._items = (nv.RaggedItem * len(items))(*[nv.RaggedItem(*d) for d in items])
    a._counts = (ctypes.c_int32 * len(counts))(*counts)
    a.B, a.H, a.W, a.E, a.hidden, a.ks, a.nh, a.P = len(items), 6, 6, D, 64, 3, 9, 0
    a.chunks, a.out_dt, a.l_scale = 3, nv.DT_F32, 0.125
    a.items, a.guide_counts, a.n_guide_counts = a._items, a._counts, len(counts)
    for f in ("ff", "guide", "out", "lw0_f16", "lb0", "lw2_f16", "lb2", "wq", "bq", "wk", "wv", "bv", "wo", "bo", "gw0", "gb0", "gw2", "gb2"):
        setattr(a, f, ADDR)
    a.ldo, a.ws, a.ws_bytes = a.hidden, ADDR, 1 << 40
    for k, v in over.items():
        setattr(a, k, v)
    return a


def step(a, ll=ADDR, q_stride=540):
    L = nv.lib()
    r = L.hicom_compressor_ragged_multiguide_logits_fwd(None if a is None else ctypes.byref(a), ll, q_stride)
    return int(r), L.hicom_last_error().decode()


def test_the_step_refuses_in_front_of_its_first_launch():
    """15 frames of 6 x 6: 540 tokens.  Every case breaks one rule, so none launches."""
    assert step(None) == (EINVAL, "compressor_ragged_multiguide: NULL arguments")
    got, msg = step(step_block(), ll=None)
    assert got == EINVAL and "local_logits" in msg
    got, msg = step(step_block(), q_stride=539)
    assert got == EINVAL and "q_stride=539" in msg and "540 tokens" in msg
    got, msg = step(step_block(counts=(1, 3, 5, 2, 33)))
    assert got == EUNSUP and "Q=33 guides" in msg
    got, msg = step(step_block(ff=None))
    assert got == EINVAL and "NULL pointer" in msg
    # one guide per item: a single plane, no stride to check; a misaligned frames_embed is not looked at (the next refusal is the output's)
    got, msg = step(step_block(counts=(1, 1, 1, 1, 1), fe=ADDR + 2, ldo=63), q_stride=0)
    assert got == EINVAL and "output layout" in msg
    got, msg = step(step_block(ws_bytes=4096))
    assert got == EINVAL and "workspace of" in msg
