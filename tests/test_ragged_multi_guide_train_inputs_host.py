"""CPU checks of forward_ragged_multi_guide_train(input_grads=True): the refusals that stay (and come before any device is touched), the
pair and tile tables of the three new native calls as pure host functions on MIX6 and MIX9, the entry points (declared, exported, bound)
and their own refusals in front of anything that needs a device.  Every test here fails without the feature."""
import ctypes
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cases
import hicom_amd
from hicom_amd import native as nv
from hicom_amd import ragged
from hicom_amd import ragged_multi_guide as rmg
from host_util import ADDR, EINVAL
from test_ragged_host import HEADER, N_CUS, projector
from test_ragged_multi_guide_host import block
from test_ragged_multi_guide_train_host import MIXES, module, ws_block

P = "hicom_compressor_ragged_multiguide_"
NEW = {P + "local_bwd": 9, P + "dq_pair": 3, P + "global_dx": 10}


def tables(name):
    side, splits, modals, counts = MIXES[name]
    desc, ks = ragged.item_descriptors(projector(), splits, modals, side, side, False)
    return rmg.plan_tables(desc, counts, side, side, ks, 9, N_CUS), side, splits, counts, desc, ks


def test_entry_points_are_declared_exported_and_bound():
    lib = ctypes.CDLL(nv.LIB_PATH)
    for name, n_args in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", HEADER)
        assert m, f"{name} is not declared in include/hicom_hip.h"
        assert name in nv.EXPORTS and hasattr(lib, name) and name in nv.SIGNATURES
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args == len(getattr(nv.lib(), name).argtypes)
        assert getattr(nv.lib(), name).restype is ctypes.c_int
        assert getattr(nv.lib(), name).argtypes[0] == ctypes.POINTER(nv.CompressorRaggedMultiGuideArgs)
    assert nv.ABI_VERSION == 16 and "#define HICOM_ABI_VERSION 16" in HEADER


@pytest.mark.parametrize("name", sorted(MIXES))
def test_tile_table_is_per_item_whatever_the_guide_counts(name):
    """64 tokens of ONE item per tile, counted from the item's first token; the last tile of an item ends at the item's end; Q_i does not
    enter (a tile's workgroup adds all nh Q_i rows)."""
    t, side, splits, counts, desc, ks = tables(name)
    tab = rmg.dx_tile_table(t)
    assert tab.dtype == np.int32 and tab.shape == (sum((T * side * side + 63) // 64 for T in splits), 2)
    want = [(i, n0) for i, T in enumerate(splits) for n0 in range(0, T * side * side, 64)]
    assert [tuple(r) for r in tab.tolist()] == want
    t1 = rmg.plan_tables(desc, [1] * len(splits), side, side, ks, 9, N_CUS)
    assert np.array_equal(tab, rmg.dx_tile_table(t1)) and np.array_equal(tab, ragged.dx_tile_table(ragged.plan_tables(desc, side, side, ks, N_CUS)))
    if name == "mix6":                                          # 36, 144, 36, 288, 36 tokens: 1 + 3 + 1 + 5 + 1 tiles, tails of 36, 16, 36, 32, 36
        assert len(tab) == 11 and tuple(tab[3]) == (1, 128) and tuple(tab[9]) == (3, 256)
    else:                                                       # 81 and 324 tokens: 2 + 6 tiles, tails of 17 and 4
        assert len(tab) == 8 and tuple(tab[1]) == (0, 64) and tuple(tab[7]) == (1, 320)


@pytest.mark.parametrize("name", sorted(MIXES))
def test_pair_dq_table_partitions_the_pair_major_window_rows(name):
    t, side, splits, counts, desc, ks = tables(name)
    tab = rmg.pair_dq_table(t)
    assert tab.shape == (sum(counts), 2)
    wps = (side // ks) ** 2
    first = 0
    k = 0
    for i, (T, Q) in enumerate(zip(splits, counts)):
        w = (T // desc[i][1]) * wps
        for q in range(Q):
            assert tuple(tab[k]) == (first, w) and t.pairs[k][:2] == (i, q)
            first += w
            k += 1
    assert first == sum(q * w for q, w in zip(t.Q, t.windows))  # every row of dq in exactly one pair
    if name == "mix6":                                          # windows 4, 4, 4, 8, 4 (ks 3, kt 4 for the 4- and 8-frame videos, 1 otherwise)
        assert [int(c) for c in tab[:, 1]] == [t.windows[i] for i, _, _, _ in t.pairs]


def call(fn, a, *rest):
    r = getattr(nv.lib(), P + fn)(None if a is None else ctypes.byref(a), *rest)
    return int(r), nv.lib().hicom_last_error().decode()


def local(a, key=ADDR, value=ADDR + 4096, guide=ADDR, dctx=ADDR, dq=ADDR, dkey=ADDR + 8192, dvalue=ADDR + 12288, vik=0):
    return call("local_bwd", a, key, value, guide, dctx, dq, dkey, dvalue, vik)


def dqp(a, dq=ADDR, out=ADDR):
    return call("dq_pair", a, dq, out)


def gdx(a, scores=ADDR, ds=ADDR, ml=ADDR, qt=ADDR, dctx=ADDR, tiles=ADDR, ntiles=11, dx=ADDR, acc=1):
    return call("global_dx", a, scores, ds, ml, qt, dctx, tiles, ntiles, dx, acc)


REFUSALS = {
    "local: NULL block": (lambda: local(None), "NULL arguments"),
    "local: NULL key": (lambda: local(ws_block(), key=None), "NULL pointer"),
    "local: NULL value": (lambda: local(ws_block(), value=None), "NULL pointer"),
    "local: NULL guide": (lambda: local(ws_block(), guide=None), "NULL pointer"),
    "local: NULL dctx": (lambda: local(ws_block(), dctx=None), "NULL pointer"),
    "local: NULL dq": (lambda: local(ws_block(), dq=None), "NULL pointer"),
    "local: dkey under value_is_key": (lambda: local(ws_block(), value=ADDR, vik=1), "dkey must be NULL"),
    "local: value_is_key with other keys": (lambda: local(ws_block(), dkey=None, vik=1), "the keys are the value rows"),
    "local: unaligned dq": (lambda: local(ws_block(), dq=ADDR + 4), "aligned pointers"),
    "local: unaligned dvalue": (lambda: local(ws_block(), dvalue=ADDR + 12290), "aligned pointers"),
    "local: gradient over the tokens": (lambda: local(ws_block(), dvalue=ADDR + 4096), "cannot overwrite"),
    "local: one buffer for both gradients": (lambda: local(ws_block(), dvalue=ADDR + 8192), "cannot overwrite"),
    "local: no plan workspace": (lambda: local(block()), "workspace of"),
    "local: short plan workspace": (lambda: local(ws_block(ws_bytes=4096)), "workspace of"),
    "dq_pair: NULL block": (lambda: dqp(None), "NULL arguments"),
    "dq_pair: NULL dq": (lambda: dqp(ws_block(), dq=None), "NULL pointer"),
    "dq_pair: NULL out": (lambda: dqp(ws_block(), out=None), "NULL pointer"),
    "dq_pair: unaligned": (lambda: dqp(ws_block(), out=ADDR + 8), "16-byte aligned"),
    "dq_pair: no plan workspace": (lambda: dqp(block()), "workspace of"),
    "global_dx: NULL block": (lambda: gdx(None), "NULL arguments"),
    "global_dx: NULL scores": (lambda: gdx(ws_block(), scores=None), "NULL pointer"),
    "global_dx: NULL ds": (lambda: gdx(ws_block(), ds=None), "NULL pointer"),
    "global_dx: NULL ml": (lambda: gdx(ws_block(), ml=None), "NULL pointer"),
    "global_dx: NULL qt": (lambda: gdx(ws_block(), qt=None), "NULL pointer"),
    "global_dx: NULL dctx": (lambda: gdx(ws_block(), dctx=None), "NULL pointer"),
    "global_dx: NULL tiles": (lambda: gdx(ws_block(), tiles=None), "NULL pointer"),
    "global_dx: NULL dx": (lambda: gdx(ws_block(), dx=None), "NULL pointer"),
    "global_dx: unaligned qt": (lambda: gdx(ws_block(), qt=ADDR + 8), "aligned pointers"),
    "global_dx: unaligned dx": (lambda: gdx(ws_block(), dx=ADDR + 4), "aligned pointers"),
    "global_dx: tiles of another plan": (lambda: gdx(ws_block(), ntiles=15), "15 tiles, the items have 11 tiles"),
    "global_dx: no plan workspace": (lambda: gdx(block()), "workspace of"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_native_calls_refuse_before_a_device_is_needed(name):
    make, needle = REFUSALS[name]
    got, text = make()
    assert got == EINVAL and needle in text and text.startswith("compressor_ragged_multiguide"), (got, text)


def test_the_per_item_partition_is_checked_in_front_of_the_pointers_use():
    for make in (lambda a: local(a), lambda a: dqp(a), lambda a: gdx(a)):
        got, text = make(ws_block(counts=(1, 3, 5, 2, 33)))
        assert got < 0 and "Q=33 guides" in text


def test_input_grads_false_refuses_exactly_as_before_and_true_refuses_what_stays_out_of_scope():
    """CPU tensors and CPU modules: a refusal that came after the first device access would be another error."""
    ff = torch.zeros((5, 6, 6, cases.D), dtype=torch.bfloat16)
    g = torch.zeros((7, cases.D), dtype=torch.bfloat16)
    store = rmg.STORE
    call_ = lambda m, ff=ff, fe=ff, g=g, **kw: m.forward_ragged_multi_guide_train(ff, fe, g, [1, 4], [3, 4], ["image", "video"], **kw)
    m = module()
    ll = torch.zeros((4, 5, 6, 6))
    leaf = lambda t: t.clone().requires_grad_(True)
    # the default, and input_grads=False spelled out: the four refusals of an input that requires grad
    for extra in ({}, {"input_grads": False}):
        for kw, word in ((dict(ff=leaf(ff)), "frames_feature"), (dict(fe=leaf(ff)), "frames_embed"), (dict(g=leaf(g)), "guide_embeds"),
                         (dict(fe=None, local_logits=leaf(ll)), "local_logits")):
            with pytest.raises(NotImplementedError, match=word) as e:
                call_(m, **kw, **extra)
            assert "forward()" in str(e.value) and "(stage 3) is not built for the ragged multi-guide training step" in str(e.value)
            assert not m.__dict__.get(store)
    # input_grads=True: the logits form and every other out-of-scope form still refuse, in front of any device work, naming the loop
    for kw, word in ((dict(fe=None, local_logits=leaf(ll)), "local_logits"), (dict(fe=None, ff=leaf(ff), local_logits=ll), "logits form"),
                     (dict(fe=None, g=leaf(g), local_logits=ll), "logits form"), (dict(ff=leaf(ff).half()), "float16"), (dict(g=leaf(g).float()), "float32")):
        with pytest.raises(NotImplementedError, match=word) as e:
            call_(m, input_grads=True, **kw)
        assert "forward()" in str(e.value) and not m.__dict__.get(store)
    for bad, word in ((module("local43_adaptkv_global32"), "adaptor"), (module(use_clip_scale="local"), "clip-scale"),
                      (module(use_guide="coarse"), "plain release recipe"), (module().to(torch.float16), "float16"), (module().to(torch.float32), "float32")):
        with pytest.raises(NotImplementedError, match=word) as e:
            call_(bad, ff=leaf(ff), input_grads=True)
        assert "forward()" in str(e.value) and not bad.__dict__.get(store)
    with pytest.raises(NotImplementedError, match=r"anyres.*forward\(\)"):
        m.forward_ragged_multi_guide_train({"base": None, "patch": ff[0]}, None, leaf(g), [1, 4], [3, 4], ["image", "video"], input_grads=True)
    with pytest.raises(ValueError, match="frames_embed=None"):
        call_(m, local_logits=ll, input_grads=True)
    # in scope: a frozen module with an input requiring grad is trainable -- the first thing that needs a device says so
    with pytest.raises(nv.HicomNativeError, match="GPU only"):
        call_(m.requires_grad_(False), ff=leaf(ff), input_grads=True)
    assert not m.__dict__.get(store)
