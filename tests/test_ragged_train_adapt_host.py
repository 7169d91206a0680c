"""CPU checks of forward_ragged_train(adaptors=True): the new entry points (declared, exported, bound), their refusals in front of any device
call, the refusals of the Python call with and without the keyword, and the window -> item and token -> (item, window) maps against a
brute-force walk.  Every test here fails without the feature."""
import ctypes
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cases
import hicom_amd
from hicom_amd import native, ragged
from test_ragged_host import HEADER, N_CUS, projector

NEW = {"hicom_compressor_ragged_local_adapt_bwd": 21, "hicom_compressor_ragged_adapt_dy": 14, "hicom_compressor_ragged_dq_item": 3,
       "hicom_compressor_ragged_adapt_train_state": 3}


def test_entry_points_are_declared_exported_and_bound():
    lib = ctypes.CDLL(native.LIB_PATH)                 # loading needs no GPU; no compute call is made
    for name, n_args in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", HEADER)
        assert m, f"{name} is not declared in include/hicom_hip.h"
        assert name in native.EXPORTS and hasattr(lib, name)
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args == len(getattr(native.lib(), name).argtypes)
        assert getattr(native.lib(), name).restype is ctypes.c_int
        block = native.CompressorRaggedAdaptArgs if name.endswith("train_state") else native.CompressorRaggedArgs
        assert getattr(native.lib(), name).argtypes[0] == ctypes.POINTER(block)
        assert "struct" not in m.group(1)                                      # scalars and plain pointers behind the block
    assert native.ABI_VERSION == 16 and "#define HICOM_ABI_VERSION 16" in HEADER
    kw = hicom_amd.HIComProjector.forward_ragged_train.__kwdefaults__
    assert kw["adaptors"] is False and kw["input_grads"] is False


def block(T1=8):
    a = native.CompressorRaggedArgs()
    items = (native.RaggedItem * 2)(native.RaggedItem(1, 1, 0, 0, 0, 1, 32), native.RaggedItem(T1, 4, 0, 0, 0, 1, 32))
    a.B, a.H, a.W, a.E, a.hidden, a.ks, a.nh, a.chunks, a.items = 2, 6, 6, 1152, 64, 3, 9, 1, items
    a.l_scale = 1152 ** -0.5
    return a, items


P = 4096                                                 # an address that is never dereferenced: every refusal below comes first


def window_call(lib, a, **over):
    """hicom_compressor_ragged_local_adapt_bwd with every pointer given (both streams adapted); `over` replaces arguments by name."""
    names = ("key_x", "key_y", "k_gamma", "k_beta", "k_alpha", "value_x", "value_y", "v_gamma", "v_beta", "v_alpha", "alpha_dt", "eps", "guide", "dctx",
             "ds", "pw", "sxk", "syk", "sxv", "syv")
    v = {n: P for n in names}
    v.update(alpha_dt=native.DT_BF16, eps=1e-6)
    v.update(over)
    return lib.hicom_compressor_ragged_local_adapt_bwd(ctypes.byref(a), *[v[n] for n in names])


def dy_call(lib, a, **over):
    names = ("y", "gamma", "vec", "vec_dt", "vec_per_item", "coef", "alpha", "alpha_dt", "eps", "dy", "r1", "col_parts", "nparts")
    v = {n: P for n in names}
    v.update(vec_dt=native.DT_F32, vec_per_item=0, alpha_dt=native.DT_BF16, eps=1e-6, r1=None, col_parts=None, nparts=0)
    v.update(over)
    return lib.hicom_compressor_ragged_adapt_dy(ctypes.byref(a), *[v[n] for n in names])


def test_null_misaligned_and_non_partition_arguments_are_refused_without_a_launch():
    """chunks = 1: the layout needs no CU count, so nothing here can have asked for a device; every call returns an argument error with the
    message set, and the complete calls end at the workspace check (the block has none), still in front of any launch."""
    lib = native.lib()
    err = lambda: lib.hicom_last_error().decode()
    a, keep = block()
    # NULL pointers
    for name in ("key_x", "value_x", "guide", "dctx", "ds", "pw"):
        assert window_call(lib, a, **{name: None}) == -1 and "compressor_ragged_local_adapt_bwd: NULL pointer" in err(), name
    assert window_call(lib, a, key_y=None, value_y=None, syk=None, syv=None) == -1 and "no adapted stream" in err()
    assert window_call(lib, a, k_gamma=None) == -1 and "adaptor parameters" in err()
    assert window_call(lib, a, v_alpha=None) == -1 and "adaptor parameters" in err()
    assert window_call(lib, a, key_y=None) == -1 and "syk / syv" in err()          # syk given for a stream without adaptor
    assert window_call(lib, a, alpha_dt=7) == -1 and "alpha dtype" in err()
    for name in ("y", "gamma", "vec", "coef", "alpha", "dy"):
        assert dy_call(lib, a, **{name: None}) == -1 and "compressor_ragged_adapt_dy: NULL pointer" in err(), name
    assert dy_call(lib, a, col_parts=P, nparts=0) == -1 and "NULL pointer" in err()
    assert dy_call(lib, a, vec_dt=native.DT_F16) == -1 and "dtypes" in err()
    assert lib.hicom_compressor_ragged_dq_item(ctypes.byref(a), None, P) == -1 and "compressor_ragged_dq_item: NULL pointer" in err()
    assert lib.hicom_compressor_ragged_dq_item(ctypes.byref(a), P, None) == -1 and "NULL pointer" in err()
    assert lib.hicom_compressor_ragged_local_adapt_bwd(None, *([None] * 10), 0, 0.0, *([None] * 8)) == -1 and "NULL arguments" in err()
    # misaligned pointers: 16-bit rows on 4 bytes, f32 matrices on 16
    for name in ("key_x", "key_y", "value_y", "guide", "ds"):
        assert window_call(lib, a, **{name: P + 2}) == -1 and "4-byte aligned" in err(), name
    for name in ("dctx", "sxk", "syv"):
        assert window_call(lib, a, **{name: P + 4}) == -1 and "16-byte aligned" in err(), name
    for name in ("y", "vec", "dy", "r1"):
        assert dy_call(lib, a, **{name: P + 2}) == -1 and "4-byte aligned" in err(), name
    assert lib.hicom_compressor_ragged_dq_item(ctypes.byref(a), P + 4, P) == -1 and "16-byte aligned" in err()
    # every NULL-output combination passes the argument checks: refused at the workspace check only
    for sums in ({}, {"sxk": None}, {"sxv": None}, {"sxk": None, "sxv": None, "syk": None, "syv": None}, {"key_y": None, "syk": None, "sxk": None}):
        assert window_call(lib, a, **sums) == -1 and "workspace" in err(), sums
    assert dy_call(lib, a) == -1 and "workspace" in err()
    assert dy_call(lib, a, r1=P, col_parts=P, nparts=4, vec_per_item=1, vec_dt=native.DT_BF16) == -1 and "workspace" in err()
    assert lib.hicom_compressor_ragged_dq_item(ctypes.byref(a), P, P) == -1 and "workspace" in err()
    # a non-exact partition: 6 frames under a temporal window of 4
    b, keep2 = block(T1=6)
    for call in (lambda: window_call(lib, b), lambda: dy_call(lib, b), lambda: lib.hicom_compressor_ragged_dq_item(ctypes.byref(b), P, P)):
        assert call() < 0 and re.search("item 1.*partition", err())
    # the y planes: a zeroed adaptor block adapts neither stream
    z = native.CompressorRaggedAdaptArgs()
    z.base = a
    assert lib.hicom_compressor_ragged_adapt_train_state(ctypes.byref(z), P, P) < 0 and "neither stream has an adaptor" in err()
    assert lib.hicom_compressor_ragged_adapt_train_state(None, P, P) == -1 and "NULL arguments" in err()


def module(recipe="local43_global32", **over):
    return hicom_amd.build_vision_projector(SimpleNamespace(**{**cases.DEFAULT_CFG, "hidden_size": 64, "mm_projector_type": recipe, **over})).to(torch.bfloat16)


def test_refusals_with_and_without_the_keyword_touch_no_device_and_leave_no_plan():
    ff = torch.zeros((2, 6, 6, cases.D), dtype=torch.bfloat16)
    g = torch.zeros((2, cases.D), dtype=torch.bfloat16)
    adapt = module("local43_adaptkv_global32")
    for kw in ({}, {"adaptors": False}, {"input_grads": True}):
        with pytest.raises(NotImplementedError, match="adaptor") as e:
            adapt.forward_ragged_train(ff, ff, g, [1, 1], "image", **kw)
        assert "forward()" in str(e.value) and "adaptors=True" in str(e.value) and "_ragged_plans" not in adapt.__dict__
    # with the keyword: clip-scale, anyres dicts, non-release recipes and an input that requires grad without input_grads still raise
    for m, word in ((module("local43_adaptkv_global32", use_clip_scale="local"), "clip-scale"), (module(use_clip_scale="local"), "clip-scale"),
                    (module("local43_adaptkv_global32", use_guide="coarse"), "release recipe"), (module(use_guide="coarse"), "release recipe")):
        with pytest.raises(NotImplementedError, match=word) as e:
            m.forward_ragged_train(ff, ff, g, [1, 1], "image", adaptors=True)
        assert "forward()" in str(e.value) and "_ragged_plans" not in m.__dict__
    with pytest.raises(NotImplementedError, match=r"anyres.*forward\(\)"):
        adapt.forward_ragged_train({"base": None, "patch": ff[0]}, None, g, [1, 1], "image", adaptors=True)
    with pytest.raises(NotImplementedError, match="frames_embed"):
        adapt.forward_ragged_train(ff, ff.clone().requires_grad_(True), g, [1, 1], "image", adaptors=True)
    assert "_ragged_plans" not in adapt.__dict__
    # the CPU tensors of a call in scope are refused by forward_ragged's own input checks, in front of any plan
    with pytest.raises((ValueError, NotImplementedError, RuntimeError)):
        adapt.forward_ragged_train(ff, ff, g, [1, 1], "image", adaptors=True)
    assert "_ragged_plans" not in adapt.__dict__


MIX6 = (6, [1, 4, 1, 8, 1], ["image", "video", "video", "video", "image"])
MIX9 = (9, [1, 4], ["image", "video"])
BATCH = (6, [4, 4, 4], ["video"] * 3)


@pytest.mark.parametrize("mix", [MIX6, MIX9, BATCH], ids=["mix6", "mix9", "batch"])
def test_window_and_token_maps_against_a_brute_force_walk(mix):
    """Every window of the concatenated list belongs to the item whose windows it was counted with; every token lies in exactly the window
    whose token walk (WindowGeom::token_of, restated) reaches it, and in the item whose tokens it was stacked with."""
    side, splits, modals = mix
    proj = projector()
    desc, ks = ragged.item_descriptors(proj, splits, modals, side, side, False)
    t = ragged.plan_tables(desc, side, side, ks, N_CUS)
    item_of, win_of = ragged.token_item_window(t, side, side, ks)
    n_tok, n_win = sum(t.N), sum(t.windows)
    assert item_of.shape == win_of.shape == (n_tok,) and t.win_item.shape == (n_win,)
    want_item, want_win, want_win_item = np.full(n_tok, -1), np.full(n_tok, -1), np.full(n_win, -1)
    win = 0
    for i, (T, kt) in enumerate((d[0], d[1]) for d in desc):
        for t1 in range(T // kt):
            for h1 in range(side // ks):
                for w1 in range(side // ks):
                    want_win_item[win] = i
                    for t2 in range(kt):
                        for h2 in range(ks):
                            for w2 in range(ks):
                                tok = t.tok0[i] + ((t1 * kt + t2) * side + h1 * ks + h2) * side + w1 * ks + w2
                                assert want_win[tok] == -1                      # (an exact partition: every token once)
                                want_item[tok], want_win[tok] = i, win
                    win += 1
    assert win == n_win and (want_win >= 0).all()
    assert np.array_equal(t.win_item, want_win_item)
    assert np.array_equal(item_of, want_item) and np.array_equal(win_of, want_win)
    assert np.array_equal(t.win_item[win_of], item_of)                          # the two maps agree with each other
