"""CPU checks of forward_ragged_train(input_grads=True): the two new entry points (declared, exported, bound), their refusals in front of
any device call, the tile -> item table of hicom_compressor_ragged_global_dx against a brute-force walk, and the refusals that stay.
Every test here fails without the feature."""
import ctypes
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cases
import hicom_amd
import ragged_input_bwd_reference as rr
from hicom_amd import native, ragged
from test_ragged_host import HEADER, MIXES, N_CUS, projector

NEW = {"hicom_compressor_ragged_local_bwd": 10, "hicom_compressor_ragged_global_dx": 10}


def test_entry_points_are_declared_exported_and_bound():
    lib = ctypes.CDLL(native.LIB_PATH)                 # loading needs no GPU; no compute call is made
    for name, n_args in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", HEADER)
        assert m, f"{name} is not declared in include/hicom_hip.h"
        assert name in native.EXPORTS and hasattr(lib, name)
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args == len(getattr(native.lib(), name).argtypes)
        assert getattr(native.lib(), name).restype is ctypes.c_int
        assert getattr(native.lib(), name).argtypes[0] == ctypes.POINTER(native.CompressorRaggedArgs)
        assert "struct" not in m.group(1).replace("const hicom_compressor_ragged_args*", "")          # scalars and plain pointers behind the block
    assert native.ABI_VERSION == 16 and "#define HICOM_ABI_VERSION 16" in HEADER
    assert "input_grads" in hicom_amd.HIComProjector.forward_ragged_train.__kwdefaults__
    assert hicom_amd.HIComProjector.forward_ragged_train.__kwdefaults__["input_grads"] is False


def block(T1=8):
    a = native.CompressorRaggedArgs()
    items = (native.RaggedItem * 2)(native.RaggedItem(1, 1, 0, 0, 0, 1, 32), native.RaggedItem(T1, 4, 0, 0, 0, 1, 32))
    a.B, a.H, a.W, a.E, a.hidden, a.ks, a.nh, a.chunks, a.items = 2, 6, 6, 1152, 64, 3, 9, 1, items
    a.l_scale = 1152 ** -0.5
    return a, items


def test_null_pointers_and_a_non_partition_item_are_refused_without_a_device():
    """chunks = 1: the layout needs no CU count, so nothing here can have asked for a device; every call returns -1 with the message set."""
    lib = native.lib()
    err = lambda: lib.hicom_last_error().decode()
    a, keep = block()
    assert lib.hicom_compressor_ragged_local_bwd(ctypes.byref(a), None, None, None, None, None, None, None, None, 0) == -1
    assert "compressor_ragged_local_bwd: NULL pointer" in err()
    assert lib.hicom_compressor_ragged_global_dx(ctypes.byref(a), None, None, None, None, None, None, 0, None, 0) == -1
    assert "compressor_ragged_global_dx: NULL pointer" in err()
    p = 4096                                             # (an address that is never dereferenced: every refusal below comes first)
    # value_is_key with a dkey, and with two different streams
    assert lib.hicom_compressor_ragged_local_bwd(ctypes.byref(a), p, p, p, p, p, None, p, p, 1) == -1 and "dkey must be NULL" in err()
    assert lib.hicom_compressor_ragged_local_bwd(ctypes.byref(a), p, 2 * p, p, p, p, None, None, p, 1) == -1 and "value rows" in err()
    # the tile count is held against the items: 36 and 288 tokens are 1 + 5 tiles of 64
    assert lib.hicom_compressor_ragged_global_dx(ctypes.byref(a), p, p, p, p, p, p, 5, p, 0) == -1 and "6 tiles" in err()
    # all pointers given, no workspace: refused at the workspace check, still in front of any launch
    assert lib.hicom_compressor_ragged_local_bwd(ctypes.byref(a), p, p, p, p, p, None, None, None, 0) == -1 and "workspace" in err()
    assert lib.hicom_compressor_ragged_global_dx(ctypes.byref(a), p, p, p, p, p, p, 6, p, 0) == -1 and "workspace" in err()
    b, keep2 = block(T1=6)                               # 6 frames under a temporal window of 4: no exact partition
    for call in (lambda: lib.hicom_compressor_ragged_local_bwd(ctypes.byref(b), p, p, p, p, p, None, None, None, 0),
                 lambda: lib.hicom_compressor_ragged_global_dx(ctypes.byref(b), p, p, p, p, p, p, 6, p, 0)):
        assert call() < 0 and re.search("item 1.*partition", err())          # (the shape check's own code: unsupported)


@pytest.mark.parametrize("name", sorted(MIXES))
def test_tile_table_against_a_brute_force_walk(name):
    """Every token in exactly one tile, no tile across an item edge, tiles counted from the item's first token."""
    side, splits, modals, over, newline = MIXES[name]
    proj = projector(**over)
    desc, ks = ragged.item_descriptors(proj, splits, modals, side, side, newline)
    t = ragged.plan_tables(desc, side, side, ks, N_CUS)
    tab = ragged.dx_tile_table(t)
    assert tab.dtype == np.int32 and tab.ndim == 2 and tab.shape[1] == 2 and tab.flags["C_CONTIGUOUS"]
    assert tab.shape[0] == sum((n + 63) // 64 for n in t.N)
    covered = np.zeros(sum(t.N), dtype=np.int64)
    walk = rr.tile_walk(t.N)
    for item, n0 in tab:
        assert 0 <= item < len(t.N) and 0 <= n0 < t.N[item] and n0 % 64 == 0
        end = min(n0 + 64, t.N[item])                    # (the kernel masks the tile at the item's end)
        lo, hi = t.tok0[item] + n0, t.tok0[item] + end
        assert hi <= t.tok0[item] + t.N[item]
        covered[lo:hi] += 1
        assert all(walk[k] == (item, n0) for k in range(lo, hi))
    assert (covered == 1).all()
    assert [tuple(r) for r in tab] == sorted(set(walk))  # ... in the order of the stack


def module(recipe="local43_global32", **over):
    return hicom_amd.build_vision_projector(SimpleNamespace(**{**cases.DEFAULT_CFG, "hidden_size": 64, "mm_projector_type": recipe, **over})).to(torch.bfloat16)


def test_the_default_keeps_the_three_refusals_on_cpu_tensors():
    ff = torch.zeros((2, 6, 6, cases.D), dtype=torch.bfloat16)
    g = torch.zeros((2, cases.D), dtype=torch.bfloat16)
    m = module()
    for kw, word in ((dict(ff=ff.clone().requires_grad_(True)), "frames_feature"), (dict(fe=ff.clone().requires_grad_(True)), "frames_embed"),
                     (dict(g=g.clone().requires_grad_(True)), "guide_embeds")):
        for extra in ({}, {"input_grads": False}):
            with pytest.raises(NotImplementedError, match=word) as e:
                m.forward_ragged_train(kw.get("ff", ff), kw.get("fe", ff), kw.get("g", g), [1, 1], "image", **extra)
            assert "forward()" in str(e.value) and "_ragged_plans" not in m.__dict__


def test_adaptor_and_clip_scale_still_raise_with_input_grads():
    ff = torch.zeros((2, 6, 6, cases.D), dtype=torch.bfloat16).requires_grad_(True)
    g = torch.zeros((2, cases.D), dtype=torch.bfloat16)
    for m, word in ((module("local43_adaptkv_global32"), "adaptor"), (module(use_clip_scale="local"), "clip-scale"), (module(use_guide="coarse"), "release recipe")):
        with pytest.raises(NotImplementedError, match=word) as e:
            m.forward_ragged_train(ff, ff.detach(), g, [1, 1], "image", input_grads=True)
        assert "forward()" in str(e.value) and "_ragged_plans" not in m.__dict__
    with pytest.raises(NotImplementedError, match=r"anyres.*forward\(\)"):
        module().forward_ragged_train({"base": None, "patch": ff[0]}, None, g, [1, 1], "image", input_grads=True)
