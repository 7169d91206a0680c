"""CPU checks of the ragged training step (HIComProjector.forward_ragged_train): the row maps of its backward against the oracle's packing,
the three new entry points (declared, exported, bound), the host arithmetic of the backward's workspace function, and the refusals that
must come before any device is touched.  Every test here fails without the feature."""
import ctypes
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cases
import hicom_amd
from hicom_amd import native, ragged
from hicom_amd.projector import HIComProjector
from oracle import hicom_oracle as orc
from test_ragged_host import HEADER, MIXES, N_CUS, projector

NEW = {"hicom_compressor_ragged_train_state": (ctypes.c_int, 5), "hicom_compressor_ragged_global_bwd_workspace_bytes": (ctypes.c_int64, 1),
       "hicom_compressor_ragged_global_bwd": (ctypes.c_int, 10)}
NG = 32


@pytest.mark.parametrize("name", sorted(MIXES))
def test_row_maps_are_the_oracles_packing(name):
    """Rows that carry their own index through the oracle's post_process: window w of the concatenated window list sits in row local[w],
    the newline vector in the rows `newline`, and the item's global rows are `glob`; together they are every row once."""
    side, splits, modals, over, newline = MIXES[name]
    proj = projector(**over)
    desc, ks = ragged.item_descriptors(proj, splits, modals, side, side, newline)
    t = ragged.plan_tables(desc, side, side, ks, N_CUS)
    local, nl_rows, glob = ragged.train_row_maps(t)
    packed = []
    for i, (T, modal) in enumerate(zip(splits, modals)):
        grid = (T // desc[i][1], side // ks, side // ks)
        feat = (t.win0[i] + torch.arange(t.windows[i], dtype=torch.float64)).reshape(*grid, 1)
        nl = torch.full((1,), -1.0, dtype=torch.float64) if newline else None
        loc = orc.post_process(proj.config, feat, modal, nl, False)
        packed.append(torch.cat([loc, torch.full((NG, 1), -2.0 - i, dtype=torch.float64)]))
        assert packed[-1].shape[0] == t.rows[i]
    packed = torch.cat(packed).reshape(-1).numpy()
    assert local.dtype == nl_rows.dtype == glob.dtype == np.int64
    assert np.array_equal(packed[local], np.arange(sum(t.windows)))
    assert np.all(packed[nl_rows] == -1.0) and len(nl_rows) == int((packed == -1.0).sum())
    assert glob.shape == (len(splits), NG)
    for i in range(len(splits)):
        assert np.all(packed[glob[i]] == -2.0 - i)
    assert sorted(np.concatenate([local, nl_rows, glob.reshape(-1)]).tolist()) == list(range(packed.size))
    if name == "9x9_grid_newline":
        assert len(nl_rows) == 1 + 3 and nl_rows[0] == 9                         # the image's one row, the clip's one per grid row


def test_entry_points_are_declared_exported_and_bound():
    lib = ctypes.CDLL(native.LIB_PATH)                 # loading needs no GPU; no compute call is made
    for name, (restype, n_args) in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", HEADER)
        assert m, f"{name} is not declared in include/hicom_hip.h"
        assert name in native.EXPORTS and hasattr(lib, name)
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args == len(getattr(native.lib(), name).argtypes)
        assert getattr(native.lib(), name).restype is restype
        assert getattr(native.lib(), name).argtypes[0] == ctypes.POINTER(native.CompressorRaggedArgs)
    assert native.ABI_VERSION == 16 and "#define HICOM_ABI_VERSION 16" in HEADER
    assert callable(getattr(HIComProjector, "forward_ragged_train"))
    assert not any("ragged" in n.lower() for n in getattr(hicom_amd, "__all__"))


def test_backward_workspace_function_refuses_without_a_device_call():
    a = native.CompressorRaggedArgs()
    items = (native.RaggedItem * 2)(native.RaggedItem(1, 1, 0, 0, 0, 1, 32), native.RaggedItem(6, 4, 0, 0, 0, 1, 32))
    a.B, a.H, a.W, a.E, a.hidden, a.ks, a.nh, a.chunks, a.items = 2, 6, 6, 1152, 64, 3, 9, 1, items
    with pytest.raises(native.HicomNativeError, match="item 1.*partition"):
        native.compressor_ragged_global_bwd_workspace(a)
    items[1].T = 8
    a.E = 1024
    with pytest.raises(native.HicomNativeError, match="E=1024"):
        native.compressor_ragged_global_bwd_workspace(a)
    a.E = 1152
    n1 = native.compressor_ragged_global_bwd_workspace(a)
    # planes of dctx (2 x R x E bf16) and one partial sum [16][E] f32 per work unit, each region rounded up to 256 bytes; no pe: no pos_b
    r256 = lambda n: (n + 255) // 256 * 256
    assert n1 == 2 * r256(2 * 9 * 1152 * 2) + r256(2 * 16 * 1152 * 4)
    a.chunks = 3
    assert native.compressor_ragged_global_bwd_workspace(a) == n1 + (6 - 2) * 16 * 1152 * 4          # 3 + 3 units instead of 1 + 1
    # the two calls that launch check their pointers in front of everything else that needs a device
    assert native.lib().hicom_compressor_ragged_global_bwd(ctypes.byref(a), None, None, None, None, None, None, None, None, 0) == -1
    assert native.lib().hicom_compressor_ragged_train_state(ctypes.byref(a), None, None, None, None) == -1


def module(recipe="local43_global32", **over):
    return hicom_amd.build_vision_projector(SimpleNamespace(**{**cases.DEFAULT_CFG, "hidden_size": 64, "mm_projector_type": recipe, **over})).to(torch.bfloat16)


def test_out_of_scope_calls_refuse_before_touching_a_device():
    """CPU tensors and CPU modules: a refusal that came after the first device access would be another error."""
    ff = torch.zeros((2, 6, 6, cases.D), dtype=torch.bfloat16)
    g = torch.zeros((2, cases.D), dtype=torch.bfloat16)
    call = lambda m, ff=ff, fe=ff, g=g: m.forward_ragged_train(ff, fe, g, [1, 1], "image")
    for m, word in ((module("local43_adaptkv_global32"), "adaptor"), (module(use_clip_scale="local"), "clip-scale"),
                    (module(use_guide="coarse"), "release recipe")):
        with pytest.raises(NotImplementedError, match=word) as e:
            call(m)
        assert "forward()" in str(e.value) and "_ragged_plans" not in m.__dict__
    m = module()
    with pytest.raises(NotImplementedError, match=r"anyres.*forward\(\)"):
        m.forward_ragged_train({"base": None, "patch": ff[0]}, None, g, [1, 1], "image")
    for kw, word in ((dict(ff=ff.clone().requires_grad_(True)), "frames_feature"), (dict(fe=ff.clone().requires_grad_(True)), "frames_embed"),
                     (dict(g=g.clone().requires_grad_(True)), "guide_embeds")):
        with pytest.raises(NotImplementedError, match=word) as e:
            call(m, **kw)
        assert "forward()" in str(e.value) and "_ragged_plans" not in m.__dict__
