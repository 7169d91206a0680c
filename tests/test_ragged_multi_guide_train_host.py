"""CPU checks of the ragged multi-guide training step (HIComProjector.forward_ragged_multi_guide_train): the row maps of its backward
against plan_tables and the oracle's packing, the three new entry points (declared, exported, bound), the host arithmetic of the
backward's workspace function, and the refusals that must come before any device is touched.  Every test here fails without the
feature."""
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
from hicom_amd.projector import HIComProjector
from host_util import ADDR, EINVAL
from oracle import hicom_oracle as orc
from test_ragged_host import HEADER, N_CUS, projector
from test_ragged_multi_guide_host import block

P = "hicom_compressor_ragged_multiguide_"
NEW = {P + "train_state": (ctypes.c_int, 5), P + "global_bwd_workspace_bytes": (ctypes.c_int64, 1), P + "global_bwd": (ctypes.c_int, 10)}
NG = 32
# (grid side, splits, modals, guide counts): the two mixes of tests/ragged_multi_guide_inputs.py
MIXES = {"mix6": (6, (1, 4, 1, 8, 1), ("image", "video", "video", "video", "image"), (1, 3, 5, 2, 4)), "mix9": (9, (1, 4), ("image", "video"), (4, 8))}


@pytest.mark.parametrize("grid_newline", [None, False, True], ids=["no_newline", "newline", "newline_grid"])
@pytest.mark.parametrize("name", sorted(MIXES))
def test_pair_row_maps_cover_every_row_once_in_window_order(name, grid_newline):
    """Rows that carry their own index through the oracle's post_process, per pair: context row c of the pair-major window contexts sits
    in row local[c], the newline vector in the rows `newline`, and pair p's global rows are glob[p]; together they are every row of every
    pair exactly once, and each pair's rows lie inside [row0_p, row0_p + rows_i) of plan_tables."""
    side, splits, modals, counts = MIXES[name]
    newline = grid_newline is not None
    proj = projector(**({"mm_newline_position": "grid"} if grid_newline else {}))
    desc, ks = ragged.item_descriptors(proj, splits, modals, side, side, newline)
    t = rmg.plan_tables(desc, counts, side, side, ks, 9, N_CUS)
    local, nl_rows, glob = rmg.train_row_maps(t)
    packed = []
    for p, (i, q, ctx_row0, row0) in enumerate(t.pairs):
        T, modal = splits[i], modals[i]
        grid = (T // desc[i][1], side // ks, side // ks)
        feat = (ctx_row0 + torch.arange(t.windows[i], dtype=torch.float64)).reshape(*grid, 1)
        nl = torch.full((1,), -1.0, dtype=torch.float64) if newline else None
        loc = orc.post_process(proj.config, feat, modal, nl, False)
        packed.append(torch.cat([loc, torch.full((NG, 1), -2.0 - p, dtype=torch.float64)]))
        assert packed[-1].shape[0] == t.rows[i] and row0 == sum(x.shape[0] for x in packed[:-1])
    packed = torch.cat(packed).reshape(-1).numpy()
    assert local.dtype == nl_rows.dtype == glob.dtype == np.int64
    assert np.array_equal(packed[local], np.arange(sum(q * w for q, w in zip(t.Q, t.windows))))          # window order per pair, pair-major
    assert np.all(packed[nl_rows] == -1.0) and len(nl_rows) == int((packed == -1.0).sum())
    assert glob.shape == (len(t.pairs), NG)
    for p, (i, q, _, row0) in enumerate(t.pairs):
        assert np.all(packed[glob[p]] == -2.0 - p)
        mine = np.concatenate([local[t.pairs[p][2]:t.pairs[p][2] + t.windows[i]], glob[p]])
        assert mine.min() >= row0 and mine.max() < row0 + t.rows[i]
    assert sorted(np.concatenate([local, nl_rows, glob.reshape(-1)]).tolist()) == list(range(packed.size))
    if newline:
        assert len(nl_rows) >= sum(q for q, m in zip(counts, modals) if m == "image")                   # every pair of an image carries one
    if name == "mix6" and not newline:      # every Q_i = 1 is the ragged step's map
        t1, r1 = rmg.plan_tables(desc, [1] * len(splits), side, side, ks, 9, N_CUS), ragged.plan_tables(desc, side, side, ks, N_CUS)
        assert all(np.array_equal(a, b) for a, b in zip(rmg.train_row_maps(t1), ragged.train_row_maps(r1)))


def test_entry_points_are_declared_exported_and_bound():
    lib = ctypes.CDLL(nv.LIB_PATH)                     # loading needs no GPU; no compute call is made
    for name, (restype, n_args) in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", HEADER)
        assert m, f"{name} is not declared in include/hicom_hip.h"
        assert name in nv.EXPORTS and hasattr(lib, name)
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args == len(getattr(nv.lib(), name).argtypes)
        assert getattr(nv.lib(), name).restype is restype
        assert getattr(nv.lib(), name).argtypes[0] == ctypes.POINTER(nv.CompressorRaggedMultiGuideArgs)
    assert nv.ABI_VERSION == 16 and "#define HICOM_ABI_VERSION 16" in HEADER
    assert callable(getattr(HIComProjector, "forward_ragged_multi_guide_train"))
    assert not any("ragged" in n.lower() for n in getattr(hicom_amd, "__all__"))


def _up(n):
    return (n + 255) // 256 * 256


def test_backward_workspace_arithmetic():
    """chunks > 0: pure host code.  Planes of dctx (2 x R x E bf16), pos_b (R x P f32, absent without pe) and one partial sum [16][E] f32 per
    slot (two per work unit), each region rounded up to 256 bytes."""
    a = block()                                        # MIX6, counts (1, 3, 5, 2, 4): 15 pairs, 7 passes, 3 chunks -> 21 units, 42 slots
    Rr = 15 * 9
    assert nv.compressor_ragged_multiguide_global_bwd_workspace(a) == 2 * _up(Rr * 1152 * 2) + _up(42 * 16 * 1152 * 4)
    a.chunks = 1
    assert nv.compressor_ragged_multiguide_global_bwd_workspace(a) == 2 * _up(Rr * 1152 * 2) + _up(14 * 16 * 1152 * 4)
    a = block(pe=ADDR, kpe=ADDR, P=28)
    assert nv.compressor_ragged_multiguide_global_bwd_workspace(a) == 2 * _up(Rr * 1152 * 2) + _up(Rr * 28 * 4) + _up(42 * 16 * 1152 * 4)
    with pytest.raises(nv.HicomNativeError, match="Q=33 guides"):
        nv.compressor_ragged_multiguide_global_bwd_workspace(block(counts=(1, 3, 5, 2, 33)))


def call_bwd(a, x=ADDR, dctx=ADDR, delta=ADDR, scores=ADDR, ml=ADDR, ds=ADDR + 4096, dqt=ADDR, bws=ADDR, bws_bytes=1 << 40):
    r = nv.lib().hicom_compressor_ragged_multiguide_global_bwd(None if a is None else ctypes.byref(a), x, dctx, delta, scores, ml, ds, dqt, bws, bws_bytes)
    return int(r), nv.lib().hicom_last_error().decode()


def call_state(a, ctx16=ADDR, scores=ADDR, ml=ADDR, ctxg=ADDR):
    r = nv.lib().hicom_compressor_ragged_multiguide_train_state(None if a is None else ctypes.byref(a), ctx16, scores, ml, ctxg)
    return int(r), nv.lib().hicom_last_error().decode()


def ws_block(**over):
    return block(**{"ws": ADDR, "ws_bytes": 1 << 40, **over})


BWD_REFUSALS = {
    "NULL block": (lambda: call_bwd(None), "NULL arguments"),
    "NULL x": (lambda: call_bwd(ws_block(), x=None), "NULL pointer"),
    "NULL dctx": (lambda: call_bwd(ws_block(), dctx=None), "NULL pointer"),
    "NULL delta": (lambda: call_bwd(ws_block(), delta=None), "NULL pointer"),
    "NULL scores": (lambda: call_bwd(ws_block(), scores=None), "NULL pointer"),
    "NULL ml": (lambda: call_bwd(ws_block(), ml=None), "NULL pointer"),
    "NULL ds": (lambda: call_bwd(ws_block(), ds=None), "NULL pointer"),
    "NULL dqt": (lambda: call_bwd(ws_block(), dqt=None), "NULL pointer"),
    "unaligned x": (lambda: call_bwd(ws_block(), x=ADDR + 2), "16-byte aligned"),
    "unaligned ds": (lambda: call_bwd(ws_block(), ds=ADDR + 4100), "16-byte aligned"),
    "unaligned dctx": (lambda: call_bwd(ws_block(), dctx=ADDR + 8), "16-byte aligned"),
    "dS over the logits": (lambda: call_bwd(ws_block(), ds=ADDR), "dS cannot overwrite the logits"),
    "no plan workspace": (lambda: call_bwd(block()), "workspace of"),
    "short plan workspace": (lambda: call_bwd(ws_block(ws_bytes=4096)), "workspace of"),
    "misaligned plan workspace": (lambda: call_bwd(ws_block(ws=ADDR + 128)), "256-byte aligned"),
    "NULL backward workspace": (lambda: call_bwd(ws_block(), bws=None), "backward workspace of"),
    "short backward workspace": (lambda: call_bwd(ws_block(), bws_bytes=4096), "backward workspace of"),
    "misaligned backward workspace": (lambda: call_bwd(ws_block(), bws=ADDR + 64), "256-byte aligned"),
}
STATE_REFUSALS = {
    "NULL block": (lambda: call_state(None), "NULL arguments"),
    "NULL ctx16": (lambda: call_state(ws_block(), ctx16=None), "NULL pointer"),
    "NULL scores": (lambda: call_state(ws_block(), scores=None), "NULL pointer"),
    "NULL ml": (lambda: call_state(ws_block(), ml=None), "NULL pointer"),
    "NULL ctxg": (lambda: call_state(ws_block(), ctxg=None), "NULL pointer"),
    "unaligned ml": (lambda: call_state(ws_block(), ml=ADDR + 2), "aligned pointers"),
    "no plan workspace": (lambda: call_state(block()), "workspace of"),
    "short plan workspace": (lambda: call_state(ws_block(ws_bytes=4096)), "workspace of"),
}


@pytest.mark.parametrize("name", list(BWD_REFUSALS))
def test_global_bwd_refuses_before_a_device_is_needed(name):
    make, needle = BWD_REFUSALS[name]
    got, text = make()
    assert got == EINVAL and needle in text and text.startswith("compressor_ragged_multiguide"), (got, text)


@pytest.mark.parametrize("name", list(STATE_REFUSALS))
def test_train_state_refuses_before_a_device_is_needed(name):
    make, needle = STATE_REFUSALS[name]
    got, text = make()
    assert got == EINVAL and needle in text and text.startswith("compressor_ragged_multiguide"), (got, text)


def module(recipe="local43_global32", **over):
    return hicom_amd.build_vision_projector(SimpleNamespace(**{**cases.DEFAULT_CFG, "hidden_size": 64, "mm_projector_type": recipe, **over})).to(torch.bfloat16)


def test_out_of_scope_calls_refuse_before_touching_a_device():
    """CPU tensors and CPU modules: a refusal that came after the first device access would be another error."""
    ff = torch.zeros((5, 6, 6, cases.D), dtype=torch.bfloat16)
    g = torch.zeros((7, cases.D), dtype=torch.bfloat16)
    store = rmg.STORE
    call = lambda m, ff=ff, fe=ff, g=g, **kw: m.forward_ragged_multi_guide_train(ff, fe, g, [1, 4], [3, 4], ["image", "video"], **kw)
    for m, word in ((module("local43_adaptkv_global32"), "adaptor"), (module(use_clip_scale="local"), "clip-scale"),
                    (module(use_guide="coarse"), "plain release recipe"), (module().to(torch.float16), "float16"), (module().to(torch.float32), "float32")):
        with pytest.raises(NotImplementedError, match=word) as e:
            call(m)
        assert "forward()" in str(e.value) and not m.__dict__.get(store)
    m = module()
    with pytest.raises(NotImplementedError, match=r"anyres.*forward\(\)"):
        m.forward_ragged_multi_guide_train({"base": None, "patch": ff[0]}, None, g, [1, 4], [3, 4], ["image", "video"])
    ll = torch.zeros((4, 5, 6, 6))
    for kw, word in ((dict(ff=ff.clone().requires_grad_(True)), "frames_feature"), (dict(fe=ff.clone().requires_grad_(True)), "frames_embed"),
                     (dict(g=g.clone().requires_grad_(True)), "guide_embeds"), (dict(fe=None, local_logits=ll.clone().requires_grad_(True)), "local_logits"),
                     (dict(ff=ff.half()), "float16"), (dict(g=g.float()), "float32")):
        with pytest.raises(NotImplementedError, match=word) as e:
            call(m, **kw)
        assert "forward()" in str(e.value) and not m.__dict__.get(store)
    with pytest.raises(ValueError, match="frames_embed=None"):
        call(m, local_logits=ll)
    with pytest.raises(nv.HicomNativeError, match="GPU only"):             # in scope: the first thing that needs a device says so
        call(m)
    assert not m.__dict__.get(store)
