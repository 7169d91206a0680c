"""CPU checks of the adaptor recipe's batched / ragged entry points: the new argument structs as the host C compiler lays them out
against the ctypes mirrors in hicom_amd/native.py, the existing structs' sizes (the ABI stays 16: the change is additive), the new
symbols, and the scope rule that picks the recipe."""
from types import SimpleNamespace

import pytest

import cases
import hicom_amd
from hicom_amd import batch, native as nv


def ragged_block(adapt):
    args = nv.CompressorRaggedAdaptArgs() if adapt else nv.CompressorRaggedArgs()
    a = args.base if adapt else args
    items = (nv.RaggedItem * 2)(nv.RaggedItem(1, 1, 0, 0, 0, 1, 32), nv.RaggedItem(8, 4, 0, 0, 0, 1, 32))
    a.B, a.H, a.W, a.E, a.hidden, a.ks, a.nh, a.chunks, a.items = 2, 6, 6, 1152, 896, 3, 9, 1, items
    return args, a, items


def test_workspace_grows_by_the_token_sized_planes_only():
    """Host arithmetic, no device call: two fp16 [tokens, E] planes per adapted stream behind the plain layout."""
    plain, _, keep0 = ragged_block(False)
    n0 = nv.compressor_ragged_workspace(plain)
    args, a, keep1 = ragged_block(True)
    with pytest.raises(nv.HicomNativeError, match="neither stream"):
        nv.compressor_ragged_workspace(args)
    plane = 9 * 36 * 1152 * 2
    args.ak.w0 = 256                                   # (an address: the workspace functions read no memory behind it)
    assert nv.compressor_ragged_workspace(args) == n0 + 2 * plane
    args.av.w0 = 256
    assert nv.compressor_ragged_workspace(args) == n0 + 4 * plane
    a.items[1].T = 6                                   # the plain limits carry over
    with pytest.raises(NotImplementedError, match="item 1.*partition"):
        nv.compressor_ragged_workspace(args)
    b = nv.CompressorBatchAdaptArgs()
    b.base.B, b.base.T, b.base.H, b.base.W, b.base.E, b.base.hidden, b.base.kt, b.base.ks, b.base.nh, b.base.chunks = 3, 4, 6, 6, 1152, 896, 4, 3, 9, 1
    b.av.w0 = 256
    assert nv.compressor_batch_workspace(b) == nv.compressor_batch_workspace(b.base) + 2 * (3 * 4 * 36 * 1152 * 2)


@pytest.mark.parametrize("ptype,use_guide,want", [
    ("local43_global32", "direct", "plain"), ("local43_adaptkv_global32", "direct", "adaptkv"), ("local43_adaptk_global32", "direct", "adaptkv"),
    ("local43_adaptv_global32", "direct", "adaptkv"), ("local43_adaptqkvg_global32_adaptg", "direct", None), ("local43_adaptkv_global32", "coarse", None),
    ("local43_adaptkv_global32_adaptg", "direct", None), ("local43_adaptkv_global32", None, None), ("local43_adaptkv", "direct", None)])
def test_scope_rule(ptype, use_guide, want):
    proj = hicom_amd.build_vision_projector(SimpleNamespace(**{**cases.DEFAULT_CFG, "mm_projector_type": ptype, "use_guide": use_guide}))
    assert batch.seg_recipe(proj) == want
