"""CPU checks of the adaptor recipe's batched / ragged entry points: the new argument structs as the host C compiler lays them out
against the ctypes mirrors in hicom_amd/native.py, the existing structs' sizes (the ABI stays 16: the change is additive), the new
symbols, and the scope rule that picks the recipe."""
import ctypes
import os
import shutil
import subprocess
from types import SimpleNamespace

import pytest

import cases
import hicom_amd
from hicom_amd import batch, native as nv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hicom_compressor_batch_adapt_workspace_bytes", "hicom_compressor_batch_adapt_fwd", "hicom_compressor_ragged_adapt_workspace_bytes",
       "hicom_compressor_ragged_adapt_prepare", "hicom_compressor_ragged_adapt_fwd")
# sizeof of the existing argument structs at the parent commit of this feature (x86-64, from the same C snippet)
PARENT_SIZES = {"hicom_compressor_args": 1168, "hicom_compressor_batch_args": 320, "hicom_compressor_ragged_args": 272, "hicom_ragged_item": 28}

SRC = r"""
#include <stddef.h>
#include <stdio.h>
#include "hicom_hip.h"
#define B hicom_compressor_batch_adapt_args
#define R hicom_compressor_ragged_adapt_args
int main(void) {
    printf("%d\n", HICOM_ABI_VERSION);
    printf("%zu %zu %zu %zu\n", sizeof(hicom_compressor_args), sizeof(hicom_compressor_batch_args), sizeof(hicom_compressor_ragged_args),
           sizeof(hicom_ragged_item));
    printf("%zu %zu %zu\n", sizeof(hicom_seg_adaptor), offsetof(hicom_seg_adaptor, w2_f16), offsetof(hicom_seg_adaptor, alpha));
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(B), offsetof(B, base), offsetof(B, ak), offsetof(B, av), offsetof(B, alpha_dt), offsetof(B, eps));
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(R), offsetof(R, base), offsetof(R, ak), offsetof(R, av), offsetof(R, alpha_dt), offsetof(R, eps));
    return 0;
}
"""


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no host C compiler")
    d = tmp_path_factory.mktemp("seg_adapt_abi")
    src, exe = d / "abi.c", d / "abi"
    src.write_text(SRC)
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return [[int(v) for v in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]


def test_abi_version_is_still_16(layout):
    assert layout[0] == [16] and nv.ABI_VERSION == 16


def test_existing_structs_keep_their_sizes(layout):
    assert layout[1] == [PARENT_SIZES[k] for k in ("hicom_compressor_args", "hicom_compressor_batch_args", "hicom_compressor_ragged_args",
                                                   "hicom_ragged_item")]
    assert [ctypes.sizeof(t) for t in (nv.CompressorArgs, nv.CompressorBatchArgs, nv.CompressorRaggedArgs, nv.RaggedItem)] == layout[1]


def test_new_structs_match_the_ctypes_mirrors(layout):
    A = nv.SegAdaptor
    assert layout[2] == [ctypes.sizeof(A), A.w2_f16.offset, A.alpha.offset]
    assert [n for n, _ in A._fields_] == ["w0", "b0", "w2_f16", "b2", "gamma", "beta", "alpha"]
    for line, T, base in ((layout[3], nv.CompressorBatchAdaptArgs, nv.CompressorBatchArgs), (layout[4], nv.CompressorRaggedAdaptArgs, nv.CompressorRaggedArgs)):
        assert line == [ctypes.sizeof(T), T.base.offset, T.ak.offset, T.av.offset, T.alpha_dt.offset, T.eps.offset]
        assert T.base.offset == 0 and T.ak.offset == ctypes.sizeof(base)           # the plain block first, untouched
        assert T().ak.w0 is None and T().av.w0 is None                              # a zeroed block adapts neither stream


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "hicom_hip.h")).read()
    lib = ctypes.CDLL(nv.LIB_PATH)                     # loading needs no GPU; no compute call is made
    for name in NEW:
        assert name + "(" in header and name in nv.EXPORTS and hasattr(lib, name)
        assert len(getattr(nv.lib(), name).argtypes) == 1
    assert nv.lib().hicom_compressor_batch_adapt_workspace_bytes.restype is ctypes.c_int64
    assert nv.lib().hicom_compressor_ragged_adapt_workspace_bytes.restype is ctypes.c_int64
    assert nv.lib().hicom_compressor_ragged_adapt_fwd.restype is ctypes.c_int


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
