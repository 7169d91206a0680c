"""The whole C surface against include/hicom_hip.h, once (CPU: the built library and the host C compiler, no device).

Names:       the prototypes of the header are the rows of native.SIGNATURES and the exports of the library; the ABI version.
Signatures:  return type and every parameter of every prototype against the restype / argtypes bound on the loaded library.
Structs:     every ctypes.Structure of native.py against the header as the host C compiler lays it out -- field names in order, offsets,
             field sizes, total size -- from ONE generated C program, compiled once per session.
Frozen:      the sizes that the features pinned when they were added.
The small named tests behind them hold what the rules do not imply: which block embeds which, last fields, zeroed blocks, the Python
entry points of the features."""
import ctypes
import functools
import inspect
import re

import pytest

import hicom_amd
from hicom_amd import clip_stream as cs
from hicom_amd import native as nv
from hicom_amd.projector import HIComProjector
from host_util import HEADER, compile_and_run

CODE = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))                     # the header without its comments
PROTOTYPES = {name: (ret, [" ".join(p.split()) for p in params.split(",")])
              for ret, name, params in re.findall(r"^(int|int64_t|const char\*)\s+(hicom_\w+)\s*\(([^)]*)\)\s*;", CODE, flags=re.M)}

# C type name -> ctypes mirror.  The two types declared inside hicom_compressor_args are reached with their struct tag (C99).
STRUCTS = {
    "hicom_axis": nv.Axis, "hicom_aux_gemv": nv.AuxGemv, "hicom_r16_role": nv.R16Role, "hicom_r16_gemm": nv.R16Gemm,
    "struct hicom_adaptor": nv.Adaptor, "struct hicom_injector": nv.Injector, "hicom_compressor_args": nv.CompressorArgs,
    "hicom_compressor_batch_args": nv.CompressorBatchArgs, "hicom_ragged_item": nv.RaggedItem,
    "hicom_compressor_ragged_args": nv.CompressorRaggedArgs, "hicom_seg_adaptor": nv.SegAdaptor,
    "hicom_compressor_batch_adapt_args": nv.CompressorBatchAdaptArgs, "hicom_compressor_ragged_adapt_args": nv.CompressorRaggedAdaptArgs,
    "hicom_compressor_multiguide_args": nv.CompressorMultiGuideArgs, "hicom_compressor_multiguide_adapt_args": nv.CompressorMultiGuideAdaptArgs,
    "hicom_compressor_ragged_multiguide_args": nv.CompressorRaggedMultiGuideArgs,
    "hicom_compressor_clips_multiguide_args": nv.CompressorClipsMultiGuideArgs,
    "hicom_stream_push_args": nv.StreamPushArgs, "hicom_stream_push_multi_args": nv.StreamPushMultiArgs,
    "hicom_stream_push_multi_adapt_args": nv.StreamPushMultiAdaptArgs, "hicom_stream_group_push_args": nv.StreamGroupPushArgs,
    "hicom_stream_group_multi_push_args": nv.StreamGroupMultiPushArgs, "hicom_stream_group_adapt_push_args": nv.StreamGroupAdaptPushArgs,
}

# sizeof on x86-64 as the tests of the features stated them when each block was added: a block that an earlier entry point takes never grows
FROZEN_SIZES = {
    "hicom_compressor_args": 1168, "hicom_compressor_batch_args": 320, "hicom_compressor_ragged_args": 272, "hicom_ragged_item": 28,
    "hicom_seg_adaptor": 56, "hicom_stream_push_args": 280, "hicom_stream_push_multi_args": 344, "hicom_stream_push_multi_adapt_args": 496,
    "hicom_stream_group_push_args": 744, "hicom_stream_group_multi_push_args": 1008,
}

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float}


def allowed(ctype):
    """The ctypes types that may stand for one C parameter type (or return type) of the header."""
    if ctype == "const char*":
        return (ctypes.c_char_p,)                               # hicom_last_error: a C string
    if ctype in SCALARS:
        return (SCALARS[ctype],)                                # a scalar by value: its ctypes scalar
    if ctype == "hicom_axis":
        return (nv.Axis,)                                       # the one struct that travels by value
    struct = re.fullmatch(r"(?:const )?(hicom_\w+)\*", ctype)
    if struct:
        return (ctypes.POINTER(STRUCTS[struct.group(1)]),)      # a pointer to a struct: a pointer to the mirror of exactly that struct
    if re.fullmatch(r"(?:const )?int32_t\*", ctype):
        return (ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p)        # a host array of ints (a ctypes array) or a device address
    assert ctype.endswith("*"), f"no rule for the C type {ctype!r}"
    return (ctypes.c_void_p,)                                   # every other pointer: an address


def test_the_prototypes_are_the_table_rows_and_the_exports():
    assert set(PROTOTYPES) == set(nv.SIGNATURES), set(PROTOTYPES) ^ set(nv.SIGNATURES)
    assert nv.EXPORTS == tuple(nv.SIGNATURES) and len(set(nv.EXPORTS)) == len(nv.EXPORTS)
    raw = ctypes.CDLL(nv.LIB_PATH)                              # loading needs no GPU; no compute call is made
    assert [name for name in nv.SIGNATURES if not hasattr(raw, name)] == []
    assert nv.ABI_VERSION == nv.lib().hicom_abi_version() == 16 and "#define HICOM_ABI_VERSION 16" in HEADER


@pytest.mark.parametrize("name", list(PROTOTYPES))
def test_signature_matches_the_header(name):
    ret, params = PROTOTYPES[name]
    fn = getattr(nv.lib(), name)
    assert fn.restype in allowed(ret), f"{name}: returns {ret}, bound as {fn.restype}"
    params = [] if params == ["void"] else params
    assert len(fn.argtypes) == len(params), f"{name}: {len(params)} parameters in the header, {len(fn.argtypes)} argtypes"
    for i, (param, bound) in enumerate(zip(params, fn.argtypes)):
        assert bound in allowed(re.sub(r"\s*\w+$", "", param)), f"{name}: parameter {i} is `{param}`, bound as {bound}"


def test_every_structure_of_the_binding_has_a_row():
    mirrors = {obj for _, obj in inspect.getmembers(nv, inspect.isclass) if issubclass(obj, ctypes.Structure) and obj.__module__ == nv.__name__}
    assert mirrors == set(STRUCTS.values()), {m.__name__ for m in mirrors ^ set(STRUCTS.values())}
    assert len(set(STRUCTS.values())) == len(STRUCTS) == 23


def header_fields(ctype):
    """The top-level field names of one struct of the header, in order."""
    if ctype.startswith("struct "):                              # declared inside another struct: no further nesting
        body = re.search(r"%s \{(.*?)\}" % ctype, CODE, flags=re.S).group(1)
    else:
        body = re.search(r"typedef struct %s \{(.*?)\n\} %s;" % (ctype, ctype), CODE, flags=re.S).group(1)
        body = re.sub(r"(struct hicom_\w+) \{.*?\}", r"\1", body, flags=re.S)                # a nested declaration: its declarators stay
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        names += [re.search(r"(\w+)\s*(?:\[[^\]]*\])?$", d.strip()).group(1) for d in decl.split(",")]
    return names


@functools.lru_cache(maxsize=None)
def c_layouts():
    """{C type name: (sizeof, [(offsetof, sizeof) per field of the mirror])} from one C program, compiled once per session."""
    lines = []
    for ctype, mirror in STRUCTS.items():
        lines.append(f'    printf("%zu", sizeof({ctype}));')
        lines += [f'    printf(" %zu %zu", offsetof({ctype}, {f}), sizeof((({ctype}*)0)->{f}));' for f, _ in mirror._fields_]
        lines.append(r'    printf("\n");')
    out = compile_and_run('#include <stddef.h>\n#include <stdio.h>\n#include "hicom_hip.h"\nint main(void) {\n'
                          '    printf("%d\\n", HICOM_ABI_VERSION);\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    version, *rows = out.splitlines()
    assert int(version) == nv.ABI_VERSION == 16 and len(rows) == len(STRUCTS)
    rows = [[int(v) for v in row.split()] for row in rows]
    return {ctype: (row[0], list(zip(row[1::2], row[2::2]))) for ctype, row in zip(STRUCTS, rows)}


@pytest.mark.parametrize("ctype", list(STRUCTS))
def test_struct_matches_the_header_field_for_field(ctype):
    mirror = STRUCTS[ctype]
    names = [f for f, _ in mirror._fields_]
    assert names == header_fields(ctype), f"{mirror.__name__}: field names or their order differ from {ctype}"
    size, fields = c_layouts()[ctype]
    for name, (offset, width) in zip(names, fields):
        got = getattr(mirror, name)
        assert (got.offset, got.size) == (offset, width), f"{mirror.__name__}.{name}: (offset, size) {got.offset, got.size}, the header has {offset, width}"
    assert ctypes.sizeof(mirror) == size, f"{mirror.__name__}: {ctypes.sizeof(mirror)} bytes, {ctype} has {size}"
    assert f"typedef struct {ctype} {{" in HEADER or ctype.startswith("struct ")


@pytest.mark.parametrize("ctype", list(FROZEN_SIZES))
def test_earlier_blocks_keep_their_sizes(ctype):
    assert c_layouts()[ctype][0] == ctypes.sizeof(STRUCTS[ctype]) == FROZEN_SIZES[ctype], f"{ctype} changed its size"


# ---- what the rules above do not imply ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in nv.SIGNATURES if n.endswith("_workspace_bytes")])
def test_workspace_functions_return_64_bits(name):
    assert getattr(nv.lib(), name).restype is ctypes.c_int64


EMBEDS = [(nv.CompressorBatchAdaptArgs, nv.CompressorBatchArgs), (nv.CompressorRaggedAdaptArgs, nv.CompressorRaggedArgs),
          (nv.CompressorMultiGuideAdaptArgs, nv.CompressorMultiGuideArgs), (nv.CompressorClipsMultiGuideArgs, nv.CompressorRaggedMultiGuideArgs),
          (nv.StreamPushMultiAdaptArgs, nv.StreamPushMultiArgs), (nv.StreamGroupAdaptPushArgs, nv.StreamGroupMultiPushArgs)]


@pytest.mark.parametrize("T,base", EMBEDS, ids=[T.__name__ for T, _ in EMBEDS])
def test_an_extended_block_starts_with_the_plain_block_untouched(T, base):
    assert T._fields_[0] == ("base", base) and [n for n, _ in T._fields_[1:3]] == ["ak", "av"]
    assert T.base.offset == 0 and T.ak.offset == ctypes.sizeof(base)
    assert T().ak.w0 is None and T().av.w0 is None                              # a zeroed block adapts neither stream


def test_last_fields():
    for T in (nv.CompressorMultiGuideArgs, nv.CompressorRaggedMultiGuideArgs, nv.StreamPushArgs, nv.StreamPushMultiArgs, nv.StreamGroupPushArgs,
              nv.StreamGroupMultiPushArgs):
        assert T._fields_[-1][0] == "stream", T.__name__
    assert [n for n, _ in nv.StreamPushMultiAdaptArgs._fields_][-2:] == ["alpha_dt", "eps"]
    assert [n for n, _ in nv.StreamGroupAdaptPushArgs._fields_] == ["base", "ak", "av", "alpha_dt", "eps"]
    assert [n for n, _ in nv.SegAdaptor._fields_] == ["w0", "b0", "w2_f16", "b2", "gamma", "beta", "alpha"]
    assert tuple(n for n, _ in nv.CompressorMultiGuideAdaptArgs._fields_) == ("base", "ak", "av", "ky", "vy", "alpha_dt", "eps")
    assert tuple(n for n, _ in nv.CompressorClipsMultiGuideArgs._fields_) == ("base", "ak", "av", "alpha_dt", "eps", "item_ptrs")


def test_group_arrays_hold_one_int_per_slot():
    assert nv.StreamGroupPushArgs.tc.size == 4 * nv.GROUP_MAX == 128
    assert nv.StreamGroupMultiPushArgs.pair0.size == 4 * nv.GROUP_MAX == 128


def test_zeroed_blocks_mean_the_plain_recipe():
    assert nv.CompressorArgs().tok_dt == nv.DT_BF16 == 0           # (a zeroed argument block keeps meaning bf16 tokens)
    z = nv.CompressorMultiGuideAdaptArgs()
    assert z.ky is None and z.vy is None and z.ak.w0 is None and z.av.w0 is None                  # a zeroed block adapts neither stream
    z = nv.CompressorClipsMultiGuideArgs()
    assert z.item_ptrs is None and z.ak.w0 is None and z.av.w0 is None and z.base.ff is None      # a zeroed block: the plain recipe


def test_multi_guide_blocks_are_the_plain_blocks_with_the_guides():
    assert not hasattr(nv.CompressorMultiGuideArgs, "B")
    A = nv.CompressorRaggedMultiGuideArgs
    assert ctypes.sizeof(A) == ctypes.sizeof(nv.CompressorRaggedArgs) + 16
    # every field of the ragged block, in its order, with the guide counts behind `items`
    names = [n for n, _ in A._fields_]
    assert [n for n in names if n not in ("guide_counts", "n_guide_counts", "reserved_")] == [n for n, _ in nv.CompressorRaggedArgs._fields_]
    assert names[names.index("items") + 1:names.index("items") + 4] == ["guide_counts", "n_guide_counts", "reserved_"]
    assert ctypes.sizeof(nv.StreamPushArgs) != ctypes.sizeof(nv.StreamPushMultiArgs)               # (the single-guide block is another struct, untouched)


def test_the_python_entry_points_of_the_features_are_there():
    for entry in ("forward_ragged_multi_guide", "forward_prepared_many"):
        assert callable(getattr(HIComProjector, entry))
    for entry in ("open_stream", "open_stream_multi", "open_stream_adapt", "open_stream_group"):
        assert hasattr(hicom_amd.HIComProjector, entry)
    assert issubclass(cs.ClipStreamAdapt, cs.ClipStreamMulti)
