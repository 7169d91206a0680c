"""CPU checks of the batched step's surface: header, binding and module agree on the new entry points."""
import ctypes
import os
import re

import hicom_amd
from hicom_amd import native
from hicom_amd.projector import HIComProjector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "hicom_hip.h")).read()
NEW = ("hicom_compressor_batch_fwd", "hicom_compressor_batch_workspace_bytes")


def test_batch_entry_points_are_declared_exported_and_bound():
    lib = ctypes.CDLL(native.LIB_PATH)                 # loading needs no GPU; no compute call is made
    for name in NEW:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", HEADER)
        assert m, f"{name} is not declared in include/hicom_hip.h"
        assert name in native.EXPORTS and hasattr(lib, name)
        n_declared = len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(native.lib(), name).argtypes) == n_declared == 1
    assert native.lib().hicom_compressor_batch_workspace_bytes.restype is ctypes.c_int64
    assert native.ABI_VERSION == 16 and "#define HICOM_ABI_VERSION 16" in HEADER


def test_batch_args_struct_matches_the_header_field_for_field():
    body = re.search(r"typedef struct hicom_compressor_batch_args \{(.*?)\} hicom_compressor_batch_args;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    declared = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        base = re.match(r"(const\s+)?(\w+)", stmt).group(2)
        for var in stmt[re.match(r"(const\s+)?\w+", stmt).end():].split(","):
            var = var.strip()
            declared.append((var.lstrip("* "), ctypes.c_void_p if var.startswith("*") or "*" in stmt.split(var)[0][-2:] else ctype[base]))
    assert [(n, t) for n, t in native.CompressorBatchArgs._fields_] == declared


def test_projector_has_forward_batch_and_the_package_exports_nothing_new():
    assert callable(getattr(HIComProjector, "forward_batch"))
    assert not any("batch" in n.lower() for n in getattr(hicom_amd, "__all__", dir(hicom_amd)) if n != "batch")
