"""ABI 16 (CPU): the ctypes mirror of hicom_compressor_args in hicom_amd/native.py matches include/hicom_hip.h as the host C compiler
lays it out -- size, and the offset of the appended tok_dt (the dtype of frames_feature / frames_embed)."""
import ctypes
import os
import shutil
import subprocess

import pytest

from hicom_amd import native as nv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <stddef.h>
#include <stdio.h>
#include "hicom_hip.h"
int main(void) {
    printf("%d %zu %zu %zu\n", HICOM_ABI_VERSION, sizeof(hicom_compressor_args), offsetof(hicom_compressor_args, tok_dt),
           offsetof(hicom_compressor_args, ag_bytes2));
    return 0;
}
"""


def test_compressor_args_layout_matches_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no host C compiler")
    src = tmp_path / "abi.c"
    src.write_text(SRC)
    exe = tmp_path / "abi"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    ver, size, off_tok, off_ag2 = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert ver == nv.ABI_VERSION == 16
    assert size == ctypes.sizeof(nv.CompressorArgs)
    assert off_tok == nv.CompressorArgs.tok_dt.offset
    assert off_ag2 == nv.CompressorArgs.ag_bytes2.offset
    assert nv.CompressorArgs().tok_dt == nv.DT_BF16 == 0           # (a zeroed argument block keeps meaning bf16 tokens)
