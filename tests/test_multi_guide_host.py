"""CPU checks of the host side of the multi-guide step (csrc/multi_guide.hip, hicom_amd/native.py): the new symbols, the layout of the
argument block as the host C compiler sees it, the workspace arithmetic DESIGN.md §3.8 states, and the refusals of the C entry points
in front of any device call.

As in tests/test_seg_host_pins.py: with chunks > 0 the workspace function and every check in front of the first launch are pure host
code, pointer fields are made-up aligned addresses that nothing reads before a launch, and every *_fwd case breaks one rule, so none
launches."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from hicom_amd import native as nv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDR = 0x7F0000001000                # a made-up address, 4096-byte aligned
EINVAL, EUNSUP = -1, -2
POINTERS = ("ff", "fe", "guide", "out", "newline", "lw0_f16", "lb0", "lw2_f16", "lb2", "wq", "bq", "wk", "wv", "bv", "wo", "bo", "gw0", "gb0", "gw2", "gb2",
            "pe", "kpe")
SYMBOLS = ("hicom_compressor_multiguide_fwd", "hicom_compressor_multiguide_workspace_bytes")


def block(fwd=False, **over):
    """A valid argument block: Q = 3 guides on a 4 x 6 x 6 clip, windows 4 x 3 x 3 (4 of them), hidden 896, fp32 rows, 3 token chunks."""
    a = nv.CompressorMultiGuideArgs()
    a.Q, a.T, a.H, a.W, a.E, a.hidden, a.kt, a.ks, a.nh, a.P = 3, 4, 6, 6, 1152, 896, 4, 3, 9, 0
    a.chunks, a.out_dt, a.l_scale = 3, nv.DT_F32, 0.125
    if fwd:
        for f in POINTERS:
            setattr(a, f, ADDR)
        a.P, a.t_index0, a.y_index0, a.x_index0 = 28, 0, 16, 22
        a.ldo, a.ws, a.ws_bytes = a.hidden, ADDR, 1 << 40
        a.global_row0, a.n_global_rows, a.item_rows = 4, 32, 36
    for k, v in over.items():
        setattr(a, k, v)
    return a


def call(fn, a):
    r = getattr(nv.lib(), f"hicom_compressor_multiguide_{fn}")(None if a is None else ctypes.byref(a))
    return int(r), nv.lib().hicom_last_error().decode()


def test_symbols_are_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "hicom_hip.h")).read()
    declared = set(re.findall(r"\b(hicom_[a-z0-9_]+)\s*\(", header))
    L = nv.lib()
    for name in SYMBOLS:
        assert name in declared and name in nv.EXPORTS and hasattr(L, name)
    assert L.hicom_compressor_multiguide_fwd.restype is ctypes.c_int
    assert L.hicom_compressor_multiguide_workspace_bytes.restype is ctypes.c_int64
    assert "typedef struct hicom_compressor_multiguide_args" in header
    assert nv.ABI_VERSION == L.hicom_abi_version() == 16


SRC = r"""
#include <stddef.h>
#include <stdio.h>
#include "hicom_hip.h"
int main(void) {
    printf("%d %zu %zu %zu %zu\n", HICOM_ABI_VERSION, sizeof(hicom_compressor_multiguide_args), offsetof(hicom_compressor_multiguide_args, Q),
           offsetof(hicom_compressor_multiguide_args, nl_first), offsetof(hicom_compressor_multiguide_args, stream));
    return 0;
}
"""


def test_args_layout_matches_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no host C compiler")
    src = tmp_path / "abi.c"
    src.write_text(SRC)
    exe = tmp_path / "abi"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    ver, size, off_q, off_nl, off_stream = (int(v) for v in subprocess.check_output([str(exe)]).split())
    A = nv.CompressorMultiGuideArgs
    assert ver == nv.ABI_VERSION == 16
    assert size == ctypes.sizeof(A)
    assert off_q == A.Q.offset
    assert off_nl == A.nl_first.offset
    assert off_stream == A.stream.offset and A._fields_[-1][0] == "stream"          # the last field
    assert not hasattr(A, "B")


def _up(n):
    return (n + 255) // 256 * 256


def per_guide_bytes(Q, windows, E, hidden, odt):
    """The Q-sized regions of DESIGN.md §3.8, each rounded up to 256 bytes: qp, o, pre (E floats per guide), hid, tok (hidden floats per
    guide), and per guide and window the fp16 context row, the fp16 hidden row and the readout row of the output dtype."""
    return (3 * _up(Q * E * 4) + 2 * _up(Q * hidden * 4)
            + _up(Q * windows * E * 2) + _up(Q * windows * hidden * 2) + _up(Q * windows * hidden * odt))


@pytest.mark.parametrize("over", [dict(), dict(out_dt=nv.DT_BF16, P=28), dict(T=1, kt=1, H=9, W=9)], ids=["clip_f32", "clip_bf16_pos", "image_9x9"])
def test_workspace_arithmetic(over):
    sizes = [call("workspace_bytes", block(Q=q, **over))[0] for q in range(1, 33)]
    assert all(n > 0 for n in sizes)
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), "workspace_bytes is monotone in Q"
    a = block(**over)
    windows = (a.T // a.kt) * (a.H // a.ks) * (a.W // a.ks)
    odt = 4 if a.out_dt == nv.DT_F32 else 2
    # Q = 1 and Q = 2 share one 32-row pass: every row-sized region (and the logits) is the same, only the per-guide regions grow
    assert sizes[1] - sizes[0] == per_guide_bytes(2, windows, a.E, a.hidden, odt) - per_guide_bytes(1, windows, a.E, a.hidden, odt)
    # the fourth guide opens a second pass of 32 rows: the row-sized regions grow as well
    assert sizes[3] - sizes[2] > per_guide_bytes(4, windows, a.E, a.hidden, odt) - per_guide_bytes(3, windows, a.E, a.hidden, odt)


REFUSALS = {
    "Q = 0": ("workspace_bytes", dict(Q=0), EUNSUP, "1 <= Q <= 32"),
    "Q = 33": ("workspace_bytes", dict(Q=33), EUNSUP, "1 <= Q <= 32"),
    "hidden = 100": ("workspace_bytes", dict(hidden=100), EUNSUP, "multiple of 64"),
    "E = 768": ("workspace_bytes", dict(E=768), EUNSUP, "only 1152"),
    "window of 72 tokens": ("workspace_bytes", dict(T=8, kt=8), EUNSUP, "<= 64"),
    "inexact partition": ("workspace_bytes", dict(H=7), EUNSUP, "exact window partition"),
    "NULL block": ("workspace_bytes", None, EINVAL, "NULL arguments"),
    "fwd: Q = 0": ("fwd", dict(fwd=True, Q=0), EUNSUP, "1 <= Q <= 32"),
    "fwd: Q = 33": ("fwd", dict(fwd=True, Q=33), EUNSUP, "1 <= Q <= 32"),
    "fwd: hidden = 100": ("fwd", dict(fwd=True, hidden=100, ldo=100), EUNSUP, "multiple of 64"),
    "fwd: E = 768": ("fwd", dict(fwd=True, E=768), EUNSUP, "only 1152"),
    "fwd: window of 72 tokens": ("fwd", dict(fwd=True, T=8, kt=8), EUNSUP, "<= 64"),
    "fwd: NULL ff": ("fwd", dict(fwd=True, ff=None), EINVAL, "NULL pointer"),
    "fwd: NULL weight": ("fwd", dict(fwd=True, gw2=None), EINVAL, "NULL weight"),
    "fwd: workspace too small": ("fwd", dict(fwd=True, ws_bytes=4096), EINVAL, "workspace of"),
    "fwd: output layout": ("fwd", dict(fwd=True, item_rows=37), EINVAL, "output layout"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_c_entry_refusals_in_front_of_any_device_call(name):
    fn, kw, code, needle = REFUSALS[name]
    got, msg = call(fn, None if kw is None else block(**kw))
    assert got == code, (got, msg)
    assert msg.startswith("compressor_multiguide: ") and needle in msg, msg
