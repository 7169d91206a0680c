"""What the CPU tests of the host side share: the header, the made-up device address and the status codes of the C refusals, a projector
on the CPU, the stand-in for `nv` that fails a host test on any native call, and the one place that compiles and runs a C program against
include/hicom_hip.h."""
import os
import shutil
import subprocess
import tempfile
from types import SimpleNamespace

import pytest
import torch

import cases
import hicom_amd
from hicom_amd import native as nv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "hicom_hip.h")).read()
ADDR = 0x7F0000001000                # a made-up address, 4096-byte aligned: nothing reads behind it before a launch
EINVAL, EUNSUP = -1, -2


def module(ptype="local43_global32", use_guide="direct", dtype=torch.bfloat16, **cfg_over):
    cfg = SimpleNamespace(**{**cases.DEFAULT_CFG, "hidden_size": 64, "mm_projector_type": ptype, "use_guide": use_guide, **cfg_over})
    return hicom_amd.build_vision_projector(cfg).to(dtype).eval()


def tokens(Tc, H=6, W=6, E=cases.D, dtype=torch.bfloat16):
    return torch.zeros((Tc, H, W, E), dtype=dtype)


class NoNative:
    """`nv` as clip_stream sees it during a host test: the constants and classes of the real module; any function call fails the test."""

    def __getattr__(self, name):
        real = getattr(nv, name)
        if isinstance(real, type) or not callable(real):
            return real

        def refuse(*a, **k):
            pytest.fail(f"native call nv.{name} in a host test")
        return refuse


def compile_and_run(source):
    """Compiles `source` as C99 against include/ with the host C compiler, runs it and returns what it printed."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no host C compiler")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "abi.c"), os.path.join(d, "abi")
        with open(src, "w") as f:
            f.write(source)
        subprocess.check_call([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        return subprocess.check_output([exe]).decode()
