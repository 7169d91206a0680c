"""fp16 token stream of the release step: an fp16 projector given fp16 frames_feature / frames_embed / guide runs the fused stream kernel's
fp16 instantiation on the tokens themselves (no cast, no rounding to bf16) and writes its fp16 (or f32) output from the fp32 accumulators.

Oracle: oracle.hicom_oracle.projector_forward in fp32 on the exact fp16 input values, with the case's (bf16-representable) weights.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cases
from gpu_util import build_module
from hicom_amd import native as nv
from oracle_util import run_oracle

pytestmark = pytest.mark.gpu
TOL = 1e-3

# the C2 benchmark shape: 64 frames of a 27 x 27 grid, LLM width 896, full output
cases.CASES_EXTRA.setdefault("F16_C2", dict(cfg=dict(hidden_size=896), T=64, h=27, w=27))


def _fp16_detail(x, seed):
    """x (bf16-representable f32) plus a relative perturbation of ~2^-10, rounded to fp16: values that use fp16's 11 significand bits."""
    g = torch.Generator().manual_seed(seed)
    t = torch.from_numpy(np.ascontiguousarray(x)).float()
    return (t * (1.0 + 2.0 ** -10 * torch.randn(t.shape, generator=g))).half().float().numpy()


def _below_bf16(x):
    """bf16-representable values plus a same-signed offset of 3/8 of a bf16 ulp (exact in fp16, removed by rounding to bf16) on every
    element whose fp16 representation keeps it."""
    b = torch.from_numpy(np.ascontiguousarray(x)).float().to(torch.bfloat16).float()
    e = torch.floor(torch.log2(b.abs().clamp_min(1e-30)))
    h = (b + torch.sign(b) * 0.375 * torch.exp2(e - 7) * (e >= -13)).half().float()
    assert torch.equal(h.to(torch.bfloat16).float(), b)
    return h.numpy()


def _f16_case(case, fn):
    c = SimpleNamespace(**vars(case))
    c.ff, c.fe = fn(case.ff, 1), fn(case.fe, 2)
    c.g = None if case.g is None else fn(case.g, 3)
    c.newline = None if case.newline is None else fn(case.newline, 4)
    return c


def _dev16(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).half().cuda()


def _inputs(c):
    return _dev16(c.ff), _dev16(c.fe), _dev16(c.g), c.modal, _dev16(c.newline)


def _fused_plan(m):
    """The plan the fp16 module's last call ran: the fused release step on fp16 tokens."""
    plan = m.__dict__["_bf16_twin"][0].__dict__["_last_plan"]
    assert plan.args.tok_dt == nv.DT_F16 and nv.compressor_is_fused(plan.args)
    return plan


@pytest.mark.parametrize("name", ["G1_direct_T8", "G11_c1_shape", "F16_C2"])
def test_fp16_tokens_output_precision(name):
    case = cases.build_case(name)
    c = _f16_case(case, _fp16_detail)
    m = build_module(case, fp32_out=True).half()
    want = run_oracle(c)["out"].numpy()
    with torch.no_grad():
        out = m(*_inputs(c))
        _fused_plan(m)
        assert out.dtype == torch.float32
        err = float(np.abs(out.cpu().numpy() - want).max())
        assert err <= TOL, err
        m.return_fp32 = False
        out16 = m(*_inputs(c))
        _fused_plan(m)
        assert out16.dtype == torch.float16
        err16 = float(np.abs(out16.float().cpu().numpy() - want).max())
        assert err16 <= TOL + 2.0 ** -11 * float(np.abs(want).max()), err16


def test_fp16_tokens_keep_detail_below_bf16():
    case = cases.build_case("G10_peaky_direct")
    case.ff, case.fe = case.ff * 4.0, case.fe * 4.0                 # (powers of two: still bf16-representable; sharper logits)
    c = _f16_case(case, lambda x, seed: _below_bf16(x))
    want = run_oracle(c)["out"].numpy()
    rounded = SimpleNamespace(**vars(c))
    rounded.ff, rounded.fe, rounded.g = (torch.from_numpy(v).to(torch.bfloat16).float().numpy() for v in (c.ff, c.fe, c.g))
    assert float(np.abs(run_oracle(rounded)["out"].numpy() - want).max()) >= 10 * TOL     # (the detail matters at this tolerance)
    m = build_module(case, fp32_out=True).half()
    with torch.no_grad():
        out = m(*_inputs(c))
    _fused_plan(m)
    err = float(np.abs(out.cpu().numpy() - want).max())
    assert err <= TOL, err


def test_fp16_tokens_allocate_no_token_sized_temporaries():
    case = cases.build_case("F16_C2")
    m = build_module(case, fp32_out=False).half()
    args = _inputs(_f16_case(case, _fp16_detail))
    with torch.no_grad():
        m(*args)                                                    # warm: twin, plan, workspace, tables
        _fused_plan(m)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = m(*args)
        torch.cuda.synchronize()
    assert out.dtype == torch.float16
    assert torch.cuda.max_memory_allocated() - base < 32 * 2 ** 20        # the cast path allocated 2 x 107.5 MB of bf16 copies


def test_fp16_tokens_deterministic_and_fallbacks():
    case = cases.build_case("G1_direct_T8")
    c = _f16_case(case, _fp16_detail)
    m = build_module(case, fp32_out=True).half()
    args = _inputs(c)
    with torch.no_grad():
        a = m(*args).clone()
        b = m(*args)
    _fused_plan(m)
    assert torch.equal(a, b)

    # mixed call (fp16 frames_feature, bf16 frames_embed): the cast path -- the fp16 tensors rounded to bf16 -- within the oracle's bound
    ff, fe, g, modal, nl = args
    rounded = _f16_case(c, lambda x, seed: torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).float().numpy())
    with torch.no_grad():
        out = m(ff, fe.to(torch.bfloat16), g, modal, nl)
    assert m.__dict__["_bf16_twin"][0].__dict__["_last_plan"].args.tok_dt == nv.DT_BF16
    want = run_oracle(rounded)["out"].numpy()
    assert float(np.abs(out.cpu().numpy() - want).max()) <= TOL

    # a guide-off fp16 module: not the release step, the cast path
    off = cases.build_case("G2_off_T8")
    co = _f16_case(off, lambda x, seed: torch.from_numpy(np.ascontiguousarray(x)).half().float().numpy())
    mo = build_module(off, fp32_out=True).half()
    with torch.no_grad():
        out = mo(*_inputs(co))
    want = run_oracle(co)["out"].numpy()
    assert float(np.abs(out.cpu().numpy() - want).max()) <= TOL
    plan = mo.__dict__["_bf16_twin"][0].__dict__["_last_plan"]
    assert plan.args.tok_dt == nv.DT_BF16 and not nv.compressor_is_fused(plan.args)

    # the generic recipe's plan told that its tokens are fp16: refused, never read as bf16
    a16 = plan.args
    a16.tok_dt = nv.DT_F16
    try:
        assert not nv.compressor_is_fused(a16)
        with pytest.raises(nv.HicomNativeError, match=r"\(-2\)"):
            nv.compressor_fwd(a16)
    finally:
        a16.tok_dt = nv.DT_BF16
