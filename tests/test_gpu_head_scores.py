"""The scores kernel of the logits form on the GPU: hicom_head_guide_fold_fwd + hicom_head_scores_multi_fwd
(csrc/head_scores.hip) against float64 on the same operands, and siglip_head_scores_multi end to end against the float64 head.

Kernel: the cases and bounds of tests/head_scores_inputs.py (derived there; tests/test_head_scores_power.py shows that a kernel which
drops the hidden term or c, takes guide 0's U for every guide or reads the pitch gap as data misses them by a factor of 4 at least).
M = 144, 729 and 16 k + 5; Q = 1, 3, 17, 32; the small head (kpad 256 = ld) everywhere, the pitched plane (kpad 4352, ld 4544) at
M = 144; two `sentinel` cases whose pad columns and pitch gap hold 30000.  The logits [Q][M] lie between two NaN guard rows, rows
q_stride = M + 3 floats apart with NaN between them: every element at its bound, guards and gaps untouched.  Every check prints
`HEAD_SCORES <case> err=<largest error> bound=<bound there> ratio=<largest error / bound>` before it asserts.

End to end: a small head (inter 200) and Q = 3 on 4 x 6 x 6 tokens against LN -> fc1 -> act -> fc2 + residual -> dot in float64.  The
yardstick is siglip_head_scores on the same inputs, guide by guide, against the same float64 values: the new path's largest absolute
error may be at most twice that (U is rounded once more, the sum is associated differently).

Measured on an MI355X: kernel errors <= 2.9e-5 (inter 200) and <= 1.1e-4 (inter 4304), at most 3.2e-4 of the bound; end to end the largest
absolute error per guide is 1.867e-2, 2.089e-2, 1.901e-2 against 1.867e-2, 2.089e-2, 1.900e-2 of siglip_head_scores."""
import pytest
import torch

import head_scores_inputs as hs
from gpu_util import DEV
from hicom_amd import native as nv
from ops_reference import up

pytestmark = pytest.mark.gpu
NAN = float("nan")
D = hs.D


def run_kernel(case):
    c = hs.hs_build(case)
    dev = lambda t: t.to(DEV).contiguous()
    x, hid, g, w2, b2 = dev(c.x), dev(c.hid), dev(c.guides), dev(c.w2), dev(c.b2)
    u_hi, u_lo, u_scale, cc = nv.head_guide_fold(w2, b2, g, nv.head_fold_ldu(c.kpad))
    stride = case.M + 3
    buf = torch.full((case.Q + 2, stride), NAN, dtype=torch.float32, device=DEV)
    out = buf[1:-1]
    nv.head_scores_multi(x, hid, c.kpad, g, u_hi, u_lo, u_scale, cc, out)
    torch.cuda.synchronize()
    return c, buf, out, (u_hi, u_lo, u_scale, cc)


@pytest.mark.parametrize("case", hs.HS_CASES, ids=[c.id for c in hs.HS_CASES])
def test_scores_match_fp64_on_the_same_operands(case):
    c, buf, out, (u_hi, u_lo, u_scale, cc) = run_kernel(case)
    got = out[:, :case.M].double().cpu()
    want, tol = hs.hs_reference(case), hs.hs_tol(case)
    assert bool(torch.isfinite(got).all())
    err = (got - want).abs()
    ratio = err / tol
    i = int(ratio.argmax())
    print(f"HEAD_SCORES {case.id} err={float(err.max()):.3e} bound={float(tol.reshape(-1)[i]):.3e} ratio={float(ratio.reshape(-1)[i]):.3e}")
    assert bool((err <= tol).all()), f"{case.id}: error {float(err.reshape(-1)[i]):.3e} over its bound {float(tol.reshape(-1)[i]):.3e}"
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all()) and bool(torch.isnan(out[:, case.M:]).all()), "a guard was written"
    # the planes of the fold: zero behind inter and behind Q, the row's largest scaled value in [2^14, 2^15)
    assert not bool(u_hi[:, case.inter:].any()) and not bool(u_lo[:, case.inter:].any())
    assert not bool(u_hi[case.Q:].any()) and not bool(u_lo[case.Q:].any()) and not bool(cc[case.Q:].any())
    top = u_hi[:case.Q].float().abs().max(1).values
    assert bool((top >= 2.0 ** 14 - 8).all()) and bool((top <= 2.0 ** 15).all()), top


def test_the_sentinel_does_not_move_the_result():
    """Pad columns and pitch gap at 30000 against the same operands with zeros there: bit for bit."""
    for case in (c for c in hs.HS_CASES if c.sentinel):
        c, _, out, planes = run_kernel(case)
        clean = c.hid.clone()
        clean[:, case.inter:] = 0
        out2 = torch.empty_like(out)
        nv.head_scores_multi(c.x.to(DEV), clean.to(DEV), c.kpad, c.guides.to(DEV), *planes, out2)
        torch.cuda.synchronize()
        assert torch.equal(out[:, :case.M], out2[:, :case.M]), case.id


class SmallHead(torch.nn.Module):
    def __init__(self, inter=200):
        super().__init__()
        g = torch.Generator().manual_seed(20)
        self.layernorm = torch.nn.LayerNorm(D, eps=1e-6)
        self.mlp = torch.nn.Module()
        self.mlp.fc1 = torch.nn.Linear(D, inter)
        self.mlp.fc2 = torch.nn.Linear(inter, D)
        with torch.no_grad():
            self.layernorm.weight.copy_(1 + 0.1 * torch.randn(D, generator=g))
            self.layernorm.bias.copy_(0.1 * torch.randn(D, generator=g))
            self.mlp.fc1.weight.copy_(torch.randn(inter, D, generator=g) / D ** 0.5)
            self.mlp.fc1.bias.copy_(0.1 * torch.randn(inter, generator=g))
            self.mlp.fc2.weight.copy_(torch.randn(D, inter, generator=g) / inter ** 0.5)
            self.mlp.fc2.bias.copy_(0.1 * torch.randn(D, generator=g))


def head_fp64(x, m):
    """LN -> fc1 -> tanh-GELU -> fc2 + residual in float64 from the module's bf16 parameters."""
    ln, fc1, fc2 = m.layernorm, m.mlp.fc1, m.mlp.fc2
    x = up(x.cpu())
    mu, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    n = (x - mu) / torch.sqrt(var + ln.eps) * up(ln.weight.detach().cpu()) + up(ln.bias.detach().cpu())
    h = torch.nn.functional.gelu(n @ up(fc1.weight.detach().cpu()).T + up(fc1.bias.detach().cpu()), approximate="tanh")
    return x + h @ up(fc2.weight.detach().cpu()).T + up(fc2.bias.detach().cpu())


def test_end_to_end_against_the_fp64_head_with_the_single_guide_path_as_yardstick():
    from hicom_amd import siglip_head_scores, siglip_head_scores_multi
    m = SmallHead().to(torch.bfloat16).to(DEV).eval()
    g = torch.Generator().manual_seed(21)
    x = torch.randn(4, 6, 6, D, generator=g).bfloat16().to(DEV)
    guides = torch.randn(3, D, generator=g).bfloat16().to(DEV)
    with torch.no_grad():
        got = siglip_head_scores_multi(x, m, guides)
        one = torch.stack([siglip_head_scores(x, m, guides[q]) for q in range(3)])
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 4, 6, 6)
    want = torch.einsum("thwd,qd->qthw", head_fp64(x, m), up(guides.cpu()))
    e_new = (got.double().cpu() - want).abs().amax((1, 2, 3))
    e_old = (one.double().cpu() - want).abs().amax((1, 2, 3))
    print(f"HEAD_SCORES end-to-end: max-abs per guide new {[f'{float(e):.3e}' for e in e_new]} single-guide {[f'{float(e):.3e}' for e in e_old]}")
    assert float(e_new.max()) <= 2 * float(e_old.max()), (float(e_new.max()), float(e_old.max()))


def test_refusals_of_the_python_entry():
    from hicom_amd import siglip_head_scores_multi
    m = SmallHead().to(torch.bfloat16).to(DEV)
    x = torch.zeros(2, 3, 3, D, dtype=torch.bfloat16, device=DEV)
    g = torch.zeros(3, D, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="autograd"):
        siglip_head_scores_multi(x, m, g)                                   # grad mode, trainable head
    with torch.no_grad():
        with pytest.raises(ValueError, match=r"\[Q, E\]"):
            siglip_head_scores_multi(x, m, g[0])
        with pytest.raises(ValueError, match="1 <= Q <= 32"):
            siglip_head_scores_multi(x, m, torch.zeros(33, D, dtype=torch.bfloat16, device=DEV))
        with pytest.raises(NotImplementedError, match="float16"):
            siglip_head_scores_multi(x.half(), m, g)
        with pytest.raises(NotImplementedError, match="float16"):
            siglip_head_scores_multi(x, m, g.half())
