"""The logits form of the ragged multi-guide step on the GPU: HIComProjector.forward_ragged_multi_guide(local_logits=)
on MIX6 and MIX9 of tests/ragged_multi_guide_inputs.py, with and without image_newline, and hicom_amd.siglip_head_scores_ragged end to end.

Step.  The kernel receives EXACT logits -- frames_embed . guide in float64, rounded to fp32 once, as tests/test_gpu_multi_guide_logits.py
makes them -- in the layout [max Q_i, sum T_i, H, W], with NaN in every cell with q >= Q_i: a kernel that walks max Q_i guides, or another
item's planes, carries the NaN into its output.  Against
  the keyed form on the same inputs   global rows bit for bit (launch 3 does not reach them), every other row within 2e-3, the bar
                                      tests/test_gpu_multi_guide_logits.py holds for the same comparison
  forward_multi_guide(local_logits=)  per item on the item's slice of the logits: one device body and the same logits, so the local rows
                                      are expected bit-equal; asserted <= 2e-3, the largest difference printed
  the oracle                          per pair and region through ragged_multi_guide_inputs.check_pair
The two forms keep their own plans in the step's store.

End to end.  siglip_head_scores_ragged on a stacked (1, 4, 1)-frame batch of 6 x 6 tokens with Q (1, 3, 5) and a small head (inter 200)
against the float64 head; the yardstick is siglip_head_scores_multi on the same item: per pair the new path's largest error may be at
most twice that (the rule of DESIGN.md §3.18).

Measured on an MI355X: local rows 3.3e-6 .. 5.2e-5 from the keyed form and 0 (bit-equal) from forward_multi_guide(local_logits=), whose
global rows differ by <= 2.4e-6 (another division of the stream); oracle local 3.7e-5 .. 1.8e-4, global <= 2.3e-6; end to end 1.4e-2 .. 2.5e-2
per pair, equal to siglip_head_scores_multi's to the printed digits."""
import numpy as np
import pytest
import torch

import ragged_multi_guide_inputs as ri
from gpu_util import DEV, build_module, dev_bf16
from ops_reference import up
from test_gpu_head_scores import SmallHead, head_fp64

pytestmark = pytest.mark.gpu
NAN = float("nan")
NG = ri.NG
D = ri.D
STORE = "_ragged_multi_guide_plans"
TOL_FORWARD = 2e-3

# MIX9 with image_newline: the table of tests/ragged_multi_guide_inputs.py has the mix without it only
ri.BY_ID.setdefault("rmg_mix9_newline_grid", ri.Entry("rmg_mix9_newline_grid", ri.MIX9, "edge", newline="grid"))
IDS = ["rmg_mix6", "rmg_mix6_newline_grid", "rmg_mix9", "rmg_mix9_newline_grid"]


def exact_logits(c):
    """fp32 [max Q_i, sum T_i, H, W]: frames_embed . guide q of the item in float64, rounded once; NaN wherever q >= Q_i."""
    L = torch.full((max(c.counts), sum(c.splits), c.h, c.w), NAN, dtype=torch.float32)
    t = 0
    for fe, g, T, Q in zip(c.fe, c.g, c.splits, c.counts):
        L[:Q, t:t + T] = torch.einsum("thwd,qd->qthw", up(torch.from_numpy(fe).bfloat16()), up(torch.from_numpy(g).bfloat16())).float()
        t += T
    return L.to(DEV)


def stacked(c):
    return dev_bf16(np.concatenate(c.ff)), dev_bf16(np.concatenate(c.fe)), dev_bf16(np.concatenate(c.g)), dev_bf16(c.newline)


@pytest.mark.parametrize("id", IDS)
def test_step_with_logits_against_the_keyed_form_the_one_clip_form_and_the_oracle(id):
    c, want = ri.build(id), ri.oracle_outputs(id)
    m = build_module(c)
    ff, fe, g, nl = stacked(c)
    L = exact_logits(c)
    with torch.no_grad():
        keyed = m.forward_ragged_multi_guide(ff, fe, g, c.splits, c.counts, c.modals, nl)
        out = m.forward_ragged_multi_guide(ff, None, g, c.splits, c.counts, c.modals, nl, local_logits=L)
        plans = dict(m.__dict__[STORE])
        again = m.forward_ragged_multi_guide(ff, fe, g, c.splits, c.counts, c.modals, nl)
        stored = dict(m.__dict__[STORE])
        # (the one-clip step comes last: it builds plans of its own on the module)
        single, t = [], 0
        for i, (T, Q) in enumerate(zip(c.splits, c.counts)):
            single.append(m.forward_multi_guide(dev_bf16(c.ff[i]), None, dev_bf16(c.g[i]), c.modals[i], nl, local_logits=L[:Q, t:t + T].contiguous()))
            t += T
    torch.cuda.synchronize()
    assert len(out) == len(keyed) == c.B
    e_keyed, e_single, e_single_global = [], [], []
    for i in range(c.B):
        assert out[i].dtype == torch.float32 and out[i].shape == keyed[i].shape == single[i].shape, (i, out[i].shape, keyed[i].shape, single[i].shape)
        assert bool(torch.isfinite(out[i]).all()), f"item {i}: a logits cell with q >= Q_i reached the output"
        assert torch.equal(out[i][:, -NG:], keyed[i][:, -NG:]), f"item {i}: the global rows changed"
        e_keyed.append(float((out[i][:, :-NG] - keyed[i][:, :-NG]).abs().max()))
        e_single.append(float((out[i][:, :-NG] - single[i][:, :-NG]).abs().max()))
        e_single_global.append(float((out[i][:, -NG:] - single[i][:, -NG:]).abs().max()))     # (another stream division: not this launch)
    print(f"forward_ragged_multi_guide(local_logits=) {id}: max-abs of the local rows per item vs the keyed form {['%.3e' % e for e in e_keyed]}, "
          f"vs forward_multi_guide(local_logits=) {['%.3e' % e for e in e_single]} (its global rows {['%.3e' % e for e in e_single_global]})")
    assert max(e_keyed) <= TOL_FORWARD and max(e_single) <= TOL_FORWARD and max(e_single_global) <= TOL_FORWARD
    bad = []
    for (i, q), w in want.items():
        bad += ri.check_pair(c, f"pair ({i}, {q})", out[i][q].cpu().numpy(), w, i)
    assert not bad, f"{id}: " + "; ".join(bad)
    # plans: one per form in the one store; the keyed form finds its own again
    assert len(plans) == 2 and sum(k[-1] == "logits" for k in plans) == 1
    (keyed_key,) = [k for k in plans if k[-1] != "logits"]
    assert len(stored) == 2 and stored[keyed_key] is plans[keyed_key]
    assert all(torch.equal(a, b) for a, b in zip(again, keyed))


def test_refusals_on_the_new_keyword_are_those_of_the_keyed_call():
    c = ri.build("rmg_mix6")
    m = build_module(c)
    ff, fe, g, _ = stacked(c)
    L = exact_logits(c)
    args = (g, c.splits, c.counts, c.modals, None)
    with pytest.raises(RuntimeError, match="autograd"):
        m.forward_ragged_multi_guide(ff, None, *args, local_logits=L)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="float16"):
            m.forward_ragged_multi_guide(ff.half(), None, *args, local_logits=L)
        with pytest.raises(ValueError, match="float32"):
            m.forward_ragged_multi_guide(ff, None, *args, local_logits=L.double())
        with pytest.raises(ValueError, match="device tensor"):
            m.forward_ragged_multi_guide(ff, None, *args, local_logits=L.cpu())
        with pytest.raises(ValueError, match="frames_embed=None"):
            m.forward_ragged_multi_guide(ff, fe, *args, local_logits=L)
        with pytest.raises(ValueError, match=r"local_logits is \[max Q_i, sum T_i, H, W\]"):
            m.forward_ragged_multi_guide(ff, None, *args, local_logits=L[:, :-1])
    assert STORE not in m.__dict__ or not m.__dict__[STORE], "a refused call built a plan"


def test_scores_end_to_end_against_the_fp64_head_with_the_multi_form_as_yardstick():
    from hicom_amd import siglip_head_scores_multi, siglip_head_scores_ragged
    splits, counts = (1, 4, 1), (1, 3, 5)
    m = SmallHead().to(torch.bfloat16).to(DEV).eval()
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(sum(splits), 6, 6, D, generator=gen).bfloat16().to(DEV)
    guides = torch.randn(sum(counts), D, generator=gen).bfloat16().to(DEV)
    with torch.no_grad():
        got = siglip_head_scores_ragged(x, m, guides, splits, counts)
        again = siglip_head_scores_ragged(x, m, guides, splits, counts)           # (the tables come from the cache)
        t = p = 0
        multi = []
        for T, Q in zip(splits, counts):
            multi.append(siglip_head_scores_multi(x[t:t + T], m, guides[p:p + Q]))
            t, p = t + T, p + Q
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (max(counts), sum(splits), 6, 6)
    embed = head_fp64(x, m)
    t = p = 0
    for i, (T, Q) in enumerate(zip(splits, counts)):
        want = torch.einsum("thwd,qd->qthw", embed[t:t + T], up(guides[p:p + Q].cpu()))
        new = got[:Q, t:t + T]
        assert bool(torch.isfinite(new).all()) and torch.equal(new, again[:Q, t:t + T])
        e_new = (new.double().cpu() - want).abs().amax((1, 2, 3))
        e_old = (multi[i].double().cpu() - want).abs().amax((1, 2, 3))
        print(f"RAGGED_HEAD_SCORES end-to-end item {i} (T={T} Q={Q}): max-abs per pair new {[f'{float(e):.3e}' for e in e_new]} "
              f"siglip_head_scores_multi {[f'{float(e):.3e}' for e in e_old]}")
        assert bool((e_new <= 2 * e_old).all()), (i, e_new.tolist(), e_old.tolist())
        t, p = t + T, p + Q
