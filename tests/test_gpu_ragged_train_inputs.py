"""HIComProjector.forward_ragged_train(input_grads=True) (GPU): the stage-3 input gradients of a mixed batch -- d frames_feature,
d frames_embed, d guide_embeds -- from one forward call and one backward over all items (hicom_amd/ragged_train.py, csrc/ragged_train.hip:
ragged_local_attn_bwd_kernel, ragged_dq_item_kernel, ragged_global_dx_kernel) against fp64 autograd through the oracle per item
(tests/ragged_train_input_grads.py has the yardstick and the bars).  Every gradient test prints the error of the new path and of the loop
of forward() + backward per item with the same inputs requiring grad, the code the step replaces.  Every test here fails without the
feature: the keyword does not exist there.
Measured on an MI355X: both paths are inside the bars on every case, and the bf16 input gradients of the new path have the loop's error to
every printed digit (d frames_feature at worst 2.26e-4 of a bar of 4.15e-4, batch_T8_chunks18 item 0; d frames_embed 4.79e-4 of 1.30e-3,
batch_image_81_outlier item 1; d guide_embeds in fp32 4.548e-3 against the loop's 4.554e-3, bar 2.12e-2, batch_image_81_outlier; the
per-item sums at most 0.2 % of their bars)."""
import pytest
import torch

import many_item_inputs as mi
import ragged_train_input_grads as ig
import ragged_train_inputs as rt
from gpu_util import build_module, dev_bf16
from hicom_amd import autograd as hag
from hicom_amd import native as nv

pytestmark = pytest.mark.gpu

NO_FE = ("ragged_mix6", "batch_image_81")           # the frames_embed=None form: a mixed 6 x 6 batch and a 9 x 9 image batch


def leaves(id, with_fe=True, need=(True, True, True)):
    ff, fe, g, splits, modals = rt.stacked(mi.build(id))
    ff, fe, g = dev_bf16(ff).requires_grad_(need[0]), (dev_bf16(fe).requires_grad_(need[1]) if with_fe else None), dev_bf16(g).requires_grad_(need[2])
    return ff, fe, g, splits, modals


def cot_list(id, outs):
    return [torch.from_numpy(rt.cotangent(id, i, tuple(o.shape))).cuda() for i, o in enumerate(outs)]


def step(m, inp, id, **kw):
    """One step of the new path: (outputs, fp32 gradients, parameter .grad, (d ff, d fe, d guide))."""
    m.zero_grad(set_to_none=True)
    ff, fe, g, splits, modals = inp
    for t in (ff, fe, g):
        if t is not None:
            t.grad = None
    outs = m.forward_ragged_train(ff, fe, g, splits, modals, **kw)
    sum((o * r).sum() for o, r in zip(outs, cot_list(id, outs))).backward()
    torch.cuda.synchronize()
    return ([o.detach() for o in outs], dict(hag.LAST_FP32_GRADS), {n: p.grad for n, p in m.named_parameters()},
            tuple(None if t is None else t.grad for t in (ff, fe, g)))


def loop_step(m, inp, id):
    """The loop the step replaces, the same inputs requiring grad: (d ff, d fe, d guide fp32 [B, E])."""
    ff, fe, g, splits, modals = inp
    for t in (ff, fe, g):
        if t is not None:
            t.grad = None
    m.zero_grad(set_to_none=True)
    t0, dg = 0, []
    for i, (T, modal) in enumerate(zip(splits, modals)):
        out = m(ff[t0:t0 + T], None if fe is None else fe[t0:t0 + T], g[i], modal, None)
        (out * torch.from_numpy(rt.cotangent(id, i, tuple(out.shape))).cuda()).sum().backward()
        dg.append(hag.LAST_FP32_GRADS["__guide_embed__"].reshape(-1).clone())
        t0 += T
    torch.cuda.synchronize()
    return ff.grad, None if fe is None else fe.grad, torch.stack(dg)


def check_inputs(what, inp, got, fp32, want_params, want_in, loop=None):
    """Asserts dtype / shape and the bars of the three input gradients; prints the loop's figures beside the new path's."""
    ff, fe, g, splits, _ = inp
    d_ff, d_fe, d_g = got
    bad = []
    for name, t, d, lp in (("frames_feature", ff, d_ff, loop and loop[0]), ("frames_embed", fe, d_fe, loop and loop[1])):
        if t is None:
            continue
        assert d is not None and d.dtype == t.dtype and d.shape == t.shape, name
        errs = ig.item_errors(d, want_in[name], splits)
        lerrs = ig.item_errors(lp, want_in[name], splits) if lp is not None else [(float("nan"),) * 4] * len(errs)
        for i, ((e, bar, se, sbar), (le, _, lse, _)) in enumerate(zip(errs, lerrs)):
            print(f"{what} d {name} item {i}: new {e:.3e}  loop {le:.3e}  bar {bar:.3e};  sum: new {se:.3e}  loop {lse:.3e}  bar {sbar:.3e}")
            if not e <= bar:
                bad.append(f"d {name} item {i}: {e:.3e} > {bar:.3e}")
            if not se <= sbar:
                bad.append(f"sum d {name} item {i}: {se:.3e} > {sbar:.3e}")
    assert d_g is not None and d_g.dtype == g.dtype and d_g.shape == g.shape
    g32 = fp32["__guide_embeds__"]
    assert g32.dtype == torch.float32 and g32.shape == g.shape and torch.equal(g32.to(g.dtype), d_g)
    wg = want_in["guide_embeds"]
    bar = ig.guide_bar(want_params, wg)
    e = float((g32.double().cpu() - torch.from_numpy(wg)).abs().max())
    le = float((loop[2].double().cpu() - torch.from_numpy(wg)).abs().max()) if loop is not None else float("nan")
    print(f"{what} d guide_embeds: new {e:.3e}  loop {le:.3e}  bar {bar:.3e}")
    if not e <= bar:
        bad.append(f"d guide_embeds: {e:.3e} > {bar:.3e}")
    assert not bad, f"{what}: " + "; ".join(bad)


def check_params(what, fp32, want):
    bar, err = rt.bars(want), rt.errors(fp32, want)
    bad = [f"{k}: {err[k]:.3e} > {bar[k]:.3e}" for k in sorted(bar) if not err[k] <= bar[k]]
    assert not bad, f"{what}: " + "; ".join(bad)


@pytest.mark.parametrize("id", rt.CASES)
def test_input_gradients_against_fp64_oracle_autograd(id):
    """Outputs bit-equal to forward_ragged; the three input gradients and every parameter gradient within their bars; the parameter
    gradients bit-equal to those of the same step with the inputs detached."""
    c = mi.build(id)
    m = build_module(c).train()
    m.graph_backward = False
    kw = {"chunks": c.entry.chunks} if c.entry.chunks else {}
    inp = leaves(id)
    with torch.no_grad():
        ref = m.forward_ragged(*(t.detach() if torch.is_tensor(t) else t for t in inp), **kw)
    outs, fp32, grads, got = step(m, inp, id, input_grads=True, **kw)
    assert len(outs) == len(ref) and all(torch.equal(a, b) for a, b in zip(outs, ref))
    keep = {n: v.clone() for n, v in grads.items() if v is not None}
    want_params, want_in = ig.yardstick(id)
    loop = loop_step(m, inp, id)
    check_inputs(id, inp, got, fp32, want_params, want_in, loop)
    check_params(id, fp32, want_params)
    _, _, detached, none = step(m, leaves(id, need=(False, False, False)), id, **kw)
    assert none == (None, None, None)
    assert keep.keys() == {n for n, v in detached.items() if v is not None}
    for n in keep:
        assert torch.equal(keep[n], detached[n]), f"{n}: moved with input_grads=True"


@pytest.mark.parametrize("id", NO_FE)
def test_without_frames_embed_the_key_side_gradient_lands_in_frames_feature(id):
    c = mi.build(id)
    m = build_module(c).train()
    m.graph_backward = False
    inp = leaves(id, with_fe=False)
    outs, fp32, grads, got = step(m, inp, id, input_grads=True)
    with torch.no_grad():
        ref = m.forward_ragged(inp[0].detach(), None, inp[2].detach(), inp[3], inp[4])
    assert all(torch.equal(a, b) for a, b in zip(outs, ref))
    want_params, want_in = ig.yardstick(id, False)
    check_inputs(f"{id} no_fe", inp, got, fp32, want_params, want_in, loop_step(m, inp, id))
    check_params(f"{id} no_fe", fp32, want_params)


class Spy:
    """Counts the calls of the three native backward wrappers."""

    def __init__(self, monkeypatch):
        self.calls = {}
        for name in ("compressor_ragged_global_bwd", "compressor_ragged_global_dx", "compressor_ragged_local_bwd"):
            self.calls[name] = 0
            monkeypatch.setattr(nv, name, self.wrap(name, getattr(nv, name)))

    def wrap(self, name, real):
        def wrapped(*a, **k):
            self.calls[name] += 1
            return real(*a, **k)
        return wrapped


def test_all_parameters_frozen_with_inputs_trainable(monkeypatch):
    id = "ragged_mix9"
    spy = Spy(monkeypatch)
    m = build_module(mi.build(id)).train().requires_grad_(False)
    inp = leaves(id)
    outs, fp32, grads, got = step(m, inp, id, input_grads=True)
    assert all(v is None for v in grads.values())
    assert spy.calls == {"compressor_ragged_global_bwd": 1, "compressor_ragged_global_dx": 1, "compressor_ragged_local_bwd": 1}
    want_params, want_in = ig.yardstick(id)
    check_inputs(f"{id} frozen", inp, got, fp32, want_params, want_in)
    with pytest.raises(NotImplementedError, match=r"frames_feature.*forward\(\)"):
        m.forward_ragged_train(*inp)                            # the default keeps the refusals


def test_only_frames_embed_requiring_grad_makes_no_global_stage_call(monkeypatch):
    id = "ragged_mix9"
    spy = Spy(monkeypatch)
    m = build_module(mi.build(id)).train().requires_grad_(False)
    inp = leaves(id, need=(False, True, False))
    outs, fp32, grads, (d_ff, d_fe, d_g) = step(m, inp, id, input_grads=True)
    assert spy.calls == {"compressor_ragged_global_bwd": 0, "compressor_ragged_global_dx": 0, "compressor_ragged_local_bwd": 1}
    assert d_ff is None and d_g is None and "__guide_embeds__" not in fp32
    _, want_in = ig.yardstick(id)
    for i, (e, bar, se, sbar) in enumerate(ig.item_errors(d_fe, want_in["frames_embed"], inp[3])):
        assert e <= bar and se <= sbar, (i, e, bar, se, sbar)


def test_two_identical_steps_give_bit_equal_input_gradients():
    id = "ragged_mix6"
    m = build_module(mi.build(id)).train()
    inp = leaves(id)
    _, f1, _, g1 = step(m, inp, id, input_grads=True)
    g1 = [t.clone() for t in g1]
    _, f2, _, g2 = step(m, inp, id, input_grads=True)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2)) and torch.equal(f1["__guide_embeds__"], f2["__guide_embeds__"])


def test_forward_forward_backward_backward_on_one_plan():
    """Forward A, forward B (same plan, other data), backward B, backward A equal A and B run alone, bit for bit."""
    ida, idb = "ragged_mix6", "ragged_mix6_outlier"
    m = build_module(mi.build(ida)).train()
    alone, inps = {}, {id: leaves(id) for id in (ida, idb)}
    for id in (ida, idb):
        _, _, grads, got = step(m, inps[id], id, input_grads=True)
        alone[id] = ({n: g.clone() for n, g in grads.items() if g is not None}, [t.clone() for t in got])
    m.zero_grad(set_to_none=True)
    for id in (ida, idb):
        for t in inps[id][:3]:
            t.grad = None
    outs = {id: m.forward_ragged_train(*inps[id], input_grads=True) for id in (ida, idb)}
    assert len(m.__dict__["_ragged_plans"]) == 1
    for id in (idb, ida):
        sum((o * r).sum() for o, r in zip(outs[id], cot_list(id, outs[id]))).backward()
        for n, p in m.named_parameters():
            assert (p.grad is None) == (n not in alone[id][0]) and (p.grad is None or torch.equal(p.grad, alone[id][0][n])), f"{id}: {n}"
        for t, w in zip(inps[id][:3], alone[id][1]):
            assert torch.equal(t.grad, w), id
        m.zero_grad(set_to_none=True)
