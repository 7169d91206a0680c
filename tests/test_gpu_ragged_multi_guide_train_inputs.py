"""HIComProjector.forward_ragged_multi_guide_train(input_grads=True) (GPU): the stage-3 input gradients of a mixed batch with Q_i guides per
item -- d frames_feature, d frames_embed, d guide_embeds -- from one forward call and one backward over all M = sum Q_i pairs
(hicom_amd/ragged_multi_guide_train.py, csrc/ragged_multi_guide_train.hip: rmg_local_bwd_kernel, rmg_dq_pair_kernel, rmg_global_dx_kernel).

Cases: the small cases of tests/ragged_multi_guide_inputs.py (MIX6: counts (1, 3, 5, 2, 4), remainder groups of 1, 2 and 3 and an item
across the group of four and the 32-row pass; MIX9: counts (4, 8), a tail tile, three passes with the last part-filled).
Reference: fp64 autograd through the oracle per pair (ragged_train_input_grads.oracle_grads on ragged_multi_guide_train_inputs.pair_items,
the cotangents of tests/ragged_multi_guide_train_inputs.py); the per-pair d frames_feature / d frames_embed are summed in fp64 over the pairs
of an item.  Bars, the project's own: ragged_train_input_grads.item_bar and its sum bar on each item's summed reference, guide_bar on the
fp32 d guide, ragged_train_inputs.bars on the parameters.  Every gradient test prints the error of forward_ragged_train(input_grads=True) on
tokens replicated Q_i times (the replicas' bf16 gradients summed in fp32: what the step replaces) beside the new path's.
Every test here fails without the feature: the keyword does not exist there.
Measured on an MI355X: both paths are inside the bars on every case.  Worst of the new path: d frames_feature 7.60e-4 of a bar of 1.56e-3
(rmg_mix6_no_fe item 2; replicated 4.85e-4), d frames_embed 9.50e-4 of 2.68e-3 (rmg_mix6_outlier item 4; replicated 6.18e-4), d guide_embeds
in fp32 3.606e-4 of 3.21e-3 (rmg_mix9_scales), equal to the replicated path's to every printed digit on every case; the per-item sums at
most 0.3 % of their bars.  DESIGN.md §3.27 has the table."""
import functools

import numpy as np
import pytest
import torch

import ragged_multi_guide_inputs as ri
import ragged_multi_guide_train_inputs as rmt
import ragged_train_input_grads as ig
import ragged_train_inputs as rt
from gpu_util import DEV, build_module, dev_bf16
from hicom_amd import autograd as hag
from hicom_amd import native as nv

pytestmark = pytest.mark.gpu

CASES = ["rmg_mix6", "rmg_mix6_chunks3", "rmg_mix6_chunks18", "rmg_mix9", "rmg_mix9_chunks3", "rmg_mix6_no_fe", "rmg_mix6_outlier", "rmg_mix9_scales"]


@functools.lru_cache(maxsize=None)
def yardstick(id):
    """(parameter references, {"frames_feature": [per item], "frames_embed": [per item] or None, "guide_embeds": [M, E]}): the per-pair
    token gradients summed in fp64 over the pairs of an item.  Computed once per process; callers must not write into it."""
    c = ri.build(id)
    params, per_pair = ig.oracle_grads(c.cfg, c.sd, rmt.pair_items(c), lambda k, shape: rmt.cotangent(id, k, shape), c.entry.with_fe)

    def per_item(name):
        if per_pair[name] is None:
            return None
        out = [None] * c.B
        for (i, _), g in zip(c.pairs, per_pair[name]):
            out[i] = g.copy() if out[i] is None else out[i] + g
        return out
    return params, {"frames_feature": per_item("frames_feature"), "frames_embed": per_item("frames_embed"), "guide_embeds": per_pair["guide_embeds"]}


def leaves(c, need=(True, True, True), single=False):
    """(ff, fe, g, splits, counts, modals) as device bf16 leaves; single: every item with its first guide only."""
    fe = dev_bf16(np.concatenate(c.fe)).requires_grad_(need[1]) if c.entry.with_fe else None
    g = np.concatenate([gi[:1] for gi in c.g]) if single else np.concatenate(c.g)
    counts = [1] * c.B if single else list(c.counts)
    return dev_bf16(np.concatenate(c.ff)).requires_grad_(need[0]), fe, dev_bf16(g).requires_grad_(need[2]), list(c.splits), counts, list(c.modals)


def pair_cots(id, outs):
    cots, k = [], 0
    for o in outs:
        cots.append(torch.stack([torch.from_numpy(rmt.cotangent(id, k + q, tuple(o.shape[1:]))) for q in range(o.shape[0])]).to(DEV))
        k += o.shape[0]
    return cots


def step(m, inp, id, **kw):
    """One step of the new path: (outputs, fp32 gradients, parameter .grad, (d ff, d fe, d guide))."""
    m.zero_grad(set_to_none=True)
    ff, fe, g, splits, counts, modals = inp
    for t in (ff, fe, g):
        if t is not None:
            t.grad = None
    outs = m.forward_ragged_multi_guide_train(ff, fe, g, splits, counts, modals, **kw)
    sum((o * r).sum() for o, r in zip(outs, pair_cots(id, outs))).backward()
    torch.cuda.synchronize()
    return ([o.detach() for o in outs], dict(hag.LAST_FP32_GRADS), {n: p.grad for n, p in m.named_parameters()},
            tuple(None if t is None else t.grad for t in (ff, fe, g)))


def replicated_step(m, c, id, **kw):
    """What the step replaces: forward_ragged_train(input_grads=True) on every item's tokens replicated Q_i times, the replicas' bf16
    gradients summed in fp32 per item: (d ff [sum T_i, ...] fp32, d fe or None, d guide fp32 [M, E])."""
    rep = lambda per: dev_bf16(np.concatenate([per[i] for i, _ in c.pairs])).requires_grad_(True)
    m.zero_grad(set_to_none=True)
    ff, fe, g = rep(c.ff), (rep(c.fe) if c.entry.with_fe else None), dev_bf16(np.concatenate(c.g)).requires_grad_(True)
    outs = m.forward_ragged_train(ff, fe, g, [c.splits[i] for i, _ in c.pairs], [c.modals[i] for i, _ in c.pairs], input_grads=True, **kw)
    sum((o * torch.from_numpy(rmt.cotangent(id, k, tuple(o.shape))).to(DEV)).sum() for k, o in enumerate(outs)).backward()
    torch.cuda.synchronize()

    def fold(t):
        if t is None:
            return None
        parts, t0, out = [], 0, [None] * c.B
        for i, _ in c.pairs:
            piece = t.grad[t0:t0 + c.splits[i]].float()
            out[i] = piece if out[i] is None else out[i] + piece
            t0 += c.splits[i]
        return torch.cat(out)
    return fold(ff), fold(fe), hag.LAST_FP32_GRADS["__guide_embeds__"].clone()


def check_inputs(what, inp, got, fp32, want_params, want_in, other=None):
    """Asserts dtype / shape and the bars of the three input gradients; prints the replicated path's figures beside the new path's."""
    ff, fe, g, splits, _, _ = inp
    d_ff, d_fe, d_g = got
    bad = []
    for name, t, d, op in (("frames_feature", ff, d_ff, other and other[0]), ("frames_embed", fe, d_fe, other and other[1])):
        if t is None:
            continue
        assert d is not None and d.dtype == t.dtype and d.shape == t.shape, name
        errs = ig.item_errors(d, want_in[name], splits)
        oerrs = ig.item_errors(op, want_in[name], splits) if op is not None else [(float("nan"),) * 4] * len(errs)
        for i, ((e, bar, se, sbar), (oe, _, ose, _)) in enumerate(zip(errs, oerrs)):
            print(f"{what} d {name} item {i}: new {e:.3e}  replicated {oe:.3e}  bar {bar:.3e};  sum: new {se:.3e}  replicated {ose:.3e}  bar {sbar:.3e}")
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
    oe = float((other[2].double().cpu() - torch.from_numpy(wg)).abs().max()) if other is not None else float("nan")
    print(f"{what} d guide_embeds: new {e:.3e}  replicated {oe:.3e}  bar {bar:.3e}")
    if not e <= bar:
        bad.append(f"d guide_embeds: {e:.3e} > {bar:.3e}")
    assert not bad, f"{what}: " + "; ".join(bad)


def check_params(what, fp32, want):
    bar, err = rt.bars(want), rt.errors(fp32, want)
    bad = [f"{k}: {err[k]:.3e} > {bar[k]:.3e}" for k in sorted(bar) if not err[k] <= bar[k]]
    assert not bad, f"{what}: " + "; ".join(bad)


@pytest.mark.parametrize("id", CASES)
def test_input_gradients_against_fp64_oracle_autograd_per_pair(id):
    """Outputs bit-equal to forward_ragged_multi_guide; the three input gradients and every parameter gradient within their bars; the
    parameter gradients bit-equal to those of the same step with the inputs detached."""
    c = ri.build(id)
    m = build_module(c).train()
    kw = {"chunks": c.entry.chunks} if c.entry.chunks else {}
    inp = leaves(c)
    with torch.no_grad():
        ref = m.forward_ragged_multi_guide(*(t.detach() if torch.is_tensor(t) else t for t in inp), **kw)
    outs, fp32, grads, got = step(m, inp, id, input_grads=True, **kw)
    assert len(outs) == len(ref) and all(torch.equal(a, b) for a, b in zip(outs, ref))
    keep = {n: v.clone() for n, v in grads.items() if v is not None}
    want_params, want_in = yardstick(id)
    other = replicated_step(m, c, id, **kw)
    check_inputs(id, inp, got, fp32, want_params, want_in, other)
    check_params(id, fp32, want_params)
    _, _, detached, none = step(m, leaves(c, need=(False, False, False)), id, **kw)
    assert all(t is None for t in none)
    assert keep.keys() == {n for n, v in detached.items() if v is not None}
    for n in keep:
        assert torch.equal(keep[n], detached[n]), f"{n}: moved with input_grads=True"


class Spy:
    """Counts the calls of the native backward wrappers."""
    NAMES = ("compressor_ragged_multiguide_global_bwd", "compressor_ragged_multiguide_global_dx", "compressor_ragged_multiguide_local_bwd",
             "compressor_ragged_multiguide_dq_pair")

    def __init__(self, monkeypatch):
        self.calls = {}
        for name in self.NAMES:
            self.calls[name] = 0
            monkeypatch.setattr(nv, name, self.wrap(name, getattr(nv, name)))

    def wrap(self, name, real):
        def wrapped(*a, **k):
            self.calls[name] += 1
            return real(*a, **k)
        return wrapped

    def counts(self):
        return tuple(self.calls[n] for n in self.NAMES)


@pytest.mark.parametrize("id", ["rmg_mix6", "rmg_mix6_no_fe"])
def test_one_input_at_a_time_with_every_parameter_frozen_is_the_all_three_run_bit_for_bit(id, monkeypatch):
    """A frozen module with an input requiring grad is trainable; an input that does not require grad costs no launch of its own."""
    c = ri.build(id)
    m = build_module(c).train().requires_grad_(False)
    _, fp_all, grads, all3 = step(m, leaves(c), id, input_grads=True)
    assert all(v is None for v in grads.values())
    all3, g32 = [None if t is None else t.clone() for t in all3], fp_all["__guide_embeds__"].clone()
    with_fe = c.entry.with_fe
    #                      need                    (global_bwd, global_dx, local_bwd, dq_pair)
    for k, (need, calls) in enumerate((((True, False, False), (1, 1, 1, 0)), ((False, True, False), (0, 0, 1, 0)), ((False, False, True), (1, 0, 1, 1)))):
        if k == 1 and not with_fe:
            continue
        spy = Spy(monkeypatch)
        _, fp32, _, got = step(m, leaves(c, need=need), id, input_grads=True)
        assert spy.counts() == calls, (need, spy.calls)
        monkeypatch.undo()
        for j, (t, w) in enumerate(zip(got, all3)):
            if j == k:
                assert t is not None and torch.equal(t, w), f"{ig.INPUTS[j]} alone differs from the all-three run"
            else:
                assert t is None, f"{ig.INPUTS[j]} got a gradient it did not ask for"
        assert ("__guide_embeds__" in fp32) == (k == 2) and (k != 2 or torch.equal(fp32["__guide_embeds__"], g32))
    with pytest.raises(NotImplementedError, match=r"frames_feature.*forward\(\)"):
        m.forward_ragged_multi_guide_train(*leaves(c))              # the default keeps the refusals


@pytest.mark.parametrize("chunks", [None, 3])
def test_single_guides_leave_forward_ragged_trains_input_gradients_bit_for_bit(chunks):
    id = "rmg_mix6"
    c = ri.build(id)
    m = build_module(c).train()
    kw = {} if chunks is None else {"chunks": chunks}
    inp = leaves(c, single=True)
    outs, fp32, _, got = step(m, inp, id, input_grads=True, **kw)
    ff, fe, g, splits, _, modals = leaves(c, single=True)
    m.zero_grad(set_to_none=True)
    rag = m.forward_ragged_train(ff, fe, g, splits, modals, input_grads=True, **kw)
    sum((o * torch.from_numpy(rmt.cotangent(id, k, tuple(o.shape))).to(DEV)).sum() for k, o in enumerate(rag)).backward()
    torch.cuda.synchronize()
    assert all(torch.equal(a[0], b) for a, b in zip(outs, rag))
    assert torch.equal(got[0], ff.grad), "d frames_feature"
    assert torch.equal(got[1], fe.grad), "d frames_embed"
    assert torch.equal(fp32["__guide_embeds__"], hag.LAST_FP32_GRADS["__guide_embeds__"]), "d guide_embeds (fp32)"


def test_frames_embed_is_kept_only_where_the_window_backward_runs():
    id = "rmg_mix6"
    c = ri.build(id)
    m = build_module(c).train()
    for need, kept in (((False, False, False), False), ((False, False, True), True)):
        ff, fe, g, splits, counts, modals = leaves(c, need=need)
        outs = m.forward_ragged_multi_guide_train(ff, fe, g, splits, counts, modals, input_grads=True)
        saved = outs[0].grad_fn
        while saved is not None and "RaggedMultiGuideTrainFn" not in type(saved).__name__:     # (through the views of the output)
            saved = saved.next_functions[0][0]
        assert (saved.saved_tensors[6] is not None) == kept
        assert not kept or saved.saved_tensors[6].data_ptr() == fe.data_ptr()       # by reference
