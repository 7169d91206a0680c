"""HIComProjector.forward_ragged_multi_guide_train (GPU): the training step of a mixed batch with Q_i guides per item in one forward call and
one backward over all M = sum Q_i pairs (hicom_amd/ragged_multi_guide_train.py, csrc/ragged_multi_guide_train.hip) against fp64 autograd
through the oracle, per pair, summed (tests/ragged_multi_guide_train_inputs.py has the cases, the cotangents and the yardstick; the bar is
ragged_train_inputs.bars: tests/test_gpu_backward.py's rule on the fp32 gradients).  Every gradient test prints, per parameter, the error of
the new path, the error of forward_ragged_train on tokens replicated Q_i times (what the step replaces) and the bar.

MIX6 (grid 6 x 6, splits (1, 4, 1, 8, 1), counts (1, 3, 5, 2, 4)): Q = 1 leaves row group 1 without a live row, Q = 2 gives it two, Q = 3
straddles the groups with a guide's 9 rows, Q = 4 and 5 open a second pass with 4 and 13 live rows; 36-token items end in a masked tail
tile.  MIX9 (9 x 9, splits (1, 4), counts (4, 8)): 81 tokens, Q = 8 is three passes, the last part-filled.  Chunk overrides 1, 3, 18.

The single-guide degenerate (every Q_i = 1) is held BIT-EQUAL to forward_ragged_train: a row's result does not depend on the number of row
groups, the chunk arithmetic is ragged.item_chunks and the summation orders are the same.

Logits form: (a) scores from siglip_head_scores_ragged under no_grad, the yardstick being the oracle run in fp64 with a frames_embed whose
dot products with the item's guides ARE those scores (the dual basis of the guides, exact in fp64): the bar of the keyed cases; (b) exact
scores fe . g beside the keyed step on the same inputs: the forwards' global rows are bit-equal, so the fp32 gradients of every
global_compressor parameter are asserted bit-equal; the local readout's follow the local rows (<= 2e-3 apart) and are held to the bar.

Measured on an MI355X: the worst parameter of every case is local_compressor.readout.0.weight, 0.12 .. 0.40 of its bar (3.8e-2 of 9.7e-2
under rmg_mix9_scales, 1.8e-1 of 4.6e-1 under rmg_mix6_outlier, 2.1e-3 of 1.4e-2 under rmg_mix6); every global_compressor gradient is
under 3e-4 of its bar (k_proj.bias 8.5e-8 of 9.7e-4); forward_ragged_train on replicated tokens prints the same errors to four digits.
Head scores: readout.0.weight 1.4e-3 of a bar of 8.1e-3.  Exact scores against the keyed step: 2.059e-3 against 2.070e-3."""
import numpy as np
import pytest
import torch

import ragged_multi_guide_inputs as ri
import ragged_multi_guide_train_inputs as rmt
import ragged_train_inputs as rt
from gpu_util import DEV, build_module, dev_bf16
from hicom_amd import autograd as hag
from hicom_amd import native as nv
from ops_reference import up

pytestmark = pytest.mark.gpu
STORE = "_ragged_multi_guide_plans"


def inputs_of(c):
    fe = dev_bf16(np.concatenate(c.fe)) if c.entry.with_fe else None
    return dev_bf16(np.concatenate(c.ff)), fe, dev_bf16(np.concatenate(c.g)), list(c.splits), list(c.counts), list(c.modals)


def pair_cots(id, outs):
    """The cotangents of the call's outputs [Q_i, rows_i, hidden] per item: pair k's is rmt.cotangent(id, k, ...)."""
    cots, k = [], 0
    for o in outs:
        cots.append(torch.stack([torch.from_numpy(rmt.cotangent(id, k + q, tuple(o.shape[1:]))) for q in range(o.shape[0])]).to(DEV))
        k += o.shape[0]
    return cots


def train_step(m, inp, id, nl=None, **kw):
    """One step of the new path: (outputs, fp32 gradients, {name: .grad}) with the gradients of `m` cleared in front."""
    m.zero_grad(set_to_none=True)
    if isinstance(nl, torch.nn.Parameter):
        nl.grad = None
    ff, fe, g, splits, counts, modals = inp
    outs = m.forward_ragged_multi_guide_train(ff, fe, g, splits, counts, modals, nl, **kw)
    assert isinstance(outs, list) and all(o.requires_grad for o in outs)
    sum((o * r).sum() for o, r in zip(outs, pair_cots(id, outs))).backward()
    torch.cuda.synchronize()
    return [o.detach() for o in outs], dict(hag.LAST_FP32_GRADS), {n: p.grad for n, p in m.named_parameters()}


def replicated_step(m, c, id, nl=None, **kw):
    """What the step replaces: forward_ragged_train on every item's tokens replicated Q_i times; returns its fp32 gradients."""
    rep = lambda per: dev_bf16(np.concatenate([per[i] for i, _ in c.pairs]))
    m.zero_grad(set_to_none=True)
    outs = m.forward_ragged_train(rep(c.ff), rep(c.fe) if c.entry.with_fe else None, dev_bf16(np.concatenate(c.g)), [c.splits[i] for i, _ in c.pairs],
                                  [c.modals[i] for i, _ in c.pairs], nl, **kw)
    sum((o * torch.from_numpy(rmt.cotangent(id, k, tuple(o.shape))).to(DEV)).sum() for k, o in enumerate(outs)).backward()
    torch.cuda.synchronize()
    return dict(hag.LAST_FP32_GRADS)


def check_gradients(what, m, fp32, want, other=None, extra=()):
    bar, err = rt.bars(want), rt.errors(fp32, want)
    oerr = rt.errors(other, want) if other is not None else {}
    bad = []
    for k in sorted(bar):
        print(f"{what} {k}: new {err[k]:.3e}  replicated {oerr.get(k, float('nan')):.3e}  bar {bar[k]:.3e}")
        if not err[k] <= bar[k]:
            bad.append(f"{k}: {err[k]:.3e} > {bar[k]:.3e}")
    for n, p in list(m.named_parameters()) + list(extra):
        if want.get(n) is None:
            assert p.grad is None, f"{n}: the reference has no gradient"
        else:
            assert p.grad is not None and p.grad.dtype == p.dtype and p.grad.shape == p.shape, n
            assert float((p.grad.float() - fp32[n].reshape(p.shape)).abs().max()) <= 2 ** -7 * float(np.abs(want[n]).max()) + bar[n], n
    assert not bad, f"{what}: " + "; ".join(bad)


# ---- 1: the step against fp64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", rmt.CASES)
def test_parameter_gradients_against_fp64_oracle_autograd_per_pair(id):
    """Bit-equal outputs to forward_ragged_multi_guide, then every parameter gradient within the bar; forward_ragged_train on replicated
    tokens runs beside it."""
    c = ri.build(id)
    m = build_module(c).train()
    inp = inputs_of(c)
    kw = {"chunks": c.entry.chunks} if c.entry.chunks else {}
    with torch.no_grad():
        ref = m.forward_ragged_multi_guide(*inp, **kw)
    outs, fp32, grads = train_step(m, inp, id, **kw)
    assert len(outs) == len(ref) == c.B and all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(outs, ref))
    keep = {n: p.grad for n, p in m.named_parameters()}
    other = replicated_step(m, c, id, **kw)
    for n, p in m.named_parameters():
        p.grad = keep[n]
    check_gradients(id, m, fp32, rmt.yardstick(id), other)


# ---- 2: image_newline -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", rmt.NEWLINE_CASES)
def test_newline_parameter_gradient(id):
    c = ri.build(id)
    m = build_module(c).train()
    nl = torch.nn.Parameter(dev_bf16(c.newline))
    inp = inputs_of(c)
    with torch.no_grad():
        ref = m.forward_ragged_multi_guide(*inp, nl)
    outs, fp32, grads = train_step(m, inp, id, nl)
    assert all(torch.equal(a, b) for a, b in zip(outs, ref))
    want = rmt.yardstick(id)
    assert "image_newline" in fp32 and want["image_newline"] is not None and np.abs(want["image_newline"]).max() > 0
    check_gradients(id, m, fp32, want, extra=[("image_newline", nl)])


# ---- 3: every Q_i = 1 is forward_ragged_train, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("chunks", [None, 3])
def test_single_guides_leave_forward_ragged_trains_gradients_bit_for_bit(chunks):
    id = "rmg_mix6"
    c = ri.build(id)
    m = build_module(c).train()
    ff, fe, _, splits, _, modals = inputs_of(c)
    g = dev_bf16(np.concatenate([gi[:1] for gi in c.g]))
    kw = {} if chunks is None else {"chunks": chunks}
    outs, fp32, _ = train_step(m, (ff, fe, g, splits, [1] * c.B, modals), id, **kw)
    m.zero_grad(set_to_none=True)
    rag = m.forward_ragged_train(ff, fe, g, splits, modals, **kw)
    sum((o * torch.from_numpy(rmt.cotangent(id, k, tuple(o.shape))).to(DEV)).sum() for k, o in enumerate(rag)).backward()
    torch.cuda.synchronize()
    single = dict(hag.LAST_FP32_GRADS)
    assert all(torch.equal(a[0], b) for a, b in zip(outs, rag))
    assert fp32.keys() == single.keys() and len(fp32) > 8
    diff = {k: float((fp32[k] - single[k]).abs().max()) for k in fp32 if not torch.equal(fp32[k], single[k])}
    assert not diff, f"chunks={chunks}: not bit-equal to forward_ragged_train: {diff}"


# ---- 4: the logits form -----------------------------------------------------------------------------------------------------------------
def dual_basis_embed(c, L):
    """Per item, float64 [T, H, W, D]: the frames_embed of least norm whose dot products with the item's guides are the scores L[:Q_i]."""
    out, t = [], 0
    for T, Q, g in zip(c.splits, c.counts, c.g):
        G = up(torch.from_numpy(g).bfloat16())                                      # [Q, D], the values the GPU reads
        l = L[:Q, t:t + T].double().cpu().reshape(Q, -1)                            # [Q, N]
        fe = (torch.linalg.solve(G @ G.t(), l).t() @ G).reshape(T, c.h, c.w, -1)
        assert float((torch.einsum("thwd,qd->qthw", fe, G) - L[:Q, t:t + T].double().cpu()).abs().max()) < 1e-9
        out.append(fe.numpy())
        t += T
    return out


def test_logits_form_with_head_scores_against_fp64_for_the_scores_own_values():
    from hicom_amd import siglip_head_scores_ragged
    from test_gpu_head_scores import SmallHead
    id = "rmg_mix6"
    c = ri.build(id)
    m = build_module(c).train()
    ff, _, g, splits, counts, modals = inputs_of(c)
    head = SmallHead().to(torch.bfloat16).to(DEV).eval()
    with torch.no_grad():
        L = siglip_head_scores_ragged(ff, head, g, splits, counts)
        ref = m.forward_ragged_multi_guide(ff, None, g, splits, counts, modals, local_logits=L)
    assert not L.requires_grad and tuple(L.shape) == (max(counts), sum(splits), c.h, c.w)
    outs, fp32, grads = train_step(m, (ff, None, g, splits, counts, modals), id, local_logits=L)
    assert all(torch.equal(a, b) for a, b in zip(outs, ref))
    assert sum(k[-1] == "logits" for k in m.__dict__[STORE]) == 1 and len(m.__dict__[STORE]) == 1
    fe64 = dual_basis_embed(c, L)
    want = rt.oracle_grads(c.cfg, c.sd, [(c.ff[i], fe64[i], c.g[i][q], c.modals[i]) for i, q in c.pairs], None,
                           lambda k, shape: rmt.cotangent(id, k, shape))
    check_gradients(f"{id} head scores", m, fp32, want)


def test_logits_form_with_exact_scores_beside_the_keyed_step():
    """Global rows of the two forwards are bit-equal, so the global stage's fp32 gradients are: asserted.  The local readout's gradients
    follow the local rows: both inside the bar of the keyed yardstick."""
    id = "rmg_mix6"
    c = ri.build(id)
    m = build_module(c).train()
    inp = inputs_of(c)
    ff, fe, g, splits, counts, modals = inp
    L = torch.full((max(counts), sum(splits), c.h, c.w), float("nan"), dtype=torch.float32)
    t = 0
    for e, gi, T, Q in zip(c.fe, c.g, c.splits, c.counts):
        L[:Q, t:t + T] = torch.einsum("thwd,qd->qthw", up(torch.from_numpy(e).bfloat16()), up(torch.from_numpy(gi).bfloat16())).float()
        t += T
    k_out, k32, _ = train_step(m, inp, id)
    l_out, l32, _ = train_step(m, (ff, None, g, splits, counts, modals), id, local_logits=L.to(DEV))
    ng = ri.NG
    assert all(torch.equal(a[:, -ng:], b[:, -ng:]) for a, b in zip(k_out, l_out))
    assert k32.keys() == l32.keys()
    for n in k32:
        if n.startswith("global_compressor."):
            assert torch.equal(k32[n], l32[n]), f"{n}: the global stage's gradient differs from the keyed step's"
    check_gradients(f"{id} exact scores", m, l32, rmt.yardstick(id), k32)


# ---- 5: behaviour ------------------------------------------------------------------------------------------------------------------------
def test_forward_forward_backward_backward_on_one_plan():
    """forward A, forward B (same plan, other data), backward B, backward A equal A and B run alone, bit for bit."""
    ida, idb = "rmg_mix6", "rmg_mix6_outlier"
    m = build_module(ri.build(ida)).train()
    alone = {}
    for id in (ida, idb):
        _, _, grads = train_step(m, inputs_of(ri.build(id)), id)
        alone[id] = {n: g.clone() for n, g in grads.items() if g is not None}
    m.zero_grad(set_to_none=True)
    outs = {id: m.forward_ragged_multi_guide_train(*inputs_of(ri.build(id))) for id in (ida, idb)}
    assert len(m.__dict__[STORE]) == 1
    for id in (idb, ida):
        sum((o * r).sum() for o, r in zip(outs[id], pair_cots(id, outs[id]))).backward()
        got = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
        assert got.keys() == alone[id].keys() and len(got) > 8
        for n in got:
            assert torch.equal(got[n], alone[id][n]), f"{id}: {n}"
        m.zero_grad(set_to_none=True)
    assert any(not torch.equal(alone[ida][n], alone[idb][n]) for n in alone[ida])


class Spy:
    """Wraps a function of hicom_amd.native / hicom_amd.autograd: counts the calls `only` accepts (all of them by default)."""

    def __init__(self, monkeypatch, mod, name, only=lambda *a, **k: True):
        self.calls, real = 0, getattr(mod, name)

        def wrapped(*a, **k):
            self.calls += bool(only(*a, **k))
            return real(*a, **k)
        monkeypatch.setattr(mod, name, wrapped)


def test_a_stage_without_trainable_parameters_is_skipped(monkeypatch):
    id = "rmg_mix9"
    c = ri.build(id)
    want = rmt.yardstick(id)
    bar = rt.bars(want)
    for stage, other in (("local_compressor.", "global_compressor."), ("global_compressor.", "local_compressor.")):
        native_spy, readout_spy = Spy(monkeypatch, nv, "compressor_ragged_multiguide_global_bwd"), Spy(monkeypatch, hag, "_readout_backward",
                                                                                                             only=lambda *a, **k: "local_compressor.readout." in a)
        m = build_module(c).train()
        for n, p in m.named_parameters():
            p.requires_grad_(n.startswith(stage))
        _, fp32, grads = train_step(m, inputs_of(c), id)
        if stage == "local_compressor.":
            assert native_spy.calls == 0 and readout_spy.calls == 1
        else:
            assert native_spy.calls == 1 and readout_spy.calls == 0
        err = rt.errors(fp32, {k: v for k, v in want.items() if k.startswith(stage)})
        assert len(err) >= 4 and all(err[k] <= bar[k] for k in err), (err, bar)
        for n, gr in grads.items():
            assert (gr is not None) == (n.startswith(stage) and want.get(n) is not None), n       # (global_compressor.query: unused under "direct")
        monkeypatch.undo()


def test_grad_disabled_or_nothing_trainable_is_the_inference_call():
    c = ri.build("rmg_mix9")
    m = build_module(c).train()
    inp = inputs_of(c)
    with torch.no_grad():
        ref = m.forward_ragged_multi_guide(*inp)
        outs = m.forward_ragged_multi_guide_train(*inp)
    assert all(not o.requires_grad and o.grad_fn is None and torch.equal(o, r) for o, r in zip(outs, ref))
    m.requires_grad_(False)
    assert torch.is_grad_enabled()
    outs = m.forward_ragged_multi_guide_train(*inp)
    assert all(not o.requires_grad and o.grad_fn is None and torch.equal(o, r) for o, r in zip(outs, ref))
    assert len(m.__dict__[STORE]) == 1


def test_refusals_on_device_tensors_leave_no_plan():
    c = ri.build("rmg_mix9")
    ff, fe, g, splits, counts, modals = inputs_of(c)
    m = build_module(c).train()
    for over in ({"ff": ff.clone().requires_grad_(True)}, {"fe": fe.clone().requires_grad_(True)}, {"g": g.clone().requires_grad_(True)},
                 {"ff": ff.half()}, {"g": g.float()}):
        with pytest.raises(NotImplementedError, match=r"forward\(\)"):
            m.forward_ragged_multi_guide_train(over.get("ff", ff), over.get("fe", fe), over.get("g", g), splits, counts, modals)
    L = torch.zeros((max(counts), sum(splits), c.h, c.w), device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError, match=r"local_logits.*forward\(\)"):
        m.forward_ragged_multi_guide_train(ff, None, g, splits, counts, modals, local_logits=L)
    with pytest.raises(ValueError, match="frames_embed=None"):
        m.forward_ragged_multi_guide_train(ff, fe, g, splits, counts, modals, local_logits=L.detach())
    with pytest.raises(ValueError, match="guide_counts"):
        m.forward_ragged_multi_guide_train(ff, fe, g, splits, [33] + counts[1:], modals)
    assert not m.__dict__.get(STORE), "a refused call built a plan"
