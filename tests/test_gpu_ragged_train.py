"""HIComProjector.forward_ragged_train (GPU): the training step of a mixed batch in one forward call and one backward over all items
(hicom_amd/ragged_train.py, csrc/ragged_train.hip) against fp64 autograd through the oracle, per item, summed (tests/ragged_train_inputs.py
has the cases, the cotangents and the bar: tests/test_gpu_backward.py's rule on the fp32 gradients).  Every gradient test prints, per
parameter, the error of the new path and of the loop of forward() + backward per item, the code the step replaces.
Measured on an MI355X: both paths are inside the bar on every case; the new path's error is 0.8 .. 1.3 x the loop's per parameter
(k_proj.weight: 1.1e-3 against 8.8e-4, bar 1.4e-1, under ragged_mix6_outlier; 1.8e-4 against 2.2e-4, bar 1.8e-2, under ragged_mix9_scales;
d image_newline 3.6e-7 of a bar of 9.0e-3)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import many_item_inputs as mi
import ragged_train_inputs as rt
from gpu_util import build_module, dev_bf16
from hicom_amd import autograd as hag
from hicom_amd import native as nv
from test_gpu_ragged import MIX9, ragged_case

pytestmark = pytest.mark.gpu


def inputs_of(id):
    ff, fe, g, splits, modals = rt.stacked(mi.build(id))
    return dev_bf16(ff), dev_bf16(fe), dev_bf16(g), splits, modals


def cot_list(id, outs):
    return [torch.from_numpy(rt.cotangent(id, i, tuple(o.shape))).cuda() for i, o in enumerate(outs)]


def train_step(m, inp, cots_of, nl=None, **kw):
    """One step of the new path: (outputs, fp32 gradients, {name: .grad}) with the gradients of `m` cleared in front."""
    m.zero_grad(set_to_none=True)
    if nl is not None:
        nl.grad = None
    ff, fe, g, splits, modals = inp
    outs = m.forward_ragged_train(ff, fe, g, splits, modals, nl, **kw)
    assert isinstance(outs, list) and all(o.requires_grad for o in outs)
    sum((o * r).sum() for o, r in zip(outs, cots_of(outs))).backward()
    torch.cuda.synchronize()
    return [o.detach() for o in outs], dict(hag.LAST_FP32_GRADS), {n: p.grad for n, p in m.named_parameters()}


def loop_step(m, inp, cots_of, nl=None):
    """The loop the step replaces: forward() + backward per item, the fp32 gradients summed over the items."""
    ff, fe, g, splits, modals = inp
    modals = [modals] * len(splits) if isinstance(modals, str) else modals
    m.zero_grad(set_to_none=True)
    total, t0, outs = {}, 0, []
    for i, (T, modal) in enumerate(zip(splits, modals)):
        outs.append(m(ff[t0:t0 + T], fe[t0:t0 + T], g[i], modal, nl))
        t0 += T
    for o, r in zip(outs, cots_of(outs)):
        (o * r).sum().backward()
        for k, v in hag.LAST_FP32_GRADS.items():
            total[k] = v.double() if k not in total else total[k] + v.double()
    torch.cuda.synchronize()
    return total


def check_gradients(what, m, fp32, grads, want, loop=None, extra=()):
    bar, err = rt.bars(want), rt.errors(fp32, want)
    lerr = rt.errors(loop, want) if loop is not None else {}
    bad = []
    for k in sorted(bar):
        print(f"{what} {k}: new {err[k]:.3e}  loop {lerr.get(k, float('nan')):.3e}  bar {bar[k]:.3e}")
        if not err[k] <= bar[k]:
            bad.append(f"{k}: {err[k]:.3e} > {bar[k]:.3e}")
    for n, p in list(m.named_parameters()) + list(extra):
        if want.get(n) is None:
            assert p.grad is None, f"{n}: the reference has no gradient"
        else:
            assert p.grad is not None and p.grad.dtype == p.dtype and p.grad.shape == p.shape, n
            assert float((p.grad.float() - fp32[n].reshape(p.shape)).abs().max()) <= 2 ** -7 * float(np.abs(want[n]).max()) + bar[n], n
    assert not bad, f"{what}: " + "; ".join(bad)


@pytest.mark.parametrize("id", rt.CASES)
def test_parameter_gradients_against_fp64_oracle_autograd(id):
    """Bit-equal outputs to forward_ragged, then every parameter gradient within the bar; the loop of forward() runs beside it."""
    c = mi.build(id)
    m = build_module(c).train()
    m.graph_backward = False
    inp = inputs_of(id)
    kw = {"chunks": c.entry.chunks} if c.entry.chunks else {}
    with torch.no_grad():
        ref = m.forward_ragged(*inp, **kw)
    outs, fp32, grads = train_step(m, inp, lambda o: cot_list(id, o), **kw)
    assert len(outs) == len(ref) and all(torch.equal(a, b) for a, b in zip(outs, ref))
    loop = loop_step(m, inp, lambda o: cot_list(id, o))
    check_gradients(id, m, fp32, grads, rt.yardstick(id), loop)


def test_grid_newline_parameter_gradient():
    """mm_newline_position="grid": the image carries one newline row, the clip one per grid row; image_newline is a Parameter."""
    key = MIX9 + (True, (("mm_newline_position", "grid"),))
    c = ragged_case(*key)
    m = build_module(c).train()
    m.graph_backward = False
    nl = torch.nn.Parameter(dev_bf16(c.newline))
    inp = (dev_bf16(np.concatenate(c.ff)), dev_bf16(np.concatenate(c.fe)), dev_bf16(c.g), c.splits, c.modals)
    cots = lambda o: [torch.from_numpy(rt.cotangent("grid_newline", i, tuple(x.shape))).cuda() for i, x in enumerate(o)]
    with torch.no_grad():
        ref = m.forward_ragged(*inp, nl)
    outs, fp32, grads = train_step(m, inp, cots, nl)
    assert all(torch.equal(a, b) for a, b in zip(outs, ref))
    want = rt.oracle_grads(c.cfg, c.sd, [(c.ff[b], c.fe[b], c.g[b], c.modals[b]) for b in range(c.B)], c.newline,
                           lambda i, shape: rt.cotangent("grid_newline", i, shape))
    assert "image_newline" in fp32 and want["image_newline"] is not None
    keep = {n: p.grad for n, p in list(m.named_parameters()) + [("image_newline", nl)]}
    loop = loop_step(m, inp, cots, nl.detach())              # (the loop's d image_newline is not among its fp32 gradients: printed as nan)
    for n, p in list(m.named_parameters()) + [("image_newline", nl)]:
        p.grad = keep[n]
    check_gradients("grid_newline", m, fp32, grads, want, loop, extra=[("image_newline", nl)])


class Spy:
    """Wraps native.compressor_ragged_global_bwd: counts the calls and keeps (dS, dqt) of the last one."""

    def __init__(self, monkeypatch):
        self.calls, self.last, real = 0, None, nv.compressor_ragged_global_bwd

        def wrapped(a, x, dctx, delta, scores, ml, ds, dqt, ws):
            self.calls += 1
            real(a, x, dctx, delta, scores, ml, ds, dqt, ws)
            self.last = (ds, dqt)
        monkeypatch.setattr(nv, "compressor_ragged_global_bwd", wrapped)


@pytest.mark.parametrize("chunks", [1, 3, None])
def test_chunk_counts_stay_within_the_bar_and_do_not_depend_on_the_position(chunks, monkeypatch):
    """ragged_mix6 with chunks = 1, 3 and the default division: gradients within the bar, and what the native backward leaves for an item
    (its dS region, its dqt rows) is bit-equal when the batch is reversed -- the division is a function of the item and the totals."""
    id = "ragged_mix6"
    spy = Spy(monkeypatch)
    c = mi.build(id)
    m = build_module(c).train()
    inp = inputs_of(id)
    kw = {} if chunks is None else {"chunks": chunks}
    outs, fp32, grads = train_step(m, inp, lambda o: cot_list(id, o), **kw)
    ds, dqt = spy.last
    keep = {n: p.grad for n, p in m.named_parameters()}
    m.graph_backward = False
    loop = loop_step(m, inp, lambda o: cot_list(id, o))       # (the loop has no chunk count: the same figures beside each division)
    for n, p in m.named_parameters():
        p.grad = keep[n]
    check_gradients(f"{id} chunks={chunks}", m, fp32, grads, rt.yardstick(id), loop)
    ff, fe, g, splits, modals = inp
    B, nh = len(splits), dqt.shape[0] // len(splits)
    rev = lambda t, sizes: torch.cat(list(t.split(sizes))[::-1])
    inp_r = (rev(ff, splits), rev(fe, splits), g.flip(0), splits[::-1], modals[::-1])
    train_step(m, inp_r, lambda o: cot_list(id, o[::-1])[::-1], **kw)
    assert spy.calls == 2
    ds_r, dqt_r = spy.last
    assert torch.equal(dqt_r.view(B, nh, -1).flip(0), dqt.view(B, nh, -1))
    sizes = [16 * 16 * ((T * 36 + 15) // 16) for T in splits]            # an item's region: [16][ceil16(N)], its nh live rows first
    for b, (mine, moved) in enumerate(zip(ds.split(sizes), list(ds_r.split(sizes[::-1]))[::-1])):
        assert torch.equal(moved.view(16, -1)[:nh], mine.view(16, -1)[:nh]), f"item {b}: dS moved with the item's position"
        assert not mine.view(16, -1)[:nh, splits[b] * 36:].any(), f"item {b}: padded tail columns of dS"


def test_forward_forward_backward_backward_on_one_plan():
    """Gradient accumulation: forward A, forward B (same plan, other data), backward B, backward A equal A and B run alone, bit for bit."""
    ida, idb = "ragged_mix6", "ragged_mix6_outlier"
    m = build_module(mi.build(ida)).train()
    alone = {}
    for id in (ida, idb):
        _, _, grads = train_step(m, inputs_of(id), lambda o, id=id: cot_list(id, o))
        alone[id] = {n: g.clone() for n, g in grads.items() if g is not None}
    m.zero_grad(set_to_none=True)
    outs = {id: m.forward_ragged_train(*inputs_of(id)) for id in (ida, idb)}
    assert len(m.__dict__["_ragged_plans"]) == 1
    for id in (idb, ida):
        sum((o * r).sum() for o, r in zip(outs[id], cot_list(id, outs[id]))).backward()
        got = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
        assert got.keys() == alone[id].keys() and len(got) > 8
        for n in got:
            assert torch.equal(got[n], alone[id][n]), f"{id}: {n}"
        m.zero_grad(set_to_none=True)


def test_weights_written_through_a_flat_alias_between_two_calls():
    """An optimizer that writes a flat buffer behind the parameters (no version counter of theirs moves): the second call's output and
    gradients equal those of a fresh module built from the new weights."""
    id = "ragged_mix9"
    c = mi.build(id)
    m = build_module(c).train()
    ps = list(m.parameters())
    flat = torch.cat([p.detach().reshape(-1) for p in ps])
    o = 0
    for p in ps:
        p.data = flat[o:o + p.numel()].view(p.shape)
        o += p.numel()
    inp, cots = inputs_of(id), (lambda o: cot_list(id, o))
    out1, _, _ = train_step(m, inp, cots)
    gen = torch.Generator(device="cuda").manual_seed(5)
    flat.add_((torch.randn(flat.shape, device="cuda", generator=gen) * 0.01).to(flat.dtype))
    out2, _, g2 = train_step(m, inp, cots)
    fresh = build_module(c).train()
    fresh.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
    out3, _, g3 = train_step(fresh, inp, cots)
    assert not torch.equal(out1[0], out2[0])
    assert all(torch.equal(a, b) for a, b in zip(out2, out3))
    for n in g2:
        assert (g2[n] is None) == (g3[n] is None) and (g2[n] is None or torch.equal(g2[n], g3[n])), n


def test_refusals_leave_no_plan_and_nothing_trainable_gives_no_graph():
    id = "ragged_mix9"
    c = mi.build(id)
    ff, fe, g, splits, modals = inputs_of(id)
    adapt = build_module(mi.build("adaptkv_mix6")).train()
    clip = build_module(SimpleNamespace(cfg=SimpleNamespace(**{**vars(c.cfg), "use_clip_scale": "local"}), sd=c.sd)).train()
    assert clip.local_use_clip_scale
    plain = build_module(c).train()
    calls = [(adapt, {}), (clip, {}), (plain, {"ff": ff.clone().requires_grad_(True)}), (plain, {"fe": fe.clone().requires_grad_(True)}),
             (plain, {"g": g.clone().requires_grad_(True)})]
    for m, over in calls:
        with pytest.raises(NotImplementedError, match=r"forward\(\)"):
            m.forward_ragged_train(over.get("ff", ff), over.get("fe", fe), over.get("g", g), splits, modals)
        assert "_ragged_plans" not in m.__dict__
    plain.requires_grad_(False)
    assert torch.is_grad_enabled()
    outs = plain.forward_ragged_train(ff, fe, g, splits, modals)
    with torch.no_grad():
        ref = plain.forward_ragged(ff, fe, g, splits, modals)
    assert all(not o.requires_grad and o.grad_fn is None and torch.equal(o, r) for o, r in zip(outs, ref))


def test_only_the_local_readout_trainable_skips_the_global_backward(monkeypatch):
    id = "ragged_mix9"
    spy = Spy(monkeypatch)
    m = build_module(mi.build(id)).train()
    for n, p in m.named_parameters():
        p.requires_grad_(n.startswith("local_compressor.readout."))
    _, fp32, grads = train_step(m, inputs_of(id), lambda o: cot_list(id, o))
    assert spy.calls == 0
    want = rt.yardstick(id)
    bar, err = rt.bars(want), rt.errors(fp32, {k: v for k, v in want.items() if k.startswith("local_compressor.readout.")})
    assert len(err) == 4 and all(err[k] <= bar[k] for k in err), (err, bar)
    for n, gr in grads.items():
        assert (gr is not None) == n.startswith("local_compressor.readout."), n
