"""forward_ragged(local_logits=) and forward_ragged_train(local_logits=) (GPU): the ragged step and its training step with
the local scores given in the place of frames_embed (csrc/ragged.hip: ragged_local_logits_kernel; csrc/ragged_train.hip:
ragged_local_logits_bwd_kernel), on the hidden-64 cases of tests/ragged_train_inputs.py under the references and bars of
tests/ragged_logits_inputs.py.  Every test here fails without the feature: the keyword and the two exports do not exist there.

The second check of d local_logits holds it against the keyed step's own d frames_embed: bf16(dl_n g_item) against the bf16 rows of
forward_ragged_train(frames_embed, input_grads=True).  Both are one rounding to bf16 of fp32 values that agree to a few fp32 ulps, so an
entry either agrees exactly or, where the two fp32 values straddle a rounding boundary, lands ONE bf16 ulp apart -- twice the half ulp that
bounds the keyed path's distance from fp64 at that entry.  A max-abs cannot be held against that distance; the test asserts that no entry
differs by more than one bf16 ulp of the item's largest (2^-7 mx) and holds the agreement per item in the L2 norm, where the rare
one-ulp entries weigh what they are: it must be no worse than the keyed path's own L2 distance from fp64.  Both distances are printed,
in both norms.

The kernel alone: hicom_compressor_ragged_local_logits_bwd from synthetic state (no forward is run), in the style of
tests/test_gpu_ragged_global_bwd.py; its bounds are derived in kernel_case().

Measured on an MI355X: forward local rows 3.7e-5 .. 8.9e-5 under `edge` (bar 1e-3), 5.4e-4 .. 9.7e-4 of bars of 1.5e-3 .. 2.5e-3 under
`edge_outlier`, bit-equal to the ragged multi-guide step's on every item; d local_logits at worst 2.16e-5 of a bar of 9.63e-5
(ragged_mix6_outlier item 0); d frames_feature at worst 2.26e-4 of 4.15e-4 (batch_T8_chunks18 item 0); d guide_embeds at most 0.9 % of its
bar; bf16(dl g) against the keyed d frames_embed: L2 at worst 0.15 of the keyed path's own distance from fp64, max-abs at most 2.4e-4
against 5.4e-4; the kernel alone: dl 6.1e-3 of its bound, dvalue 0.995 of its bound (the one rounding to bf16)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import many_item_inputs as mi
import ragged_logits_inputs as li
import ragged_train_input_grads as ig
import ragged_train_inputs as rt
from gpu_util import build_module, dev_bf16
from hicom_amd import autograd as hag
from hicom_amd import native as nv
from hicom_amd import ragged
from ops_reference import up

pytestmark = pytest.mark.gpu

NG = mi.NG


def leaves(id, need=(True, True, True)):
    """(frames_feature, guides, local_logits, frames_embed (never requiring grad), split_sizes, modals); need: (ff, guides, logits)."""
    ff, fe, g, splits, modals = rt.stacked(mi.build(id))
    ll = torch.from_numpy(np.array(li.scores(id))).cuda()
    return dev_bf16(ff).requires_grad_(need[0]), dev_bf16(g).requires_grad_(need[1]), ll.requires_grad_(need[2]), dev_bf16(fe), splits, modals


def kw_of(id):
    e = mi.build(id).entry
    return {"chunks": e.chunks} if e.chunks else {}


def cot_list(id, outs):
    return [torch.from_numpy(rt.cotangent(id, i, tuple(o.shape))).cuda() for i, o in enumerate(outs)]


def step(m, inp, id, keyed=False, **kw):
    """One training step: (outputs, fp32 gradients, parameter .grad, (d ff, d guide, d logits | d fe)).  keyed: the existing step on
    frames_embed (requiring grad) in the place of the scores."""
    m.zero_grad(set_to_none=True)
    ff, g, ll, fe, splits, modals = inp
    key = fe.detach().clone().requires_grad_(True) if keyed else ll
    for t in (ff, g, key):
        t.grad = None
    if keyed:
        outs = m.forward_ragged_train(ff, key, g, splits, modals, **kw)
    else:
        outs = m.forward_ragged_train(ff, None, g, splits, modals, local_logits=ll, **kw)
    sum((o * r).sum() for o, r in zip(outs, cot_list(id, outs))).backward()
    torch.cuda.synchronize()
    return ([o.detach() for o in outs], dict(hag.LAST_FP32_GRADS), {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()},
            tuple(None if t.grad is None else t.grad.clone() for t in (ff, g, key)))


# ---- forward ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", li.CASES)
def test_forward_against_the_keyed_step_and_the_oracle(id):
    """Global rows bit-equal to forward_ragged with frames_embed; every item's local rows inside the keyed step's bar against the oracle;
    the [1, sum T_i, H, W] form of the scores gives the same bits; the local rows are the ragged multi-guide step's with one guide per item
    (both launch multi_window_logits_ctx16<3, 1> on the same window, scores and value rows, and the same readout GEMMs over the same rows)."""
    c, want = mi.build(id), mi.oracle_outputs(id)
    m = build_module(c)
    ff, g, ll, fe, splits, modals = leaves(id, need=(False, False, False))
    kw = kw_of(id)
    with torch.no_grad():
        keyed = m.forward_ragged(ff, fe, g, splits, modals, **kw)
        out = m.forward_ragged(ff, None, g, splits, modals, local_logits=ll, **kw)
        out4 = m.forward_ragged(ff, None, g, splits, modals, local_logits=ll[None], **kw)
        rmg = m.forward_ragged_multi_guide(ff, None, g, splits, (1,) * len(splits), modals, local_logits=ll[None], **kw)
    torch.cuda.synchronize()
    bad = []
    for b in range(c.B):
        assert out[b].dtype == torch.float32 and tuple(out[b].shape) == want[b].shape
        assert torch.equal(out[b][-NG:], keyed[b][-NG:]), f"item {b}: the global rows moved with local_logits"
        assert torch.equal(out[b], out4[b]), f"item {b}: the [1, sum T_i, H, W] form"
        bad += mi.check_item(c.entry, f"item {b} (logits)", out[b].cpu().numpy(), want[b])
        same_l, same_g = torch.equal(out[b][:-NG], rmg[b][0][:-NG]), torch.equal(out[b][-NG:], rmg[b][0][-NG:])
        print(f"{id} item {b}: local rows bit-equal to forward_ragged_multi_guide(guide_counts=(1,)*B, local_logits=): {same_l}; global rows: {same_g}")
        assert same_l, f"item {b}: local rows differ from the ragged multi-guide step's"
    assert not bad, f"{id}: " + "; ".join(bad)


# ---- training --------------------------------------------------------------------------------------------------------------------------------
def check_params(what, fp32, want):
    bar, err = rt.bars(want), rt.errors(fp32, want)
    bad = [f"{k}: {err[k]:.3e} > {bar[k]:.3e}" for k in sorted(bar) if not err[k] <= bar[k]]
    assert not bad, f"{what}: " + "; ".join(bad)


@pytest.mark.parametrize("id", li.CASES)
def test_training_step_against_fp64_oracle_autograd(id):
    """Outputs bit-equal to forward_ragged(local_logits=); the parameter gradients under ragged_train_inputs.bars, bit-equal between
    input_grads=True with the inputs requiring grad, input_grads=True with them detached and input_grads=False; d local_logits,
    d frames_feature and d guide_embeds (the global share) under their bars; d local_logits against the keyed step's d frames_embed."""
    c = mi.build(id)
    m = build_module(c).train()
    m.graph_backward = False
    kw = kw_of(id)
    inp = leaves(id)
    ff, g, ll, fe, splits, modals = inp
    with torch.no_grad():
        ref = m.forward_ragged(ff.detach(), None, g.detach(), splits, modals, local_logits=ll.detach(), **kw)
    outs, fp32, grads, (d_ff, d_g, d_ll) = step(m, inp, id, input_grads=True, **kw)
    assert len(outs) == len(ref) and all(torch.equal(a, b) for a, b in zip(outs, ref))
    check_params(id, fp32, rt.yardstick(id))
    want_params, want_in = ig.yardstick(id)
    bad = []
    # d local_logits: fp32, the tensor's own shape, per item under the input-gradient bar
    assert d_ll is not None and d_ll.dtype == torch.float32 and d_ll.shape == ll.shape
    for i, (e, bar) in enumerate(li.dl_errors(d_ll, id, splits)):
        print(f"{id} d local_logits item {i}: {e:.3e}  bar {bar:.3e}")
        if not e <= bar:
            bad.append(f"d local_logits item {i}: {e:.3e} > {bar:.3e}")
    # d frames_feature: the oracle's (value-side + global share), the bars of the keyed step's input gradients
    assert d_ff is not None and d_ff.dtype == ff.dtype and d_ff.shape == ff.shape
    for i, (e, bar, se, sbar) in enumerate(ig.item_errors(d_ff, want_in["frames_feature"], splits)):
        print(f"{id} d frames_feature item {i}: {e:.3e}  bar {bar:.3e};  sum {se:.3e}  bar {sbar:.3e}")
        if not e <= bar:
            bad.append(f"d frames_feature item {i}: {e:.3e} > {bar:.3e}")
        if not se <= sbar:
            bad.append(f"sum d frames_feature item {i}: {se:.3e} > {sbar:.3e}")
    # d guide_embeds: the global share only
    g32, wg = fp32["__guide_embeds__"], li.dguide_reference(id)
    assert d_g is not None and d_g.dtype == g.dtype and d_g.shape == g.shape and torch.equal(g32.to(g.dtype), d_g)
    e, bar = float((g32.double().cpu() - torch.from_numpy(np.array(wg))).abs().max()), ig.guide_bar(want_params, wg)
    print(f"{id} d guide_embeds (global share): {e:.3e}  bar {bar:.3e}")
    if not e <= bar:
        bad.append(f"d guide_embeds: {e:.3e} > {bar:.3e}")
    # the parameter gradients do not move with the input gradients
    keep = {n: v for n, v in grads.items() if v is not None}
    for what, extra in (("input_grads=True, inputs detached", {"input_grads": True}), ("input_grads=False", {})):
        _, _, detached, none = step(m, leaves(id, need=(False, False, False)), id, **extra, **kw)
        assert none == (None, None, None), what
        assert keep.keys() == {n for n, v in detached.items() if v is not None}, what
        for n in keep:
            assert torch.equal(keep[n], detached[n]), f"{n}: moved ({what})"
    # the second check: bf16(dl_n g_item) against the keyed step's d frames_embed (module docstring)
    _, _, _, (_, _, d_fe) = step(m, inp, id, keyed=True, input_grads=True, **kw)
    t0 = 0
    for i, (T, want) in enumerate(zip(splits, want_in["frames_embed"])):
        mine = (d_ll[t0:t0 + T].reshape(-1, 1) * g[i].detach().float().reshape(1, -1)).to(torch.bfloat16).double().cpu().numpy().reshape(want.shape)
        key = d_fe[t0:t0 + T].double().cpu().numpy().reshape(want.shape)
        a_max, b_max = float(np.abs(mine - key).max()), float(np.abs(key - want).max())
        a_l2, b_l2 = float(np.sqrt(((mine - key) ** 2).sum())), float(np.sqrt(((key - want) ** 2).sum()))
        print(f"{id} item {i}: bf16(dl g) vs keyed d frames_embed: max {a_max:.3e} L2 {a_l2:.3e};  keyed vs fp64: max {b_max:.3e} L2 {b_l2:.3e}")
        ulp = 2.0 ** -7 * float(np.abs(key).max())
        if not a_max <= ulp:
            bad.append(f"item {i}: bf16(dl g) is {a_max:.3e} from the keyed d frames_embed, more than one bf16 ulp of its largest entry ({ulp:.3e})")
        if not a_l2 <= b_l2:
            bad.append(f"item {i}: bf16(dl g) agrees with the keyed d frames_embed to {a_l2:.3e} (L2), the keyed path with fp64 to {b_l2:.3e}")
        t0 += T
    assert not bad, f"{id}: " + "; ".join(bad)


class Spy:
    """Counts the calls of the native wrappers of the ragged training surface."""
    NAMES = ("compressor_ragged_fwd", "compressor_ragged_logits_fwd", "compressor_ragged_local_bwd", "compressor_ragged_local_logits_bwd",
             "compressor_ragged_global_bwd", "compressor_ragged_global_dx")

    def __init__(self, monkeypatch):
        self.calls = dict.fromkeys(self.NAMES, 0)
        for name in self.NAMES:
            monkeypatch.setattr(nv, name, self.wrap(name, getattr(nv, name)))

    def wrap(self, name, real):
        def wrapped(*a, **k):
            self.calls[name] += 1
            return real(*a, **k)
        return wrapped


def test_a_parameters_only_step_runs_the_new_forward_and_no_new_backward_launch(monkeypatch):
    """Stages 1 and 2: the head is frozen, nothing of the inputs requires grad.  The parameter gradients are those of the keyed step up to
    the local contexts' own difference: held against the oracle."""
    id = "ragged_mix6"
    spy = Spy(monkeypatch)
    m = build_module(mi.build(id)).train()
    m.graph_backward = False
    _, fp32, grads, none = step(m, leaves(id, need=(False, False, False)), id)
    assert none == (None, None, None)
    assert spy.calls == {"compressor_ragged_fwd": 0, "compressor_ragged_logits_fwd": 1, "compressor_ragged_local_bwd": 0,
                         "compressor_ragged_local_logits_bwd": 0, "compressor_ragged_global_bwd": 1, "compressor_ragged_global_dx": 0}
    check_params(id, fp32, rt.yardstick(id))


def test_only_the_scores_requiring_grad_makes_no_global_stage_call(monkeypatch):
    id = "ragged_mix9"
    spy = Spy(monkeypatch)
    m = build_module(mi.build(id)).train().requires_grad_(False)
    inp = leaves(id, need=(False, False, True))
    _, fp32, grads, (d_ff, d_g, d_ll) = step(m, inp, id, input_grads=True)
    assert spy.calls["compressor_ragged_local_logits_bwd"] == 1 and spy.calls["compressor_ragged_global_bwd"] == 0 and spy.calls["compressor_ragged_global_dx"] == 0
    assert d_ff is None and d_g is None and all(v is None for v in grads.values())
    assert all(e <= bar for e, bar in li.dl_errors(d_ll, id, inp[4]))
    with pytest.raises(NotImplementedError, match=r"local_logits.*forward\(\)"):
        m.forward_ragged_train(inp[0], None, inp[1], inp[4], inp[5], local_logits=inp[2])       # the default keeps the refusal


def test_two_identical_steps_give_bit_equal_gradients():
    id = "ragged_mix6_outlier"
    m = build_module(mi.build(id)).train()
    inp = leaves(id)
    _, f1, _, g1 = step(m, inp, id, input_grads=True)
    _, f2, _, g2 = step(m, inp, id, input_grads=True)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2)) and torch.equal(f1["__guide_embeds__"], f2["__guide_embeds__"])


# ---- the kernel alone ------------------------------------------------------------------------------------------------------------------------
E, NH, H, W, KS, HIDDEN = 1152, 9, 6, 6, 3, 64
SPLITS = (1, 4, 1, 8, 1)                # token offsets 36, 180, 216, 504; windows of 9, 36, 9, 36, 9 tokens: 4 + 4 + 4 + 8 + 4 of them
L_SCALE = 0.125
SPIKE = 30.0                            # one token per window stands 30 above the rest of its raw scores: 3.75 in the softmax's units
LEVEL = 1000.0                          # item b's raw scores stand on b x 1000: a window that took its neighbour item's scores, or a softmax
                                        # without its own maximum, is off by e^(+-125)
GUARD = 64


def descriptors():
    return [(T, 4 if T % 4 == 0 else 1, 0, 0, 0, 1, 32) for T in SPLITS]


@functools.lru_cache(maxsize=None)
def kernel_case():
    """Host tensors, the float64 restatement of the three formulas and the bounds.
    Bounds, per token n of a window (u = 2^-24; dc = dctx_w):
      dp_n      a 1152-term fp32 dot product: 18 fma per lane and six levels of the wave sum: e_n = 32 u |dc| . |v_n|
      p_n       scale l, the maximum, expf, the 64-lane sum and one division: relative 2^-18 (a window holds <= 36 live terms)
      dl_n      scale p_n (dp_n - delta), delta = sum_m p_m dp_m:
                scale p_n [e_n + sum_m p_m e_m + 2^-17 (|dp_n| + sum_m p_m |dp_m|)]   (the last term: p's relative error on both, the sums' and
                the products' roundings)
      dv_n      bf16(p_n dc): half a bf16 ulp, <= 2^-8 |p_n dc|, + p's 2^-18."""
    gen = torch.Generator().manual_seed(4321)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    desc = descriptors()
    t = ragged.plan_tables(desc, H, W, KS, 256, 1)
    N, nwin = sum(t.N), sum(t.windows)
    c = SimpleNamespace(N=N, nwin=nwin, t=t)
    c.value = rnd(N, E).bfloat16().contiguous()
    c.dctx = (0.05 * rnd(nwin, E)).contiguous()
    c.logits = torch.zeros(N)
    c.dl, c.dl_tol = torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    c.dv, c.dv_tol = torch.zeros(N, E, dtype=torch.float64), torch.zeros(N, E, dtype=torch.float64)
    c.count = torch.zeros(N, dtype=torch.int64)
    c.spiked_mass = []
    u = 2.0 ** -24
    for b, (T, kt, *_) in enumerate(desc):
        wins = [(t1, h1, w1) for t1 in range(T // kt) for h1 in range(H // KS) for w1 in range(W // KS)]
        for k, (t1, h1, w1) in enumerate(wins):
            toks = torch.tensor([t.tok0[b] + ((t1 * kt + t2) * H + h1 * KS + h2) * W + w1 * KS + w2
                                 for t2 in range(kt) for h2 in range(KS) for w2 in range(KS)])
            win = t.win0[b] + k
            raw = 2.0 * rnd(len(toks)) + LEVEL * b                 # (0.25 in the softmax's units: the spike stands clear of the noise)
            raw[(7 * win + 3) % len(toks)] += SPIKE
            c.logits[toks] = raw
            l = up(c.logits[toks])                               # (the fp32 values the kernel reads)
            p = torch.softmax(L_SCALE * l, 0)
            dc, v = up(c.dctx[win]), up(c.value[toks])
            dp, e = v @ dc, 32 * u * (v.abs() @ dc.abs())
            delta = (p * dp).sum()
            c.dl[toks] = L_SCALE * p * (dp - delta)
            c.dl_tol[toks] = L_SCALE * p * (e + (p * e).sum() + 2.0 ** -17 * (dp.abs() + (p * dp.abs()).sum())) + 1e-300
            c.dv[toks] = p[:, None] * dc[None, :]
            c.dv_tol[toks] = (2.0 ** -8 + 2.0 ** -18) * c.dv[toks].abs() + 1e-300
            c.count[toks] += 1
            c.spiked_mass.append(float(p.max()))
    return c


def run_kernel(with_dvalue=True):
    dev = torch.device("cuda")
    c = kernel_case()
    desc = descriptors()
    a = nv.CompressorRaggedArgs()
    items = (nv.RaggedItem * len(desc))(*[nv.RaggedItem(*d) for d in desc])
    a.B, a.H, a.W, a.E, a.hidden, a.ks, a.nh, a.chunks, a.items = len(desc), H, W, E, HIDDEN, KS, NH, 1, items
    a.l_scale = L_SCALE
    a.stream = torch.cuda.current_stream(dev).cuda_stream
    pws = torch.zeros((nv.compressor_ragged_workspace(a),), dtype=torch.uint8, device=dev)
    a.ws, a.ws_bytes = pws.data_ptr(), pws.numel()
    nv.compressor_ragged_prepare(a)
    dl_buf = torch.full((c.N + 2 * GUARD,), float("nan"), device=dev)
    dv_buf = torch.full((c.N + 2, E), float("nan"), dtype=torch.bfloat16, device=dev)          # a guard row in front and behind
    value, logits, dctx = (v.to(dev) for v in (c.value, c.logits, c.dctx))
    before = [v.clone() for v in (value, logits, dctx)]
    nv.compressor_ragged_local_logits_bwd(a, value, logits, dctx, dl_buf[GUARD:-GUARD], dv_buf[1:-1] if with_dvalue else None)
    torch.cuda.synchronize()
    assert all(torch.equal(v.view(torch.uint8), w.view(torch.uint8)) for v, w in zip((value, logits, dctx), before)), "an input was written"
    return c, dl_buf.cpu(), dv_buf.cpu()


def test_kernel_alone_against_the_float64_formulas():
    c, dl_buf, dv_buf = run_kernel()
    assert (c.count == 1).all()                                  # (the host's own walk: every token in exactly one window)
    dl, dv = up(dl_buf[GUARD:-GUARD]), up(dv_buf[1:-1])
    assert torch.isfinite(dl).all() and torch.isfinite(dv).all(), "a token was not written"
    assert torch.isnan(dl_buf[:GUARD]).all() and torch.isnan(dl_buf[-GUARD:]).all(), "d local_logits: written outside its tokens"
    assert torch.isnan(dv_buf[0].float()).all() and torch.isnan(dv_buf[-1].float()).all(), "dvalue: written outside its rows"
    r_dl, r_dv = ((dl - c.dl).abs() / c.dl_tol).max(), ((dv - c.dv).abs() / c.dv_tol).max()
    print(f"kernel alone: dl {float((dl - c.dl).abs().max()):.3e} ({float(r_dl):.2e} of its bound, max |dl| {float(c.dl.abs().max()):.3e}), "
          f"dvalue {float((dv - c.dv).abs().max()):.3e} ({float(r_dv):.2e} of its bound); spiked token's mass {min(c.spiked_mass):.2f} .. {max(c.spiked_mass):.2f}")
    assert float(r_dl) <= 1.0 and float(r_dv) <= 1.0
    assert min(c.spiked_mass) > 0.3                              # the spikes do what they are for


def test_kernel_alone_without_dvalue_writes_the_same_scores_gradient():
    c, dl_a, _ = run_kernel()
    _, dl_b, dv_b = run_kernel(with_dvalue=False)
    assert torch.equal(dl_a[GUARD:-GUARD], dl_b[GUARD:-GUARD])
    assert torch.isnan(dv_b.float()).all(), "dvalue NULL: nothing may be written"
