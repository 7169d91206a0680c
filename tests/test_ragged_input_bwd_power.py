"""What the references of tests/ragged_input_bwd_reference.py are, and what the cases of tests/test_gpu_ragged_train_inputs.py can see
(CPU, float64; no code of the package's hot path runs: this file says something about the REFERENCES and the TESTS, not about the kernels).

1. The two references are the autograd gradients of a small float64 model of the ragged local stage (per item: windows of the item's own
   grid, the item's guide as the query, loss = sum ctx_w . dctx_w) and of the folded global stage (per item: ctx_r = sum_n softmax(qt_r .
   x_n) x_n over the item's tokens, loss = sum ctx_r . g_r).
2. A model of the input gradients as the ragged training step computes them -- the window backward reference on the cotangent of the
   window contexts, the global dx reference on (S, dS, M, L, qt, dctx) per item -- reproduces the yardstick (fp64 autograd through the
   oracle) on d frames_feature and d frames_embed far inside the bar.  Each planted defect moves one of the two past the bar, by several
   bars, for every GPU case:
     neighbour_guide  item i's windows take the guide of item i + 1
     drop_tok0        every item reads (and writes) the stack's first tokens
     clip_kt          an image's window geometry built with the clip's temporal window
     no_global        the global share of d frames_feature dropped
     flat_tiles       64-token tiles counted from the stack's first token: a tile's tail reads the next item's coefficients
     no_key_side      (frames_embed None) the key-side term missing from d frames_feature
   The test prints, per case and mutant, the largest error in units of the bar."""
import math

import numpy as np
import pytest
import torch

import many_item_inputs as mi
import ops_reference as R
import ragged_input_bwd_reference as rr
import ragged_train_input_grads as ig
import ragged_train_inputs as rt
from oracle_util import to_t
from test_ragged_train_power import forward_state, gelu_grad

KS = 3
L = "local_compressor.readout."
MUTANTS = ("neighbour_guide", "drop_tok0", "clip_kt", "no_global", "flat_tiles")
SEVERAL = 3.0                   # "several bars"


# ---- 1: the references are autograd gradients -----------------------------------------------------------------------------------------
def small(seed=0, D=24, nh=3):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    items, H, W = [(1, 1), (4, 4), (1, 1), (8, 4)], 6, 6
    tok0, N, win0, nw = rr.offsets(items, H, W, KS)
    return dict(items=items, H=H, W=W, D=D, nh=nh, tok0=tok0, N=N, win0=win0, nw=nw, key=rnd(sum(N), D), value=rnd(sum(N), D), guides=rnd(len(items), D),
                dctx=rnd(sum(nw), D), qt=0.3 * rnd(len(items) * nh, D), gg=rnd(len(items) * nh, D))


@pytest.mark.parametrize("value_is_key", [False, True])
def test_local_reference_is_the_gradient_of_the_ragged_window_attention(value_is_key):
    s = small()
    H, W, D, scale = s["H"], s["W"], s["D"], 0.2
    key, value, guides = (s[k].clone().requires_grad_(True) for k in ("key", "value", "guides"))
    loss = 0.0
    for i, (T, kt) in enumerate(s["items"]):
        rows = slice(s["tok0"][i], s["tok0"][i] + s["N"][i])
        k_i = value[rows] if value_is_key else key[rows]
        o = R.window_attention_ref(k_i, value[rows], guides[i].expand(s["nw"][i], D), (T, H, W, kt, KS), scale, 0.0)
        loss = loss + (o["ctx"] * s["dctx"][s["win0"][i]:s["win0"][i] + s["nw"][i]]).sum()
    loss.backward()
    ref = rr.ragged_local_bwd_ref(s["value"] if value_is_key else s["key"], s["value"], s["guides"], s["dctx"], s["items"], H, W, KS, scale,
                                  value_is_key=value_is_key)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * (1 + float(b.abs().max()))
    assert close(ref["dvalue"], value.grad) and close(ref["dq_item"], guides.grad)
    assert close(ref["dq"].sum(0), guides.grad.sum(0))
    if not value_is_key:
        assert close(ref["dkey"], key.grad)
    else:
        assert key.grad is None and not ref["dkey"].any()
        lost = rr.ragged_local_bwd_ref(s["value"], s["value"], s["guides"], s["dctx"], s["items"], H, W, KS, scale, value_is_key=True, key_grad_in_dvalue=False)
        assert not close(lost["dvalue"], value.grad)
    for kw in (dict(neighbour_guide=True), dict(drop_tok0=True), dict(clip_kt=4)):
        bad = rr.ragged_local_bwd_ref(s["value"] if value_is_key else s["key"], s["value"], s["guides"], s["dctx"], s["items"], H, W, KS, scale,
                                      value_is_key=value_is_key, **kw)
        assert not close(bad["dvalue"], value.grad), kw


def test_global_reference_is_the_gradient_of_the_folded_global_attention_per_item():
    s = small(1)
    nh, x = s["nh"], s["value"].clone().requires_grad_(True)
    S, dS, ml, loss = [], [], [], 0.0
    for i, n in enumerate(s["N"]):
        rows, tok = slice(i * nh, (i + 1) * nh), slice(s["tok0"][i], s["tok0"][i] + n)
        qt, gg = s["qt"][rows], s["gg"][rows]
        ctx = torch.softmax(qt @ x[tok].t(), 1) @ x[tok]
        loss = loss + (ctx * gg).sum()
        S_i, ml_i, dS_i, _ = R.global_attention_backward_ref(qt, s["value"][tok], gg)
        pad = torch.full((nh, 16 - n % 16), float("nan"), dtype=torch.float64)              # (padding columns are never read)
        S.append(torch.cat([S_i, pad], 1)); dS.append(torch.cat([dS_i, pad], 1)); ml.append(ml_i)
    loss.backward()
    dx, _, _ = rr.ragged_global_dx_ref(S, dS, torch.cat(ml), s["qt"], s["gg"], s["N"], nh)
    assert float((dx - x.grad).abs().max()) <= 1e-12 * (1 + float(x.grad.abs().max()))
    dx0 = torch.ones_like(dx)
    assert torch.equal(rr.ragged_global_dx_ref(S, dS, torch.cat(ml), s["qt"], s["gg"], s["N"], nh, dx0=dx0)[0], dx + dx0)
    wrong, _, _ = rr.ragged_global_dx_ref(S, dS, torch.cat(ml), s["qt"], s["gg"], s["N"], nh, flat_tiles=64)
    edges = [t for t in s["tok0"][1:] if t % 64]
    assert edges and all(not torch.equal(wrong[t], dx[t]) for t in edges) and torch.equal(wrong[:s["tok0"][1]], dx[:s["tok0"][1]])


# ---- 2: the model of the step's input gradients, and its mutants ------------------------------------------------------------------------
def model_input_grads(id, with_fe=True, mutant=None):
    """(d frames_feature, d frames_embed or None) [sum N_i, E] float64 of case `id` as the ragged training step forms them."""
    c = mi.build(id)
    f64 = torch.float64
    sd = {k: to_t(v, f64) for k, v in c.sd.items() if k.startswith(L)}
    W0, b0, W2 = sd[L + "0.weight"], sd[L + "0.bias"], sd[L + "2.weight"]
    st = forward_state(id)
    E, nh = st["E"], st["Wk"].shape[0]
    items = [(ff.shape[0], 4 if ff.shape[0] % 4 == 0 else 1) for ff, _, _, _ in c.items]
    H, W = c.items[0][0].shape[1:3]
    x = torch.cat([to_t(ff, f64).reshape(-1, E) for ff, _, _, _ in c.items])
    keys = torch.cat([to_t(fe, f64).reshape(-1, E) for _, fe, _, _ in c.items]) if with_fe else x
    guides = torch.stack([to_t(g, f64) for _, _, g, _ in c.items])
    tok0, N, win0, nw = rr.offsets(items, H, W, KS)
    scale = E ** -0.5
    dctx_l = []
    for i, (T, kt) in enumerate(items):                               # the cotangent of the window contexts, through the local readout
        rows = slice(tok0[i], tok0[i] + N[i])
        ctx = R.window_attention_ref(keys[rows], x[rows], guides[i].expand(nw[i], E), (T, H, W, kt, KS), scale, 0.0)["ctx"]
        cot = torch.from_numpy(rt.cotangent(id, i, (nw[i] + mi.NG, W2.shape[0]))).double()[:nw[i]]
        dctx_l.append((gelu_grad(ctx @ W0.t() + b0) * (cot @ W2)) @ W0)
    kw = {"neighbour_guide": dict(neighbour_guide=True), "drop_tok0": dict(drop_tok0=True), "clip_kt": dict(clip_kt=4),
          "no_key_side": dict(key_grad_in_dvalue=False)}.get(mutant, {})
    loc = rr.ragged_local_bwd_ref(keys, x, guides, torch.cat(dctx_l), items, H, W, KS, scale, value_is_key=not with_fe, **kw)
    d_ff = loc["dvalue"]
    if mutant != "no_global":
        S, dS, ml, qt, dctx = [], [], [], [], []
        for it in st["items"]:
            p = torch.exp(it["S"] - it["M"][:, None]) / it["L"][:, None]
            S.append(it["S"]); ml.append(torch.stack([it["M"], it["L"]], 1)); dctx.append(it["dctx"])
            dS.append(p * (it["dctx"] @ it["xp"].t() - it["delta"][:, None]))
            qt.append(st["scale"] * torch.einsum("hje,hj->he", st["Wk"], it["qp"]))
        d_ff = d_ff + rr.ragged_global_dx_ref(S, dS, torch.cat(ml), torch.cat(qt), torch.cat(dctx), N, nh, flat_tiles=64 if mutant == "flat_tiles" else None)[0]
    return d_ff, (loc["dkey"] if with_fe else None), N


def in_bars(id, with_fe, got):
    """Largest error of d frames_feature / d frames_embed against the yardstick, per item in units of the item's bar."""
    _, want = ig.yardstick(id, with_fe)
    d_ff, d_fe, N = got
    worst = {}
    for name, d in (("frames_feature", d_ff), ("frames_embed", d_fe)):
        if d is None:
            continue
        errs = [float(np.abs(part.numpy().reshape(w.shape) - w).max()) / ig.item_bar(w) for part, w in zip(d.split(N), want[name])]
        worst[name] = max(e if math.isfinite(e) else math.inf for e in errs)
    return worst


def has_image_in_front_of_a_clip(id):
    T = [ff.shape[0] for ff, _, _, _ in mi.build(id).items]
    return any(t < 4 for t in T)


@pytest.mark.parametrize("id", rt.CASES)
def test_every_mutant_moves_an_input_gradient_by_several_bars(id):
    clean = in_bars(id, True, model_input_grads(id))
    print(f"{id} model vs yardstick: " + "  ".join(f"{k} {v:.2e}" for k, v in clean.items()) + "  (bars)")
    assert max(clean.values()) <= 0.05, f"{id}: the model is not the yardstick's backward: {clean}"
    slipped = []
    for mutant in MUTANTS:
        if mutant == "clip_kt" and not has_image_in_front_of_a_clip(id):
            continue                                                   # (no item shorter than the clip's temporal window: the defect has nothing to act on)
        moved = in_bars(id, True, model_input_grads(id, mutant=mutant))
        print(f"{id} {mutant}: " + "  ".join(f"{k} {v:.3g}" for k, v in moved.items()) + "  (bars)")
        if not max(moved.values()) > SEVERAL:
            slipped.append(f"{mutant}: at most {max(moved.values()):.3g} bars")
    assert not slipped, f"{id}: " + "; ".join(slipped)


@pytest.mark.parametrize("id", ["ragged_mix6", "batch_image_81"])
def test_the_missing_key_side_term_is_seen_without_frames_embed(id):
    clean = in_bars(id, False, model_input_grads(id, with_fe=False))
    assert max(clean.values()) <= 0.05, clean
    moved = in_bars(id, False, model_input_grads(id, with_fe=False, mutant="no_key_side"))
    print(f"{id} no_key_side: {moved}  (bars)")
    assert max(moved.values()) > SEVERAL, moved
