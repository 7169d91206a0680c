"""Whether the GPU tests of forward_ragged_train(adaptors=True) can see the mistakes a ragged adaptor backward can make (CPU, fp64).

A model of the step's local stage as ragged_train.py and csrc/ragged_train.hip compute it -- the window backward's per-token (ds, pw) and per-window
sums, the dy step with the token -> (item, window) lookup of ragged.token_item_window, the adaptor MLPs' backward over the stacked tokens, the
input gradients -- is held against torch autograd (fp64) through the same local stage written as a plain forward, on the inputs and weights of
every case of tests/test_gpu_ragged_train_adapt.py with a seeded cotangent of the window contexts.  Without a defect the model equals autograd
to fp64 rounding.  Each of five planted defects must move some gradient by more than MIN_BARS of that gradient's bar on EVERY case (bars:
tests/ragged_train_inputs.bars' rule for parameters and d guide, tests/ragged_train_input_grads.item_bar for the bf16 inputs); the smallest
figure over the cases is printed per defect."""
import functools

import numpy as np
import pytest
import torch

import ragged_train_adapt_inputs as ra
import ragged_train_input_grads as ig
import ragged_train_inputs as rt
from hicom_amd import ragged

F = torch.nn.functional
DEFECTS = ("neighbour_guide_in_k_vector", "tok0_dropped_from_y_rows", "image_built_with_clip_kt", "item_local_window_for_v_vector",
           "key_side_term_missing_without_fe")
MIN_BARS = 5.0
L = "local_compressor."
KS, LN_EPS = 3, 1e-6


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


@functools.lru_cache(maxsize=None)
def setup(id):
    c = ra.build(id)
    side = c.ff[0].shape[1]
    items = [(T, 1 if (m == "image" or T == 1) else 4, 0, 0, 0, 1, 32) for T, m in zip(c.splits, c.modals)]
    tab = ragged.plan_tables(items, side, side, KS, 256)
    item_of, win_of = ragged.token_item_window(tab, side, side, KS)
    sd = {k[len(L):]: t64(v) for k, v in c.sd.items() if k.startswith((L + "k_", L + "v_"))}
    D = c.g.shape[1]
    ff = t64(np.concatenate(c.ff)).reshape(-1, D)
    fe = None if c.fe is None else t64(np.concatenate(c.fe)).reshape(-1, D)
    rng = np.random.default_rng(5)
    dctx = t64(rng.standard_normal((sum(tab.windows), D)) * 0.1)
    return dict(c=c, side=side, tab=tab, item_of=torch.from_numpy(item_of), win_of=torch.from_numpy(win_of), sd=sd, ff=ff, fe=fe, g=t64(c.g), dctx=dctx,
                adapt_k="k_alpha" in sd, adapt_v="v_alpha" in sd, scale=D ** -0.5, D=D)


def mlp(x, p, s):
    return F.linear(F.gelu(F.linear(x, p[s + "_proj.0.weight"], p[s + "_proj.0.bias"])), p[s + "_proj.2.weight"], p[s + "_proj.2.bias"])


def lnorm(y):
    mu = y.mean(-1, keepdim=True)
    rstd = torch.rsqrt(y.var(-1, unbiased=False, keepdim=True) + LN_EPS)
    return (y - mu) * rstd, rstd


def segment_softmax(s, win_of, NW):
    mx = torch.full((NW,), -1e300, dtype=s.dtype).scatter_reduce(0, win_of, s, "amax")
    e = torch.exp(s - mx[win_of])
    return e / torch.zeros(NW, dtype=s.dtype).index_add(0, win_of, e)[win_of]


def autograd_reference(S):
    """Gradients of sum(ctx * dctx) through the local stage written as a forward: parameters, d ff, d fe, d guide."""
    p = {k: v.clone().requires_grad_(True) for k, v in S["sd"].items()}
    ff, g = S["ff"].clone().requires_grad_(True), S["g"].clone().requires_grad_(True)
    fe = None if S["fe"] is None else S["fe"].clone().requires_grad_(True)
    key = fe if fe is not None else ff
    K = (1 - p["k_alpha"]) * key + p["k_alpha"] * F.layer_norm(mlp(key, p, "k"), (S["D"],), p["k_norm.weight"], p["k_norm.bias"], LN_EPS) if S["adapt_k"] else key
    V = (1 - p["v_alpha"]) * ff + p["v_alpha"] * F.layer_norm(mlp(ff, p, "v"), (S["D"],), p["v_norm.weight"], p["v_norm.bias"], LN_EPS) if S["adapt_v"] else ff
    NW = S["dctx"].shape[0]
    pr = segment_softmax(S["scale"] * (K * g[S["item_of"]]).sum(-1), S["win_of"], NW)
    ctx = torch.zeros((NW, S["D"]), dtype=torch.float64).index_add(0, S["win_of"], pr[:, None] * V)
    (ctx * S["dctx"]).sum().backward()
    out = {L + k: v.grad for k, v in p.items() if v.grad is not None}
    out.update(frames_feature=ff.grad, guide_embeds=g.grad)
    if fe is not None:
        out["frames_embed"] = fe.grad
    return out


def step_model(S, defect=None):
    """The same gradients as the step computes them; `defect` plants one mistake."""
    sd, D, NW = S["sd"], S["D"], S["dctx"].shape[0]
    tab, side = S["tab"], S["side"]
    item_of, win_of = S["item_of"], S["win_of"]
    if defect == "image_built_with_clip_kt":              # every item's windows from its right neighbour's kt (the last item: its left one's)
        kts = [it[1] for it in tab.items]
        items = [(it[0], min(it[0], kts[(i + 1) % len(kts)] if i + 1 < len(kts) else kts[i - 1]), *it[2:]) for i, it in enumerate(tab.items)]
        bad = ragged.plan_tables(items, side, side, KS, 256)
        bad.win0 = tab.win0                               # (the table's first windows stay: only the geometry inside an item is wrong)
        _, w = ragged.token_item_window(bad, side, side, KS)
        win_of = torch.from_numpy(np.minimum(w, NW - 1))
    ff, fe, g, dctx = S["ff"], S["fe"], S["g"], S["dctx"]
    key = fe if fe is not None else ff
    tok0 = torch.tensor(tab.tok0)[item_of]
    grads = {}
    y, yh, rs = {}, {}, {}
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xin = {"k": key.clone().requires_grad_(True), "v": ff.clone().requires_grad_(True)}
    for s_, on in (("k", S["adapt_k"]), ("v", S["adapt_v"])):
        if on:
            y[s_] = mlp(xin[s_], leaf, s_)
            yd = y[s_].detach()
            if defect == "tok0_dropped_from_y_rows":      # the y row of a token read at its item-local index
                yd = yd[torch.arange(yd.shape[0]) - tok0]
            yh[s_], rs[s_] = lnorm(yd)
    blend = lambda x, s_: (1 - sd[s_ + "_alpha"]) * x + sd[s_ + "_alpha"] * (yh[s_] * sd[s_ + "_norm.weight"] + sd[s_ + "_norm.bias"]) if s_ in yh else x
    K, V = blend(key, "k"), blend(ff, "v")
    q = g[item_of]
    pw = segment_softmax(S["scale"] * (K * q).sum(-1), win_of, NW)
    dP = (V * dctx[win_of]).sum(-1)
    delta = torch.zeros(NW, dtype=torch.float64).index_add(0, win_of, pw * dP)
    ds = S["scale"] * pw * (dP - delta[win_of])
    wsum = lambda wt, rows: torch.zeros((NW, D), dtype=torch.float64).index_add(0, win_of, wt[:, None] * rows)
    qf = g[torch.from_numpy(tab.win_item.astype(np.int64))]
    # the rank-1 vectors as the dy step indexes them
    k_vec = g[(item_of + 1) % g.shape[0]] if defect == "neighbour_guide_in_k_vector" else q
    v_vec = dctx[win_of - torch.tensor(tab.win0)[item_of]] if defect == "item_local_window_for_v_vector" else dctx[win_of]

    def stream(s_, coef, vec, x):
        """d x of one stream and its adaptor's gradients (the MLP's by autograd through y with dy as the cotangent)."""
        if s_ not in yh:
            return coef[:, None] * vec
        a, gm = sd[s_ + "_alpha"], sd[s_ + "_norm.weight"]
        vg = vec * gm
        dy = a * coef[:, None] * rs[s_] * (vg - vg.mean(-1, keepdim=True) - yh[s_] * (vg * yh[s_]).mean(-1, keepdim=True))
        names = [n for n in leaf if n.startswith(s_ + "_proj.")]
        got = torch.autograd.grad(y[s_], [leaf[n] for n in names] + [xin[s_]], grad_outputs=dy)
        grads.update({L + n: v for n, v in zip(names, got)})
        return got[-1] + (1 - a) * coef[:, None] * vec
    d_kx, d_vx = stream("k", ds, k_vec, key), stream("v", pw, v_vec, ff)
    sxk, sxv = wsum(ds, key), wsum(pw, ff)
    dq_w = sxk
    if S["adapt_k"]:
        a, gm, syk = sd["k_alpha"], sd["k_norm.weight"], wsum(ds, yh["k"])
        dq_w = (1 - a) * sxk + a * gm * syk
        grads.update({L + "k_alpha": (qf * (gm * syk - sxk)).sum().reshape(1), L + "k_norm.weight": a * (qf * syk).sum(0), L + "k_norm.bias": torch.zeros(D, dtype=torch.float64)})
    if S["adapt_v"]:
        a, gm, bt, syv = sd["v_alpha"], sd["v_norm.weight"], sd["v_norm.bias"], wsum(pw, yh["v"])
        grads.update({L + "v_alpha": (dctx * (gm * syv + bt - sxv)).sum().reshape(1), L + "v_norm.weight": a * (dctx * syv).sum(0), L + "v_norm.bias": a * dctx.sum(0)})
    grads["guide_embeds"] = torch.zeros_like(g).index_add(0, torch.from_numpy(tab.win_item.astype(np.int64)), dq_w)
    if fe is not None:
        grads["frames_embed"], grads["frames_feature"] = d_kx, d_vx
    else:
        grads["frames_feature"] = d_vx if defect == "key_side_term_missing_without_fe" else d_vx + d_kx
    return grads


def bars_moved(S, got, want):
    """The largest error of any gradient in units of its bar."""
    params = {k: v.numpy() for k, v in want.items() if k.startswith(L)}
    bar = rt.bars({**params, "guide_embeds": want["guide_embeds"].numpy()})
    worst = max(float((got[k] - want[k]).abs().max()) / bar[k] for k in bar)
    splits = [n for n in S["tab"].N]
    for name in ("frames_feature", "frames_embed"):
        if name in want:
            for gi, wi in zip(got[name].split(splits), want[name].split(splits)):
                worst = max(worst, float((gi - wi).abs().max()) / ig.item_bar(wi.numpy()))
    return worst


@pytest.mark.parametrize("id", ra.CASES)
def test_the_model_of_the_step_equals_autograd(id):
    S = setup(id)
    want, got = autograd_reference(S), step_model(S)
    assert set(want) == set(got)
    moved = bars_moved(S, got, want)
    print(f"RAGGED_ADAPT_POWER {id} no defect: {moved:.3e} bars")
    assert moved < 1e-6


def applies(defect, S):
    """Every defect touches every case (a plain stream beside an adapted one takes its input gradient from the same dy step), but the last
    one: the key-side term of d frames_feature exists only without frames_embed."""
    return defect != "key_side_term_missing_without_fe" or S["fe"] is None


@pytest.mark.parametrize("defect", DEFECTS)
def test_each_planted_defect_moves_a_gradient_of_every_case(defect):
    figures = {}
    for id in ra.CASES:
        S = setup(id)
        if not applies(defect, S):
            continue
        figures[id] = bars_moved(S, step_model(S, defect), autograd_reference(S))
    assert figures, defect
    worst = min(figures, key=figures.get)
    print(f"RAGGED_ADAPT_POWER {defect}: smallest {figures[worst]:.3e} bars ({worst}); " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    assert figures[worst] >= MIN_BARS, f"{defect}: moves the gradients of {worst} by {figures[worst]:.3e} bars only"
