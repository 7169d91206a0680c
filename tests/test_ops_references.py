"""CPU checks of the float64 references in tests/ops_reference.py: each non-trivial closed form against float64 autograd or the
oracle, so that a wrong reference cannot bless a wrong kernel in tests/test_gpu_ops_small.py.  Agreement to 1e-10 (float64)."""
import math

import pytest
import torch

import ops_reference as R
from oracle import hicom_oracle as orc

TOL = 1e-10


def _maxabs(a, b):
    return float((a - b).abs().max())


@pytest.mark.parametrize("rows,N,E", [(6, 37, 24), (9, 64, 16), (1, 5, 8)])
def test_global_dx_reference_is_the_gradient_of_the_folded_global_attention(rows, N, E):
    g = torch.Generator().manual_seed(rows * 100 + N)
    qt = torch.randn(rows, E, generator=g, dtype=torch.float64)
    x = torch.randn(N, E, generator=g, dtype=torch.float64, requires_grad=True)
    cot = torch.randn(rows, E, generator=g, dtype=torch.float64)
    ctx = torch.softmax(qt @ x.t(), dim=1) @ x                        # [rows, E]: sum_n softmax_n(q~_r . x_n) x_n
    (ctx * cot).sum().backward()
    S, ml, dS, _ = R.global_attention_backward_ref(qt, x.detach(), cot)
    # padding columns beyond N must not matter to the reference either
    pad = torch.full((rows, 3), float("nan"), dtype=torch.float64)
    dx, ab, p = R.global_dx_ref(torch.cat([S, pad], 1), torch.cat([dS, pad], 1), ml, qt, cot, N)
    assert _maxabs(dx, x.grad) <= TOL
    assert bool((ab >= dx.abs() - 1e-12).all()) and _maxabs(p.sum(1), torch.ones(rows, dtype=torch.float64)) <= TOL
    dx2, _, _ = R.global_dx_ref(S, dS, ml, qt, cot, N, dx0=torch.ones(N, E, dtype=torch.float64))
    assert _maxabs(dx2, x.grad + 1) <= TOL


@pytest.mark.parametrize("which", ["both", "key", "value"])
@pytest.mark.parametrize("T,H,W,kt,ks,shared", [(4, 6, 6, 4, 3, True), (2, 4, 4, 1, 2, False)])
def test_adapt_bwd_reference_equals_autograd_through_blend_and_window_attention(T, H, W, kt, ks, shared, which):
    D, eps, scale, bias = 12, 1e-6, 0.3, 0.25
    g = torch.Generator().manual_seed(T * 10 + H)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    N = T * H * W
    win = R.window_of_token(T, H, W, kt, ks)
    nw = int(win.max()) + 1
    use_k, use_v = which in ("both", "key"), which in ("both", "value")
    kx, vx, ky, vy = rnd(N, D), rnd(N, D), rnd(N, D) * 1.5 + 0.3, rnd(N, D)
    kg, kb, vg, vb = 1 + 0.1 * rnd(D), 0.1 * rnd(D), 1 + 0.1 * rnd(D), 0.1 * rnd(D)
    ak, av = 0.4, 0.7
    q = (rnd(1, D).expand(nw, D) if shared else rnd(nw, D)).clone().requires_grad_(True)
    dctx = rnd(nw, D)
    # reference-style forward: materialised blends (leaves of the graph), window softmax, context
    ln = lambda y, ga, be: torch.nn.functional.layer_norm(y, (D,), ga, be, eps)
    K = ((1 - ak) * kx + ak * ln(ky, kg, kb)) if use_k else kx.clone()
    V = ((1 - av) * vx + av * ln(vy, vg, vb)) if use_v else vx.clone()
    K.requires_grad_(True); V.requires_grad_(True)
    loss = 0
    for w in range(nw):
        m = win == w
        p = torch.softmax(K[m] @ q[w] * scale + bias, 0)
        loss = loss + (p @ V[m]) @ dctx[w]
    loss.backward()
    out, ab = R.adapt_bwd_ref(kx, ky if use_k else None, kg, kb, ak, vx, vy if use_v else None, vg, vb, av, win, nw, q.detach(),
                              scale, bias, dctx, eps)
    assert _maxabs(out["ds"][:, None] * q.detach()[win], K.grad) <= TOL          # d K_n = ds_n q_w
    assert _maxabs(out["pw"][:, None] * dctx[win], V.grad) <= TOL                # d V_n = pw_n dctx_w
    dq = ((1 - ak) * out["sxk"] + ak * kg * out["syk"]) if use_k else out["sxk"]
    assert _maxabs(dq, q.grad) <= TOL                                            # dq_w = (1 - a_k) sxk_w + a_k gamma_k syk_w
    # sxv / syv: the value-side weighted sums reproduce the context: ctx = (1 - a_v) sxv + a_v (gamma_v syv + beta_v)
    ctx = torch.stack([torch.softmax(K[win == w].detach() @ q[w].detach() * scale + bias, 0) @ V[win == w].detach() for w in range(nw)])
    got = ((1 - av) * out["sxv"] + av * (vg * out["syv"] + vb)) if use_v else out["sxv"]
    assert _maxabs(got, ctx) <= TOL
    assert ("syk" in out) == use_k and ("syv" in out) == use_v
    assert all(bool((ab[k] >= out[k].abs() - 1e-12).all()) for k in out if k in ab)


def test_adapt_dy_reference_equals_autograd_through_the_layernorm_blend():
    g = torch.Generator().manual_seed(3)
    N, D, eps, alpha = 9, 16, 1e-6, 0.4
    y = torch.randn(N, D, generator=g, dtype=torch.float64, requires_grad=True)
    gamma, vec, coef = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((D,), (N, D), (N,)))
    blend = alpha * torch.nn.functional.layer_norm(y, (D,), gamma, None, eps)
    (blend * coef[:, None] * vec).sum().backward()
    dy, r1, ab = R.adapt_dy_ref(y.detach(), gamma, vec, coef, alpha, eps)
    assert _maxabs(dy, y.grad) <= TOL and bool((ab >= dy.abs() - 1e-12).all())
    assert _maxabs(r1, (1 - alpha) * coef[:, None] * vec) == 0.0


def test_gelu_references_equal_torch_and_autograd():
    h = torch.linspace(-12, 12, 481, dtype=torch.float64, requires_grad=True)
    want = torch.nn.functional.gelu(h)
    want.sum().backward()
    assert _maxabs(R.gelu_ref(h.detach())[0], want.detach()) <= 1e-14
    assert _maxabs(R.gelu_grad_ref(h.detach())[0], h.grad) <= 1e-14


def test_ln_blend_l2norm_and_small_mha_references_equal_torch():
    g = torch.Generator().manual_seed(5)
    x, src = torch.randn(7, 24, generator=g, dtype=torch.float64), torch.randn(7, 24, generator=g, dtype=torch.float64)
    gamma, beta = torch.randn(24, generator=g, dtype=torch.float64), torch.randn(24, generator=g, dtype=torch.float64)
    ln = torch.nn.functional.layer_norm(x, (24,), gamma, beta, 1e-6)
    assert _maxabs(R.ln_blend_ref(x, gamma, beta)[0], ln) <= 1e-12
    assert _maxabs(R.ln_blend_ref(x, gamma, beta, src, 0.3)[0], 0.7 * src + 0.3 * ln) <= 1e-12
    assert _maxabs(R.l2norm_ref(x), torch.nn.functional.normalize(x, dim=1, eps=0)) <= 1e-14
    q, k, v = (torch.randn(n, 24, generator=g, dtype=torch.float64) for n in (5, 9, 9))
    mha = torch.nn.functional.scaled_dot_product_attention
    want = mha(*(t.reshape(-1, 3, 8).permute(1, 0, 2) for t in (q, k, v)), scale=2.5).permute(1, 0, 2).reshape(5, 24)
    assert _maxabs(R.small_mha_ref(q, k, v, 3, 2.5)[0], want) <= 1e-12


def test_clip_attention_reference_equals_the_oracle_clip_scale_global_stage():
    """Folded form (normalised q_proj output folded through k_proj, key-bias constant, per-token inverse key norms) against
    oracle/hicom_oracle.py::mha with logit_scale: its scores to 1e-10; its output through v_proj / out_proj to 1e-6 only, because the
    oracle takes the softmax in fp32 (2^-24 per weight) as the reference module does."""
    g = torch.Generator().manual_seed(11)
    E, nh, nq, N = 24, 3, 2, 40
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    sd = {f"a.{p}.{k}": rnd(*s) * (0.3 if k == "weight" else 0.1) for p in ("q_proj", "k_proj", "v_proj", "out_proj")
          for k, s in (("weight", (E, E)), ("bias", (E,)))}
    query, x = rnd(nq, E), rnd(N, E)
    ls, lb = torch.tensor(2.3, dtype=torch.float64), torch.tensor(-1.5, dtype=torch.float64)
    want_out, want_scores = orc.mha(query, x, x, sd, "a", nh, ls, lb, return_scores=True)           # scores [nh, nq, N]
    scale = math.exp(float(ls))
    qp = query @ sd["a.q_proj.weight"].t() + sd["a.q_proj.bias"]
    qhat, c, _ = R.clip_query_prep_ref(qp, sd["a.k_proj.bias"], nh, scale)
    qt = R.fold_query_ref(qhat, sd["a.k_proj.weight"], nh, scale)
    kproj = x @ sd["a.k_proj.weight"].t() + sd["a.k_proj.bias"]
    # the key norms as the product forms them: per-64-column partial sums of squares, then hicom_inv_norm_fwd
    ssq = torch.stack([(kproj[:, :16] ** 2).sum(1), (kproj[:, 16:] ** 2).sum(1)])
    inv = R.inv_norm_ref(ssq)
    S, ctx, ab, _ = R.clip_attention_ref(qt, x, inv, c)
    assert _maxabs(S.reshape(nq, nh, N).permute(1, 0, 2) + lb, want_scores) <= TOL          # (logit_bias: a shift softmax cancels)
    assert bool((ab >= S.abs() - 1e-12).all())
    hd = E // nh
    wv, bv = sd["a.v_proj.weight"], sd["a.v_proj.bias"]
    o = torch.cat([ctx.reshape(nq, nh, E)[:, h] @ wv[h * hd:(h + 1) * hd].t() + bv[h * hd:(h + 1) * hd] for h in range(nh)], 1)
    out = o @ sd["a.out_proj.weight"].t() + sd["a.out_proj.bias"]
    assert _maxabs(out, want_out) <= 1e-6


def test_clip_attention_reference_positional_terms():
    """With a score-side table pos_a = q . pe^T and the value-side rows pe, the folded reference equals plain attention over x + pos."""
    g = torch.Generator().manual_seed(12)
    E, T, H, W, rows = 8, 2, 3, 2, 5
    N = T * H * W
    q, x, pe = (torch.randn(n, E, generator=g, dtype=torch.float64) for n in (rows, N, T + 1 + H + W))
    inv, c = torch.rand(N, generator=g, dtype=torch.float64) + 0.5, torch.randn(rows, generator=g, dtype=torch.float64)
    t, y, xx = R.token_axes(N, H, W)
    xp = x + pe[t] + pe[T + 1 + y] + pe[T + 1 + H + xx]
    S, ctx, _, _ = R.clip_attention_ref(q, x, inv, c, q @ pe.t(), pe, H, W, 0, T + 1, T + 1 + H)
    want_S = (q @ xp.t() + c[:, None]) * inv[None, :]
    assert _maxabs(S, want_S) <= 1e-12 and _maxabs(ctx, torch.softmax(want_S, 1) @ xp) <= 1e-12


@pytest.mark.parametrize("T,H,W,rows,t0", [(3, 2, 4, 5, 0), (2, 3, 3, 1, 2), (1, 4, 2, 3, 1)])
def test_global_stream_references_equal_autograd_through_attention_over_x_plus_pos(T, H, W, rows, t0):
    """f = sum_r ctx_r . g_r with ctx_r = sum_n softmax_n(qt_r . (x_n + pos_n)) (x_n + pos_n): the forward reference restates it, and
    the backward reference's outputs assemble its gradients: d f / d qt = sum_n dS x_n + marginals(dS) @ PE, d f / d S = dS, with the
    score-side tables pos_a = qt PE^T, pos_b = g PE^T and delta_r = g_r . ctx_r."""
    gen = torch.Generator().manual_seed(T * 100 + H * 10 + W)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    E, N = 12, T * H * W
    cap = t0 + T + 2
    y0, x0 = cap, cap + H
    pe, x, g = rnd(cap + H + W + 3, E), rnd(N, E), rnd(rows, E)
    qt = (0.6 * rnd(rows, E)).requires_grad_(True)
    t, y, xx = R.token_axes(N, H, W)
    xp = x + pe[t0 + t] + pe[y0 + y] + pe[x0 + xx]                       # attention over x + pos, written out
    S_plain = qt @ xp.t()
    ctx_plain = torch.softmax(S_plain, 1) @ xp
    (dqt,) = torch.autograd.grad((ctx_plain * g).sum(), qt)
    qd = qt.detach()
    fw = R.global_stream_ref(qd, x, qd @ pe.t(), pe, H, W, t0, y0, x0)
    assert _maxabs(fw["S"], S_plain.detach()) <= TOL and _maxabs(fw["ctx"], ctx_plain.detach()) <= TOL
    assert _maxabs(fw["lse"], torch.logsumexp(S_plain.detach(), 1)) <= TOL
    assert _maxabs(fw["ctx"] - fw["ctx_x"], torch.softmax(S_plain.detach(), 1) @ (xp - x)) <= TOL      # the positional part alone
    assert bool((fw["S_ab"] >= fw["S"].abs() - 1e-12).all()) and bool((fw["ctx_ab"] >= fw["ctx"].abs() - 1e-12).all())
    for m in fw["marg"]:
        assert _maxabs(m.sum(1), torch.ones(rows, dtype=torch.float64)) <= TOL
    ml = torch.stack([fw["M"], fw["L"]], 1)
    delta = (g * fw["ctx"]).sum(1)
    pad = torch.full((rows, 5), float("nan"), dtype=torch.float64)      # columns beyond N do not matter
    bw = R.global_stream_bwd_ref(g, x, g @ pe.t(), torch.cat([fw["S"], pad], 1), ml, delta, H, W, t0, y0, x0)
    mt, my, mx = bw["marg"]
    assert _maxabs(bw["dSx"] + mt @ pe[t0:t0 + T] + my @ pe[y0:y0 + H] + mx @ pe[x0:x0 + W], dqt) <= TOL
    # the gradient with respect to the logits themselves
    S_leaf = fw["S"].clone().requires_grad_(True)
    (dS,) = torch.autograd.grad(((torch.softmax(S_leaf, 1) @ xp) * g).sum(), S_leaf)
    assert _maxabs(bw["dS"], dS) <= TOL and float(bw["dS"].abs().max()) > 1e-3
    assert _maxabs(bw["dS"].sum(1), torch.zeros(rows, dtype=torch.float64)) <= TOL          # the true delta: every row of dS sums to zero
    assert bool((bw["dS_ab"] >= bw["dS"].abs() - 1e-12).all()) and bool((bw["dSx_ab"] >= bw["dSx"].abs() - 1e-12).all())
    # without the positional tables both references are the plain folded attention of global_attention_backward_ref
    S0, ml0, dS0, delta0 = R.global_attention_backward_ref(qd, x, g)
    f0 = R.global_stream_ref(qd, x)
    assert _maxabs(f0["S"], S0) <= TOL and _maxabs(torch.stack([f0["M"], f0["L"]], 1), ml0) <= TOL and "marg" not in f0
    b0 = R.global_stream_bwd_ref(g, x, None, S0, ml0, delta0)
    assert _maxabs(b0["dS"], dS0) <= TOL and "marg" not in b0


def test_window_index_and_sequential_sum():
    win = R.window_of_token(4, 4, 6, 2, 2)
    assert int(win.max()) + 1 == 2 * 2 * 3 and bool((torch.bincount(win) == 8).all())
    assert int(win[(1 * 4 + 3) * 6 + 5]) == (0 * 2 + 1) * 3 + 2 and int(win[(2 * 4 + 0) * 6 + 0]) == 6
    parts = torch.tensor([[1e8], [1.0], [-1e8], [1.0]], dtype=torch.float32)
    assert float(R.sequential_f32_sum(parts)[0]) == 1.0            # (1e8 + 1) rounds to 1e8 in fp32: order is visible


# ---- hicom_fused_stream_fwd / hicom_query_prep_fwd: the references of tests/test_gpu_fused_ring.py ---------------------------
from types import SimpleNamespace

import fused_ring_inputs as G                                            # (the inputs, limits and tolerances of tests/test_gpu_fused_ring.py)


def _small_ring(seed, rows=3, with_pos=True):
    T, H, W, kt, ks, E = 4, 4, 6, 2, 2, 24
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    N, P = T * H * W, T + H + W + 5
    a = dict(ff=rnd(N, E), fe=rnd(N, E), q_local=rnd(E), qt=0.4 * rnd(rows, E), pos_a=rnd(rows, P) if with_pos else None,
             pe=rnd(P, E) if with_pos else None, t0i=2, y0i=2 + T + 1, x0i=2 + T + 1 + H)
    return (T, H, W, kt, ks, E), a


def _ring(shape, a, nparts, **kw):
    T, H, W, kt, ks, _ = shape
    return R.fused_ring_ref(a["ff"], T, H, W, kt, ks, a["q_local"], 0.3, 0.7, a["qt"], fe=a["fe"], pos_a=a["pos_a"], pe=a["pe"], t0i=a["t0i"],
                            y0i=a["y0i"], x0i=a["x0i"], nparts=nparts, **kw)


@pytest.mark.parametrize("nparts", [1, 2, 4, 12])
def test_fused_ring_reference_against_explicit_loops_and_the_direct_softmax(nparts):
    shape, a = _small_ring(nparts)
    T, H, W, kt, ks, E = shape
    o = _ring(shape, a, nparts)
    idx = orc.window_token_index(T, H, W, kt, ks)                        # the oracle's windows: [NW, wsz] token ids
    NW = idx.shape[0]
    assert o["NW"] == NW
    pos = lambda n: (a["t0i"] + n // (H * W), a["y0i"] + (n // W) % H, a["x0i"] + n % W)
    S = torch.empty(a["qt"].shape[0], T * H * W, dtype=torch.float64)
    val = torch.empty(T * H * W, E, dtype=torch.float64)
    for n in range(T * H * W):
        pt, py, px = pos(n)
        S[:, n] = a["qt"] @ a["ff"][n] + a["pos_a"][:, pt] + a["pos_a"][:, py] + a["pos_a"][:, px]
        val[n] = a["ff"][n] + a["pe"][pt] + a["pe"][py] + a["pe"][px]
    assert _maxabs(o["S"], S) <= TOL
    for w in range(NW):
        p = torch.softmax(0.3 * (a["fe"][idx[w]] @ a["q_local"]) + 0.7, 0)
        assert _maxabs(o["ctx_local"][w], p @ a["ff"][idx[w]]) <= TOL
    wpw = -(-NW // nparts)
    for p_ in range(nparts):
        toks = idx[p_ * wpw:min((p_ + 1) * wpw, NW)].reshape(-1)
        assert sorted(toks.tolist()) == sorted(o["part_tokens"][p_].tolist())
        assert _maxabs(o["lse"][p_], torch.logsumexp(S[:, toks], 1)) <= TOL
        pw = torch.softmax(S[:, toks], 1)
        assert _maxabs(o["part_ctx"][p_], pw @ val[toks]) <= TOL
        # marginals x pe rows = the positional part of the context
        pe_sel = torch.cat([a["pe"][a["t0i"]:a["t0i"] + T], a["pe"][a["y0i"]:a["y0i"] + H], a["pe"][a["x0i"]:a["x0i"] + W]])
        assert _maxabs(o["marg"][p_] @ pe_sel, pw @ (val[toks] - a["ff"][toks])) <= TOL
        assert _maxabs(o["marg"][p_][:, :T].sum(1), torch.ones(S.shape[0], dtype=torch.float64)) <= TOL
    assert _maxabs(o["merged"], torch.softmax(S, 1) @ val) <= TOL       # merged over the partitions = the direct softmax over all tokens
    assert bool((o["merged_ab"] >= o["merged"].abs() - 1e-12).all()) and bool((o["part_ctx_ab"] >= o["part_ctx"].abs() - 1e-12).all())
    # precomputed logits in place of frames_embed
    o2 = R.fused_ring_ref(a["ff"], T, H, W, kt, ks, a["q_local"], 0.3, 0.7, a["qt"], llog=a["fe"] @ a["q_local"], nparts=nparts)
    assert _maxabs(o2["ctx_local"], o["ctx_local"]) <= TOL


def test_query_prep_reference_against_the_unfused_chain():
    g = torch.Generator().manual_seed(4)
    E, nh, P, hidden = 36, 3, 7, 10
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    guide, wq, bq, wk, kpe, gw0, gb0, bo = rnd(E), rnd(E, E), rnd(E), rnd(E, E), rnd(E, P), rnd(hidden, E), rnd(hidden), rnd(E)
    (qt, pa, r0), (qt_ab, pa_ab, r0_ab) = R.query_prep_ref(guide, wq, bq, wk, kpe, nh, 0.5, gw0, gb0, bo)
    qp = (wq @ guide + bq)[None, :]
    assert _maxabs(qt, R.fold_query_ref(qp, wk, nh, 0.5)) <= TOL
    hd = E // nh
    for h in range(nh):
        assert _maxabs(pa[h], 0.5 * qp[0, h * hd:(h + 1) * hd] @ kpe[h * hd:(h + 1) * hd]) <= TOL
    assert _maxabs(r0, gw0 @ (bo + guide) + gb0) <= TOL
    assert bool((qt_ab >= qt.abs() - 1e-12).all()) and bool((pa_ab >= pa.abs() - 1e-12).all()) and bool((r0_ab >= r0.abs() - 1e-12).all())


def test_ring_limits_restatement_matches_the_issue_list():
    """Every listed shape has valid partitions for rows 1 / 9 / 12 except the LDS overflows; nparts = 1 is mostly a frame-span refusal."""
    assert all(G.valid_nparts(s, r, f) for s in G.SHAPES for r in (1, 2, 9) for f in G.FORMS)
    assert sum(G.ring_refusal(*s, 9, 1, False) is not None for s in G.SHAPES) >= 6
    assert not G.valid_nparts((4, 36, 36, 4, 3), 9, "logits") and G.valid_nparts((4, 36, 36, 4, 3), 9, "bf16")


# Defect sensitivity: each defect is planted into the reference on input sets of the GPU test; on at least one set it has to differ
# from the reference by >= 2 x the GPU test's own tolerance (a kernel with the defect then misses the bound by >= 1 x of it whatever
# its legitimate rounding does).  A non-finite result counts: check() asserts finiteness first.
_SETS = [(fam, form, shape, rows) for fam in ("plain", "flat", "offsets", "extremes") for form in ("bf16", "f16")
         for shape, rows in (((8, 6, 6, 4, 3), 9), ((12, 9, 6, 4, 3), 12), ((4, 4, 8, 1, 4), 9))]
assert all((fam, shape, rows, form) in G.FAMILY_CASES or (fam == "plain" and (shape, rows, form) in G.CASES) for fam, form, shape, rows in _SETS)


def _ratio(i, ref, bounds, bad, keys):
    worst = 0.0
    for k in keys:
        r = ((bad[k] - ref[k]).abs() / bounds[k])
        r = torch.nan_to_num(r, nan=math.inf)
        worst = max(worst, float(r.max()))
    return worst


def _x_neighbour(i):
    T, H, W, kt, ks = i.shape
    win = R.window_of_token(*i.shape).clone()
    x = torch.arange(T * H * W) % W
    win[x == ks - 1] += 1                                                # the last column of the first window column goes to its x neighbour
    return dict(win=win)


def _drop_last_window(i, nparts):
    pw = R.ring_partitions(G.n_windows(*i.shape), nparts).clone()
    for p in range(nparts):
        own = torch.nonzero(pw == p)[:, 0]
        if own.numel() > 1:
            pw[own[-1]] = -1
    return dict(part_of_window=pw)


def _padded_tables(i):
    """pos_a / pe with NaN slots behind the last one: a swapped base may look past the table (on the device: whatever lies there)."""
    pad = max(i.shape[1:3])
    pe = R.up(i.pe_hi) + R.up(i.pe_lo)
    nan = lambda r, c: torch.full((r, c), float("nan"), dtype=torch.float64)
    return dict(pos_a=torch.cat([R.up(i.pos_a[:i.rows]), nan(i.rows, pad)], 1), pe=torch.cat([pe, nan(pad, pe.shape[1])], 0))


_LOCAL, _GLOBAL = ("ctx_local",), ("lse", "part_ctx", "merged")
DEFECTS = {
    "x_neighbour_column": (lambda i, n: _x_neighbour(i), _LOCAL + _GLOBAL, None),
    "partition_loses_last_window": (_drop_last_window, _GLOBAL, None),
    "t_index0_ignored": (lambda i, n: dict(t0i=0), _GLOBAL, None),
    "y_x_bases_swapped": (lambda i, n: dict(y0i=i.x0i, x0i=i.y0i, **_padded_tables(i)), _GLOBAL, None),
    "value_pe_omitted": (lambda i, n: dict(value_pe=False), _GLOBAL, None),
    "pe_lo_dropped": (lambda i, n: dict(pe=R.up(i.pe_hi)), _GLOBAL, "bf16"),
    "local_weight_lo_dropped": (lambda i, n: dict(local_p_map=lambda e: e.bfloat16().double()), _LOCAL, "bf16"),
    "global_row_as_local_query": (lambda i, n: dict(q_local_override=0), _LOCAL, None),
    "fp16_query_without_row_scale": (lambda i, n: dict(qt_override=i.qt.clamp(-65504, 65504).half().double()), _GLOBAL, "f16"),
}


def _defect_reference(i, nparts, over):
    over = dict(over)
    j = SimpleNamespace(**vars(i))
    if "q_local_override" in over:
        j.q_local = i.qt[over.pop("q_local_override")]
    if "qt_override" in over:
        j.qt = over.pop("qt_override")
    return G.ring_reference(j, nparts, **over)



def _sweep(name):
    make, keys, only_form = DEFECTS[name]
    best = (0.0, None)
    for fam, form, shape, rows in _SETS:
        if only_form and form != only_form:
            continue
        i = G.ring_inputs(fam, form, shape, rows)
        for nparts in G.valid_nparts(shape, rows, form):
            ref = G.ring_reference(i, nparts)
            b = G.ring_bounds(i, ref)
            r = _ratio(i, ref, b, _defect_reference(i, nparts, make(i, nparts)), keys)
            if r > best[0]:
                best = (r, (fam, form, shape, rows, nparts))
    print(f"RING_DEFECT {name} ratio={best[0]:.3e} on {best[1]}")
    return best[0]


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_ring_defect_exceeds_twice_the_gpu_tolerance(name):
    assert _sweep(name) >= 2.0


def test_ring_defect_ctx_lo_dropped_exceeds_twice_the_plane_tolerance():
    worst = 0.0
    for fam, form, shape, rows in _SETS:
        i = G.ring_inputs(fam, form, shape, rows)
        ref = G.ring_reference(i, G.n_windows(*shape))
        tol = G.ring_bounds(i, ref)["ctx_local"] + G.BF16_PLANES * ref["ctx_local"].abs()
        worst = max(worst, float(((ref["ctx_local"].bfloat16().double() - ref["ctx_local"]).abs() / tol).max()))
    print(f"RING_DEFECT ctx_lo_dropped ratio={worst:.3e}")
    assert worst >= 2.0


def test_ring_defect_query_lo_plane_dropped_is_reported():
    """The lo plane of the bf16 global queries (2^-9 of q) against the worst-case 2 E-term fp32 bound on the same logits (2^-11.8 of
    sum |q||x|): reachable only with coherent inputs (family `coherent`).  Measured ratio: 10.2 with the coherent
    inputs (printed below), so it is asserted at 2 like the required defects."""
    best = 0.0
    for shape, rows in (((8, 6, 6, 4, 3), 9), ((12, 9, 6, 4, 3), 12)):
        i = G.ring_inputs("coherent", "bf16", shape, rows)
        for nparts in G.valid_nparts(shape, rows, "bf16"):
            ref = G.ring_reference(i, nparts)
            b = G.ring_bounds(i, ref)
            bad = _defect_reference(i, nparts, dict(qt_override=R.up(i.q_hi[:rows])))
            best = max(best, _ratio(i, ref, b, bad, _GLOBAL))
    print(f"RING_DEFECT query_lo_dropped ratio={best:.3e}")
    assert best >= 2.0


# ---- dense 16-bit GEMM references ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,H,W,N,offs", [(3, 4, 5, 136, (0, 3, 7)), (2, 3, 7, 132, (5, 9, 14)), (1, 6, 6, 64, (0, 1, 7))])
def test_dense16_reference_is_the_projection_of_tokens_plus_a_separable_positional_embedding(T, H, W, N, offs):
    """The identity the clip-scale global stage rests on (csrc/dense16.hip, DenseParams::tab): with a separable positional embedding
    pos(m) = PE[t0 + t] + PE[y0 + y] + PE[x0 + x] and tab = PE W^T, (x + pos) W^T + b = x W^T + tab[t0 + t] + tab[y0 + y] + tab[x0 + x] + b,
    and the per-slice sums of squares add up to the squared row norm of that product."""
    g = torch.Generator().manual_seed(T * 100 + N)
    M, K, P, ld = T * H * W, 24, 24, N + 8
    x, w, b = (torch.randn(s, dtype=torch.float64, generator=g) for s in ((M, K + 5), (N, K), (N,)))
    pe = torch.randn(P, K, dtype=torch.float64, generator=g)
    tab = torch.full((P, ld), float("nan"), dtype=torch.float64)             # a pitch above N: the pad columns are never read
    tab[:, :N] = pe @ w.t()
    t0, y0, x0 = offs
    m = torch.arange(M)
    pos = pe[t0 + m // (H * W)] + pe[y0 + (m // W) % H] + pe[x0 + m % W]
    direct = (x[:, :K] + pos) @ w.t() + b
    res, vec = torch.randn(M, N, dtype=torch.float64, generator=g), torch.randn(N, dtype=torch.float64, generator=g)
    o = R.dense16_ref(x, w, b, K=K, tab=tab, geom=(H, W, t0, y0, x0), act="gelu", res=res, dot_vec=vec)
    assert _maxabs(o["pre"], direct) <= 1e-12
    assert o["ssq"].shape == ((N + 63) // 64, M) and _maxabs(o["ssq"].sum(0), (direct ** 2).sum(1)) <= 1e-12 * float((direct ** 2).sum(1).max())
    gelu = torch.nn.functional.gelu(direct)
    assert _maxabs(o["val"], gelu) <= 1e-12 and _maxabs(o["y"], gelu + res) <= 1e-12
    assert _maxabs(o["rdot"].sum(0), (gelu + res) @ vec) <= 1e-11
    plain = R.dense16_ref(x, w, None, K=K, act="gelu_tanh")
    assert _maxabs(plain["pre"], x[:, :K] @ w.t()) <= 1e-12 and _maxabs(plain["y"], torch.nn.functional.gelu(plain["pre"], approximate="tanh")) <= 1e-12
    assert "rdot" not in plain


@pytest.mark.parametrize("N", [136, 132])
def test_dense16_reference_slice_boundaries_by_hand_built_columns(N):
    """One row, a = e_0, w[n, 0] = the column's value: columns 0 .. 63 carry 1, 64 .. 127 carry 2, the last N - 128 carry 3."""
    a = torch.zeros(1, 8, dtype=torch.float64)
    a[0, 0] = 1.0
    w = torch.zeros(N, 8, dtype=torch.float64)
    w[:64, 0], w[64:128, 0], w[128:, 0] = 1.0, 2.0, 3.0
    vec = torch.ones(N, dtype=torch.float64)
    o = R.dense16_ref(a, w, None, K=8, dot_vec=vec)
    assert o["ssq"].shape == (3, 1) and o["ssq"][:, 0].tolist() == [64.0, 256.0, 9.0 * (N - 128)]
    assert o["rdot"][:, 0].tolist() == [64.0, 128.0, 3.0 * (N - 128)]
    # one column at a time: column n lands in slice n // 64 and nowhere else
    for n in (0, 63, 64, 127, 128, N - 1):
        w1 = torch.zeros(N, 8, dtype=torch.float64)
        w1[n, 0] = 5.0
        s = R.dense16_ref(a, w1, None, K=8)["ssq"][:, 0]
        assert float(s[n // 64]) == 25.0 and float(s.sum()) == 25.0
    # the planted slice faults do what they say
    b = torch.zeros(N, dtype=torch.float64)
    b[N - 1] = 0.5
    good, pad = R.dense16_ref(a, w, b, K=8), R.dense16_ref(a, w, b, K=8, pad_cols_in_ssq=True)
    assert float(pad["ssq"][2, 0] - good["ssq"][2, 0]) == (192 - N) * 0.25 and torch.equal(pad["ssq"][:2], good["ssq"][:2])
    assert R.dense16_ref(a, w, None, K=8, dot_vec=vec, slices_swapped=True)["ssq"][:, 0].tolist() == [256.0, 64.0, 9.0 * (N - 128)]


def test_dense16_tn_reference_and_slice_sums():
    g = torch.Generator().manual_seed(9)
    a, b = torch.randn(11, 16, dtype=torch.float64, generator=g), torch.randn(11, 24, dtype=torch.float64, generator=g)
    want = sum(torch.outer(a[k, :8], b[k, :16]) for k in range(11))
    assert _maxabs(R.dense16_tn_ref(a, b, 8, 16), want) <= 1e-13
    assert _maxabs(R.dense16_tn_ref(a, b, 8, 16, k_rows=slice(0, 4)), sum(torch.outer(a[k, :8], b[k, :16]) for k in range(4))) <= 1e-13
    v = torch.arange(2 * 70, dtype=torch.float64).reshape(2, 70)
    assert R.slice_sums(v).tolist() == [[float(v[0, :64].sum()), float(v[1, :64].sum())], [float(v[0, 64:].sum()), float(v[1, 64:].sum())]]


# ---- window attention and the pooled queries (tests/test_gpu_window_attn.py) --------------------------------------------------
def _gathered_window_attention(key, value, q, tok, scale, bias, l2norm_key):
    """Autograd's view: gather the windows' rows, softmax per window, contexts; returns (ctx, s)."""
    K, V = key[tok], value[tok]
    if l2norm_key:
        K = K / K.norm(dim=2, keepdim=True)
    s = scale * torch.einsum("wid,wd->wi", K, q) + bias
    return torch.einsum("wi,wid->wd", torch.softmax(s, 1), V), s


@pytest.mark.parametrize("l2norm_key", [False, True])
@pytest.mark.parametrize("geom,shared,value_is_key", [((3, 7, 5, 2, 3), True, False), ((3, 7, 5, 2, 3), False, True),
                                                      ((4, 4, 6, 2, 2), False, False), ((4, 4, 6, 2, 2), True, True)])
def test_window_attention_references_equal_autograd_through_a_gathered_window_softmax(geom, shared, value_is_key, l2norm_key):
    """One overlapping geometry (every axis) and one exact one: contexts, dq, dkey, dvalue (also with the key-side gradient added) and
    dls against float64 autograd, <= 1e-12 relative."""
    T, H, W, kt, ks = geom
    D, bias = 12, 0.25
    g = torch.Generator().manual_seed(T * 10 + H + int(l2norm_key))
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    N = T * H * W
    tok, idx = R.window_tokens(*geom)
    NW = tok.shape[0]
    # the restated geometry: every token covered, shared planes only where an axis is not divided
    assert sorted(set(tok.reshape(-1).tolist())) == list(range(N))
    assert (tok.numel() == N) == (T % kt == 0 and H % ks == 0 and W % ks == 0)
    key, q0, dctx = rnd(N, D).requires_grad_(True), rnd(1 if shared else NW, D), rnd(NW, D)
    value = key if value_is_key else rnd(N, D).requires_grad_(True)
    q = q0.expand(NW, D).clone().requires_grad_(True)
    ls = torch.tensor(math.log(3.0) if l2norm_key else math.log(0.3), dtype=torch.float64, requires_grad=True)
    ctx, s = _gathered_window_attention(key, value, q, tok, torch.exp(ls), bias, l2norm_key)
    (ctx * dctx).sum().backward()
    scale = float(torch.exp(ls.detach()))
    rel = lambda a, b: _maxabs(a, b) / max(1.0, float(b.abs().max()))
    fw = R.window_attention_ref(key.detach(), value.detach(), q.detach(), geom, scale, bias, l2norm=1 if l2norm_key else 0)
    assert rel(fw["ctx"], ctx.detach()) <= 1e-12 and rel(fw["s"], s.detach()) <= 1e-12
    assert bool((fw["s_ab"] + abs(bias) >= fw["s"].abs() - 1e-12).all()) and bool((fw["ctx_ab"] >= fw["ctx"].abs() - 1e-12).all())
    bw = R.window_attention_bwd_ref(key.detach(), value.detach(), q.detach(), dctx, geom, scale, bias, l2norm_key=l2norm_key,
                                    value_is_key=value_is_key)
    assert rel(bw["dq"], q.grad) <= 1e-12
    assert rel(bw["dls"].sum(), ls.grad) <= 1e-12                      # d s / d ls = s - bias, summed over the windows
    if value_is_key:
        assert rel(bw["dvalue"], key.grad) <= 1e-12                    # the key-side gradient of the same rows is added in
    else:
        assert rel(bw["dkey"], key.grad) <= 1e-12 and rel(bw["dvalue"], value.grad) <= 1e-12
    # the contribution list sums to the outputs, one launch for an exact partition, parity classes otherwise
    exact = tok.numel() == N
    assert len(bw["steps"]) == (1 if exact else 8)
    tot = torch.zeros(N, D, dtype=torch.float64)
    for st in bw["steps"]:
        tot.index_add_(0, st["tok"], st["dk"])
    assert _maxabs(tot, bw["dkey"]) <= 1e-12
    # the forward's other l2norm bit and the planted switches do what they say
    f2 = R.window_attention_ref(key.detach(), value.detach(), q.detach(), geom, scale, bias, l2norm=2)
    qn = q.detach() / q.detach().norm(dim=1, keepdim=True)
    assert rel(f2["ctx"], R.window_attention_ref(key.detach(), value.detach(), qn, geom, scale, bias)["ctx"]) <= 1e-12
    assert rel(R.window_attention_ref(key.detach(), value.detach(), q.detach(), geom, scale, bias + 95.0, l2norm=int(l2norm_key))["ctx"],
               fw["ctx"]) <= 1e-9                                       # invariant to the bias
    lost = R.window_attention_ref(key.detach(), value.detach(), q.detach(), geom, scale, bias, l2norm=int(l2norm_key), lost=(0,))
    assert float(lost["p"][:, 0].abs().max()) == 0.0 and _maxabs(lost["p"].sum(1), torch.ones(NW, dtype=torch.float64)) <= 1e-12
    lim = R.window_attention_ref(key.detach(), value.detach(), q.detach(), geom, scale, bias, l2norm=int(l2norm_key), stats_limit=5)
    assert _maxabs(lim["p"][:, :5].sum(1), torch.ones(NW, dtype=torch.float64)) <= 1e-12 and float(lim["p"].sum(1).min()) > 1.0
    if not exact:
        assert not torch.equal(R.window_tokens(*geom, wrong_overlap=True)[0], tok)


def test_window_geometry_restated():
    assert R.window_axis(7, 3) == (3, 3, 1) and R.window_axis_starts(7, 3) == [0, 2, 4]
    assert R.window_axis(8, 3) == (3, 3, 2) and R.window_axis_starts(8, 3) == [0, 3, 5]
    assert R.window_axis(7, 4) == (4, 2, 1) and R.window_axis_starts(7, 4) == [0, 3]
    assert R.window_axis_starts(7, 3, wrong_overlap=True) == [0, 3, 5]
    assert R.window_axis(6, 3) == (3, 2, 2) and R.window_axis(2, 3) == (2, 1, 1)
    tok, idx = R.window_tokens(2, 4, 4, 1, 2)
    assert tok[0].tolist() == [0, 1, 4, 5] and tok[1].tolist() == [2, 3, 6, 7] and tok[4].tolist() == [16, 17, 20, 21]
    assert idx[5].tolist() == [1, 0, 1]
    assert torch.equal(R.window_of_token(2, 4, 4, 1, 2)[tok], torch.arange(8)[:, None].expand(8, 4))
    cls = R.window_launch_classes(7, 7, 5, 4, 3)
    assert len(cls) == 8 and sorted(torch.cat(cls).tolist()) == list(range(12)) and R.window_launch_classes(8, 6, 6, 4, 3) is None
    assert [c.tolist() for c in R.window_launch_classes(4, 8, 3, 4, 3)] == [[0, 2], [1]]            # only y overlaps: classes 0 and 2


@pytest.mark.parametrize("shape,out", [((7, 7, 5), (2, 3, 2)), ((4, 27, 27), (1, 9, 9)), ((8, 6, 6), (8, 6, 6)), ((1, 6, 6), (1, 2, 2)),
                                       ((5, 3, 2), (2, 1, 1))])
def test_trilinear_pool_reference_equals_torch_interpolate(shape, out):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, 8, generator=g, dtype=torch.float64)
    want = torch.nn.functional.interpolate(x.permute(3, 0, 1, 2)[None], size=out, mode="trilinear", align_corners=False)[0].permute(1, 2, 3, 0)
    got, ab, slopes = R.trilinear_pool_ref(x, *out)
    assert _maxabs(got, want) <= 1e-12
    assert bool((ab >= got.abs() - 1e-12).all()) and all(s.shape == got.shape for s in slopes)
    if shape == out:
        assert torch.equal(got, x)
    # the planted defect shows wherever a second tap has weight ((1, 6, 6) -> (1, 2, 2): every source index is a grid point)
    on_grid = all(float(R._pool_taps(n, m)[2].abs().max()) == 0.0 for n, m in zip(shape, out))
    assert on_grid == (shape in ((8, 6, 6), (1, 6, 6)))
    assert (_maxabs(R.trilinear_pool_ref(x, *out, second_tap_is_first=True)[0], got) > 0.1) == (not on_grid)


def test_merge_reference_equals_softmax_attention_over_x_plus_pos():
    """merge_ref on partials formed from real values (chunk maxima, sums and accumulators of e^(s - m) x_n over contiguous token chunks)
    is the plain attention softmax(S) (x + pos): the partial weights and the token-by-token positional term together."""
    from global_stream_inputs import chunk_token_ranges
    g = torch.Generator().manual_seed(11)
    T, H, W, rows, E, nparts, rows_pad = 3, 4, 5, 5, 8, 3, 8
    N, (t0, y0, x0) = T * H * W, (2, 7, 13)
    x = torch.randn(N, E, generator=g, dtype=torch.float64)
    S = 3.0 * torch.randn(rows_pad, N + 4, generator=g, dtype=torch.float64)
    pe = torch.randn(x0 + W, E, generator=g, dtype=torch.float64)
    pm, pl = torch.zeros(nparts, rows_pad, dtype=torch.float64), torch.zeros(nparts, rows_pad, dtype=torch.float64)
    pacc = torch.zeros(nparts, rows_pad, E, dtype=torch.float64)
    for i, (lo, hi) in enumerate(chunk_token_ranges(N, nparts)):
        assert hi > lo
        pm[i] = S[:, lo:hi].max(1).values
        e = torch.exp(S[:, lo:hi] - pm[i][:, None])
        pl[i], pacc[i] = e.sum(1), e @ x[lo:hi]
    t, y, xx = R.token_axes(N, H, W)
    val = x + pe[t0 + t] + pe[y0 + y] + pe[x0 + xx]
    p = torch.softmax(S[:rows, :N], 1)
    M, L, ctx = R.merge_ref(pm, pl, pacc, rows, S, N, H, W, pe, t0, y0, x0, normalize=True)
    assert torch.allclose(ctx, p @ val, rtol=1e-12, atol=1e-13)
    assert torch.allclose(M + torch.log(L), torch.logsumexp(S[:rows, :N], 1), rtol=1e-13, atol=0)
    _, _, acc = R.merge_ref(pm, pl, pacc, rows, S, N, H, W, pe, t0, y0, x0, normalize=False)
    assert torch.allclose(acc, L[:, None] * (p @ val), rtol=1e-12, atol=1e-13)
    assert torch.allclose(R.merge_ref(pm, pl, pacc, rows, normalize=True)[2], p @ x, rtol=1e-12, atol=1e-13)
    ab = R.merge_ref(pm, pl, pacc, rows, S, N, H, W, pe, t0, y0, x0, absolute=True)[2]
    assert bool((ab >= acc.abs() - 1e-12).all())
    # the combine of the partials seen as shard states, and merge + v_proj, are the same attention
    cx, Lc = R.combine_ref(torch.stack([pm, pl], 2)[:, :rows], pacc[:, :rows])
    assert torch.allclose(cx, p @ x, rtol=1e-12, atol=1e-13) and torch.allclose(Lc, L)
    wv = torch.randn(rows * 4, rows * 4, generator=g, dtype=torch.float64)
    x2 = torch.randn(N, rows * 4, generator=g, dtype=torch.float64)
    for i, (lo, hi) in enumerate(chunk_token_ranges(N, nparts)):
        e = torch.exp(S[:, lo:hi] - pm[i][:, None])
        pacc2 = e @ x2[lo:hi] if i == 0 else torch.cat([pacc2, e @ x2[lo:hi]])
    pacc2 = pacc2.reshape(nparts, rows_pad, rows * 4)
    M2, L2, c2, o = R.merge_vproj_ref(pm, pl, pacc2, rows, wv)
    want = torch.cat([wv[4 * h:4 * h + 4] @ (p[h] @ x2) for h in range(rows)])
    assert torch.allclose(o, want, rtol=1e-12, atol=1e-13) and torch.equal(M2, M) and torch.allclose(L2, L)
    o16 = R.merge_vproj_ref(pm, pl, pacc2 / pl[:, :, None], rows, wv, normalised=True)[3]
    assert torch.allclose(o16, want, rtol=1e-12, atol=1e-13)


# ---- readout GEMMs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,planes,bias", [(5, 7, 128, 2, True), (3, 4, 64, 1, False), (9, 2, 192, 2, True)])
def test_readout_gemm_reference_is_linear_plus_erf_gelu(M, N, K, planes, bias):
    g = torch.Generator().manual_seed(M * 31 + N)
    a_terms = [torch.randn(M, K, generator=g, dtype=torch.float64) * 2.0 ** (-9 * p) for p in range(planes)]
    w = torch.randn(N, K, generator=g, dtype=torch.float64)
    b = torch.randn(N, generator=g, dtype=torch.float64) if bias else None
    lin = torch.nn.functional.linear(sum(a_terms), w, b)
    val, ab, pre = R.readout_gemm_ref(a_terms, w, b)
    assert _maxabs(val, lin) <= TOL and torch.equal(val, pre) and bool((ab >= val.abs() - 1e-12).all())
    want_ab = sum(a.abs() for a in a_terms) @ w.abs().t() + (b.abs() if bias else 0.0)
    assert _maxabs(ab, want_ab) <= TOL
    val, _, pre = R.readout_gemm_ref(a_terms, w, b, "gelu")
    assert _maxabs(val, torch.nn.functional.gelu(lin)) <= TOL and _maxabs(pre, lin) <= TOL
    # every planted fault is a different function; the stage faults are what their names say
    s = K // 64 - 1
    ks = slice(64 * s, 64 * s + 64)
    last = sum(a_terms)[:, ks] @ w[:, ks].t()
    assert _maxabs(R.readout_gemm_ref(a_terms, w, b, drop_stage=s)[0], lin - last) <= TOL
    assert _maxabs(R.readout_gemm_ref(a_terms, w, b, double_stage=s)[0], lin + last) <= TOL
    if planes == 2:
        assert _maxabs(R.readout_gemm_ref(a_terms, w, b, drop_lo_stage=s)[0], lin - a_terms[1][:, ks] @ w[:, ks].t()) <= TOL
    if s >= 1:
        prev = sum(a_terms)[:, 64 * s - 64:64 * s] @ w[:, 64 * s - 64:64 * s].t()
        assert _maxabs(R.readout_gemm_ref(a_terms, w, b, stale_stage=s)[0], lin - last + prev) <= TOL
    half = sum(a_terms)[:, 64 * s + 32:64 * s + 64] @ w[1:2, 64 * s + 32:64 * s + 64].t()
    lost = R.readout_gemm_ref(a_terms, w, b, lost_half=(s, 1, 1, 2))[0]
    assert _maxabs(lost[:, 1:2], lin[:, 1:2] - half) <= TOL and _maxabs(lost[:, :1], lin[:, :1]) <= TOL
    if bias:
        early = R.readout_gemm_ref(a_terms, w, b, "gelu", gelu_before_bias=True)[0]
        assert _maxabs(early, torch.nn.functional.gelu(lin - b) + b) <= TOL


def test_the_rational_erf_of_gelu_erf_keeps_its_stated_error_and_the_gelu_slope_its_bound():
    x = torch.linspace(-8, 8, 400001, dtype=torch.float64)
    assert _maxabs(R.erf_as7126(x), torch.erf(x)) <= R.ERF_AS_ERR
    assert 1.128 < float(R.gelu_grad_ref(x)[0].abs().max()) <= R.GELU_SLOPE


def test_split_bf16_reference_carries_sixteen_bits():
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.randn(4096, generator=g) * 3, torch.randn(4096, generator=g) * 1e-3, torch.tensor([0.0, 1.0, -1.0, 1 + 2.0 ** -9, 255.0 / 256])])
    hi, lo = R.split_bf16_ref(x)
    assert hi.dtype == lo.dtype == torch.bfloat16 and torch.equal(hi, x.bfloat16())
    assert bool(((R.up(hi) + R.up(lo) - R.up(x)).abs() <= 2.0 ** -17 * R.up(x).abs()).all())
    assert bool((R.up(lo).abs() <= 2.0 ** -8 * R.up(hi).abs()).all())                      # the remainder is at most one bf16 ulp of hi
    assert float(lo[-2]) == 2.0 ** -9 and float(lo[-1]) == 0.0


@pytest.mark.parametrize("M,row0,g", [(1, 0, 0), (20, 3, 9), (7, 2, 1), (9, 0, 9), (8, 5, 9)])
def test_packed_rows_and_place_rows_against_an_explicit_loop(M, row0, g):
    rows, gaps = [], 0
    for m in range(M):
        if g > 0 and m > 0 and m % g == 0:
            gaps += 1
        rows.append(row0 + m + gaps)
    got = R.packed_rows(M, row0, g)
    assert got.tolist() == rows
    val = torch.arange(M * 3, dtype=torch.float64).reshape(M, 3) + 1
    img = R.place_rows(val, rows[-1] + 3, 5, got)
    for r in range(img.shape[0]):
        for col in range(5):
            want = val[rows.index(r), col] if (r in rows and col < 3) else None
            assert (want is None and math.isnan(float(img[r, col]))) or float(img[r, col]) == float(want)
    if g > 0 and M >= g:
        assert R.packed_rows(M, row0, g, gap_late=True).tolist() != rows


@pytest.mark.parametrize("pos,modal,t,h,w,anyres", [("grid", "video", 2, 3, 4, False), ("frame", "video", 3, 2, 5, False), ("one_token", "video", 2, 2, 2, False),
                                                     ("grid", "image", 1, 4, 3, True)])
def test_packed_rows_are_the_token_rows_of_the_packing_layout(pos, modal, t, h, w, anyres):
    from hicom_amd import geometry as geo
    lay = geo.pack_layout("spatial_unpad", pos, modal, t, h, w, True, anyres)
    tokens = [r for r in range(lay.n_rows) if r not in set(lay.newline_rows)]
    assert R.packed_rows(lay.n_tokens, 0, lay.nl_group).tolist() == tokens
    assert [lay.row_of(m) for m in range(lay.n_tokens)] == tokens
