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


def test_window_index_and_sequential_sum():
    win = R.window_of_token(4, 4, 6, 2, 2)
    assert int(win.max()) + 1 == 2 * 2 * 3 and bool((torch.bincount(win) == 8).all())
    assert int(win[(1 * 4 + 3) * 6 + 5]) == (0 * 2 + 1) * 3 + 2 and int(win[(2 * 4 + 0) * 6 + 0]) == 6
    parts = torch.tensor([[1e8], [1.0], [-1e8], [1.0]], dtype=torch.float32)
    assert float(R.sequential_f32_sum(parts)[0]) == 1.0            # (1e8 + 1) rounds to 1e8 in fp32: order is visible
