"""Plain float64 restatements of the small operators declared in include/hicom_hip.h (torch on the CPU; no call into hicom_amd).

Shared by tests/test_gpu_ops_small.py (the kernels against these) and tests/test_ops_references.py (these against float64 autograd
and the oracle, so that a wrong reference cannot bless a wrong kernel).  Every function takes the values the kernel received,
up-cast: `up(t)` of the bf16 / fp16 / f32 tensor that was uploaded.  Functions that feed a tolerance also return the same
expression evaluated on absolute values (the sum of |terms| an fp32 summation error is proportional to)."""
import math

import torch

EPS23 = 2.0 ** -23          # one unit in the last place of an fp32 value in [1, 2)


def up(t):
    return t.detach().cpu().double()


def sum_tol(k, abs_sum):
    """fp32 error bound of a k-term sum / FMA chain in any order: k * 2^-23 * sum |terms| (first order; Higham 4.4)."""
    return k * EPS23 * abs_sum


# ---- d frames_feature of the global stage -----------------------------------------------------------------------------------
def global_dx_ref(S, dS, ml, qt, dctx, N, dx0=None):
    """dx[n, :] (+)= sum_r dS[r, n] qt[r, :] + exp(S[r, n] - M_r) / L_r dctx[r, :];  S, dS [rows, >= N], ml [rows, 2].
    Returns (dx, abs_terms, p) with p = exp(S - M) / L."""
    rows = qt.shape[0]
    S, dS = S[:rows, :N], dS[:rows, :N]
    p = torch.exp(S - ml[:, 0:1]) / ml[:, 1:2]
    dx = dS.t() @ qt + p.t() @ dctx
    ab = dS.abs().t() @ qt.abs() + p.t() @ dctx.abs()
    if dx0 is not None:
        dx, ab = dx + dx0, ab + dx0.abs()
    return dx, ab, p


def global_attention_backward_ref(qt, x, g):
    """Folded global attention f = sum_r ctx_r . g_r, ctx_r = sum_n softmax_n(qt_r . x_n) x_n: the tensors its backward leaves
    (S, ml, dS as hicom_global_stream_bwd defines them: dS = p (dP - delta), dP = g_r . x_n, delta_r = g_r . ctx_r)."""
    S = qt @ x.t()
    M = S.max(1).values
    L = torch.exp(S - M[:, None]).sum(1)
    p = torch.exp(S - M[:, None]) / L[:, None]
    dP = g @ x.t()
    delta = (p * dP).sum(1)
    dS = p * (dP - delta[:, None])
    return S, torch.stack([M, L], 1), dS, delta


# ---- clip-scale global stage ------------------------------------------------------------------------------------------------
def clip_query_prep_ref(qp, b_k, nh, scale):
    """qhat = qp / ||qp||_2 over E;  c[q * nh + h] = scale * sum_j qhat[q, h hd + j] b_k[h hd + j]  (0 without b_k)."""
    nq, E = qp.shape
    qhat = qp / qp.norm(dim=1, keepdim=True)
    if b_k is None:
        z = torch.zeros(nq * nh, dtype=torch.float64)
        return qhat, z, z.clone()
    prod = (qhat * b_k[None, :]).reshape(nq, nh, E // nh)
    return qhat, scale * prod.sum(-1).reshape(-1), abs(scale) * prod.abs().sum(-1).reshape(-1)


def fold_query_ref(qp, w_k, nh, scale):
    """qt[q nh + h, c] = scale sum_j w_k[h hd + j, c] qp[q, h hd + j]."""
    nq, E = qp.shape
    hd = E // nh
    return scale * torch.einsum("qhj,hjc->qhc", qp.reshape(nq, nh, hd), w_k.reshape(nh, hd, E)).reshape(nq * nh, E)


def inv_norm_ref(ssq):
    return 1.0 / torch.sqrt(ssq.sum(0))


def token_axes(N, H, W):
    n = torch.arange(N)
    return n // (H * W), (n // W) % H, n % W


def stream_terms(q, x, pos, pe=None, H=1, W=1, t0i=0, y0i=0, x0i=0, axes=(True, True, True), t_of=None):
    """The score tile of the stream kernels and the rows their values stand for:
        dot[r, n] = q_r . x_n + pos[r, t0i + t] + pos[r, y0i + y] + pos[r, x0i + x],   val_n = x_n + pe[t0i + t] + pe[y0i + y] + pe[x0i + x]
    (pos [rows, P] or None; pe [P, E] or None: val = x).  Returns (dot, abs terms of dot, val, |x| + |pe rows|).
    axes / t_of (the frame the score side takes each token for) are the defects tests/test_global_stream_power.py plants: a dropped
    positional term, a wrong frame index.  The value side always uses the token's own frame."""
    N = x.shape[0]
    dot, ab = q @ x.t(), q.abs() @ x.abs().t()
    val, vabs = x, x.abs()
    if pos is not None or pe is not None:
        t, y, xx = token_axes(N, H, W)
        if pos is not None:
            for on, c in zip(axes, (t0i + (t if t_of is None else t_of), y0i + y, x0i + xx)):
                if on:
                    dot, ab = dot + pos[:, c], ab + pos[:, c].abs()
        if pe is not None:
            val = x + pe[t0i + t] + pe[y0i + y] + pe[x0i + xx]
            vabs = x.abs() + pe[t0i + t].abs() + pe[y0i + y].abs() + pe[x0i + xx].abs()
    return dot, ab, val, vabs


def clip_attention_ref(q, x, inv, row_const, pos_a=None, pe=None, H=1, W=1, t0i=0, y0i=0, x0i=0):
    """logit[r, n] = (q_r . x_n + pos_a[r, t0i + t] + pos_a[r, y0i + y] + pos_a[r, x0i + x] + row_const[r]) * inv[n];
    ctx_r = sum_n softmax_n(logit[r, :]) (x_n + pe[t0i + t] + pe[y0i + y] + pe[x0i + x]).
    Returns (logit, ctx, abs terms of logit, sum_n p (|x_n| + |pe rows|): the value-side terms are summed separately)."""
    dot, ab, val, vabs = stream_terms(q, x, pos_a, pe if pos_a is not None else None, H, W, t0i, y0i, x0i)
    S = (dot + row_const[:, None]) * inv[None, :]
    ab = (ab + row_const.abs()[:, None]) * inv[None, :]
    p = torch.softmax(S, dim=1)
    return S, p @ val, ab, p @ vabs


# ---- the two global-stage stream kernels (hicom_global_stream_fwd / _marg_fwd / _bwd) and the merge behind them ---------------
def axis_marginals(w, H, W, t_of=None):
    """The t / y / x marginals of w [rows, N] over the token grid (T, H, W), N = T H W: ([rows, T], [rows, H], [rows, W]).
    t_of: the frame each token is counted under (a planted defect; default its own)."""
    rows, N = w.shape
    t, y, xx = token_axes(N, H, W)
    t = t if t_of is None else t_of
    return tuple(torch.zeros(rows, n, dtype=w.dtype).index_add_(1, ax, w) for ax, n in ((t, N // (H * W)), (y, H), (xx, W)))


def global_stream_ref(q, x, pos_a=None, pe=None, H=1, W=1, t0i=0, y0i=0, x0i=0, scale=1.0, axes=(True, True, True), t_of=None, lost=()):
    """What hicom_global_stream_fwd / _marg_fwd and the merge behind them stand for, in float64:
        S[r, n] = q_r . x_n + pos_a[r, t0i + t] + pos_a[r, y0i + y] + pos_a[r, x0i + x],  (M, L) and lse = M + log L per row,
        p = softmax_n S,  ctx_r = sum_n p[r, n] x_n + mt_r . pe[t0i + .] + my_r . pe[y0i + .] + mx_r . pe[x0i + .]
    with (mt, my, mx) the t / y / x marginals of p: the form the merge uses, equal to sum_n p (x_n + pe rows of n).  pos_a and pe
    None: no positional part (H, W unused).  scale / axes / t_of / lost (tokens left out of the softmax) plant defects.
    Returns a dict; `*_ab` is the same expression on absolute values; ctx_x is the token part of ctx alone."""
    N = x.shape[0]
    dot, ab, _, vabs = stream_terms(q, x, pos_a, pe, H, W, t0i, y0i, x0i, axes, t_of)
    S, S_ab = scale * dot, abs(scale) * ab
    Sk = S.clone()
    Sk[:, list(lost)] = -math.inf
    M = Sk.max(1).values
    e = torch.exp(Sk - M[:, None])
    L = e.sum(1)
    p = e / L[:, None]
    o = {"S": S, "S_ab": S_ab, "M": M, "L": L, "lse": M + torch.log(L), "p": p, "ctx_x": p @ x, "ctx_x_ab": p @ x.abs(), "vabs": vabs}
    o["ctx"], o["ctx_ab"] = o["ctx_x"], p @ vabs
    if pe is not None:
        T = N // (H * W)
        o["marg"] = axis_marginals(p, H, W, t_of)
        for m, c0, n in zip(o["marg"], (t0i, y0i, x0i), (T, H, W)):
            o["ctx"] = o["ctx"] + m @ pe[c0:c0 + n]
    return o


def global_stream_bwd_ref(g, x, pos_b, S, ml, delta, H=1, W=1, t0i=0, y0i=0, x0i=0, scale=1.0, axes=(True, True, True), t_of=None,
                          lost=(), use_delta=True):
    """hicom_global_stream_bwd in float64: dP[r, n] = g_r . x_n + pos_b[r, t0i + t] + pos_b[r, y0i + y] + pos_b[r, x0i + x],
        dS = exp(S - M) / L (dP - delta),   dSx_r = sum_n dS[r, n] x_n,   (mt, my, mx) = the t / y / x marginals of dS
    S [rows, >= N] the forward's logits, ml [rows, 2] = (M, L), delta [rows].  pos_b None: no positional part, no marginals.
    scale (of dP) / axes / t_of / lost (tokens whose dS is dropped) / use_delta plant defects.  Returns a dict with `*_ab` companions."""
    rows, N = g.shape[0], x.shape[0]
    dP, dP_ab, _, _ = stream_terms(g, x, pos_b, None, H, W, t0i, y0i, x0i, axes, t_of)
    dP, dP_ab = scale * dP, abs(scale) * dP_ab
    p = torch.exp(S[:rows, :N] - ml[:, 0:1]) / ml[:, 1:2]
    d = delta[:, None] if use_delta else torch.zeros(rows, 1, dtype=torch.float64)
    dS, dS_ab = p * (dP - d), p * (dP_ab + d.abs())
    dS[:, list(lost)] = 0
    o = {"p": p, "dP": dP, "dP_ab": dP_ab, "dS": dS, "dS_ab": dS_ab, "dSx": dS @ x, "dSx_ab": dS.abs() @ x.abs()}
    if pos_b is not None:
        o["marg"], o["marg_ab"] = axis_marginals(dS, H, W, t_of), axis_marginals(dS.abs(), H, W, t_of)
    return o


# ---- row operators over the token stream ------------------------------------------------------------------------------------
def l2norm_ref(x):
    return x / x.norm(dim=1, keepdim=True)


def layer_norm_stats(y, eps):
    mu = y.mean(-1, keepdim=True)
    var = ((y - mu) ** 2).mean(-1, keepdim=True)
    return mu, 1.0 / torch.sqrt(var + eps)


def ln_blend_ref(x, gamma, beta, src=None, alpha=1.0, eps=1e-6):
    """(1 - alpha) src + alpha (LayerNorm_eps(x) gamma + beta); also the same with every term's absolute value."""
    mu, rstd = layer_norm_stats(x, eps)
    ln = (x - mu) * rstd * gamma + beta
    ab = (x.abs() + mu.abs()) * rstd * gamma.abs() + beta.abs()
    if src is None:
        return ln, ab
    return (1 - alpha) * src + alpha * ln, abs(1 - alpha) * src.abs() + abs(alpha) * ab


def ln_fp32_tol(x, gamma, beta, eps):
    """fp32 error bound of LayerNorm_eps(x) gamma + beta computed with E-term fp32 sums, from the reference's own quantities:
      mean:  |d mu| <= E 2^-23 mean|x|                                   (E-term sum)
      var:   relative error of var + eps <= (2 |d mu| mean|x - mu| + E 2^-23 var) / (var + eps); rstd takes half of it, + 2^-22
             for the square root and the division
      value: |d mu| rstd |gamma| + |x - mu| rstd |gamma| rel(rstd) + 4 roundings of the final expression."""
    E = x.shape[-1]
    mu, rstd = layer_norm_stats(x, eps)
    d = x - mu
    var = (d * d).mean(-1, keepdim=True)
    dmu = E * EPS23 * x.abs().mean(-1, keepdim=True)
    rel = 0.5 * (2 * dmu * d.abs().mean(-1, keepdim=True) + E * EPS23 * var) / (var + eps) + 2.0 ** -22
    ab = (x.abs() + mu.abs()) * rstd * gamma.abs() + beta.abs()
    return dmu * rstd * gamma.abs() + d.abs() * rstd * gamma.abs() * rel + 4 * EPS23 * ab


def small_mha_ref(q, k, v, nh, scale):
    M, E = q.shape
    hd = E // nh
    qh, kh, vh = (t.reshape(-1, nh, hd).permute(1, 0, 2) for t in (q, k, v))
    S = qh @ kh.transpose(1, 2) * scale
    p = torch.softmax(S, dim=-1)
    out = (p @ vh).permute(1, 0, 2).reshape(M, E)
    ab = (p @ vh.abs()).permute(1, 0, 2).reshape(M, E)
    sab = (qh.abs() @ kh.abs().transpose(1, 2) * abs(scale))        # [nh, M, L]
    return out, ab, sab


# ---- window attention with the adaptor blends: backward ---------------------------------------------------------------------
def window_of_token(T, H, W, kt, ks):
    """Window index of every token of an exact (kt, ks, ks) partition, window order (t1, h1, w1) row-major."""
    assert T % kt == 0 and H % ks == 0 and W % ks == 0
    t, y, x = token_axes(T * H * W, H, W)
    return ((t // kt) * (H // ks) + y // ks) * (W // ks) + x // ks


def blend_rows(x, y, gamma, beta, alpha, eps):
    """K_n = (1 - a) x_n + a (gamma yhat_n + beta); returns (K, yhat).  y None: K = x."""
    if y is None:
        return x, None
    mu, rstd = layer_norm_stats(y, eps)
    yhat = (y - mu) * rstd
    return (1 - alpha) * x + alpha * (yhat * gamma + beta), yhat


def adapt_bwd_ref(kx, ky, kg, kb, ak, vx, vy, vg, vb, av, win, nw, q, scale, bias, dctx, eps=1e-6):
    """The six outputs of hicom_local_attn_adapt_bwd in closed form.  kx, vx [N, D]; ky, vy [N, D] or None; win [N] window of
    each token; q [nw, D] (a shared query repeated); dctx [nw, D].
    Returns dict(ds, pw [N]; sxk, syk, sxv, syv [nw, D]) and dict of absolute-term companions."""
    N, D = kx.shape
    K, yk = blend_rows(kx, ky, kg, kb, ak, eps)
    V, yv = blend_rows(vx, vy, vg, vb, av, eps)
    s = (K * q[win]).sum(1) * scale + bias
    dP = (V * dctx[win]).sum(1)
    ds, pw = torch.empty(N, dtype=torch.float64), torch.empty(N, dtype=torch.float64)
    for w in range(nw):
        m = win == w
        p = torch.softmax(s[m], 0)
        delta = (p * dP[m]).sum()
        pw[m] = p
        ds[m] = scale * p * (dP[m] - delta)
    out = {"ds": ds, "pw": pw}
    ab = {"s": (K.abs() * q[win].abs()).sum(1) * abs(scale), "dP": (V.abs() * dctx[win].abs()).sum(1)}

    def wsum(c, rows):
        o = torch.zeros(nw, D, dtype=torch.float64)
        o.index_add_(0, win, c[:, None] * rows)
        return o
    for name, c, rows in (("sxk", ds, kx), ("syk", ds, yk), ("sxv", pw, vx), ("syv", pw, yv)):
        if rows is not None:
            out[name], ab[name] = wsum(c, rows), wsum(c.abs(), rows.abs())
    return out, ab


def adapt_dy_ref(y, gamma, vec_tok, coef, alpha, eps=1e-6):
    """dy = d/dy of alpha LN(y) gamma for the upstream gradient coef[tok] vec[w(tok)]:  g = alpha coef (vec gamma),
    dy = rstd (g - mean(g) - yhat mean(g yhat));  r1 = (1 - alpha) coef vec.  vec_tok [N, D] = vec[w(tok)]."""
    mu, rstd = layer_norm_stats(y, eps)
    yhat = (y - mu) * rstd
    g = alpha * coef[:, None] * vec_tok * gamma
    m1, m2 = g.mean(1, keepdim=True), (g * yhat).mean(1, keepdim=True)
    dy = rstd * (g - m1 - yhat * m2)
    ab = rstd * (g.abs() + g.abs().mean(1, keepdim=True) + yhat.abs() * (g * yhat).abs().mean(1, keepdim=True))
    return dy, (1 - alpha) * coef[:, None] * vec_tok, ab


# ---- elementwise ------------------------------------------------------------------------------------------------------------
def gelu_ref(h):
    """erf GELU, and |d GELU / d erf| = |h| / 2 (what an error of the device erf is multiplied by)."""
    return 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0))), 0.5 * h.abs()


def gelu_grad_ref(h):
    """Phi(h) + h phi(h); second value: the magnitudes of its two transcendental factors, erf / 2 and h phi(h)."""
    erf = torch.erf(h / math.sqrt(2.0))
    hphi = h * torch.exp(-h * h / 2) / math.sqrt(2 * math.pi)
    return 0.5 * (1 + erf) + hphi, 0.5 * erf.abs() + hphi.abs()


def sequential_f32_sum(parts):
    """s = 0; s += parts[k] for k in slice order, every step rounded to fp32 (parts f32 [nparts, M])."""
    s = torch.zeros(parts.shape[1], dtype=torch.float32)
    for k in range(parts.shape[0]):
        s = s + parts[k]
    return s


# ---- dense 16-bit GEMM (hicom_dense16_gemm_fwd, hicom_dense16_tn_fwd) -----------------------------------------------------------
def slice_sums(v):
    """Sums of v [M, N] over the 64-column slices [64 s, min(64 s + 64, N)) -> [ceil(N / 64), M] (the layout of ssq / row_dot)."""
    M, N = v.shape
    S = (N + 63) // 64
    pad = torch.zeros(M, 64 * S, dtype=v.dtype)
    pad[:, :N] = v
    return pad.reshape(M, S, 64).sum(-1).t().contiguous()


def dense16_ref(a, w, b, *, K, tab=None, geom=None, act="none", res=None, dot_vec=None, t_of=None, swap_yx=False, tab_pitch=None,
                row_of=None, tab_at="pre", pre_has_tab=True, pad_cols_in_ssq=False, slices_swapped=False):
    """hicom_dense16_gemm_fwd in float64 on the exactly widened operands: a [M, >= K], w [N, >= K], b [N] or None,
        pre = a[:, :K] . w[:, :K]^T + table + b,   val = act(pre),   y = val + res,
        ssq[s, m] = sum of pre^2 over slice s (columns [64 s, min(64 s + 64, N))),   rdot[s, m] = sum of dot_vec . y over slice s,
    table[m, n] = tab[t0 + m // (H W), n] + tab[y0 + (m // W) % H, n] + tab[x0 + m % W, n] for n < N, geom = (H, W, t0, y0, x0),
    tab [P, tab_ld >= N].  act: "none" | "gelu" (erf) | "gelu_tanh".  Returns a dict (rdot only with dot_vec).
    The remaining keywords plant the defects of tests/test_dense16_power.py:
      t_of [M]         the frame row m is taken for;   swap_yx: y = rem % H, x = rem // H
      tab_pitch        the table read as a flat array with this pitch in place of tab_ld
      row_of [M]       the row whose (t, y, x) row m takes
      tab_at           "pre" (right) | "after_ssq": ssq is taken without the table | "after_act": the table is added to act(acc + b)
      pre_has_tab      False: the `pre` output alone lacks the table
      pad_cols_in_ssq  every padded column of the last slice adds b[N - 1]^2;   slices_swapped: slices 0 and 1 of ssq / rdot exchanged"""
    M, N = a.shape[0], w.shape[0]
    acc = a[:, :K] @ w[:, :K].t()
    bias = torch.zeros(N, dtype=torch.float64) if b is None else b
    term = torch.zeros(M, N, dtype=torch.float64)
    if tab is not None:
        H, W, t0, y0, x0 = geom
        m = torch.arange(M) if row_of is None else row_of
        t, rem = (m // (H * W) if t_of is None else t_of), m % (H * W)
        y, x = (rem % H, rem // H) if swap_yx else (rem // W, rem % W)
        flat, pitch, cols = tab.reshape(-1), (tab.shape[1] if tab_pitch is None else tab_pitch), torch.arange(N)
        rows = lambda r: flat[r[:, None] * pitch + cols[None, :]]
        term = rows(t0 + t) + rows(y0 + y) + rows(x0 + x)
    plain = acc + bias
    full = plain + term
    f = {"none": lambda h: h, "gelu": lambda h: gelu_ref(h)[0], "gelu_tanh": lambda h: torch.nn.functional.gelu(h, approximate="tanh")}[act]
    val = f(plain) + term if tab_at == "after_act" else f(full)
    sq_of = full if tab_at == "pre" else plain
    o = {"pre": full if (pre_has_tab and tab_at != "after_act") else plain, "val": val, "y": val if res is None else val + res}
    o["ssq"] = slice_sums(sq_of * sq_of)
    if pad_cols_in_ssq:
        o["ssq"][-1] += (64 * o["ssq"].shape[0] - N) * bias[N - 1] ** 2
    if dot_vec is not None:
        o["rdot"] = slice_sums(o["y"] * dot_vec[None, :])
    if slices_swapped:
        for k in ("ssq", "rdot"):
            if k in o:
                o[k] = o[k][[1, 0] + list(range(2, o[k].shape[0]))]
    return o


def dense16_tn_ref(a, b, M, N, k_rows=None):
    """hicom_dense16_tn_fwd (all splits summed) in float64: a[:, :M]^T . b[:, :N] over the rows of a [Kt, >= M] and b [Kt, >= N].
    k_rows (a slice of the contraction rows that are kept) plants a dropped split."""
    k_rows = slice(None) if k_rows is None else k_rows
    return a[k_rows, :M].t() @ b[k_rows, :N]


# ---- fused local + global stream (hicom_fused_stream_fwd) and its query producer (hicom_query_prep_fwd) -----------------------
def ring_partitions(NW, nparts):
    """Partition of every window: the contiguous window-major ranges [p wpw, min((p + 1) wpw, NW)), wpw = ceil(NW / nparts)."""
    wpw = (NW + nparts - 1) // nparts
    return torch.arange(NW) // wpw


def _seg_max(src, idx, n):
    """max of src[..., k] over the k with idx[k] == s, for s < n (-inf for an empty segment)."""
    out = torch.full(src.shape[:-1] + (n,), -math.inf, dtype=src.dtype)
    return out.scatter_reduce(-1, idx.expand(src.shape), src, "amax")


def fused_ring_ref(ff, T, H, W, kt, ks, q_local, l_scale, l_bias, qt, fe=None, llog=None, pos_a=None, pe=None, t0i=0, y0i=0, x0i=0,
                   nparts=1, win=None, part_of_window=None, value_pe=True, local_p_map=None):
    """What include/hicom_hip.h promises for hicom_fused_stream_fwd, in float64.  ff (fe) [N, E] in token order (t, y, x);
    q_local [E]; qt [rows, E] the folded global queries as the kernel received them (hi + lo planes, or the q_f32 rows);
    llog [N] replaces fe_n . q_local;  pos_a [rows, P], pe [P, E] (hi + lo planes summed) or both None.
    win / part_of_window (-1: in no partition) / value_pe / local_p_map override the token -> window map, the window -> partition
    map, the value-side pe rows and the un-normalised local weights: the defects tests/test_ops_references.py plants.
    Returns a dict; `x_ab` beside `x` is the same expression on absolute values."""
    N, E = ff.shape
    rows = qt.shape[0]
    if win is None:
        win = window_of_token(T, H, W, kt, ks)
    NW = (T // kt) * (H // ks) * (W // ks)
    o = {"win": win, "NW": NW}
    # local window contexts
    if llog is not None:
        d, d_ab = llog, llog.abs()
    else:
        d, d_ab = fe @ q_local, fe.abs() @ q_local.abs()
    s = l_scale * d + l_bias
    m_w = _seg_max(s, win, NW)
    e = torch.exp(s - m_w[win])
    l_w = torch.zeros(NW, dtype=torch.float64).index_add_(0, win, e)
    ew = e if local_p_map is None else local_p_map(e)
    o["ctx_local"] = torch.zeros(NW, E, dtype=torch.float64).index_add_(0, win, ew[:, None] * ff) / l_w[:, None]
    o["ctx_local_ab"] = torch.zeros(NW, E, dtype=torch.float64).index_add_(0, win, e[:, None] * ff.abs()) / l_w[:, None]
    o["local_s"], o["local_dot_ab"], o["local_m"] = s, d_ab, m_w
    # global logits
    S, qx_ab = qt @ ff.t(), qt.abs() @ ff.abs().t()
    S_ab = qx_ab
    val, val_ab = ff, ff.abs()
    t, y, x = token_axes(N, H, W)
    if pos_a is not None:
        cols = (t0i + t, y0i + y, x0i + x)
        for c in cols:
            S, S_ab = S + pos_a[:, c], S_ab + pos_a[:, c].abs()
        if value_pe:
            val = ff + pe[cols[0]] + pe[cols[1]] + pe[cols[2]]
            val_ab = ff.abs() + pe[cols[0]].abs() + pe[cols[1]].abs() + pe[cols[2]].abs()
    o["S"], o["S_ab"], o["qx_ab"] = S, S_ab, qx_ab
    # partitions
    if part_of_window is None:
        part_of_window = ring_partitions(NW, nparts)
    part = part_of_window[win]
    order = torch.argsort(part, stable=True)
    counts = torch.bincount(part[part >= 0], minlength=nparts)
    start = int((part < 0).sum())
    slots = T + H + W
    lse = torch.empty(nparts, rows, dtype=torch.float64)
    ctx = torch.empty(nparts, rows, E, dtype=torch.float64)
    ctx_ab, marg = torch.empty_like(ctx), torch.zeros(nparts, rows, slots, dtype=torch.float64)
    tokens = []
    for p in range(nparts):
        idx = order[start:start + int(counts[p])]
        start += int(counts[p])
        tokens.append(idx)
        Sp = S[:, idx]
        M = Sp.max(1, keepdim=True).values
        ep = torch.exp(Sp - M)
        L = ep.sum(1, keepdim=True)
        lse[p] = (M + torch.log(L))[:, 0]
        ctx[p], ctx_ab[p] = ep @ val[idx] / L, ep @ val_ab[idx] / L
        for base, ax in ((0, t), (T, y), (T + H, x)):
            marg[p].index_add_(1, base + ax[idx], ep / L)
    o["part_tokens"], o["lse"], o["part_ctx"], o["part_ctx_ab"], o["marg"] = tokens, lse, ctx, ctx_ab, marg
    w = torch.softmax(lse, 0)                                        # weight of every partition in the whole softmax
    o["merged"], o["merged_ab"] = (w[:, :, None] * ctx).sum(0), (w[:, :, None] * ctx_ab).sum(0)
    return o


def query_prep_ref(guide, w_q, b_q, w_k, kpe, nh, scale, g_w0, g_b0, b_o):
    """hicom_query_prep_fwd: qp = w_q guide + b_q;  qt[h] = scale w_k[h]^T qp[h];  pos_a[h] = scale kpe[h]^T qp[h] (kpe [E, P] or None);
    r0 = g_w0 (b_o + guide) + g_b0 (g_w0 None: no r0).  Returns (qt, pos_a, r0) and their absolute terms, the inner qp sum included."""
    E = w_q.shape[0]
    hd = E // nh
    qp, qp_ab = w_q @ guide + b_q, w_q.abs() @ guide.abs() + b_q.abs()
    qt = scale * torch.einsum("hje,hj->he", w_k.view(nh, hd, E), qp.view(nh, hd))
    qt_ab = abs(scale) * torch.einsum("hje,hj->he", w_k.abs().view(nh, hd, E), qp_ab.view(nh, hd))
    pa = pa_ab = r0 = r0_ab = None
    if kpe is not None:
        P = kpe.shape[1]
        pa = scale * torch.einsum("hjp,hj->hp", kpe.view(nh, hd, P), qp.view(nh, hd))
        pa_ab = abs(scale) * torch.einsum("hjp,hj->hp", kpe.abs().view(nh, hd, P), qp_ab.view(nh, hd))
    if g_w0 is not None:
        r0, r0_ab = g_w0 @ (b_o + guide) + g_b0, g_w0.abs() @ (b_o.abs() + guide.abs()) + g_b0.abs()
    return (qt, pa, r0), (qt_ab, pa_ab, r0_ab)


# ---- window attention (hicom_local_attn_fwd / _adapt_fwd / _bwd) and the pooled per-window queries ------------------------------
def window_axis(n, k):
    """(k, nwin, nfull) of one axis, restated from the balance rule the kernels are handed: n a multiple of k: n / k full windows;
    otherwise ceil(n / k) windows of which the first nfull = n mod nwin (or all) are full and every other one shares ONE element with
    its predecessor.  (n < k: one short window.)"""
    if n % k == 0:
        return k, n // k, n // k
    if n < k:
        return n, 1, 1
    nwin = -(-n // k)
    nfull = n % nwin or nwin
    assert nfull * k + (nwin - nfull) * (k - 1) == n, (n, k)
    return k, nwin, nfull


def window_axis_starts(n, k, wrong_overlap=False):
    """Start of every window of an axis (csrc/window_rows.hpp, axis_start): i k for i < nfull, else nfull k + (i - nfull)(k - 1) - 1.
    wrong_overlap plants the `- 1` dropped."""
    k, nwin, nfull = window_axis(n, k)
    return [i * k if i < nfull else nfull * k + (i - nfull) * (k - 1) - (0 if wrong_overlap else 1) for i in range(nwin)]


def window_tokens(T, H, W, kt, ks, wrong_overlap=False):
    """tok [NW, WIN]: token index of position i of window w; windows t-major over (t1, h1, w1), positions t-major over (t2, h2, w2),
    the flat index ((t0 + t2) H + y0 + h2) W + x0 + w2 as WindowGeom::token_of forms it.  Second value: the windows' (t1, h1, w1)
    [NW, 3].  (With wrong_overlap the last window runs one element off its axis; the flat index is kept below T H W.)"""
    axes = [(window_axis(n, k)[0], window_axis_starts(n, k, wrong_overlap)) for n, k in ((T, kt), (H, ks), (W, ks))]
    (ktt, st), (ky, sy), (kx, sx) = axes
    t2, h2, w2 = torch.meshgrid(torch.arange(ktt), torch.arange(ky), torch.arange(kx), indexing="ij")
    t2, h2, w2 = t2.reshape(-1), h2.reshape(-1), w2.reshape(-1)
    tok, idx = [], []
    for a, t0 in enumerate(st):
        for b, y0 in enumerate(sy):
            for c, x0 in enumerate(sx):
                tok.append(((t0 + t2) * H + (y0 + h2)) * W + (x0 + w2))
                idx.append((a, b, c))
    return torch.stack(tok).clamp_(max=T * H * W - 1), torch.tensor(idx)


def window_launch_classes(T, H, W, kt, ks):
    """Launch order of the backward's per-token outputs: None for an exact partition (one launch, plain stores); otherwise the list
    of window-index tensors per launch, parity class val = 0 .. 7 of (t1 & 1) | (h1 & 1) << 1 | (w1 & 1) << 2 restricted to the axes
    that overlap (windows of one class share no token)."""
    mask = sum(1 << a for a, (n, k) in enumerate(((T, kt), (H, ks), (W, ks))) if window_axis(n, k)[1] * window_axis(n, k)[0] != n)
    if not mask:
        return None
    _, idx = window_tokens(T, H, W, kt, ks)
    cls = ((idx[:, 0] & 1) | ((idx[:, 1] & 1) << 1) | ((idx[:, 2] & 1) << 2)) & mask
    return [torch.nonzero(cls == val).reshape(-1) for val in range(8) if not (val & ~mask)]


def _window_softmax(s, lost, stats_limit):
    s = s.clone()
    s[:, list(lost)] = -math.inf
    n = s.shape[1] if stats_limit is None else min(stats_limit, s.shape[1])
    mx = s[:, :n].max(1, keepdim=True).values
    e = torch.exp(s - mx)
    return e / e[:, :n].sum(1, keepdim=True), mx


def window_attention_ref(key, value, query, geom, scale, bias, l2norm=0, lost=(), stats_limit=None, wrong_overlap=False,
                         key_ab=None, value_ab=None):
    """hicom_local_attn_fwd (and, on blend_rows' rows, hicom_local_attn_adapt_fwd) in float64.  key, value [N, D] per token, already
    up-cast; query [NW, D] per window (a shared query repeated); geom = (T, H, W, kt, ks).
        s[w, i] = scale (q_w . k_n) / (|k_n| if l2norm & 1) / (|q_w| if l2norm & 2) + bias,  n = tok[w, i];   p = softmax_i s;
        ctx_w = sum_i p[w, i] v_n.
    key_ab / value_ab: the rows' absolute terms where a row is itself a sum (the adaptor blend); default |key|, |value|.
    lost (window positions out of the softmax), stats_limit (maximum and sum over the first n positions only) and wrong_overlap
    plant the defects of tests/test_window_attn_power.py.  Returns a dict: ctx, p, s, tok, and the absolute-term sums s_ab (of
    s - bias) and ctx_ab."""
    tok, _ = window_tokens(*geom, wrong_overlap=wrong_overlap)
    K, V = key[tok], value[tok]                                                  # [NW, WIN, D]
    Kab = K.abs() if key_ab is None else key_ab[tok]
    Vab = V.abs() if value_ab is None else value_ab[tok]
    den = torch.ones(tok.shape, dtype=torch.float64)
    if l2norm & 1:
        den = den * K.norm(dim=2)
    if l2norm & 2:
        den = den * query.norm(dim=1, keepdim=True)
    s = scale * torch.einsum("wid,wd->wi", K, query) / den + bias
    s_ab = abs(scale) * torch.einsum("wid,wd->wi", Kab, query.abs()) / den
    p, mx = _window_softmax(s, lost, stats_limit)
    return {"tok": tok, "s": s, "s_ab": s_ab, "p": p, "mx": mx, "ctx": torch.einsum("wi,wid->wd", p, V),
            "ctx_ab": torch.einsum("wi,wid->wd", p, Vab)}


def window_attention_bwd_ref(key, value, query, dctx, geom, scale, bias, l2norm_key=False, value_is_key=False, use_delta=True,
                             drop_kc=False, overwrite_shared=False, lost=(), key_grad_in_dvalue=True, stats_limit=None, wrong_overlap=False):
    """hicom_local_attn_bwd in closed form (the kernel's header comment), float64.  Per window, khat_i = k_i / |k_i| with l2norm_key
    (else k_i), r_i = 1 / |k_i| (else 1):
        s_i = scale q . khat_i + bias,  p = softmax(s),  dP_i = dctx_w . v_i,  delta = sum_j p_j dP_j,  dS_i = p_i (dP_i - delta)
        dq_w = scale sum_i dS_i khat_i,    dls_w = sum_i dS_i (s_i - bias)
        dk_i = dsk_i q - kc_i k_i,  dsk_i = scale dS_i r_i,  kc_i = dsk_i (q . khat_i) r_i  (0 without l2norm_key)
        dv_i = p_i dctx_w  (+ dk_i with value_is_key)
    dkey / dvalue [N, D] sum the windows that hold a token.  `steps`: the per-token contributions in launch order -- one entry per
    launch (window_launch_classes; a single one for an exact partition) with the tokens it writes (each once) and the rows it adds,
    and their absolute terms -- which the bf16 read-modify-write bound needs.
    use_delta, drop_kc, overwrite_shared (a shared token keeps only its last contribution), lost (window positions out of the
    softmax: no contribution anywhere), key_grad_in_dvalue, stats_limit and wrong_overlap (as in the forward) plant defects."""
    T, H, W, kt, ks = geom
    N, D = key.shape
    tok, _ = window_tokens(*geom, wrong_overlap=wrong_overlap)
    NW, WIN = tok.shape
    K, V = key[tok], value[tok]
    r = 1.0 / K.norm(dim=2) if l2norm_key else torch.ones(NW, WIN, dtype=torch.float64)
    sraw = torch.einsum("wid,wd->wi", K, query) * r
    sraw_ab = torch.einsum("wid,wd->wi", K.abs(), query.abs()) * r
    s = scale * sraw + bias
    p, mx = _window_softmax(s, lost, stats_limit)
    dP, dP_ab = torch.einsum("wid,wd->wi", V, dctx), torch.einsum("wid,wd->wi", V.abs(), dctx.abs())
    delta = (p * dP).sum(1, keepdim=True) if use_delta else torch.zeros(NW, 1, dtype=torch.float64)
    dS = p * (dP - delta)
    dsk = scale * dS * r
    kc = torch.zeros_like(dsk) if (not l2norm_key or drop_kc) else dsk * sraw * r
    o = {"tok": tok, "s": s, "s_ab": abs(scale) * sraw_ab, "sraw": sraw, "sraw_ab": sraw_ab, "r": r, "p": p, "mx": mx, "dP": dP,
         "dP_ab": dP_ab, "delta": delta, "dS": dS, "dsk": dsk, "kc": kc}
    o["dq"], o["dq_ab"] = torch.einsum("wi,wid->wd", dsk, K), torch.einsum("wi,wid->wd", dsk.abs(), K.abs())
    o["dls"], o["dls_ab"] = (dS * (s - bias)).sum(1), (dS * (s - bias)).abs().sum(1)
    dk = dsk[:, :, None] * query[:, None, :] - kc[:, :, None] * K
    dk_ab = dsk.abs()[:, :, None] * query.abs()[:, None, :] + kc.abs()[:, :, None] * K.abs()
    dv, dv_ab = p[:, :, None] * dctx[:, None, :], p[:, :, None] * dctx.abs()[:, None, :]
    if value_is_key and key_grad_in_dvalue:
        dv, dv_ab = dv + dk, dv_ab + dk_ab
    o["dk_rows"], o["dv_rows"] = dk, dv
    classes = window_launch_classes(*geom)
    launches = [torch.arange(NW)] if classes is None else classes
    o["steps"] = []
    o["dkey"], o["dvalue"] = torch.zeros(N, D, dtype=torch.float64), torch.zeros(N, D, dtype=torch.float64)
    for ws in launches:
        if ws.numel() == 0:
            continue
        t = tok[ws].reshape(-1)
        assert wrong_overlap or t.unique().numel() == t.numel(), "windows of one launch share a token"
        step = {"tok": t, "win": ws, "dk": dk[ws].reshape(-1, D), "dk_ab": dk_ab[ws].reshape(-1, D), "dv": dv[ws].reshape(-1, D),
                "dv_ab": dv_ab[ws].reshape(-1, D)}
        o["steps"].append(step)
        for name, rows in (("dkey", step["dk"]), ("dvalue", step["dv"])):
            if overwrite_shared:
                o[name][t] = rows
            else:
                o[name].index_add_(0, t, rows)
    return o


def _pool_taps(n_in, n_out):
    """PyTorch's align_corners=False source index (area_pixel_compute_source_index), clamped at 0: (i0, i1, lam) per output index."""
    src = ((torch.arange(n_out, dtype=torch.float64) + 0.5) * (n_in / n_out) - 0.5).clamp_min(0.0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, src - i0


def trilinear_pool_ref(x, To, Ho, Wo, second_tap_is_first=False):
    """hicom_trilinear_pool_fwd in float64: x [T, H, W, D] -> [To, Ho, Wo, D], taps and lerp nested t, then h, then w.  Also returns
    the same expression on absolute values, and per axis |upper neighbour - tap 0| + |tap 0 - lower neighbour| of the partially
    interpolated field (what an error of that axis' source index is multiplied by, on whichever side of an integer it falls).
    second_tap_is_first plants a defect (tests/test_window_attn_power.py)."""
    def lerp(v, dim, n_out):
        n_in = v.shape[dim]
        i0, i1, lam = _pool_taps(n_in, n_out)
        if second_tap_is_first:
            i1 = i0
        shape = [1] * v.dim()
        shape[dim] = n_out
        lam = lam.reshape(shape)
        a, b = v.index_select(dim, i0), v.index_select(dim, i1)
        return a * (1 - lam) + b * lam

    def absl(v, dim, n_out):
        return lerp(v.abs(), dim, n_out)

    def slope(v, dim, n_out):
        n_in = v.shape[dim]
        i0, _, _ = _pool_taps(n_in, n_out)
        a = v.index_select(dim, i0)
        return (v.index_select(dim, (i0 + 1).clamp_max(n_in - 1)) - a).abs() + (a - v.index_select(dim, (i0 - 1).clamp_min(0))).abs()

    out = lerp(lerp(lerp(x, 0, To), 1, Ho), 2, Wo)
    ab = absl(absl(absl(x, 0, To), 1, Ho), 2, Wo)
    sl_t = absl(absl(slope(x, 0, To), 1, Ho), 2, Wo)
    sl_h = absl(slope(lerp(x, 0, To), 1, Ho), 2, Wo)
    sl_w = slope(lerp(lerp(x, 0, To), 1, Ho), 2, Wo)
    return out, ab, (sl_t, sl_h, sl_w)


# ---- merge of streaming partials, cross-shard combine, merge + v_proj (csrc/merge.hip, csrc/merge_item.hpp) ---------------------
def merge_ref(part_m, part_l, part_acc, rows, scores=None, N=0, H=1, W=1, pe=None, t0i=0, y0i=0, x0i=0, normalize=False, absolute=False,
              lose_last_partial=False, lose_partial_batch=False, frame_max_unscaled=False, lose_frames_from_64=False,
              lose_pos_from_128=False, ignore_t0=False, swap_yx=False, neighbour_record=False, pad_leak=False, unnormalised_L=False):
    """hicom_global_merge_fwd / hicom_global_merge_marg_fwd as include/hicom_hip.h states them, in float64:
        M_r = max_p m_p,   L_r = sum_p e^(m_p - M_r) l_p,
        ACC[r, :] = sum_p e^(m_p - M_r) acc_p[r, :] + sum_n e^(s_n - M_r) (pe[t0i + t] + pe[y0i + y] + pe[x0i + x]),   (/ L_r with normalize)
    part_m, part_l [nparts, rows_pad], part_acc [nparts, rows_pad, E], scores [rows_pad, >= N] (or None: no positional term), pe [P, E].
    The positional term is taken token by token from the logits; no marginal is formed.  Returns (M, L, acc) of the first `rows` rows.
    absolute: acc is the same expression on absolute values, un-normalised (what an fp32 summation error is proportional to).
    The remaining keywords plant the faults of tests/test_merge_power.py (see its docstring)."""
    nparts = part_m.shape[0]
    nrow = rows + 1 if pad_leak else rows

    def weights(rsel):
        m, l = part_m[:, rsel], part_l[:, rsel]
        M = m.max(0).values
        w = torch.exp(m - M[None, :])
        wl = w.clone()
        if lose_last_partial:
            wl[nparts - 1] = 0
        wa = wl.clone()
        if lose_partial_batch and nparts >= 225:
            wa[:256] = 0
        wn = None
        if scores is not None and pe is not None:
            s = scores[rsel, :N]
            t, y, x = token_axes(N, H, W)
            wn = torch.exp(s - M[:, None])
            if frame_max_unscaled:
                fmax = _seg_max(s, t, N // (H * W))
                wn = torch.exp(s - fmax[:, t])
            if lose_frames_from_64:
                wn = wn * (t < 64)
        return M, (wl * l).sum(0), wa, wn, l.sum(0)

    sel = torch.arange(nrow)
    M, L, wa, wn, lsum = weights(sel)
    if neighbour_record:
        nb = (torch.arange(rows) + 1) % rows
        nb = torch.cat([nb, sel[rows:]])
        _, Lr, wa, wn, lsum = weights(nb)
    else:
        Lr = L
    vals = part_acc[:, :nrow].abs() if absolute else part_acc[:, :nrow]
    acc = (wa[:, :, None] * vals).sum(0)
    if wn is not None:
        T = N // (H * W)
        t, y, x = token_axes(N, H, W)
        ty, tx = (x % H, y % W) if swap_yx else (y, x)
        rows_of = ((0 if ignore_t0 else t0i) + t, y0i + ty, x0i + tx)
        keep = (t < 128, T + ty < 128, T + H + tx < 128) if lose_pos_from_128 else (None, None, None)
        pos = None                                                   # [N, E]: the positional rows of every token, summed in place
        for idx, k in zip(rows_of, keep):
            term = pe[idx]
            if absolute:
                term.abs_()
            if k is not None:
                term[~k] = 0
            pos = term if pos is None else pos.add_(term)
        acc = acc + wn @ pos
    if normalize and not absolute:
        acc = acc / (lsum if unnormalised_L else Lr)[:, None]
    if pad_leak:
        acc[rows - 1] = acc[rows - 1] + acc[rows]
    return M[:rows], L[:rows], acc[:rows]


def combine_ref(ml, acc, absolute=False, unnormalised_L=False, lose_second_column_block=False):
    """hicom_global_combine_fwd / _strided_fwd in float64: ml [nsets, rows, 2] = (M, L) per set, acc [nsets, rows, E] un-normalised:
    ctx = sum_k e^(M_k - M) acc_k / sum_k e^(M_k - M) L_k,  M = max_k M_k.  Returns (ctx, L); absolute: the numerator on absolute values."""
    Mk, Lk = ml[:, :, 0], ml[:, :, 1]
    w = torch.exp(Mk - Mk.max(0).values[None])
    L = (w * Lk).sum(0)
    if absolute:
        return (w[:, :, None] * acc.abs()).sum(0), L
    ctx = (w[:, :, None] * acc).sum(0) / (Lk.sum(0) if unnormalised_L else L)[:, None]
    if lose_second_column_block:
        ctx[:, 256:] = (acc[0] / Lk[0][:, None])[:, 256:]
    return ctx, L


def merge_vproj_ref(part_m, part_l, part_acc, rows, w_v, normalised=False, absolute=False, head_off_by_one=False, lose_last_slab=False):
    """hicom_merge_vproj_fwd / _fixed_fwd / _sets_fwd in float64, from the values the kernel received (bf16 weights and f16 partials
    up-cast): (M, L) and ctx_h = sum_p e^(m_p - M) acc_p[h] / L of head h = row h, o[h hd + j] = W_v[h hd + j, :] . ctx_h, hd = E / rows.
    normalised: part_acc holds the normalised contexts acc_p / l_p (the f16 form), weighed with l_p e^(m_p - M).
    absolute: (M, L, sum_p w_p |acc_p| / L, sum_c |W_v| |ctx|).  head_off_by_one / lose_last_slab plant faults."""
    E = part_acc.shape[-1]
    hd = E // rows
    m, l = part_m[:, :rows], part_l[:, :rows]
    M = m.max(0).values
    w = torch.exp(m - M[None])
    L = (w * l).sum(0)
    wa = w * l if normalised else w
    ctx = (wa[:, :, None] * (part_acc[:, :rows].abs() if absolute else part_acc[:, :rows])).sum(0) / L[:, None]
    wv = w_v.reshape(rows, hd, E)
    if head_off_by_one:
        wv = wv.roll(-1, 0)
    cx = ctx.abs() if absolute else ctx
    if lose_last_slab:
        cx = cx.clone()
        cx[:, E - 64:] = 0
    o = torch.einsum("hjc,hc->hj", wv.abs() if absolute else wv, cx).reshape(E)
    return M, L, ctx, o


# ---- readout GEMMs (hicom_readout_gemm_fwd, hicom_planes_gemm_fwd, hicom_readout16_gemm_fwd) ---------------------------------------
ERF_AS_ERR = 1.5e-7         # Abramowitz-Stegun 7.1.26: |erf_as7126(x) - erf(x)| <= 1.5e-7 (its stated error; gelu_erf of csrc/common.hpp)
GELU_SLOPE = 1.13           # max |GELU'(h)| = Phi(h) + h phi(h) at h = sqrt 2: 1.12893


def erf_as7126(x):
    """gelu_erf's erf restated in float64: 1 - (a1 t + .. + a5 t^5) exp(-x^2), t = 1 / (1 + 0.3275911 |x|), odd in x."""
    z = x.abs()
    t = 1.0 / (1.0 + 0.3275911 * z)
    poly = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
    return torch.sign(x) * (1.0 - poly * torch.exp(-z * z))


def split_bf16_ref(x):
    """split_bf16 of csrc/common.hpp on an f32 tensor: hi = RNE bf16 of x, lo = RNE bf16 of the fp32 remainder x - hi."""
    assert x.dtype == torch.float32
    hi = x.bfloat16()
    return hi, (x - hi.float()).bfloat16()


def packed_rows(M, row0, nl_group, gap_late=False):
    """Output row of token row m: row0 + m + m // nl_group (no gaps with nl_group = 0).  gap_late plants (m + 1) // nl_group."""
    m = torch.arange(M)
    return row0 + m + ((m + (1 if gap_late else 0)) // nl_group if nl_group > 0 else 0)


def place_rows(val, rows, ld, orow, pitch=None):
    """The [rows, ld] output image with val [M, N] stored at flat index orow[m] * pitch + n (pitch = ld unless a fault is planted) and
    NaN everywhere else."""
    M, N = val.shape
    flat = torch.full((rows * ld,), float("nan"), dtype=torch.float64)
    flat[(orow[:, None] * (ld if pitch is None else pitch) + torch.arange(N)[None, :]).reshape(-1)] = val.reshape(-1)
    return flat.view(rows, ld)


def readout_gemm_ref(a_terms, w, b, act="none", *, drop_lo_stage=None, stale_stage=None, drop_stage=None, double_stage=None, lost_half=None,
                     row_of=None, col_of=None, bias_of=None, gelu_before_bias=False):
    """y = act(sum_p a_terms[p] . w^T + b) in float64 on the operands the kernel multiplies, already up-cast: a_terms = [hi, lo] (the
    split forms), [hi] (planes_gemm without a lo plane) or [a16]; each [M, K], w [N, K], b [N] or None, act "none" | "gelu" (erf).
    Returns (value, sum of |terms| including |b|, pre-activation).  K runs in stages of 64, as in the kernels.  The keywords plant the
    faults of tests/test_readout_gemm_power.py:
      drop_lo_stage s      the planes behind the first (lo) leave stage s out
      stale_stage s        stage s contributes what stage s - 1 does (a ring slot read before its data landed)
      drop_stage s / double_stage s   stage s missing / counted twice
      lost_half (s, h, n_lo, n_hi)    columns [n_lo, n_hi) lose the 32-wide k half h of stage s
      row_of [M] / col_of [N]         the row of a_terms / the row of w that output row m / column n is computed from
      bias_of [N]          the bias element column n takes;   gelu_before_bias: act(acc) + b"""
    M, K = a_terms[0].shape
    N = w.shape[0]
    assert K % 64 == 0 and w.shape[1] == K
    acc = torch.zeros(M, N, dtype=torch.float64)
    ab = torch.zeros(M, N, dtype=torch.float64)
    for p, a in enumerate(a_terms):
        for s in range(K // 64):
            if s == drop_stage or (p >= 1 and s == drop_lo_stage):
                continue
            src = s - 1 if s == stale_stage else s
            ks = slice(64 * src, 64 * src + 64)
            t, ta = a[:, ks] @ w[:, ks].t(), a[:, ks].abs() @ w[:, ks].abs().t()
            if lost_half is not None and lost_half[0] == s:
                _, h, n_lo, n_hi = lost_half
                kh = slice(64 * src + 32 * h, 64 * src + 32 * h + 32)
                t[:, n_lo:n_hi] -= a[:, kh] @ w[n_lo:n_hi, kh].t()
                ta[:, n_lo:n_hi] -= a[:, kh].abs() @ w[n_lo:n_hi, kh].abs().t()
            mult = 2.0 if s == double_stage else 1.0
            acc += mult * t
            ab += mult * ta
    if row_of is not None:
        acc, ab = acc[row_of], ab[row_of]
    if col_of is not None:
        acc, ab = acc[:, col_of], ab[:, col_of]
    bias = torch.zeros(N, dtype=torch.float64) if b is None else (b if bias_of is None else b[bias_of])
    pre = acc + bias
    if act == "gelu":
        val = gelu_ref(acc)[0] + bias if gelu_before_bias else gelu_ref(pre)[0]
    else:
        assert act == "none"
        val = pre
    return val, ab + bias.abs(), pre
