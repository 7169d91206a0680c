"""fp64 reference, synthetic state and error bounds of the ragged adaptor backward's native calls (tests/test_gpu_ragged_adapt_bwd.py):
hicom_compressor_ragged_local_adapt_bwd, hicom_compressor_ragged_adapt_dy and hicom_compressor_ragged_dq_item.

State (numpy, no device): a mixed batch at a 6 x 6 grid, items of (T, kt); token streams x_k, x_v and guides N(0, SIGMA) times 4^b for item b
(a power of two: exact in bf16), so the x part of every logit of item b is 16^b times item 0's and neighbouring windows of one launch see
softmax levels that far apart; fp16 y planes N(0, 1); seeded dctx; at the item's tokens 0, 15, 16 and N - 1 the key row is raised along the
item's guide so that its logit stands SPIKE above its flat value (the window that holds it is then far from uniform).

Bounds (first-order propagation of fp32 rounding through the kernels' own order of operations, every term named; eps = 2^-24):
  eta                 (D + 64) eps: a D-term fp32 dot product with its cross-lane tree and the few operations around it, relative to the sum
                      of the absolute products
  d_s                 scale eta (2 A + 2 a B): A = sum_c |q_c| |blended K_c| terms taken apart, B = sum_c |q gamma|_c (|yhat_c| + |mu| rstd): the
                      LayerNorm statistics' own rounding (rstd and mu to eta) reaches the logit through the y branch
  d_p                 p (expm1(2 max_window d_s) + TRANS + 4 eps): softmax of perturbed logits and the device exponential
  d_delta, d_dS       the product rule on dS = p (dP - sum p dP), + the rounding of the WIN-term sum
  sums                sum_n (d_ds_n |x_n| + (WIN + 2) eps |ds_n| |x_n|), with the statistics' term for the yhat sums
  dy, r1              one bf16 rounding (2^-8 relative) + 4 eta of the absolute terms of the LayerNorm backward
  column sums         against the sum of the kernel's OWN stored dy in fp64: (N + 8) eps sum |dy| -- a pure fp32 summation bound, any order"""
import numpy as np

from hicom_amd import synth

D, H, W, KS = 1152, 6, 6, 3
EPS32, TRANS, LN_EPS = 2.0 ** -24, 2.0 ** -21, 1e-6
ETA = (D + 64) * EPS32
SIGMA, SPIKE = 0.02, 8.0
ITEMS = ((1, 1), (4, 4), (1, 1), (8, 4), (1, 1))           # (T, kt): MIX6 as forward_ragged lays it out (image, clips, 1-frame video)


def bf16(a):
    return synth.round_to_bf16(np.asarray(a, np.float32))


def item_windows(T, kt):
    """Token indices (item-local) of every window of one item, windows t-major, tokens t-major: WindowGeom restated."""
    out = []
    for t1 in range(T // kt):
        for h1 in range(H // KS):
            for w1 in range(W // KS):
                out.append(np.array([((t1 * kt + t2) * H + h1 * KS + h2) * W + w1 * KS + w2
                                     for t2 in range(kt) for h2 in range(KS) for w2 in range(KS)], dtype=np.int64))
    return out


def layout(items=ITEMS):
    """tok0, N per item, and per window of the concatenated list (item, stacked token indices)."""
    tok0, wins = [], []
    n = 0
    for i, (T, kt) in enumerate(items):
        tok0.append(n)
        wins += [(i, n + w) for w in item_windows(T, kt)]
        n += T * H * W
    return tok0, [T * H * W for T, _ in items], wins


def state(seed=7, items=ITEMS, adapt_k=True, adapt_v=True):
    rng = np.random.default_rng(seed)
    tok0, Ns, wins = layout(items)
    N, B, NW = sum(Ns), len(items), len(wins)
    level = np.concatenate([np.full(n, 4.0 ** b, np.float32) for b, n in enumerate(Ns)])[:, None]
    g = bf16(rng.standard_normal((B, D)) * SIGMA) * (4.0 ** np.arange(B, dtype=np.float32))[:, None]
    kx = bf16(rng.standard_normal((N, D)) * SIGMA).astype(np.float64)
    alpha = float(bf16(0.5))
    for b, (t0, n) in enumerate(zip(tok0, Ns)):               # the spikes, on the flat rows (levelled below with the item)
        gb = g[b].astype(np.float64) / 4.0 ** b
        for tok in sorted({0, 15, 16, n - 1}):
            kx[t0 + tok] += SPIKE * np.sqrt(D) * gb / (gb @ gb) / ((1 - alpha) if adapt_k else 1.0) / 16.0 ** b
    s = dict(items=items, tok0=tok0, Ns=Ns, wins=wins, g=g, kx=bf16(kx) * level, vx=bf16(rng.standard_normal((N, D)) * SIGMA) * level,
             ky=rng.standard_normal((N, D)).astype(np.float16) if adapt_k else None,
             vy=rng.standard_normal((N, D)).astype(np.float16) if adapt_v else None,
             dctx=(rng.standard_normal((NW, D)) * 0.1).astype(np.float32), alpha=alpha, scale=D ** -0.5)
    for n_ in ("k", "v"):
        s[n_ + "gamma"], s[n_ + "beta"] = bf16(1.0 + 0.1 * rng.standard_normal(D)), bf16(0.1 * rng.standard_normal(D))
    return s


def ln(y):
    y = y.astype(np.float64)
    mu = y.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(y.var(-1, keepdims=True) + LN_EPS)
    return (y - mu) * rstd, mu, rstd


def _stream(x, y, gamma, beta, a, v):
    """(values v . blended row per token, A, B of the bound, yhat or None, stats term) for the rows x, y of one window against the vector v."""
    x = x.astype(np.float64)
    if y is None:
        return x @ v, np.abs(x) @ np.abs(v), 0.0, None, 0.0
    yhat, mu, rstd = ln(y)
    gm, bt = gamma.astype(np.float64), beta.astype(np.float64)
    val = (1 - a) * (x @ v) + a * ((yhat * gm + bt) @ v)
    A = (1 - a) * (np.abs(x) @ np.abs(v)) + a * ((np.abs(yhat * gm) + np.abs(bt)) @ np.abs(v))
    stat = np.abs(yhat) + np.abs(mu) * rstd
    return val, A, a * (stat @ np.abs(gm * v)), yhat, stat


def window_backward(s):
    """fp64 outputs of hicom_compressor_ragged_local_adapt_bwd on `s` and their bounds: ({name: array}, {name: bound array})."""
    N, NW = sum(s["Ns"]), len(s["wins"])
    out = {k: np.zeros(N) for k in ("ds", "pw")}
    out.update({k: np.zeros((NW, D)) for k in ("sxk", "sxv")})
    if s["ky"] is not None:
        out["syk"] = np.zeros((NW, D))
    if s["vy"] is not None:
        out["syv"] = np.zeros((NW, D))
    tol = {k: np.zeros_like(v) for k, v in out.items()}
    a, sc = s["alpha"], s["scale"]
    for w, (item, toks) in enumerate(s["wins"]):
        WIN = len(toks)
        q, gd = s["g"][item].astype(np.float64), s["dctx"][w].astype(np.float64)
        lk, Ak, Bk, yk, stk = _stream(s["kx"][toks], None if s["ky"] is None else s["ky"][toks], s["kgamma"], s["kbeta"], a, q)
        dP, Av, Bv, yv, stv = _stream(s["vx"][toks], None if s["vy"] is None else s["vy"][toks], s["vgamma"], s["vbeta"], a, gd)
        logit = sc * lk
        d_s = sc * ETA * (2 * Ak + 2 * Bk) + 4 * EPS32 * np.abs(logit)
        d_d = ETA * (2 * Av + 2 * Bv)
        p = np.exp(logit - logit.max())
        p /= p.sum()
        d_p = p * (np.expm1(2 * d_s.max()) + TRANS + (WIN + 4) * EPS32)
        delta = p @ dP
        d_delta = d_p @ np.abs(dP) + p @ d_d + (WIN + 2) * EPS32 * (p @ np.abs(dP))
        dS = p * (dP - delta)
        d_dS = d_p * np.abs(dP - delta) + p * (d_d + d_delta) + 4 * EPS32 * np.abs(dS)
        ds, d_ds = sc * dS, sc * d_dS + 2 * EPS32 * sc * np.abs(dS)
        out["ds"][toks], out["pw"][toks], tol["ds"][toks], tol["pw"][toks] = ds, p, d_ds, d_p
        for name, wt, d_wt, rows, yhat, stat in (("k", ds, d_ds, s["kx"][toks], yk, stk), ("v", p, d_p, s["vx"][toks], yv, stv)):
            rows = rows.astype(np.float64)
            out["sx" + name][w] = wt @ rows
            tol["sx" + name][w] = d_wt @ np.abs(rows) + (WIN + 2) * EPS32 * (np.abs(wt) @ np.abs(rows))
            if yhat is not None:
                out["sy" + name][w] = wt @ yhat
                tol["sy" + name][w] = d_wt @ np.abs(yhat) + np.abs(wt) @ (2 * ETA * stat) + (WIN + 4) * EPS32 * (np.abs(wt) @ np.abs(yhat))
    return out, tol


def adapt_dy(y, gamma, vec_rows, coef, alpha):
    """fp64 (dy, r1) of the dy step for per-token rows of the rank-1 vector, and their bounds."""
    yhat, mu, rstd = ln(y)
    vg = vec_rows.astype(np.float64) * gamma.astype(np.float64)
    m1, m2 = vg.mean(-1, keepdims=True), (vg * yhat).mean(-1, keepdims=True)
    k = alpha * coef.astype(np.float64)[:, None] * rstd
    dy = k * (vg - m1 - yhat * m2)
    stat = np.abs(yhat) + np.abs(mu) * rstd
    tol_dy = 2.0 ** -8 * np.abs(dy) + 4 * ETA * np.abs(k) * (np.abs(vg) + np.abs(vg).mean(-1, keepdims=True) + stat * (np.abs(vg) * stat).mean(-1, keepdims=True))
    r1 = (1 - alpha) * coef.astype(np.float64)[:, None] * vec_rows.astype(np.float64)
    return dy, r1, tol_dy, (2.0 ** -8 + 4 * EPS32) * np.abs(r1)


def colsum_bound(dy_stored):
    """|column sums - fp64 sum of the stored dy|: fp32 summation of N values in any order."""
    return (dy_stored.shape[0] + 8) * EPS32 * np.abs(dy_stored).sum(0)
