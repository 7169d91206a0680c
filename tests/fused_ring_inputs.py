"""Inputs, case lists, float64 references and error bounds of the fused ring kernel (hicom_fused_stream_fwd): what
tests/test_gpu_fused_ring.py runs on the device and tests/test_ops_references.py checks on the CPU.  tests/test_gpu_fused_ring.py's
docstring has the derivation of the bounds."""
import math
from types import SimpleNamespace

import torch

import ops_reference as R
from ops_reference import EPS23, sum_tol, up

E = 1152
F16_RND, F16_SUB, TRANS, BF16_PLANES = 2.0 ** -10, 2.0 ** -24, 2.0 ** -21, 2.0 ** -16
NAN = float("nan")
FORMS = ("bf16", "logits", "f16")
SHAPES = [(8, 6, 6, 4, 3), (16, 27, 27, 4, 3), (4, 27, 27, 4, 3), (8, 6, 6, 4, 2), (8, 8, 8, 4, 4), (8, 6, 6, 2, 3), (4, 4, 8, 1, 4),
          (12, 9, 6, 4, 3), (2, 8, 8, 1, 8), (8, 30, 30, 4, 3)]
ROWS = (1, 2, 9, 12)
COLLECT_CUS = 256            # workgroup slots assumed when the cases are listed; the run asks hicom_fused_stream_nparts itself


# =============================================================================================================================
# the documented limits of hicom_fused_stream_fwd, restated
# =============================================================================================================================
def ring_refusal(T, H, W, kt, ks, rows, nparts, logits, E_=E):
    """None when include/hicom_hip.h and the entry point's checks admit the launch, else the limit it breaks."""
    if E_ != 1152:
        return "E"
    if min(T, H, W, kt, ks) <= 0 or T % kt or H % ks or W % ks:
        return "inexact windows"
    wsz = kt * ks * ks
    if not 16 <= wsz <= 64:
        return "window size"
    if not 1 <= rows <= 12:
        return "rows"
    NW = (T // kt) * (H // ks) * (W // ks)
    if not 1 <= nparts <= NW:
        return "nparts"
    wpw = (NW + nparts - 1) // nparts
    if wpw > 32 or (nparts - 1) * wpw >= NW:
        return "windows per workgroup / empty workgroup"
    per_t = (H // ks) * (W // ks)
    if ((wpw + per_t - 2) // per_t + 1) * kt > 8:
        return "frame span"
    if H > 64 or W > 64:
        return "grid"
    nwx = W // ks
    if 8 + min(H, ((wpw + nwx - 2) // nwx + 1) * ks) + min(W, wpw * ks) > 64:
        return "pos-emb slots"
    if rows * (8 + H + W) > 1024:
        return "pos-emb table"
    lds = 4 * 9 * 4096 + 9 * 1024 + 8 * 80 * 4 + 8 * 64 + (64 + 32 + 65 + 32 + 16) * 4 + rows * (8 + H + W) * 4 + ((32 + 64) * 4 if logits else 0)
    if lds > 163840:
        return "LDS"
    return None


def n_windows(T, H, W, kt, ks):
    return (T // kt) * (H // ks) * (W // ks)


def cu_nparts(NW, cus):
    wpw = min((NW + cus - 1) // cus, 32)
    return (NW + wpw - 1) // wpw


def valid_nparts(shape, rows, form, cus=COLLECT_CUS):
    """[smallest valid nparts, the one hicom_fused_stream_nparts suggests, one window per workgroup], those the limits admit."""
    NW = n_windows(*shape)
    ok = [n for n in range(1, NW + 1) if ring_refusal(*shape, rows, n, form == "logits") is None]
    picks = ([ok[0]] if ok else []) + [n for n in (cu_nparts(NW, cus), NW) if n in ok]
    return sorted(set(picks))


# shapes the limits refuse for every nparts (LDS): they belong to the refusal test
REFUSED = {((16, 27, 27, 4, 3), 12, "logits"), ((4, 27, 27, 4, 3), 12, "logits")} | {((8, 30, 30, 4, 3), 12, f) for f in FORMS}
CASES = [(s, r, f) for s in SHAPES for r in ROWS for f in FORMS if valid_nparts(s, r, f)]
assert {(s, r, f) for s in SHAPES for r in ROWS for f in FORMS} - set(CASES) == REFUSED, "the case list and the documented limits disagree"


# =============================================================================================================================
# inputs (CPU tensors; seeded) -- shared with the defect-sensitivity checks
# =============================================================================================================================
def split_tok(x, dt):
    """hi / lo planes of f32 values in the token type (what hicom_split16_fwd computes for finite values in range)."""
    hi = x.to(dt)
    return hi, (x - hi.float()).to(dt)


def stream_order(T, H, W, kt, ks):
    """Position of every token in the window-major stream (window, then (t2, h2, w2) inside it)."""
    win = R.window_of_token(T, H, W, kt, ks)
    order = torch.argsort(win, stable=True)
    pos = torch.empty_like(order)
    pos[order] = torch.arange(order.numel())
    return pos


FAMILIES = ("plain", "flat", "peaky_up", "peaky_down", "offsets", "bias+", "bias-", "extremes", "coherent")


def ring_inputs(family, form, shape, rows, seed=0):
    """Every operand of one hicom_fused_stream_fwd call as CPU tensors in the kernel's types, and the float64 view of the same
    values the reference takes (`ref_args()`)."""
    T, H, W, kt, ks = shape
    N = T * H * W
    g = torch.Generator().manual_seed(1000 * seed + 17 * T + 3 * H + W + 131 * rows + len(family))
    rnd = lambda *s: torch.randn(*s, generator=g)
    dt = torch.float16 if form == "f16" else torch.bfloat16
    i = SimpleNamespace(family=family, form=form, shape=shape, rows=rows, dt=dt, l_scale=1.0 / math.sqrt(E), l_bias=0.0)
    ff, fe, q_local, qt = rnd(N, E), rnd(N, E), rnd(E), 0.05 * rnd(rows, E)
    i.t0i, cap = 0, T
    i.y0i, i.x0i = cap, cap + H
    P = cap + H + W
    pos_scale = 0.5
    if family == "flat":
        # nearly constant logits on both sides: the logit terms of the bounds vanish, what is left polices the weight planes, the pe
        # planes, P.x and the output planes
        fe, qt, pos_scale = fe * 2.0 ** -10, qt * 2.0 ** -12, 0.0
    elif family in ("peaky_up", "peaky_down"):
        # global logits (r + 1) / rows * ramp along the stream through one direction v: rising = the running max moves at every tile,
        # falling = it never moves after a partition's first token
        v = (torch.randint(0, 2, (E,), generator=g).float() * 2 - 1) * 2.0 ** -5
        pos = stream_order(*shape).float() / N
        ramp = 20.0 * pos if family == "peaky_up" else 30.0 - 20.0 * pos
        ff = 0.1 * ff + ramp[:, None] * v
        qt = (torch.arange(1, rows + 1).float() / rows)[:, None] * v[None, :] / float(v @ v)
        pos_scale = 0.0
        # one window whose whole local weight sits on a single token
        n0 = int(torch.nonzero(R.window_of_token(*shape) == n_windows(*shape) // 2)[3])
        fe[n0] = q_local * (60.0 / i.l_scale / float(q_local @ q_local))
    elif family == "coherent":
        # every q lo plane and every token value positive, half of the tokens zero: a lost lo plane of q moves the logits of the other
        # half by 2^-8.4 relative, all in one direction
        ff = 0.25 * ff.abs() * (stream_order(*shape) % 2 == 0)[:, None]
        qt = torch.full((rows, E), 2.0 ** -5 * (1 + 3 * 2.0 ** -10))
        pos_scale = 0.0
    elif family == "offsets":
        i.t0i, cap = 5, T + 5 + 3
        i.y0i = cap + 4
        i.x0i = i.y0i + H + 7
        P, pos_scale = i.x0i + max(H, W) + 2, 40.0
    elif family in ("bias+", "bias-"):
        i.l_scale, i.l_bias = math.exp(4.6) / 1152, 7.5 if family == "bias+" else -7.5
    elif family == "extremes":
        w0 = torch.nonzero(R.window_of_token(*shape) == 1)[:, 0]
        if form == "f16":
            ff[w0[0], :8] = torch.tensor([65504.0, -65504.0, 2.0 ** -24, -0.0, 65504.0, -2.0 ** -24, 0.0, -65504.0])
            # a tiny query row that only a per-row scale keeps: it looks along the channels where a few tokens are huge
            big = torch.arange(0, N, 7)
            ff[big, 64:128] = 60000.0
            if rows >= 2:
                qt[0] = 0.0
                qt[0, 64:128] = 2.0 ** -30
                qt[1] = qt[1] * 2.0 ** 20 / float(qt[1].abs().max())
            if rows >= 9:
                qt[2] = 0.0
        else:
            ff[w0] = 1e5                                    # local context of window 1 = 1e5 (99840 in bf16): ctx_f16 saturates
            if rows >= 9:
                qt[2] = 0.0
        pos_scale = 0.0 if form == "f16" else 0.5
    i.ff, i.fe = ff.to(dt).view(T, H, W, E), fe.to(dt).view(T, H, W, E)
    qloc = q_local.to(dt)
    i.q_hi, i.q_lo = torch.zeros(16, E, dtype=dt), torch.zeros(16, E, dtype=dt)
    i.q_hi[rows:] = qloc
    i.q_f32 = None
    if form == "f16":
        i.q_hi[:rows], i.q_lo[:rows] = NAN, NAN              # ignored: the global rows come as q_f32
        i.q_f32 = torch.full((16, E), NAN)
        i.q_f32[:rows] = qt
        i.qt = up(i.q_f32[:rows])
    else:
        i.q_hi[:rows], i.q_lo[:rows] = split_tok(qt, dt)
        i.qt = up(i.q_hi[:rows]) + up(i.q_lo[:rows])
    i.q_local = up(qloc)
    i.llog = (up(i.fe).view(N, E) @ i.q_local).float() if form == "logits" else None
    # score-side table and value-side rows: NaN wherever the call may not look (rows >= rows, slots outside the three used ranges)
    used = torch.zeros(P, dtype=torch.bool)
    for a, n in ((i.t0i, T), (i.y0i, H), (i.x0i, W)):
        used[a:a + n] = True
    i.pos_a = torch.full((16, P), NAN)
    pa = pos_scale * rnd(rows, P)
    if family == "offsets":
        pa = pa + torch.linspace(-40, 40, P)[None, :]            # large and distinct per slot
    i.pos_a[:rows] = torch.where(used[None, :], pa, torch.tensor(NAN))
    pe = torch.where(used[:, None], rnd(P, E).clamp(-1, 1), torch.tensor(NAN))
    i.pe_hi, i.pe_lo = split_tok(pe, dt)
    i.used = used
    return i


def ref_args(i, with_pe=True):
    T, H, W, kt, ks = i.shape
    N = T * H * W
    pe = (up(i.pe_hi) + up(i.pe_lo)) if with_pe else None
    kw = dict(pos_a=up(i.pos_a[:i.rows]), pe=pe, t0i=i.t0i, y0i=i.y0i, x0i=i.x0i, value_pe=with_pe)
    if i.form == "logits":
        kw["llog"] = up(i.llog)
    else:
        kw["fe"] = up(i.fe).view(N, E)
    return (up(i.ff).view(N, E), T, H, W, kt, ks, i.q_local, i.l_scale, i.l_bias, i.qt), kw


def ring_reference(i, nparts, with_pe=True, **defect):
    a, kw = ref_args(i, with_pe)
    kw.update(defect)
    return R.fused_ring_ref(*a, nparts=nparts, **kw)


# =============================================================================================================================
# tolerances, from the reference's own quantities
# =============================================================================================================================
def ring_bounds(i, ref, with_pe=True):
    """Tolerance tensors for ctx_local, lse, part_ctx, merged, marg (same shapes as the reference's)."""
    T, H, W, kt, ks = i.shape
    wsz, rows, f16 = kt * ks * ks, i.rows, i.form == "f16"
    plane = EPS23 if f16 else BF16_PLANES                              # weight planes hi + lo, relative
    win, NW = ref["win"], ref["NW"]
    x_abs = up(i.ff).view(-1, E).abs()
    b = {}
    # ---- local ----
    s, m_w = ref["local_s"], ref["local_m"]
    s_ab = abs(i.l_scale) * ref["local_dot_ab"] + abs(i.l_bias)
    dl = 2 * EPS23 * s_ab                                              # the product with l_scale, the sum with l_bias
    if i.form != "logits":
        dl = dl + abs(i.l_scale) * sum_tol(E + 16, ref["local_dot_ab"])      # fe . q: E products, eight slices
    dl = dl + 2 * EPS23 * (s.abs() + m_w[win].abs())                    # s - m, (s - m) log2(e)
    d_w = R._seg_max(dl, win, NW)
    ntile_w = wsz // 16 + 2                                            # tiles a window can straddle
    rel_w = torch.expm1(2 * d_w) + TRANS + plane + (wsz + 2 * ntile_w + 4) * EPS23   # weights | expf | planes | l sum, rescales, 1 / l
    tol = relmul(rel_w[:, None], ref["ctx_local_ab"]) + sum_tol(2 * wsz + 8, ref["ctx_local_ab"])   # ... | P.x over hi and lo planes
    if f16:
        tol = tol + 2.0 ** -39 * torch.zeros(NW, E, dtype=torch.float64).index_add_(0, win, x_abs)   # absolute part of the fp16 weight split
    b["ctx_local"] = tol + 1e-37
    # ---- global ----
    S, S_ab, qx_ab = ref["S"], ref["S_ab"], ref["qx_ab"]
    dS = sum_tol(2 * E + 16, qx_ab) + 4 * EPS23 * S_ab                  # q . x over both planes | the three pos_a terms and their sum
    if f16:
        dS = dS + 2.0 ** -22 * i.qt.abs().max(1).values[:, None] * x_abs.sum(1)[None, :]   # per-row split of q_f32
    # (bf16 forms: the reference takes the hi + lo planes of q as given: no split term)
    nparts = len(ref["part_tokens"])
    d_p = torch.zeros(nparts, rows, dtype=torch.float64)
    eps_l, rel_p = torch.zeros_like(d_p), torch.zeros_like(d_p)
    k_p = torch.zeros(nparts, dtype=torch.float64)
    abs16 = torch.zeros(nparts, E, dtype=torch.float64)
    pe_abs = (up(i.pe_hi) + up(i.pe_lo))[i.used].abs().sum(0) if with_pe else 0.0
    for p, idx in enumerate(ref["part_tokens"]):
        Sp = S[:, idx]
        M = Sp.max(1, keepdim=True).values
        d_p[p] = (dS[:, idx] + 2 * EPS23 * (Sp.abs() + M.abs())).max(1).values      # ... | s - m, (s - m) log2(e)
        ntok, ntile = idx.numel(), (idx.numel() + 15) // 16
        # l: expf and one rounding per token, per tile the rescale factor (expf, its argument, the product)
        eps_l[p] = TRANS + ntok * EPS23 + ntile * (TRANS + 2 * EPS23) + 2 * EPS23 * (M - Sp.min(1, keepdim=True).values)[:, 0]
        rel_p[p] = torch.expm1(2 * d_p[p]) + TRANS + plane + (ntok + 2 * ntile + 4) * EPS23
        k_p[p] = 2 * (ntok + 64) + 16                                    # P.x terms: hi and lo planes of the tokens and of <= 64 pe slots
        if f16:
            abs16[p] = 2.0 ** -39 * x_abs[idx].sum(0) + 2.0 ** -29 * pe_abs            # fp16 split of the weights | of the marginals at 2^4
    b["lse"] = d_p + eps_l
    b["part_ctx"] = relmul(rel_p[:, :, None], ref["part_ctx_ab"]) + sum_tol(k_p[:, None, None], ref["part_ctx_ab"]) + abs16[:, None, :] + 1e-37
    b["merged"] = relmul(rel_p.max(0).values[:, None], ref["merged_ab"]) + sum_tol(float(k_p.max()), ref["merged_ab"]) + abs16.max(0).values[None, :] + 1e-37
    b["marg"] = relmul(rel_p[:, :, None], ref["marg"]) + sum_tol((k_p - 128)[:, None, None], ref["marg"]) + F16_RND * ref["marg"] + F16_SUB
    return b


def relmul(rel, ab):
    """rel * ab with 0 where ab is exactly 0 (a structural zero stays one however large the relative bound, inf included)."""
    return torch.where(ab == 0, torch.zeros_like(ab), rel * ab)


def f16_out(tol, ref):
    return tol + F16_RND * ref.abs() + F16_SUB


FAMILY_CASES = [(fam, s, r, f) for fam in FAMILIES[1:] for (s, r) in (((8, 6, 6, 4, 3), 9), ((12, 9, 6, 4, 3), 12), ((8, 8, 8, 4, 4), 2), ((4, 4, 8, 1, 4), 9))
                for f in FORMS]
