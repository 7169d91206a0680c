"""Operator-level tests (GPU) of the entry points that were reached only through a whole forward() / backward(): each native.py
wrapper on its own against the float64 restatement of its formula in tests/ops_reference.py, computed from the values the kernel
received (bf16 / fp16 / f32 inputs up-cast, never regenerated), at the shapes, dtypes and edges where such kernels go wrong.

Tolerances are derived, not tuned (one line at each check):
  casts / copies / integer-valued sums                  bit-exact
  f32 result of a K-term fp32 sum                       K 2^-23 sum|terms|          (ops_reference.sum_tol, |terms| from the reference)
  result rounded to bf16 / fp16                         + 2^-8 |ref|  /  + 2^-10 |ref| (+ 2^-24 where fp16 subnormals occur)
  a device transcendental (expf, erf) in the path       + 2^-21 relative on that factor
Every check prints `OPS_SMALL <name> err=<largest error> bound=<bound there> ratio=<largest error / bound>` before it asserts."""
import math
from types import SimpleNamespace

import pytest
import torch

import ops_reference as R
from ops_reference import EPS23, sum_tol, up
from hicom_amd import geometry as geo
from hicom_amd import native as nv

pytestmark = pytest.mark.gpu

BF16_RND, F16_RND, F16_SUB, TRANS = 2.0 ** -8, 2.0 ** -10, 2.0 ** -24, 2.0 ** -21
NAN = float("nan")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def nan_like(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def check(name, got, ref, tol):
    """|got - ref| <= tol elementwise (float64 on the CPU); the figures are printed first."""
    got, ref = up(got), ref.double()
    tol = torch.broadcast_to(tol.double(), ref.shape) if torch.is_tensor(tol) else torch.full_like(ref, float(tol))
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values in the result"
    err = (got - ref).abs()
    ratio = err / tol.clamp_min(1e-300)
    i = int(ratio.argmax())
    print(f"OPS_SMALL {name} err={float(err.max()):.3e} bound={float(tol.reshape(-1)[i]):.3e} ratio={float(ratio.reshape(-1)[i]):.3e}")
    assert bool((err <= tol).all()), f"{name}: error {float(err.reshape(-1)[i]):.3e} over its bound {float(tol.reshape(-1)[i]):.3e}"


def split_planes(x, rows_pad):
    """bf16 hi / lo planes of f32 rows on the CPU (operands of the stream kernels), zero rows up to rows_pad."""
    hi = torch.zeros(rows_pad, x.shape[1], dtype=torch.bfloat16)
    lo = torch.zeros_like(hi)
    hi[:x.shape[0]] = x.bfloat16()
    lo[:x.shape[0]] = (x - hi[:x.shape[0]].float()).bfloat16()
    return hi, lo


# =============================================================================================================================
# hicom_global_dx_fwd
# =============================================================================================================================
def _global_dx_inputs(rows, E, N, stride, seed, peaky=False):
    g = gen(seed)
    S = torch.full((16, stride), NAN)                       # padding rows and columns are never read: NaN proves it
    dS = torch.full((16, stride), NAN)
    s = torch.randn(rows, N, generator=g) * (30.0 if peaky else 3.0)
    if peaky:
        s[:, N // 2] += 120.0                               # S - M spans far more than 80: expf underflows for most tokens
    S[:rows, :N] = s
    dS[:rows, :N] = torch.randn(rows, N, generator=g) * 0.1
    M = s.double().max(1).values
    ml = torch.stack([M, torch.exp(s.double() - M[:, None]).sum(1)], 1).float().contiguous()
    qt, dctx = torch.randn(rows, E, generator=g), torch.randn(rows, E, generator=g)
    dx0 = torch.randn(N, E, generator=g).bfloat16()
    return S, dS, ml, qt, dctx, dx0


def _global_dx_check(name, rows, E, N, stride, accumulate, seed, peaky=False):
    S, dS, ml, qt, dctx, dx0 = _global_dx_inputs(rows, E, N, stride, seed, peaky)
    dx = dx0.cuda() if accumulate else nan_like((N, E), torch.bfloat16)      # accumulate = 0: overwritten, never read
    nv.global_dx(S.cuda(), dS.cuda(), ml.cuda(), qt.cuda(), dctx.cuda(), N, dx, accumulate)
    torch.cuda.synchronize()
    ref, ab, p = R.global_dx_ref(up(S), up(dS), up(ml), up(qt), up(dctx), N, up(dx0) if accumulate else None)
    # chain of 2 rows FMAs (+ the old value) in fp32; the softmax weight carries expf (2^-21), the rounding of S - M (2^-24 |S - M|
    # in the exponent) and the division; then one rounding to bf16
    span = (up(S)[:rows, :N] - up(ml)[:, 0:1]).abs()
    p_rel = TRANS + 2 * EPS23 + 2.0 ** -24 * span
    tol = sum_tol(2 * rows + 1, ab) + (p * p_rel).t() @ up(dctx).abs() + BF16_RND * ref.abs() + 1e-37
    check(name, dx, ref, tol)


@pytest.mark.parametrize("E", [768, 1024, 1152, 1280, 100])
@pytest.mark.parametrize("rows", [1, 6, 8, 9, 10, 12, 16])
def test_global_dx_matches_fp64_reference(rows, E):
    """Every row count of both instantiations (<= 9 and <= 16), E with a ragged last thread group, token counts around the 64-token
    workgroup, padded score rows (NaN in the padding), overwrite (NaN in dx) and accumulate."""
    for N in (1, 63, 64, 65, 729 * 4 + 5):
        for stride in (N, (N + 15) // 16 * 16 + 16):
            for accumulate in (0, 1):
                _global_dx_check(f"global_dx[r{rows},E{E},N{N},s{stride},a{accumulate}]", rows, E, N, stride, accumulate,
                                 seed=rows * 7919 + E + N + accumulate)


@pytest.mark.parametrize("rows,E", [(6, 768), (9, 1152), (10, 1280)])
def test_global_dx_peaky_scores_underflow_to_zero_weights(rows, E):
    for accumulate in (0, 1):
        _global_dx_check(f"global_dx_peaky[r{rows},E{E},a{accumulate}]", rows, E, 700, 704, accumulate, seed=rows, peaky=True)


def test_global_dx_refuses_unsupported_arguments():
    """No launch happens for any of these: the entry point returns an error code."""
    def call(rows, E, misalign=False):
        N = 8
        z = lambda *s: torch.zeros(*s, device="cuda")
        dx = torch.zeros(N * E + 8, dtype=torch.bfloat16, device="cuda")
        dx = (dx[1:1 + N * E] if misalign else dx[:N * E]).view(N, E)
        nv.global_dx(z(32, 16), z(32, 16), z(rows, 2) + 1, z(rows, E), z(rows, E), N, dx, 0)
    call(16, 1280)                                           # the largest supported shape goes through
    for kw in (dict(rows=17, E=768), dict(rows=6, E=1284), dict(rows=6, E=1282), dict(rows=6, E=768, misalign=True)):
        with pytest.raises(nv.HicomNativeError):
            call(**kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows,E", [(6, 768), (10, 1280)])
def test_global_dx_does_not_read_stale_lds(rows, E):
    """The kernel's coefficient table has RMAX = 9 / 16 rows per token; with fewer folded rows the unrolled FMA loop used to read the
    unwritten ones (times the zeroed weights): stale Inf / NaN in LDS became NaN in d frames_feature.  Here the launch directly in
    front of it on the stream is hicom_partials_sum_fwd in its tall form over all-NaN partials -- 4096 workgroups, so every CU runs
    some -- whose red[16][17] at the start of LDS overlaps the table of each workgroup's first tokens.  The poison is plain data in a
    tensor of this test.  Measured once against the kernel as it was before the table was zero-filled (the previous small_ops.hip, same
    inputs, MI355X): this test FAILED there -- 17405 of 19205 token rows non-finite at rows = 6 / E = 768, 17164 of 19205 at rows = 10 /
    E = 1280 -- so the poison does land where expected.  The fixed kernel must return finite values equal to the reference."""
    N = 64 * 300 + 5
    S, dS, ml, qt, dctx, _ = _global_dx_inputs(rows, E, N, N, seed=rows + E)
    poison = nan_like((64, 65536), torch.float32)
    sink = torch.empty(65536, device="cuda")
    dev = [t.cuda() for t in (S, dS, ml, qt, dctx)]
    dx = nan_like((N, E), torch.bfloat16)
    torch.cuda.synchronize()
    nv.partials_sum(poison, sink)
    nv.global_dx(*dev, N, dx, 0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(sink).all())                     # the poisoning launch did run in its NaN-carrying form
    n_bad = int((~torch.isfinite(dx.float())).any(1).sum())
    print(f"OPS_SMALL global_dx_stale_lds[r{rows},E{E}] non-finite token rows: {n_bad} of {N}")
    assert n_bad == 0
    ref, ab, p = R.global_dx_ref(up(S), up(dS), up(ml), up(qt), up(dctx), N)
    span = (up(S)[:rows, :N] - up(ml)[:, 0:1]).abs()
    # as in _global_dx_check: 2 rows FMAs, expf + rounding of S - M + division on the weight, one rounding to bf16
    tol = sum_tol(2 * rows + 1, ab) + (p * (TRANS + 2 * EPS23 + 2.0 ** -24 * span)).t() @ up(dctx).abs() + BF16_RND * ref.abs() + 1e-37
    check(f"global_dx_after_poison[r{rows},E{E}]", dx, ref, tol)


# =============================================================================================================================
# clip-scale global stage: hicom_clip_query_prep_fwd, hicom_inv_norm_fwd, hicom_global_stream_clip_fwd (+ hicom_global_merge_fwd)
# =============================================================================================================================
@pytest.mark.parametrize("with_bk", [False, True])
@pytest.mark.parametrize("nq,nh,E", [(32, 9, 1152), (1, 6, 768), (5, 1, 1152), (32, 10, 1280), (3, 8, 1024)])
def test_clip_query_prep_matches_fp64_reference(nq, nh, E, with_bk):
    g = gen(nq * 31 + nh)
    qp0 = torch.randn(nq, E, generator=g) * 3.0
    b_k = (torch.randn(E, generator=g) * 0.5).bfloat16() if with_bk else None
    scale = math.exp(4.6)
    qp, c = qp0.cuda(), nan_like((nq * nh,), torch.float32)
    nv.clip_query_prep(qp, b_k.cuda() if with_bk else None, nh, scale, c)
    torch.cuda.synchronize()
    qhat, cref, cab = R.clip_query_prep_ref(up(qp0), up(b_k) if with_bk else None, nh, scale)
    # E-term sum of squares (the square root halves its relative error), then sqrt, division, product: E + 4 roundings at most
    rel_q = (E + 4) * EPS23
    check(f"clip_query_prep.qhat[{nq},{nh},{E}]", qp, qhat, rel_q * qhat.abs())
    if with_bk:
        # hd-term dot of the (already inexact) normalised row with b_k, times scale
        check(f"clip_query_prep.c[{nq},{nh},{E}]", c, cref, sum_tol(E // nh + 2, cab) + rel_q * cab)
    else:
        assert bool((c == 0).all())                          # no key bias: the constant is exactly zero (and written)


@pytest.mark.parametrize("M", [1, 255, 256, 257, 46656])
@pytest.mark.parametrize("parts", [1, 3, 18])
def test_inv_norm_matches_fp64_reference(parts, M):
    g = gen(parts * 1000 + M)
    ssq = torch.rand(parts, M, generator=g) * 50 + 0.01
    ssq[:, M // 2] = 1.0e-40 / parts                         # a column whose sum is denormal-small but positive
    if M > 1:
        ssq[:, 0] *= 1.0e6
    inv = nan_like((M,), torch.float32)
    nv.inv_norm(ssq.cuda(), inv)
    torch.cuda.synchronize()
    ref = R.inv_norm_ref(up(ssq))
    # parts-term sum of positive terms (relative parts 2^-23, halved by the square root), square root and division
    check(f"inv_norm[{parts},{M}]", inv, ref, (parts + 3) * EPS23 * ref)
    assert float(up(ssq).sum(0)[M // 2]) < 2.0 ** -126 and float(inv[M // 2]) > 1e19


@pytest.mark.parametrize("T,H,W,R_,E", [(8, 6, 6, 9, 1152), (4, 7, 5, 27, 1152), (8, 6, 6, 18, 1152), (2, 27, 27, 9, 1152),
                                        (4, 7, 5, 33, 1152), (3, 5, 7, 16, 768), (2, 9, 9, 5, 768)])
def test_global_stream_clip_and_merge_match_fp64_clip_attention(T, H, W, R_, E):
    """logit = (q . x + pos + row_const) / ||key||, peaky (clip scale: |logit| up to ~100), through hicom_global_merge_fwd: the
    scores and the merged, normalised contexts (value-side pos-emb included) against float64 attention over the folded form."""
    g = gen(T * 1000 + R_)
    N, rows_pad = T * H * W, (R_ + 15) // 16 * 16
    cap = T + 3
    P = cap + H + W
    x = torch.randn(N, E, generator=g).bfloat16()
    q = torch.randn(R_, E, generator=g) * 25.0
    qhi, qlo = split_planes(q, rows_pad)
    pe = torch.randn(P, E, generator=g) * 0.5
    pos_a = torch.zeros(rows_pad, P)
    pos_a[:R_] = torch.randn(R_, P, generator=g) * 40.0
    inv = torch.rand(N, generator=g) * 0.02 + 0.02
    row_const = torch.zeros(rows_pad)
    row_const[:R_] = torch.randn(R_, generator=g) * 30.0
    qd = up(qhi)[:R_] + up(qlo)[:R_]                           # what the kernel's two planes hold
    S, ctx_ref, ab, vab = R.clip_attention_ref(qd, up(x), up(inv), up(row_const)[:R_], up(pos_a)[:R_], up(pe), H, W, 0, cap, cap + H)
    assert float(S.abs().max()) > 60.0                         # clip-scale magnitudes
    dev = {k: v.cuda() for k, v in dict(x=x, qhi=qhi, qlo=qlo, pos_a=pos_a, inv=inv, rc=row_const, pe=pe).items()}
    stride = (N + 15) // 16 * 16
    for nparts in (1, 3, nv.global_stream_nparts(N, rows_pad)):
        scores = nan_like((rows_pad, stride), torch.float32)
        pm, pl, pacc = (nan_like(s, torch.float32) for s in ((nparts, rows_pad), (nparts, rows_pad), (nparts, rows_pad, E)))
        nv.global_stream_clip(dev["x"], N, dev["qhi"], dev["qlo"], dev["pos_a"], H, W, 0, cap, cap + H, dev["inv"], dev["rc"], scores,
                              pm, pl, pacc, R_)
        ml, acc = nan_like((R_, 2), torch.float32), nan_like((R_, E), torch.float32)
        scratch = torch.empty(R_ * T * (H + W + 2), device="cuda")
        nv.global_merge(pm, pl, pacc, R_, scores, N, H, W, dev["pe"], 0, cap, cap + H, scratch, ml, acc, normalize=True)
        torch.cuda.synchronize()
        # matrix-core dot products over both planes: 2 E products accumulated in fp32, + 3 positional terms, the constant, the scaling
        s_tol = sum_tol(2 * E + 6, ab)
        check(f"global_stream_clip.scores[{T},{H},{W},{R_},{E},p{nparts}]", scores[:R_, :N], S, s_tol)
        # contexts: a logit error d changes every softmax weight by at most e^(2 d) - 1 relative; then N weights (expf: 2^-21) times
        # values summed in fp32 over chunks and partials, and the division by L
        d = s_tol.max(1, keepdim=True).values
        c_rel = torch.expm1(2 * d) + (N + nparts + 8) * EPS23 + 2 * TRANS
        check(f"global_merge.ctx[{T},{H},{W},{R_},{E},p{nparts}]", acc, ctx_ref, c_rel * vab)
        # the same contexts against float64 attention over the logits the kernel itself wrote (checked above): no logit error left,
        # only expf (2^-21 on the weight and on L), the rounding of S - M, and the fp32 sums
        Sk = up(scores)[:R_, :N]
        pk = torch.softmax(Sk, 1)
        t, y, xx = R.token_axes(N, H, W)
        val = up(x) + up(pe)[t] + up(pe)[cap + y] + up(pe)[cap + H + xx]
        vabs = up(x).abs() + up(pe)[t].abs() + up(pe)[cap + y].abs() + up(pe)[cap + H + xx].abs()      # (token and pos-emb parts: separate sums)
        span = float((Sk.max(1, keepdim=True).values - Sk).max())
        k_rel = (N + nparts + 8) * EPS23 + 2 * TRANS + 2.0 ** -23 * min(span, 104.0)      # (weights below e^-104 are zero in fp32)
        check(f"global_merge.ctx_from_written_scores[{T},{H},{W},{R_},{E},p{nparts}]", acc, pk @ val, k_rel * (pk @ vabs))
        # the softmax state (M, L) enters everything behind it as M + log L: N-term sum of expf values, one log, one addition
        lse = torch.logsumexp(Sk, 1)
        check(f"global_merge.ml[{R_},p{nparts}]", up(ml)[:, 0] + torch.log(up(ml)[:, 1]), lse, k_rel + 2 * EPS23 * lse.abs())


@pytest.mark.parametrize("E", [1152, 768])
def test_global_stream_bwd_ds_out_matches_fp64_reference(E):
    """hicom_global_stream_bwd as the direct recipe calls it (no positional table: H = 1, W = N; no marginals): ds_out elementwise,
    dS[r, n] = exp(S[r, n] - M_r) / L_r (dctx_r . x_n - delta_r)."""
    g = gen(E)
    N, R_ = 729 * 4 + 5, 9
    stride = (N + 15) // 16 * 16
    x = torch.randn(N, E, generator=g).bfloat16()
    dctx = torch.randn(R_, E, generator=g) * 0.05
    dhi, dlo = split_planes(dctx, 16)
    s_in = torch.zeros(16, stride)
    s_in[:R_, :N] = torch.randn(R_, N, generator=g) * 3
    Sd = up(s_in)[:R_, :N]
    Md = Sd.max(1).values
    ml = torch.stack([Md, torch.exp(Sd - Md[:, None]).sum(1)], 1).float().contiguous()
    delta = torch.randn(R_, generator=g) * 0.1
    nparts = nv.global_stream_nparts(N, 16)
    ds, part = nan_like((16, stride), torch.float32), torch.empty(nparts, 16, E, device="cuda")
    nv.global_stream_bwd(x.cuda(), N, dhi.cuda(), dlo.cuda(), None, 1, N, 0, 0, 0, s_in.cuda(), ml.cuda(), delta.cuda(), ds, part, R_)
    torch.cuda.synchronize()
    gd = up(dhi)[:R_] + up(dlo)[:R_]
    p = torch.exp(Sd - up(ml)[:, 0:1]) / up(ml)[:, 1:2]
    dP, dP_ab = gd @ up(x).t(), gd.abs() @ up(x).abs().t()
    ref = p * (dP - up(delta)[:, None])
    # 2 E products on the matrix cores in fp32 + the subtraction; the weight carries expf, the rounding of S - M and the division
    p_rel = TRANS + 2 * EPS23 + 2.0 ** -24 * (Sd - up(ml)[:, 0:1]).abs()
    tol = p * sum_tol(2 * E + 2, dP_ab + up(delta).abs()[:, None]) + p_rel * ref.abs() + EPS23 * ref.abs()
    check(f"global_stream_bwd.ds_out[{E}]", ds[:R_, :N], ref, tol)


# =============================================================================================================================
# row operators over the token stream: hicom_l2norm_stream_fwd, hicom_ln_stream_fwd
# =============================================================================================================================
@pytest.mark.parametrize("M", [1, 7, 4097])
@pytest.mark.parametrize("E", [768, 1152, 1536, 8])
def test_l2norm_stream_matches_fp64_reference(E, M):
    x = (torch.randn(M, E, generator=gen(E + M)) * 2.0).bfloat16()
    out = nan_like((M, E), torch.bfloat16)
    nv.l2norm_stream(x.cuda(), out)
    torch.cuda.synchronize()
    ref = R.l2norm_ref(up(x))
    # E-term sum of squares (halved by the square root) + sqrt, division, product; one rounding to bf16
    check(f"l2norm_stream[{E},{M}]", out, ref, ((E + 4) * EPS23 + BF16_RND) * ref.abs())


@pytest.mark.parametrize("M", [1, 7, 4097])
@pytest.mark.parametrize("E", [768, 1152, 1536, 8])
def test_ln_stream_matches_fp64_reference(E, M):
    """x fp16 / bf16 / f32, dense and pitched (NaN in the pitch padding), with and without the alpha blend, fp16 and bf16 outputs; row 0
    is constant (variance 0: only eps in the denominator)."""
    g = gen(E * 3 + M)
    eps = 1e-6
    gamma, beta = (1 + 0.2 * torch.randn(E, generator=g)).bfloat16(), (0.3 * torch.randn(E, generator=g)).bfloat16()
    src = torch.randn(M, E, generator=g).bfloat16()
    base = torch.randn(M, E, generator=g) * 1.7 + 0.4
    base[0] = 3.0
    for x_dt in (torch.float16, torch.bfloat16, torch.float32):
        for ldx in (E, E + 8):
            x = torch.full((M, ldx), NAN, dtype=x_dt)
            x[:, :E] = base.to(x_dt)
            xd = up(x)[:, :E]
            for blend, alpha_dt in ((False, None), (True, torch.bfloat16), (True, torch.float32)):
                alpha = torch.tensor([0.4], dtype=alpha_dt) if blend else None
                a = float(alpha.double()) if blend else 1.0
                ref, ab = R.ln_blend_ref(xd, up(gamma), up(beta), up(src) if blend else None, a, eps)
                # LayerNorm in fp32 (ops_reference.ln_fp32_tol), scaled by alpha; 3 more roundings for the blend
                tol32 = a * R.ln_fp32_tol(xd, up(gamma), up(beta), eps) + 3 * EPS23 * ab
                for out_dt, rnd in ((torch.float16, F16_RND), (torch.bfloat16, BF16_RND)):
                    out = nan_like((M, E), out_dt)
                    nv.ln_stream(x.cuda(), gamma.cuda(), beta.cuda(), out, src.cuda() if blend else None, alpha.cuda() if blend else None, eps)
                    torch.cuda.synchronize()
                    sub = F16_SUB if out_dt == torch.float16 else 0.0
                    check(f"ln_stream[{E},{M},{x_dt},ld{ldx},blend{alpha_dt},{out_dt}]", out, ref, tol32 + rnd * ref.abs() + sub)


@pytest.mark.parametrize("E", [1544, 12])
def test_l2norm_and_ln_stream_refuse_unsupported_widths(E):
    x = torch.zeros(4, E, dtype=torch.bfloat16, device="cuda")
    gb = torch.zeros(E, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(nv.HicomNativeError):
        nv.l2norm_stream(x, torch.empty_like(x))
    with pytest.raises(nv.HicomNativeError):
        nv.ln_stream(x, gb, gb, torch.empty_like(x))


# =============================================================================================================================
# hicom_small_mha_scaled_fwd
# =============================================================================================================================
@pytest.mark.parametrize("M,L,nh,hd", [(21, 64, 9, 128), (1296, 64, 9, 128), (100, 37, 12, 64), (70, 5, 6, 96), (65, 64, 3, 256)])
def test_small_mha_scaled_clip_logits_match_fp64_reference(M, L, nh, hd):
    """L2-normalised projected states and scale = exp(4.6): every second query row repeats a key whose mass sits in head 0, so that
    head's logits reach ~100 -- an unsafe softmax overflows there."""
    g = gen(M + L)
    E = nh * hd
    k, v = torch.randn(L, E, generator=g), torch.randn(L, E, generator=g) * 0.3
    k[::2, :hd] *= 12.0
    q = torch.randn(M, E, generator=g)
    idx = torch.arange(0, M, 2)
    q[idx] = k[(idx // 2 * 2) % L] + 0.05 * torch.randn(len(idx), E, generator=g)
    q, k = q / q.norm(dim=1, keepdim=True), k / k.norm(dim=1, keepdim=True)
    scale = math.exp(4.6)
    out = nan_like((M, E), torch.float32)
    nv.small_mha(q.cuda(), k.cuda(), v.cuda(), nh, out, scale=scale)
    torch.cuda.synchronize()
    ref, ab, sab = R.small_mha_ref(up(q), up(k), up(v), nh, scale)
    assert float((up(q)[:, :hd] @ up(k)[:, :hd].t()).max()) * scale > 85.0
    # logits: hd-term dot + scaling; a logit error d changes every weight by at most e^(2 d) - 1; expf on the weight and on the sum;
    # L weights times values summed in fp32
    d = sum_tol(hd + 2, sab).max(-1).values.permute(1, 0)                   # [M, nh]
    rel = (torch.expm1(2 * d) + (L + 4) * EPS23 + 2 * TRANS).repeat_interleave(hd, dim=1)
    check(f"small_mha_scaled[{M},{L},{nh},{hd}]", out, ref, rel * ab)


# =============================================================================================================================
# adaptor backward: hicom_local_attn_adapt_bwd, hicom_adapt_dy_fwd, hicom_gelu_bwd_fwd, hicom_gelu_split_fwd, hicom_colsum_fwd
# =============================================================================================================================
def _axes(T, H, W, kt, ks):
    tiles = (geo.axis_tiling(T, kt), geo.axis_tiling(H, ks), geo.axis_tiling(W, ks))
    return tuple(nv.Axis(a.n, a.k, a.nwin, a.nfull) for a in tiles), tiles[0].nwin * tiles[1].nwin * tiles[2].nwin


def _adapt_streams(T, H, W, D, g):
    N = T * H * W
    kx, vx = torch.randn(N, D, generator=g).bfloat16(), torch.randn(N, D, generator=g).bfloat16()
    ky, vy = (torch.randn(N, D, generator=g) * 1.5 + 0.3).half(), (torch.randn(N, D, generator=g) * 0.7 - 0.2).half()
    norms = [SimpleNamespace(weight=(1 + 0.1 * torch.randn(D, generator=g)).bfloat16().cuda(),
                             bias=(0.1 * torch.randn(D, generator=g)).bfloat16().cuda()) for _ in range(2)]
    return kx, ky, vx, vy, norms


@pytest.mark.parametrize("D", [1152, 768])
@pytest.mark.parametrize("which", ["both", "key", "value"])
@pytest.mark.parametrize("T,H,W,kt,ks", [(4, 6, 6, 4, 3), (8, 6, 9, 4, 3), (1, 4, 4, 1, 2)])
def test_local_attn_adapt_bwd_matches_fp64_reference(T, H, W, kt, ks, which, D):
    """All six outputs, adaptor on the key stream, the value stream or both; bf16 and f32 queries, shared and per window."""
    g = gen(T * 100 + H + D)
    axes, nw = _axes(T, H, W, kt, ks)
    N = T * H * W
    kx, ky, vx, vy, norms = _adapt_streams(T, H, W, D, g)
    ak, av = torch.tensor([0.4]).bfloat16(), torch.tensor([0.7]).bfloat16()
    use_k, use_v = which in ("both", "key"), which in ("both", "value")
    dctx = torch.randn(nw, D, generator=g)
    win = R.window_of_token(T, H, W, kt, ks)
    WIN = N // nw
    scale, bias = 1.0 / math.sqrt(D), 0.25
    for q_dt in (torch.bfloat16, torch.float32):
        for shared in (True, False):
            q = torch.randn(1 if shared else nw, D, generator=g).to(q_dt)
            ds, pw = nan_like((N,), torch.float32), nan_like((N,), torch.float32)
            sx = {k: nan_like((nw, D), torch.float32) for k in ("sxk", "syk", "sxv", "syv")}
            nv.local_attn_adapt_bwd(kx.cuda(), ky.cuda() if use_k else None, norms[0] if use_k else None, ak.cuda() if use_k else None,
                                    vx.cuda(), vy.cuda() if use_v else None, norms[1] if use_v else None, av.cuda() if use_v else None,
                                    axes, q.cuda().reshape(-1) if shared else q.cuda(), 0 if shared else D, scale, bias, dctx.cuda(),
                                    ds, pw, sx["sxk"], sx["syk"] if use_k else None, sx["sxv"], sx["syv"] if use_v else None)
            torch.cuda.synchronize()
            qd = up(q).expand(nw, D) if shared else up(q)
            out, ab = R.adapt_bwd_ref(up(kx), up(ky) if use_k else None, up(norms[0].weight), up(norms[0].bias), float(ak.double()),
                                      up(vx), up(vy) if use_v else None, up(norms[1].weight), up(norms[1].bias), float(av.double()),
                                      win, nw, qd, scale, bias, up(dctx))
            tag = f"[{T},{H},{W},{which},{D},{q_dt},shared{shared}]"
            # logits and dP: four chained D-term fp32 sums (LayerNorm mean and variance, the x and the y dot product) bounded together
            # by 4 D 2^-23 times the absolute terms of the blended expression
            d_s, d_P = sum_tol(4 * D, ab["s"]), sum_tol(4 * D, ab["dP"])
            wmax = lambda v: torch.zeros(nw, dtype=torch.float64).scatter_reduce(0, win, v, "amax")[win]
            wsum = lambda v: torch.zeros(nw, dtype=torch.float64).index_add_(0, win, v)[win]
            # softmax weight: a logit error d moves it by e^(2 d) - 1 relative; expf (2^-21, numerator and denominator); WIN-term sum
            p_rel = torch.expm1(2 * wmax(d_s)) + 2 * TRANS + (WIN + 2) * EPS23
            p = out["pw"]
            check("adapt_bwd.pw" + tag, pw, p, p_rel * p)
            # ds = scale p (dP - delta), delta = sum p dP over the window: weight error on both terms, dP error on both, 4 roundings
            V = R.blend_rows(up(vx), up(vy) if use_v else None, up(norms[1].weight), up(norms[1].bias), float(av.double()), 1e-6)[0]
            dP = (V * up(dctx)[win]).sum(1)
            mag = dP.abs() + wsum(p * dP.abs())
            ds_tol = scale * ((p_rel + 4 * EPS23) * p * mag + p * (d_P + wsum(p * d_P)) + p * wsum(p * p_rel * dP.abs()))
            check("adapt_bwd.ds" + tag, ds, out["ds"], ds_tol)
            # weighted sums over the window: the coefficient's error times |row|, WIN-term fp32 sum (+ 4-way reduction); the normalised
            # rows yhat carry the LayerNorm statistics' error 2 D 2^-23 (|y| + |mu|) rstd
            def wrows(c, rows):
                return torch.zeros(nw, D, dtype=torch.float64).index_add_(0, win, c[:, None] * rows)
            for name, coef, ctol, rows, y in (("sxk", out["ds"], ds_tol, up(kx), None), ("syk", out["ds"], ds_tol, None, up(ky)),
                                              ("sxv", p, p_rel * p, up(vx), None), ("syv", p, p_rel * p, None, up(vy))):
                if name not in out:
                    continue
                if y is not None:
                    mu, rstd = R.layer_norm_stats(y, 1e-6)
                    rows = ((y - mu) * rstd)
                    drow = 2 * D * EPS23 * (y.abs() + mu.abs()) * rstd
                else:
                    drow = torch.zeros_like(rows)
                tol = wrows(ctol, rows.abs()) + wrows(coef.abs(), drow) + sum_tol(WIN + 4, ab[name])
                check(f"adapt_bwd.{name}" + tag, sx[name], out[name], tol)


def test_local_attn_adapt_bwd_refuses_an_inexact_partition():
    g = gen(7)
    T, H, W, D = 7, 6, 6, 1152
    axes, nw = _axes(T, H, W, 4, 3)
    kx, ky, vx, vy, norms = _adapt_streams(T, H, W, D, g)
    a = torch.tensor([0.5]).bfloat16().cuda()
    N = T * H * W
    f = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(nv.HicomNativeError):
        nv.local_attn_adapt_bwd(kx.cuda(), ky.cuda(), norms[0], a, vx.cuda(), vy.cuda(), norms[1], a, axes, f(D).bfloat16(), 0, 0.03, 0.0,
                                f(nw, D), f(N), f(N), f(nw, D), f(nw, D), f(nw, D), f(nw, D))


@pytest.mark.parametrize("shared_bf16_vec", [False, True])
@pytest.mark.parametrize("D", [1152, 768])
def test_adapt_dy_matches_fp64_reference_elementwise(D, shared_bf16_vec):
    """dy (bf16) and r1 (given and NULL) elementwise; vec f32 per window and bf16 shared; the column sums of the same launch."""
    g = gen(D + 5)
    T, H, W, kt, ks = 8, 6, 6, 4, 3
    axes, nw = _axes(T, H, W, kt, ks)
    N = T * H * W
    win = R.window_of_token(T, H, W, kt, ks)
    y = (torch.randn(N, D, generator=g) * 1.3 + 0.2).half()
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).bfloat16()
    vec = torch.randn(1, D, generator=g).bfloat16() if shared_bf16_vec else torch.randn(nw, D, generator=g)
    coef = torch.randn(N, generator=g)
    alpha = torch.tensor([0.4]).bfloat16()
    a = float(alpha.double())
    vec_tok = up(vec).expand(nw, D)[win] if shared_bf16_vec else up(vec)[win]
    ref, r1_ref, ab = R.adapt_dy_ref(up(y), up(gamma), vec_tok, up(coef), a)
    # four chained D-term fp32 sums (mean, variance, mean(g), mean(g yhat)) bounded together on the absolute terms; one rounding to bf16
    tol = sum_tol(4 * D, ab) + BF16_RND * ref.abs()
    dev = [t.cuda() for t in (y, gamma, vec.reshape(-1) if shared_bf16_vec else vec, coef, alpha)]
    stride = 0 if shared_bf16_vec else D
    for with_r1 in (False, True):
        for colsum in (False, True):
            dy = nan_like((N, D), torch.bfloat16)
            r1 = nan_like((N, D), torch.bfloat16) if with_r1 else None
            cs = nv.adapt_dy(dev[0], dev[1], dev[2], stride, dev[3], dev[4], axes, dy, r1=r1, colsum=colsum)
            torch.cuda.synchronize()
            check(f"adapt_dy.dy[{D},sharedvec{shared_bf16_vec},r1{with_r1},cs{colsum}]", dy, ref, tol)
            if with_r1:
                # (1 - alpha) coef vec: three fp32 roundings, one to bf16
                check(f"adapt_dy.r1[{D},sharedvec{shared_bf16_vec}]", r1, r1_ref, (3 * EPS23 + BF16_RND) * r1_ref.abs())
            if colsum:
                # column sums of dy AS STORED: an N-term fp32 sum of the written bf16 values
                check(f"adapt_dy.colsum[{D}]", cs, up(dy).sum(0), sum_tol(N, up(dy).abs().sum(0)))


def _gelu_edge_values():
    return torch.tensor([65504.0, -65504.0, 0.0, -0.0, -10.0, 10.0, -5.0, 5.0, -3.0, 0.1, -0.1, 6.1e-5, -6.0e-8, 1.0, -1.0, 0.70703125])


def test_gelu_bwd_matches_fp64_reference_elementwise():
    """da *= GELU'(h) in place, elementwise: the plain form on a length that is no multiple of D, and the row form with column sums."""
    g = gen(21)
    for shape, colsum in (((1000, 8), False), ((16 * 36 + 3, 1152), True), ((35, 768), True), ((35, 768), False)):
        h = (torch.randn(shape, generator=g) * 2.0).half()
        h.view(-1)[:16] = _gelu_edge_values().half()
        da0 = torch.randn(shape, generator=g).bfloat16()
        da = da0.cuda()
        cs = nv.gelu_bwd_(da, h.cuda(), colsum=colsum)
        torch.cuda.synchronize()
        grad, fac = R.gelu_grad_ref(up(h))
        ref = up(da0) * grad
        # erf and exp factors: 2^-21 relative each; 4 fp32 roundings; one rounding to bf16
        tol = up(da0).abs() * (TRANS * fac + 4 * EPS23 * (grad.abs() + fac)) + BF16_RND * ref.abs()
        check(f"gelu_bwd[{shape},cs{colsum}]", da, ref, tol)
        if colsum:
            # column sums of the result AS STORED: N-term fp32 sum
            check(f"gelu_bwd.colsum[{shape}]", cs, up(da).sum(0), sum_tol(shape[0], up(da).abs().sum(0)))
        else:
            assert cs is None


@pytest.mark.parametrize("with_a16", [False, True])
def test_gelu_split_matches_fp64_reference(with_a16):
    """a = GELU(h) as fp16 (optional) and bf16: +-65504, +-0, -10 (GELU about -0), fp16 subnormal inputs, and random values (whose
    fp16 and bf16 roundings differ)."""
    g = gen(22)
    n = 8 * 1000
    h = (torch.randn(n, generator=g) * 2.5).half()
    h[:16] = _gelu_edge_values().half()
    a16 = nan_like((n,), torch.float16) if with_a16 else None
    abf = nan_like((n,), torch.bfloat16)
    nv.gelu_split(h.cuda(), a16, abf)
    torch.cuda.synchronize()
    ref, derf = R.gelu_ref(up(h))
    # erf: 2^-21 relative on that factor (|erf| <= 1, multiplied by |h| / 2); 3 fp32 roundings; the output rounding
    tol32 = TRANS * derf + 3 * EPS23 * (ref.abs() + derf)
    check(f"gelu_split.bf16[a16={with_a16}]", abf, ref, tol32 + BF16_RND * ref.abs())
    if with_a16:
        check("gelu_split.f16", a16, ref, tol32 + F16_RND * ref.abs() + F16_SUB)
        assert float(a16[0]) == 65504.0 and float(a16[1]) == 0.0                 # saturating; GELU(-65504) = -0
        assert int((up(a16) != up(abf)).sum()) > n // 4                          # the two roundings do differ on this input
    assert float(abf[2]) == 0.0 and float(abf[3]) == 0.0 and abs(float(abf[4])) < 1e-20


@pytest.mark.parametrize("D", [768, 1152])
@pytest.mark.parametrize("N", [1, 3, 4, 5, 511, 46656])
def test_colsum_matches_fp64_reference(N, D):
    """nparts clamps to 1, 1, 1, 2, 128, 128 for these N.  Column 0 alternates +-32768 and column 1 holds small integers: every partial
    sum of those is exactly representable in fp32, so any summation order gives the exact result and a dropped tail row shows."""
    g = gen(N + D)
    x = torch.randn(N, D, generator=g)
    x[:, 0] = 32768.0 * (1 - 2 * (torch.arange(N) % 2))
    x[:, 1] = torch.randint(-8, 9, (N,), generator=g).float()
    x[N - 1, 2] = 1024.0                                       # the tail row carries a value nothing else hides
    x = x.bfloat16()
    out = nv.colsum(x.cuda())
    torch.cuda.synchronize()
    ref = up(x).sum(0)
    assert out.shape == (D,)
    check(f"colsum.exact[{N},{D}]", out[:2], ref[:2], 0.0)     # integer-valued sums below 2^24 units: exact in any order
    # N-term fp32 sum
    check(f"colsum[{N},{D}]", out, ref, sum_tol(N, up(x).abs().sum(0)))


# =============================================================================================================================
# hicom_partials_sum_fwd: the plain and the tall form at the dispatch switch
# =============================================================================================================================
@pytest.mark.parametrize("nparts,M", [(63, 100), (64, 100), (64, 65536), (64, 65537), (1024, 1152), (1, 1)])
def test_partials_sum_both_forms(nparts, M):
    g = gen(nparts + M)
    parts = torch.randn(nparts, M, generator=g) * torch.logspace(-3, 3, nparts)[:, None]
    dparts = parts.cuda()
    out, again = nan_like((M,), torch.float32), nan_like((M,), torch.float32)
    nv.partials_sum(dparts, out)
    nv.partials_sum(dparts, again)
    torch.cuda.synchronize()
    assert torch.equal(out, again)                             # run-to-run bit-identical (both forms)
    tall = nparts >= 64 and M <= 65536
    if not tall:
        # plain form: fp32 additions in slice order, bit for bit
        assert torch.equal(out.cpu(), R.sequential_f32_sum(parts)), f"partials_sum[{nparts},{M}]: not the sequential fp32 sum"
        print(f"OPS_SMALL partials_sum.plain[{nparts},{M}] bit-equal to the sequential fp32 sum")
    # either form: nparts-term fp32 sum
    check(f"partials_sum[{nparts},{M},tall={tall}]", out, up(parts).sum(0), sum_tol(nparts, up(parts).abs().sum(0)))


# =============================================================================================================================
# operand preparation: hicom_split16_fwd, hicom_to_f16_padded_fwd, hicom_cast16_fwd
# =============================================================================================================================
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_split16_planes(dt):
    """hi + lo planes of f32 rows: the header's bounds, zero padding rows, bf16 bit-equal to hicom_split_bf16_fwd.  fp16 planes saturate
    (|x| > 65504: hi = +-65504, lo = the saturating fp16 of the remainder; never Inf - Inf)."""
    g = gen(31)
    rows, rows_pad, E = 37, 48, 200
    x = torch.randn(rows, E, generator=g) * torch.logspace(-6, 4, E)[None, :]
    x[0, :6] = torch.tensor([0.0, -0.0, 65504.0, -65504.0, 1.0, 2.0 ** -14])
    big = torch.tensor([65520.0, -70000.0, 1.0e5, 131008.0, -3.0e38, 65505.0])
    if dt == torch.float16:
        x[1, :6] = big
    hi, lo = nan_like((rows_pad, E), dt), nan_like((rows_pad, E), dt)
    nv.split16(x.cuda(), rows_pad, hi, lo)
    torch.cuda.synchronize()
    assert bool((hi[rows:].float() == 0).all()) and bool((lo[rows:].float() == 0).all())      # padding rows: zero in both planes
    xd, hd, ld = up(x), up(hi)[:rows], up(lo)[:rows]
    assert bool(torch.isfinite(hd).all()) and bool(torch.isfinite(ld).all())
    if dt == torch.bfloat16:
        h2, l2 = nan_like((rows_pad, E), dt), nan_like((rows_pad, E), dt)
        nv.split_bf16(x.cuda(), rows_pad, h2, l2)
        torch.cuda.synchronize()
        assert torch.equal(hi.view(torch.int16), h2.view(torch.int16)) and torch.equal(lo.view(torch.int16), l2.view(torch.int16))
        check("split16.bf16", hd + ld, xd, 2.0 ** -16 * xd.abs())                              # the header's bound
        return
    # two casts and one exact-by-IEEE subtraction: bit-exact against the same casts on the CPU
    want_hi = x.clamp(-65504.0, 65504.0).half()
    want_lo = (x - want_hi.float()).clamp(-65504.0, 65504.0).half()
    assert torch.equal(hi[:rows].cpu().view(torch.int16), want_hi.view(torch.int16))
    assert torch.equal(lo[:rows].cpu().view(torch.int16), want_lo.view(torch.int16))
    inr = xd.abs() <= 65504.0
    err = (xd - hd - ld).abs()
    bound = EPS23 * xd.abs() + 2.0 ** -25                                                         # the header's bound
    print(f"OPS_SMALL split16.f16 err/bound max {float((err[inr] / bound[inr]).max()):.3e}")
    assert bool((err[inr] <= bound[inr]).all())
    assert [float(v) for v in hd[1, :6]] == [65504.0, -65504.0, 65504.0, 65504.0, -65504.0, 65504.0]
    assert [float(v) for v in ld[1, :6]] == [16.0, -4496.0, 34496.0, 65504.0, -65504.0, 1.0]


@pytest.mark.parametrize("src_dt", [torch.bfloat16, torch.float32])
def test_to_f16_padded_is_a_saturating_cast_with_zero_padding(src_dt):
    g = gen(41)
    rows, cols, ld = 13, 70, 96
    src = (torch.randn(rows, cols, generator=g) * torch.logspace(-8, 4, cols)[None, :]).to(src_dt)
    src[0, :8] = torch.tensor([65504.0, -65504.0, 1.0e5, -1.0e5, 70000.0, float("inf"), float("-inf"), 65519.0]).to(src_dt)
    dst = nan_like((rows, ld), torch.float16)
    got = nv.to_f16_padded(src.cuda(), ld, dst)
    torch.cuda.synchronize()
    assert got.data_ptr() == dst.data_ptr()
    want = torch.zeros(rows, ld, dtype=torch.float16)
    want[:, :cols] = src.float().clamp(-65504.0, 65504.0).half()
    # a pure cast: bit-exact; padding columns zero (dst held NaN)
    assert torch.equal(dst.cpu().view(torch.int16), want.view(torch.int16))
    assert [float(v) for v in dst[0, 2:7]] == [65504.0, -65504.0, 65504.0, 65504.0, -65504.0]
    fresh = nv.to_f16_padded(src.cuda(), cols)
    assert torch.equal(fresh.cpu().view(torch.int16), want[:, :cols].contiguous().view(torch.int16))


@pytest.mark.parametrize("n", [1, 7, 8, 9, 8 * 256 + 3])
def test_cast16_both_directions_bit_exact(n):
    g = gen(n)
    # fp16 -> bf16, round to nearest even: exact ties (low three fraction bits 100) with an even and an odd kept bit, both signs,
    # normal and subnormal fp16, Inf
    ties = torch.tensor([0x3C04, 0x3C0C, 0xBC04, 0xBC0C, 0x0004, 0x000C, 0x7BFC, 0x7C00, 0x0001, 0x03FF, 0x3C03, 0x3C05], dtype=torch.int32).to(torch.int16)
    bits = torch.randint(0, 0x7C00, (n,), generator=g, dtype=torch.int32)
    bits = (bits | (torch.randint(0, 2, (n,), generator=g, dtype=torch.int32) << 15)).to(torch.int16)
    bits[:min(n, len(ties))] = ties[:n]
    h = bits.view(torch.float16)
    got = nv.cast16(h.cuda(), torch.bfloat16)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu().view(torch.int16), h.float().bfloat16().view(torch.int16)), "cast16 fp16 -> bf16"
    if n >= 2:
        assert got.cpu().view(torch.int16)[:2].tolist() == [0x3F80, 0x3F82]                  # tie to even: down, then up
    # bf16 -> fp16, saturating: out-of-range magnitudes, Inf, values that land on fp16 subnormals (and the tie 2^-25 -> 0)
    special = torch.tensor([65504.0, 65536.0, -1.0e20, float("inf"), float("-inf"), 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 1.0e-6, -4.0e-8,
                            6.1e-5, 0.0])
    b = (torch.randn(n, generator=g) * torch.logspace(-9, 6, n)).bfloat16()
    b[:min(n, len(special))] = special[:n].bfloat16()
    got = nv.cast16(b.cuda(), torch.float16)
    torch.cuda.synchronize()
    want = b.float().clamp(-65504.0, 65504.0).half()                                           # (torch does not saturate: clamp first)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)), "cast16 bf16 -> fp16"
    print(f"OPS_SMALL cast16[{n}] bit-exact both directions")
