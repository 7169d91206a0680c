"""hicom_fused_stream_fwd (all three instantiations) and the fp16 form of hicom_query_prep_fwd against the float64 restatements in
tests/ops_reference.py, computed from the values the kernels received.  Conventions of tests/test_gpu_ops_small.py: elementwise
check() against float64, derived tolerances (one line per term), outputs prefilled with NaN, the figures printed before every assert
as `OPS_RING <name> err= bound= ratio=`.

The input builders, the restatement of the entry point's limits and the tolerance tensors (ring_inputs, ring_refusal, ring_bounds)
need no GPU: tests/test_ops_references.py plants defects into the reference on these very inputs and requires each to exceed twice
these very bounds.

Bound terms (EPS23 = 2^-23):
  logit of a token        K-term fp32 sum of exact 16-bit products: K EPS23 sum|q||x| (K = E + 16 local, 2 E + 16 global: hi and lo
                          plane, the eight channel slices), the query planes (2^-16 sum|q||x| bf16; 2^-22 max|q_r| sum|x| for the fp16
                          form's per-row split), one rounding per further operation (scale, bias, three pos_a terms), and the
                          argument of the exponential: s - m and its product with log2(e), EPS23 (|s| + |m|) each
  weights                 a perturbation <= d of every logit of a softmax moves each weight by <= expm1(2 d) relative
  expf                    2^-21 relative; weight planes 2^-16 (bf16) or 2^-23 p + 2^-39 (fp16, of the largest weight)
  P.x                     (2 tokens + 8) EPS23 sum p|x|; normaliser: one rounding per token, two per tile (rescale of acc and of l)
  outputs                 + 2^-10 |ref| + 2^-24 (fp16), + 2^-16 |ref| (bf16 hi + lo)"""
import math
from types import SimpleNamespace

import pytest
import torch

import ops_reference as R
from fused_ring_inputs import (BF16_PLANES, CASES, COLLECT_CUS, E, F16_RND, FAMILY_CASES, NAN, REFUSED, cu_nparts, f16_out, n_windows, ref_args,
                               ring_bounds, ring_inputs, ring_reference, ring_refusal)
from hicom_amd import native as nv
from ops_reference import sum_tol, up

pytestmark = pytest.mark.gpu


# =============================================================================================================================
# the launches
# =============================================================================================================================
def check(name, got, ref, tol, fam):
    """|got - ref| <= tol elementwise (float64 on the CPU); the figures are printed first."""
    got, ref = up(got), ref.double()
    tol = torch.broadcast_to(tol.double(), ref.shape)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values in the result"
    err = (got - ref).abs()
    ratio = err / tol.clamp_min(1e-300)
    k = int(ratio.argmax())
    where = tuple(int(v) for v in torch.unravel_index(torch.tensor(k), ref.shape))
    print(f"OPS_RING {name} family={fam} err={float(err.reshape(-1)[k]):.3e} bound={float(tol.reshape(-1)[k]):.3e} ratio={float(ratio.reshape(-1)[k]):.3e} at={where}")
    assert bool((err <= tol).all()), f"{name}: error {float(err.reshape(-1)[k]):.3e} over its bound {float(tol.reshape(-1)[k]):.3e} at {where}"


def nan_dev(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def launch(i, d, nparts, mode):
    """mode "acc": every local output + part_acc + zero_ptr;  "ctx16": part_ctx_f16;  "marg": part_marg_f16 without pe planes."""
    T, H, W, kt, ks = i.shape
    NW, rows = n_windows(*i.shape), i.rows
    o = SimpleNamespace(pm=nan_dev((nparts, 16)), pl=nan_dev((nparts, 16)))
    kw = dict(local_logits=d.llog, q_f32=d.q_f32)
    fe = None if i.form == "logits" else d.fe
    pe_hi, pe_lo = d.pe_hi, d.pe_lo
    if mode == "acc":
        o.pacc, o.ctx = nan_dev((nparts, 16, E)), nan_dev((NW, E))
        o.chi, o.clo = nan_dev((NW, E), torch.bfloat16), nan_dev((NW, E), torch.bfloat16)
        o.c16 = nan_dev((NW, E), torch.float16)
        o.guard = torch.full((16 + 24 + 16,), 77, dtype=torch.int64, device="cuda")
        kw.update(ctx_hi=o.chi, ctx_lo=o.clo, ctx_f16=o.c16, zero=o.guard[16:40])
    else:
        o.pacc, o.ctx = None, None
        o.c16, o.p16 = nan_dev((NW, E), torch.float16), nan_dev((nparts, 16, E), torch.float16)
        kw.update(ctx_f16=o.c16, part_ctx_f16=o.p16)
        if mode == "marg":
            o.mg = nan_dev((nparts, rows, (T + H + W + 7) // 8 * 8 + 8), torch.float16)
            kw.update(part_marg=o.mg)
            pe_hi = pe_lo = None
    nv.fused_stream(d.ff, fe, kt, ks, d.q_hi, d.q_lo, rows, i.l_scale, i.l_bias, d.pos_a, pe_hi, pe_lo, i.t0i, i.y0i, i.x0i,
                    o.pm, o.pl, o.pacc, o.ctx, **kw)
    return o


def to_dev(i):
    d = SimpleNamespace()
    for k in ("ff", "fe", "q_hi", "q_lo", "q_f32", "llog", "pos_a", "pe_hi", "pe_lo"):
        v = getattr(i, k)
        setattr(d, k, None if v is None else v.contiguous().cuda())
    return d


def run_case(i, nparts_list, tag, local_ref_bias0=False):
    d = to_dev(i)
    T, H, W, kt, ks = i.shape
    rows, fam = i.rows, i.family
    for nparts in nparts_list:
        name = f"[{tag},np{nparts}]"
        assert ring_refusal(*i.shape, rows, nparts, i.form == "logits") is None, (name, "listed case outside the limits")
        ref = ring_reference(i, nparts)
        b = ring_bounds(i, ref)
        a = launch(i, d, nparts, "acc")
        a2 = launch(i, d, nparts, "acc")
        c = launch(i, d, nparts, "ctx16")
        torch.cuda.synchronize()
        # local contexts: f32, bf16 planes, fp16 plane
        check("ctx_local" + name, a.ctx, ref["ctx_local"], b["ctx_local"], fam)
        if local_ref_bias0:                                            # the softmax cancels l_bias: the contexts are those of l_bias = 0
            i0 = SimpleNamespace(**{**vars(i), "l_bias": 0.0})
            ref0 = ring_reference(i0, nparts)
            check("ctx_local_vs_bias0" + name, a.ctx, ref0["ctx_local"], b["ctx_local"], fam)
        check("ctx_hi+lo" + name, up(a.chi) + up(a.clo), ref["ctx_local"], b["ctx_local"] + BF16_PLANES * ref["ctx_local"].abs(), fam)
        assert torch.equal(a.chi, a.ctx.bfloat16()), name + ": ctx_hi is bf16(ctx)"
        assert float((up(a.chi) + up(a.clo) - up(a.ctx)).abs().sub(BF16_PLANES * up(a.ctx).abs()).max()) <= 0.0, name + ": hi + lo = ctx to 2^-16"
        sat = ref["ctx_local"].clamp(-65504.0, 65504.0)
        check("ctx_f16" + name, a.c16, sat, f16_out(b["ctx_local"], sat), fam)
        assert torch.equal(a.c16, c.c16), name + ": ctx_f16 of both launches"
        # partition state
        lse = up(a.pm[:, :rows]) + torch.log(up(a.pl[:, :rows]))
        check("part_lse" + name, lse, ref["lse"], b["lse"], fam)
        check("part_ctx" + name, up(a.pacc[:, :rows]) / up(a.pl[:, :rows, None]), ref["part_ctx"], b["part_ctx"], fam)
        sat_p = ref["part_ctx"].clamp(-65504.0, 65504.0)                 # the fp16 plane saturates, like ctx_f16
        check("part_ctx_f16" + name, c.p16[:, :rows], sat_p, f16_out(b["part_ctx"], sat_p), fam)
        assert torch.equal(a.pm[:, :rows], c.pm[:, :rows]) and torch.equal(a.pl[:, :rows], c.pl[:, :rows]), name + ": (m, l) of both launches"
        # merged over the partitions, in float64 from the kernel's state
        wgt = torch.exp(up(a.pm[:, :rows]) - up(a.pm[:, :rows]).max(0).values)
        merged = (wgt[:, :, None] * up(a.pacc[:, :rows])).sum(0) / (wgt * up(a.pl[:, :rows])).sum(0)[:, None]
        check("merged" + name, merged, ref["merged"], b["merged"], fam)
        # scratch cleared, its neighbours untouched; run-to-run bit equality
        assert int(a.guard[16:40].abs().sum()) == 0 and bool((a.guard[:16] == 77).all()) and bool((a.guard[40:] == 77).all()), name + ": zero_ptr"
        for k in ("ctx", "chi", "clo", "c16"):
            assert torch.equal(getattr(a, k), getattr(a2, k)), name + ": run-to-run " + k
        assert torch.equal(a.pacc[:, :rows], a2.pacc[:, :rows]) and torch.equal(a.pm[:, :rows], a2.pm[:, :rows]) \
            and torch.equal(a.pl[:, :rows], a2.pl[:, :rows]), name + ": run-to-run partition state"
        if i.form != "f16":
            # marginals out, value-side pe not folded in
            refm = ring_reference(i, nparts, with_pe=False)
            bm = ring_bounds(i, refm, with_pe=False)
            m = launch(i, d, nparts, "marg")
            torch.cuda.synchronize()
            S = T + H + W
            check("marg" + name, m.mg[..., :S], refm["marg"], bm["marg"], fam)
            assert float(m.mg[..., S:].float().abs().max()) == 0.0, name + ": marginal padding"
            for lo, n in ((0, T), (T, H), (T + H, W)):                  # n fp16 roundings of entries that sum to 1, + the bound of their sum
                tol_sum = n * (F16_RND / 2) + float(bm["marg"][..., lo:lo + n].sum(-1).max())
                assert float((up(m.mg[..., lo:lo + n]).sum(-1) - 1.0).abs().max()) <= tol_sum, name + ": marginals sum to 1"
            sat_m = refm["part_ctx"].clamp(-65504.0, 65504.0)
            check("part_ctx_f16_nope" + name, m.p16[:, :rows], sat_m, f16_out(bm["part_ctx"], sat_m), fam)
            assert torch.equal(m.c16, a.c16), name + ": ctx_f16 of the marginal launch"


def runtime_nparts(i):
    """The listed nparts with the suggestion of the library on THIS device in place of the one assumed at collection."""
    NW = n_windows(*i.shape)
    ok = [n for n in range(1, NW + 1) if ring_refusal(*i.shape, i.rows, n, i.form == "logits") is None]
    sug = nv.fused_stream_nparts(NW)
    assert sug in ok, f"hicom_fused_stream_nparts({NW}) = {sug} is outside the documented limits for {i.shape}, rows {i.rows}, {i.form}"
    return sorted({ok[0], sug, NW} & set(ok))


def case_id(c):
    s, r, f = c
    return f"{'x'.join(map(str, s))}-r{r}-{f}"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fused_stream_plain_inputs_match_fp64_reference(case):
    """Every listed shape, row count and instantiation at the smallest valid nparts, the suggested one and one window per workgroup."""
    shape, rows, form = case
    i = ring_inputs("plain", form, shape, rows)
    run_case(i, runtime_nparts(i), case_id(case))


@pytest.mark.parametrize("fam,shape,rows,form", FAMILY_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fused_stream_input_families_match_fp64_reference(fam, shape, rows, form):
    """flat / peaky / offsets / bias / extremes inputs (see ring_inputs): each isolates one path of the kernel under a small bound."""
    i = ring_inputs(fam, form, shape, rows)
    run_case(i, runtime_nparts(i), f"{fam},{case_id((shape, rows, form))}", local_ref_bias0=fam.startswith("bias"))
    if fam == "extremes" and form != "f16":
        # window 1 holds 1e5 everywhere: its fp16 context saturates at exactly 65504 while the f32 one is finite and right
        d = to_dev(i)
        a = launch(i, d, n_windows(*shape), "acc")
        torch.cuda.synchronize()
        assert bool((a.c16[1].float() == 65504.0).all()) and bool(torch.isfinite(a.ctx[1]).all())


# =============================================================================================================================
# hicom_query_prep_fwd, fp16 form
# =============================================================================================================================
def _qp_weights(P, hidden, seed):
    g = torch.Generator().manual_seed(seed)
    nh = 9
    w = SimpleNamespace(nh=nh, scale=(E // nh) ** -0.5)
    w.wq, w.wk = (torch.randn(E, E, generator=g) * 0.02).bfloat16(), (torch.randn(E, E, generator=g) * 0.02).bfloat16()
    w.bq = (torch.randn(E, generator=g) * 0.1).bfloat16()
    w.kpe = torch.randn(E, P, generator=g) * 0.3 if P else None
    w.gw0, w.gb0 = (torch.randn(hidden, E, generator=g) * 0.02).bfloat16(), (torch.randn(hidden, generator=g) * 0.1).bfloat16()
    w.bo = (torch.randn(E, generator=g) * 0.1).bfloat16()
    w.guides = [torch.randn(E, generator=g).half() for _ in range(3)]
    return w


def _qp_bounds(w, ab, hidden):
    """fp32 chains: qp = E-term sum (+ bias); qt / pos_a = hd-term sums over qp (the inner error rides along in the absolute terms:
    (E + hd + 4) roundings of sum |w_k| sum |w_q||g|); r0 = E-term sum + 2."""
    hd = E // w.nh
    qt_ab, pa_ab, r0_ab = ab
    tol = lambda k, a: None if a is None else sum_tol(k, a) + 1e-37
    return tol(E + hd + 4, qt_ab), tol(E + hd + 4, pa_ab), tol(E + 4, r0_ab)


@pytest.mark.parametrize("P", [0, 310])
@pytest.mark.parametrize("hidden", [64, 896, 3584])
def test_query_prep_fp16_form_matches_fp64_reference(P, hidden):
    """g_dt = HICOM_DT_F16: qt_f32 / pos_a / r0 elementwise against query_prep_ref; the local query rows are the fp16 guide bit for
    bit, the global rows of qt_hi / qt_lo stay as the caller filled them, no hand-off failed.  A train of launches with alternating
    guides and no host sync, as the bf16 test runs."""
    w = _qp_weights(P, hidden, 23 + P + hidden)
    dv = lambda t: None if t is None else t.cuda()
    wq, wk, bq, kpe, gw0, gb0, bo = map(dv, (w.wq, w.wk, w.bq, w.kpe, w.gw0, w.gb0, w.bo))
    state = nv.query_prep_state(E, "cuda")
    outs = []
    FILL = 0.4375
    for it in range(12):
        gd = w.guides[it % 3].cuda()
        qhi = torch.full((16, E), FILL, dtype=torch.float16, device="cuda")
        qlo = torch.full((16, E), FILL, dtype=torch.float16, device="cuda")
        qlo[w.nh:] = 0
        pos_a = nan_dev((16, P)) if P else None
        r0, qf = nan_dev((hidden,)), nan_dev((16, E))
        nv.query_prep(gd, gd, wq, bq, wk, kpe, w.nh, w.scale, qhi, qlo, pos_a, state, gw0, gb0, bo, r0, q_f32=qf)
        outs.append((it % 3, qhi, qlo, pos_a, r0, qf))
    torch.cuda.synchronize()
    assert int(state[:16].view(torch.int32)[2]) == 0                    # word 2: failed hand-offs
    for k, qhi, qlo, pos_a, r0, qf in outs:
        (qt, pa, rr), ab = R.query_prep_ref(up(w.guides[k]), up(w.wq), up(w.bq), up(w.wk), None if w.kpe is None else up(w.kpe), w.nh, w.scale,
                                            up(w.gw0), up(w.gb0), up(w.bo))
        t_qt, t_pa, t_r0 = _qp_bounds(w, ab, hidden)
        tag = f"[P{P},h{hidden},g{k}]"
        check("qprep_qt_f32" + tag, qf[:w.nh], qt, t_qt, "query_prep")
        if P:
            check("qprep_pos_a" + tag, pos_a[:w.nh], pa, t_pa, "query_prep")
        check("qprep_r0" + tag, r0, rr, t_r0, "query_prep")
        assert torch.equal(qhi[w.nh:].cpu(), w.guides[k].view(1, E).expand(16 - w.nh, E)), tag + ": local rows = the fp16 guide"
        assert bool((qhi[:w.nh] == FILL).all()) and bool((qlo[:w.nh] == FILL).all()), tag + ": global rows of qt_hi / qt_lo untouched"


def test_query_prep_fp16_into_fused_stream_fp16_matches_reference_from_the_guide():
    """The chain of the fp16 recipe: hicom_query_prep_fwd (fp16) hands q_f32 / pos_a / the local rows to hicom_fused_stream_fwd (fp16).
    Reference from the guide alone; the query-prep bound on qt and pos_a enters the logit bound as a further perturbation."""
    shape, rows = (8, 6, 6, 4, 3), 9
    T, H, W, kt, ks = shape
    i = ring_inputs("plain", "f16", shape, rows, seed=5)
    P = i.pos_a.shape[1]
    w = _qp_weights(P, 64, 77)
    pe = up(i.pe_hi) + up(i.pe_lo)
    w.kpe = torch.nan_to_num(up(w.wk) @ pe.t(), nan=0.0).float()        # kpe = w_k . pe^T (unused slots: 0)
    guide = (0.3 * torch.randn(E, generator=torch.Generator().manual_seed(3))).half()
    dv = lambda t: t.cuda()
    qhi = torch.full((16, E), NAN, dtype=torch.float16, device="cuda")
    qlo = torch.zeros(16, E, dtype=torch.float16, device="cuda")
    pos_a, qf = torch.zeros(16, P, device="cuda"), nan_dev((16, E))
    state = nv.query_prep_state(E, "cuda")
    nv.query_prep(dv(guide), dv(guide), dv(w.wq), dv(w.bq), dv(w.wk), dv(w.kpe), w.nh, w.scale, qhi, qlo, pos_a, state, q_f32=qf)
    (qt, pa, _), (qt_ab, pa_ab, _) = R.query_prep_ref(up(guide), up(w.wq), up(w.bq), up(w.wk), up(w.kpe), w.nh, w.scale, None, None, None)
    i.qt, i.q_local, i.pos_a = qt, up(guide), pa.float()
    i.pos_a = torch.where(i.used[None, :], pa, torch.tensor(NAN, dtype=torch.float64))
    nparts = runtime_nparts(i)[0]
    a, kw = ref_args(i)
    kw["pos_a"] = torch.where(i.used[None, :], pa, torch.tensor(NAN, dtype=torch.float64))
    ref = R.fused_ring_ref(*a, nparts=nparts, **kw)
    b = ring_bounds(i, ref)
    # the producer's own error on qt and pos_a, as a perturbation of every global logit
    t_qt, t_pa, _ = _qp_bounds(w, (qt_ab, pa_ab, None), 64)
    x_abs = up(i.ff).view(-1, E).abs()
    dq = float((t_qt @ x_abs.t()).max() + 3 * t_pa[:, i.used].max())
    extra = math.expm1(2 * dq)
    d = to_dev(i)
    o = SimpleNamespace(pm=nan_dev((nparts, 16)), pl=nan_dev((nparts, 16)), pacc=nan_dev((nparts, 16, E)), ctx=nan_dev((n_windows(*shape), E)))
    nv.fused_stream(d.ff, d.fe, kt, ks, qhi, qlo, rows, i.l_scale, 0.0, pos_a, d.pe_hi, d.pe_lo, i.t0i, i.y0i, i.x0i, o.pm, o.pl, o.pacc, o.ctx, q_f32=qf)
    torch.cuda.synchronize()
    assert int(state[:16].view(torch.int32)[2]) == 0
    check("chain_ctx_local", o.ctx, ref["ctx_local"], b["ctx_local"], "chain")
    check("chain_part_lse", up(o.pm[:, :rows]) + torch.log(up(o.pl[:, :rows])), ref["lse"], b["lse"] + dq, "chain")
    check("chain_part_ctx", up(o.pacc[:, :rows]) / up(o.pl[:, :rows, None]), ref["part_ctx"], b["part_ctx"] + extra * ref["part_ctx_ab"], "chain")


# =============================================================================================================================
# refusals: an error code, no launch
# =============================================================================================================================
def test_fused_stream_refuses_what_the_header_excludes():
    def call(shape=(8, 6, 6, 4, 3), rows=9, form="bf16", nparts=None, Ex=E, **over):
        T, H, W, kt, ks = shape
        NW = max(1, (T // kt) * (H // ks) * (W // ks))
        nparts = nparts or NW
        dt = torch.float16 if form == "f16" else torch.bfloat16
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="cuda")
        P = T + H + W
        a = dict(ff=z(T, H, W, Ex, dtype=dt), fe=z(T, H, W, Ex, dtype=dt), q_hi=z(16, Ex, dtype=dt), q_lo=z(16, Ex, dtype=dt), pos_a=z(16, P),
                 pe_hi=z(P, Ex, dtype=dt), pe_lo=z(P, Ex, dtype=dt), pm=nan_dev((nparts, 16)), pl=nan_dev((nparts, 16)), pacc=nan_dev((nparts, 16, Ex)),
                 ctx=nan_dev((NW, Ex)), kw={})
        if form == "logits":
            a["kw"]["local_logits"], a["fe"] = z(T * H * W), None
        if form == "f16":
            a["kw"]["q_f32"] = z(16, Ex)
        a["kw"].update(over.pop("kw", {}))
        a.update(over)
        with pytest.raises(nv.HicomNativeError):
            nv.fused_stream(a["ff"], a["fe"], kt, ks, a["q_hi"], a["q_lo"], rows, 0.03, 0.0, a["pos_a"], a["pe_hi"], a["pe_lo"], 0, T, T + H,
                            a["pm"], a["pl"], a["pacc"], a["ctx"], **a["kw"])
        torch.cuda.synchronize()
        # nothing was launched: every output still holds its prefill
        assert bool(torch.isnan(a["pm"]).all()) and bool(torch.isnan(a["pacc"]).all()) and bool(torch.isnan(a["ctx"]).all())

    call(rows=13)
    call(shape=(15, 2, 2, 15, 1))                                    # wsz = 15
    call(shape=(65, 2, 2, 65, 1))                                    # wsz = 65
    call(Ex=768)
    call(shape=(4, 65, 5, 1, 5), rows=1)                             # H = 65
    # LDS / slot overflows of the shape list: refused for EVERY nparts the other limits would admit
    for shape, rows, form in sorted(REFUSED) + [((4, 36, 36, 4, 3), 9, "logits"), ((4, 36, 36, 4, 3), 12, "logits")]:
        NW = n_windows(*shape)
        assert all(ring_refusal(*shape, rows, n, form == "logits") for n in range(1, NW + 1))
        call(shape=shape, rows=rows, form=form, nparts=cu_nparts(NW, COLLECT_CUS))
    assert ring_refusal(4, 64, 64, 1, 4, 1, 32, False) == "pos-emb slots"
    call(shape=(4, 64, 64, 1, 4), rows=1, nparts=32)                 # 32 windows per workgroup touch 8 + 12 + 64 pos-emb slots
    call(nparts=1)                                                   # a workgroup would span 12 frames
    call(nparts=7)                                                   # 8 windows, 2 per workgroup: workgroups 4 .. 6 would be empty
    # fp16 tokens: the two-tensor form with pe planes and aligned fp32 rows only
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="cuda")
    call(form="f16", kw=dict(local_logits=z(8 * 36)))
    call(form="f16", kw=dict(q_f32=z(16 * E + 1)[1:].view(16, E)))     # 4-byte aligned only
    call(form="f16", kw=dict(q_f32=None))
    call(kw=dict(ctx_hi=z(8, E, dtype=torch.bfloat16)))                # ctx_hi without ctx_lo


def test_fused_stream_refuses_fp16_tokens_with_marginals():
    shape, rows = (8, 6, 6, 4, 3), 9
    i = ring_inputs("plain", "f16", shape, rows)
    d = to_dev(i)
    NW = n_windows(*shape)
    pm, pl = nan_dev((NW, 16)), nan_dev((NW, 16))
    c16, p16, mg = nan_dev((NW, E), torch.float16), nan_dev((NW, 16, E), torch.float16), nan_dev((NW, rows, 24), torch.float16)
    with pytest.raises(nv.HicomNativeError):
        nv.fused_stream(d.ff, d.fe, 4, 3, d.q_hi, d.q_lo, rows, i.l_scale, 0.0, d.pos_a, None, None, 0, 8, 14, pm, pl, None, None, ctx_f16=c16,
                        part_ctx_f16=p16, part_marg=mg, q_f32=d.q_f32)
    torch.cuda.synchronize()
    assert bool(torch.isnan(pm).all()) and bool(torch.isnan(p16.float()).all()) and bool(torch.isnan(mg.float()).all())
