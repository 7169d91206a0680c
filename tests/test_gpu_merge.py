"""Every dispatch form of csrc/merge.hip / csrc/merge_item.hpp against the float64 references of tests/ops_reference.py (merge_ref,
combine_ref, merge_vproj_ref), from synthetic partials (tests/merge_inputs.py: how they are built, the restated dispatch predicates, the
case table with the form every case is built for, the branches that stay unreached, and the derivation of the bounds).
tests/test_merge_power.py shows on the references alone that each planted fault -- a lost partial or batch of partials, a frame weight
left unscaled, frames >= 64 or positional rows >= 128 dropped, an ignored offset, swapped y / x blocks, a neighbour's weight record, a
leaking padded row, an unweighted L, a lost column block, a neighbouring head's weights, a lost slab -- misses these bounds by a factor
of 250 at the least.

The kernels cannot be asked which form ran; every case carries the form its shape must select (mi.Case.form / .marg) and the tests
assert it against the restated predicates (mi.form_of, mi.marg_form_of), so a moved threshold fails a named case.  Per case:

  nopos_p{1,31,32,33,224,225,256,257,300,500}, nopos_p33_e{768,100,36}   mode0: no pe.  224 | 225: the prefetched 8-deep batch; 257, 300: behind
                                                                      it; 500: the 8-deep loop's own trip
  wave_3x27x27_p7, wave_2x32x32_p5, wave_4x7x5_p3                     wave marginals, mode1 + mode2: the record fits, R = 9 < 64
  wave_1x5x3_p9                                                       wave, mode0 with the positional term: T = 1, no room for the record
  regs_2x33x4_p3, regs_2x4x40_p3, reread_2x33x32_p3                   block marginals (H or W > 32), registers / re-reading (H W = 1056)
  stage_65x3x2_p4, stage_130x3x2_p4                                   mode1 + mode2 with 2 and 3 staging passes (last: 1 and 2 frames)
  stage_65x1x1_p200                                                   mode0 with the positional term, 2 passes: 200 + 65 + 4 > 64 x 4
  pos132_100x16x16_r9_p{4,16}                                         mode2 with 132 positional rows (second batch of four pe rows)
  a8_{4x7x5,100x16x16}_r{64,69}_p{1,16,17,32}_e{1152,100}             the 8-row apply, all 32: rows >= 64, nparts <= 32, the record in
                                                                      LDS; r69: a 5-row tail group; p17, p32: the second register slot;
                                                                      e100: col_ok; 100x16x16: the j >= 128 tail
  m2_4x7x5_r63_p16, m2_4x7x5_r64_p33, m2_1000x15x1_r64_p8             the predicate's other side, through mode2: 63 rows, 33 partials, a
                                                                      record of 1026 floats (8 of them exceed 64 KB of LDS)
  m0_1000x1x1_r64_p16                                                 mode0 with the positional term, 16 passes
  marg_4x7x5_r{9,69}_p{1,2,15,16,17}                                  nparts and R of the marginal entry's own list
Every positional case the part_marg layout can hold (mi.marg_layout_ok; all but the T = 1, H W < 16 and one-chunk-of-many-frames cases listed
in tests/merge_inputs.py) ALSO runs through hicom_global_merge_marg_fwd: merge_marg_weights_kernel + mode2 or apply8, with H and W in one,
two and three blocks of 16, up to 33 chunks, 63 rows and 33 partials into mode2.

What is asserted.  Every output starts as NaN and ends finite; out_ml as M exactly and log L within its bound; out_acc elementwise;
with pe the result differs from the reference without pe by more than 10 bounds; two launches on the same inputs are bit-identical
(o_fix included); the logit form and the marginal form of one case both meet the same bounds (no bit equality is asked between them).
Rows >= R of every input are NaN, so finite results prove they are not read.  `scratch` is exactly rows T (H + W + 2) floats inside a
larger NaN buffer whose tail must still be NaN (the weight record stays inside the row's region); out_ml / out_acc likewise end in a
NaN guard.  Refusals: every shape just outside a predicate raises HicomNativeError with the entry's text and leaves the outputs NaN.

Every check prints `MERGE <name> err=<largest error> bound=<bound there> ratio=<largest error / bound>`.

Measured on an MI355X (all cases; largest error and the range of the largest error / bound per check): no fault found.
  merge    log L  err <= 1.6e-07  ratio 0 .. 4.8e-02 (logits), 0 .. 4.3e-02 (marginals)
           out_acc  err <= 3.6e-03  ratio 0 .. 1.3e-01 (logits; nparts = 1 without pe is exact), 8.1e-03 .. 1.3e-01 (marginals)
           out_acc against the reference without pe: 3.5e+03 .. 1.5e+05 bounds (must exceed 10)
  combine  ctx    err <= 1.1e-05  ratio 1.6e-02 .. 8.5e-02    (dense and strided alike)
  vproj    log L  err <= 1.1e-07  ratio 0 .. 2.6e-02          ctx      err <= 8.8e-06  ratio 1.9e-03 .. 5.6e-02
           o      err <= 2.5e-05  ratio 1.6e-04 .. 8.6e-03    (partial-vector, fixed f32, fixed f16 and sets forms alike)
The largest ratios belong to the shortest chains (one partial, 16 positional rows), where the bound has the fewest terms to be
pessimistic about; the planted faults of tests/test_merge_power.py move an output by 251 bounds at the least.  The whole file (78 tests)
runs in about 11 s, its slowest tests (a8_100x16x16_*_e1152: 25 600 tokens x 1152 columns of float64 reference, both entries and both
normalize values) in 0.7 s each.
"""
import pytest
import torch

import merge_inputs as mi
import ops_reference as R
from ops_reference import up
from hicom_amd import native as nv

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64


def nan_dev(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def guarded(*shape):
    """A NaN tensor of `shape` at the head of a larger NaN buffer: (tensor, the guard floats behind it)."""
    n = 1
    for k in shape:
        n *= k
    buf = nan_dev(n + GUARD)
    return buf[:n].view(*shape), buf[n:]


def untouched(t):
    return bool(torch.isnan(t).all())


def check(name, got, ref, tol):
    """|got - ref| <= tol elementwise (float64 on the CPU); the figures are printed first."""
    got, ref = up(got), ref.double()
    tol = torch.broadcast_to(tol.double(), ref.shape)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values in the result"
    err = (got - ref).abs()
    ratio = (err / tol.clamp_min(1e-300)).reshape(-1)
    i = int(ratio.argmax())
    print(f"MERGE {name} err={float(err.max()):.3e} bound={float(tol.reshape(-1)[i]):.3e} ratio={float(ratio[i]):.3e}")
    assert bool((err <= tol).all()), f"{name}: error {float(err.reshape(-1)[i]):.3e} over its bound {float(tol.reshape(-1)[i]):.3e}"


def check_state(name, ml, M, L, tol):
    assert torch.equal(up(ml)[:, 0], M.float().double()), f"{name}: M differs"
    check(f"{name}.logL", torch.log(up(ml)[:, 1]), torch.log(L), tol)


# =============================================================================================================================
# hicom_global_merge_fwd / hicom_global_merge_marg_fwd
# =============================================================================================================================
def run_merge(c, d, normalize, marg):
    R_, E = c.R, c.E
    (ml, ml_g), (acc, acc_g) = guarded(R_, 2), guarded(R_, E)
    scratch = tail = None
    if c.pos:
        scratch, tail = guarded(R_ * c.T * (c.H + c.W + 2))
    if marg:
        nv.global_merge_marg(d["pm"], d["pl"], d["pacc"], d["pmarg"], R_, c.N, c.H, c.W, d["pe"], c.t0, c.y0, c.x0, scratch, ml, acc,
                             normalize=bool(normalize))
    else:
        nv.global_merge(d["pm"], d["pl"], d["pacc"], R_, d["scores"], c.N, c.H, c.W, d["pe"], c.t0, c.y0, c.x0, scratch, ml, acc,
                        normalize=bool(normalize))
    torch.cuda.synchronize()
    assert untouched(ml_g) and untouched(acc_g) and (tail is None or untouched(tail)), "a store behind the end of an output or of scratch"
    return ml, acc


@pytest.mark.parametrize("id", [e.id for e in mi.CASES])
def test_merge_matches_fp64_reference(id):
    c = mi.build(id)
    e = c.entry
    assert mi.form_of(e) == e.form and (not e.marg or mi.marg_form_of(e) == e.marg), (id, mi.form_of(e))
    d = {n: (getattr(c, n).cuda() if getattr(c, n) is not None else None) for n in ("pm", "pl", "pacc", "scores", "pe", "pmarg")}
    for normalize in e.normalize:
        ref = mi.merge_reference(id, normalize)
        b = mi.merge_bounds(c, ref, normalize)
        for marg in ((False, True) if e.marg else (False,)):
            tag = f"{id}.n{normalize}.{'marg' if marg else 'logits'}"
            ml, acc = run_merge(c, d, normalize, marg)
            check_state(tag, ml, ref["M"], ref["L"], b["logL"])
            check(f"{tag}.acc", acc, ref["acc"], b["acc"])
            if c.pos:
                off = float(((up(acc) - ref["acc_nope"]).abs() / b["acc"]).max())
                print(f"MERGE {tag}.acc_without_pe ratio={off:.3e}")
                assert off > 10.0
            ml2, acc2 = run_merge(c, d, normalize, marg)
            assert torch.equal(ml, ml2) and torch.equal(acc, acc2), f"{tag}: two launches differ"


def small_merge_args(T, H, W, E, nparts=1, rows=2, N=None):
    g = torch.Generator().manual_seed(5)
    N = T * H * W if N is None else N
    pm, pl = torch.randn(nparts, 16, generator=g).cuda(), (0.5 + torch.rand(nparts, 16, generator=g)).cuda()
    pacc = torch.randn(nparts, 16, E, generator=g).cuda()
    scores = torch.randn(16, N + 16, generator=g).cuda()
    pe = torch.randn(T + H + W, E, generator=g).cuda()
    scratch = nan_dev(rows * (T + 1) * (H + W + 2))
    return dict(pm=pm, pl=pl, pacc=pacc, scores=scores, pe=pe, scratch=scratch, ml=nan_dev(rows, 2), acc=nan_dev(rows, E), rows=rows, N=N,
                geom=(H, W, 0, T, T + H))


def refused_merge(a, match, scores=True, pe=True, E=None):
    H, W, t0, y0, x0 = a["geom"]
    with pytest.raises(nv.HicomNativeError, match=match):
        nv.global_merge(a["pm"], a["pl"], a["pacc"], a["rows"], a["scores"] if scores else None, a["N"], H, W, a["pe"] if pe else None,
                        t0, y0, x0, a["scratch"], a["ml"], a["acc"], normalize=True)
    torch.cuda.synchronize()
    assert untouched(a["ml"]) and untouched(a["acc"])


def test_global_merge_refuses_shapes_just_outside_its_predicates():
    assert mi.refusal(4, 7, 5, 3, 102, pos=False) == "global_merge: E"
    refused_merge(small_merge_args(4, 7, 5, 102, nparts=3), "global_merge: E", scores=False, pe=False)                 # E % 4 != 0
    # (N % (H W) != 0 and pe without scores fail ONE requirement of the entry, with one text: only the arguments tell the two calls apart)
    refused_merge(small_merge_args(4, 7, 5, 64, N=141), "positional term needs scores")                              # N % (H W) != 0
    refused_merge(small_merge_args(4, 7, 5, 64), "positional term needs scores", scores=False)                       # pe without scores
    assert mi.refusal(1, 110, 110, 1, 64) == "too many partials/frames for one pass" and mi.refusal(1, 106, 106, 1, 64) is None
    refused_merge(small_merge_args(1, 110, 110, 64), "too many partials/frames for one pass")                        # the smem2 cap
    # the marginal kernel's cap: 121 x 121 is the last grid it takes (59 064 bytes; the smem2 cap then refuses it), 122 x 122 the first it refuses
    assert mi.refusal(1, 121, 121, 1, 64) == "too many partials/frames for one pass" and mi.refusal(1, 122, 122, 1, 64) == "too large for the marginal kernel"
    refused_merge(small_merge_args(1, 122, 122, 64), "too large for the marginal kernel")


def test_global_merge_marg_refuses_shapes_just_outside_its_predicates():
    def call(T, H, W, nparts, match):
        a = small_merge_args(T, H, W, 64, nparts=nparts)
        pmarg = torch.zeros(nparts, 16, mi.marg_width(H, W), device="cuda")
        h, w, t0, y0, x0 = a["geom"]
        with pytest.raises(nv.HicomNativeError, match=match):
            nv.global_merge_marg(a["pm"], a["pl"], a["pacc"], pmarg, a["rows"], a["N"], h, w, a["pe"], t0, y0, x0, a["scratch"], a["ml"], a["acc"],
                                 normalize=True)
        torch.cuda.synchronize()
        assert untouched(a["ml"]) and untouched(a["acc"]) and untouched(a["scratch"])
    call(2, 65, 4, 2, "global_merge_marg: bad shape")                                  # H = 65
    assert mi.marg_layout_ok(544, 17, 16, 33) and not mi.marg_layout_ok(544, 17, 16, 34)
    call(2, 17, 16, 34, "weight record exceeds the row's scratch region")              # 2 + 34 + 2 + 33 = 71 floats for a region of 70


# =============================================================================================================================
# hicom_global_combine_fwd / hicom_global_combine_strided_fwd
# =============================================================================================================================
@pytest.mark.parametrize("family", mi.COMBINE_FAMILIES)
def test_combine_matches_fp64_reference(family):
    for nsets, rows, E in mi.COMBINE_SHAPES:
        c = mi.build_combine(family, nsets, rows, E)
        ref, _ = R.combine_ref(up(c.ml), up(c.acc))
        tol = mi.combine_bounds(c, ref)
        tag = f"combine.{family}.s{nsets}.r{rows}.e{E}"
        ml, acc, flat = c.ml.cuda(), c.acc.cuda(), c.packed.cuda().reshape(-1)
        for name in ("dense", "strided"):
            outs = []
            for _ in range(2):
                ctx, guard = guarded(rows, E)
                if name == "dense":
                    nv.global_combine(ml, acc, ctx)
                else:                           # (M, L) pairs and accumulators of a set `stride` floats apart, NaN in the gap
                    nv.global_combine_strided(flat, flat[2 * rows:], c.stride, nsets, rows, E, ctx)
                torch.cuda.synchronize()
                assert untouched(guard)
                outs.append(ctx)
            check(f"{tag}.{name}", outs[0], ref, tol)
            assert torch.equal(outs[0], outs[1])


# =============================================================================================================================
# hicom_merge_vproj_fwd / hicom_merge_vproj_fixed_fwd (f32 and f16 partials) / hicom_merge_vproj_sets_fwd
# =============================================================================================================================
def run_vproj(c, d, form):
    E, rows = c.E, c.rows
    (ml, g1), (ctx, g2) = guarded(rows, 2), guarded(rows, E)
    if form == "po":
        po, g3 = guarded(E // 64, E)
        nv.merge_vproj(d["pm"], d["pl"], d["pacc"], rows, d["wv"], po, ml, ctx)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(po).all())
        raw, o = po, po.double().sum(0)
    else:
        raw = torch.zeros(E + 8, dtype=torch.int64, device="cuda")
        ofx = raw[:E]
        if form == "sets":
            nv.merge_vproj_sets(d["sets"], rows, E, d["wv"], ofx, ml, ctx)
        else:
            nv.merge_vproj_fixed(d["pm"], d["pl"], d["p16"] if form == "fixed16" else d["pacc"], rows, d["wv"], ofx, ml, ctx)
        torch.cuda.synchronize()
        assert bool((raw[E:] == 0).all())
        o, g3 = ofx.double() / 2.0 ** 36, g1
    assert untouched(g1) and untouched(g2) and untouched(g3)
    return ml, ctx, o, raw


@pytest.mark.parametrize("E,rows", mi.VPROJ_SHAPES)
def test_merge_vproj_matches_fp64_reference(E, rows):
    for nparts in mi.VPROJ_NPARTS:
        c = mi.build_vproj(E, rows, nparts)
        d = {n: getattr(c, n).cuda() for n in ("pm", "pl", "pacc", "p16", "wv", "sets")}
        for form in ("po", "fixed", "fixed16", "sets"):
            f16 = form == "fixed16"
            ref = mi.vproj_reference(E, rows, nparts, f16)
            b = mi.vproj_bounds(c, ref, f16, fixed=form != "po")
            tag = f"vproj.e{E}.r{rows}.p{nparts}.{form}"
            ml, ctx, o, raw = run_vproj(c, d, form)
            check_state(tag, ml, ref[0], ref[1], b["logL"])
            check(f"{tag}.ctx", ctx, ref[2], b["ctx"])
            check(f"{tag}.o", o, ref[3], b["o"])
            ml2, ctx2, _, raw2 = run_vproj(c, d, form)
            assert torch.equal(ml, ml2) and torch.equal(ctx, ctx2) and torch.equal(raw, raw2), f"{tag}: two launches differ"


def test_merge_vproj_refuses_shapes_just_outside_its_predicates():
    def call(E, rows, nparts, match_tail, dt=torch.float32):
        rows_pad = max(16, rows)
        pm, pl = torch.zeros(nparts, rows_pad, device="cuda"), torch.ones(nparts, rows_pad, device="cuda")
        pacc = torch.zeros(nparts, rows_pad, E, device="cuda", dtype=dt)
        wv = torch.zeros(E, E, dtype=torch.bfloat16, device="cuda")
        po, ofx = nan_dev((E + 63) // 64, E), torch.zeros(E, dtype=torch.int64, device="cuda")
        stride = 2 * rows + rows * E
        sets = torch.zeros(nparts, stride + stride % 2, device="cuda")
        calls = {"merge_vproj": lambda: nv.merge_vproj(pm, pl, pacc, rows, wv, po),
                 "merge_vproj_fixed": lambda: nv.merge_vproj_fixed(pm, pl, pacc, rows, wv, ofx),
                 "merge_vproj_sets": lambda: nv.merge_vproj_sets(sets, rows, E, wv, ofx)}
        for name, fn in calls.items():
            if dt != torch.float32 and name != "merge_vproj_fixed":
                continue
            with pytest.raises(nv.HicomNativeError, match=f"{name}: {match_tail}"):
                fn()
        torch.cuda.synchronize()
        assert untouched(po) and bool((ofx == 0).all())
    call(64, 1, 257, "bad shape")                       # nparts = 257
    call(96, 1, 2, "bad shape")                         # E % 64 != 0
    call(8256, 64, 1, "bad shape")                      # head dim 129
    call(64, 1, 2, "part_dt", dt=torch.bfloat16)        # partials neither f32 nor f16
