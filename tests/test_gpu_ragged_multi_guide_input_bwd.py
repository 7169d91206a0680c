"""hicom_compressor_ragged_multiguide_local_bwd, _dq_pair and _global_dx alone (csrc/ragged_multi_guide_train.hip: rmg_local_bwd_kernel,
rmg_dq_pair_kernel, rmg_global_dx_kernel), from synthetic state built on the host -- no forward is run -- against the float64 references
of tests/ragged_multi_guide_input_bwd_reference.py.

Inputs: those of tests/test_gpu_ragged_multi_guide_global_bwd.py (MIX6: five items of 1, 4, 1, 8, 1 frames at 6 x 6 with 1, 3, 5, 2, 4
guides -- 9 .. 45 rows per item, the 45 across the 32-row pass; MIX9: 81 and 324 tokens with 4 and 8 guides -- 72 rows, three passes; the
spiked logits, item b's on a level of 16^b - 1, NaN in the dead rows and columns of the scores region), with dS the float64 reference of
that case rounded to fp32.  The window backward reads the same tokens as values and seeded keys whose logit under EVERY guide of the item
is raised at the item's tokens {0, 15, 16, N - 1}; the guides of item b are scaled by 2^b.

Tolerances are the derived rules of the single-guide tests (tests/test_gpu_ragged_input_bwd.py), restated for the sums over the guides:
  global dx   the (2 nh Q_i + 1)-term fp32 FMA chain over ALL rows of the item, (2 nh Q_i + 1) 2^-23 sum |terms|; the softmax weights' error as
              there; ONE rounding to bf16 of the finished sum, 2^-8 |ref|
  window bwd  per guide the fp32 bounds of the plain kernel (test_gpu_ragged_input_bwd.local_bounds' terms before its bf16 rounding); the
              token side adds a Q_i-term (value_is_key: 2 Q_i) chain, and ONE rounding to bf16: 2^-8 (|sum over the guides| + the fp32 bound)
  dq_pair     the sum of a pair's w_i window rows in some order: the rows' own bounds + w_i 2^-23 sum |rows|
Outputs are NaN-filled with NaN guard rows around them: every live element is written, the guards keep their NaN."""
import functools

import pytest
import torch

import ragged_multi_guide_input_bwd_reference as mr
from hicom_amd import native as nv
from hicom_amd import ragged
from hicom_amd import ragged_multi_guide as rmg
from ops_reference import EPS23, sum_tol, up
from test_gpu_ragged_input_bwd import BF16_RND, TRANS, check, guarded, guards_untouched
from test_gpu_ragged_multi_guide_global_bwd import E, KS, MIXES, NH, block, case

pytestmark = pytest.mark.gpu

DEV = "cuda"
SCALE = E ** -0.5
CHUNKS = 3


def plan(mix):
    """A block whose table region is prepared (no forward): (args, what keeps its memory alive, the host tables, the synthetic case)."""
    a, desc = block(mix, CHUNKS)
    a.l_scale = SCALE
    a.stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    ws = torch.zeros((nv.compressor_ragged_multiguide_workspace(a),), dtype=torch.uint8, device=DEV)
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
    nv.compressor_ragged_multiguide_prepare(a)
    t = rmg.plan_tables(desc, a._counts[:], a.H, a.W, KS, NH, torch.cuda.get_device_properties(0).multi_processor_count, CHUNKS)
    return a, ws, t, case(mix, tuple(t.chunks))


# =============================================================================================================================
# hicom_compressor_ragged_multiguide_global_dx
# =============================================================================================================================
@functools.lru_cache(maxsize=None)
def dx_case(mix):
    c = case(mix, (CHUNKS,) * len(MIXES[mix][0]))
    g = torch.Generator().manual_seed(177)
    ds = torch.full_like(c.scores, float("nan"))
    for it in c.items:
        ds[it.off:it.off + it.prows * it.stride].view(it.prows, it.stride)[:it.R, :it.N] = it.dS.float()
    return ds, torch.randn(c.R, E, generator=g), torch.randn(sum(c.N), E, generator=g).bfloat16()


@pytest.mark.parametrize("mix,accumulate", [("mix6", 1), ("mix6", 0), ("mix9", 1)])
def test_global_dx_against_float64_over_all_rows_of_the_item(mix, accumulate):
    a, keep, t, c = plan(mix)
    assert tuple(t.chunks) == (CHUNKS,) * c.B
    ds, qt, dx0 = dx_case(mix)
    tiles = torch.from_numpy(rmg.dx_tile_table(t)).to(DEV)
    buf, dx = guarded(sum(c.N), E, torch.bfloat16)
    if accumulate:
        dx.copy_(dx0)
    dev = [v.to(DEV) for v in (c.scores, ds, c.ml, qt, c.dctx)]
    before = [v.clone() for v in dev]
    nv.compressor_ragged_multiguide_global_dx(a, *dev, tiles, dx, accumulate)
    torch.cuda.synchronize()
    assert all(torch.equal(v.view(torch.uint8), w.view(torch.uint8)) for v, w in zip(dev, before)), "an input was written"
    guards_untouched("dx", buf)
    region = lambda v, it: up(v[it.off:it.off + it.prows * it.stride].view(it.prows, it.stride))
    S, dS = [region(c.scores, it) for it in c.items], [region(ds, it) for it in c.items]
    args = (up(c.ml), up(qt), up(c.dctx), c.N, c.counts, NH, up(dx0) if accumulate else None)
    ref, ab, ps = mr.rmg_global_dx_ref(S, dS, *args)
    wt = []
    for it, s, p in zip(c.items, S, ps):
        span = (s[:it.R, :it.N] - up(c.ml)[it.rows][:, 0:1]).abs()
        wt.append((p * (TRANS + 2 * EPS23 + 2.0 ** -24 * span)).t() @ up(c.dctx)[it.rows].abs())
    chain = torch.cat([sum_tol(2 * it.R + 1, ab[tok:tok + it.N]) for it, tok in zip(c.items, [sum(c.N[:b]) for b in range(c.B)])])
    tol = chain + torch.cat(wt) + BF16_RND * ref.abs()
    check(f"rmg_global_dx[{mix} a{accumulate}]", dx, ref, tol)
    # the case does what it is for: rows of the second pass read from the first would be far outside the bound
    wrong, _, _ = mr.rmg_global_dx_ref([s.nan_to_num(0.0) for s in S], [d.nan_to_num(0.0) for d in dS], *args, drop_pass_offset=True)
    assert float(((wrong - ref).abs() / (tol + 1e-37)).nan_to_num(nan=float("inf")).max()) > 10


def test_global_dx_skips_a_tile_that_names_no_item_or_no_token():
    a, keep, t, c = plan("mix6")
    ds, qt, _ = dx_case("mix6")
    tab = rmg.dx_tile_table(t).copy()
    tab[0], tab[3] = (c.B, 0), (1, c.N[1])                      # no such item; a first token behind the item's end
    buf, dx = guarded(sum(c.N), E, torch.bfloat16)
    nv.compressor_ragged_multiguide_global_dx(a, *[v.to(DEV) for v in (c.scores, ds, c.ml, qt, c.dctx)], torch.from_numpy(tab).to(DEV), dx, 0)
    torch.cuda.synchronize()
    guards_untouched("dx", buf)
    written = torch.isfinite(dx.float()).all(1).cpu()
    skipped = torch.zeros(sum(c.N), dtype=torch.bool)
    skipped[:36] = True                                         # tile 0: item 0
    skipped[36 + 128:36 + 144] = True                           # tile 3: the third tile of item 1 (its tokens 128 .. 143)
    assert torch.equal(written, ~skipped)                       # tokens of no tile keep their fill


# =============================================================================================================================
# hicom_compressor_ragged_multiguide_local_bwd, hicom_compressor_ragged_multiguide_dq_pair
# =============================================================================================================================
def items_of(mix):
    return [(T, 4 if T % 4 == 0 else 1) for T in MIXES[mix][0]]


@functools.lru_cache(maxsize=None)
def local_case(mix):
    splits, _, H, W, counts = MIXES[mix]
    c = case(mix, (CHUNKS,) * len(splits))
    g = torch.Generator().manual_seed(199)
    tok0, N, nw, pair0, row0 = mr.pair_offsets(items_of(mix), counts, H, W, KS)
    guides = torch.randn(sum(counts), E, generator=g)
    key = torch.randn(sum(N), E, generator=g)
    for b, Q in enumerate(counts):
        guides[pair0[b]:pair0[b] + Q] *= 2.0 ** b
    guides = guides.bfloat16()
    for b, Q in enumerate(counts):
        G = guides[pair0[b]:pair0[b] + Q].double()
        lift = (torch.linalg.solve(G @ G.t(), torch.full((Q,), 4.0 * E ** 0.5, dtype=torch.float64)) @ G).float()   # + 4 on every guide's logit
        for n in (0, 15, 16, N[b] - 1):
            key[tok0[b] + n] += lift
    dctx = (0.05 * torch.randn(sum(q * w for q, w in zip(counts, nw)), E, generator=g)).contiguous()
    return c, key.bfloat16().contiguous(), guides.contiguous(), dctx


def pair_bounds(o, q, g, K):
    """The fp32 bounds of one (item, guide) pair before any rounding to bf16: test_gpu_ragged_input_bwd.local_bounds' terms (tests/
    window_attn_inputs.py: backward_bounds for the plain kernel)."""
    D, WIN = E, o["tok"].shape[1]
    wsum = lambda v: v.sum(1, keepdim=True)
    d_s = sum_tol(D + 2, o["s_ab"])
    d_P = sum_tol(D + 1, o["dP_ab"])
    p, dP, dS = o["p"], o["dP"], o["dS"]
    span = (o["mx"] - o["s"]).clamp(0.0, 104.0)
    p_rel = torch.expm1(2 * d_s.max(1, keepdim=True).values) + 2 * TRANS + (WIN + 2) * EPS23 + EPS23 * (span + wsum(p * span))
    d_dS = (p_rel + 4 * EPS23) * p * (dP.abs() + wsum(p * dP.abs())) + p * (d_P + wsum(p * d_P)) + p * wsum(p * p_rel * dP.abs())
    d_dsk = SCALE * (d_dS + dS.abs() * 3 * EPS23)
    dq = torch.einsum("wi,wid->wd", d_dsk, K.abs()) + sum_tol(WIN + 4, o["dq_ab"])
    dk_rows = o["dsk"][:, :, None] * q[None, None, :]
    dv_rows = p[:, :, None] * g[:, None, :]
    d_dk = d_dsk[:, :, None] * q.abs()[None, None, :] + 2 * EPS23 * dk_rows.abs()
    d_dv = (p_rel * p)[:, :, None] * g.abs()[:, None, :] + 2 * EPS23 * dv_rows.abs()
    return dq, d_dk.reshape(-1, D), d_dv.reshape(-1, D), dk_rows.abs().reshape(-1, D), dv_rows.abs().reshape(-1, D)


# (dkey, dvalue, dq_pair, value_is_key): every NULL-output combination once
COMBOS = [(True, True, True, False), (True, False, False, False), (False, True, True, False), (False, False, True, False), (False, True, False, True)]


@pytest.mark.parametrize("want_dkey,want_dvalue,want_pair,vik", COMBOS, ids=["all", "dkey", "dvalue+pair", "pair", "value_is_key"])
def test_window_backward_against_float64_per_pair(want_dkey, want_dvalue, want_pair, vik):
    mix = "mix6"
    splits, _, H, W, counts = MIXES[mix]
    c, key, guides, dctx = local_case(mix)
    a, keep, t, _ = plan(mix)
    items = items_of(mix)
    tok0, N, nw, pair0, row0 = mr.pair_offsets(items, counts, H, W, KS)
    M = sum(counts)
    x = c.x.to(DEV)
    k_dev = x if vik else key.to(DEV)
    qbuf, dq = guarded(dctx.shape[0], E, torch.float32)
    pbuf, dqp = guarded(M, E, torch.float32)
    kbuf, dkey = guarded(sum(N), E, torch.bfloat16)
    vbuf, dval = guarded(sum(N), E, torch.bfloat16)
    g_dev, d_dev = guides.to(DEV), dctx.to(DEV)
    nv.compressor_ragged_multiguide_local_bwd(a, k_dev, x, g_dev, d_dev, dq, dqp if want_pair else None, dkey if want_dkey else None,
                                              dval if want_dvalue else None, value_is_key=vik)
    torch.cuda.synchronize()
    for name, buf, live, used in (("dq", qbuf, dq, True), ("dq_pair", pbuf, dqp, want_pair), ("dkey", kbuf, dkey, want_dkey), ("dvalue", vbuf, dval, want_dvalue)):
        guards_untouched(name, buf)
        if not used:
            assert bool(torch.isnan(live.float()).all()), f"{name}: written though NULL was passed"
    keys64 = up(c.x) if vik else up(key)
    ref = mr.rmg_local_bwd_ref(keys64, up(c.x), up(guides), up(dctx), items, counts, H, W, KS, SCALE, value_is_key=vik)
    tag = "+".join(n for n, u in (("dkey", want_dkey), ("dvalue", want_dvalue), ("pair", want_pair), ("vik", vik)) if u) or "dq"
    for b, Q in enumerate(counts):
        rows = slice(tok0[b], tok0[b] + N[b])
        e_k, e_v = torch.zeros(N[b], E, dtype=torch.float64), torch.zeros(N[b], E, dtype=torch.float64)
        ab_k, ab_v = torch.zeros_like(e_k), torch.zeros_like(e_v)
        for q in range(Q):
            p = pair0[b] + q
            wins = slice(row0[p], row0[p] + nw[b])
            o = ref["per_pair"][p]
            tokens = o["tok"].reshape(-1)
            bq, d_dk, d_dv, a_dk, a_dv = pair_bounds(o, up(guides)[p], up(dctx)[wins], keys64[rows][o["tok"]])
            check(f"rmg_local_bwd[{tag}] pair {p} dq", dq[wins], ref["dq"][wins], bq)
            if want_pair:
                check(f"rmg_local_bwd[{tag}] pair {p} dq_pair", dqp[p], ref["dq_pair"][p], bq.sum(0) + sum_tol(nw[b], ref["dq"][wins].abs().sum(0)))
            e_k[tokens] += d_dk; ab_k[tokens] += a_dk; e_v[tokens] += d_dv; ab_v[tokens] += a_dv
        if vik:
            e_v, ab_v = e_v + e_k, ab_v + ab_k
        for name, want, live, e, ab, terms in (("dkey", want_dkey, dkey, e_k, ab_k, Q), ("dvalue", want_dvalue, dval, e_v, ab_v, 2 * Q if vik else Q)):
            if want:
                f32 = e + sum_tol(terms, ab)                    # the per-guide terms' own errors + the chain over the guides
                check(f"rmg_local_bwd[{tag}] item {b} {name}", live[rows], ref[name][rows], f32 + BF16_RND * (ref[name][rows].abs() + f32))
    if want_pair:                                               # the same call twice: bit-equal sums (a fixed order, no atomics)
        again = torch.empty_like(dqp)
        nv.compressor_ragged_multiguide_local_bwd(a, k_dev, x, g_dev, d_dev, torch.empty_like(dq), again, None, None, value_is_key=False)
        torch.cuda.synchronize()
        if not vik:
            assert torch.equal(again, dqp)
    # the case does what it is for: guide q's dS paired with guide q + 1's row is far outside the bound wherever an item has two guides
    if want_dkey:
        wrong = mr.rmg_local_bwd_ref(keys64, up(c.x), up(guides), up(dctx), items, counts, H, W, KS, SCALE, shifted_dS=True)
        b = 2                                                   # (Q = 5)
        rows = slice(tok0[b], tok0[b] + N[b])
        assert float((wrong["dkey"][rows] - ref["dkey"][rows]).abs().max()) > 100 * BF16_RND * float(ref["dkey"][rows].abs().max())
