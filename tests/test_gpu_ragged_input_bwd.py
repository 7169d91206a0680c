"""hicom_compressor_ragged_local_bwd and hicom_compressor_ragged_global_dx alone (csrc/ragged_train.hip: ragged_local_attn_bwd_kernel,
ragged_dq_item_kernel, ragged_global_dx_kernel), from synthetic state built on the host -- no forward is run -- against the float64
references of tests/ragged_input_bwd_reference.py.

Inputs: those of tests/test_gpu_ragged_global_bwd.py (five items of 1, 4, 1, 8, 1 frames at 6 x 6: token offsets 36, 180, 216, 504, no
multiple of a 64-token tile, a masked tail tile in every item; the spiked logits, item b's on a level of 16^b - 1, NaN in the rows >= nh
and the columns >= N_i of the scores region), with dS the float64 reference of that case rounded to fp32.  The window backward reads the
same tokens as values and seeded keys whose logit under the item's guide is raised at the item's tokens {0, 15, 16, N - 1}; guide b is
scaled by 2^b, so the logit levels of neighbouring items differ.

Tolerances are the derived rules of the single-item kernels, restated here for the shapes used (nothing new):
  global dx   tests/test_gpu_ops_small.py (_global_dx_check): the (2 rows + 1)-term fp32 FMA chain, (2 rows + 1) 2^-23 sum |terms|; the
              softmax weight carries expf (2^-21), the rounding of S - M (2^-24 |S - M|) and the division (2 2^-23); one rounding to bf16
  window bwd  tests/window_attn_inputs.py (backward_bounds, plain kernel: no l2norm, bias 0, every token written once): logits and dP are
              D-term dot products; the weights' relative error (weight_rel); dS = p (dP - delta) with 4 roundings; dq a (WIN + 4)-term sum;
              dk = dsk q, dv = p dctx (+ dk), 2 roundings, one fp32 store-side rounding and ONE rounding to bf16
  dq_item     the sum of an item's w_i window rows in some order: the rows' own bounds + w_i 2^-23 sum |rows|
Outputs are NaN-filled with NaN guard rows around them: every live element is written, the guards keep their NaN."""
import functools

import pytest
import torch

import ragged_input_bwd_reference as rr
from hicom_amd import native as nv
from hicom_amd import ragged
from ops_reference import EPS23, sum_tol, up
from test_gpu_ragged_global_bwd import E, H, HIDDEN, KS, NH, SPLITS, W, case, descriptors

pytestmark = pytest.mark.gpu

BF16_RND, TRANS = 2.0 ** -8, 2.0 ** -21
GUARD = 2                        # NaN rows in front of and behind every output
DEV = "cuda"
ITEMS = [(d[0], d[1]) for d in descriptors()]
SCALE = E ** -0.5


def plan():
    """A plain block whose table region is prepared (no forward): (args, what keeps its memory alive, the host tables)."""
    desc = descriptors()
    a = nv.CompressorRaggedArgs()
    items = (nv.RaggedItem * len(desc))(*[nv.RaggedItem(*d) for d in desc])
    a.B, a.H, a.W, a.E, a.hidden, a.ks, a.nh, a.chunks, a.items = len(desc), H, W, E, HIDDEN, KS, NH, 1, items
    a.l_scale = SCALE
    a.stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    ws = torch.zeros((nv.compressor_ragged_workspace(a),), dtype=torch.uint8, device=DEV)
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
    nv.compressor_ragged_prepare(a)
    return a, (items, ws), ragged.plan_tables(desc, H, W, KS, 1, 1)


def guarded(rows, cols, dtype):
    buf = torch.full((rows + 2 * GUARD, cols), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + rows]


def check(name, got, ref, tol):
    got = up(got)
    assert bool(torch.isfinite(got).all()), f"{name}: a live element was not written"
    err, tol = (got - ref).abs(), tol + 1e-37
    i = int((err / tol).argmax())
    print(f"RAGGED_INPUT_BWD {name} err={float(err.max()):.3e} bound={float(tol.reshape(-1)[i]):.3e} ratio={float((err / tol).max()):.3e}")
    assert bool((err <= tol).all()), f"{name}: error {float(err.reshape(-1)[i]):.3e} over its bound {float(tol.reshape(-1)[i]):.3e}"


def guards_untouched(name, buf):
    assert bool(torch.isnan(buf[:GUARD].float()).all()) and bool(torch.isnan(buf[-GUARD:].float()).all()), f"{name}: a guard row was written"


# =============================================================================================================================
# hicom_compressor_ragged_global_dx
# =============================================================================================================================
@functools.lru_cache(maxsize=None)
def dx_case():
    c = case((1,) * len(SPLITS))
    g = torch.Generator().manual_seed(77)
    ds = torch.full_like(c.scores, float("nan"))
    for it in c.items:
        ds[16 * it.off:16 * (it.off + it.stride)].view(16, it.stride)[:NH, :it.N] = it.dS.float()
    qt = torch.randn(c.R, E, generator=g)
    dx0 = torch.randn(sum(c.N), E, generator=g).bfloat16()
    return c, ds, qt, dx0


@pytest.mark.parametrize("accumulate", [0, 1])
def test_global_dx_against_float64_per_item(accumulate):
    c, ds, qt, dx0 = dx_case()
    a, keep, t = plan()
    tiles = torch.from_numpy(ragged.dx_tile_table(t)).to(DEV)
    buf, dx = guarded(sum(c.N), E, torch.bfloat16)
    if accumulate:
        dx.copy_(dx0)
    dev = [v.to(DEV) for v in (c.scores, ds, c.ml, qt, c.dctx)]
    before = [v.clone() for v in dev]
    nv.compressor_ragged_global_dx(a, *dev, tiles, dx, accumulate)
    torch.cuda.synchronize()
    assert all(torch.equal(v.view(torch.uint8), w.view(torch.uint8)) for v, w in zip(dev, before)), "an input was written"
    guards_untouched("dx", buf)
    S = [up(c.scores[16 * it.off:16 * (it.off + it.stride)].view(16, it.stride)) for it in c.items]
    dS = [up(ds[16 * it.off:16 * (it.off + it.stride)].view(16, it.stride)) for it in c.items]
    ref, ab, ps = rr.ragged_global_dx_ref(S, dS, up(c.ml), up(qt), up(c.dctx), c.N, NH, up(dx0) if accumulate else None)
    # the rule of tests/test_gpu_ops_small.py, per item: the weights' error times |dctx| of the item's own rows
    wt = []
    for b, (it, p) in enumerate(zip(c.items, ps)):
        rows = slice(b * NH, (b + 1) * NH)
        span = (S[b][:NH, :it.N] - up(c.ml)[rows][:, 0:1]).abs()
        wt.append((p * (TRANS + 2 * EPS23 + 2.0 ** -24 * span)).t() @ up(c.dctx)[rows].abs())
    tol = sum_tol(2 * NH + 1, ab) + torch.cat(wt) + BF16_RND * ref.abs()
    check(f"global_dx[a{accumulate}]", dx, ref, tol)
    # the case does what it is for: a tile's tail that read the next item's coefficients would be far outside the bound
    wrong, _, _ = rr.ragged_global_dx_ref(S, dS, up(c.ml), up(qt), up(c.dctx), c.N, NH, up(dx0) if accumulate else None, flat_tiles=64)
    # (item i + 1 stands 16 x higher: its logits under item i's M overflow, which counts as infinitely wrong)
    assert float(((wrong - ref).abs() / (tol + 1e-37)).nan_to_num(nan=float("inf")).max()) > 10


def test_global_dx_skips_a_tile_that_names_no_item_or_no_token():
    c, ds, qt, _ = dx_case()
    a, keep, t = plan()
    tab = ragged.dx_tile_table(t).copy()
    tab[0], tab[3] = (len(SPLITS), 0), (1, c.N[1])              # no such item; a first token behind the item's end
    buf, dx = guarded(sum(c.N), E, torch.bfloat16)
    nv.compressor_ragged_global_dx(a, *[v.to(DEV) for v in (c.scores, ds, c.ml, qt, c.dctx)], torch.from_numpy(tab).to(DEV), dx, 0)
    torch.cuda.synchronize()
    guards_untouched("dx", buf)
    written = torch.isfinite(dx.float()).all(1).cpu()
    skipped = torch.zeros(sum(c.N), dtype=torch.bool)
    skipped[:36] = True                                         # tile 0: item 0
    skipped[36 + 128:36 + 144] = True                           # tile 3: the third tile of item 1 (its tokens 128 .. 143)
    assert torch.equal(written, ~skipped)


# =============================================================================================================================
# hicom_compressor_ragged_local_bwd
# =============================================================================================================================
@functools.lru_cache(maxsize=None)
def local_case():
    c = case((1,) * len(SPLITS))
    g = torch.Generator().manual_seed(99)
    B = len(SPLITS)
    guides = (torch.randn(B, E, generator=g) * torch.tensor([2.0 ** b for b in range(B)])[:, None]).bfloat16()
    key = torch.randn(sum(c.N), E, generator=g)
    tok0, N, win0, nw = rr.offsets(ITEMS, H, W, KS)
    for b in range(B):
        gd = guides[b].double()
        for n in (0, 15, 16, N[b] - 1):                         # + 4 on the logit g . k / sqrt(E) at the item's edge tokens
            key[tok0[b] + n] += (4.0 * E ** 0.5 * gd / (gd @ gd)).float()
    dctx = (0.05 * torch.randn(sum(nw), E, generator=g)).contiguous()
    return c, key.bfloat16().contiguous(), guides.contiguous(), dctx


def local_bounds(o, q, g, key_rows, value_is_key):
    """tests/window_attn_inputs.py: backward_bounds for the plain kernel (no l2norm, bias 0), on one item's reference dict `o`."""
    D, WIN = E, o["tok"].shape[1]
    K = key_rows[o["tok"]]
    wsum = lambda v: v.sum(1, keepdim=True)
    d_s = sum_tol(D + 2, o["s_ab"])
    d_P = sum_tol(D + 1, o["dP_ab"])
    p, dP, dS = o["p"], o["dP"], o["dS"]
    span = (o["mx"] - o["s"]).clamp(0.0, 104.0)
    p_rel = torch.expm1(2 * d_s.max(1, keepdim=True).values) + 2 * TRANS + (WIN + 2) * EPS23 + EPS23 * (span + wsum(p * span))
    d_dS = (p_rel + 4 * EPS23) * p * (dP.abs() + wsum(p * dP.abs())) + p * (d_P + wsum(p * d_P)) + p * wsum(p * p_rel * dP.abs())
    d_dsk = SCALE * (d_dS + dS.abs() * 3 * EPS23)
    out = {"dq": torch.einsum("wi,wid->wd", d_dsk, K.abs()) + sum_tol(WIN + 4, o["dq_ab"])}
    d_dk = d_dsk[:, :, None] * q.abs()[None, None, :]
    d_dv = (p_rel * p)[:, :, None] * g.abs()[:, None, :]
    if value_is_key:
        d_dv = d_dv + d_dk
    st = o["steps"][0]                                          # an exact partition: one launch, every token written once
    for name, rows_key, ab_key, d_rows in (("dkey", "dk", "dk_ab", d_dk), ("dvalue", "dv", "dv_ab", d_dv)):
        tol = torch.zeros(key_rows.shape[0], D, dtype=torch.float64)
        e = d_rows.reshape(-1, D) + 2 * EPS23 * st[ab_key] + EPS23 * st[rows_key].abs()
        tol[st["tok"]] = e + BF16_RND * (st[rows_key].abs() + e)
        out[name] = tol
    return out


# (dkey, dvalue, dq_item, value_is_key): every NULL-output combination once
COMBOS = [(True, True, True, False), (True, False, False, False), (False, True, True, False), (False, False, True, False), (False, True, False, True)]


@pytest.mark.parametrize("want_dkey,want_dvalue,want_item,vik", COMBOS, ids=["all", "dkey", "dvalue+item", "item", "value_is_key"])
def test_window_backward_against_float64_per_item(want_dkey, want_dvalue, want_item, vik):
    c, key, guides, dctx = local_case()
    a, keep, t = plan()
    tok0, N, win0, nw = rr.offsets(ITEMS, H, W, KS)
    x = c.x.to(DEV)
    k_dev = x if vik else key.to(DEV)
    qbuf, dq = guarded(sum(nw), E, torch.float32)
    ibuf, dqi = guarded(len(SPLITS), E, torch.float32)
    kbuf, dkey = guarded(sum(N), E, torch.bfloat16)
    vbuf, dval = guarded(sum(N), E, torch.bfloat16)
    g_dev, d_dev = guides.to(DEV), dctx.to(DEV)
    nv.compressor_ragged_local_bwd(a, k_dev, x, g_dev, d_dev, dq, dqi if want_item else None, dkey if want_dkey else None,
                                   dval if want_dvalue else None, value_is_key=vik)
    torch.cuda.synchronize()
    for name, buf, live, used in (("dq", qbuf, dq, True), ("dq_item", ibuf, dqi, want_item), ("dkey", kbuf, dkey, want_dkey), ("dvalue", vbuf, dval, want_dvalue)):
        guards_untouched(name, buf)
        if not used:
            assert bool(torch.isnan(live.float()).all()), f"{name}: written though NULL was passed"
    keys64 = up(c.x) if vik else up(key)
    ref = rr.ragged_local_bwd_ref(keys64, up(c.x), up(guides), up(dctx), ITEMS, H, W, KS, SCALE, value_is_key=vik)
    tag = "+".join(n for n, u in (("dkey", want_dkey), ("dvalue", want_dvalue), ("item", want_item), ("vik", vik)) if u) or "dq"
    for b, o in enumerate(ref["per_item"]):
        rows, wins = slice(tok0[b], tok0[b] + N[b]), slice(win0[b], win0[b] + nw[b])
        bnd = local_bounds(o, up(guides)[b], up(dctx)[wins], keys64[rows], vik)
        check(f"local_bwd[{tag}] item {b} dq", dq[wins], ref["dq"][wins], bnd["dq"])
        if want_item:
            check(f"local_bwd[{tag}] item {b} dq_item", dqi[b], ref["dq_item"][b], bnd["dq"].sum(0) + sum_tol(nw[b], ref["dq"][wins].abs().sum(0)))
        if want_dkey:
            check(f"local_bwd[{tag}] item {b} dkey", dkey[rows], ref["dkey"][rows], bnd["dkey"])
        if want_dvalue:
            check(f"local_bwd[{tag}] item {b} dvalue", dval[rows], ref["dvalue"][rows], bnd["dvalue"])
    if want_item:                                               # the same call twice: bit-equal sums (a fixed order, no atomics)
        again = torch.empty_like(dqi)
        nv.compressor_ragged_local_bwd(a, k_dev, x, g_dev, d_dev, torch.empty_like(dq), again, None, None, value_is_key=False)
        torch.cuda.synchronize()
        if not vik:
            assert torch.equal(again, dqi)
