"""hicom_compressor_ragged_multiguide_global_bwd and _train_state alone (csrc/ragged_multi_guide_train.hip: planes of dctx,
pos_b = dctx . pe^T, rmg_stream_bwd_kernel -- stream_segment<9, 2, Bwd> on the forward's work units -- and rmg_dq_merge_kernel).

global_bwd runs from synthetic state built on the host -- no forward is run -- as tests/test_gpu_ragged_global_bwd.py does for the
single-guide call, on the two mixes of tests/ragged_multi_guide_inputs.py: MIX6 (6 x 6, frames (1, 4, 1, 8, 1), guides (1, 3, 5, 2, 4): 9,
27, 45, 18, 36 rows; a dead row group, a group of two live rows, a guide across the groups, second passes of 13 and 4 rows, masked tail
tiles) and MIX9 (9 x 9, frames (1, 4), guides (4, 8): 36 and 72 rows, three passes).  Per item: seeded bf16 tokens, dctx ~ N(0, 0.05), logits
~ N(0, 1) spiked by SHIFT at the item's edge tokens and both sides of every chunk boundary (row r leaves out spike r mod k), on a level of
16^b - 1 for item b, so neighbouring items' M differ by a factor of about 16; (M, L) in float64 from the fp32 logits; delta the true
dctx_r . ctx_r.  Rows >= nh Q_i and columns >= N_i of an item's scores region hold NaN.

dS and dqt against float64 (ops_reference.global_stream_bwd_ref per item, all nh Q_i rows at once) under
global_stream_inputs.backward_bounds with nparts = the item's chunks: the kernel runs the same body for every row.  The two terms the call
adds are derived here as in tests/test_gpu_ragged_global_bwd.py:
  pos_b    = dctx . pe^T formed by the call, an E-term fp32 sum per entry: E 2^-23 (|dctx| . |pe_c|) per positional column, three columns per
           token, and the planes of dctx it splits itself, PSPLIT |dctx| . |x_n|; both enter dP, so times p in dS
  dqt      = dSx + mt . pe[t..] + my . pe[y..] + mx . pe[x..] in the merge: the marginals' bounds times |pe rows|, + the fp32 sums over
           nparts partial sums and T + H + W positional rows: (nparts + T + H + W + 2) 2^-23 sum |terms|.
Outputs and workspace are filled (NaN / 0xFF) with guards around them: dS rows >= nh Q_i of an item's last pass, the partial-sum rows of a
dead row group or behind a group's last live row, and the guards keep the fill bit for bit.

train_state runs behind a real forward: ctx16 and ctxg bit-equal to the workspace regions (the layout of segment_host.hpp restated below),
(M, L) against float64 from the copied scores (the stream stores the full logits, positional terms included): M exactly, L within
(N + chunks + 8) 2^-23 + TRANS relative."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import global_stream_inputs as gi
import many_item_inputs as mi
import ops_reference as R
import ragged_multi_guide_inputs as ri
from gpu_util import build_module, dev_bf16
from hicom_amd import native as nv
from hicom_amd import ragged_multi_guide as rmg
from ops_reference import EPS23, sum_tol, up

pytestmark = pytest.mark.gpu

E, NH, KS, HIDDEN = 1152, 9, 3, 64
GUARD = 64                      # floats in front of and behind ds and dqt (256 bytes: the alignment of the regions is kept)
MIXES = {"mix6": ri.MIX6, "mix9": ri.MIX9}


def descriptors(splits):
    return [(T, 4 if T % 4 == 0 else 1, 0, 0, 0, 1, 32) for T in splits]


@functools.lru_cache(maxsize=None)
def case(mix, chunks_per_item):
    """The host tensors of the call for the given chunks per item, and the float64 reference and bounds per item."""
    splits, _, H, W, counts = MIXES[mix]
    g = torch.Generator().manual_seed(4321 + sum(chunks_per_item) + H)
    rnd = lambda *s: torch.randn(*s, generator=g)
    cap = max(splits) + 2
    c = SimpleNamespace(y0=cap, x0=cap + H, P=cap + H + W + 3, B=len(splits), R=NH * sum(counts), H=H, W=W, splits=splits, counts=counts)
    c.N = [T * H * W for T in splits]
    c.stride = [(n + 15) // 16 * 16 for n in c.N]
    c.prows = [32 * rmg.item_passes(NH, q) for q in counts]            # rows of an item's scores region
    c.x = rnd(sum(c.N), E).bfloat16().contiguous()
    c.pe = (rnd(c.P, E) * 0.5).contiguous()
    c.dctx = (0.05 * rnd(c.R, E)).contiguous()
    hi = c.dctx.bfloat16()
    gd = up(hi) + up((c.dctx - hi.float()).bfloat16())             # what the planes hold
    pos_b = up(c.dctx) @ up(c.pe).t()
    pos_b_err = sum_tol(E, up(c.dctx).abs() @ up(c.pe).abs().t())
    c.scores = torch.full((sum(p * s for p, s in zip(c.prows, c.stride)),), float("nan"))
    c.ml = torch.zeros(c.R, 2)
    c.delta = torch.zeros(c.R)
    c.items, tok, off, row = [], 0, 0, 0
    for b, (T, N, stride, nparts, Q, prows) in enumerate(zip(splits, c.N, c.stride, chunks_per_item, counts, c.prows)):
        nr = NH * Q
        rows = slice(row, row + nr)
        toks = mi.edge_tokens(N, nparts)
        tgt = torch.zeros(nr, N, dtype=torch.float64)
        for n in toks:
            tgt[:, n] = gi.SHIFT * mi.spike_weight(n, N)
        for r in range(nr):
            tgt[r, toks[r % len(toks)]] = 0.0
        region = c.scores[off:off + prows * stride].view(prows, stride)
        region[:nr, :N] = (rnd(nr, N).double() + tgt + (16.0 ** b - 1.0)).float()
        Sd = up(region)[:nr, :N]
        Md = Sd.max(1).values
        c.ml[rows] = torch.stack([Md, torch.exp(Sd - Md[:, None]).sum(1)], 1).float()
        xi = up(c.x[tok:tok + N])
        p = torch.exp(Sd - up(c.ml[rows])[:, 0:1]) / up(c.ml[rows])[:, 1:2]
        dP = R.stream_terms(gd[rows], xi, pos_b[rows], None, H, W, 0, c.y0, c.x0)[0]
        c.delta[rows] = (p * dP).sum(1).float()
        it = SimpleNamespace(entry=SimpleNamespace(pos=True), T=T, H=H, W=W, N=N, E=E, R=nr, s_in=region, ml=c.ml[rows], delta=c.delta[rows],
                             x=c.x[tok:tok + N], rows=rows, off=off, stride=stride, prows=prows, nparts=nparts, toks=toks)
        bw = R.global_stream_bwd_ref(g=gd[rows], x=xi, pos_b=pos_b[rows], S=up(region), ml=up(it.ml), delta=up(it.delta), H=H, W=W, t0i=0, y0i=c.y0,
                                     x0i=c.x0)
        tol = gi.backward_bounds(it, bw, nparts)
        t, y, xx = R.token_axes(N, H, W)
        dp_extra = pos_b_err[rows][:, t] + pos_b_err[rows][:, c.y0 + y] + pos_b_err[rows][:, c.x0 + xx] + gi.PSPLIT * (gd[rows].abs() @ xi.abs().t())
        ds_extra = bw["p"] * dp_extra
        it.dS, it.dS_tol = bw["dS"], tol["dS"] + ds_extra
        pes = [up(c.pe)[c0:c0 + n] for c0, n in ((0, T), (c.y0, H), (c.x0, W))]
        it.dqt = bw["dSx"] + sum(m @ pe for m, pe in zip(bw["marg"], pes))
        marg_tol = [a + b_ for a, b_ in zip(tol["marg"], R.axis_marginals(ds_extra, H, W))]
        terms = bw["dSx_ab"] + sum(m.abs() @ pe.abs() for m, pe in zip(bw["marg"], pes))
        it.dqt_tol = (tol["dSx"] + ds_extra @ xi.abs() + sum(mt @ pe.abs() for mt, pe in zip(marg_tol, pes))
                      + sum_tol(nparts + T + H + W + 2, terms))
        c.items.append(it)
        tok, off, row = tok + N, off + prows * stride, row + nr
    return c


def block(mix, chunks):
    splits, _, H, W, counts = MIXES[mix]
    desc = descriptors(splits)
    a = nv.CompressorRaggedMultiGuideArgs()
    a._items = (nv.RaggedItem * len(desc))(*[nv.RaggedItem(*d) for d in desc])
    a._counts = (ctypes.c_int32 * len(counts))(*counts)
    a.B, a.H, a.W, a.E, a.hidden, a.ks, a.nh, a.chunks = len(desc), H, W, E, HIDDEN, KS, NH, chunks
    a.items, a.guide_counts, a.n_guide_counts = a._items, a._counts, len(counts)
    return a, desc


@functools.lru_cache(maxsize=None)
def run(mix, chunks):
    """Prepares the table region of a block (no forward), runs the call on filled outputs; returns (case, tables, ds, dqt, ws, total)."""
    dev = torch.device("cuda")
    a, desc = block(mix, chunks)
    n_cus = torch.cuda.get_device_properties(dev).multi_processor_count
    t = rmg.plan_tables(desc, a._counts[:], a.H, a.W, KS, NH, n_cus, chunks)
    c = case(mix, tuple(t.chunks))
    pe, kpe = c.pe.to(dev), torch.zeros(8, device=dev)             # (kpe: the forward's table, only its presence is checked)
    a.pe, a.kpe, a.P, a.t_index0, a.y_index0, a.x_index0 = pe.data_ptr(), kpe.data_ptr(), c.P, 0, c.y0, c.x0
    a.stream = torch.cuda.current_stream(dev).cuda_stream
    pws = torch.zeros((nv.compressor_ragged_multiguide_workspace(a),), dtype=torch.uint8, device=dev)
    a.ws, a.ws_bytes = pws.data_ptr(), pws.numel()
    nv.compressor_ragged_multiguide_prepare(a)
    img = rmg.table_image(t)
    assert pws[:4 * img.size].cpu().numpy().view("int32").tolist() == img.tolist()      # the device's tables are the ones the spikes were placed for
    nan = lambda n: torch.full((n,), float("nan"), device=dev)
    ds_buf, dqt_buf = nan(c.scores.numel() + 2 * GUARD), nan(c.R * E + 2 * GUARD)
    ds, dqt = ds_buf[GUARD:-GUARD], dqt_buf[GUARD:-GUARD].view(c.R, E)
    total = nv.compressor_ragged_multiguide_global_bwd_workspace(a)
    ws_buf = torch.full((total + 1024,), 0xFF, dtype=torch.uint8, device=dev)
    x, dctx, delta, scores, ml = (v.to(dev) for v in (c.x, c.dctx, c.delta, c.scores, c.ml))
    before = [v.clone() for v in (x, dctx, delta, scores, ml)]
    nv.compressor_ragged_multiguide_global_bwd(a, x, dctx, delta, scores, ml, ds, dqt, ws_buf[:total])
    torch.cuda.synchronize()
    assert all(torch.equal(v.view(torch.uint8), w.view(torch.uint8)) for v, w in zip((x, dctx, delta, scores, ml), before)), "an input was written"
    return c, t, ds_buf.cpu(), dqt_buf.cpu(), ws_buf.cpu(), total


CALLS = [("mix6", 1), ("mix6", 3), ("mix6", 18), ("mix9", 3), ("mix9", 0)]


@pytest.mark.parametrize("mix,chunks", CALLS)
def test_dS_and_dqt_against_float64_per_item(mix, chunks):
    c, t, ds_buf, dqt_buf, _, _ = run(mix, chunks)
    ds, dqt = ds_buf[GUARD:-GUARD], dqt_buf[GUARD:-GUARD].view(c.R, E)
    bad = []
    for b, it in enumerate(c.items):
        got_ds = up(ds[it.off:it.off + it.prows * it.stride].view(it.prows, it.stride))[:it.R, :it.N]
        got_dq = up(dqt[it.rows])
        assert torch.isfinite(got_ds).all() and torch.isfinite(got_dq).all(), f"item {b}: a live element was not written"
        w_ds = float(((got_ds - it.dS).abs() / it.dS_tol).max())
        w_dq = float(((got_dq - it.dqt).abs() / it.dqt_tol).max())
        print(f"{mix} chunks={chunks} item {b} (N {it.N}, {it.R} rows, {it.nparts} chunks, M {float(it.ml[0, 0]):.1f}): dS "
              f"{float((got_ds - it.dS).abs().max()):.3e} ({w_ds:.1e} of its bound), dqt {float((got_dq - it.dqt).abs().max()):.3e} ({w_dq:.1e} of its bound), "
              f"max |dqt| {float(it.dqt.abs().max()):.3e}")
        if not w_ds <= 1.0:
            bad.append(f"item {b} dS: {w_ds:.3f} bounds")
        if not w_dq <= 1.0:
            bad.append(f"item {b} dqt: {w_dq:.3f} bounds")
        mass = (it.dS.abs()[:, it.toks].sum(1) / it.dS.abs().sum(1)).min()        # the spiked tokens carry the mass, in every row
        assert float(mass) > 0.5, (b, float(mass))
    assert not bad, "; ".join(bad)
    assert all(abs(float(a.ml[0, 0]) - float(b_.ml[0, 0])) > 10 for a, b_ in zip(c.items, c.items[1:]))


@pytest.mark.parametrize("mix,chunks", [("mix6", 3), ("mix9", 3)])
def test_dead_rows_dead_groups_and_guards_keep_the_fill(mix, chunks):
    c, t, ds_buf, dqt_buf, ws_buf, total = run(mix, chunks)
    ds = ds_buf[GUARD:-GUARD]
    nan_bits = lambda v: bool((v.contiguous().view(torch.int32) == torch.tensor(float("nan")).view(torch.int32)).all())
    assert nan_bits(ds_buf[:GUARD]) and nan_bits(ds_buf[-GUARD:]), "dS: written outside the scores region"
    assert nan_bits(dqt_buf[:GUARD]) and nan_bits(dqt_buf[-GUARD:]), "dqt: written outside its rows"
    assert torch.isfinite(dqt_buf[GUARD:-GUARD]).all()
    for b, it in enumerate(c.items):
        region = ds[it.off:it.off + it.prows * it.stride].view(it.prows, it.stride)
        assert torch.isfinite(region[:it.R, :it.N]).all(), f"item {b}: live dS"
        assert (region[:it.R, it.N:] == 0).all(), f"item {b}: padded tail columns of a live row"
        assert nan_bits(region[it.R:]), f"item {b}: rows >= nh Q of the last pass were written"
    # the workspace: dctx planes [R, E] bf16 x 2, pos_b [R, P] f32, part_acc [slots][16][E] f32, each rounded up to 256 bytes
    r256 = lambda n: (n + 255) // 256 * 256
    o_lo, o_pos = r256(c.R * E * 2), 2 * r256(c.R * E * 2)
    o_acc = o_pos + r256(c.R * c.P * 4)
    assert total == o_acc + r256(t.slots * 16 * E * 4)
    assert (ws_buf[total:] == 0xFF).all(), "written behind the workspace"
    acc = ws_buf[o_acc:o_acc + t.slots * 16 * E * 4].view(torch.float32).view(t.slots, 16, E)
    raw = ws_buf[o_acc:o_acc + t.slots * 16 * E * 4].view(t.slots, 16, E * 4)
    dead_groups = 0
    for i in range(c.B):
        for p in range(t.passes[i]):
            for grp in range(2):
                live = min(16, max(0, NH * c.counts[i] - 32 * p - 16 * grp))
                dead_groups += live == 0
                for ch in range(t.chunks[i]):
                    s = t.slot0[i] + 2 * p * t.chunks[i] + grp * t.chunks[i] + ch
                    assert torch.isfinite(acc[s, :live]).all(), f"item {i} pass {p} group {grp} chunk {ch}: a live partial sum was not written"
                    assert (raw[s, live:] == 0xFF).all(), f"item {i} pass {p} group {grp} chunk {ch}: partial-sum rows >= {live} were written"
    assert dead_groups >= 1


# ---- train_state behind a real forward -------------------------------------------------------------------------------------------------
def seg_regions(t, a, M, odt=4):
    """Byte offsets of the step's regions behind the table region: csrc/ragged_multi_guide_host.hpp (rmg_layout) on segment_host.hpp (seg_layout)."""
    r256 = lambda n: (n + 255) // 256 * 256
    off, out = 0, {}
    rows = sum(q * r for q, r in zip(t.Q, t.rows))
    for nbytes in (len(t.Q) * 64, len(t.units) * 32, sum(t.windows) * 4, M * 16, rows * 4):
        off += r256(nbytes)
    Rr, P, windows = M * a.nh, max(a.P, 1), sum(q * w for q, w in zip(t.Q, t.windows))
    score_floats = 16 * sum(p * 32 * n for p, n in zip(t.passes, t.ntiles))
    part_rows = t.slots * 16
    for name, nbytes in (("qp", M * E * 4), ("qhi", Rr * E * 2), ("qlo", Rr * E * 2), ("pos_a", Rr * P * 4), ("scores", score_floats * 4), ("part_m", part_rows * 4),
                         ("part_l", part_rows * 4), ("part_acc", part_rows * E * 4), ("ctxg", Rr * E * 4), ("o", M * E * 4), ("pre", M * E * 4),
                         ("hid", M * a.hidden * 4), ("tok", M * a.hidden * 4), ("ctx16", windows * E * 2)):
        out[name] = (off, nbytes)
        off += r256(nbytes)
    return out


@pytest.mark.parametrize("id", ["rmg_mix6_chunks3", "rmg_mix9"])
def test_train_state_behind_a_real_forward(id):
    c = ri.build(id)
    m = build_module(c)
    ff, fe, g = dev_bf16(np.concatenate(c.ff)), dev_bf16(np.concatenate(c.fe)), dev_bf16(np.concatenate(c.g))
    with torch.no_grad():
        m.forward_ragged_multi_guide(ff, fe, g, c.splits, c.counts, c.modals, chunks=c.entry.chunks)
    (plan,) = m.__dict__["_ragged_multi_guide_plans"].values()
    t, a, M = plan.tables, plan.io, len(plan.tables.pairs)
    reg = seg_regions(t, a, M)
    dev = ff.device
    ctx16 = torch.full((reg["ctx16"][1] // (2 * E), E), float("nan"), dtype=torch.float16, device=dev)
    scores = torch.full((reg["scores"][1] // 4,), float("nan"), device=dev)
    ml, ctxg = torch.full((M * NH, 2), float("nan"), device=dev), torch.full((M * NH, E), float("nan"), device=dev)
    nv.compressor_ragged_multiguide_train_state(a, ctx16, scores, ml, ctxg)
    torch.cuda.synchronize()
    ws = plan.ws
    view = lambda name: ws[reg[name][0]:reg[name][0] + reg[name][1]]
    assert torch.equal(ctx16.view(torch.uint8).reshape(-1), view("ctx16")) and torch.equal(ctxg.view(torch.uint8).reshape(-1), view("ctxg"))
    assert torch.equal(scores.view(torch.uint8), view("scores"))
    assert torch.isfinite(ctx16.float()).all() and torch.isfinite(ctxg).all() and torch.isfinite(ml).all()
    S, mlh, off, row = scores.cpu(), ml.cpu(), 0, 0
    for i in range(c.B):
        N, nr, prows = t.N[i], NH * t.Q[i], 32 * t.passes[i]
        stride = (N + 15) // 16 * 16
        Sd = up(S[off:off + prows * stride].view(prows, stride))[:nr, :N]
        Md = Sd.max(1).values
        Ld = torch.exp(Sd - Md[:, None]).sum(1)
        got = up(mlh[row:row + nr])
        assert torch.equal(got[:, 0], Md), f"item {i}: M is the largest logit of the row"
        rel = float(((got[:, 1] - Ld).abs() / Ld).max())
        bound = (N + t.chunks[i] + 8) * EPS23 + gi.TRANS
        print(f"{id} item {i} ({nr} rows, {t.chunks[i]} chunks): L rel {rel:.3e} (bound {bound:.3e})")
        assert rel <= bound, (i, rel, bound)
        off, row = off + prows * stride, row + nr
