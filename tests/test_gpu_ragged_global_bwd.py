"""hicom_compressor_ragged_global_bwd alone (csrc/ragged_train.hip: planes of dctx, pos_b = dctx . pe^T, ragged_global_stream_bwd_kernel,
ragged_dq_merge_kernel), from synthetic state built on the host -- no forward is run -- in the style of tests/test_gpu_global_stream.py.

Inputs per item (five items of 1, 4, 1, 8, 1 frames at 6 x 6: token offsets 36, 180, 216, 504, none a multiple of a tile, a masked tail
tile in every item; nh = 9 rows per item): seeded bf16 tokens, dctx ~ N(0, 0.05), and the forward's state spiked directly, as
tests/global_stream_inputs.py spikes s_in: logits ~ N(0, 1) + SHIFT at the item's tokens {0, 15, 16, N - 1} and 0.6 SHIFT on both sides of
every chunk boundary of the division the call runs with; row r leaves out spike r mod k.  Item b's logits stand on a level of 16^b - 1, so
the M of neighbouring items differ by a factor of about 16 (0, 15, 255, 4095, 65535) and their L by the items' lengths: a row that took
its neighbour's (M, L) would be off by e^(+-15 ...).  (M, L) in float64 from the fp32 logits, rounded to fp32; delta is the true
dctx_r . ctx_r of these inputs.  Rows >= nh and columns >= N_i of the scores region hold NaN.

dS and dqt against float64 (ops_reference.global_stream_bwd_ref per item) under global_stream_inputs.backward_bounds applied per item with
nparts = the item's work units: the segmented kernel runs the same body.  Two terms that model lacks are derived HERE (it takes pos_b and
the planes as given, this call makes them):
  pos_b    the call forms pos_b = dctx . pe^T itself, an E-term fp32 sum per entry: E 2^-23 (|dctx| . |pe_c|) per positional column c, three
           columns per token, and the planes of dctx it splits itself, PSPLIT |dctx| . |x_n|; both enter dP, so times p in dS
  dqt      = dSx + mt . pe[t..] + my . pe[y..] + mx . pe[x..] in the merge: the marginals' bounds times |pe rows|, + the fp32 sums over
           nparts partial sums and T + H + W positional rows: (nparts + T + H + W + 2) 2^-23 sum |terms|.

ds, dqt and the workspace are NaN-filled with NaN guards around them: every live element is written, the padded tail columns of a live
row are zero, the rows >= nh of an item's region, the partial-sum rows >= nh of a slot and the guards keep their NaN."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

import global_stream_inputs as gi
import many_item_inputs as mi
import ops_reference as R
from hicom_amd import native as nv
from hicom_amd import ragged
from ops_reference import EPS23, sum_tol, up

pytestmark = pytest.mark.gpu

E, NH, H, W, KS, HIDDEN = 1152, 9, 6, 6, 3, 64
SPLITS = (1, 4, 1, 8, 1)
GUARD = 64                      # floats of NaN in front of and behind ds and dqt (256 bytes: the alignment of the regions is kept)


def descriptors():
    return [(T, 4 if T % 4 == 0 else 1, 0, 0, 0, 1, 32) for T in SPLITS]


@functools.lru_cache(maxsize=None)
def case(chunks_per_item):
    """The host tensors of the call for the given work units per item, and the float64 reference and bounds per item."""
    g = torch.Generator().manual_seed(1234 + sum(chunks_per_item))
    rnd = lambda *s: torch.randn(*s, generator=g)
    B, maxT = len(SPLITS), max(SPLITS)
    cap = maxT + 2
    c = SimpleNamespace(y0=cap, x0=cap + H, P=cap + H + W + 3, B=B, R=B * NH)
    c.N = [T * H * W for T in SPLITS]
    c.stride = [(n + 15) // 16 * 16 for n in c.N]
    c.x = rnd(sum(c.N), E).bfloat16().contiguous()
    c.pe = (rnd(c.P, E) * 0.5).contiguous()
    c.dctx = (0.05 * rnd(c.R, E)).contiguous()
    hi = c.dctx.bfloat16()
    gd = up(hi) + up((c.dctx - hi.float()).bfloat16())             # what the planes hold
    pos_b = up(c.dctx) @ up(c.pe).t()
    pos_b_err = sum_tol(E, up(c.dctx).abs() @ up(c.pe).abs().t())
    c.scores = torch.full((16 * sum(c.stride),), float("nan"))
    c.ml = torch.zeros(c.R, 2)
    c.delta = torch.zeros(c.R)
    c.items, tok, off = [], 0, 0
    for b, (T, N, stride, nparts) in enumerate(zip(SPLITS, c.N, c.stride, chunks_per_item)):
        rows = slice(b * NH, (b + 1) * NH)
        toks = mi.edge_tokens(N, nparts)
        tgt = torch.zeros(NH, N, dtype=torch.float64)
        for n in toks:
            tgt[:, n] = gi.SHIFT * mi.spike_weight(n, N)
        for r in range(NH):
            tgt[r, toks[r % len(toks)]] = 0.0
        region = c.scores[16 * off:16 * (off + stride)].view(16, stride)
        region[:NH, :N] = (rnd(NH, N).double() + tgt + (16.0 ** b - 1.0)).float()
        Sd = up(region)[:NH, :N]
        Md = Sd.max(1).values
        c.ml[rows] = torch.stack([Md, torch.exp(Sd - Md[:, None]).sum(1)], 1).float()
        xi = up(c.x[tok:tok + N])
        p = torch.exp(Sd - up(c.ml[rows])[:, 0:1]) / up(c.ml[rows])[:, 1:2]
        dP = R.stream_terms(gd[rows], xi, pos_b[rows], None, H, W, 0, c.y0, c.x0)[0]
        c.delta[rows] = (p * dP).sum(1).float()
        it = SimpleNamespace(entry=SimpleNamespace(pos=True), T=T, H=H, W=W, N=N, E=E, R=NH, s_in=region, ml=c.ml[rows], delta=c.delta[rows],
                             x=c.x[tok:tok + N], rows=rows, off=off, stride=stride, nparts=nparts, toks=toks)
        bw = R.global_stream_bwd_ref(g=gd[rows], x=xi, pos_b=pos_b[rows], S=up(region), ml=up(it.ml), delta=up(it.delta), H=H, W=W, t0i=0, y0i=c.y0,
                                     x0i=c.x0)
        tol = gi.backward_bounds(it, bw, nparts)
        # the two terms the model lacks (module docstring)
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
        tok, off = tok + N, off + stride
    return c


def run(chunks):
    """Prepares the table region of a plain block (no forward), runs the call on NaN-filled outputs; returns (case, ds, dqt, ws, layout)."""
    dev = torch.device("cuda")
    desc = descriptors()
    a = nv.CompressorRaggedArgs()
    items = (nv.RaggedItem * len(desc))(*[nv.RaggedItem(*d) for d in desc])
    a.B, a.H, a.W, a.E, a.hidden, a.ks, a.nh, a.chunks, a.items = len(desc), H, W, E, HIDDEN, KS, NH, chunks, items
    n_cus = torch.cuda.get_device_properties(dev).multi_processor_count
    t = ragged.plan_tables(desc, H, W, KS, n_cus, chunks)
    c = case(tuple(t.chunks))
    pe, kpe = c.pe.to(dev), torch.zeros(8, device=dev)             # (kpe: the forward's table, only its presence is checked)
    a.pe, a.kpe, a.P, a.t_index0, a.y_index0, a.x_index0 = pe.data_ptr(), kpe.data_ptr(), c.P, 0, c.y0, c.x0
    a.stream = torch.cuda.current_stream(dev).cuda_stream
    pws = torch.zeros((nv.compressor_ragged_workspace(a),), dtype=torch.uint8, device=dev)
    a.ws, a.ws_bytes = pws.data_ptr(), pws.numel()
    nv.compressor_ragged_prepare(a)
    assert [tuple(u) for u in pws[4 * 64 * ((16 * c.B + 63) // 64):][:16 * len(t.units)].cpu().numpy().view("int32").reshape(-1, 4)] == \
        [tuple(u) for u in t.units]                                # the device's unit table is the one the spikes were placed for
    nan = lambda n: torch.full((n,), float("nan"), device=dev)
    ds_buf, dqt_buf = nan(c.scores.numel() + 2 * GUARD), nan(c.R * E + 2 * GUARD)
    ds, dqt = ds_buf[GUARD:-GUARD], dqt_buf[GUARD:-GUARD].view(c.R, E)
    total = nv.compressor_ragged_global_bwd_workspace(a)
    ws_buf = torch.full((total + 1024,), 0xFF, dtype=torch.uint8, device=dev)
    x, dctx, delta, scores, ml = (v.to(dev) for v in (c.x, c.dctx, c.delta, c.scores, c.ml))
    before = [v.clone() for v in (x, dctx, delta, scores, ml)]
    nv.compressor_ragged_global_bwd(a, x, dctx, delta, scores, ml, ds, dqt, ws_buf[:total])
    torch.cuda.synchronize()
    assert all(torch.equal(v.view(torch.uint8), w.view(torch.uint8)) for v, w in zip((x, dctx, delta, scores, ml), before)), "an input was written"
    return c, t, ds_buf.cpu(), dqt_buf.cpu(), ws_buf.cpu(), total


def worst(got, want, tol):
    r = ((got - want).abs() / tol)
    return float(r.max())


@pytest.mark.parametrize("chunks", [1, 3, 0], ids=["chunks1", "chunks3", "default"])
def test_dS_and_dqt_against_float64_per_item(chunks):
    c, t, ds_buf, dqt_buf, _, _ = run(chunks)
    ds, dqt = ds_buf[GUARD:-GUARD], dqt_buf[GUARD:-GUARD].view(c.R, E)
    bad = []
    for b, it in enumerate(c.items):
        got_ds = up(ds[16 * it.off:16 * (it.off + it.stride)].view(16, it.stride))[:NH, :it.N]
        got_dq = up(dqt[it.rows])
        assert torch.isfinite(got_ds).all() and torch.isfinite(got_dq).all(), f"item {b}: a live element was not written"
        w_ds, w_dq = worst(got_ds, it.dS, it.dS_tol), worst(got_dq, it.dqt, it.dqt_tol)
        print(f"chunks={chunks} item {b} (N {it.N}, {it.nparts} units, M {float(it.ml[0, 0]):.1f}): dS {float((got_ds - it.dS).abs().max()):.3e} "
              f"({w_ds:.1e} of its bound), dqt {float((got_dq - it.dqt).abs().max()):.3e} ({w_dq:.1e} of its bound), max |dqt| {float(it.dqt.abs().max()):.3e}")
        if not w_ds <= 1.0:
            bad.append(f"item {b} dS: {w_ds:.3f} bounds")
        if not w_dq <= 1.0:
            bad.append(f"item {b} dqt: {w_dq:.3f} bounds")
        # the family does what it is for: the spiked tokens carry the mass, in every row
        mass = (it.dS.abs()[:, it.toks].sum(1) / it.dS.abs().sum(1)).min()
        assert float(mass) > 0.5, (b, float(mass))
    assert not bad, "; ".join(bad)
    assert all(abs(float(a.ml[0, 0]) - float(b_.ml[0, 0])) > 10 for a, b_ in zip(c.items, c.items[1:]))


@pytest.mark.parametrize("chunks", [3, 0], ids=["chunks3", "default"])
def test_every_live_element_is_written_and_nothing_else(chunks):
    c, t, ds_buf, dqt_buf, ws_buf, total = run(chunks)
    ds = ds_buf[GUARD:-GUARD]
    assert torch.isnan(ds_buf[:GUARD]).all() and torch.isnan(ds_buf[-GUARD:]).all(), "dS: written outside the scores region"
    assert torch.isnan(dqt_buf[:GUARD]).all() and torch.isnan(dqt_buf[-GUARD:]).all(), "dqt: written outside its rows"
    assert torch.isfinite(dqt_buf[GUARD:-GUARD]).all()
    for b, it in enumerate(c.items):
        region = ds[16 * it.off:16 * (it.off + it.stride)].view(16, it.stride)
        assert torch.isfinite(region[:NH, :it.N]).all(), f"item {b}: live dS"
        assert (region[:NH, it.N:] == 0).all(), f"item {b}: padded tail columns of a live row"
        assert torch.isnan(region[NH:]).all(), f"item {b}: rows >= nh of the region were written"
    # the workspace: dctx planes [R, E] bf16 x 2, pos_b [R, P] f32, part_acc [slots][16][E] f32, each rounded up to 256 bytes
    r256 = lambda n: (n + 255) // 256 * 256
    slots = len(t.units)
    o_lo, o_pos = r256(c.R * E * 2), 2 * r256(c.R * E * 2)
    o_acc = o_pos + r256(c.R * c.P * 4)
    assert total == o_acc + r256(slots * 16 * E * 4)
    assert (ws_buf[total:] == 0xFF).all(), "written behind the workspace"
    for o in (0, o_lo):
        assert torch.isfinite(ws_buf[o:o + c.R * E * 2].view(torch.bfloat16).float()).all(), "a plane of dctx"
    assert torch.isfinite(ws_buf[o_pos:o_pos + c.R * c.P * 4].view(torch.float32)).all(), "pos_b"
    acc = ws_buf[o_acc:o_acc + slots * 16 * E * 4].view(torch.float32).view(slots, 16, E)
    assert torch.isfinite(acc[:, :NH]).all(), "a partial sum of a live row was not written"
    assert torch.isnan(acc[:, NH:]).all(), "partial-sum rows >= nh were written"
    assert math.isclose(float(up(ws_buf[o_pos:o_pos + 4].view(torch.float32))[0]), float(up(c.dctx[0]) @ up(c.pe[0])), rel_tol=1e-3, abs_tol=1e-4)
