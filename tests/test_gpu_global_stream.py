"""The two global-stage stream kernels (csrc/global_stream.hip) and the merge behind them (csrc/merge.hip) against the float64
references of tests/ops_reference.py (global_stream_ref, global_stream_bwd_ref), computed from the values the kernels received, on
the input family of tests/global_stream_inputs.py: mass on both sides of every chunk and frame boundary, on the clip's first and last
token and on both sides of the first tile boundary; per-row spike sets; positional tables as large as the dot products.
tests/test_global_stream_power.py shows on the references alone that a kernel which loses a chunk's last token, takes a chunk's first
frame for its neighbour, drops a positional term, leaves delta out, leaks a padded row into a real one or scales its logits by 1.1
misses these bounds by a factor of 4 at least, in the forward and in the backward.

Cases (global_stream_inputs.CASES; the form is derived there from the restated predicates, and asserted here against
hicom_global_stream_has_marg for every (case, nparts)):

  case                    (T, H, W)     N    E    R / pad   nparts     t0  form and why
  marg_8x6x6_r27          (8, 6, 6)    288  1152  27 / 32   2, 4, 18    0  wide + marginals: full tiles
  marg_8x6x6_r33          (8, 6, 6)    288  1152  33 / 64   2, 4, 18    5  ... a half-filled row group and a padding-only one
  marg_8x6x6_r288         (8, 6, 6)    288  1152  288       2, 4, 18    5  ... 9 workgroups of two full groups; the 8-row merge apply
  marg_4x7x5_r27 / _r33   (4, 7, 5)    140  1152  27, 33    2, 9      5/0  ... masked tail of 12 tokens
  marg_2x9x9_r27 / _r33   (2, 9, 9)    162  1152  27, 33    2, 11     0/5  ... tail of 2, the frame boundary inside a tile
  marg_2x17x16_r27 / _r33 (2, 17, 16)  544  1152  27, 33    2, 8, 33  5/0  ... H in two marginal blocks, W in exactly one; 33 chunks is
                                                                           the most the merge's weight record has room for (34 tiles)
  span_12x6x6_np2         (12, 6, 6)   432  1152  27 / 32   2           5  wide + marginals, a chunk spanning exactly 8 frames
  span_13x6x6_np2         (13, 6, 6)   468  1152  27 / 32   2           0  9 frames: narrow kernel, two row groups; part_marg refused
  wide_1x12x12_r27        (1, 12, 12)  144  1152  27 / 32   2, 9        0  wide, logit-tensor form (T = 1: no room for the weight
                                                                           record); part_marg refused
  wide_nopos_4x7x5_r27    (4, 7, 5)    140  1152  27 / 32   2, 9        -  wide, pos_a / pos_b NULL
  narrow_e1152_r9         (4, 7, 5)    140  1152  9 / 16    1, 2, 3     5  narrow (one row group)
  narrow_e768_r9          (4, 7, 5)    140   768  9 / 16    1, 2, 3     0  narrow (E = 768)
  narrow_e768_r27         (2, 9, 9)    162   768  27 / 32   1, 2, 3     5  narrow, two row groups at E = 768

What is asserted.  Forward: the logits where they are written; M + log L and the merged, normalised contexts (value-side positional
rows included) through hicom_global_merge_fwd / hicom_global_merge_marg_fwd; the contexts must differ from the reference WITHOUT the
positional rows by more than 10 bounds; the marginal form with and without the logit tensor gives the same partials and merged result
bit for bit.  Backward: ds_out elementwise, part_acc.sum(0) against sum dS x, in the marginal form the t / y / x marginals gathered as
hicom_amd/autograd.py gathers them, and ds_out = None leaves part_acc / part_marg bit-identical.
Every output starts as NaN.  include/hicom_hip.h promises that rows >= `rows` "produce no output": rows >= R of part_m / part_l /
part_acc / part_marg must still be NaN.  The wide kernel does store rows >= R of `scores` / ds_out (inside the [rows_pad, stride]
allocation; the narrow one masks them); those rows are overwritten with NaN before the merge runs, which proves the consumer does not read them, and in the backward they
must be zero or untouched.  The padding columns of part_marg (frames past the 8-frame block's use, H and W up to 16) are zero or
untouched, and no consumer column lies in them.

Bounds: global_stream_inputs.forward_bounds / backward_bounds, derived there term by term from the kernels' operations and the
references' own magnitudes.  Every check prints `GSTREAM <name> err=<largest error> bound=<bound there> ratio=<largest error / bound>`.

Measured on an MI355X (all cases, all chunk counts; largest error and the range of the largest error / bound per check): no fault found.
  scores   err <= 2.5e-06   ratio 2.4e-04 .. 4.8e-04        ds_out     err <= 5.3e-07   ratio 2.6e-04 .. 6.0e-04
  lse      err <= 1.4e-06   ratio 8.9e-05 .. 3.0e-04        part_acc   err <= 3.8e-05   ratio 6.9e-04 .. 2.8e-03
  ctx      err <= 8.2e-06   ratio 5.9e-05 .. 3.5e-04        mT, mY, mX err <= 1.4e-05   ratio 5.4e-04 .. 2.9e-03
  ctx against the reference without the positional rows: 50 .. 110 bounds (must exceed 10)
The bounds are worst-case (every one of the 2 E products rounding the same way), so a correct kernel sits three orders below them;
the planted faults of tests/test_global_stream_power.py move an output by 45 bounds at the least.  The whole file runs in about 3 s.
"""
import pytest
import torch

import global_stream_inputs as gi
from ops_reference import up
from hicom_amd import native as nv

pytestmark = pytest.mark.gpu

NAN = float("nan")
IDS = [e.id for e in gi.CASES]


def nan_dev(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def check(name, got, ref, tol):
    """|got - ref| <= tol elementwise (float64 on the CPU); the figures are printed first."""
    got, ref = up(got), ref.double()
    tol = torch.broadcast_to(tol.double(), ref.shape)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values in the result"
    err = (got - ref).abs()
    ratio = (err / tol.clamp_min(1e-300)).reshape(-1)
    i = int(ratio.argmax())
    print(f"GSTREAM {name} err={float(err.max()):.3e} bound={float(tol.reshape(-1)[i]):.3e} ratio={float(ratio[i]):.3e}")
    assert bool((err <= tol).all()), f"{name}: error {float(err.reshape(-1)[i]):.3e} over its bound {float(tol.reshape(-1)[i]):.3e}"


def untouched(t):
    return bool(torch.isnan(t).all())


def zero_or_untouched(t):
    return bool(((t == 0) | torch.isnan(t)).all())


_DEV = {}


def device_inputs(id):
    if id not in _DEV:
        c = gi.build(id)
        names = ("x", "qhi", "qlo", "pos_a", "pe", "dhi", "dlo", "pos_b", "s_in", "ml", "delta")
        _DEV[id] = {n: (getattr(c, n).cuda() if getattr(c, n) is not None else None) for n in names}
    return _DEV[id]


def geometry(c):
    """(H, W, t0, y0, x0) as the product passes them: without a positional table the clip is one row of N tokens."""
    return (c.H, c.W, c.t0, c.y0, c.x0) if c.entry.pos else (1, c.N, 0, 0, 0)


def native_has_marg(c, nparts):
    return nv.lib().hicom_global_stream_has_marg(c.N, c.E, c.rows_pad, c.H, c.W, nparts)


def marg_layout(c):
    """Column of the first grid row / grid column in a part_marg row: [8 frames | pad to 16 | H | pad to 16 | W | pad to 16]."""
    ybase = 16
    xbase = ybase + 16 * ((c.H + 15) // 16)
    return ybase, xbase, xbase + 16 * ((c.W + 15) // 16)


def check_marg_padding(c, pmarg):
    """Rows >= R untouched; in real rows every column outside [0, 8), [ybase, ybase + H), [xbase, xbase + W) zero or untouched."""
    ybase, xbase, width = marg_layout(c)
    assert pmarg.shape[2] == width == nv.global_stream_marg_width(c.H, c.W)
    assert untouched(pmarg[:, c.R:])
    real = pmarg[:, :c.R]
    assert bool(torch.isfinite(real[:, :, :8]).all()) and bool(torch.isfinite(real[:, :, ybase:ybase + c.H]).all())
    assert bool(torch.isfinite(real[:, :, xbase:xbase + c.W]).all())
    for lo, hi in ((8, ybase), (ybase + c.H, xbase), (xbase + c.W, width)):
        assert zero_or_untouched(real[:, :, lo:hi]), (lo, hi)


# =============================================================================================================================
# forward: hicom_global_stream_fwd / hicom_global_stream_marg_fwd + hicom_global_merge_fwd / hicom_global_merge_marg_fwd
# =============================================================================================================================
def run_forward(c, d, nparts, with_scores, marg):
    H, W, t0, y0, x0 = geometry(c)
    R_, rows_pad, E, N = c.R, c.rows_pad, c.E, c.N
    scores = nan_dev(rows_pad, c.stride) if with_scores else None
    pm, pl, pacc = nan_dev(nparts, rows_pad), nan_dev(nparts, rows_pad), nan_dev(nparts, rows_pad, E)
    pmarg = nan_dev(nparts, rows_pad, nv.global_stream_marg_width(H, W)) if marg else None
    if marg:
        nv.global_stream_marg(d["x"], N, d["qhi"], d["qlo"], d["pos_a"], H, W, t0, y0, x0, scores, pm, pl, pacc, pmarg, rows=R_)
    else:
        nv.global_stream(d["x"], N, d["qhi"], d["qlo"], d["pos_a"], H, W, t0, y0, x0, scores, pm, pl, pacc, rows=R_)
    torch.cuda.synchronize()
    # rows >= R produce no output (include/hicom_hip.h); every real row of every chunk is written
    assert untouched(pm[:, R_:]) and untouched(pl[:, R_:]) and untouched(pacc[:, R_:])
    assert bool(torch.isfinite(pm[:, :R_]).all()) and bool(torch.isfinite(pl[:, :R_]).all()) and bool(torch.isfinite(pacc[:, :R_]).all())
    if marg:
        check_marg_padding(c, pmarg)
    logits = scores.clone() if with_scores else None
    if with_scores:
        scores[R_:] = NAN                       # rows >= R of the logit tensor: whatever the kernel left there, no consumer may read it
    ml, acc = nan_dev(R_, 2), nan_dev(R_, E)
    scratch = nan_dev(max(1, R_ * c.T * (c.H + c.W + 2)))
    if marg:
        nv.global_merge_marg(pm, pl, pacc, pmarg, R_, N, H, W, d["pe"], t0, y0, x0, scratch, ml, acc, normalize=True)
    else:
        nv.global_merge(pm, pl, pacc, R_, scores, N, H, W, d["pe"], t0, y0, x0, scratch, ml, acc, normalize=True)
    torch.cuda.synchronize()
    return dict(scores=logits, pm=pm, pl=pl, pacc=pacc, pmarg=pmarg, ml=ml, acc=acc)


def check_forward(tag, c, fw, fb, out):
    R_, N = c.R, c.N
    if out["scores"] is not None:
        check(f"{tag}.scores", out["scores"][:R_, :N], fw["S"], fb["S"])
    check(f"{tag}.lse", up(out["ml"])[:, 0] + torch.log(up(out["ml"])[:, 1]), fw["lse"], fb["lse"])
    check(f"{tag}.ctx", out["acc"], fw["ctx"], fb["ctx"])
    if c.entry.pos:
        # the value-side positional rows are in the result: against the reference without them it is far outside the bound
        off = float(((up(out["acc"]) - fw["ctx_x"]).abs() / fb["ctx"]).max())
        print(f"GSTREAM {tag}.ctx_without_pe ratio={off:.3e}")
        assert off > 10.0


@pytest.mark.parametrize("id", IDS)
def test_forward_matches_fp64_reference(id):
    c, d, fw = gi.build(id), device_inputs(id), gi.forward_ref(id)
    e = c.entry
    if not id.startswith("span"):
        assert nv.global_stream_nparts(c.N, c.rows_pad) == gi.suggested_nparts(c.N) and gi.suggested_nparts(c.N) in e.nparts
    for nparts in e.nparts:
        fb = gi.forward_bounds(c, fw, nparts)
        tag = f"{id}.p{nparts}"
        if e.form == "marg":
            assert gi.form_of(e, nparts) == "marg" and native_has_marg(c, nparts) == 1
            a = run_forward(c, d, nparts, with_scores=False, marg=True)
            b = run_forward(c, d, nparts, with_scores=True, marg=True)
            check_forward(tag + ".marg", c, fw, fb, a)
            check_forward(tag + ".marg+scores", c, fw, fb, b)
            # with and without the logit tensor: the same partials and the same merged result, bit for bit
            assert torch.equal(a["ml"], b["ml"]) and torch.equal(a["acc"], b["acc"])
            for k in ("pm", "pl", "pacc", "pmarg"):
                assert torch.equal(a[k][:, :c.R], b[k][:, :c.R]), k
        else:
            assert gi.form_of(e, nparts) == e.form and (not e.pos or native_has_marg(c, nparts) == 0)
        # the logit-tensor form (per-frame marginals taken from the logits by the merge): every shape has it
        check_forward(tag + ".logits", c, fw, fb, run_forward(c, d, nparts, with_scores=True, marg=False))


# =============================================================================================================================
# backward: hicom_global_stream_bwd
# =============================================================================================================================
def run_backward(c, d, nparts, with_ds, marg):
    H, W, t0, y0, x0 = geometry(c)
    ds = nan_dev(c.rows_pad, c.stride) if with_ds else None
    part = nan_dev(nparts, c.rows_pad, c.E)
    pmarg = nan_dev(nparts, c.rows_pad, nv.global_stream_marg_width(H, W)) if marg else None
    nv.global_stream_bwd(d["x"], c.N, d["dhi"], d["dlo"], d["pos_b"], H, W, t0, y0, x0, d["s_in"], d["ml"], d["delta"], ds, part, c.R,
                         part_marg=pmarg)
    torch.cuda.synchronize()
    assert untouched(part[:, c.R:]) and bool(torch.isfinite(part[:, :c.R]).all())
    if marg:
        check_marg_padding(c, pmarg)
    if with_ds:
        # rows >= R and the columns behind N: zero or never stored; no garbage of the padded rows' tables, no NaN of s_in's padding
        assert zero_or_untouched(ds[c.R:]) and zero_or_untouched(ds[:c.R, c.N:])
    return dict(ds=ds, part=part, pmarg=pmarg)


def gathered_marginals(c, pmarg, nparts):
    """The t / y / x marginals of dS out of part_marg, as hicom_amd/autograd.py gathers them."""
    ybase, xbase, _ = marg_layout(c)
    idx = nv.marg_frame_index(c.N, c.H, c.W, nparts, pmarg.device)
    assert idx[:, 0].tolist() == gi.chunk_first_frames(c.N, c.H * c.W, nparts)          # the kernels' chunk rule, restated independently
    mT = torch.zeros(c.R, c.T, device=pmarg.device)
    mT.index_add_(1, idx.reshape(-1), pmarg[:, :c.R, :8].permute(1, 0, 2).reshape(c.R, -1))
    return mT, pmarg[:, :c.R, ybase:ybase + c.H].sum(0), pmarg[:, :c.R, xbase:xbase + c.W].sum(0)


@pytest.mark.parametrize("id", IDS)
def test_backward_matches_fp64_reference(id):
    c, d, bw = gi.build(id), device_inputs(id), gi.backward_ref(id)
    e = c.entry
    for nparts in e.nparts:
        bb = gi.backward_bounds(c, bw, nparts)
        tag = f"{id}.p{nparts}"
        marg = e.form == "marg"
        if marg:
            assert native_has_marg(c, nparts) == 1
        a = run_backward(c, d, nparts, with_ds=True, marg=marg)
        check(f"{tag}.ds_out", a["ds"][:c.R, :c.N], bw["dS"], bb["dS"])
        check(f"{tag}.part_acc", a["part"][:, :c.R].sum(0), bw["dSx"], bb["dSx"])
        if marg:
            for name, got, ref, tol in zip(("mT", "mY", "mX"), gathered_marginals(c, a["pmarg"], nparts), bw["marg"], bb["marg"]):
                check(f"{tag}.{name}", got, ref, tol)
            # without the dS tensor: the same partial sums and marginals, bit for bit
            b = run_backward(c, d, nparts, with_ds=False, marg=True)
            assert torch.equal(a["part"][:, :c.R], b["part"][:, :c.R]) and torch.equal(a["pmarg"][:, :c.R], b["pmarg"][:, :c.R])


# =============================================================================================================================
# the boundaries of hicom_global_stream_has_marg
# =============================================================================================================================
@pytest.mark.parametrize("id", [e.id for e in gi.CASES if e.refuse_marg])
def test_part_marg_is_refused_just_outside_the_predicate(id):
    """A chunk spanning 9 frames ((13, 6, 6) in 2 chunks) and a single image (T = 1: no room for the merge's weight record): the
    predicate says 0 and asking for in-kernel marginals returns an error instead of launching."""
    c, d = gi.build(id), device_inputs(id)
    H, W, t0, y0, x0 = geometry(c)
    for nparts in c.entry.nparts:
        assert native_has_marg(c, nparts) == 0 and not gi.has_marg(c.N, c.E, c.rows_pad, H, W, nparts)
        pm, pl, pacc = nan_dev(nparts, c.rows_pad), nan_dev(nparts, c.rows_pad), nan_dev(nparts, c.rows_pad, c.E)
        pmarg = nan_dev(nparts, c.rows_pad, nv.global_stream_marg_width(H, W))
        with pytest.raises(nv.HicomNativeError):
            nv.global_stream_marg(d["x"], c.N, d["qhi"], d["qlo"], d["pos_a"], H, W, t0, y0, x0, None, pm, pl, pacc, pmarg, rows=c.R)
        with pytest.raises(nv.HicomNativeError):
            nv.global_stream_bwd(d["x"], c.N, d["dhi"], d["dlo"], d["pos_b"], H, W, t0, y0, x0, d["s_in"], d["ml"], d["delta"], None, pacc, c.R,
                                 part_marg=pmarg)
        torch.cuda.synchronize()
        assert untouched(pm) and untouched(pacc) and untouched(pmarg)               # nothing was launched
    # the neighbouring shapes inside the predicate
    assert nv.lib().hicom_global_stream_has_marg(432, 1152, 32, 6, 6, 2) == 1
    assert nv.lib().hicom_global_stream_has_marg(468, 1152, 32, 6, 6, 7) == 1
    assert nv.lib().hicom_global_stream_has_marg(544, 1152, 32, 17, 16, 33) == 1 and nv.lib().hicom_global_stream_has_marg(544, 1152, 32, 17, 16, 34) == 0
