"""The dense 16-bit GEMM kernels of csrc/dense16.hip against the float64 references of tests/ops_reference.py (dense16_ref,
dense16_tn_ref), computed from the values the kernels received, on the input table of tests/dense16_inputs.py (its docstring lists the
cases and what each reaches).  tests/test_dense16_power.py shows on the references alone that a kernel which takes a row's frame from
its 16-row block, swaps y and x, drops an offset, reads the table with pitch N, clamps the rows of the last tile, adds the table
behind ssq or behind the activation, counts padded columns in ssq, swaps two slices, leaves the table out of the pre-activation plane,
reads token rows past Kt or drops a split misses these bounds by a factor of 4 at least.

NT form (hicom_dense16_gemm_fwd), every case with and without the positional table:
  product form   ssq + row_tab and nothing else, as the clip-scale global stage calls it: every [slice, m] entry, NaN-prefilled, in an
                 allocation with one guard row in front and one behind that must stay NaN
  everything     erf GELU, the fp16 plane with n_store = N rounded up to 128 (columns [N, n_store) exact zeros), y f32 + residual, ssq,
                 and with the row epilogue (N % 8 == 0) the pre-activation plane and row_dot with an f32 vector: the order
                 "table, bias, ssq / pre, activation, residual" per element
  type paths     (rows_4x7x5, general_4x7x5) an f32 bias gives the same outputs within the bounds; a bf16 y equals y_f32.to(bfloat16)
  refusals       M % (H W) != 0, tab_ld < N, tab_ld % 4 != 0, a table base off 16 bytes, H = 0: HicomNativeError, nothing written
TN form (hicom_dense16_tn_fwd): the summed product is finite and within the tolerance of test_dense16_tn_matches_torch, two launches
are bit-identical, the partials of splits that own no stage are exact zeros (the allocation's guard partial stays NaN), one split
agrees within the tolerance; refused: splits > ceil(Kt / 64), M % 8 != 0, lda < M.

Bounds: dense16_inputs.nt_bounds / tn_tol.  Every check prints `DENSE16 <name> err=<largest error> bound=<bound there> ratio=<largest
error / bound>`.

Measured on an MI355X (all cases; the range over the cases of the largest error / bound per output): no fault found.
  ssq (both launches)  err <= 1.8e-05  ratio 5.8e-04 .. 2.5e-03      y       err <= 8.0e-07  ratio 5.9e-03 .. 1.1e-02
  row_dot              err <= 4.0e-06  ratio 5.2e-04 .. 3.1e-03      val16   err <= 1.9e-03  ratio 0.35 .. 0.74
  pre16                err <= 1.9e-03  ratio 0.25 .. 0.44
  TN sum               err <= 5.2e-06  ratio <= 9.1e-03              TN one partial  err <= 2.5e-06  ratio <= 5.7e-03
  TN one split         err <= 1.4e-05  ratio <= 2.4e-02
The fp16 planes sit near half their bound (a half-ulp rounding against a one-ulp term); the f32 outputs sit two to three orders below
theirs, and the planted faults of tests/test_dense16_power.py move an output by 500 bounds at the least.  The whole file runs in
about 3 s.
"""
import pytest
import torch

import dense16_inputs as di
from ops_reference import up
from hicom_amd import native as nv

pytestmark = pytest.mark.gpu

NAN = float("nan")
NT_IDS = [e.id for e in di.NT_CASES]
TN_IDS = [e.id for e in di.TN_CASES]


def nan_dev(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def untouched(t):
    return bool(torch.isnan(t).all())


def check(name, got, ref, tol):
    """|got - ref| <= tol elementwise (float64 on the CPU); the figures are printed first."""
    got, ref = up(got), ref.double()
    tol = torch.broadcast_to(torch.as_tensor(tol, dtype=torch.float64), ref.shape)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values in the result"
    err = (got - ref).abs()
    ratio = (err / tol.clamp_min(1e-300)).reshape(-1)
    i = int(ratio.argmax())
    print(f"DENSE16 {name} err={float(err.max()):.3e} bound={float(tol.reshape(-1)[i]):.3e} ratio={float(ratio[i]):.3e}")
    assert bool((err <= tol).all()), f"{name}: error {float(err.reshape(-1)[i]):.3e} over its bound {float(tol.reshape(-1)[i]):.3e}"


_DEV = {}


def device_inputs(id):
    if id not in _DEV:
        c = di.build(id)
        _DEV[id] = {n: getattr(c, n).cuda() for n in ("a", "w", "b", "tab", "res", "vec")}
    return _DEV[id]


def guarded_slices(c):
    """(whole allocation [slices + 2, M], the [slices, M] view the kernel gets): all NaN."""
    full = nan_dev(c.slices + 2, c.M)
    return full, full[1:c.slices + 1]


def guards_untouched(full):
    return untouched(full[0]) and untouched(full[-1])


def row_tab(c, d, table):
    return ((d["tab"],) + c.geom) if table else None


def launch_everything(c, d, table, b=None, y_dtype=torch.float32):
    """The everything-at-once launch; returns the outputs as a dict (pre / rdot only with the row epilogue)."""
    rows = c.N % 8 == 0
    o = {"o16": torch.full((c.M, c.npad), 7.0, dtype=torch.float16, device="cuda"), "y": nan_dev(c.M, c.N, dtype=y_dtype)}
    o["ssq_full"], o["ssq"] = guarded_slices(c)
    if rows:
        o["pre"] = nan_dev(c.M, c.N, dtype=torch.float16)
        o["rdot_full"], o["rdot"] = guarded_slices(c)
    nv.dense16_gemm(d["a"], d["w"], d["b"] if b is None else b, K=c.K, act=nv.ACT_GELU, out_f16=o["o16"], n_store=c.npad, y=o["y"], res=d["res"],
                    ssq=o["ssq"], row_tab=row_tab(c, d, table), row_dot=(d["vec"], o["rdot"]) if rows else None, pre_f16=o.get("pre"))
    torch.cuda.synchronize()
    return o


def check_everything(tag, c, o, ref, bounds):
    check(f"{tag} y", o["y"], ref["y"], bounds["y"])
    check(f"{tag} val16", o["o16"][:, :c.N], ref["val"], bounds["val"])
    assert bool((o["o16"][:, c.N:] == 0).all()), f"{tag}: columns [N, n_store) of the fp16 plane are not exact zeros"
    assert guards_untouched(o["ssq_full"]), f"{tag}: a guard row of ssq was written"
    check(f"{tag} ssq", o["ssq"], ref["ssq"], bounds["ssq"])
    if "pre" in o:
        check(f"{tag} pre16", o["pre"], ref["pre"], bounds["pre"])
        assert guards_untouched(o["rdot_full"]), f"{tag}: a guard row of row_dot was written"
        check(f"{tag} rdot", o["rdot"], ref["rdot"], bounds["rdot"])


@pytest.mark.parametrize("table", [True, False], ids=["tab", "notab"])
@pytest.mark.parametrize("id", NT_IDS)
def test_nt_product_form_ssq_per_slice(id, table):
    c, d = di.build(id), device_inputs(id)
    ref = di.reference(id, table)
    full, ssq = guarded_slices(c)
    nv.dense16_gemm(d["a"], d["w"], d["b"], K=c.K, ssq=ssq, row_tab=row_tab(c, d, table))
    torch.cuda.synchronize()
    assert guards_untouched(full), "a guard row of ssq was written"
    check(f"{id} {'tab' if table else 'notab'} product ssq", ssq, ref["ssq"], di.nt_bounds(c, ref)["ssq"])


@pytest.mark.parametrize("table", [True, False], ids=["tab", "notab"])
@pytest.mark.parametrize("id", NT_IDS)
def test_nt_everything_at_once_per_element(id, table):
    c, d = di.build(id), device_inputs(id)
    ref = di.reference(id, table)
    o = launch_everything(c, d, table)
    assert ("pre" in o) == ("pre" in di.checked_outputs(c))
    check_everything(f"{id} {'tab' if table else 'notab'} all", c, o, ref, di.nt_bounds(c, ref))


@pytest.mark.parametrize("id", ["rows_4x7x5", "general_4x7x5"])
def test_nt_f32_bias_and_bf16_y(id):
    c, d = di.build(id), device_inputs(id)
    ref = di.reference(id)
    b32 = d["b"].float()
    o = launch_everything(c, d, True, b=b32)
    check_everything(f"{id} f32-bias", c, o, ref, di.nt_bounds(c, ref))
    o16 = launch_everything(c, d, True, b=b32, y_dtype=torch.bfloat16)
    assert torch.equal(o16["y"], o["y"].to(torch.bfloat16)), "bf16 y is not the round-to-nearest cast of the f32 y"
    assert torch.equal(o16["ssq"], o["ssq"]) and torch.equal(o16["o16"], o["o16"])
    # the bf16 bias with a bf16 y: the other branch pair of the same stores
    o16b = launch_everything(c, d, True, y_dtype=torch.bfloat16)
    assert torch.equal(o16b["y"], launch_everything(c, d, True)["y"].to(torch.bfloat16))


def test_nt_positional_table_refusals_write_nothing():
    c, d = di.build("rows_4x7x5"), device_inputs("rows_4x7x5")
    H, W, t0, y0, x0 = c.geom
    P, ld = d["tab"].shape
    narrow = d["tab"][:, :128].contiguous()                                           # tab_ld < N
    odd = torch.zeros(P, 138, device="cuda")                                          # tab_ld % 4 != 0
    shifted = torch.zeros(P * ld + 4, device="cuda")[1:1 + P * ld].view(P, ld)        # base 4 bytes off a 16-byte boundary
    assert shifted.data_ptr() % 16 == 4
    bad = {"M % (H W)": (d["tab"], H, W + 1, t0, y0, x0), "tab_ld < N": (narrow, H, W, t0, y0, x0), "tab_ld % 4": (odd, H, W, t0, y0, x0),
           "base alignment": (shifted, H, W, t0, y0, x0), "H = 0": (d["tab"], 0, W, t0, y0, x0)}
    for what, rt in bad.items():
        full, ssq = guarded_slices(c)
        with pytest.raises(nv.HicomNativeError):
            nv.dense16_gemm(d["a"], d["w"], d["b"], K=c.K, ssq=ssq, row_tab=rt)
        torch.cuda.synchronize()
        assert untouched(full), what


# ---- TN -----------------------------------------------------------------------------------------------------------------------------
def tn_operands(id):
    c = di.build_tn(id)
    e = c.entry
    return e, c.a_full.cuda()[:e.Kt], c.b_full.cuda()[:e.Kt]


def tn_partials(a, b, M, N, splits):
    """hicom_dense16_tn_fwd alone: ([splits + 1, M, N] NaN-prefilled, the last one a guard), status."""
    parts = nan_dev(splits + 1, M, N)
    status = nv.lib().hicom_dense16_tn_fwd(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), nv.DT_F16 if a.dtype == torch.float16 else nv.DT_BF16,
                                           a.shape[0], M, N, parts.data_ptr(), N, splits, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return parts, status


@pytest.mark.parametrize("id", TN_IDS)
def test_tn_pitched_ragged_and_empty_splits(id):
    e, a, b = tn_operands(id)
    assert a.is_contiguous() and a.stride(0) == e.lda and b.stride(0) == e.ldb
    want = di.reference_tn(id)
    tol = di.tn_tol(e.Kt, want)
    c = nv.dense16_tn(a, b, M=e.M, N=e.N, splits=e.splits)
    c2 = nv.dense16_tn(a, b, M=e.M, N=e.N, splits=e.splits)
    torch.cuda.synchronize()
    assert c.shape == (e.M, e.N) and c.dtype == torch.float32 and torch.equal(c, c2)
    check(f"{id} sum", c, want, tol)
    parts, status = tn_partials(a, b, e.M, e.N, e.splits)
    assert status == 0 and untouched(parts[e.splits]), "the guard partial was written"
    per, live = di.tn_live_splits(e.Kt, e.splits)
    assert bool(torch.isfinite(parts[:e.splits]).all())
    assert bool((parts[live:e.splits] == 0).all()), "the partial of a split that owns no stage is not exact zeros"
    for s in range(live):
        rows = slice(64 * per * s, min(64 * per * (s + 1), e.Kt))
        check(f"{id} split {s}", parts[s], up(a)[rows, :e.M].t() @ up(b)[rows, :e.N], tol)
    check(f"{id} partials summed", parts[:e.splits].double().sum(0), want, tol)
    if e.splits > 1:
        c1 = nv.dense16_tn(a, b, M=e.M, N=e.N, splits=1)
        torch.cuda.synchronize()
        check(f"{id} one split", c1, want, tol)
        assert float((c1 - c).abs().max()) <= tol


def test_tn_refusals_write_nothing():
    e, a, b = tn_operands("tn_200x136x264_bf16_s3")
    for what, (M, N, splits) in {"splits > stages": (e.M, e.N, 5), "M % 8": (12, e.N, 1), "lda < M": (e.lda + 8, e.N, 1)}.items():
        parts, status = tn_partials(a, b, M, N, splits)
        assert status != 0 and untouched(parts), what
        with pytest.raises(nv.HicomNativeError):
            nv.dense16_tn(a, b, M=M, N=N, splits=splits)
