"""The window kernels of csrc/local_attn.hip -- local_attn_kernel (plain forward), local_attn_adapt_kernel (forward of the k / v
adaptor recipe), local_attn_bwd_kernel (plain backward) -- and trilinear_pool_kernel (csrc/rowwise_ops.hip) against the float64
references of tests/ops_reference.py (window_attention_ref, window_attention_bwd_ref, trilinear_pool_ref), computed from the values
the kernels received, on the input family of tests/window_attn_inputs.py: every window's mass on its first and last position, on
positions 3 and 4 (the four waves' second tokens), on both sides of every 8- and 12-token pass boundary and of position 64.
tests/test_window_attn_power.py shows on the references alone that a kernel which loses a window's first or last token or a pass's
last one, takes its statistics over 64 scores, starts a trailing window one token late, scales its logits by 1.1, loses an l2norm
bit, leaves delta or the - kc k term out, overwrites where it must accumulate or forgets the key-side gradient misses these bounds by
a factor of 4 at least.

What is run: window_attn_inputs.RUNS (the option matrix: geometries with WIN 1 .. 100 and 2401, exact and overlapping on every
subset of axes, D 768 / 1152, all nine key x value stream dtypes, the four l2norm settings, bf16 / f32 queries shared, per window and
strided, ctx / ctx16 / both with a saturating ctx16, bias 95, the adaptor on key / value / both with bf16 and f32 alpha, the backward
with dkey + dvalue, with value_is_key and with l2norm_key, dls always) and window_attn_inputs.POOLS.
Every stream is uploaded as an interior view of a larger buffer with a NaN row in front and behind (the gaps of a strided query are NaN
too), and every output starts as NaN -- dkey / dvalue over overlapping windows included, where the host clears them itself.

Bounds: window_attn_inputs.forward_bounds / backward_bounds / pool_bounds, derived there term by term.  Every check prints
`WINDOW_ATTN <name> err=<largest error> bound=<bound there> ratio=<largest error / bound>` before it asserts.

Measured on an MI355X (all runs; largest error, and the largest error / bound of any check of that output): no fault found.
  fwd.ctx     err <= 4.5e-03 (the 1e5 value row; 1e-5 elsewhere)   ratio <= 6.2e-04        bwd.dq      err <= 1.6e-04   ratio <= 6.2e-05
  fwd.ctx16   err <= 9.8e-04   ratio <= 1.0e-01 (the fp16 rounding)                     bwd.dls     err <= 3.1e-03   ratio <= 1.7e-05
  adapt.ctx   err <= 7.9e-06   ratio <= 7.6e-05                                         bwd.dkey    err <= 2.7e-01   ratio <= 3.9e-01
  pool        err <= 1.0e-06   ratio <= 1.7e-01                                         bwd.dvalue  err <= 3.3e-01   ratio <= 6.0e-01
The fp32 outputs sit three to four orders below their worst-case bounds (every one of D products rounding the same way); the bf16
outputs dkey / dvalue and ctx16 are held by their own rounding, one unit per store, and sit within a factor of two of it.  The planted
faults of tests/test_window_attn_power.py move an output by 5 bounds at the least.  The whole file runs in about 5 s.
"""
from types import SimpleNamespace

import pytest
import torch

import ops_reference as R
import window_attn_inputs as wi
from ops_reference import up
from hicom_amd import geometry as geo
from hicom_amd import native as nv

pytestmark = pytest.mark.gpu

NAN = float("nan")
DEV = "cuda"


def nan_dev(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def check(name, got, ref, tol):
    """|got - ref| <= tol elementwise (float64 on the CPU); the figures are printed first."""
    got, ref = up(got), ref.double()
    tol = torch.broadcast_to(tol.double(), ref.shape) if torch.is_tensor(tol) else torch.full_like(ref, float(tol))
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values in the result"
    err = (got - ref).abs()
    ratio = err / tol.clamp_min(1e-300)
    i = int(ratio.argmax())
    print(f"WINDOW_ATTN {name} err={float(err.max()):.3e} bound={float(tol.reshape(-1)[i]):.3e} ratio={float(ratio.reshape(-1)[i]):.3e}")
    assert bool((err <= tol).all()), f"{name}: error {float(err.reshape(-1)[i]):.3e} over its bound {float(tol.reshape(-1)[i]):.3e}"


def axes_of(geom):
    """The three hicom_axis of a geometry, from the restated tiling (ops_reference.window_axis)."""
    T, H, W, kt, ks = geom
    return tuple(nv.Axis(n, *R.window_axis(n, k)) for n, k in ((T, kt), (H, ks), (W, ks)))


def test_the_restated_window_geometry_is_the_product_geometry():
    for T, H, W, kt, ks in wi.GEOMS.values():
        for n, k in ((T, kt), (H, ks), (W, ks)):
            a = geo.axis_tiling(n, k)
            assert (a.k, a.nwin, a.nfull) == R.window_axis(n, k), (n, k)


# =============================================================================================================================
# hicom_local_attn_fwd
# =============================================================================================================================
@pytest.mark.parametrize("run", wi.FWD_RUNS, ids=[r.id for r in wi.FWD_RUNS])
def test_local_attn_forward_matches_fp64_reference(run):
    c = wi.build(run)
    ref = wi.reference(run)
    b = wi.forward_bounds(run, ref)
    key = wi.guard_rows(c.key, DEV)
    value = wi.guard_rows(c.value, DEV)
    q = wi.guard_query(c.q, c.q_stride, DEV)
    ctx = nan_dev((c.NW, c.D)) if run.out in ("ctx", "both") else None
    ctx16 = nan_dev((c.NW, c.D), torch.float16) if run.out in ("ctx16", "both") else None
    nv.local_attn(key, value, axes_of(c.geom), q, c.q_stride, c.scale, c.bias, run.l2norm, ctx, ctx16)
    torch.cuda.synchronize()
    if ctx is not None:
        check(f"fwd.ctx[{run.id}]", ctx, ref["ctx"], b["ctx"])
    if ctx16 is not None:
        want = wi.ctx16_of(ref["ctx"])
        sat = ref["ctx"].abs() - b["ctx"] > 65504.0                   # beyond the fp16 range whatever the error: exactly +-65504
        got = up(ctx16)
        assert bool((got[sat] == want[sat]).all()), f"fwd.ctx16[{run.id}]: not saturated at +-65504"
        check(f"fwd.ctx16[{run.id}]", torch.where(sat, want, got), want, b["ctx16"])
        assert int(sat.sum()) == (1 if run.big_value else 0)
    if run.big_value:
        assert float(ref["ctx"][0, 5]) > 65504.0 and float(ctx16[0, 5]) == 65504.0 and float(ctx[0, 5]) > 65504.0


# =============================================================================================================================
# hicom_local_attn_adapt_fwd
# =============================================================================================================================
def _norm(gamma, beta):
    return SimpleNamespace(weight=gamma.to(DEV), bias=beta.to(DEV))


@pytest.mark.parametrize("run", wi.ADAPT_RUNS, ids=[r.id for r in wi.ADAPT_RUNS])
def test_local_attn_adapt_forward_matches_fp64_reference(run):
    c = wi.build(run)
    ref = wi.reference(run)
    b = wi.forward_bounds(run, ref)
    g = lambda t: wi.guard_rows(t, DEV) if t is not None else None
    d = lambda t: t.to(DEV) if t is not None else None
    ctx = nan_dev((c.NW, c.D))
    nv.local_attn_adapt(g(c.kx), g(c.ky), _norm(c.kg, c.kb) if c.ky is not None else None, d(c.ak),
                        g(c.vx), g(c.vy), _norm(c.vg, c.vb) if c.vy is not None else None, d(c.av),
                        axes_of(c.geom), wi.guard_query(c.q, c.q_stride, DEV), c.q_stride, c.scale, c.bias, ctx)
    torch.cuda.synchronize()
    check(f"adapt.ctx[{run.id}]", ctx, ref["ctx"], b["ctx"])


# =============================================================================================================================
# hicom_local_attn_bwd
# =============================================================================================================================
@pytest.mark.parametrize("run", wi.BWD_RUNS, ids=[r.id for r in wi.BWD_RUNS])
def test_local_attn_backward_matches_fp64_reference(run):
    c = wi.build(run)
    ref = wi.reference(run)
    b = wi.backward_bounds(run, ref)
    key = wi.guard_rows(c.key, DEV)
    value = key if run.value_is_key else wi.guard_rows(c.value, DEV)
    out = {"dq": nan_dev((c.NW, c.D)), "dls": nan_dev((c.NW,)), "dvalue": nan_dev((c.N, c.D), torch.bfloat16),
           "dkey": None if run.value_is_key else nan_dev((c.N, c.D), torch.bfloat16)}
    nv.local_attn_bwd(key, value, axes_of(c.geom), wi.guard_query(c.q, c.q_stride, DEV), c.q_stride, c.scale, c.bias, c.dctx.to(DEV),
                      out["dq"], dkey=out["dkey"], l2norm_key=bool(run.l2norm), dls=out["dls"], dvalue=out["dvalue"],
                      value_is_key=run.value_is_key)
    torch.cuda.synchronize()
    for name in wi.bwd_outputs(run):
        check(f"bwd.{name}[{run.id}]", out[name], ref[name], b[name])


def test_local_attn_backward_refusals():
    """value_is_key with dkey, and an unsupported D: an error code, no launch (the outputs stay NaN)."""
    T, H, W, kt, ks = geom = wi.GEOMS["w16"]
    N = T * H * W
    for D, kw in ((768, dict(value_is_key=True, with_dkey=True)), (1024, dict(value_is_key=False, with_dkey=True))):
        x = torch.zeros(N, D, dtype=torch.bfloat16, device=DEV)
        dq, dkey, dvalue = nan_dev((1, D)), nan_dev((N, D), torch.bfloat16), nan_dev((N, D), torch.bfloat16)
        with pytest.raises(nv.HicomNativeError):
            nv.local_attn_bwd(x, x, axes_of(geom), torch.zeros(D, dtype=torch.bfloat16, device=DEV), 0, 0.03, 0.0,
                              torch.zeros(1, D, device=DEV), dq, dkey=dkey, dvalue=dvalue, value_is_key=kw["value_is_key"])
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in (dq, dkey, dvalue))
    with pytest.raises(nv.HicomNativeError):
        nv.local_attn(torch.zeros(N, 1024, dtype=torch.bfloat16, device=DEV), torch.zeros(N, 1024, dtype=torch.bfloat16, device=DEV),
                      axes_of(geom), torch.zeros(1024, dtype=torch.bfloat16, device=DEV), 0, 0.03, 0.0, 0, nan_dev((1, 1024)))


def test_window_whose_lds_does_not_fit_is_refused_without_a_launch():
    """(1, 49, 49), kt = 1, ks = 49: one window of 2401 tokens at D = 768.  The backward's five per-token arrays and the partial rows
    need 60368 bytes of dynamic LDS, over the 60000 the project allows itself: refused, nothing launched.  The forward needs about 22
    KB and runs -- test_local_attn_forward_matches_fp64_reference[fwd-w2401-768] holds it to its bound."""
    geom = wi.GEOMS["w2401"]
    N, D = 2401, 768
    assert wi.Run("fwd", "w2401", 768) in wi.FWD_RUNS
    assert 5 * ((N + 3) // 4 * 4) * 4 + 16 * D > 60000 > 1 * ((N + 3) // 4 * 4) * 4 + 16 * D
    x = torch.zeros(N, D, dtype=torch.bfloat16, device=DEV)
    dq, dvalue = nan_dev((1, D)), nan_dev((N, D), torch.bfloat16)
    with pytest.raises(nv.HicomNativeError):
        nv.local_attn_bwd(x, x, axes_of(geom), torch.zeros(D, dtype=torch.bfloat16, device=DEV), 0, 0.03, 0.0, torch.zeros(1, D, device=DEV),
                          dq, dvalue=dvalue)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dq).all()) and bool(torch.isnan(dvalue).all())


# =============================================================================================================================
# hicom_trilinear_pool_fwd
# =============================================================================================================================
@pytest.mark.parametrize("D", wi.POOL_D)
@pytest.mark.parametrize("shape,out_shape", wi.POOLS)
def test_trilinear_pool_matches_fp64_reference(shape, out_shape, D):
    x = wi.pool_input(shape, D)
    T, H, W = shape
    xd = wi.guard_rows(x.reshape(-1, D), DEV).view(T, H, W, D)
    out = nan_dev((*out_shape, D))
    nv.trilinear_pool(xd, out)
    torch.cuda.synchronize()
    ref, ab, slopes = R.trilinear_pool_ref(up(x), *out_shape)
    check(f"pool[{shape}->{out_shape},D{D}]", out, ref, wi.pool_bounds(shape, ab, slopes))
    if shape == out_shape:
        assert torch.equal(out.cpu(), x.float()), "identity pool: not bit-exact"
