"""The native calls of the ragged adaptor backward alone (GPU), from synthetic state (tests/ragged_adapt_bwd_reference.py): seeded dctx,
spiked logits, item levels 16^b apart; every output NaN-filled with guard rows before and after; every NULL-output combination once.

Two yardsticks:
  the single-item calls   per item, ds / pw / sx* / sy* of hicom_compressor_ragged_local_adapt_bwd equal hicom_local_attn_adapt_bwd run on
                          that item alone, and dy / r1 of hicom_compressor_ragged_adapt_dy equal hicom_adapt_dy_fwd on that item alone, BIT
                          FOR BIT (one body, one order: csrc/window_rows.hpp); the column sums within the fp32 summation bound
  fp64                    the reference and the first-order bounds of tests/ragged_adapt_bwd_reference.py
Every check prints `RAGGED_ADAPT_BWD <name> err=<largest error>` and the element nearest to its bound (error, bound, ratio) before it asserts.  Fails without the feature: the
entry points do not exist there."""
import numpy as np
import pytest
import torch

import many_item_inputs as mi
import ragged_adapt_bwd_reference as ref
from gpu_util import build_module, dev_bf16
from hicom_amd import native as nv

pytestmark = pytest.mark.gpu

GUARD = 2                                                # rows in front of and behind every output


@pytest.fixture(scope="module")
def plan():
    """A ragged plan of MIX6 at 6 x 6 whose table region the calls read: one forward_ragged call of the adaptor module builds it."""
    c = mi.build("adaptkv_mix6")
    m = build_module(c)
    with torch.no_grad():
        m.forward_ragged(dev_bf16(np.concatenate(c.ff)), dev_bf16(np.concatenate(c.fe)), dev_bf16(c.g), list(c.splits), list(c.modals))
    (p,) = m.__dict__["_ragged_plans"].values()
    assert [(it[0], it[1]) for it in p.tables.items] == list(ref.ITEMS)
    return m, p


def guarded(shape, dtype):
    """(whole NaN-filled buffer, the view the kernel writes): GUARD rows in front and behind."""
    rows = shape[0] + 2 * GUARD
    whole = torch.full((rows, *shape[1:]), float("nan"), dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + shape[0]]


def guards_intact(whole):
    return bool(torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[-GUARD:]).all())


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def device_state(s):
    d = dict(kx=dev(s["kx"], torch.bfloat16), vx=dev(s["vx"], torch.bfloat16), g=dev(s["g"], torch.bfloat16), dctx=dev(s["dctx"]),
             ky=None if s["ky"] is None else dev(s["ky"]), vy=None if s["vy"] is None else dev(s["vy"]),
             alpha=torch.full((1,), s["alpha"], dtype=torch.bfloat16, device="cuda"))
    for n in ("k", "v"):
        d[n + "norm"] = torch.nn.LayerNorm(ref.D, eps=ref.LN_EPS).to(torch.bfloat16).cuda()
        with torch.no_grad():
            d[n + "norm"].weight.copy_(dev(s[n + "gamma"])), d[n + "norm"].bias.copy_(dev(s[n + "beta"]))
    return d


def run_window(a, s, d, outputs=("sxk", "syk", "sxv", "syv")):
    """The ragged window call on guarded NaN-filled outputs; `outputs`: which of the four sums are given (the rest NULL)."""
    N, NW = sum(s["Ns"]), len(s["wins"])
    bufs = {"ds": guarded((N,), torch.float32), "pw": guarded((N,), torch.float32)}
    for n in outputs:
        if (n != "syk" or s["ky"] is not None) and (n != "syv" or s["vy"] is not None):
            bufs[n] = guarded((NW, ref.D), torch.float32)
    v = {n: b[1] for n, b in bufs.items()}
    nv.compressor_ragged_local_adapt_bwd(a, d["kx"], d["ky"], d["knorm"], d["alpha"], d["vx"], d["vy"], d["vnorm"], d["alpha"], d["g"], d["dctx"], v["ds"], v["pw"],
                                         v.get("sxk"), v.get("syk"), v.get("sxv"), v.get("syv"), eps=ref.LN_EPS)
    torch.cuda.synchronize()
    for n, (whole, view) in bufs.items():
        assert guards_intact(whole), f"{n}: a guard row was written"
        assert not torch.isnan(view).any(), f"{n}: an element was not written"
    return v


def axes_of(T, kt):
    ax = lambda n, k: nv.Axis(n, k, n // k, n // k)
    return ax(T, kt), ax(ref.H, ref.KS), ax(ref.W, ref.KS)


def check(name, got, want, tol):
    err = np.abs(got.double().cpu().numpy() - want)
    i = np.unravel_index(np.argmax(err / np.maximum(tol, 1e-300)), err.shape)         # the element nearest to its bound
    print(f"RAGGED_ADAPT_BWD {name} err={err.max():.3e} nearest to its bound: err {err[i]:.3e} bound {tol[i]:.3e} ratio {err[i] / max(tol[i], 1e-300):.3e}")
    assert (err <= tol).all(), f"{name}: error {err[i]:.3e} over its bound {tol[i]:.3e}"


@pytest.mark.parametrize("adapt", [(True, True), (True, False), (False, True)], ids=["kv", "k", "v"])
def test_window_backward_equals_the_single_item_call_per_item_and_the_fp64_reference(plan, adapt):
    _, p = plan
    a = p.io
    s = ref.state(adapt_k=adapt[0], adapt_v=adapt[1])
    d = device_state(s)
    got = run_window(a, s, d)
    # yardstick 1: the single-item kernel on each item alone, bit for bit
    w0 = 0
    for b, ((T, kt), t0, n) in enumerate(zip(s["items"], s["tok0"], s["Ns"])):
        nw = (T // kt) * (ref.H // ref.KS) * (ref.W // ref.KS)
        sl, wl = slice(t0, t0 + n), slice(w0, w0 + nw)
        f = lambda *sh: torch.full(sh, float("nan"), dtype=torch.float32, device="cuda")
        one = dict(ds=f(n), pw=f(n), sxk=f(nw, ref.D), sxv=f(nw, ref.D), syk=f(nw, ref.D) if adapt[0] else None, syv=f(nw, ref.D) if adapt[1] else None)
        nv.local_attn_adapt_bwd(d["kx"][sl].contiguous(), None if d["ky"] is None else d["ky"][sl].contiguous(), d["knorm"], d["alpha"],
                                d["vx"][sl].contiguous(), None if d["vy"] is None else d["vy"][sl].contiguous(), d["vnorm"], d["alpha"], axes_of(T, kt),
                                d["g"][b].contiguous(), 0, s["scale"], 0.0, d["dctx"][wl].contiguous(), one["ds"], one["pw"], one["sxk"], one["syk"],
                                one["sxv"], one["syv"], eps=ref.LN_EPS)
        torch.cuda.synchronize()
        for n_, t in one.items():
            if t is not None:
                mine = got[n_][sl] if n_ in ("ds", "pw") else got[n_][wl]
                assert torch.equal(mine, t), f"item {b}: {n_} differs from the single-item call"
        w0 += nw
    # yardstick 2: fp64
    want, tol = ref.window_backward(s)
    assert set(want) == set(got)
    for n_ in sorted(want):
        check(f"window[{'k' * adapt[0] + 'v' * adapt[1]}] {n_}", got[n_], want[n_], tol[n_])


NULLS = [(), ("sxk",), ("sxv",), ("syk",), ("syv",), ("sxk", "syk"), ("sxv", "syv"), ("sxk", "sxv"), ("syk", "syv"), ("sxk", "syv"), ("sxv", "syk"),
         ("sxk", "syk", "sxv"), ("sxk", "syk", "syv"), ("sxk", "sxv", "syv"), ("syk", "sxv", "syv"), ("sxk", "syk", "sxv", "syv")]


def test_every_null_output_combination_leaves_the_given_outputs_unchanged(plan):
    """The four sums are optional one by one: all sixteen combinations, each output that is given bit-equal to the call with all four."""
    _, p = plan
    s = ref.state()
    d = device_state(s)
    full = run_window(p.io, s, d)
    assert len(set(NULLS)) == 16
    for given in NULLS:
        got = run_window(p.io, s, d, outputs=given)
        assert set(got) == {"ds", "pw", *given}
        for n_ in got:
            assert torch.equal(got[n_], full[n_]), f"{given}: {n_}"


@pytest.mark.parametrize("stream", ["k", "v", "plain"])
def test_adapt_dy_equals_the_single_item_call_per_item_and_the_fp64_reference(plan, stream):
    """K stream: the rank-1 vector is the item's guide row (bf16, one per item); V stream: dctx (f32, one row per window of the concatenated
    list); plain: alpha = 0 with r1, the use of _plain_stream_grad.  dy, optional r1 and the column sums."""
    _, p = plan
    a = p.io
    s = ref.state()
    d = device_state(s)
    N = sum(s["Ns"])
    rng = np.random.default_rng(11)
    coef = dev((rng.standard_normal(N) * 0.1).astype(np.float32))
    per_item = stream == "k"
    y, norm = (d["ky"], d["knorm"]) if per_item else (d["vy"], d["vnorm"])
    vec = d["g"] if per_item else d["dctx"]
    alpha = torch.zeros(1, dtype=torch.float32, device="cuda") if stream == "plain" else d["alpha"]
    (dy_w, dy), (r1_w, r1) = guarded((N, ref.D), torch.bfloat16), guarded((N, ref.D), torch.bfloat16)
    colsum = nv.compressor_ragged_adapt_dy(a, y, norm.weight.detach(), vec, per_item, coef, alpha, dy, r1, eps=ref.LN_EPS, colsum=True)
    (dy2_w, dy2) = guarded((N, ref.D), torch.bfloat16)
    assert nv.compressor_ragged_adapt_dy(a, y, norm.weight.detach(), vec, per_item, coef, alpha, dy2, None, eps=ref.LN_EPS) is None      # (r1 NULL, no partials)
    torch.cuda.synchronize()
    for whole in (dy_w, r1_w, dy2_w):
        assert guards_intact(whole)
    assert not torch.isnan(dy).any() and not torch.isnan(r1).any() and torch.equal(dy, dy2)
    # yardstick 1: hicom_adapt_dy_fwd per item, bit for bit
    w0 = 0
    for b, ((T, kt), t0, n) in enumerate(zip(s["items"], s["tok0"], s["Ns"])):
        nw = (T // kt) * (ref.H // ref.KS) * (ref.W // ref.KS)
        sl = slice(t0, t0 + n)
        one_dy, one_r1 = torch.empty((n, ref.D), dtype=torch.bfloat16, device="cuda"), torch.empty((n, ref.D), dtype=torch.bfloat16, device="cuda")
        v1, stride = (d["g"][b].contiguous(), 0) if per_item else (d["dctx"][w0:w0 + nw].contiguous(), ref.D)
        nv.adapt_dy(y[sl].contiguous(), norm.weight.detach(), v1, stride, coef[sl].contiguous(), alpha, axes_of(T, kt), one_dy, one_r1, eps=ref.LN_EPS)
        torch.cuda.synchronize()
        assert torch.equal(dy[sl], one_dy) and torch.equal(r1[sl], one_r1), f"item {b}"
        w0 += nw
    # the column sums against the stored dy, in fp64: the fp32 summation bound
    stored = dy.double().cpu().numpy()
    check(f"dy[{stream}] column sums", colsum, stored.sum(0), ref.colsum_bound(stored) + 1e-30)
    # yardstick 2: fp64
    tok_item = np.repeat(np.arange(len(s["Ns"])), s["Ns"])
    tok_win = np.empty(N, dtype=np.int64)
    for w, (_, toks) in enumerate(s["wins"]):
        tok_win[toks] = w
    rows = s["g"][tok_item] if per_item else s["dctx"][tok_win]
    gamma = s["kgamma"] if per_item else s["vgamma"]
    want_dy, want_r1, tol_dy, tol_r1 = ref.adapt_dy((s["ky"] if per_item else s["vy"]), gamma, rows, coef.cpu().numpy(), float(alpha.float()))
    check(f"dy[{stream}] dy", dy, want_dy, tol_dy + 1e-30)
    check(f"dy[{stream}] r1", r1, want_r1, tol_r1 + 1e-30)


def test_dq_item_sums_the_windows_of_each_item_in_a_fixed_order(plan):
    _, p = plan
    s = ref.state()
    NW, B = len(s["wins"]), len(s["Ns"])
    rng = np.random.default_rng(3)
    dq_np = (rng.standard_normal((NW, ref.D)) * (16.0 ** np.array([i for i, _ in s["wins"]]))[:, None]).astype(np.float32)
    dq = dev(dq_np)
    whole, out = guarded((B, ref.D), torch.float32)
    nv.compressor_ragged_dq_item(p.io, dq, out)
    again = torch.empty_like(out)
    nv.compressor_ragged_dq_item(p.io, dq, again)
    torch.cuda.synchronize()
    assert guards_intact(whole) and torch.equal(out, again)
    item = np.array([i for i, _ in s["wins"]])
    want = np.stack([dq_np[item == b].astype(np.float64).sum(0) for b in range(B)])
    tol = np.stack([((item == b).sum() + 4) * ref.EPS32 * np.abs(dq_np[item == b]).astype(np.float64).sum(0) for b in range(B)])
    check("dq_item", out, want, tol + 1e-30)
