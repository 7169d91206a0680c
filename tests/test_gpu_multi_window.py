"""The window bodies of the many-guide local stage -- multi_window_ctx16<NV, NG> and multi_window_adapt_ctx16<NV, NG>
(csrc/multi_window.hpp) through their own entry points hicom_multi_guide_local_fwd and hicom_multi_guide_local_adapt_fwd -- and the
single-guide body local_window_ctx16 (csrc/segment_item.hpp) through forward_batch / forward_ragged, against the float64 references of
tests/multi_window_inputs.py (blend_rows, then window_attention_ref per guide, from the values the kernels received), on that file's
input family: every guide of a window with its own spikes on positions 0, 3, 4, WIN - 1 (lane 63 at WIN 64) and both sides of every
multiple of 8 and 12, one of them left out per (guide, window), y planes whose LayerNorm statistics change by up to 100 x from row to
row.  tests/test_multi_window_power.py shows on the references alone that a body which gives a guide its neighbour's maximum or
weights, reads the guide rows of the group in front, strides its planes by plane - D, loses position 0 or WIN - 1, scales its logits by
1.1, takes mu / rstd from another row, leaves smu out or uses guide 0's cg misses these bounds by a factor of 4 at least.

What is run: multi_window_inputs.RUNS -- WIN 1, 3, 8, 9 (three windows: one live wave in the last workgroup), 16, 36 (eight windows) and
64 (four windows, and one window in one frame); Q = 1 .. 7 and 9 at WIN 36 / 64 (every NG alone, a full group plus every remainder, two
groups plus one), Q = 1, 4, 5 elsewhere; the adaptor on key / value / both with bf16 and f32 alpha; the `far` runs (maxima of
neighbouring guides 110 apart).  Every stream (key, value, guides, both planes) is an interior view of a larger buffer with NaN rows in
front and behind, 16-byte aligned; the output [Q][windows][1152] starts as NaN between two NaN guard planes.  Checked: every guide,
window and element at its bound, every output finite, the guard planes untouched.
Independence (the comments of csrc/multi_window.hpp promise it): guide q's plane of a Q-guide call, bit for bit, is the plane of a call
with that guide alone and of a call with the guides in reversed order -- WIN 36 and WIN 64, both forms.
Single-guide body: forward_batch (3 items of 4 x 6 x 6) and forward_ragged (items of T = 4, 8 and an image) on planted items; ctx16 is
read from the tail of the plan's workspace (csrc/segment_host.hpp, seg_layout: ... ctx16 | hid16 | loc, each rounded up to 256 bytes).
Refusals: WIN 100, an inexact partition, E = 768, a misaligned pointer, both planes NULL -- the error code, the output untouched.

Bounds: multi_window_inputs.bounds, derived there term by term.  Every check prints
`MULTI_WINDOW <name> err=<largest error> bound=<bound there> ratio=<largest error / bound>` before it asserts.

Measured on an MI355X (all runs; largest error, and the largest error / bound of any check of that output): no fault found.
  plain.ctx16   err <= 9.7e-04   ratio <= 1.3e-01        plain.ctx16 (far)   err <= 7.8e-04   ratio <= 1.1e-01
  adapt.ctx16   err <= 3.9e-03   ratio <= 9.9e-02        adapt.ctx16 (far)   err <= 1.0e-03   ratio <= 2.2e-02
  item.ctx16    err <= 9.5e-04   ratio <= 6.6e-02 (forward_batch and forward_ragged)
Every output is held by its one fp16 rounding (errors of half a unit of contexts of size 1 .. 8; the adaptor's second-height value rows
are twenty times as large); the fp32 part of the bounds is never approached.  The independence and refusal tests pass as stated.  The
planted faults of tests/test_multi_window_power.py move an output by 6.5 bounds at the least.  The whole file (137 tests) runs in
about 5 s.
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cases
import multi_window_inputs as mw
import ops_reference as R
from gpu_util import DEV, build_module, check, guarded, ptr, stream
from hicom_amd import native as nv
from hicom_amd import synth
from oracle import hicom_oracle as orc

pytestmark = pytest.mark.gpu

NAN = float("nan")
D = mw.D
EINVAL, EUNSUP = -1, -2


def out_planes(Q, NW):
    """(buffer [Q + 2, NW, D] fp16 of NaN, the view of the Q planes in the middle)."""
    buf = torch.full((Q + 2, NW, D), NAN, dtype=torch.float16, device=DEV)
    return buf, buf[1:-1]


def guards_untouched(buf):
    return bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())


@functools.lru_cache(maxsize=None)
def device_run(run):
    """The uploads of a run, kept for the independence tests."""
    c = mw.build(run)
    d = SimpleNamespace(c=c, guides=guarded(c.guides), keep=[])
    if run.form == "plain":
        d.key, d.value = guarded(c.key), guarded(c.value)
        return d
    d.key, d.value, d.ky, d.vy = guarded(c.kx), guarded(c.vx), guarded(c.ky), guarded(c.vy)
    dev = lambda t: None if t is None else t.to(DEV)
    d.keep = [dev(t) for t in (c.kg, c.kb, c.ak, c.vg, c.vb, c.av)]
    kg, kb, ak, vg, vb, av = d.keep
    d.ak = nv.SegAdaptor(gamma=ptr(kg), beta=ptr(kb), alpha=ptr(ak)) if c.ky is not None else nv.SegAdaptor()
    d.av = nv.SegAdaptor(gamma=ptr(vg), beta=ptr(vb), alpha=ptr(av)) if c.vy is not None else nv.SegAdaptor()
    d.alpha_dt = nv.DT_F32 if run.alpha_dt == "f32" else nv.DT_BF16
    return d


def launch(run, guides=None, Q=None):
    """One call of the run's entry point on `guides` (a guarded device view; default: the run's own); returns (buffer, planes)."""
    d = device_run(run)
    c = d.c
    T, H, W, kt, ks = c.geom
    guides = d.guides if guides is None else guides
    Q = c.Q if Q is None else Q
    buf, out = out_planes(Q, c.NW)
    if run.form == "plain":
        nv.multi_guide_local(ptr(d.key), ptr(d.value), ptr(guides), Q, T, H, W, D, kt, ks, c.scale, out.data_ptr(), stream())
    else:
        nv.multi_guide_local_adapt(ptr(d.key), ptr(d.value), ptr(guides), ptr(d.ky), ptr(d.vy), d.ak, d.av, d.alpha_dt, c.eps, Q, T, H, W, D, kt, ks,
                                   c.scale, out.data_ptr(), stream())
    torch.cuda.synchronize()
    return buf, out


@pytest.mark.parametrize("run", mw.RUNS, ids=[r.id for r in mw.RUNS])
def test_every_guide_plane_matches_the_fp64_reference(run):
    buf, out = launch(run)
    check(f"{run.form}.ctx16[{run.id}]", out, mw.want16(run), mw.bounds(run))
    assert guards_untouched(buf), f"{run.id}: a guard plane was written"


INDEPENDENT = tuple(r for r in mw.RUNS if r.geom in ("w36", "w64") and r.Q in (3, 6, 7, 9) and not r.far and r.which == "both")


@pytest.mark.parametrize("run", INDEPENDENT, ids=[r.id for r in INDEPENDENT])
def test_a_guide_plane_does_not_depend_on_its_group_or_its_place(run):
    """Guide q alone (NG = 1, group offset 0) and the guides in reversed order (another u, another group, another NG for most): the
    plane of guide q, bit for bit."""
    c = mw.build(run)
    _, full = launch(run)
    assert bool(torch.isfinite(full).all())
    for q in range(c.Q):
        buf, one = launch(run, guarded(c.guides[q:q + 1]), 1)
        assert guards_untouched(buf)
        assert torch.equal(one[0], full[q]), f"{run.id}: guide {q} alone differs from its plane of the {c.Q}-guide call"
    buf, rev = launch(run, guarded(c.guides.flip(0)))
    assert guards_untouched(buf)
    assert torch.equal(rev.flip(0), full), f"{run.id}: the planes depend on the order of the guides"


# =============================================================================================================================
# local_window_ctx16 behind forward_batch / forward_ragged
# =============================================================================================================================
@functools.lru_cache(maxsize=None)
def plain_module():
    cfg = SimpleNamespace(**cases.DEFAULT_CFG)
    return build_module(SimpleNamespace(cfg=cfg, sd=synth.synth_state_dict(orc.param_shapes(cfg), tag="multi_window")))


def ctx16_of_plan(plan, windows, hidden, out_bytes):
    r256 = lambda n: (n + 255) // 256 * 256
    off = plan.ws.numel() - r256(windows * hidden * out_bytes) - r256(windows * hidden * 2) - r256(windows * D * 2)
    return plan.ws[off:off + windows * D * 2].view(torch.float16).view(windows, D)


@pytest.mark.parametrize("name", list(mw.ITEM_CASES))
def test_single_guide_body_matches_the_fp64_reference_per_item(name):
    """The fp16 contexts of the step, from the tail of the plan's workspace, item by item: the only place a wrong item pointer, guide
    row or win_item entry shows at the kernel's own precision (the step's outputs lie behind two GEMMs)."""
    c = mw.item_case(name)
    m = plain_module()
    for store in ("_batch_plans", "_ragged_plans"):
        m.__dict__.pop(store, None)
    frames = sum(c.Ts)
    ff = guarded(c.ff).view(frames, mw.ITEM_HW, mw.ITEM_HW, D)
    fe = guarded(c.fe).view(frames, mw.ITEM_HW, mw.ITEM_HW, D)
    g = guarded(c.guides)
    with torch.no_grad():
        if name == "batch":
            out = m.forward_batch(ff.view(len(c.Ts), c.Ts[0], mw.ITEM_HW, mw.ITEM_HW, D), fe.view(len(c.Ts), c.Ts[0], mw.ITEM_HW, mw.ITEM_HW, D), g,
                                  "video", None)
            hidden, dt = out.shape[-1], out.dtype
        else:
            out = m.forward_ragged(ff, fe, g, list(c.Ts), list(c.modals), None)
            hidden, dt = out[0].shape[-1], out[0].dtype
    torch.cuda.synchronize()
    (plan,) = m.__dict__["_batch_plans" if name == "batch" else "_ragged_plans"].values()
    assert abs(plan.io.l_scale - c.scale) < 1e-9
    got = ctx16_of_plan(plan, c.windows, hidden, 4 if dt == torch.float32 else 2).clone()
    w0 = 0
    for i, (want, tol) in enumerate(zip(c.ctx, c.tol)):
        check(f"item.ctx16[{name}, item {i}]", got[w0:w0 + want.shape[0]], want, tol)
        w0 += want.shape[0]
    assert w0 == c.windows


# =============================================================================================================================
# refusals
# =============================================================================================================================
def test_refusals_leave_the_output_untouched():
    """WIN 100, an inexact partition, E = 768, a misaligned pointer, both planes NULL: the error code, nothing launched."""
    L = nv.lib()
    x = torch.zeros(4 * 10 * 10 + 2, D, dtype=torch.bfloat16, device=DEV)[1:-1]
    y = torch.zeros(4 * 10 * 10, D, dtype=torch.float16, device=DEV)
    g = torch.zeros(4, D, dtype=torch.bfloat16, device=DEV)
    w = torch.ones(D, dtype=torch.bfloat16, device=DEV)
    al = torch.tensor([0.5], dtype=torch.bfloat16, device=DEV)
    ad = nv.SegAdaptor(gamma=ptr(w), beta=ptr(w), alpha=ptr(al))
    buf, out = out_planes(4, 400)
    o, s = out.data_ptr(), stream()
    plain = lambda key, T, H, W, E, kt, ks, o_=o: L.hicom_multi_guide_local_fwd(key, ptr(x), ptr(g), 4, T, H, W, E, kt, ks, 0.03, o_, s)
    adapt = lambda key, ky, vy, T, H, W, E, kt, ks: L.hicom_multi_guide_local_adapt_fwd(key, ptr(x), ptr(g), ky, vy, ctypes.byref(ad), ctypes.byref(ad),
                                                                                     nv.DT_BF16, 1e-6, 4, T, H, W, E, kt, ks, 0.03, o, s)
    got = {
        "plain WIN 100": (plain(ptr(x), 4, 10, 10, D, 4, 5), EUNSUP),
        "adapt WIN 100": (adapt(ptr(x), ptr(y), ptr(y), 4, 10, 10, D, 4, 5), EUNSUP),
        "plain inexact": (plain(ptr(x), 4, 7, 6, D, 4, 3), EUNSUP),
        "adapt inexact": (adapt(ptr(x), ptr(y), ptr(y), 7, 6, 6, D, 4, 3), EUNSUP),
        "plain E 768": (plain(ptr(x), 4, 6, 6, 768, 4, 3), EUNSUP),
        "adapt E 768": (adapt(ptr(x), ptr(y), ptr(y), 4, 6, 6, 768, 4, 3), EUNSUP),
        "plain misaligned key": (plain(ptr(x) + 8, 4, 6, 6, D, 4, 3), EINVAL),
        "plain misaligned output": (plain(ptr(x), 4, 6, 6, D, 4, 3, o + 8), EINVAL),
        "adapt misaligned plane": (adapt(ptr(x), ptr(y) + 8, ptr(y), 4, 6, 6, D, 4, 3), EINVAL),
        "adapt both planes NULL": (adapt(ptr(x), None, None, 4, 6, 6, D, 4, 3), EINVAL),
    }
    torch.cuda.synchronize()
    assert all(code == want for code, want in got.values()), got
    assert bool(torch.isnan(buf).all()), "a refused call wrote the output"
