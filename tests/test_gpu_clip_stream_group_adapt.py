"""HIComProjector.open_stream_group_adapt (GPU; hicom_amd/clip_stream_group_adapt.py, csrc/clip_stream_group_multi.hip: the flavour Adapt):
the adaptor local stage of a push alone against float64, the schedule of tests/clip_stream_group_adapt_inputs.py against the CPU oracle and
forward() on every slot's concatenation with every guide of the slot, against prepare_clip + forward_prepared_many per push and against a
plain module's group, finish_many, and the host behaviour of a push.  tests/test_clip_stream_group_adapt_power.py shows on the CPU that a
dropped plane offset, swapped planes, the previous tick's planes, a blend skipped behind the first item and a k adaptor fed frames_feature
each move every pair they can touch by >= 4 bars, and the nine faults of the many-pair schedule some region.

Bars.  Launch 3 alone: every element within the bound of tests/multi_window_inputs.py (derived there term by term), on that file's input
family -- three packed items of Tc = 4 at 6 x 6 (four windows of 36 tokens each), Q = 1, 4, 5, ky only / vy only / both; NaN guard planes
around the contexts bit-identical; an item's contexts bit-equal at either end of the stack and equal to hicom_multi_guide_local_adapt_fwd
on the item alone.  The schedule: <= 1e-3 per pair and region against oracle.projector_forward, <= 2e-3 against forward() (the project's
bars for this recipe); each push's local rows bit-equal to prepare_clip per chunk + forward_prepared_many over the tick's chunks (the same
window body and context layout; the planes' rows do not depend on the GEMM's M); the 32 global rows of every pair
bit-equal to a plain module's group with the same weights; newline rows bit-exact; two identical schedules bit-equal.

Measured on an MI355X (every figure is printed as `MULTI_WINDOW ...` / `CLIPGROUPADAPT ...` before its assertion).  Launch 3
over the 27 item checks: largest error 1.9e-3, at most 0.036 of its bound.  The schedule at 6 x 6, hidden 64: against the oracle local
1.7e-5 .. 7.6e-5, global 1.5e-6 .. 4.5e-6; against forward() local <= 1.2e-5, global <= 4.5e-6; against prepare_clip + forward_prepared_many
the local rows of every push are bit-equal (59 comparisons).  The wide case (9 x 9, hidden 896): oracle local <= 2.6e-4, global <= 1.5e-5.  The
v adaptor's second layer scaled by 1.5 moves the local rows by 3.1e-3 .. 1.1e-2.  The whole file (20 tests) runs in about 6 s."""
import copy
import functools
from types import SimpleNamespace

import pytest
import torch

import clip_stream_group_adapt_inputs as gi
import multi_window_inputs as mw
import ops_reference as R
import window_attn_inputs as wi
from gpu_util import DEV, build_module, check, dev_bf16, guarded, ptr, stream
from hicom_amd import native as nv
from ops_reference import up

pytestmark = pytest.mark.gpu

NG, NAN, D = gi.NG, float("nan"), mw.D
STORE = "_clip_stream_group_adapt_plans"

# ============================================================================================================================
# launch 3 alone: three packed items of 4 x 6 x 6 (multi_window_inputs' family at the geometry of a chunk), the guides of item i at pair0[i]
# ============================================================================================================================
ITEM_GEOMS = ("w36_t4_a", "w36_t4_b", "w36_t4_c")     # names of this file's own: the seed of a run follows its id
CHUNK_GEOM = (4, 6, 6, 4, 3)                            # one chunk of the schedule: four windows of 36 tokens


def chunk_item(name, Q, which, alpha_dt):
    """multi_window_inputs.build at the geometry of a chunk, which is not among its GEOMS: entered for this one call only, so that the
    family's own run matrix stays what its tests document."""
    mw.GEOMS[name] = CHUNK_GEOM
    try:
        return copy.copy(mw.build(mw.MRun("adapt", name, Q, which, alpha_dt)))
    finally:
        del mw.GEOMS[name]


@functools.lru_cache(maxsize=None)
def packed_case(Q, which, alpha_dt):
    """Three items of multi_window_inputs.build under ONE set of LayerNorm weights (item 0's: a call has one), each with its float64
    reference and bounds from the values the kernel receives."""
    items = [chunk_item(g, Q, which, alpha_dt) for g in ITEM_GEOMS]
    for c in items[1:]:
        c.kg, c.kb, c.vg, c.vb = items[0].kg, items[0].kb, items[0].vg, items[0].vb
    like = wi.Run("adapt", "w36", D)
    for c in items:
        (K, Kab, _), (V, Vab, _) = mw.streams(c)
        per = [R.window_attention_ref(K, V, up(c.guides[q]).expand(c.NW, D), c.geom, c.scale, 0.0, key_ab=Kab, value_ab=Vab) for q in range(Q)]
        tol_rows = R.ln_fp32_tol(up(c.ky), up(c.kg), up(c.kb), mw.EPS)[c.tok] if c.ky is not None else None
        tol = []
        for q in range(Q):
            more = c.scale * float(c.ak.double()) * torch.einsum("wid,d->wi", tol_rows, up(c.guides[q]).abs()) if tol_rows is not None else 0.0
            tol.append(wi.forward_bounds_of(like, c, per[q], more)["ctx16"])
        c.want, c.tol = wi.ctx16_of(torch.stack([fw["ctx"] for fw in per])), torch.stack(tol)
    return items


def launch_packed(items, order, pair0, Q, alone=None):
    """The stand-alone entry on the items in `order` (alone: hicom_multi_guide_local_adapt_fwd on that one item with the same planes);
    returns (buffer with a NaN guard plane at either end, contexts [items, Q, windows, D])."""
    c0 = items[0]
    cat = lambda name: None if getattr(c0, name) is None else guarded(torch.cat([getattr(items[i], name) for i in order]))
    key, value, ky, vy = cat("kx"), cat("vx"), cat("ky"), cat("vy")
    guides = torch.empty((3 * Q, D), dtype=torch.bfloat16)
    for i, p in zip(order, pair0):
        guides[p:p + Q] = items[i].guides
    guides = guarded(guides)
    w = [None if t is None else t.to(DEV) for t in (c0.kg, c0.kb, c0.ak, c0.vg, c0.vb, c0.av)]
    ak = nv.SegAdaptor(gamma=ptr(w[0]), beta=ptr(w[1]), alpha=ptr(w[2])) if ky is not None else nv.SegAdaptor()
    av = nv.SegAdaptor(gamma=ptr(w[3]), beta=ptr(w[4]), alpha=ptr(w[5])) if vy is not None else nv.SegAdaptor()
    adt = nv.DT_F32 if c0.run.alpha_dt == "f32" else nv.DT_BF16
    T, H, W, kt, ks = c0.geom
    n = len(order)
    buf = torch.full((n + 2, Q, c0.NW, D), NAN, dtype=torch.float16, device=DEV)
    if alone is None:
        nv.stream_group_local_adapt(key.view(n * T, H, W, D), value.view(n * T, H, W, D), guides, ky, vy, ak, av, adt, c0.eps, n, Q, T, kt, ks, c0.scale,
                                    list(pair0), buf[1:-1])
    else:
        N = T * H * W
        rows = lambda t: None if t is None else t[alone * N:(alone + 1) * N].data_ptr()
        nv.multi_guide_local_adapt(rows(key), rows(value), guides[pair0[alone]:].data_ptr(), rows(ky), rows(vy), ak, av, adt, c0.eps, Q, T, H, W, D, kt, ks,
                                   c0.scale, buf[1 + alone].data_ptr(), stream())
    torch.cuda.synchronize()
    return buf, buf[1:-1]


@pytest.mark.parametrize("which", mw.WHICH)
@pytest.mark.parametrize("Q", [1, 4, 5])
def test_local_adapt_launch_against_fp64(Q, which):
    """Q = 1: NG = 1 alone; Q = 4: one full guide group; Q = 5: a full group and a remainder of 1."""
    items = packed_case(Q, which, ("bf16", "f32")[Q % 2])
    order, pair0 = (0, 1, 2), (2 * Q, 0, Q)
    buf, out = launch_packed(items, order, pair0, Q)
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all()), "a context row that no pair owns was written"
    for at, i in enumerate(order):
        check(f"group_adapt.ctx16[Q{Q}-{which}] item {i}", out[at], items[i].want, items[i].tol)
    # item 0 last in the stack instead of first, with other first pairs: the same bits
    buf2, out2 = launch_packed(items, (1, 2, 0), (Q, 2 * Q, 0), Q)
    assert bool(torch.isnan(buf2[0]).all()) and bool(torch.isnan(buf2[-1]).all())
    assert torch.equal(out2[2], out[0]) and torch.equal(out2[0], out[1]), "an item's contexts depend on its place in the stack"
    # ... and the one-clip launch on the item alone, with the same rows of the planes
    for alone in (0, 2):
        _, one = launch_packed(items, order, pair0, Q, alone=alone)
        assert torch.equal(one[alone], out[alone]), f"item {alone}: hicom_multi_guide_local_adapt_fwd on the item alone gives other bits"


# ============================================================================================================================
# the schedule against the oracle, forward(), prepare_clip + forward_prepared_many and a plain module's group
# ============================================================================================================================
@functools.lru_cache(maxsize=None)
def _module(key, recipe):
    return build_module(gi.build(key, recipe))


def module(key, recipe=gi.ADAPTKV):
    return _module(key, recipe)             # (one cache entry per module, however the recipe is passed)


@functools.lru_cache(maxsize=None)
def plain_module(key):
    """A plain-recipe module with the same readout and global weights (the plain configuration of the clip's family)."""
    return build_module(SimpleNamespace(cfg=gi.gm.build(key).cfg, sd=gi.plain_state_dict(gi.build(key))))


@functools.lru_cache(maxsize=None)
def device_clips(key):
    c = gi.build(key)
    return [dev_bf16(a) for a in c.gff], [dev_bf16(a) for a in c.gfe], torch.stack([dev_bf16(g) for g in c.mg]), dev_bf16(c.newline)


def open_group(key, counts=gi.COUNTS, recipe=gi.ADAPTKV, m=None):
    c = gi.build(key, recipe)
    _, _, guides, nl = device_clips(key)
    with torch.no_grad():
        return (m or module(key, recipe)).open_stream_group_adapt(guides[:sum(counts)].contiguous(), counts, c.h, c.w, gi.MAX_FRAMES, nl)


def push(g, key, items, with_fe=True):
    """One push of ((slot, Tc), ...): every slot's next frames of its own clip.  Returns (views, per-item (ff, fe) chunks)."""
    ffs, fes, _, _ = device_clips(key)
    t0s = [g.frames[s] for s, _ in items]
    chunks = [(ffs[s][t:t + n], fes[s][t:t + n] if with_fe else None) for (s, n), t in zip(items, t0s)]
    ff = torch.cat([a for a, _ in chunks])
    fe = torch.cat([b for _, b in chunks]) if with_fe else None
    with torch.no_grad():
        views = g.push(ff, fe, [n for _, n in items], [s for s, _ in items])
    return views, chunks


def check_rows(what, got, want, tol):
    got = got.detach().float().cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    errs = gi.pair_errors(got[None], want[None])[0]
    print(f"CLIPGROUPADAPT {what}: local {errs['local']:.3e}  global {errs['global']:.3e}  (bar {tol:.0e})")
    bad = [f"{what} {r} rows: {v:.3e} > {tol:.0e}" for r, v in errs.items() if not v <= tol]
    assert not bad, "; ".join(bad)


def run_schedule(key, schedule, counts, recipe=gi.ADAPTKV, with_fe=True, against_forward=True, against_plain=False):
    """Replays the schedule on a group with every check of the module docstring; returns the clones of every finish."""
    c, m = gi.build(key, recipe), module(key, recipe)
    ffs, fes, guides, nl = device_clips(key)
    g = open_group(key, counts, recipe)
    assert type(g).__name__ == "ClipStreamGroupAdapt"
    gp = None
    if against_plain:
        with torch.no_grad():
            gp = plain_module(key).open_stream_group_multi(guides[:sum(counts)].contiguous(), counts, c.h, c.w, gi.MAX_FRAMES, nl)
    guide0 = list(g.pair0)
    want = iter(gi.final_state(schedule, counts))
    kept, nfin = [], 0
    for op in schedule:
        if op[0] == "reset":
            for grp in (g, gp):
                if grp is not None:
                    with torch.no_grad():
                        grp.reset(op[1], None if op[2] is None else guides[op[2]:op[2] + counts[op[1]]])
            guide0[op[1]] = guide0[op[1]] if op[2] is None else op[2]
            assert g.frames[op[1]] == 0
        elif op[0] == "push":
            views, chunks = push(g, key, op[1], with_fe)
            if gp is not None:
                push(gp, key, op[1], with_fe)
            qs = [counts[s] for s, _ in op[1]]
            call_guides = torch.cat([guides[guide0[s]:guide0[s] + counts[s]] for s, _ in op[1]]).contiguous()
            with torch.no_grad():
                clips = [m.prepare_clip(a, b, "video") for a, b in chunks]
                prepared = m.forward_prepared_many(clips, call_guides, qs, nl)
            torch.cuda.synchronize()
            for (s, n), v, r in zip(op[1], views, prepared):
                assert v.shape[0] == counts[s] and v.data_ptr() == g.out[g.pair0[s], gi.gm.cs_prefix_rows(m, g.frames[s] - n, c):].data_ptr()
                diff = float((v.float() - r[:, :v.shape[1]].float()).abs().max())
                print(f"CLIPGROUPADAPT {key} {recipe} push {op[1]} slot {s}: local rows vs prepare_clip + forward_prepared_many: max |diff| {diff:.3e}")
                assert torch.equal(v, r[:, :v.shape[1]]), f"slot {s}: the chunk's local rows differ from prepare_clip + forward_prepared_many's"
        else:
            fin = next(want)
            with torch.no_grad():
                outs = g.finish_many(op[1])
                pouts = gp.finish_many(op[1]) if gp is not None else None
            torch.cuda.synchronize()
            assert sorted(outs) == sorted(fin)
            kept.append({s: o.clone() for s, o in outs.items()})
            for s, (frames, g0) in fin.items():
                out = outs[s]
                assert out.dtype == torch.float32 and out.shape[0] == counts[s] and g.frames[s] == frames and g.rows(s) == out.shape[1] - NG
                if pouts is not None:
                    assert torch.equal(out[:, -NG:], pouts[s][:, -NG:]), f"slot {s}: the global rows differ from a plain module's group"
                for q in range(counts[s]):
                    tag = f"{key} {recipe} fe={with_fe} finish {nfin} slot {s} guide {q} ({frames} frames)"
                    check_rows(tag + " vs oracle", out[q], gi.oracle_output(key, recipe, s, frames, g0 + q, with_fe), gi.TOL)
                    if against_forward:
                        with torch.no_grad():
                            whole = m(ffs[s][:frames], fes[s][:frames] if with_fe else None, guides[g0 + q], "video", nl)
                        check_rows(tag + " vs forward()", out[q], whole.float().cpu().numpy(), 2 * gi.TOL)
                    glob = out[q, -NG:]
                    assert torch.equal(glob, glob[:1].expand_as(glob)), f"the {NG} global rows of slot {s} guide {q} differ"
                    if c.newline is not None:
                        lay = m._layout((frames // gi.KT, c.h // gi.KS, c.w // gi.KS), "video", True, False)
                        assert lay.newline_rows
                        for r in lay.newline_rows:
                            assert torch.equal(out[q, r], nl.float()), f"slot {s} guide {q}: newline row {r}"
            nfin += 1
    return g, kept


@pytest.mark.parametrize("key,recipe,with_fe", [(gi.G12, gi.ADAPTKV, True), (gi.G12, gi.ADAPTKV, False), (gi.G12_GRID, gi.ADAPTKV, True),
                                                (gi.G12_ONE, gi.ADAPTKV, True), (gi.G12, gi.ADAPTK, True), (gi.G12, gi.ADAPTV, True)],
                         ids=["fe", "no_fe", "grid_newline", "one_token_newline", "adapt_k_only", "adapt_v_only"])
def test_schedule_against_the_oracle_forward_prepared_clips_and_a_plain_group(key, recipe, with_fe):
    first_run = key == gi.G12 and recipe == gi.ADAPTKV and with_fe
    _, first = run_schedule(key, gi.SCHEDULE, gi.COUNTS, recipe, with_fe, against_plain=first_run)
    if first_run:
        _, again = run_schedule(key, gi.SCHEDULE, gi.COUNTS, recipe, with_fe, against_forward=False)
        for a, b in zip(first, again):
            assert all(torch.equal(a[s], b[s]) for s in a), "two identical schedules differ"


def test_wider_case_two_slots_9x9_hidden_896():
    """27 windows per chunk and guide at hidden 896, counts (2, 4); the second push has one item."""
    run_schedule(gi.WIDE, gi.SCHEDULE_WIDE, gi.COUNTS_WIDE, against_forward=False)


# ============================================================================================================================
# finish_many, absent slots
# ============================================================================================================================
ALL = ((0, 4), (1, 4), (2, 4))
SENTINEL = 7.0


def test_finish_many_equals_finish_and_leaves_unnamed_slots_alone():
    key = gi.G12_ONE
    g = open_group(key)
    push(g, key, ALL)
    push(g, key, ((1, 4), (2, 8)))
    with torch.no_grad():
        single = {s: g.finish(s).clone() for s in (0, 2)}
    torch.cuda.synchronize()
    p1 = slice(g.pair0[1], g.pair0[1] + 2)
    behind = g.out[p1, g.rows(1) - 1:]                   # slot 1's part behind its local rows (one_token: the newline row is finish's)
    g.out[g.pair0[0]:g.pair0[0] + 1, g.rows(0) - 1:].fill_(SENTINEL)
    g.out[g.pair0[2]:, g.rows(2) - 1:].fill_(SENTINEL)
    behind.fill_(SENTINEL)
    local1 = g.out[p1, :g.rows(1) - 1].clone()
    with torch.no_grad():
        many = g.finish_many([0, 2])
    torch.cuda.synchronize()
    assert sorted(many) == [0, 2]
    for s in (0, 2):
        assert torch.equal(many[s], single[s]), f"finish_many([0, 2])[{s}] differs from finish({s})"
    assert bool((behind == SENTINEL).all()), "finish_many wrote rows of a slot it was not given"
    assert torch.equal(g.out[p1, :g.rows(1) - 1], local1), "finish_many wrote local rows of a slot it was not given"


def test_an_absent_slots_state_and_output_are_untouched_by_a_push():
    key = gi.G12
    g = open_group(key)
    push(g, key, ALL)
    torch.cuda.synchronize()
    p1 = slice(g.pair0[1], g.pair0[1] + 2)
    rows1 = slice(g.pair0[1] * g.nh, (g.pair0[1] + 2) * g.nh)
    g.out[p1, g.rows(1):].fill_(SENTINEL)
    before = (g.out[p1].clone(), g.state_ml.view(-1, 2)[rows1].clone(), g.state_acc.view(-1, g.E)[rows1].clone())
    push(g, key, ((2, 4), (0, 8)))
    torch.cuda.synchronize()
    after = (g.out[p1], g.state_ml.view(-1, 2)[rows1], g.state_acc.view(-1, g.E)[rows1])
    for name, a, b in zip(("output", "(M, L)", "ACC"), before, after):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), \
            f"the absent slot's {name} changed"


# ============================================================================================================================
# plans, allocation, the weights
# ============================================================================================================================
def test_push_and_finish_many_allocate_nothing_and_a_second_push_builds_no_plan():
    key = gi.G12
    m = module(key)
    m.__dict__.pop(STORE, None)
    g = open_group(key)
    push(g, key, ALL)
    with torch.no_grad():
        g.finish_many()
    torch.cuda.synchronize()
    ffs, fes, _, _ = device_clips(key)
    stacks = [(torch.cat([ffs[s][t:t + 4] for s in range(3)]), torch.cat([fes[s][t:t + 4] for s in range(3)])) for t in (4, 8)]
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        g.push(*stacks[0], [4, 4, 4])
        g.push(*stacks[1], [4, 4, 4], [0, 1, 2])
        outs = g.finish_many()
    assert torch.cuda.memory_allocated() == before, "push or finish_many allocated device memory"
    del outs
    plans = m.__dict__[STORE]
    assert len(plans) == 1 and next(iter(plans.values())).hits == 3, "one plan serves equal (Tc, Q) tuples at different t0"
    with torch.no_grad():
        g.reset(2)
    push(g, key, ((2, 8),))
    assert len(plans) == 2


def test_the_plan_follows_the_adaptor_weights():
    key = gi.G12
    m = module(key)
    w = m.local_compressor.v_proj[2].weight
    first = push(open_group(key), key, ALL)[0]
    first = [v.clone() for v in first]
    with torch.no_grad():
        saved = w.detach().clone()
        w.mul_(1.5)
    try:
        moved = [v.clone() for v in push(open_group(key), key, ALL)[0]]
    finally:
        with torch.no_grad():
            w.copy_(saved)
    back = push(open_group(key), key, ALL)[0]
    torch.cuda.synchronize()
    for s, (a, b, c) in enumerate(zip(first, moved, back)):
        shift = float((a - b).abs().max())
        print(f"CLIPGROUPADAPT slot {s}: the local rows moved by {shift:.3e} under a scaled second layer of the v adaptor")
        assert shift > 0.0, f"slot {s}: the local rows did not follow the adaptor's second-layer weight"
        assert torch.equal(a, c), f"slot {s}: the weights written back do not give the first result"
