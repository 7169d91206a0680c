"""HIComProjector.open_stream_group_multi (GPU; hicom_amd/clip_stream_group_multi.py, csrc/clip_stream_group_multi.hip): the merge + fold
launch alone against float64, the schedule of tests/clip_stream_group_multi_inputs.py against the CPU oracle on every slot's concatenation
with every guide of the slot, finish_many, and the host behaviour of a push.  tests/test_clip_stream_group_multi_power.py shows on the CPU
that swapped guides, a wrong first pair, row group 0's partials for rows >= 16, pass 0's logits for pass 1, a state shared by a slot's
guides, a shared frame offset, no rescale, finish_many placing at another slot's row or writing an unnamed slot each move a region by >= 4
bars.

Bars.  Parity: <= 1e-3 (clip_stream_inputs.TOL) per region against oracle.projector_forward on the slot's concatenation with guide q; <= 2e-3
against forward() on it (the bar of tests/test_gpu_clip_stream.py).  Each push's local rows equal forward_ragged_multi_guide's on the same
stacked tensor with the same guides and counts bit for bit; newline rows equal image_newline bit for bit; the 32 global rows of a pair are
identical bit for bit; two identical schedules give bit-equal outputs.  The merge + fold launch: M' exact, L' and ACC' within the bound
derived in clip_stream_group_inputs' docstring, computed by the function the single-guide group's test uses (the arithmetic is the same
device function, merge_fold_row).

Measured on an MI355X.  The merge + fold launch over the 24 cases x 3 items x Q guides: L' err <= 6.5e-6, 0 .. 0.031 of the
bound (0 from the empty state with one partial); ACC' err <= 4.5e-6, 0.009 .. 0.030 of the bound; M' exact; the absent slot's NaN pairs
bit-identical.  The schedule at 6 x 6, hidden 64: against the oracle local 4.3e-6 .. 1.8e-5, global 7.9e-7 .. 2.1e-6; against forward() local
1.8e-6 .. 1.1e-5, global 7.7e-6 .. 2.0e-5; against forward_ragged_multi_guide the local rows of every push are bit-equal.  The wide case
(9 x 9, hidden 896): oracle local <= 7.7e-5, global <= 5.7e-6; forward() local <= 3.7e-5, global <= 5.4e-5.  The whole file runs in about 4 s."""
import functools

import numpy as np
import pytest
import torch

import clip_stream_group_multi_inputs as mi
from clip_stream_group_inputs import E, H, ITEMS, N, NSLOTS, P, R, SLOTS, T0S, TC, W, X0, Y0, merge_fold_ref
from gpu_util import build_module, check_table_region, dev_bf16
from hicom_amd import native as nv
from stream_blocks import group_multi_push_block

pytestmark = pytest.mark.gpu

NG = mi.NG
NAN = float("nan")
STORE = "_clip_stream_group_multi_plans"


# =============================================================================================================================
# launch 3 alone: ITEMS chunks with Q guides each; item i's slot is SLOTS[i] of NSLOTS slots with Q guides each (the last slot is absent)
# =============================================================================================================================
def merge_fold_case(Q, nparts, carried, seed):
    """Per-row random inputs in the device layout (NaN everywhere a row must not be read) and, per guide q, the arrays merge_fold_ref takes."""
    rng = np.random.default_rng(seed)
    rows = R * Q
    passes = (rows + 31) // 32
    S = 2 * passes * nparts
    m = rng.normal(0.0, 3.0, (ITEMS, nparts, rows)).astype(np.float32)
    l = rng.uniform(1.0, 40.0, (ITEMS, nparts, rows)).astype(np.float32)
    a = rng.normal(0.0, 5.0, (ITEMS, nparts, rows, E)).astype(np.float32)
    top = m.max(axis=1)                                                                     # [items, rows]: M_c
    lg = rng.normal(0.0, 3.0, (ITEMS, rows, N)).astype(np.float32)
    lg = lg - lg.max(axis=2, keepdims=True) + top[:, :, None]                               # the chunk maximum is the largest logit
    pe = rng.normal(0.0, 1.0, (P, E)).astype(np.float32)
    pm = np.full((ITEMS * S, 16), NAN, dtype=np.float32)
    pl = np.full((ITEMS * S, 16), NAN, dtype=np.float32)
    pacc = np.full((ITEMS * S, 16, E), NAN, dtype=np.float32)
    s = np.full((ITEMS, 32 * passes, N), NAN, dtype=np.float32)
    s[:, :rows] = lg
    for i in range(ITEMS):
        for r in range(rows):
            for c in range(nparts):
                at = i * S + (r >> 4) * nparts + c
                pm[at, r & 15], pl[at, r & 15], pacc[at, r & 15] = m[i, c, r], l[i, c, r], a[i, c, r]
    ml = np.full((NSLOTS * Q * R, 2), NAN, dtype=np.float32)
    acc = np.full((NSLOTS * Q * R, E), NAN, dtype=np.float32)
    for i, slot in enumerate(SLOTS):
        at = slice(slot * Q * R, (slot + 1) * Q * R)
        if carried == "empty":
            ml[at, 0], ml[at, 1], acc[at] = -np.inf, 0.0, 0.0
        else:
            ml[at, 0] = top[i] + {"below": -2.5, "above": 2.5, "equal": 0.0}[carried]
            ml[at, 1] = rng.uniform(1.0, 40.0, rows)
            acc[at] = rng.normal(0.0, 5.0, (rows, E))

    def of_guide(q, ml_, acc_):
        """What merge_fold_ref takes for guide q's R rows: partials [items nparts, R], logits [items, R, N], state [slots, R, 2] / [slots, R, E]."""
        rs = slice(q * R, (q + 1) * R)
        return (m[:, :, rs].reshape(ITEMS * nparts, R), l[:, :, rs].reshape(ITEMS * nparts, R), a[:, :, rs].reshape(ITEMS * nparts, R, E), lg[:, rs], pe,
                ml_.reshape(NSLOTS, Q, R, 2)[:, q], acc_.reshape(NSLOTS, Q, R, E)[:, q])
    return (pm, pl, pacc, s, pe, ml, acc), of_guide


@pytest.mark.parametrize("nparts", [1, 3])
@pytest.mark.parametrize("carried", ["below", "above", "equal", "empty"])
@pytest.mark.parametrize("Q", [1, 2, 4])
def test_merge_fold_launch_against_fp64(Q, nparts, carried):
    """Q = 1: 9 rows; Q = 2: 18 rows, guide 1's heads straddle the two row groups; Q = 4: 36 rows, a second pass."""
    (pm, pl, pacc, s, pe, ml, acc), of_guide = merge_fold_case(Q, nparts, carried, 1000 * Q + 100 * nparts + len(carried))
    d = lambda x: torch.from_numpy(x).cuda()
    ml_d, acc_d = d(ml), d(acc)
    nv.stream_group_multi_merge_fold(d(pm), d(pl), d(pacc), d(s), ITEMS, R, Q, TC, H, W, d(pe), Y0, X0, [slot * Q for slot in SLOTS], T0S, ml_d, acc_d)
    torch.cuda.synchronize()
    got_ml, got_acc = ml_d.cpu().numpy(), acc_d.cpu().numpy()
    absent = slice((NSLOTS - 1) * Q * R, NSLOTS * Q * R)
    assert np.array_equal(got_ml[absent].view(np.uint32), ml[absent].view(np.uint32)), "the absent slot's (M, L) was written"
    assert np.array_equal(got_acc[absent].view(np.uint32), acc[absent].view(np.uint32)), "the absent slot's ACC was written"
    for q in range(Q):
        ref_in = of_guide(q, ml, acc)
        _, _, _, _, _, g_ml, g_acc = of_guide(q, got_ml, got_acc)
        for slot, Mn, Ln, An, l_tol, a_tol in merge_fold_ref(nparts, *ref_in):
            gm, gl, ga = g_ml[slot, :, 0].astype(np.float64), g_ml[slot, :, 1].astype(np.float64), g_acc[slot].astype(np.float64)
            assert np.isfinite(gm).all() and np.isfinite(gl).all() and np.isfinite(ga).all(), "NaN / Inf: a padding row was read, or -inf - -inf"
            l_err, a_err = np.abs(gl - Ln), np.abs(ga - An)
            print(f"CLIPGROUPMULTI merge+fold Q={Q} nparts={nparts} {carried} slot {slot} guide {q}: L err={l_err.max():.3e} ratio={(l_err / l_tol).max():.3e}  "
                  f"ACC err={a_err.max():.3e} ratio={(a_err / a_tol).max():.3e}")
            assert np.array_equal(gm, Mn.astype(np.float32).astype(np.float64)), "M' is a maximum: exact"
            assert (l_err <= l_tol).all() and (a_err <= a_tol).all()


# =============================================================================================================================
# the schedule against the oracle, forward() and forward_ragged_multi_guide
# =============================================================================================================================
@functools.lru_cache(maxsize=None)
def module(key):
    return build_module(mi.build(key))


@functools.lru_cache(maxsize=None)
def device_clips(key):
    c = mi.build(key)
    return [dev_bf16(a) for a in c.gff], [dev_bf16(a) for a in c.gfe], torch.stack([dev_bf16(g) for g in c.mg]), dev_bf16(c.newline)


def open_group(key, counts=mi.COUNTS):
    c = mi.build(key)
    _, _, guides, nl = device_clips(key)
    with torch.no_grad():
        return module(key).open_stream_group_multi(guides[:sum(counts)].contiguous(), counts, c.h, c.w, mi.MAX_FRAMES, nl)


def push(g, key, items, with_fe=True):
    """One push of ((slot, Tc), ...): every slot's next frames of its own clip.  Returns (views, stacked ff, fe)."""
    ffs, fes, _, _ = device_clips(key)
    t0s = [g.frames[s] for s, _ in items]
    ff = torch.cat([ffs[s][t:t + n] for (s, n), t in zip(items, t0s)])
    fe = torch.cat([fes[s][t:t + n] for (s, n), t in zip(items, t0s)]) if with_fe else None
    with torch.no_grad():
        views = g.push(ff, fe, [n for _, n in items], [s for s, _ in items])
    return views, ff, fe


def check(what, got, want, tol=mi.TOL):
    got = got.detach().float().cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    errs = mi.region_errors(got[None], want[None])
    print(f"CLIPGROUPMULTI {what}: local {errs['local']:.3e}  global {errs['global']:.3e}  (bar {tol:.0e})")
    bad = [f"{what} {r} rows: {v:.3e} > {tol:.0e}" for r, v in errs.items() if not v <= tol]
    assert not bad, "; ".join(bad)


def run_schedule(key, schedule, counts, with_fe=True, against_forward=True):
    """Replays the schedule on a group with every check of the module docstring; returns the clones of every finish."""
    c, m = mi.build(key), module(key)
    ffs, fes, guides, nl = device_clips(key)
    g = open_group(key, counts)
    guide0 = list(g.pair0)
    want = iter(mi.final_state(schedule, counts))
    kept, nfin = [], 0
    for op in schedule:
        if op[0] == "reset":
            with torch.no_grad():
                g.reset(op[1], None if op[2] is None else guides[op[2]:op[2] + counts[op[1]]])
            guide0[op[1]] = guide0[op[1]] if op[2] is None else op[2]
            assert g.frames[op[1]] == 0
        elif op[0] == "push":
            views, ff, fe = push(g, key, op[1], with_fe)
            qs = [counts[s] for s, _ in op[1]]
            call_guides = torch.cat([guides[guide0[s]:guide0[s] + counts[s]] for s, _ in op[1]]).contiguous()
            with torch.no_grad():
                rag = m.forward_ragged_multi_guide(ff, fe, call_guides, [n for _, n in op[1]], qs, ["video"] * len(qs), nl)
            torch.cuda.synchronize()
            for (s, n), v, r in zip(op[1], views, rag):
                tail = g.rows(s) - mi.cs_prefix_rows(m, g.frames[s], c)      # (the `one_token` newline row belongs to finish)
                assert v.shape[0] == counts[s] and v.data_ptr() == g.out[g.pair0[s], g.rows(s) - tail - v.shape[1]:].data_ptr()
                assert torch.equal(v, r[:, :v.shape[1]]), f"slot {s}: the chunk's local rows differ from forward_ragged_multi_guide's"
        else:
            fin = next(want)
            with torch.no_grad():
                outs = g.finish_many(op[1])
            torch.cuda.synchronize()
            assert sorted(outs) == sorted(fin)
            kept.append({s: o.clone() for s, o in outs.items()})
            for s, (frames, g0) in fin.items():
                out = outs[s]
                assert out.dtype == torch.float32 and out.shape[0] == counts[s] and g.frames[s] == frames and g.rows(s) == out.shape[1] - NG
                for q in range(counts[s]):
                    tag = f"{key} fe={with_fe} finish {nfin} slot {s} guide {q} ({frames} frames)"
                    check(tag + " vs oracle", out[q], mi.oracle_output(key, s, frames, g0 + q, with_fe))
                    if against_forward:
                        with torch.no_grad():
                            whole = m(ffs[s][:frames], fes[s][:frames] if with_fe else None, guides[g0 + q], "video", nl)
                        check(tag + " vs forward()", out[q], whole.float().cpu().numpy(), 2 * mi.TOL)
                    glob = out[q, -NG:]
                    assert torch.equal(glob, glob[:1].expand_as(glob)), f"the {NG} global rows of slot {s} guide {q} differ"
                    if c.newline is not None:
                        lay = m._layout((frames // mi.KT, c.h // mi.KS, c.w // mi.KS), "video", True, False)
                        assert lay.newline_rows
                        for r in lay.newline_rows:
                            assert torch.equal(out[q, r], nl.float()), f"slot {s} guide {q}: newline row {r}"
            nfin += 1
    return g, kept


@pytest.mark.parametrize("key,with_fe", [(mi.G12, True), (mi.G12, False), (mi.G12_GRID, True), (mi.G12_ONE, True)],
                         ids=["fe", "no_fe", "grid_newline", "one_token_newline"])
def test_schedule_against_the_oracle_forward_and_forward_ragged_multi_guide(key, with_fe):
    _, first = run_schedule(key, mi.SCHEDULE, mi.COUNTS, with_fe)
    if key == mi.G12 and with_fe:
        _, again = run_schedule(key, mi.SCHEDULE, mi.COUNTS, with_fe, against_forward=False)
        for a, b in zip(first, again):
            assert all(torch.equal(a[s], b[s]) for s in a), "two identical schedules differ"


def test_wider_case_two_slots_9x9_hidden_896():
    """27 windows per chunk and guide at hidden 896: the readout's tile choice changes with the row count; the second push has one item."""
    run_schedule(mi.WIDE, mi.SCHEDULE_WIDE, mi.COUNTS_WIDE)


# =============================================================================================================================
# finish_many
# =============================================================================================================================
ALL = ((0, 4), (1, 4), (2, 4))
SENTINEL = 7.0


def test_finish_many_equals_finish_and_leaves_unnamed_slots_alone():
    key = mi.G12_ONE
    g = open_group(key)
    push(g, key, ALL)
    push(g, key, ((1, 4), (2, 8)))
    with torch.no_grad():
        single = {s: g.finish(s).clone() for s in (0, 2)}
    torch.cuda.synchronize()
    behind = g.out[g.pair0[1]:g.pair0[1] + 2, g.rows(1) - 1:]           # slot 1's part behind its local rows (one_token: the newline row is finish's)
    g.out[g.pair0[0]:g.pair0[0] + 1, g.rows(0) - 1:].fill_(SENTINEL)
    g.out[g.pair0[2]:, g.rows(2) - 1:].fill_(SENTINEL)
    behind.fill_(SENTINEL)
    local1 = g.out[g.pair0[1]:g.pair0[1] + 2, :g.rows(1) - 1].clone()
    with torch.no_grad():
        many = g.finish_many([0, 2])
    torch.cuda.synchronize()
    assert sorted(many) == [0, 2]
    for s in (0, 2):
        assert torch.equal(many[s], single[s]), f"finish_many([0, 2])[{s}] differs from finish({s})"
    assert bool((behind == SENTINEL).all()), "finish_many wrote rows of a slot it was not given"
    assert torch.equal(g.out[g.pair0[1]:g.pair0[1] + 2, :g.rows(1) - 1], local1), "finish_many wrote local rows of a slot it was not given"
    with torch.no_grad():
        both = g.finish_many([2, 1])
        alone = g.finish(1).clone()
    torch.cuda.synchronize()
    assert torch.equal(both[1], alone) and torch.equal(both[2], single[2]), "a slot's result depends on which slots are finished with it"


def test_a_never_pushed_slot_does_not_reach_the_others():
    key = mi.G12
    g = open_group(key)
    push(g, key, ((0, 4), (2, 4)))
    g.out[g.pair0[1]:g.pair0[1] + 2].fill_(SENTINEL)
    with torch.no_grad():
        outs = g.finish_many()
    torch.cuda.synchronize()
    assert sorted(outs) == [0, 2]
    for s in (0, 2):
        assert bool(torch.isfinite(outs[s]).all()), f"slot {s}: not finite beside an empty slot"
        for q in range(mi.COUNTS[s]):
            check(f"slot {s} guide {q} beside an empty slot vs oracle", outs[s][q], mi.oracle_output(key, s, 4, g.pair0[s] + q))
    assert bool((g.out[g.pair0[1]:g.pair0[1] + 2] == SENTINEL).all()), "the empty slot's rows were written"
    with torch.no_grad():
        with pytest.raises(ValueError, match="nothing has been pushed into slot 1"):
            g.finish_many([0, 1])


# =============================================================================================================================
# plans and allocation
# =============================================================================================================================
def test_two_groups_of_other_guide_counts_share_a_plan():
    """Counts (2, 2) and (4, 2) on one projector: the push of [4] into slot 1 is one (Tc, Q) tuple, so the second group runs on the plan the
    first built, with its own pair count (6, not 4) and first pair (4, not 2)."""
    key = mi.G12
    m = module(key)
    m.__dict__.pop(STORE, None)
    ga, gb = open_group(key, (2, 2)), open_group(key, (4, 2))
    for g in (ga, gb, ga):
        push(g, key, ((1, 4),))
    plans = m.__dict__[STORE]
    assert len(plans) == 1 and next(iter(plans.values())).hits == 3
    with torch.no_grad():
        out_a, out_b = ga.finish(1), gb.finish(1)
    torch.cuda.synchronize()
    for q in range(2):
        check(f"counts (2, 2): slot 1 guide {q}, 8 frames vs oracle", out_a[q], mi.oracle_output(key, 1, 8, 2 + q))
        check(f"counts (4, 2): slot 1 guide {q}, 4 frames vs oracle", out_b[q], mi.oracle_output(key, 1, 4, 4 + q))



def test_a_second_push_of_the_same_tuple_allocates_nothing_and_builds_no_plan():
    key = mi.G12
    m = module(key)
    m.__dict__.pop(STORE, None)
    g = open_group(key)
    push(g, key, ALL)
    torch.cuda.synchronize()
    ffs, fes, _, _ = device_clips(key)
    stacks = [(torch.cat([ffs[s][t:t + 4] for s in range(3)]), torch.cat([fes[s][t:t + 4] for s in range(3)])) for t in (4, 8)]
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        g.push(*stacks[0], [4, 4, 4])
        g.push(*stacks[1], [4, 4, 4], [0, 1, 2])
    assert torch.cuda.memory_allocated() == before, "push allocated device memory"
    plans = m.__dict__[STORE]
    assert len(plans) == 1 and next(iter(plans.values())).hits == 3, "one plan serves equal (Tc, Q) tuples at different t0"
    with torch.no_grad():
        g.reset(2)
    push(g, key, ((2, 8),))
    assert len(plans) == 2


# the table region hicom_compressor_stream_group_multi_prepare wrote for the host tests' push_block (three items of 4 / 8 / 4 frames with
# 4 / 1 / 2 guides, chunks = 2) at commit 740012d on an MI355X, 256 ints: GmItem x 3 | GmUnit x 8 (item 0 has two passes) | window -> item |
# row -> item
TABLE_REGION = ([0, 144, 4, 0, 4, 0, 2, 0, 4, 0, 0, 4, 0, 0, 0, 0, 144, 288, 8, 4, 8, 8, 2, 576, 1, 16, 16, 8, 0, 0, 0, 0, 432, 144, 4, 12, 4, 12, 2, 1152, 2, 24, 24, 4]
                + [0] * 20
                + [0, 0, 4, 0, 0, 0, 0, 0, 0, 4, 9, 0, 1, 0, 0, 0, 0, 0, 4, 1, 4, 0, 0, 0, 0, 4, 9, 1, 5, 0, 0, 0, 1, 0, 9, 0, 8, 0, 0, 0, 1, 9, 18, 0, 9, 0, 0, 0,
                   2, 0, 4, 0, 12, 0, 0, 0, 2, 4, 9, 0, 13] + [0] * 3
                + [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2] + [0] * 48
                + [0] * 16 + [1] * 8 + [2] * 8 + [0] * 32)


def test_prepare_writes_the_parents_table_region():
    assert len(TABLE_REGION) == 256
    check_table_region(group_multi_push_block(), nv.compressor_stream_group_multi_workspace, nv.compressor_stream_group_multi_prepare, TABLE_REGION)
