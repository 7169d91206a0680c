"""HIComProjector.open_stream_group (GPU; hicom_amd/clip_stream_group.py, csrc/clip_stream_group.hip): the merge + fold kernel alone against
float64, the schedule of tests/clip_stream_group_inputs.py against the CPU oracle on every slot's concatenation, and what only B carried
states behind one push can break.  tests/test_clip_stream_group_power.py shows on the CPU that a push that shares or restarts the frame
offset, swaps slots, shares the row offset, touches an absent slot, does not rescale, resets every slot or normalises the positional term
moves a region by >= 4 bars.

Bars.  Parity: <= 1e-3 (clip_stream_inputs.TOL) per region against oracle.projector_forward on the slot's concatenation; <= 2e-3 against
forward() on it (the bar of tests/test_gpu_clip_stream.py).  Each push's local rows equal forward_ragged's on the same stacked tensor with
the same guides bit for bit (one device body, the same GEMMs on the same windows); newline rows equal image_newline bit for bit; the 32
global rows of a slot are identical bit for bit.  The merge + fold kernel: M' exact, L' and ACC' within the bound derived in
clip_stream_group_inputs' docstring (the un-normalised merge terms of global_stream_inputs.forward_bounds with the positional rows, plus
the fold bound of tests/test_gpu_clip_stream.py for one more term).

Measured on an MI355X (DESIGN.md §3.15 has the table).  The merge + fold kernel over the 12 cases x 3 items: L' err <= 7.2e-6, 0.009 .. 0.038
of the bound (0 from the empty state with one partial); ACC' err <= 4.6e-6, 0.009 .. 0.030 of the bound; M' exact; the absent slot's NaN
state bit-identical.  The schedule at 6 x 6, hidden 64: against the oracle local 2.0e-6 .. 1.8e-5, global 8.2e-8 .. 1.5e-7; against forward()
local 5.2e-7 .. 7.4e-6 (forward() runs the fused ring kernel, another body), global 6.2e-6 .. 1.9e-5; against forward_ragged the local rows
of every push are bit-equal.  The wide case (9 x 9, hidden 896): oracle local 6.2e-5, global 6.6e-7; forward() local 3.1e-5, global 5.6e-5.
The whole file runs in about 4 s."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import clip_stream_group_inputs as gi
from clip_stream_group_inputs import E, H, ITEMS, N, NSLOTS, P, R, RP, SLOTS, T0S, TC, W, X0, Y0, merge_fold_ref
from gpu_util import build_module, check_table_region, dev_bf16
from stream_blocks import group_push_block
from hicom_amd import native as nv

pytestmark = pytest.mark.gpu

NG = gi.NG
NAN = float("nan")
STORE = "_clip_stream_group_plans"


def merge_fold_inputs(nparts, carried, seed):
    rng = np.random.default_rng(seed)
    pm = np.full((ITEMS * nparts, RP), NAN, dtype=np.float32)
    pl = np.full((ITEMS * nparts, RP), NAN, dtype=np.float32)
    pacc = np.full((ITEMS * nparts, RP, E), NAN, dtype=np.float32)
    pm[:, :R] = rng.normal(0.0, 3.0, (ITEMS * nparts, R))
    pl[:, :R] = rng.uniform(1.0, 40.0, (ITEMS * nparts, R))
    pacc[:, :R] = rng.normal(0.0, 5.0, (ITEMS * nparts, R, E))
    top = pm[:, :R].reshape(ITEMS, nparts, R).max(axis=1)                                   # [items, R]: M_c
    s = np.full((ITEMS, RP, N), NAN, dtype=np.float32)
    lg = rng.normal(0.0, 3.0, (ITEMS, R, N)).astype(np.float32)
    s[:, :R] = lg - lg.max(axis=2, keepdims=True) + top[:, :, None]                         # the chunk maximum is the largest logit
    pe = rng.normal(0.0, 1.0, (P, E)).astype(np.float32)
    ml = np.full((NSLOTS, R, 2), NAN, dtype=np.float32)
    acc = np.full((NSLOTS, R, E), NAN, dtype=np.float32)
    for i, slot in enumerate(SLOTS):
        if carried == "empty":
            ml[slot, :, 0], ml[slot, :, 1], acc[slot] = -np.inf, 0.0, 0.0
        else:
            ml[slot, :, 0] = top[i] + {"below": -2.5, "above": 2.5, "equal": 0.0}[carried]
            ml[slot, :, 1] = rng.uniform(1.0, 40.0, R)
            acc[slot] = rng.normal(0.0, 5.0, (R, E))
    return pm, pl, pacc, s, pe, ml, acc


@pytest.mark.parametrize("nparts", [1, 3, 7])
@pytest.mark.parametrize("carried", ["below", "above", "equal", "empty"])
def test_merge_fold_kernel_against_fp64(nparts, carried):
    pm, pl, pacc, s, pe, ml, acc = merge_fold_inputs(nparts, carried, 100 * nparts + len(carried))
    d = lambda x: torch.from_numpy(x).cuda()
    ml_d, acc_d = d(ml), d(acc)
    nv.stream_group_merge_fold(d(pm), d(pl), d(pacc), d(s), ITEMS, R, TC, H, W, d(pe), Y0, X0, SLOTS, T0S, ml_d, acc_d)
    torch.cuda.synchronize()
    got_ml, got_acc = ml_d.cpu().numpy(), acc_d.cpu().numpy()
    absent = NSLOTS - 1
    assert np.array_equal(got_ml[absent].view(np.uint32), ml[absent].view(np.uint32)), "the absent slot's (M, L) was written"
    assert np.array_equal(got_acc[absent].view(np.uint32), acc[absent].view(np.uint32)), "the absent slot's ACC was written"
    for slot, Mn, Ln, An, l_tol, a_tol in merge_fold_ref(nparts, pm, pl, pacc, s, pe, ml, acc):
        gm, gl, ga = got_ml[slot, :, 0].astype(np.float64), got_ml[slot, :, 1].astype(np.float64), got_acc[slot].astype(np.float64)
        assert np.isfinite(gm).all() and np.isfinite(gl).all() and np.isfinite(ga).all(), "NaN / Inf: a padding row was read, or -inf - -inf"
        l_err, a_err = np.abs(gl - Ln), np.abs(ga - An)
        print(f"CLIPGROUP merge+fold nparts={nparts} {carried} slot {slot}: L err={l_err.max():.3e} ratio={(l_err / l_tol).max():.3e}  "
              f"ACC err={a_err.max():.3e} ratio={(a_err / a_tol).max():.3e}")
        assert np.array_equal(gm, Mn.astype(np.float32).astype(np.float64)), "M' is a maximum: exact"
        assert (l_err <= l_tol).all() and (a_err <= a_tol).all()


# =============================================================================================================================
# the schedule against the oracle, forward() and forward_ragged
# =============================================================================================================================
@functools.lru_cache(maxsize=None)
def module(key):
    return build_module(gi.build(key))


@functools.lru_cache(maxsize=None)
def device_clips(key):
    c = gi.build(key)
    return [dev_bf16(a) for a in c.gff], [dev_bf16(a) for a in c.gfe], torch.stack([dev_bf16(g) for g in c.gg]), dev_bf16(c.newline)


def open_group(key, nslots=gi.B, max_frames=None):
    c = gi.build(key)
    _, _, guides, nl = device_clips(key)
    with torch.no_grad():
        return module(key).open_stream_group(guides[:nslots].contiguous(), c.h, c.w, max_frames or c.T, nl)


def push(g, key, items, with_fe=True, wrap=False):
    """One push of ((slot, Tc), ...): every slot's next frames of its own clip (wrap: modulo the clip).  Returns (views, stacked ff, fe, t0s)."""
    ffs, fes, _, _ = device_clips(key)
    T = gi.build(key).T
    t0s = [g.frames[s] for s, _ in items]
    at = [t % T if wrap else t for t in t0s]
    ff = torch.cat([ffs[s][t:t + n] for (s, n), t in zip(items, at)])
    fe = torch.cat([fes[s][t:t + n] for (s, n), t in zip(items, at)]) if with_fe else None
    with torch.no_grad():
        views = g.push(ff, fe, [n for _, n in items], [s for s, _ in items])
    return views, ff, fe, t0s


def check(what, got, want, tol=gi.TOL):
    got = got.detach().float().cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    errs = gi.region_errors(got, want)
    print(f"CLIPGROUP {what}: local {errs['local']:.3e}  global {errs['global']:.3e}  (bar {tol:.0e})")
    bad = [f"{what} {r} rows: {v:.3e} > {tol:.0e}" for r, v in errs.items() if not v <= tol]
    assert not bad, "; ".join(bad)


def run_schedule(key, schedule, nslots, with_fe=True):
    """Replays the schedule on a group with every check of the module docstring."""
    c, m = gi.build(key), module(key)
    ffs, fes, guides, nl = device_clips(key)
    g = open_group(key, nslots)
    guide = list(range(nslots))
    want = iter(gi.final_state(schedule, nslots))
    nfin = 0
    for op in schedule:
        if op[0] == "reset":
            with torch.no_grad():
                g.reset(op[1], None if op[2] is None else guides[op[2]])
            guide[op[1]] = guide[op[1]] if op[2] is None else op[2]
            assert g.frames[op[1]] == 0
        elif op[0] == "push":
            views, ff, fe, _ = push(g, key, op[1], with_fe)
            with torch.no_grad():
                rag = m.forward_ragged(ff, fe, guides[[guide[s] for s, _ in op[1]]].contiguous(), [n for _, n in op[1]], "video", nl)
            torch.cuda.synchronize()
            for (s, n), v, r in zip(op[1], views, rag):
                assert v.shape == r[:-NG].shape and v.data_ptr() == g.out[s, g.rows(s) - v.shape[0]:].data_ptr()
                assert torch.equal(v, r[:-NG]), f"slot {s}: the chunk's local rows differ from forward_ragged's"
        else:
            for s, (frames, gidx) in next(want).items():
                with torch.no_grad():
                    out = g.finish(s)
                    whole = m(ffs[s][:frames], fes[s][:frames] if with_fe else None, guides[gidx], "video", nl)
                torch.cuda.synchronize()
                tag = f"{key} fe={with_fe} finish {nfin} slot {s} ({frames} frames, guide {gidx})"
                assert out.dtype == torch.float32 and g.frames[s] == frames and g.rows(s) == out.shape[0] - NG
                check(tag + " vs oracle", out, gi.oracle_output(key, s, frames, gidx, with_fe))
                check(tag + " vs forward()", out, whole.float().cpu().numpy(), 2 * gi.TOL)
                glob = out[-NG:]
                assert torch.equal(glob, glob[:1].expand_as(glob)), f"the {NG} global rows of slot {s} differ"
                if c.newline is not None:
                    lay = m._layout((frames // gi.KT, c.h // gi.KS, c.w // gi.KS), "video", True, False)
                    assert lay.newline_rows
                    for r in lay.newline_rows:
                        assert torch.equal(out[r], nl.float()), f"slot {s}: newline row {r}"
            nfin += 1
    return g


@pytest.mark.parametrize("key,with_fe", [(gi.G12, True), (gi.G12, False), (gi.G12_GRID, True)], ids=["fe", "no_fe", "grid_newline"])
def test_schedule_against_the_oracle_forward_and_forward_ragged(key, with_fe):
    run_schedule(key, gi.SCHEDULE, gi.B, with_fe)


def test_wider_case_two_slots_9x9_hidden_896():
    """27 windows per chunk at hidden 896: the readout's tile choice changes with the row count; the second push has one item."""
    run_schedule(gi.WIDE, gi.SCHEDULE_WIDE, 2)


# =============================================================================================================================
# state behaviour
# =============================================================================================================================
ALL = ((0, 4), (1, 4), (2, 4))


def finish_all(g, slots=range(gi.B)):
    with torch.no_grad():
        outs = {s: g.finish(s).clone() for s in slots}
    torch.cuda.synchronize()
    return outs


def test_finish_does_not_consume_the_state():
    key = gi.G12
    g = open_group(key)
    push(g, key, ALL)
    push(g, key, ALL)
    first = finish_all(g)
    again = finish_all(g)
    assert all(torch.equal(first[s], again[s]) for s in first), "finish() twice without a push"
    check("8 frames of slot 1 vs oracle", first[1], gi.oracle_output(key, 1, 8, 1))
    push(g, key, ALL)
    longer = finish_all(g)
    for s in range(gi.B):
        check(f"push, finish, push, finish: slot {s} vs oracle on 12 frames", longer[s], gi.oracle_output(key, s, 12, s))
        assert torch.equal(longer[s][:first[s].shape[0] - NG], first[s][:-NG]), "the rows of the earlier chunks stay"


def test_reset_replays_bit_for_bit_and_leaves_the_other_slots_alone():
    """Equal call tuples make equal work divisions, so whole runs can be compared bit for bit: four pushes of all slots with and without
    reset(1) behind the second (16 frames of capacity; the clips wrap)."""
    key = gi.G12
    plain = open_group(key, max_frames=16)
    for _ in range(4):
        push(plain, key, ALL, wrap=True)
    no_reset = finish_all(plain)
    g = open_group(key, max_frames=16)
    push(g, key, ALL)
    push(g, key, ALL)
    first = finish_all(g, [1])[1]
    with torch.no_grad():
        g.reset(1)
    assert g.frames == [8, 0, 8]
    push(g, key, ALL, wrap=True)
    push(g, key, ALL, wrap=True)
    outs = finish_all(g)
    assert torch.equal(outs[1], first), "reset(slot) and replay"
    assert torch.equal(outs[0], no_reset[0]) and torch.equal(outs[2], no_reset[2]), "a reset of slot 1 moved another slot"


def test_a_group_and_a_plain_stream_on_one_projector_do_not_disturb_each_other():
    key = gi.G12
    ffs, fes, guides, nl = device_clips(key)
    c, m = gi.build(key), module(key)

    def plain_stream():
        with torch.no_grad():
            return m.open_stream(guides[0], c.h, c.w, c.T, nl)
    solo_s = plain_stream()
    with torch.no_grad():
        for t in (0, 4, 8):
            solo_s.push(ffs[0][t:t + 4], fes[0][t:t + 4])
        solo_stream = solo_s.finish().clone()
    solo_g = open_group(key)
    for _ in range(3):
        push(solo_g, key, ALL)
    solo_group = finish_all(solo_g)
    s, g = plain_stream(), open_group(key)
    with torch.no_grad():
        for t in (0, 4, 8):
            s.push(ffs[0][t:t + 4], fes[0][t:t + 4])
            push(g, key, ALL)
        out_s = s.finish()
    outs = finish_all(g)
    assert torch.equal(out_s, solo_stream) and all(torch.equal(outs[k], solo_group[k]) for k in outs)
    check("slot 0 of the group vs the plain stream", outs[0], solo_stream.float().cpu().numpy(), 2 * gi.TOL)


# =============================================================================================================================
# plans, allocation, refusals of the device entry
# =============================================================================================================================
def test_one_plan_serves_equal_tuples_and_push_allocates_nothing():
    key = gi.G12
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
    assert len(plans) == 1 and next(iter(plans.values())).hits == 3, "one plan serves equal tuples at different t0"
    with torch.no_grad():
        g.reset(2)
    push(g, key, ((2, 8),))
    assert len(plans) == 2


def test_refusals_on_the_device_entry_launch_nothing():
    key = gi.G12
    m = module(key)
    g = open_group(key)
    push(g, key, ALL)
    torch.cuda.synchronize()
    a = next(p for p in m.__dict__[STORE].values() if tuple(p.args.tc[:3]) == (4, 4, 4)).args
    call = lambda: nv.lib().hicom_compressor_stream_group_push(ctypes.byref(a))
    g.out.fill_(7.0)
    state = g.state_ml.clone(), g.state_acc.clone()
    for i in range(3):
        a.slot[i], a.t0[i], a.row0[i] = i, 4, 4
    for field, i, value, needle in (("slot", 1, 0, "appears twice"), ("slot", 2, 3, "0 <= slot < B"), ("slot", 0, -1, "0 <= slot < B"),
                                    ("t0", 1, a.y_index0 // 4 * 4, "outside the positional tables"), ("t0", 2, 2, "whole window groups"),
                                    ("row0", 0, g.out.shape[1] - 3, "outside the slot's buffer"), ("row0", 1, -4, "outside the slot's buffer")):
        old = getattr(a, field)[i]
        getattr(a, field)[i] = value
        status = call()
        msg = nv.lib().hicom_last_error().decode()
        getattr(a, field)[i] = old
        assert status == -1 and msg.startswith("compressor_stream_group: ") and needle in msg, (field, value, status, msg)
    torch.cuda.synchronize()
    assert bool((g.out == 7.0).all()), "a refused push wrote the output"
    assert torch.equal(g.state_ml, state[0]) and torch.equal(g.state_acc, state[1]), "a refused push wrote a state"
    with torch.no_grad():
        with pytest.raises(ValueError, match="at most once per push"):
            g.push(torch.cat([device_clips(key)[0][0][4:8]] * 2), None, [4, 4], [1, 1])
        with pytest.raises(ValueError, match="nothing has been pushed"):
            open_group(key).finish(0)
    assert g.frames == [4, 4, 4]


# the table region hicom_compressor_stream_group_prepare wrote for the host tests' push_block (three items of 4 / 8 / 4 frames, chunks = 2)
# at commit 740012d on an MI355X, 256 ints: GroupItem x 3 | {item, first tile, last tile, partial slot} x 6 | window -> item | row -> item
TABLE_REGION = ([0, 144, 4, 0, 0, 2, 0, 0, 4, 0, 0, 0, 144, 288, 8, 4, 2, 2, 144, 4, 8, 0, 0, 0, 432, 144, 4, 12, 4, 2, 432, 12, 4] + [0] * 31
                + [0, 0, 4, 0, 0, 4, 9, 1, 1, 0, 9, 2, 1, 9, 18, 3, 2, 0, 4, 4, 2, 4, 9, 5] + [0] * 40
                + [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2] + [0] * 48
                + [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2] + [0] * 48)


def test_prepare_writes_the_parents_table_region():
    assert len(TABLE_REGION) == 256
    check_table_region(group_push_block(), nv.compressor_stream_group_workspace, nv.compressor_stream_group_prepare, TABLE_REGION)
