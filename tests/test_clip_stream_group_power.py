"""The float64 reference of the clip stream group and the power of its schedule (CPU, the oracle alone; tests/clip_stream_group_inputs.py).

1. group_ref -- the schedule replayed with per-slot local rows, per-slot online-softmax carry with absolute frame numbers and the finish
   chain -- is oracle.projector_forward on each slot's concatenation with the slot's guide, within the tolerance
   tests/test_clip_stream_power.py uses for chunked_ref: 1e-12 on the local rows, 2e-7 on the global rows (the oracle's fp32 softmax).
2. POWER = 4 is a condition, not a measurement: every mutant of group_ref moves a region it can touch (clip_stream_group_inputs.touches)
   by at least 4 x the bar the GPU test applies there (TOL = 1e-3), and no entry that `touches` leaves out moves at all.  Which mutants a
   schedule cannot show is stated by `touches` returning nothing for them: the wide schedule has no reset, so it cannot show reset_all.
Nothing here runs the code under test."""
import pytest
import torch

import clip_stream_group_inputs as gi

POWER = 4.0
CASES = {"B3_T12": (gi.G12, gi.SCHEDULE, 3), "B3_T12_grid": (gi.G12_GRID, gi.SCHEDULE, 3), "B2_wide": (gi.WIDE, gi.SCHEDULE_WIDE, 2)}


@pytest.mark.parametrize("name,with_fe", [(n, True) for n in CASES] + [("B3_T12", False)])
def test_group_reference_is_the_oracle_on_each_slots_concatenation(name, with_fe):
    key, schedule, nslots = CASES[name]
    got = gi.group_ref(key, schedule, with_fe, nslots=nslots)
    want = gi.final_state(schedule, nslots)
    assert len(got) == len(want)
    for i, (res, fin) in enumerate(zip(got, want)):
        assert sorted(res) == sorted(fin)
        for s, (frames, guide) in fin.items():
            errs = gi.region_errors(res[s], gi.oracle_output(key, s, frames, guide, with_fe, dtype=torch.float64))
            print(f"{name} fe={with_fe} finish {i} slot {s} ({frames} frames, guide {guide}): local {errs['local']:.2e} global {errs['global']:.2e}")
            assert errs["local"] <= 1e-12 and errs["global"] <= 2e-7


@pytest.mark.parametrize("name", list(CASES))
def test_every_mutant_moves_a_region_it_can_touch_by_four_bars(name):
    key, schedule, nslots = CASES[name]
    ref = gi.group_ref(key, schedule, nslots=nslots)
    short = []
    for m in gi.MUTANTS:
        mut = gi.group_ref(key, schedule, mutant=m, nslots=nslots)
        can = gi.touches(m, schedule, nslots)
        moved = {}
        for i, (a, b) in enumerate(zip(mut, ref)):
            for s in b:
                for r, v in gi.region_errors(a[s], b[s]).items():
                    moved[(i, s, r)] = v = float("inf") if v != v else v           # (NaN: an emptied slot finished)
                    if (i, s, r) not in can:
                        assert v == 0.0, f"{m} moves {(i, s, r)} of {name}, which `touches` says it cannot"
        line = "  ".join(f"f{i}s{s}{r[0]}={moved[(i, s, r)] / gi.TOL:.1f}" for i, s, r in sorted(can))
        print(f"{name} {m}: moved / bar: {line or 'cannot be shown by this schedule'}")
        if can and not max(moved[e] for e in can) >= POWER * gi.TOL:
            short.append(f"{m}: {max(moved[e] for e in can):.3e} < {POWER:g} x {gi.TOL:.0e}")
    assert not short, "the schedule lacks power: " + "; ".join(short)


def test_the_schedule_does_what_the_issue_asks_and_shows_every_mutant():
    pushes = [op[1] for op in gi.SCHEDULE if op[0] == "push"]
    assert sorted(s for s, _ in pushes[0]) == [0, 1, 2] and len({n for _, n in pushes[0]}) > 1            # all slots, unequal chunks
    assert [s for s, _ in pushes[1]] != sorted(s for s, _ in pushes[1]) and len({n for _, n in pushes[1]}) == 2   # a permuted subset, Tc differ
    assert len(pushes[2]) == 1
    fin = gi.final_state(gi.SCHEDULE)
    assert all(f <= 12 for res in fin for f, _ in res.values()) and fin[1][0] == (4, 3) and fin[1][2][0] == 12   # slot 0 at t0 = 0, slot 2 at 8
    for m in gi.MUTANTS:
        assert gi.touches(m, gi.SCHEDULE), m
    # what the wide schedule cannot show: it has no reset, no permuted subset, and its second push has one item
    assert [m for m in gi.MUTANTS if not gi.touches(m, gi.SCHEDULE_WIDE, 2)] == ["t0_shared", "slot_swap", "row0_shared", "reset_all"]
