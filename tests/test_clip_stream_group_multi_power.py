"""The float64 reference of the clip stream group with several guides per slot and the power of its schedule (CPU, the oracle alone;
tests/clip_stream_group_multi_inputs.py).

1. multi_ref -- the schedule replayed in the device's row space (folded rows nh q + h per item, per-pair carry in E-space with absolute frame
   numbers, the finish chain per pair) -- is oracle.projector_forward on each slot's concatenation with each of the slot's guides, within
   the tolerance tests/test_clip_stream_group_power.py uses: 1e-12 on the local rows, 2e-7 on the global rows (the oracle's fp32 softmax).
2. POWER = 4 is a condition, not a measurement: every mutant of multi_ref moves some region of some finish by at least 4 x the bar the GPU
   test applies there (TOL = 1e-3).  If a fault moved less, the schedule's inputs would have to change, not the bar.
Nothing here runs the code under test."""
import pytest
import torch

import clip_stream_group_multi_inputs as mi

POWER = 4.0
CASES = {"B3_T12": (mi.G12, mi.SCHEDULE, mi.COUNTS), "B3_T12_grid": (mi.G12_GRID, mi.SCHEDULE, mi.COUNTS), "B3_T12_one_token": (mi.G12_ONE, mi.SCHEDULE, mi.COUNTS),
         "B2_wide": (mi.WIDE, mi.SCHEDULE_WIDE, mi.COUNTS_WIDE)}


@pytest.mark.parametrize("name,with_fe", [(n, True) for n in CASES] + [("B3_T12", False)])
def test_reference_is_the_oracle_on_each_slots_concatenation_with_each_guide(name, with_fe):
    key, schedule, counts = CASES[name]
    got = mi.multi_ref(key, schedule, counts, with_fe)
    want = mi.final_state(schedule, counts)
    assert len(got) == len(want)
    for i, (res, fin) in enumerate(zip(got, want)):
        assert sorted(res) == sorted(fin)
        for s, (frames, guide0) in fin.items():
            assert res[s].shape[0] == counts[s]
            for q in range(counts[s]):
                errs = mi.region_errors(res[s][q:q + 1], mi.oracle_output(key, s, frames, guide0 + q, with_fe, dtype=torch.float64)[None])
                print(f"{name} fe={with_fe} finish {i} slot {s} guide {q} ({frames} frames): local {errs['local']:.2e} global {errs['global']:.2e}")
                assert errs["local"] <= 1e-12 and errs["global"] <= 2e-7


def test_every_mutant_moves_a_region_by_four_bars():
    key, schedule, counts = CASES["B3_T12"]
    ref = mi.multi_ref(key, schedule, counts)
    short = []
    for m in mi.MUTANTS:
        mut = mi.multi_ref(key, schedule, counts, mutant=m)
        moved = {}
        for i, (a, b) in enumerate(zip(mut, ref)):
            for s in b:
                for r, v in mi.region_errors(a[s], b[s]).items():
                    moved[(i, s, r)] = v
        line = "  ".join(f"f{i}s{s}{r[0]}={v / mi.TOL:.1f}" for (i, s, r), v in sorted(moved.items()) if v)
        print(f"{m}: moved / bar: {line}")
        if not max(moved.values()) >= POWER * mi.TOL:
            short.append(f"{m}: {max(moved.values()):.3e} < {POWER:g} x {mi.TOL:.0e}")
    assert not short, "the schedule lacks power: " + "; ".join(short)


def test_the_schedule_does_what_the_issue_asks():
    pushes = [op[1] for op in mi.SCHEDULE if op[0] == "push"]
    assert sorted(s for s, _ in pushes[0]) == [0, 1, 2] and len({n for _, n in pushes[0]}) > 1            # all slots, unequal chunks
    assert [s for s, _ in pushes[1]] != sorted(s for s, _ in pushes[1]) and len({n for _, n in pushes[1]}) == 2   # a permuted subset, t0 8 and 4
    assert len(pushes[2]) == 1
    fins = [op for op in mi.SCHEDULE if op[0] == "finish"]
    assert fins[0][1] == (0, 2) and fins[1][1] is None, "finish_many on a subset, then on every slot"
    assert ("reset", 1, mi.M) in mi.SCHEDULE and mi.COUNTS == (1, 2, 4) and mi.PAIR0 == (0, 1, 3)
    fin = mi.final_state(mi.SCHEDULE)
    assert all(f <= 12 for res in fin for f, _ in res.values())
    assert fin[2][1] == (4, mi.M) and fin[2][2][0] == 12, "slot 1 at t0 = 0 beside slot 2 at t0 = 8 in the last push"
    # rows >= 16 (Q = 2: 18 rows) and a second pass (Q = 4: 36 rows) are in the schedule
    assert mi.NH * mi.COUNTS[1] > 16 and mi.NH * mi.COUNTS[2] > 32
