"""The float64 reference of the clip stream group on the k / v adaptor recipe and the power of its schedule (CPU, the oracle alone;
tests/clip_stream_group_adapt_inputs.py).

1. adapt_ref -- the schedule replayed in the device's row space with the adaptor MLPs over each push's stacked tokens -- is
   oracle.projector_forward on each slot's concatenation with each of the slot's guides: 1e-10 on the local rows (LayerNorm of the MLP's
   output in float64 on both sides), 2e-7 on the global rows (the oracle's fp32 softmax), as tests/test_clip_stream_group_multi_power.py.
2. POWER = 4 is a condition, not a measurement.  Every fault of a stacked adaptor stage moves the local rows of EVERY pair of every
   (finish, slot) it can touch (clip_stream_group_adapt_inputs.touches) by at least 4 x the bar the GPU test applies there (TOL = 1e-3), and
   moves nothing else.  Each of the nine faults of the many-pair schedule moves some region of some finish by at least 4
   bars, the condition tests/test_clip_stream_group_multi_power.py holds them to under the plain weights.  If a fault moved less, the
   inputs would have to change (GUIDE_SCALE), not the bar.
Nothing here runs the code under test."""
import functools

import pytest
import torch

import clip_stream_group_adapt_inputs as gi
import clip_stream_group_multi_inputs as gm

POWER = 4.0
CASES = {"B3_T12": (gi.G12, gi.SCHEDULE, gi.COUNTS, gi.ADAPTKV), "B3_T12_grid": (gi.G12_GRID, gi.SCHEDULE, gi.COUNTS, gi.ADAPTKV),
         "B3_T12_one_token": (gi.G12_ONE, gi.SCHEDULE, gi.COUNTS, gi.ADAPTKV), "B3_T12_k_only": (gi.G12, gi.SCHEDULE, gi.COUNTS, gi.ADAPTK),
         "B3_T12_v_only": (gi.G12, gi.SCHEDULE, gi.COUNTS, gi.ADAPTV), "B2_wide": (gi.WIDE, gi.SCHEDULE_WIDE, gi.COUNTS_WIDE, gi.ADAPTKV)}


@pytest.mark.parametrize("name,with_fe", [(n, True) for n in CASES] + [("B3_T12", False)])
def test_reference_is_the_oracle_on_each_slots_concatenation_with_each_guide(name, with_fe):
    key, schedule, counts, recipe = CASES[name]
    got = gi.adapt_ref(key, schedule, counts, recipe, with_fe)
    want = gi.final_state(schedule, counts)
    assert len(got) == len(want)
    for i, (res, fin) in enumerate(zip(got, want)):
        assert sorted(res) == sorted(fin)
        for s, (frames, guide0) in fin.items():
            assert res[s].shape[0] == counts[s]
            for q in range(counts[s]):
                errs = gi.pair_errors(res[s][q:q + 1], gi.oracle_output(key, recipe, s, frames, guide0 + q, with_fe, dtype=torch.float64)[None])[0]
                print(f"{name} fe={with_fe} finish {i} slot {s} guide {q} ({frames} frames): local {errs['local']:.2e} global {errs['global']:.2e}")
                assert errs["local"] <= 1e-10 and errs["global"] <= 2e-7


@functools.lru_cache(maxsize=None)
def reference():
    return gi.adapt_ref(gi.G12, gi.SCHEDULE, gi.COUNTS)


def movement(mutant):
    """{(finish, slot, pair of the slot, region): |mutant - reference|} over the schedule."""
    moved = {}
    for i, (a, b) in enumerate(zip(gi.adapt_ref(gi.G12, gi.SCHEDULE, gi.COUNTS, mutant=mutant), reference())):
        for s in b:
            for q, errs in enumerate(gi.pair_errors(a[s], b[s])):
                for r, v in errs.items():
                    moved[(i, s, q, r)] = v
    return moved


@pytest.mark.parametrize("mutant", gi.ADAPT_MUTANTS)
def test_a_stacked_adaptor_fault_moves_every_pair_it_can_touch_by_four_bars(mutant):
    moved = movement(mutant)
    can = gi.touches(mutant, gi.SCHEDULE, gi.COUNTS)
    assert can, "the schedule never reaches the fault"
    short, stray = [], []
    for (i, s, q, r), v in sorted(moved.items()):
        if r == "local" and (i, s) in can:
            print(f"{mutant}: finish {i} slot {s} guide {q} local moved {v / gi.TOL:.1f} bars")
            if not v >= POWER * gi.TOL:
                short.append(f"finish {i} slot {s} guide {q}: {v:.3e}")
        elif v != 0.0:
            stray.append(f"finish {i} slot {s} guide {q} {r}: {v:.3e}")
    assert not short, f"{mutant}: the schedule lacks power (< {POWER:g} x {gi.TOL:.0e}): " + "; ".join(short)
    assert not stray, f"{mutant} moved what it cannot touch: " + "; ".join(stray)


@pytest.mark.parametrize("mutant", gm.MUTANTS)
def test_every_fault_of_the_many_pair_schedule_moves_a_region_by_four_bars(mutant):
    moved = movement(mutant)
    top = max(moved, key=moved.get)
    print(f"{mutant}: largest movement {moved[top] / gi.TOL:.1f} bars at (finish, slot, guide, region) = {top}")
    assert moved[top] >= POWER * gi.TOL, f"{mutant}: {moved[top]:.3e} < {POWER:g} x {gi.TOL:.0e}"


def test_the_schedule_does_what_the_issue_asks():
    pushes = [op[1] for op in gi.SCHEDULE if op[0] == "push"]
    assert sorted(s for s, _ in pushes[0]) == [0, 1, 2] and len({n for _, n in pushes[0]}) > 1            # all slots, unequal chunks
    assert [s for s, _ in pushes[1]] != sorted(s for s, _ in pushes[1]) and len({n for _, n in pushes[1]}) == 2   # a permuted subset, t0 8 and 4
    assert len(pushes[2]) == 1
    fins = [op for op in gi.SCHEDULE if op[0] == "finish"]
    assert fins[0][1] == (0, 2) and fins[1][1] is None, "finish_many on a subset, then on every slot"
    assert ("reset", 1, gi.M) in gi.SCHEDULE and gi.COUNTS == (1, 2, 5) and gi.PAIR0 == (0, 1, 3) and gi.M == 8
    fin = gi.final_state(gi.SCHEDULE, gi.COUNTS)
    assert all(f <= 12 for res in fin for f, _ in res.values())
    assert fin[2][1] == (4, gi.M) and fin[2][2][0] == 12, "slot 1 at t0 = 0 beside slot 2 at t0 = 8 in the last push"
    # a full guide group of the adaptor window kernel plus a remainder of 1; 45 folded rows: a second pass of the stream
    assert gi.COUNTS[2] == 4 + 1 and 32 < gi.NH * gi.COUNTS[2] <= 64 and gi.NH * gi.COUNTS[1] > 16
    assert {n for p in pushes for _, n in p} == {4, 8}
