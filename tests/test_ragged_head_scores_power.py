"""CPU: the mixes of tests/ragged_head_scores_inputs.py against planted faults of their own float64 reference, at the bound the GPU test
uses (tests/test_gpu_ragged_head_scores.py).  A segmented scores kernel with one wrong index computes the mutant, so a mutant that stayed
inside the bound would be a fault the GPU test cannot see.  Every fault must leave the per-item bound by MARGIN at least on EVERY mix where
it is defined -- by a wrong value in a cell of an item's guides, by a cell of an item's guides left at the pre-fill, or by a written cell
with q >= Q_i -- and the unmutated reference holds the bound on every mix.

Faults: the guide rows of the previous item (pair0 of item i - 1); a tile that runs on into the next item's tokens; item 0's Q for every
item; c indexed by the guide's number inside its item instead of by its pair."""
import pytest
import torch

import head_scores_inputs as hs
import ragged_head_scores_inputs as rh

MARGIN = 4.0
IDS = [m.id for m in rh.MIXES]


@pytest.mark.parametrize("mix", rh.MIXES, ids=IDS)
def test_reference_holds_its_bound_and_every_defined_fault_leaves_it(mix):
    want = rh.reference(mix)
    assert tuple(want.shape) == (max(mix.Q), sum(mix.N))
    for i in range(len(mix.N)):
        tol = rh.item_tol(mix, i)
        assert bool((tol > 0).all()) and tuple(tol.shape) == (mix.Q[i], mix.N[i])
        # a precision bound: a few hundredths of the size of the three terms at the most (the figures of test_head_scores_power.py)
        assert float(tol.max()) < (0.15 if mix.inter < 2048 else 1.5), float(tol.max())
    assert rh.worst(mix, want) == 0.0
    assert rh.worst(mix, want.float()) <= 1.0, "one fp32 rounding of the reference leaves its own bound"
    B = len(mix.N)
    crosses = any(sum(mix.N[:i + 1]) % rh.TILE for i in range(B - 1))
    defined = {"pair0_of_previous_item": B > 1, "tile_runs_into_next_item": crosses, "q_of_item_0": len(set(mix.Q)) > 1, "c_by_guide_number": B > 1}
    for name in rh.MUTANTS:
        m = rh.mutant(mix, name)
        assert (m is not None) == defined[name], (mix.id, name)
        if m is not None:
            assert rh.worst(mix, m) >= MARGIN, f"{mix.id}: {name} stays within {rh.worst(mix, m):.2f} bounds"


def test_every_fault_is_defined_on_a_mix_of_each_plane_and_the_required_mixes_are_there():
    for name in rh.MUTANTS:
        assert any(rh.mutant(m, name) is not None for m in rh.MIXES if m.inter < 2048), name
        assert any(rh.mutant(m, name) is not None for m in rh.MIXES if m.inter > 2048), name
    by = rh.BY_ID
    assert (by["n4"].N, by["n4"].Q, by["n4"].inter) == ((5, 36, 53, 729), (1, 3, 17, 2), 200)
    assert (by["mix6"].N, by["mix6"].Q, by["mix6"].inter) == ((36, 144, 36, 288, 36), (1, 3, 5, 2, 4), 200)
    assert (by["q32"].N, by["q32"].Q, by["q32"].inter) == ((9, 9), (32, 1), 200)
    assert (by["pitched"].N, by["pitched"].Q, by["pitched"].inter) == ((144,), (3,), 4304)
    b = rh.build(by["pitched"])
    assert b.ld > b.kpad > by["pitched"].inter, "the pitched plane has pad columns and a pitch gap"


def test_a_write_behind_an_items_guides_is_seen():
    """The cells q >= Q_i are part of the check: the reference with one of them written fails."""
    mix = rh.BY_ID["n4"]
    got = rh.reference(mix).clone()
    got[mix.Q[0], 0] = 0.0
    assert rh.worst(mix, got) == float("inf")


@pytest.mark.parametrize("case", [c for c in hs.HS_CASES if c.M <= 144 and not c.sentinel], ids=lambda c: c.id)
def test_the_item_bound_is_the_hs_tol_formula(case):
    """rh.tol_of on the operands of a case of tests/head_scores_inputs.py is that file's hs_tol, element for element."""
    assert torch.equal(rh.tol_of(hs.hs_build(case)), hs.hs_tol(case))


def test_the_sentinel_fills_pad_columns_and_pitch_gap_and_the_clean_plane_is_zero_there():
    for mix in rh.MIXES:
        b = rh.build(mix)
        assert bool((b.hid[:, mix.inter:] == hs.SENTINEL).all()) and not bool(b.clean[:, mix.inter:].any())
        assert torch.equal(b.hid[:, :mix.inter], b.clean[:, :mix.inter]) and b.hid.shape[1] == b.ld
