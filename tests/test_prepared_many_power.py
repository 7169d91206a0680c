"""The power of the cases of tests/prepared_many_inputs.py (CPU, the oracle alone): for every entry, for every (clip, guide) pair and for
both softmax-fed output regions (the local token rows, the 32 global rows), each wrong-softmax oracle of tests/softmax_mutants.py must
move each region it can touch by at least POWER = 4 bars of the GPU test (tests/test_gpu_prepared_many.py), the threshold of
tests/test_many_item_power.py: a condition, not a measurement.  A family that cannot meet it on a case is not used on that case; the
factor is never lowered.  Nothing here runs the code under test.

Worst figure per case (moved / bar), recorded from this test's output: 9.52 (pm_mix6_outlier), 16.8 (the MIX6 `edge` cases; 19.1 without
frames_embed), 43.9 (pm_mix9_chunks3)."""
import numpy as np
import pytest
import torch

import many_item_inputs as mi
import prepared_many_inputs as pmi
import softmax_mutants as sm
from oracle import hicom_oracle as orc

POWER = 4.0


def moved(c, item, q, want):
    """{mutant: {region: max-abs the oracle's output of this pair moves}} over the regions the mutant can touch."""
    n_tokens = int(np.prod(c.ff[item].shape[:-1]))
    reg = pmi.regions(c, item, want.shape[0])
    out = {}
    for name in sm.MUTANTS:
        touched = sm.regions(name, n_tokens)
        if not touched:
            continue
        with sm.wrong_softmax(name):
            got = pmi.run_oracle(c, item, q)
        assert orc.softmax_mha is torch.softmax and orc.softmax_local is torch.softmax
        d = np.abs(got.astype(np.float64) - want)
        out[name] = {r: float(d[reg[r]].max()) for r in touched}
    return out


@pytest.mark.parametrize("id", [e.id for e in pmi.CASES])
def test_every_wrong_softmax_moves_every_region_of_every_pair_by_four_bars(id):
    c = pmi.build(id)
    wants = pmi.oracle_outputs(id)
    short, worst = [], float("inf")
    for (item, q), want in wants.items():
        tol = mi.tolerance(c.entry, want)
        gaps = moved(c, item, q, want)
        assert set(gaps) == set(sm.MUTANTS)                     # (every clip has more than 16 tokens: drop_tile_edge applies)
        worst = min([worst] + [v / tol for g in gaps.values() for v in g.values()])
        short += [f"pair ({item}, {q}) {n} {r}: {v:.3e} < {POWER:g} x {tol:.3e}" for n, g in gaps.items() for r, v in g.items() if not v >= POWER * tol]
    print(f"{id}: worst moved / bar over {len(wants)} pairs: {worst:.2f}")
    assert not short, f"{id}: the family lacks power: " + "; ".join(short)


def test_the_table_covers_what_the_gpu_test_needs():
    by = {e.id: e for e in pmi.CASES}
    assert {e.recipe for e in pmi.CASES} == {mi.ADAPTKV, mi.ADAPTK, mi.ADAPTV, mi.PLAIN}
    assert all(e.hidden == 896 for e in pmi.CASES) and all(e.shift_l == 8.0 for e in pmi.CASES if e.recipe in (mi.ADAPTKV, mi.ADAPTK)
                                                            and e.family == "edge")
    assert any(not e.with_fe for e in pmi.CASES) and by["pm_mix9_chunks3"].chunks == 3 and by["pm_mix6_outlier"].family == "edge_outlier"
    assert pmi.build("pm_mix6_newline_grid").newline is not None
    frames, modals, h, w, counts = pmi.MIX6
    assert sorted(q % 4 for q in counts) == [0, 1, 1, 2, 3] and max(counts) * 9 > 32 and 1 in [t for t, m in zip(frames, modals) if m == "video"]
    assert pmi.MIX9[4] == (4, 8) and (pmi.MIX9[2] * pmi.MIX9[3]) % 16 != 0
