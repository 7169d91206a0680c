"""The power of the input families on the cases of forward_ragged_multi_guide (CPU, the oracle alone): for every entry of
tests/ragged_multi_guide_inputs.py, for every (item, guide) pair and for both softmax-fed output regions (the local token rows, the 32
global rows), each wrong-softmax oracle of tests/softmax_mutants.py must move each region it can touch by at least POWER = 4 bars of the
GPU test, the threshold tests/test_many_item_power.py uses.  Nothing here runs the code under test.

Worst figure over the table (moved / bar), recorded from this test's output: 4.47 (rmg_mix6_chunks3 and rmg_mix6_chunks18); per case 4.47 ..
26.7."""
import numpy as np
import pytest
import torch

import ragged_multi_guide_inputs as ri
import many_item_inputs as mi
import softmax_mutants as sm
from oracle import hicom_oracle as orc

POWER = 4.0


def moved(c, item, q, want):
    """{mutant: {region: max-abs the oracle's output of this pair moves}} over the regions the mutant can touch."""
    n_tokens = int(np.prod(c.ff[item].shape[:-1]))
    reg = ri.regions(c, item, want.shape[0])
    out = {}
    for name in sm.MUTANTS:
        touched = sm.regions(name, n_tokens)
        if not touched:
            continue
        with sm.wrong_softmax(name):
            got = ri.run_oracle(c, item, q)
        assert orc.softmax_mha is torch.softmax and orc.softmax_local is torch.softmax
        d = np.abs(got.astype(np.float64) - want)
        out[name] = {r: float(d[reg[r]].max()) for r in touched}
    return out


@pytest.mark.parametrize("id", [e.id for e in ri.CASES])
def test_every_wrong_softmax_moves_every_region_of_every_pair_by_four_bars(id):
    c = ri.build(id)
    wants = ri.oracle_outputs(id)
    short, worst = [], float("inf")
    for (item, q), want in wants.items():
        tol = mi.tolerance(c.entry, want)
        gaps = moved(c, item, q, want)
        assert set(gaps) >= set(sm.MUTANTS) - {"drop_tile_edge"}
        worst = min([worst] + [v / tol for g in gaps.values() for v in g.values()])
        short += [f"pair ({item}, {q}) {n} {r}: {v:.3e} < {POWER:g} x {tol:.3e}" for n, g in gaps.items() for r, v in g.items() if not v >= POWER * tol]
    print(f"{id}: worst moved / bar over {len(wants)} pairs: {worst:.2f}")
    assert not short, f"{id}: the family lacks power: " + "; ".join(short)
