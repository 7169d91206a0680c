"""The power of the cases of tests/prepared_clip_inputs.py (CPU, the oracle alone): for every (case, family, guide) that
tests/test_gpu_prepared_clip.py holds to the oracle, each wrong-softmax oracle of tests/softmax_mutants.py must move each output region it
can touch by at least POWER x the bar the GPU test applies there; and the adaptors must matter -- the oracle's local rows under the
case's recipe differ from the oracle on the same weights under local43_global32 by at least POWER bars, or parity would say nothing
about the blend.

POWER = 4 is the project's condition (tests/test_many_item_power.py), not a measurement.  A family that cannot meet it on a case is not
used on that case; the factor is never lowered.  Nothing here runs the code under test."""
import numpy as np
import pytest
import torch

import many_item_inputs as mi
import prepared_clip_inputs as pci
import softmax_mutants as sm
from oracle import hicom_oracle as orc

POWER = 4.0


@pytest.mark.parametrize("id", [e.id for e in pci.CASES])
def test_every_wrong_softmax_moves_every_region_by_four_bars(id):
    c = pci.build(id)
    wants = pci.oracle_outputs(id)
    short = []
    for q, want in enumerate(wants):
        tol = mi.tolerance(c.entry, want)
        gaps = {}
        for name in sm.MUTANTS:
            regions = sm.regions(name, c.n_tokens)
            if not regions:
                continue
            with sm.wrong_softmax(name):
                errs = mi.region_errors(pci.run_oracle(c, q), want)
            gaps[name] = {r: errs[r] for r in regions}
        assert orc.softmax_mha is torch.softmax and orc.softmax_local is torch.softmax
        print(f"{id} guide {q}: bar {tol:.2e}; moved / bar: "
              + "  ".join(f"{n} " + "/".join(f"{r[0]}{v / tol:.1f}" for r, v in g.items()) for n, g in gaps.items()))
        assert set(gaps) == set(sm.MUTANTS)                                 # (every case has more than 16 tokens: drop_tile_edge applies)
        short += [f"guide {q} {n} {r}: {v:.3e} < {POWER:g} x {tol:.3e}" for n, g in gaps.items() for r, v in g.items() if not v >= POWER * tol]
    assert not short, f"{id}: the family lacks power: " + "; ".join(short)


@pytest.mark.parametrize("id", [e.id for e in pci.CASES])
def test_the_adaptors_move_the_local_rows_by_four_bars(id):
    c = pci.build(id)
    with_ad, without = pci.oracle_outputs(id), pci.oracle_outputs(id, mi.PLAIN)
    gaps = []
    for q, (a, b) in enumerate(zip(with_ad, without)):
        tol = mi.tolerance(c.entry, a)
        gaps.append(float(np.abs(a[:-mi.NG] - b[:-mi.NG]).max()) / tol)
        assert np.array_equal(a[-mi.NG:], b[-mi.NG:]), "the global stage of this recipe is plain"
    print(f"{id}: oracle local rows, {c.entry.recipe} vs {mi.PLAIN} on the same weights, in bars per guide: {['%.1f' % g for g in gaps]}")
    assert min(gaps) >= POWER, gaps


def test_the_table_covers_what_the_gpu_test_needs():
    qs = sorted({e.shape[0] for e in pci.CASES})
    assert qs == [1, 2, 3, 4, 5, 6, 7, 9]                                   # a full group, every remainder, three groups: for groups of 2, 3 and 4
    assert {e.recipe for e in pci.CASES} == {mi.ADAPTKV, mi.ADAPTK, mi.ADAPTV}
    assert {e.shape[1:] for e in pci.CASES} >= {(4, 6, 6, "video"), (8, 6, 6, "video"), (1, 6, 6, "image"), (1, 9, 9, "image")}
    assert any(not e.with_fe for e in pci.CASES) and all(e.hidden == 896 for e in pci.CASES)
    for id in pci.NEWLINE:
        assert pci.build(id).newline is not None
