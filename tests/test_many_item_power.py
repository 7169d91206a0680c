"""The power of the input families of tests/many_item_inputs.py (CPU, the oracle alone): for every entry of its table of cases -- every
(step, case, family) a GPU test holds to the oracle -- for every item or guide and for both output regions (the local rows, the 32
global rows), each wrong-softmax oracle of tests/softmax_mutants.py must move each region it can touch by at least POWER x the
tolerance the GPU test applies to that region.

POWER = 4 is a condition, not a measurement: a kernel wrong in one of these ways then misses the bar even where its own rounding error
or a partial cancellation takes a tolerance or two off the gap.  A family that cannot meet it on a case is not used on that case; the
factor is never lowered.  Nothing here runs the code under test, so the claim "a wrong softmax cannot pass" never rests on it."""
import numpy as np
import pytest
import torch

import many_item_inputs as mi
import softmax_mutants as sm
from hicom_amd import synth
from oracle import hicom_oracle as orc
from oracle_util import to_t

POWER = 4.0


def moved(c, item, want):
    """{mutant: {region: max-abs the oracle's output of this item moves}} over the regions the mutant can touch."""
    n_tokens = int(np.prod(c.items[item][0].shape[:-1]))
    out = {}
    for name in sm.MUTANTS:
        regions = sm.regions(name, n_tokens)
        if not regions:
            continue
        with sm.wrong_softmax(name):
            got = mi.run_oracle(c, item)
        assert orc.softmax_mha is torch.softmax and orc.softmax_local is torch.softmax
        errs = mi.region_errors(got, want)
        out[name] = {r: errs[r] for r in regions}
    return out


@pytest.mark.parametrize("id", [e.id for e in mi.CASES])
def test_every_wrong_softmax_moves_every_region_by_four_tolerances(id):
    c = mi.build(id)
    wants = mi.oracle_outputs(id)
    short = []
    for item, want in enumerate(wants):
        tol = mi.tolerance(c.entry, want)
        gaps = moved(c, item, want)
        print(f"{id} item {item}: bar {tol:.2e}, max|out| local {np.abs(want[:-mi.NG]).max():.3f} global {np.abs(want[-mi.NG:]).max():.3f}; moved / bar: "
              + "  ".join(f"{n} " + "/".join(f"{r[0]}{v / tol:.1f}" for r, v in g.items()) for n, g in gaps.items()))
        assert set(gaps) >= set(sm.MUTANTS) - {"drop_tile_edge"}
        assert sm.GLOBAL in gaps["pos_off"] and all(len(g) == 2 for n, g in gaps.items() if n not in ("pos_off", "drop_tile_edge"))
        short += [f"item {item} {n} {r}: {v:.3e} < {POWER:g} x {tol:.3e}" for n, g in gaps.items() for r, v in g.items() if not v >= POWER * tol]
    assert not short, f"{id}: the family lacks power: " + "; ".join(short)


def test_flat_law_figures_for_the_record():
    """What the flat law hides, printed and not asserted: the suite's batch weights, item 0, a 6x6 grid, hidden 64, T = 4 and T = 8."""
    cfg, sd = mi._weights("batch", None, 64)
    tsd = {k: to_t(v) for k, v in sd.items()}
    for T in (4, 8):
        x = synth.synth_inputs(T, 6, 6, mi.D, tag="batch:item0")
        run = lambda: orc.projector_forward(cfg, tsd, to_t(x["ff"]), to_t(x["fe"]), to_t(x["g"]), "video", None).numpy()
        want = run()
        for name in sm.MUTANTS:
            with sm.wrong_softmax(name):
                errs = mi.region_errors(run(), want)
            print(f"flat law T={T} 6x6, {name}: local rows move {errs['local']:.3e}, global rows {errs['global']:.3e}  (bar {mi.TOL:.0e})")


def test_the_context_manager_restores_the_oracle_when_the_block_raises():
    saved = orc.softmax_mha, orc.softmax_local, orc.global_forward
    for name in sm.MUTANTS:
        with pytest.raises(KeyError):
            with sm.wrong_softmax(name):
                raise KeyError(name)
        assert (orc.softmax_mha, orc.softmax_local, orc.global_forward) == saved
    assert saved[0] is torch.softmax and saved[1] is torch.softmax


def test_families_keep_bf16_values_and_spike_the_documented_tokens():
    assert mi.edge_tokens(81) == [0, 15, 16, 80]
    assert mi.edge_tokens(36) == [0, 15, 16, 35]
    assert mi.edge_tokens(288, chunks=3) == [0, 15, 16, 95, 96, 191, 192, 287]
    assert mi.edge_tokens(288, chunks=18) == sorted({0, 287} | {16 * t - 1 for t in range(1, 18)} | {16 * t for t in range(1, 18)})
    assert mi.edge_tokens(36, chunks=18) == [0, 15, 16, 31, 32, 35]                # clamped to the item's 3 tiles
    for id in ("batch_image_81", "batch_image_81_outlier", "batch_image_81_scales", "mg_video3_no_fe"):
        c = mi.build(id)
        for ff, fe, g, _ in c.items:
            for a in (ff, fe, g):
                assert a is None or (a.dtype == np.float32 and np.array_equal(synth.round_to_bf16(a), a))
    # the global spike does what it says: the mean per-head logit shift of the guide's own query
    c = mi.build("batch_image_81")
    _, per = mi.global_spike(c.sd, c.g[0], 5.0)
    assert abs(per.mean() - 5.0) < 1e-9 and per.min() > 0
