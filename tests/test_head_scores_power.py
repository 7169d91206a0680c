"""CPU: the input families of tests/head_scores_inputs.py against planted faults of their own float64 references, at the bounds the GPU
tests use (tests/test_gpu_head_scores.py, tests/test_gpu_multi_guide_logits.py).  A kernel with one of these faults computes the mutant,
so a mutant that stayed inside the bounds would be a fault the GPU tests cannot see.  Every mutant must miss a bound by MARGIN at least
somewhere; the unmutated reference holds every bound on every case, nothing skipped.

Scores kernel: the hidden term dropped, c[q] dropped, U of guide 0 for every guide, the pitch gap read as data.
Local kernel:  uniform weights (logits ignored), guide 0's logits for every guide, the 1 / sqrt(D) scale missing, a window's logits taken
               from its neighbour."""
import pytest
import torch

import head_scores_inputs as hs

MARGIN = 4.0


def worst(got, want, tol):
    err = (got - want).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return float((err / tol).max())


@pytest.mark.parametrize("case", hs.HS_CASES, ids=[c.id for c in hs.HS_CASES])
def test_scores_reference_holds_its_bound_and_every_mutant_misses_it(case):
    want, tol = hs.hs_reference(case), hs.hs_tol(case)
    assert bool((tol > 0).all()) and bool(torch.isfinite(want).all())
    # a precision bound: a few hundredths of the size of the three terms (g . x ~ 34, the hidden term ~ 14 resp. 60, c ~ 17) at the most
    assert float(tol.max()) < (0.15 if case.inter < 2048 else 1.5), float(tol.max())
    assert worst(want.float().double(), want, tol) <= 1.0, "one fp32 rounding of the reference leaves its own bound"
    applied = []
    for name in hs.HS_MUTANTS:
        m = hs.hs_mutant(case, name)
        if m is None:
            continue
        applied.append(name)
        assert worst(m, want, tol) >= MARGIN, f"{case.id}: {name} stays within {worst(m, want, tol):.2f} bounds"
    assert {"no_hidden", "no_c"} <= set(applied)
    assert ("u_of_guide_0" in applied) == (case.Q > 1) and ("pitch_is_kpad" in applied) == (case.inter > 2048)


def test_every_scores_mutant_is_applied_somewhere():
    for name in hs.HS_MUTANTS:
        assert any(hs.hs_mutant(c, name) is not None for c in hs.HS_CASES), name
    assert any(c.sentinel and c.inter > 2048 for c in hs.HS_CASES) and any(c.sentinel and c.inter < 2048 for c in hs.HS_CASES)


@pytest.mark.parametrize("run", hs.LOCAL_RUNS, ids=[r.id for r in hs.LOCAL_RUNS])
def test_local_reference_holds_its_bound_and_every_mutant_misses_it(run):
    b = hs.local_build(run)
    assert b.logits.dtype == torch.float32 and tuple(b.logits.shape) == (b.Q, b.N)
    # the contexts from the fp32 logits the kernel receives are the reference's own, to a small share of the bound
    assert worst(hs.local_reference_from_logits(run), b.want, b.tol) <= 0.25
    for name in hs.LOCAL_MUTANTS:
        m = hs.local_mutant(run, name)
        if m is None:
            assert (name, b.Q == 1 or b.NW == 1) in (("logits_of_guide_0", True), ("next_window", True)), (run.id, name)
            continue
        if run.family == "flat" and name in ("uniform", "no_scale", "next_window"):
            # near-equal logits: every weight is about 1 / WIN whatever the logits are; these faults belong to the `spike` family
            continue
        assert worst(m, b.want, b.tol) >= MARGIN, f"{run.id}: {name} stays within {worst(m, b.want, b.tol):.2f} bounds"


def test_the_flat_family_is_flat_and_the_spike_family_is_not():
    for run in hs.LOCAL_RUNS:
        b = hs.local_build(run)
        p = torch.softmax(b.s, -1)
        if run.family == "flat":
            assert float(p.max()) < 3.0 / b.WIN, run.id
        elif b.WIN > 1 and b.Q * b.NW > 1:
            assert float(p.max(-1).values.min()) > 0.15, run.id
