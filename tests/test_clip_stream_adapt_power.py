"""The float64 reference of the multi-guide clip stream on the k / v adaptor recipe and the power of its input family (CPU, the oracle
alone; tests/clip_stream_adapt_inputs.py).

1. chunked_ref_adapt -- per chunk the adaptor MLPs over the chunk's tokens, the blend, every guide's local rows at their packed offset in
   the guide's plane, one un-normalised set per guide and head folded into the carried state, the finish chain per guide -- is
   oracle.projector_forward per guide on the concatenated clip, whatever the chunking, for the three adaptor sets.  Bars as
   tests/test_clip_stream_multi_power.py: 2e-7 on the global rows (the float64 oracle takes its global softmax in fp32); 1e-11 on the local
   rows (a LayerNorm of an MLP in front of the window softmax: ten times the plain recipe's 1e-12).
2. POWER = 4 is a condition, not a measurement: every mutant of chunked_ref_adapt -- the eight of a chunked multi-guide stream, the y planes
   of the previous push read, the two planes swapped, the blend skipped from the second push on, the k adaptor fed frames_feature -- moves
   every (guide, region) it can touch (clip_stream_adapt_inputs.touches) by at least 4 x the bar the GPU test applies there (1e-3 per guide
   and region), for every adaptkv case and chunking the GPU test runs.  What a mutant cannot touch does not move at all.  Nothing here runs
   the code under test."""
import numpy as np
import pytest
import torch

import clip_stream_adapt_inputs as ca
import clip_stream_multi_inputs as cm
from hicom_amd import synth

POWER = 4.0
TOL = ca.mi.TOL
REF_CASES = [(k, r, Q, fe, ch) for k, r, Q, fe, chs in ca.CASES for ch in chs]
POWER_CASES = [c for c in REF_CASES if c[1] == ca.ADAPTKV]


def case_id(c):
    k, r, Q, fe, ch = c
    return f"T{k[0]}_{k[1]}x{k[2]}_h{k[3]}_{k[4] or 'plain'}-{r.split('_')[1]}-Q{Q}-{'fe' if fe else 'no_fe'}-" + "+".join(map(str, ch))


def assert_is_oracle(got, want, what):
    assert got.shape == want.shape
    errs = ca.region_errors(got, want)
    loc, glob = max(v for (q, r), v in errs.items() if r == "local"), max(v for (q, r), v in errs.items() if r == "global")
    print(f"{what}: chunked_ref_adapt against the float64 oracle: local {loc:.2e} global {glob:.2e}")
    assert loc <= 1e-11 and glob <= 2e-7


@pytest.mark.parametrize("case", REF_CASES, ids=case_id)
def test_chunked_reference_is_the_oracle_per_guide_on_the_concatenation(case):
    key, recipe, Q, with_fe, chunking = case
    assert_is_oracle(ca.chunked_ref_adapt(key, chunking, Q, recipe, with_fe=with_fe), ca.oracle_guides(key, recipe, Q, with_fe, dtype=torch.float64),
                     case_id(case))


def test_prefix_and_second_guide_set_references():
    """What the state tests of the GPU file compare with: the first 8 frames alone, and the clip under the second set of guides."""
    K, R = ca.T12, ca.ADAPTKV
    assert_is_oracle(ca.chunked_ref_adapt(K, (4, 4), 4), ca.oracle_guides(K, R, 4, frames=8, dtype=torch.float64), "8 frames")
    assert_is_oracle(ca.chunked_ref_adapt(K, (4, 4, 4), 4, second=True), ca.oracle_guides(K, R, 4, second=True, dtype=torch.float64), "second set")
    a, b = ca.oracle_guides(K, R, 4), ca.oracle_guides(K, R, 4, second=True)
    for q in range(4):                                       # the second set is another answer in both regions of every guide
        assert np.abs(a[q] - b[q])[-ca.NG:].max() > 4 * TOL and np.abs(a[q] - b[q])[:-ca.NG].max() > 4 * TOL


@pytest.mark.parametrize("case", POWER_CASES, ids=case_id)
def test_every_mutant_moves_every_guide_and_region_it_can_touch_by_four_bars(case):
    key, recipe, Q, with_fe, chunking = case
    ref = ca.chunked_ref_adapt(key, chunking, Q, recipe, with_fe=with_fe)
    short, line = [], []
    for m in ca.MUTANTS:
        errs = ca.region_errors(ca.chunked_ref_adapt(key, chunking, Q, recipe, mutant=m, with_fe=with_fe), ref)
        hit = ca.touches(m, chunking, Q, with_fe)
        if hit:
            line.append(f"{m} {min(errs[k] for k in hit) / TOL:.1f}")
        short += [f"{m} guide {q} {r}: {errs[q, r]:.3e} < {POWER:g} x {TOL:.0e}" for q, r in sorted(hit) if not errs[q, r] >= POWER * TOL]
        for k, v in errs.items():
            if k not in hit and k not in ca.uncounted(m, chunking, Q):
                assert v == 0.0, f"{m} moves the {k[1]} rows of guide {k[0]} under {chunking}, which `touches` says it cannot"
    print(f"{case_id(case)}: least move / bar: " + "  ".join(line))
    assert not short, "the family lacks power: " + "; ".join(short)
    assert ca.touches("planes_swapped", chunking, Q, with_fe) and ca.touches("guide_swap", chunking, Q, with_fe)


def test_the_family_does_what_it_says():
    for Q in (2, 5, 9):
        g = ca.guides(ca.T12, Q)
        assert g.dtype == np.float32 and np.array_equal(synth.round_to_bf16(g), g)
        s = [ca.guide_scale(q) for q in range(Q)]
        assert all(np.log2(v) == round(np.log2(v)) for v in s), "powers of two: exact in bf16"
        assert all(a != b for a, b in zip(s, s[1:])), "neighbouring guides differ in scale"
    assert np.array_equal(ca.guides(ca.T12, 9)[:5], cm.guides(ca.T12, 5)), "the first five guides are clip_stream_multi_inputs'"
    assert ca.top_guides(5) == {2} and ca.top_guides(9) == {2, 6, 8}
    c = ca.build(ca.T12)
    assert c.ff is ca.ci.build(ca.T12).ff and c.adapt_k and c.adapt_v
    assert {k for k in c.sd if k.endswith("_alpha")} == {"local_compressor.k_alpha", "local_compressor.v_alpha"}
    only_k = ca.build(ca.T12, ca.ADAPTK)
    assert only_k.adapt_k and not only_k.adapt_v and not any(".v_proj." in k and k.startswith("local_compressor") for k in only_k.sd)
    assert ca.tolerance(ca.oracle_guides(ca.T12, ca.ADAPTKV, 4)[0]) == 1e-3
    # one clip for every chunking: the oracle outputs are cached per (case, recipe, Q)
    assert ca.oracle_guides(ca.T12, ca.ADAPTKV, 4) is ca.oracle_guides(ca.T12, ca.ADAPTKV, 4)
    assert ca.touches("prev_planes", (12,), 4) == set() and ca.touches("key_from_ff", (4, 8), 4, with_fe=False) == set()
