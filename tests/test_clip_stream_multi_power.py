"""The float64 reference of the multi-guide clip stream and the power of its input family (CPU, the oracle alone;
tests/clip_stream_multi_inputs.py).

1. chunked_ref_multi -- per guide the local rows per chunk at their packed offset in the guide's plane, per chunk one un-normalised set per
   guide and head folded into the carried state, the finish chain per guide -- is oracle.projector_forward per guide on the concatenated
   clip, whatever the chunking.  Bars as tests/test_clip_stream_power.py: the float64 oracle takes its global softmax in fp32, which leaves
   up to 2e-7 in the global rows; 1e-12 on the local rows.
2. POWER = 4 is a condition, not a measurement: every mutant of chunked_ref_multi moves every (guide, region) it can touch
   (clip_stream_multi_inputs.touches) by at least 4 x the bar the GPU test applies there (1e-3 per guide and region), for every case and
   chunking the GPU test runs.  Guide scales that cannot meet it are not used; the factor is never lowered.  What a mutant cannot touch does
   not move at all.  Nothing here runs the code under test."""
import numpy as np
import pytest
import torch

import clip_stream_multi_inputs as cm
from hicom_amd import synth

POWER = 4.0
CASES = [(key, Q, ch) for key, Q, chs in cm.CASES for ch in chs]
IDS = [f"T{k[0]}_{k[1]}x{k[2]}_h{k[3]}_{k[4] or 'plain'}-Q{Q}-" + "+".join(map(str, ch)) for k, Q, ch in CASES]
REF_CASES = [(k, Q, ch, True) for k, Q, ch in CASES] + [(cm.T12, Q, ch, False) for Q in (3, 5) for ch in cm.T12_CHUNKINGS]


def assert_is_oracle(got, want, what):
    assert got.shape == want.shape
    errs = cm.region_errors(got, want)
    loc, glob = max(v for (q, r), v in errs.items() if r == "local"), max(v for (q, r), v in errs.items() if r == "global")
    print(f"{what}: chunked_ref_multi against the float64 oracle: local {loc:.2e} global {glob:.2e}")
    assert loc <= 1e-12 and glob <= 2e-7


@pytest.mark.parametrize("key,Q,chunking,with_fe", REF_CASES,
                         ids=[i + "-fe" for i in IDS] + [f"T12_no_fe-Q{Q}-{'+'.join(map(str, ch))}" for Q in (3, 5) for ch in cm.T12_CHUNKINGS])
def test_chunked_reference_is_the_oracle_per_guide_on_the_concatenation(key, Q, chunking, with_fe):
    assert_is_oracle(cm.chunked_ref_multi(key, chunking, Q, with_fe=with_fe), cm.oracle_guides(key, Q, with_fe, dtype=torch.float64),
                     f"{key} Q={Q} {chunking} fe={with_fe}")


def test_prefix_and_second_guide_set_references():
    """What the state tests of the GPU file compare with: the first 8 frames alone, and the clip under the second set of guides."""
    assert_is_oracle(cm.chunked_ref_multi(cm.T12, (4, 4), 3), cm.oracle_guides(cm.T12, 3, frames=8, dtype=torch.float64), "8 frames")
    assert_is_oracle(cm.chunked_ref_multi(cm.T12, (4, 4, 4), 3, second=True), cm.oracle_guides(cm.T12, 3, second=True, dtype=torch.float64), "second set")
    a, b = cm.oracle_guides(cm.T12, 3), cm.oracle_guides(cm.T12, 3, second=True)
    for q in range(3):                                       # the second set is another answer in both regions of every guide
        assert np.abs(a[q] - b[q])[-cm.NG:].max() > 4 * cm.TOL and np.abs(a[q] - b[q])[:-cm.NG].max() > 4 * cm.TOL


@pytest.mark.parametrize("key,Q,chunking", CASES, ids=IDS)
def test_every_mutant_moves_every_guide_and_region_it_can_touch_by_four_bars(key, Q, chunking):
    ref = cm.chunked_ref_multi(key, chunking, Q)
    short, line = [], []
    for m in cm.MUTANTS:
        errs = cm.region_errors(cm.chunked_ref_multi(key, chunking, Q, mutant=m), ref)
        hit = cm.touches(m, chunking, Q)
        if hit:
            line.append(f"{m} {min(errs[k] for k in hit) / cm.TOL:.1f}")
        short += [f"{m} guide {q} {r}: {errs[q, r]:.3e} < {POWER:g} x {cm.TOL:.0e}" for q, r in sorted(hit) if not errs[q, r] >= POWER * cm.TOL]
        for k, v in errs.items():
            if k not in hit and k not in cm.uncounted(m, chunking, Q):
                assert v == 0.0, f"{m} moves the {k[1]} rows of guide {k[0]} under {chunking}, which `touches` says it cannot"
    print(f"{key} Q={Q} {chunking}: least move / bar: " + "  ".join(line))
    assert not short, "the family lacks power: " + "; ".join(short)
    assert cm.touches("guide_swap", chunking, Q) and cm.touches("plane_zero", chunking, Q)


def test_the_family_does_what_it_says():
    for Q in (2, 3, 5):
        g = cm.guides(cm.T12, Q)
        assert g.dtype == np.float32 and np.array_equal(synth.round_to_bf16(g), g)
        assert all(np.log2(s) == round(np.log2(s)) for s in cm.GUIDE_SCALES[:Q]), "powers of two: exact in bf16"
        assert all(a != b for a, b in zip(cm.GUIDE_SCALES[:Q], cm.GUIDE_SCALES[1:Q])), "neighbouring guides differ in scale"
    assert cm.top_guide(3) == cm.top_guide(5) == 2 and cm.GUIDE_SCALES.count(max(cm.GUIDE_SCALES)) == 1
    # one clip for every chunking and every Q: the oracle outputs are cached per (case, Q)
    assert cm.oracle_guides(cm.T12, 3) is cm.oracle_guides(cm.T12, 3)
    assert cm.touches("shared_max", (12,), 3) == set() and (2, "global") not in cm.touches("shared_max", (4, 8), 3)
