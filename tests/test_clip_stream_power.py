"""The float64 reference of the clip stream and the power of its input family (CPU, the oracle alone; tests/clip_stream_inputs.py).

1. chunked_ref -- local rows per chunk at their packed offset, the online-softmax carry with absolute frame numbers, the finish chain -- is
   oracle.projector_forward on the concatenated clip, whatever the chunking.  The oracle is run in float64; its global softmax is taken in
   fp32 whatever the dtype (reference projector.py:213), which leaves 1e-8 .. 7e-8 in the global rows: the bar there is 2e-7, on the local
   rows 1e-12.
2. POWER = 4 is a condition, not a measurement (the convention of tests/test_many_item_power.py): every mutant of chunked_ref moves every
   region it can touch (clip_stream_inputs.touches) by at least 4 x the bar the GPU test applies there, for every case and chunking the GPU
   test runs.  A chunking or scale law that cannot meet it is not used; the factor is never lowered.  Nothing here runs the code under test."""
import numpy as np
import pytest
import torch

import clip_stream_inputs as ci
from hicom_amd import synth

POWER = 4.0
CASES = [(key, ch) for key, chs in ci.CHUNKINGS.items() for ch in chs]
IDS = [f"T{k[0]}_{k[1]}x{k[2]}_h{k[3]}_{k[4] or 'plain'}-" + "+".join(map(str, ch)) for k, ch in CASES]


REF_CASES = [(k, ch, True) for k, ch in CASES] + [(ci.T12, ch, False) for ch in ci.CHUNKINGS[ci.T12]]      # without frames_embed: the 12-frame clip


@pytest.mark.parametrize("key,chunking,with_fe", REF_CASES, ids=[i + "-fe" for i in IDS] + [f"T12_no_fe-{'+'.join(map(str, ch))}" for ch in ci.CHUNKINGS[ci.T12]])
def test_chunked_reference_is_the_oracle_on_the_concatenation(key, chunking, with_fe):
    want = ci.oracle_output(key, with_fe, dtype=torch.float64)
    got = ci.chunked_ref(key, chunking, with_fe)
    assert got.shape == want.shape
    errs = ci.region_errors(got, want)
    print(f"{key} {chunking} fe={with_fe}: chunked_ref against the float64 oracle: local {errs['local']:.2e} global {errs['global']:.2e}")
    assert errs["local"] <= 1e-12 and errs["global"] <= 2e-7


def test_prefix_and_second_guide_references():
    """What the state tests of the GPU file compare with: the first 8 frames alone, and the clip under the second guide."""
    for kw in (dict(frames=8), dict(guide2=True)):
        want = ci.oracle_output(ci.T12, dtype=torch.float64, **kw)
        got = ci.chunked_ref(ci.T12, (4, 4) if "frames" in kw else (4, 4, 4), guide2=kw.get("guide2", False))
        errs = ci.region_errors(got, want)
        assert errs["local"] <= 1e-12 and errs["global"] <= 2e-7, (kw, errs)
    assert np.abs(ci.oracle_output(ci.T12, guide2=True) - ci.oracle_output(ci.T12))[-ci.NG:].max() > 4 * ci.TOL


@pytest.mark.parametrize("key,chunking", CASES, ids=IDS)
def test_every_mutant_moves_every_region_it_can_touch_by_four_bars(key, chunking):
    ref = ci.chunked_ref(key, chunking)
    short, line = [], []
    for m in ci.MUTANTS:
        errs = ci.region_errors(ci.chunked_ref(key, chunking, mutant=m), ref)
        regions = ci.touches(m, chunking)
        line.append(f"{m} " + "/".join(f"{r[0]}{errs[r] / ci.TOL:.1f}" for r in regions))
        short += [f"{m} {r}: {errs[r]:.3e} < {POWER:g} x {ci.TOL:.0e}" for r in regions if not errs[r] >= POWER * ci.TOL]
        for r in ("local", "global"):
            if r not in regions:
                assert errs[r] == 0.0, f"{m} moves the {r} rows of {chunking}, which `touches` says it cannot"
    print(f"{key} {chunking}: moved / bar: " + "  ".join(line))
    assert not short, "the family lacks power: " + "; ".join(short)
    if len(chunking) > 1:
        assert all(ci.touches(m, chunking) for m in ci.MUTANTS if m != "no_rescale")


def test_the_family_does_what_it_says():
    c = ci.build(ci.T12)
    for a in (c.ff, c.fe, c.g, c.g2):
        assert a.dtype == np.float32 and np.array_equal(synth.round_to_bf16(a), a)
    # the running maximum rises when the second group arrives and the third group stays below it
    assert ci.GROUP_SCALES[1] > ci.GROUP_SCALES[0] and ci.GROUP_SCALES[1] > ci.GROUP_SCALES[2] and max(ci.GROUP_SCALES) <= 1.0
    assert ci.touches("no_rescale", (4, 4, 4)) == ci.touches("no_rescale", (4, 8)) == ("global",)
    assert ci.touches("no_rescale", (8, 4)) == () and ci.touches("l_last", (12,)) == ()
    # one clip for every chunking: the chunkings of a case share its oracle output
    assert ci.oracle_output(ci.T12) is ci.oracle_output(ci.T12)
