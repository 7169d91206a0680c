"""The power of the input table of tests/readout_gemm_inputs.py (CPU, the float64 reference alone): for every case and family each
fault below -- planted in the reference or in the expected layout, never in the code under test -- must move at least one element of an
image tests/test_gpu_readout_gemm.py checks for that case.  Exact family: move it at all (the bound is zero; an element that is live in
one image and NaN in the other counts).  Round family: by at least POWER x the bound at that element.

  lo_stage_s         the lo plane of stage s left out: s = 0, s = ns - 1 and one s in every residue class of the ring depth (3 / 5 / 8).
                     Only with a lo plane.
  stale_stage_s      stage s contributes what stage s - 1 does (a slot read before its data landed), the same s >= 1
  last_missing / last_twice   the last stage left out / counted twice
  half_lost          the 16-column block that holds column N - 1 loses the second 32-wide k half of the last stage (the planes kernels'
                     wave-partner exchange).  planes only.
  tail_rows          the rows of the last, partly filled row tile take row M - 1.  Only where that tile holds two rows or more.
  tail_cols          the columns of the last, partly filled column tile take weight row N - 1.  Likewise.
  bias_shift4        the bias read one 4-column group further (clamped to N - 1).  With a bias and N >= 2.
  bias_tail_group    the last, partial 4-column group takes b[N - 1].  With a bias and N % 4 >= 2.
  gelu_before_bias   GELU(acc) + b.  Round family of the GELU cases with a bias.
  gap_late           the gap placed one row late: (m + 1) // nl_group.  With nl_group <= M.
  row0_dropped       only where row0 > 0
  y32_is_bf16        the f32 rows carry the bf16-rounded value
  pitch_is_N         the rows stored with pitch N.  Only where ldy > N.

POWER = 4 is the project's margin (tests/test_many_item_power.py): a condition on the inputs, never lowered.  A fault that cannot reach
it in the round family of a case is witnessed by that case's exact family alone; readout_gemm_inputs.EXACT_ONLY lists those (case,
fault) pairs, and the test below holds the list to exactly the pairs that need it.  They are lo_stage_s at 3 and more stages (the
bound of the round family grows with K, sum_tol over 2 K + 1 terms, while one stage's lo plane moves a value by a few 1e-5 whatever K
is; weakest 0.57 bounds) and y32_is_bf16 in three planes cases (K = 512 .. 704 with a handful of columns; weakest 2.7).  Every such case
runs its exact family, where these faults change bits.  The r16 cases of 16 and 17 stages run the round family alone and hold every fault
that applies to them to POWER.

Weakest figures over all (case, fault) pairs held to POWER in the round family, in bounds (inf: an element appears or disappears):
lo_stage 4.0, stale_stage 3.1e2, last_missing 2.1e2, last_twice 2.7e2, half_lost 80, tail_rows 1.8e3, tail_cols 8.3e2, bias_shift4 1.8e2,
bias_tail_group 38, gelu_before_bias 1.4e2, gap_late inf, row0_dropped inf, y32_is_bf16 4.5, pitch_is_N inf.  In the exact family every
fault moves an element of every case it applies to (any difference counts: the bound is zero).
"""
import pytest
import torch

import readout_gemm_inputs as gi

POWER = 4.0
IDS = [c.id for c in gi.CASES]


def exact_only(c, name):
    return name in gi.EXACT_ONLY.get(c.id, ())


@pytest.mark.parametrize("id", IDS)
def test_every_planted_fault_moves_a_checked_element(id):
    c = gi.BY_ID[id]
    short = []
    for family in gi.families(c):
        good, line = gi.expected(id, family), []
        for name in gi.faults(c, family):
            r = gi.moved(good, gi.expected(id, family, name))
            line.append(f"{name} {r:.3g}")
            if family == "exact":
                if r != float("inf"):
                    short.append(f"exact {name}: not moved")
            elif exact_only(c, name):
                if "exact" not in gi.families(c) or name not in gi.faults(c, "exact"):
                    short.append(f"{name}: restricted to an exact family the case does not run")
                if r >= POWER:
                    short.append(f"{name}: listed in EXACT_ONLY but moves {r:.1f} bounds")
            elif not r >= POWER:
                short.append(f"round {name}: {r:.2f} bounds")
        print(f"READOUT-POWER {id} {family} moved / bound: " + "  ".join(line))
    assert not short, f"{id}: the table lacks power: " + "; ".join(short)


@pytest.mark.parametrize("kernel", ["gemm", "planes", "r16"])
def test_every_fault_applies_to_some_case_of_every_kernel(kernel):
    cases = [c for c in gi.CASES if c.kernel == kernel]
    assert 20 <= len(cases) <= 30
    kinds = {gi.kind_of(n) for c in cases for fam in gi.families(c) for n in gi.faults(c, fam)}
    want = set(gi.FAULT_KINDS) - ({"half_lost"} if kernel != "planes" else set()) - ({"lo_stage"} if kernel == "r16" else set())
    assert kinds == want, (want - kinds, kinds - want)
    # ... and in a round family that is held to POWER
    held = {gi.kind_of(n) for c in cases for n in gi.faults(c, "round") if not exact_only(c, n)}
    assert held == want, want - held


def test_the_tables_reach_the_documented_paths():
    by = lambda k: [c for c in gi.CASES if c.kernel == k]
    g, p, r = by("gemm"), by("planes"), by("r16")
    assert {c.ns for c in g} == set(range(1, 8)) and {c.M for c in g} == {1, 63, 64, 65, 130, 513} and {c.N for c in g} == {1, 63, 64, 65, 118, 130}
    assert {c.bias for c in g} == {"bf16", "f32", None} and {c.ydt for c in g} == {"f32", "bf16"} and {c.ld_extra for c in g} == {0, 8}
    assert {(0, 0), (3, 9), (2, 1)} <= {(c.row0, c.nl_group) for c in g} and any(c.nl_group > c.M for c in g) and {c.act for c in g} == {0, 1}
    assert all((c.N + 63) // 64 == 2 for c in g if c.M == 513)
    for lo in (True, False):
        assert {c.ns for c in p if c.lo == lo} == set(range(1, 12)), lo
    assert {c.M for c in p} == {1, 47, 48, 49, 97, 385} and {c.N for c in p} == {1, 3, 4, 127, 128, 129, 130, 257}
    assert {c.out for c in p} == {"plane", "y", "both"} and {c.bias for c in p} == {"bf16", "f32", None}
    assert any(c.ld_extra == 2 and c.N % 4 == 0 for c in p) and any(c.y_off == 1 for c in p) and any(c.b_off == 1 for c in p)
    assert {c.ns for c in r} == set(range(1, 11)) | {16, 17} and {c.M for c in r} == {1, 95, 96, 97, 193, 769}
    assert {c.N for c in r} == {1, 4, 8, 63, 64, 65, 100, 200} and any(c.ld % 4 for c in r if c.has_y)
    assert {(c.out, c.ydt) for c in r} == {("plane", None), ("y", "bf16"), ("both", "f32")}
    for c in r:                                                        # the host's own tile choice stays at 96 x 64
        assert c.N % 128 != 0 and ((c.M + 95) // 96) * ((c.N + 63) // 64) <= 256
    for c in gi.CASES:
        assert c.K % 64 == 0 and (c.has_y or c.has_plane) and (c.kernel != "gemm" or c.out == "y") and (c.ydt is None) == (not c.has_y)
        assert ("exact" in gi.families(c)) == (c.K <= 704)


@pytest.mark.parametrize("id", IDS)
def test_the_inputs_keep_the_kernel_number_formats_and_are_pairwise_distinguishable(id):
    c = gi.BY_ID[id]
    for family in gi.families(c):
        d = gi.build(id, family)
        if c.kernel == "gemm":
            assert d.x.dtype == torch.float32 and d.x.shape == (c.M, c.K) and d.w.dtype == torch.bfloat16
        elif c.kernel == "planes":
            assert d.hi.dtype == torch.bfloat16 and (d.lo is None) == (not c.lo) and d.w.dtype == torch.bfloat16
        else:
            assert d.a16.dtype == torch.float16 and d.w.dtype == torch.float16
        assert (d.b is None) == (c.bias is None) and (d.b is None or d.b.dtype == gi.DTYPES[c.bias])
        a = sum(d.a_terms)
        assert len(torch.unique(a, dim=0)) == c.M and len(torch.unique(d.w64, dim=0)) == c.N        # no two rows equal
        if family == "round" and gi.nterms(c) == 2:
            assert bool((a.float().bfloat16().double() != a).any())                                     # not bf16-representable
