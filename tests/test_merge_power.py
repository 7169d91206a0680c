"""The power of the input families of tests/merge_inputs.py (CPU, the float64 references alone): for every case and every fault below
that applies to it -- planted in the reference, never in the code under test -- the faulted reference must differ from the true one by
at least POWER x the bound of tests/test_gpu_merge.py at one or more elements of an output that test always checks for the case:
log L and out_acc of the merge (per normalize value the case runs with), ctx of the combine, log L / ctx / o of merge + v_proj.

  lose_last_partial         the partial nparts - 1 left out of L and acc
  lose_partial_batch        partials 0 .. 255 (the prefetched batch) with weight 0 in acc, not in L; nparts >= 225
  frame_max_unscaled        every frame's tokens enter the positional term with e^(s - fmax_t) instead of e^(s - M); T > 1
  lose_frames_from_64       frames >= 64 left out of the positional term; T > 64
  lose_pos_from_128         positional rows >= 128 in the [T | H | W] order left out; T + H + W > 128
  ignore_t0                 the t offset taken as 0; t0 != 0
  swap_yx                   the y marginal applied to the x block and vice versa; H != W
  neighbour_record          row r merged with the weights (and L) of row r + 1
  pad_leak                  the first padded row's result (NaN: the padding is poisoned) added into row R - 1; R < rows_pad
  unnormalised_L            the division by sum l_p without the weights; normalize = 1, more than one partial
  lose_second_column_block  combine: columns >= 256 from the first set alone; E > 256, more than one set
  head_off_by_one           merge + v_proj: the W_v rows of head h + 1; more than one head
  lose_last_slab            merge + v_proj: the last 64 columns out of the dot product

Every fault must apply to at least one case (asserted).  POWER = 4 is the project's margin (tests/test_many_item_power.py): a condition
on the inputs, never lowered.  The weakest figure per fault over all cases, in bounds, as the last test prints them (a non-finite
faulted result counts as moved: the GPU test requires finite results): lose_last_partial 6.2e3, lose_partial_batch 7.4e3,
frame_max_unscaled 4.8e4, lose_frames_from_64 3.4e3, lose_pos_from_128 3.5e3, ignore_t0 5.2e3, swap_yx 1.0e4, neighbour_record 2.2e4,
pad_leak not finite, unnormalised_L 6.7e3, lose_second_column_block 2.9e5, head_off_by_one 1.7e3, lose_last_slab 251."""
import functools
import math

import pytest
import torch

import merge_inputs as mi
import ops_reference as R
from ops_reference import up

POWER = 4.0
FAULTS = mi.MERGE_FAULTS + ("lose_second_column_block",) + mi.VPROJ_FAULTS


def ratio(got, want, tol):
    """Largest |got - want| / tol; inf when the faulted result is not finite (it would fail the GPU test's finiteness check)."""
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - want).abs() / tol).max())


# ---- the figures, computed once per case and shared by the per-case tests and the summary test: (where, fault, moved / bound) ------
@functools.lru_cache(maxsize=None)
def merge_gaps(id):
    c = mi.build(id)
    e = c.entry
    out = []
    for normalize in e.normalize:
        ref = mi.merge_reference(id, normalize)
        b = mi.merge_bounds(c, ref, normalize)
        for name in mi.MERGE_FAULTS:
            if mi.fault_applies(e, name, normalize):
                M2, L2, acc2 = R.merge_ref(**mi.ref_args(c), normalize=bool(normalize), **{name: True})
                assert torch.equal(M2, ref["M"])
                out.append((f"normalize {normalize}", name, max(ratio(torch.log(L2), torch.log(ref["L"]), b["logL"]), ratio(acc2, ref["acc"], b["acc"]))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def combine_gaps(family):
    out = []
    for nsets, rows, E in mi.COMBINE_SHAPES:
        c = mi.build_combine(family, nsets, rows, E)
        ml, acc = up(c.ml), up(c.acc)
        ctx, _ = R.combine_ref(ml, acc)
        tol = mi.combine_bounds(c, ctx)
        w = torch.exp(ml[:, :, 0] - ml[:, :, 0].max(0).values)
        # (equal M: every weight is 1 and the weights cannot be missed; a second set of weight 0 cannot be lost)
        for name, on in (("unnormalised_L", bool((w != 1).any())), ("lose_second_column_block", E > 256 and bool((w[1:] > 1e-30).any()))):
            if on:
                out.append((str((nsets, rows, E)), name, ratio(R.combine_ref(ml, acc, **{name: True})[0], ctx, tol)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def vproj_gaps(E, rows):
    out = []
    for nparts in mi.VPROJ_NPARTS:
        c = mi.build_vproj(E, rows, nparts)
        for f16 in (False, True):
            ref = mi.vproj_reference(E, rows, nparts, f16)
            b = mi.vproj_bounds(c, ref, f16, fixed=True)
            for name, on in (("head_off_by_one", rows > 1), ("lose_last_slab", True)):
                if on:
                    got = R.merge_vproj_ref(up(c.pm), up(c.pl), up(c.p16 if f16 else c.pacc), rows, up(c.wv), normalised=f16, **{name: True})
                    out.append((f"nparts {nparts} f16 {f16}", name, ratio(got[3], ref[3], b["o"])))
    return tuple(out)


def assert_power(what, gaps):
    print(f"{what} moved / bound: " + "  ".join(f"{name} {v:.3g}" for _, name, v in gaps))
    short = [f"{where} {name}: {v:.2f} bounds" for where, name, v in gaps if not v >= POWER]
    assert not short, f"{what}: the family lacks power: " + "; ".join(short)


@pytest.mark.parametrize("id", [e.id for e in mi.CASES])
def test_every_merge_fault_moves_a_checked_output_by_four_bounds(id):
    e = mi.BY_ID[id]
    assert mi.form_of(e) == e.form, (id, mi.form_of(e))
    if e.marg:
        assert mi.marg_form_of(e) == e.marg and mi.build(id).pmarg is not None
    assert_power(f"{id} [{e.form}]", merge_gaps(id))


@pytest.mark.parametrize("family", mi.COMBINE_FAMILIES)
def test_every_combine_fault_moves_the_context_by_four_bounds(family):
    assert_power(f"combine {family}", combine_gaps(family))


@pytest.mark.parametrize("E,rows", mi.VPROJ_SHAPES)
def test_every_vproj_fault_moves_the_projection_by_four_bounds(E, rows):
    assert_power(f"merge_vproj {(E, rows)}", vproj_gaps(E, rows))


def test_every_fault_applies_somewhere_and_the_weakest_figures():
    gaps = [g for e in mi.CASES for g in merge_gaps(e.id)] + [g for f in mi.COMBINE_FAMILIES for g in combine_gaps(f)]
    gaps += [g for E, rows in mi.VPROJ_SHAPES for g in vproj_gaps(E, rows)]
    weakest = {}
    for _, name, v in gaps:
        weakest[name] = min(weakest.get(name, math.inf), v)
    print("weakest per fault: " + "  ".join(f"{k} {v:.3g}" for k, v in weakest.items()))
    assert set(weakest) == set(FAULTS), f"a fault applies to no case: {set(FAULTS) ^ set(weakest)}"
    assert all(v >= POWER for v in weakest.values())


def test_the_restated_predicates_at_their_boundaries():
    assert mi.two_kernel(4, 7, 5, 38) and not mi.two_kernel(4, 7, 5, 39)                       # 38 + 18 = 56 = 4 x 14
    assert not mi.two_kernel(1, 5, 3, 0)                                                        # T = 1: 0 + 1 + 8 + 2 > 10
    assert mi.two_kernel(65, 1, 1, 187) and not mi.two_kernel(65, 1, 1, 188) and not mi.two_kernel(1000, 1, 1, 1)
    assert mi.apply_form(4, 7, 5, 64, 32) == "apply8" and mi.apply_form(4, 7, 5, 63, 32) == "mode2" and mi.apply_form(4, 7, 5, 64, 33) == "mode2"
    assert mi.apply_form(1000, 15, 1, 64, 6) == "apply8" and mi.apply_form(1000, 15, 1, 64, 7) == "mode2"      # record 1024 | 1025 floats
    assert mi.refusal(1, 110, 110, 1, 1152) == "too many partials/frames for one pass" and mi.refusal(1, 100, 100, 1, 1152) is None
    assert mi.refusal(1, 123, 123, 1, 1152) == "too large for the marginal kernel" and mi.refusal(4, 7, 5, 3, 102) == "global_merge: E"
    assert mi.smem2_bytes(1, 106, 106, 1) <= 60000 < mi.smem2_bytes(1, 107, 106, 1)            # H + W = 212 | 213
    assert mi.marg_layout_ok(544, 17, 16, 33) and not mi.marg_layout_ok(544, 17, 16, 34) and not mi.marg_layout_ok(1000, 1, 1, 16)
    assert mi.marg_width(7, 5) == 48 and mi.marg_width(17, 16) == 64
    forms = {e.form for e in mi.CASES} | {e.marg for e in mi.CASES if e.marg}
    assert forms == {"mode0", "wave mode0_pos", "wave mode1 mode2", "wave mode1 apply8", "regs mode1 mode2", "reread mode1 mode2",
                     "margw mode2", "margw apply8"}


def test_the_family_is_built_as_documented():
    c = mi.build("stage_130x3x2_p4")
    assert c.toks == [0, 383, 384, 779] and c.P == c.x0 + c.W + 2 and (c.t0, c.y0, c.x0) == (0, 132, 138)
    assert bool(torch.isnan(c.pe[130:132]).all()) and bool(torch.isnan(c.pe[135:138]).all()) and bool(torch.isfinite(c.pe[138:140]).all())
    assert bool(torch.isnan(c.scores[c.R:]).all()) and bool(torch.isnan(c.scores[:, c.N:]).all()) and bool(torch.isnan(c.pacc[:, c.R:]).all())
    lvl = c.scores[:c.R, :c.N].reshape(c.R, c.T, 6).max(2).values
    assert float(lvl.max(1).values.sub(lvl.min(1).values).min()) > 3.0                          # the frame maxima differ by several units
    c = mi.build("stage_65x1x1_p200")                                                           # 5 tiles: 195 states without tokens
    assert sum(hi > lo for lo, hi in c.ranges) == 5
    w = torch.exp(up(c.pm)[:, :c.R] - up(c.pm)[:, :c.R].max(0).values)
    assert bool((w.float() == 0).any() or (w < 1e-20).any()) and bool((w == 1).any())
    c = mi.build("nopos_p300")
    w = torch.exp(c.pm[:, :c.R] - c.pm[:, :c.R].max(0).values)
    assert bool((w == 1).sum(0).ge(2).all()) and bool((w < 1e-12).any()) and c.scores is None
    c = mi.build("marg_4x7x5_r9_p2")
    assert c.pmarg.shape == (2, 16, 48) and bool(torch.isnan(c.pmarg[:, :, 8:16]).all()) and bool(torch.isnan(c.pmarg[:, c.R:]).all())
    # the chunk's marginals sum to its l three ways
    for blk in (c.pmarg[:, :c.R, :8], c.pmarg[:, :c.R, 16:23], c.pmarg[:, :c.R, 32:37]):
        assert torch.allclose(blk.sum(2), c.pl[:, :c.R], rtol=1e-5)
    v = mi.build_vproj(768, 12, 7)
    assert v.p16.dtype == torch.float16 and v.wv.dtype == torch.bfloat16 and bool(torch.isnan(v.pacc[:, 12:]).all()) and v.sets.shape[1] % 2 == 0
    k = mi.build_combine("low", 8, 9, 260)
    assert float((k.ml[0, :, 0] - k.ml[1, :, 0]).min()) > 98.0 and bool(torch.isnan(k.packed[:, -7:]).all())
