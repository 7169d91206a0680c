"""The power of the input family of tests/multi_window_inputs.py (CPU, the float64 references alone): for every run
tests/test_gpu_multi_window.py launches, each fault below -- planted in the reference, never in the code under test -- must move the fp16
context plane by at least POWER x its bound at the offending element (a reference that turns non-finite counts as moved), and the
family's own conditions must hold: no (guide, window) pair with fewer than two live positions (one at WIN 1), no two guides of a window
whose contexts lie closer than 8 bounds.  The faults are those a many-guide window body can have and a single-guide one cannot, and
the ones of tests/test_window_attn_power.py that one wave per window can still have (multi_window_inputs.mutant has each in full):

  take_max          guide u subtracts guide u ^ 1's maximum.  Counted in the `far` runs alone: softmax does not depend on the constant
                    subtracted, so where neighbouring maxima lie within fp32's exponent range the fault computes the reference's own
                    function, bit errors aside.  The `far` runs put 110 between the maxima of neighbours: the exponentials overflow.
  take_weights      guide u takes guide u ^ 1's weights
  prev_group_rows   the remainder group reads the guide rows of the group in front
  plane_stride      guide planes written at stride plane - D
  drop_last         lane 63 / position WIN - 1 lost            drop_first   position 0 lost          scale_1.1   logits scaled by 1.1
  stats_prev / stats_last   adaptor form: mu / rstd of the previous row / of the last row for all
  no_smu            adaptor form: smu left out                 cg_of_guide_0   adaptor form: the cg of guide 0 for every guide
Not counted: gamma applied once per row instead of per guide and stream (the variant csrc/multi_window.hpp warns against).  In exact
arithmetic it is the same function, and every product gamma_j y_j (bf16 x fp16: 19 bits) is exact in fp32 wherever it is formed: the
variant differs in where the fp32 sums round, which the D-term logit bound holds by construction.
test_gamma_folded_once_per_row_stays_inside_the_bound evaluates it in float64 on fp32 products: 5e-13 of a bound.

POWER = 4 is the project's margin (tests/test_many_item_power.py): a condition on the inputs, never lowered.
The weakest figures over all runs, in bounds: take_weights 23, prev_group_rows 21, drop_last 16, drop_first 13, scale_1.1 6.5,
stats_prev 54, stats_last 12, no_smu 8.7, cg_of_guide_0 9.8; take_max and plane_stride turn the plane non-finite.  The closest two guides
of any window lie 10 bounds apart.  The adaptor form with both streams adapted is the weak side (its logit bound is four D-term sums on
absolute terms); what the family does about it -- guides that keep their size on a block of their own, a lean that tells their cg apart,
y rows with one-signed means, large value rows at the second height -- is written at multi_window_inputs.
"""
import pytest
import torch

import multi_window_inputs as mw
import ops_reference as R
import window_attn_inputs as wi

POWER = 4.0


def moved(run, got):
    want, tol = mw.want16(run), mw.bounds(run)
    got = torch.where(torch.isfinite(got), got, torch.full_like(got, 1e300))
    return min(float(((got - want).abs() / tol).max()), 1e9)


@pytest.mark.parametrize("run", mw.RUNS, ids=[r.id for r in mw.RUNS])
def test_every_planted_fault_moves_the_context_plane_by_four_bounds(run):
    line = {name: moved(run, mw.mutant(run, name)) for name in mw.fault_names(run)}
    print(f"MULTI_WINDOW_POWER {run.id} moved / bound: " + "  ".join(f"{k} {v:.1f}" for k, v in line.items()))
    short = [f"{k}: {v:.2f} bounds" for k, v in line.items() if not v >= POWER]
    assert not short, f"{run.id}: the family lacks power: " + "; ".join(short)


@pytest.mark.parametrize("run", mw.RUNS, ids=[r.id for r in mw.RUNS])
def test_the_input_conditions_hold(run):
    dead, close = mw.conditions(run)
    print(f"MULTI_WINDOW_POWER {run.id} pairs with fewer than two live positions {dead:.3f}  guide pairs closer than {mw.APART:.0f} bounds {close:.3f}")
    assert dead == 0.0 and close == 0.0


def test_every_fault_is_counted_somewhere_and_the_matrix_is_the_documented_one():
    names = {n for run in mw.RUNS for n in mw.fault_names(run)}
    assert names == {"take_max", "take_weights", "prev_group_rows", "plane_stride", "drop_last", "drop_first", "scale_1.1", "stats_prev",
                     "stats_last", "no_smu", "cg_of_guide_0"}
    wins = {g: R.window_tokens(*geom)[0].shape for g, geom in mw.GEOMS.items()}
    assert wins == {"w1": (1, 1), "w3": (1, 3), "w8": (1, 8), "w16": (1, 16), "w36": (8, 36), "w64": (4, 64), "w64_flat": (1, 64), "w9_tail": (3, 9)}
    for form, runs in (("plain", mw.PLAIN_RUNS), ("adapt", mw.ADAPT_RUNS)):
        for g in mw.GEOMS:
            assert {r.Q for r in runs if r.geom == g} == set(mw.ALL_Q if wins[g][1] in (36, 64) else mw.FEW_Q), (form, g)
    for g in ("w36", "w64"):
        for q in mw.ALL_Q:
            assert {r.which for r in mw.ADAPT_RUNS if (r.geom, r.Q) == (g, q)} == set(mw.WHICH)
    assert {(r.which, r.alpha_dt) for r in mw.ADAPT_RUNS} == {(w, a) for w in mw.WHICH for a in ("bf16", "f32")}
    assert [mw.partner(q, 7) for q in range(7)] == [1, 0, 3, 2, 5, 4, 6] and mw.partner(0, 1) == 0


def test_the_family_is_what_the_docstring_says():
    for WIN in (9, 16, 36, 64):
        pos = mw.positions(WIN)
        assert all(pos[i] == 1.0 for i in (0, 3, 4, WIN - 1)) and pos == wi.spike_positions(WIN)
    assert mw.positions(1) == {0: 1.0} and mw.positions(3) == {0: 1.0, 1: 0.85, 2: 1.0} and mw.positions(8) == {0: 1.0, 3: 0.85, 4: 1.0, 7: 1.0}
    tgt = mw.multi_targets(9, 8, 36)
    keys = list(mw.positions(36))
    for q in range(9):
        for w in range(8):
            out = [i for i in keys if float(tgt[q, w, i]) == 0.0]
            assert out == [keys[(w + q) % len(keys)]]
    assert float(mw.multi_targets(1, 1, 64).min(-1).values.max()) == 0.0 and float(mw.multi_targets(1, 1, 64)[0, 0, 0]) == wi.SHIFT
    t3 = mw.multi_targets(5, 1, 3)                                          # k = 3: guides 3 and 4 are the second round
    assert t3[0].tolist() == [[0.0, 8.0 * 0.85, 8.0]] and t3[3].tolist() == [[0.0, 8.0 * 0.85 * mw.SECOND_ROUND, 8.0]]
    # the spikes do what they say through the shared key rows: every guide's maximum sits on one of its own full-height spikes
    for run in (mw.MRun("plain", "w36", 9), mw.MRun("adapt", "w64", 7, "both", "bf16"), mw.MRun("plain", "w64_flat", 5)):
        assert run in mw.RUNS
        c, ref = mw.build(run), mw.reference(run)
        top = ref["s"].argmax(-1)
        assert bool((c.tgt.gather(-1, top[..., None]) == wi.SHIFT).all()), run.id
        assert len({tuple(ref["p"][q, w].gt(mw.LIVE).tolist()) for q in range(c.Q) for w in range(c.NW)}) > 1
    # far: the maxima of neighbours lie FAR apart and the weights are what they were to the planted heights
    run = mw.MRun("plain", "w64", 2, "both", "f32", True)
    assert run in mw.FAR_RUNS
    ref = mw.reference(run)
    gap = ref["mx"][1] - ref["mx"][0]
    assert float((gap - mw.FAR).abs().max()) < 3.0 and float(ref["p"].max(-1).values.min()) > mw.LIVE


def test_the_fault_model_without_a_fault_is_the_reference():
    """mutant() rebuilds logits and contexts outside window_attention_ref; with statistics taken from the row itself it must give
    the reference (so a fault's distance is the fault's, not the restatement's)."""
    for run in (mw.MRun("adapt", "w36", 5, "both", "bf16"), mw.MRun("adapt", "w64", 3, "key", "bf16"), mw.MRun("plain", "w36", 6)):
        assert run in mw.RUNS
        c, ref = mw.build(run), mw.reference(run)
        (K, _, _), (V, _, _) = mw.streams(c, torch.arange(c.N))
        (K0, _, _), (V0, _, _) = mw.streams(c)
        assert float((K - K0).abs().max()) < 1e-11 and float((V - V0).abs().max()) < 1e-11
        s = c.scale * torch.einsum("wid,qd->qwi", K[c.tok], R.up(c.guides))
        assert float((s - ref["s"]).abs().max()) < 1e-10
        ctx = torch.einsum("qwi,wid->qwd", mw._softmax(s), V[c.tok])
        assert float((ctx - ref["ctx"]).abs().max()) < 1e-10
        # and the kernel's algebra: logit from dx, dy, cg, cb; context from the two accumulators and smu
        if run.form == "adapt" and c.ky is not None and c.vy is not None:
            up = R.up
            ak, av, q = float(c.ak.double()), float(c.av.double()), up(c.guides)
            mu, rstd = R.layer_norm_stats(up(c.ky), c.eps)
            cg, cb = (q * up(c.kg)).sum(1), q @ up(c.kb)
            dx, dy = up(c.kx) @ q.T, up(c.ky) @ (q * up(c.kg)).T                                    # [N, Q]
            logit = c.scale * ((1 - ak) * dx + ak * (rstd * (dy - mu * cg) + cb))
            assert float((logit[c.tok].permute(2, 0, 1) - ref["s"]).abs().max()) < 1e-10
            mu, rstd = R.layer_norm_stats(up(c.vy), c.eps)
            p = ref["p"]
            accx = torch.einsum("qwi,wid->qwd", p, up(c.vx)[c.tok])
            accy = torch.einsum("qwi,wid->qwd", p, (rstd * up(c.vy))[c.tok])
            smu = torch.einsum("qwi,wi->qw", p, (rstd * mu)[c.tok].squeeze(-1))
            out = (1 - av) * accx + av * (up(c.vg) * (accy - smu[..., None]) + up(c.vb))
            assert float((out - ref["ctx"]).abs().max()) < 1e-10


def test_gamma_folded_once_per_row_stays_inside_the_bound():
    """Not a counted fault (module docstring): the rounding it adds is far inside the bound, so no test at this precision tells it
    from the reference -- only the bit-equality tests of the suite do."""
    worst = max(mw.gamma_once_shift(run) for run in (mw.MRun("adapt", "w36", 4, "key", "f32"), mw.MRun("adapt", "w64", 4, "both", "f32")))
    print(f"MULTI_WINDOW_POWER gamma_once moved / bound: {worst:.2e}")
    assert worst < 1.0


def test_the_item_cases_spike_every_item():
    for name, (Ts, modals) in mw.ITEM_CASES.items():
        c = mw.item_case(name)
        assert c.windows == sum((T // (1 if m == "image" else 4)) * 4 for T, m in zip(Ts, modals)) and tuple(c.ff.shape) == (sum(Ts) * 36, mw.D)
        # a neighbour's guide row or tokens in the place of an item's own: further than POWER bounds
        for i in range(len(Ts)):
            j = (i + 1) % len(Ts)
            if c.ctx[i].shape == c.ctx[j].shape:
                assert float(((c.ctx[i] - c.ctx[j]).abs() / c.tol[i]).max()) >= POWER
