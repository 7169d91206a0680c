"""The power of the input family of tests/window_attn_inputs.py (CPU, the float64 references alone): for every run of its option
matrix -- every (kernel, geometry, D, option) tests/test_gpu_window_attn.py launches -- each fault below, planted in the reference and
never in the code under test, must move at least one output that test checks for that run by at least POWER x that output's bound at
the offending element.  Outputs counted: forward and adaptor forward, the contexts (ctx, or ctx16 where only that is written);
backward, dq, dls, dvalue and (without value_is_key) dkey.

  drop_first / drop_last   the first / last window position out of the softmax (and, in the backward, out of every sum)
  lose_pass_tail           the last position of every workgroup pass lost: every 12th in the forward, every 8th in the adaptor forward;
                           the backward has both pass lengths (phase 1: 8, phase 2: 12) and both are planted, the weaker one counted
  stats_first_64           maximum and sum over the first 64 scores only (a 64-lane loop that never takes its second trip).
                           WIN > 64 only.
  wrong_overlap            trailing windows start one token late (the `- 1` of axis_start dropped).  Overlapping geometries only.
  scale_1.1                logits scaled by 1.1.  WIN > 1 only: one token has weight 1 whatever its logit.
  no_key_norm / no_query_norm   an l2norm bit lost.  Only where the bit is set (forward bits 1 / 2, the backward's l2norm_key).
  no_delta                 dS = p dP.  Backward only.
  drop_kc                  the - kc k term of dk lost.  Backward with l2norm_key only (kc = 0 otherwise).
  overwrite_shared         a token that several windows hold keeps only its last contribution (plain stores where the kernel must
                           accumulate).  Backward over overlapping geometries only.
  no_key_grad_in_dvalue    the key-side gradient not added into dvalue.  Backward with value_is_key only, WIN > 1 (one token: dS = 0
                           and the key-side gradient is zero).
  pool_tap_off             the second tap of the pool equals the first.  Not for (8, 6, 6) -> (8, 6, 6) and (1, 6, 6) -> (1, 2, 2): every
                           source index there is a grid point, the second tap has weight 0 and the fault computes the same values.
Not planted: dls without the `- bias`.  The dS of a window sum to zero, so it cannot be seen.
At WIN = 1 drop_first and drop_last empty the softmax: the reference turns non-finite, which counts as moved.

POWER = 4 is the project's margin (tests/test_many_item_power.py): a condition on the inputs, never lowered.
The weakest figures over all runs, in bounds (forward / adaptor forward / backward; - where the fault does not apply):
  drop_first 57 / 24 / 54        drop_last 52 / 29 / 56         lose_pass_tail 22 / 10 / 66     stats_first_64 23 / 22 / 13
  wrong_overlap 133 / 109 / 124  scale_1.1 9.6 / 5.0 / 45       no_key_norm 274 / - / 102       no_query_norm 27 / - / -
  no_delta - / - / 45            drop_kc - / - / 44             overwrite_shared - / - / 57     no_key_grad_in_dvalue - / - / 50
  pool_tap_off 2e5 (the pool's bound is a few fp32 roundings)
The adaptor forward is the weak side: its logit bound (four chained D-term sums) is four times the plain one.  What the family does
about it is written at window_attn_inputs.build: flat logits a quarter as wide, and value rows ten times as large at the second height.
"""
import pytest
import torch

import ops_reference as R
import window_attn_inputs as wi

POWER = 4.0


def pass_tails(WIN, step):
    return tuple(i for i in range(step - 1, WIN, step))


def overlapping(c):
    return not c.exact


def faults_of(run, c):
    """[(name, kwargs of forward_ref / backward_ref)] that apply to `run`."""
    WIN = c.WIN
    out = [("drop_first", dict(lost=(0,))), ("drop_last", dict(lost=(WIN - 1,)))]
    if run.kernel == "bwd":
        out += [("lose_pass_tail", dict(lost=pass_tails(WIN, s))) for s in (8, 12) if WIN >= s]
    else:
        step = 8 if run.kernel == "adapt" else 12
        if WIN >= step:
            out.append(("lose_pass_tail", dict(lost=pass_tails(WIN, step))))
    if WIN > 64:
        out.append(("stats_first_64", dict(stats_limit=64)))
    if overlapping(c):
        out.append(("wrong_overlap", dict(wrong_overlap=True)))
    if WIN > 1:
        out.append(("scale_1.1", dict(scale_mul=1.1)))
    if run.kernel == "fwd":
        if run.l2norm & 1:
            out.append(("no_key_norm", dict(l2norm=run.l2norm & ~1)))
        if run.l2norm & 2:
            out.append(("no_query_norm", dict(l2norm=run.l2norm & ~2)))
    if run.kernel == "bwd":
        out.append(("no_delta", dict(use_delta=False)))
        if run.l2norm:
            out += [("no_key_norm", dict(l2norm_key=False)), ("drop_kc", dict(drop_kc=True))]
        if overlapping(c):
            out.append(("overwrite_shared", dict(overwrite_shared=True)))
        if run.value_is_key and WIN > 1:
            out.append(("no_key_grad_in_dvalue", dict(key_grad_in_dvalue=False)))
    return out


def _ratio(got, want, tol):
    got = torch.where(torch.isfinite(got), got, torch.full_like(got, 1e300))       # (a lost token can empty a window: counts as moved)
    return float(((got - want).abs() / tol).max())


def moved(run, ref, bounds, mutant):
    if run.kernel == "bwd":
        return max(_ratio(mutant[k], ref[k], bounds[k]) for k in wi.bwd_outputs(run))
    if run.out == "ctx16":
        return _ratio(wi.ctx16_of(mutant["ctx"]), wi.ctx16_of(ref["ctx"]), bounds["ctx16"])
    return _ratio(mutant["ctx"], ref["ctx"], bounds["ctx"])


@pytest.mark.parametrize("run", wi.RUNS, ids=[r.id for r in wi.RUNS])
def test_every_planted_fault_moves_a_checked_output_by_four_bounds(run):
    c = wi.build(run)
    ref = wi.reference(run)
    bounds = wi.backward_bounds(run, ref) if run.kernel == "bwd" else wi.forward_bounds(run, ref)
    make = wi.backward_ref if run.kernel == "bwd" else wi.forward_ref
    short, line = [], {}
    for name, kw in faults_of(run, c):
        v = min(moved(run, ref, bounds, make(run, **kw)), 1e9)                      # (1e9: the reference turned non-finite)
        line[name] = min(v, line.get(name, v))
        if not v >= POWER:
            short.append(f"{name}: {v:.2f} bounds")
    print(f"WINDOW_POWER {run.kernel} {run.id} moved / bound: " + "  ".join(f"{k} {v:.1f}" for k, v in line.items()))
    assert not short, f"{run.id}: the family lacks power: " + "; ".join(short)


@pytest.mark.parametrize("shape,out", wi.POOLS)
def test_pool_tap_off_moves_the_pooled_queries_by_four_bounds(shape, out):
    for D in wi.POOL_D:
        x = R.up(wi.pool_input(shape, D))
        ref, ab, slopes = R.trilinear_pool_ref(x, *out)
        tol = wi.pool_bounds(shape, ab, slopes)
        on_grid = all(float(R._pool_taps(n, m)[2].abs().max()) == 0.0 for n, m in zip(shape, out))
        v = _ratio(R.trilinear_pool_ref(x, *out, second_tap_is_first=True)[0], ref, tol.clamp_min(1e-300))
        print(f"WINDOW_POWER pool {shape}->{out} D={D} pool_tap_off {v:.1f}")
        assert on_grid == (shape in ((8, 6, 6), (1, 6, 6)))
        assert v == 0.0 if on_grid else v >= POWER


def test_the_family_spikes_the_documented_positions():
    assert wi.spike_positions(1) == {0: 1.0} and wi.spike_positions(3) == {0: 1.0, 2: 0.6}
    assert wi.spike_positions(16) == {0: 1.0, 3: 1.0, 4: 1.0, 7: 0.6, 8: 0.6, 11: 0.6, 12: 0.6, 15: 1.0}
    p72 = wi.spike_positions(72)
    assert [p72[i] for i in (11, 12, 59, 60, 63, 64, 7, 8, 71)] == [0.6] * 8 + [1.0] and 65 not in p72
    big = wi.spike_positions(2401)
    assert 2400 in big and 2399 in big and 2388 not in big and 1200 not in big and len(big) < 70
    tgt = wi.spike_targets(3, 16)
    assert float(tgt[0, 0]) == 0.0 and float(tgt[1, 0]) == wi.SHIFT and float(tgt[1, 3]) == 0.0 and float(tgt[2, 4]) == 0.0
    assert float(wi.spike_targets(1, 16)[0, 0]) == wi.SHIFT                        # one window: nothing left out
    for run in (wi.Run("fwd", "w36_exact", 1152), wi.Run("fwd", "w72", 768, l2norm=3), wi.Run("fwd", "w72", 768, l2norm=1),
                wi.Run("adapt", "w16", 768), wi.Run("bwd", "w72", 1152, l2norm=1, query="f32_win")):
        assert run in wi.RUNS or run.kernel == "adapt"
        c = wi.build(run)
        ref = wi.reference(run)
        flat = ref["s"][c.tgt == 0].mean()
        # the spikes do what they say, through the rounding of the stream and (normalised keys) the solved coefficient
        assert abs(float(ref["s"][c.tgt == wi.SHIFT].mean() - flat) - wi.SHIFT) < 0.1 * wi.SHIFT, run.id
        assert abs(float(ref["s"][c.tgt == 0.6 * wi.SHIFT].mean() - flat) - 0.6 * wi.SHIFT) < 0.1 * wi.SHIFT, run.id
        assert len(set(ref["s"].argmax(1).tolist())) > 1 or c.NW == 1
    c = wi.build(wi.Run("fwd", "w3", 1152, out="both", value_dt="f32", big_value=True))
    ref = wi.reference(c.run)
    assert c.run in wi.RUNS and c.value.dtype == torch.float32 and float(ref["ctx"][0, 5]) > 65504.0 and float(ref["p"][0, 2]) > 0.8
