"""The power of the input table of tests/dense16_inputs.py (CPU, the float64 references alone): for every case each fault below --
planted in the reference, never in the code under test -- must move at least one output tests/test_gpu_dense16.py always checks for
that case (ssq, the fp16 plane, y; pre and row_dot where N % 8 == 0) by at least POWER x that output's bound at the offending element.

  frame_by_block      t taken from the first row of the 16-row MFMA block.  Not at T = 1.
  swap_yx             y = rem % H, x = rem // H
  drop_t0 / y0 / x0   the offset left out.  Only where it is not zero.
  ld_is_N             the table read with pitch N.  Only where tab_ld > N.
  tail_rows_clamped   every row of the last, partly filled row tile takes row M - 1's table rows
  tab_after_ssq       the table added after ssq is taken
  tab_after_act       the table added to the activated value
  pad_cols_in_ssq     the padded columns of the last slice count as b[N - 1].  Only where N % 64 != 0.
  slices_swapped      slices 0 and 1 of ssq / row_dot exchanged.  Only with two slices or more.
  pre_without_tab     the pre-activation plane alone lacks the table.  Only where that plane is checked (N % 8 == 0).
  TN tail_rows_live   the rows Kt .. 64 ceil(Kt / 64) of the last stage taken from the NaN guard and not as zeros: non-finite or moved
  TN last_split_dropped   the last split that owns a stage left out of the sum

POWER = 4 is the project's margin (tests/test_many_item_power.py): a condition on the inputs, never lowered.  The weakest figures over
all cases to which the fault applies, in bounds (inf: the result is not finite): frame_by_block 2.1e4, swap_yx 3.6e4, drop_t0 2.9e4,
drop_y0 3.1e4, drop_x0 3.0e4, ld_is_N 1.7e5, tail_rows_clamped 2.0e4, tab_after_ssq 8.0e3, tab_after_act 3.8e4, pad_cols_in_ssq 5.0e2,
slices_swapped 5.3e3, pre_without_tab 9.4e2, TN tail_rows_live inf, TN last_split_dropped 1.5e4."""
import pytest
import torch

import dense16_inputs as di
import ops_reference as R
from ops_reference import up

POWER = 4.0
NT_FAULTS = ("frame_by_block", "swap_yx", "drop_t0", "drop_y0", "drop_x0", "ld_is_N", "tail_rows_clamped", "tab_after_ssq", "tab_after_act",
             "pad_cols_in_ssq", "slices_swapped", "pre_without_tab")


def planted(c, name):
    """Keywords of dense16_ref for fault `name`; None when it does not apply to the case."""
    e = c.entry
    H, W, t0, y0, x0 = c.geom
    m = torch.arange(c.M)
    if name == "frame_by_block":
        return dict(t_of=(m // 16 * 16) // (H * W)) if c.T > 1 else None
    if name == "swap_yx":
        return dict(swap_yx=True)
    if name in ("drop_t0", "drop_y0", "drop_x0"):
        i = ("drop_t0", "drop_y0", "drop_x0").index(name)
        if e.offs[i] == 0:
            return None
        offs = list(e.offs)
        offs[i] = 0
        return dict(geom=(H, W) + tuple(offs))
    if name == "ld_is_N":
        return dict(tab_pitch=c.N) if e.tab_ld > c.N else None
    if name == "tail_rows_clamped":
        if c.M % 128 == 0:
            return None
        return dict(row_of=torch.where(m >= c.M // 128 * 128, torch.full_like(m, c.M - 1), m))
    if name == "tab_after_ssq":
        return dict(tab_at="after_ssq")
    if name == "tab_after_act":
        return dict(tab_at="after_act")
    if name == "pad_cols_in_ssq":
        return dict(pad_cols_in_ssq=True) if c.N % 64 else None
    if name == "slices_swapped":
        return dict(slices_swapped=True) if c.slices >= 2 else None
    if name == "pre_without_tab":
        return dict(pre_has_tab=False) if "pre" in di.checked_outputs(c) else None
    raise KeyError(name)


def ratio(got, want, tol):
    got = torch.where(torch.isfinite(got), got, torch.full_like(got, float("inf")))
    return float(((got - want).abs() / tol).max())


@pytest.mark.parametrize("id", [e.id for e in di.NT_CASES])
def test_every_planted_nt_fault_moves_a_checked_output_by_four_bounds(id):
    c = di.build(id)
    ref = di.reference(id)
    bounds = di.nt_bounds(c, ref)
    short, line = [], []
    for name in NT_FAULTS:
        kw = planted(c, name)
        if kw is None:
            continue
        bad = R.dense16_ref(**{**di.ref_args(c), **kw})
        gaps = {k: ratio(bad[k], ref[k], bounds[k]) for k in di.checked_outputs(c)}
        best = max(gaps.values())
        line.append(f"{name} {best:.3g}")
        if not best >= POWER:
            short.append(f"{name}: {best:.2f} bounds")
    print(f"DENSE16-POWER {id} moved / bound: " + "  ".join(line))
    assert not short, f"{id}: the table lacks power: " + "; ".join(short)


def test_every_nt_fault_applies_to_some_case_and_the_row_epilogue_cases_check_all_outputs():
    for name in NT_FAULTS:
        assert any(planted(di.build(e.id), name) is not None for e in di.NT_CASES), name
    assert di.checked_outputs(di.build("general_4x7x5")) == ("ssq", "val", "y")
    assert set(di.checked_outputs(di.build("rows_4x7x5"))) == {"ssq", "val", "y", "pre", "rdot"}


@pytest.mark.parametrize("id", [e.id for e in di.TN_CASES])
def test_every_planted_tn_fault_moves_the_product_by_four_bounds(id):
    c = di.build_tn(id)
    e = c.entry
    want = di.reference_tn(id)
    tol = di.tn_tol(e.Kt, want)
    assert bool(torch.isfinite(want).all())
    line = []
    if e.Kt % 64:
        live = R.dense16_tn_ref(up(c.a_full)[:64 * di.tn_stages(e.Kt)], up(c.b_full)[:64 * di.tn_stages(e.Kt)], e.M, e.N)
        line.append(("tail_rows_live", ratio(live, want, tol)))
    per, live_splits = di.tn_live_splits(e.Kt, e.splits)
    dropped = R.dense16_tn_ref(up(c.a_full)[:e.Kt], up(c.b_full)[:e.Kt], e.M, e.N, k_rows=slice(0, 64 * per * (live_splits - 1)))
    line.append(("last_split_dropped", ratio(dropped, want, tol)))
    print(f"DENSE16-POWER {id} moved / bound: " + "  ".join(f"{n} {v:.3g}" for n, v in line))
    assert all(v >= POWER for _, v in line), line


def test_the_tables_hold_the_documented_cases_and_keep_the_kernel_number_formats():
    assert [(e.id, e.grid[0] * e.grid[1] * e.grid[2], e.N, e.K) for e in di.NT_CASES] == [
        ("rows_4x7x5", 140, 136, 128), ("general_4x7x5", 140, 132, 128), ("wide_3x9x11", 297, 1152, 64), ("tall_2x27x19", 1026, 72, 64),
        ("one_frame_1x6x6", 36, 64, 64)]
    assert [tuple(e) for e in di.TN_CASES] == [(1, 8, 8, 8, 8, "bf16", 1), (40, 136, 72, 144, 80, "f16", 1), (200, 136, 264, 136, 264, "bf16", 3),
                                               (700, 264, 136, 272, 144, "f16", 8), (1090, 136, 136, 136, 136, "bf16", 16)]
    assert [di.tn_live_splits(e.Kt, e.splits) for e in di.TN_CASES] == [(1, 1), (1, 1), (2, 2), (2, 6), (2, 9)]
    for e in di.NT_CASES:
        c = di.build(e.id)
        assert c.a.dtype == c.w.dtype == di.DTYPES[e.dtype] and c.b.dtype == c.res.dtype == torch.bfloat16 and c.tab.dtype == torch.float32
        assert c.a.shape == (c.M, c.K + 64) and bool(torch.isnan(c.a[:, c.K:]).all()) and bool(torch.isfinite(c.a[:, :c.K]).all())
        assert c.tab.shape == (e.P, e.tab_ld) and bool(torch.isfinite(c.tab).all()) and abs(float(c.b[-1])) >= 0.05
    rows, gen = di.build("rows_4x7x5"), di.build("general_4x7x5")
    assert rows.entry.tab_ld == 144 and rows.geom == (7, 5, 3, 11, 20) and gen.N % 8 == 4 and gen.entry.tab_ld == gen.N
    for e in di.TN_CASES:
        c = di.build_tn(e.id)
        assert c.a_full.shape == (64 * di.tn_stages(e.Kt) + 8, e.lda) and bool(torch.isnan(c.a_full[e.Kt:]).all())
        assert bool(torch.isnan(c.a_full[:, e.M:]).all()) and bool(torch.isnan(c.b_full[:, e.N:]).all()) and bool(torch.isnan(c.b_full[e.Kt:]).all())
        assert bool(torch.isfinite(c.a_full[:e.Kt, :e.M]).all()) and bool(torch.isfinite(c.b_full[:e.Kt, :e.N]).all())
