"""The power of the input family of tests/global_stream_inputs.py (CPU, the float64 references alone): for every case of its table and
every chunk count the GPU tests run it with, each fault below -- planted in the reference, never in the code under test -- must move at
least one output tests/test_gpu_global_stream.py always checks for that form by at least POWER x that output's bound at the offending
element.  The outputs counted: forward M + log L and the merged contexts; backward sum dS x, the t / y / x marginals of dS in the
marginal form, dS itself in the other forms (where it is always written).  The logits are not counted: the marginal form runs without
them.

  lose_chunk_last   every chunk loses its last token (a loop bound or a tail mask one short): out of the softmax, out of dS
  first_frame_off   the tokens of a chunk's first frame are taken for the neighbouring frame, on the score side and in the marginals
                    (`f_first`, the `tf` clamp, the merge's first-frame table).  Not at T = 1: there is no other frame.
  drop_y / drop_x   the y / x positional term of the score tile left out.  Not without a positional table.
  no_delta          dS = p dP in the backward
  pad_leak          the first padded row's result added into the last real row (R < rows_pad only): its context in the forward, its
                    dS (zero gradient row, its own positional row, the last real row's softmax state) in the backward
  scale_1.1         the score tile times 1.1

POWER = 4 is the project's margin (tests/test_many_item_power.py): a condition on the inputs, never lowered.  It is asked of the forward
outputs and of the backward outputs separately (two launches: a fault of one must show in that one).  The weakest figures over all
cases and chunk counts, forward / backward, in bounds: lose_chunk_last 55 / 220, first_frame_off 110 / 218, drop_y 109 / 173,
drop_x 85 / 169, no_delta - / 238, pad_leak 55 / 880, scale_1.1 134 / 45."""
import pytest
import torch

import global_stream_inputs as gi
import ops_reference as R

POWER = 4.0
MUTANTS = ("lose_chunk_last", "first_frame_off", "drop_y", "drop_x", "no_delta", "pad_leak", "scale_1.1")


def wrong_frames(c, nparts):
    """t_of: every token's own frame, but the tokens of a chunk's first frame (inside the chunk) under the next frame (the previous one
    where there is no next)."""
    HW = c.H * c.W
    t_of = torch.arange(c.N) // HW
    for (lo, hi), f in zip(gi.chunk_token_ranges(c.N, nparts), gi.chunk_first_frames(c.N, HW, nparts)):
        n = torch.arange(lo, hi)
        n = n[n // HW == f]
        t_of[n] = f + 1 if f + 1 < c.T else f - 1
    return t_of


def planted(c, name, nparts):
    """(forward kwargs, backward kwargs) of fault `name`, None for a direction it cannot touch; () when it does not apply to the case."""
    e = c.entry
    if name == "lose_chunk_last":
        kw = dict(lost=tuple(hi - 1 for lo, hi in gi.chunk_token_ranges(c.N, nparts) if hi > lo))
        return kw, kw
    if name == "first_frame_off":
        if not e.pos or c.T == 1:
            return ()
        kw = dict(t_of=wrong_frames(c, nparts))
        return kw, kw
    if name in ("drop_y", "drop_x"):
        if not e.pos:
            return ()
        kw = dict(axes=(True, name != "drop_y", name != "drop_x"))
        return kw, kw
    if name == "no_delta":
        return None, dict(use_delta=False)
    if name == "scale_1.1":
        return dict(scale=1.1), dict(scale=1.1)
    raise KeyError(name)


def pad_leak(c, fw, bw):
    """Copies of the two references with the first padded row's result added into row R - 1."""
    R_, E = c.R, c.E
    fa, ba = gi.fwd_args(c), gi.bwd_args(c)
    zero = torch.zeros(1, E, dtype=torch.float64)
    pad = R.global_stream_ref(**{**fa, "q": zero, "pos_a": R.up(c.pos_a)[R_:R_ + 1] if c.entry.pos else None})
    fw2 = dict(fw, ctx=fw["ctx"].clone())
    fw2["ctx"][R_ - 1] += pad["ctx"][0]
    bw2 = None
    if c.entry.pos:
        pb = R.global_stream_bwd_ref(**{**ba, "g": zero, "pos_b": R.up(c.pos_b)[R_:R_ + 1], "S": ba["S"][R_ - 1:R_], "ml": ba["ml"][R_ - 1:R_],
                                        "delta": ba["delta"][R_ - 1:R_]})
        bw2 = dict(bw, dSx=bw["dSx"].clone(), dS=bw["dS"].clone(), marg=tuple(m.clone() for m in bw["marg"]))
        bw2["dSx"][R_ - 1] += pb["dSx"][0]
        bw2["dS"][R_ - 1] += pb["dS"][0]
        for m, a in zip(bw2["marg"], pb["marg"]):
            m[R_ - 1] += a[0]
    return fw2, bw2


def _ratio(got, want, tol):
    got = torch.where(torch.isfinite(got), got, torch.full_like(got, 1e300))       # (a lost token can empty a row: counts as moved)
    return float(((got - want).abs() / tol).max())


def moved(c, form, fw, bw, fb, bb, fw2, bw2):
    """{output: largest |mutant - reference| / bound} over the outputs always checked for `form`."""
    out = {}
    if fw2 is not None:
        out["lse"], out["ctx"] = _ratio(fw2["lse"], fw["lse"], fb["lse"]), _ratio(fw2["ctx"], fw["ctx"], fb["ctx"])
    if bw2 is not None:
        out["dSx"] = _ratio(bw2["dSx"], bw["dSx"], bb["dSx"])
        if form == "marg":
            for name, a, b, t in zip(("mT", "mY", "mX"), bw2["marg"], bw["marg"], bb["marg"]):
                out[name] = _ratio(a, b, t)
        else:
            out["dS"] = _ratio(bw2["dS"], bw["dS"], bb["dS"])
    return out


@pytest.mark.parametrize("id", [e.id for e in gi.CASES])
def test_every_planted_fault_moves_a_checked_output_by_four_bounds(id):
    c = gi.build(id)
    e = c.entry
    fw, bw = gi.forward_ref(id), gi.backward_ref(id)
    short = []
    for nparts in e.nparts:
        form = gi.form_of(e, nparts)
        assert form == e.form, (id, nparts, form)
        fb, bb = gi.forward_bounds(c, fw, nparts), gi.backward_bounds(c, bw, nparts)
        line = []
        for name in MUTANTS:
            if name == "pad_leak":
                if c.R == c.rows_pad:
                    continue
                fw2, bw2 = pad_leak(c, fw, bw)
            else:
                kws = planted(c, name, nparts)
                if kws == ():
                    continue
                fw2 = R.global_stream_ref(**{**gi.fwd_args(c), **kws[0]}) if kws[0] is not None else None
                bw2 = R.global_stream_bwd_ref(**{**gi.bwd_args(c), **kws[1]}) if kws[1] is not None else None
            gaps = moved(c, form, fw, bw, fb, bb, fw2, bw2)
            # a fault of one direction must show in that direction: forward and backward are separate launches
            fwd_best = max((v for k, v in gaps.items() if k in ("lse", "ctx")), default=None)
            bwd_best = max((v for k, v in gaps.items() if k not in ("lse", "ctx")), default=None)
            line.append(f"{name} " + "/".join("-" if v is None else f"{v:.0f}" for v in (fwd_best, bwd_best)))
            for side, v in (("forward", fwd_best), ("backward", bwd_best)):
                if v is not None and not v >= POWER:
                    short.append(f"nparts {nparts} {name} {side}: {v:.2f} bounds")
        print(f"{id} nparts {nparts} [{form}] moved / bound, forward/backward: " + "  ".join(line))
    assert not short, f"{id}: the family lacks power: " + "; ".join(short)


def test_the_family_spikes_the_documented_tokens_and_keeps_the_kernel_number_formats():
    assert gi.chunk_tiles(288, 4) == [0, 4, 9, 13, 18] and gi.chunk_tiles(140, 2) == [0, 4, 9]
    assert gi.chunk_token_ranges(140, 2) == [(0, 64), (64, 140)]
    assert gi.chunk_first_frames(288, 36, 4) == [0, 1, 4, 5]
    assert gi.spike_tokens(140, 35, (2,)) == [0, 15, 16, 34, 35, 63, 64, 69, 70, 104, 105, 139]
    assert gi.spike_tokens(162, 81, (2, 11)) == sorted({0, 161, 80, 81} | {16 * t - 1 for t in range(1, 11)} | {16 * t for t in range(1, 11)})
    tgt = gi.spike_targets(5, 140, gi.spike_tokens(140, 35, (2,)))
    assert float(tgt[0, 0]) == 0.0 and float(tgt[1, 0]) == gi.SHIFT and float(tgt[1, 15]) == 0.0 and float(tgt[0, 34]) == 0.6 * gi.SHIFT
    for id in ("marg_4x7x5_r33", "wide_nopos_4x7x5_r27", "narrow_e768_r27"):
        c = gi.build(id)
        assert c.x.dtype == torch.bfloat16 and c.qhi.dtype == torch.bfloat16 and c.s_in.dtype == torch.float32
        assert bool((c.qhi[c.R:] == 0).all()) and bool((c.dlo[c.R:] == 0).all())
        assert c.P > c.x0 + c.W and bool(torch.isnan(c.s_in[c.R:]).all()) and bool(torch.isnan(c.s_in[:, c.N:]).all())
        fw = gi.forward_ref(id)
        # the forward spikes do what they say: every row's spiked tokens stand about their height above its flat logits
        tg = gi.spike_targets(c.R, c.N, c.toks)
        flat = fw["S"][tg == 0]
        assert float(fw["S"][tg == gi.SHIFT].mean() - flat.mean()) > 0.9 * gi.SHIFT
        assert abs(float(fw["S"][tg == 0.6 * gi.SHIFT].mean() - flat.mean()) - 0.6 * gi.SHIFT) < 0.1 * gi.SHIFT
        if c.entry.pos:
            assert float(c.pe.abs().max()) > 0.5
            # rows of one 16-row group do not share a maximum
            assert len(set(fw["S"][:16].argmax(1).tolist())) > 1


def test_the_restated_predicates_at_their_boundaries():
    assert gi.has_marg(432, 1152, 32, 6, 6, 2) and not gi.has_marg(468, 1152, 32, 6, 6, 2) and gi.has_marg(468, 1152, 32, 6, 6, 7)
    assert not gi.wide_ok(468, 1152, 32, 6, 6, 2) and gi.wide_ok(468, 1152, 32, 6, 6, 2, pos=False)
    assert gi.wide_ok(144, 1152, 32, 12, 12, 2) and not gi.has_marg(144, 1152, 32, 12, 12, 2)             # T = 1
    assert gi.has_marg(544, 1152, 32, 17, 16, 33) and not gi.has_marg(544, 1152, 32, 17, 16, 34)          # the weight record's room
    assert not gi.wide_ok(140, 768, 32, 7, 5, 2) and not gi.wide_ok(140, 1152, 16, 7, 5, 2)
    assert [gi.rows_pad_of(r) for r in (9, 16, 27, 33, 288)] == [16, 16, 32, 64, 288]
