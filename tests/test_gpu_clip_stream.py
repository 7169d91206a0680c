"""HIComProjector.open_stream (GPU; hicom_amd/clip_stream.py, csrc/clip_stream.hip): a clip pushed in chunks against the CPU oracle on the
concatenated clip, the fold kernel alone against float64, and what only a carried state can break.

Inputs: the family of tests/clip_stream_inputs.py (every group of 4 frames times its own power of two, so the running maximum of the global
softmax rises in the second group and not in the third); tests/test_clip_stream_power.py shows on the CPU that a stream that does not rescale
its state, restarts the frame index, resets the state, takes L from the last chunk or misplaces a chunk's rows moves a region by >= 4 bars.

Bars.  Parity: <= 1e-3 max-abs on the fp32 output against oracle.projector_forward on the whole clip, per region (local rows, the 32 global
rows): the bar tests/test_gpu_parity.py holds forward() to.  Against forward() on the concatenation: 2e-3 (each side within 1e-3 of the
oracle; the bar of tests/test_gpu_multi_guide.py).  The 32 global rows are identical bit for bit, newline rows equal image_newline bit for bit.
Fold kernel: the bar tests/test_gpu_global_stream.py applies to the merge (global_stream_inputs.forward_bounds, the terms of `ctx` that belong
to the merge of partials -- no logit error, no matrix cores, no tokens, no positional rows): every weight e^(m - M') carries the device
exponential and the rounding of its argument, the nparts + 1 terms are summed with their rescales,
    |err| <= ((nparts + 8) 2^-23 + 2 TRANS) sum_i w_i |term_i| + sum_i w_i 2^-23 |m_i - M'| |term_i|        for L' and every ACC' element,
and M' is exact.  It is the same arithmetic as hicom_global_merge_fwd's un-normalised output.

Measured on an MI355X (DESIGN.md §3.12 has the table).  Against the oracle: local 2.6e-6 .. 1.4e-5, global 1.0e-7 .. 1.9e-7 at hidden 64; local
5.7e-5, global 6.9e-7 on the 9 x 9 grid at hidden 896.  Against forward(): the local rows are bit-equal, global 1.1e-5 .. 3.3e-5.  The fold alone:
L' err <= 5.9e-6, ACC' err <= 4.7e-6, 0.02 .. 0.10 of the bound; M' exact.  The whole file runs in about 4 s."""
import functools

import numpy as np
import pytest
import torch

import clip_stream_inputs as ci
from clip_stream_inputs import fold_ref
from gpu_util import build_module, dev_bf16
from hicom_amd import native as nv

pytestmark = pytest.mark.gpu

NG = ci.NG
NAN = float("nan")
STORE = "_clip_stream_plans"


# =============================================================================================================================
# the fold kernel alone
# =============================================================================================================================
def fold_inputs(nparts, carried, seed):
    """rows = 9 of rows_pad = 16; the padding rows of the partials are NaN.  carried: "below" / "above" / "equal" (the carried max against
    the chunk's max) or "empty"."""
    rng = np.random.default_rng(seed)
    R, RP, E = 9, 16, 1152
    pm = np.full((nparts, RP), NAN, dtype=np.float32)
    pl = np.full((nparts, RP), NAN, dtype=np.float32)
    pacc = np.full((nparts, RP, E), NAN, dtype=np.float32)
    pm[:, :R] = rng.normal(0.0, 3.0, (nparts, R))
    pl[:, :R] = rng.uniform(1.0, 40.0, (nparts, R))
    pacc[:, :R] = rng.normal(0.0, 5.0, (nparts, R, E))
    top = pm[:, :R].max(axis=0)
    if carried == "empty":
        M, L, A = np.full(R, -np.inf, dtype=np.float32), np.zeros(R, dtype=np.float32), np.zeros((R, E), dtype=np.float32)
    else:
        M = (top + {"below": -2.5, "above": 2.5, "equal": 0.0}[carried]).astype(np.float32)
        L = rng.uniform(1.0, 40.0, R).astype(np.float32)
        A = rng.normal(0.0, 5.0, (R, E)).astype(np.float32)
    return pm, pl, pacc, M, L, A


@pytest.mark.parametrize("nparts", [1, 3, 7])
@pytest.mark.parametrize("carried", ["below", "above", "equal", "empty"])
def test_fold_kernel_against_fp64(nparts, carried):
    pm, pl, pacc, M, L, A = fold_inputs(nparts, carried, 100 * nparts + len(carried))
    d = lambda x: torch.from_numpy(x).cuda()
    ml_in = torch.stack([d(M), d(L)], dim=1).contiguous()
    ml_out = torch.full((9, 2), NAN, dtype=torch.float32, device="cuda")
    acc = d(A).clone()
    nv.stream_state_fold(d(pm), d(pl), d(pacc), 9, ml_in, ml_out, acc)
    torch.cuda.synchronize()
    Mn, Ln, An, l_tol, a_tol = fold_ref(pm, pl, pacc, M, L, A)
    got_ml, got_acc = ml_out.cpu().numpy().astype(np.float64), acc.cpu().numpy().astype(np.float64)
    assert np.isfinite(got_ml).all() and np.isfinite(got_acc).all(), "NaN / Inf: a padding row was read, or -inf - -inf"
    l_err, a_err = np.abs(got_ml[:, 1] - Ln), np.abs(got_acc - An)
    print(f"CLIPSTREAM fold nparts={nparts} {carried}: L err={l_err.max():.3e} ratio={(l_err / l_tol).max():.3e}  "
          f"ACC err={a_err.max():.3e} ratio={(a_err / a_tol).max():.3e}")
    assert np.array_equal(got_ml[:, 0], Mn), "M' is a maximum: exact"
    assert (l_err <= l_tol).all() and (a_err <= a_tol).all()
    assert torch.equal(ml_in, torch.stack([d(M), d(L)], dim=1)), "the block that was read is left alone"
    if carried == "empty":
        # the merge of the partials alone: the same call from any other state that weighs nothing
        ml2, acc2 = torch.full((9, 2), NAN, dtype=torch.float32, device="cuda"), torch.zeros((9, 1152), device="cuda")
        far = torch.stack([torch.full((9,), -1e30, device="cuda"), torch.zeros(9, device="cuda")], dim=1).contiguous()
        nv.stream_state_fold(d(pm), d(pl), d(pacc), 9, far, ml2, acc2)
        assert torch.equal(ml2, ml_out) and torch.equal(acc2, acc)


def test_state_clear_writes_the_empty_state():
    ml = torch.full((2, 9, 2), NAN, dtype=torch.float32, device="cuda")
    acc = torch.full((1, 9, 1152), NAN, dtype=torch.float32, device="cuda")
    nv.stream_state_clear(ml, acc)
    torch.cuda.synchronize()
    assert bool((ml[..., 0] == float("-inf")).all()) and bool((ml[..., 1] == 0).all()) and bool((acc == 0).all())


# =============================================================================================================================
# the stream against the oracle
# =============================================================================================================================
@functools.lru_cache(maxsize=None)
def module(key):
    return build_module(ci.build(key))


@functools.lru_cache(maxsize=None)
def device_clip(key):
    c = ci.build(key)
    return dev_bf16(c.ff), dev_bf16(c.fe), dev_bf16(c.g), dev_bf16(c.g2), dev_bf16(c.newline)


def open_stream(key, guide2=False, max_frames=None):
    c = ci.build(key)
    _, _, g, g2, nl = device_clip(key)
    with torch.no_grad():
        return module(key).open_stream(g2 if guide2 else g, c.h, c.w, max_frames or c.T, nl)


def push_all(s, key, chunking, with_fe=True, t0=0):
    ff, fe, *_ = device_clip(key)
    views = []
    with torch.no_grad():
        for n in chunking:
            views.append(s.push(ff[t0:t0 + n], fe[t0:t0 + n] if with_fe else None))
            t0 += n
    return views


def finish(s):
    with torch.no_grad():
        out = s.finish()
    torch.cuda.synchronize()
    return out


def check(what, got, want, tol=ci.TOL):
    got = got.detach().float().cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    errs = ci.region_errors(got, want)
    print(f"CLIPSTREAM {what}: local {errs['local']:.3e}  global {errs['global']:.3e}  (bar {tol:.0e})")
    bad = [f"{what} {r} rows: {v:.3e} > {tol:.0e}" for r, v in errs.items() if not v <= tol]
    assert not bad, "; ".join(bad)


def check_rows(key, out):
    glob = out[-NG:]
    assert torch.equal(glob, glob[:1].expand_as(glob)), f"the {NG} global rows differ"
    c = ci.build(key)
    if c.newline is not None:
        m = module(key)
        lay = m._layout((c.T // ci.KT, c.h // ci.KS, c.w // ci.KS), "video", True, False)
        nl = device_clip(key)[4].float()
        assert lay.newline_rows and out.shape[0] == lay.n_rows + NG
        for r in lay.newline_rows:
            assert torch.equal(out[r], nl), f"newline row {r}"


PARITY = [(k, ch, True) for k in (ci.T12, ci.T12_GRID, ci.T4) for ch in ci.CHUNKINGS[k]] + [(ci.T12, ch, False) for ch in ci.CHUNKINGS[ci.T12]]


@pytest.mark.parametrize("key,chunking,with_fe", PARITY,
                         ids=[f"T{k[0]}_{k[4] or 'plain'}-{'+'.join(map(str, ch))}-{'fe' if fe else 'no_fe'}" for k, ch, fe in PARITY])
def test_parity_with_the_oracle_and_forward(key, chunking, with_fe):
    s = open_stream(key)
    push_all(s, key, chunking, with_fe)
    out = finish(s)
    assert out.dtype == torch.float32
    tag = f"{key} {chunking} fe={with_fe}"
    check(tag + " vs oracle", out, ci.oracle_output(key, with_fe))
    check_rows(key, out)
    ff, fe, g, _, nl = device_clip(key)
    with torch.no_grad():
        whole = module(key)(ff, fe if with_fe else None, g, "video", nl)
    torch.cuda.synchronize()
    check(tag + " vs forward()", out, whole.float().cpu().numpy(), 2 * ci.TOL)


def test_wider_case_grid_9x9_hidden_896():
    """27 windows per chunk at hidden 896: the readout's tile choice changes with the row count."""
    s = open_stream(ci.WIDE)
    push_all(s, ci.WIDE, (4, 4))
    out = finish(s)
    check(f"{ci.WIDE} (4, 4) vs oracle", out, ci.oracle_output(ci.WIDE))
    check_rows(ci.WIDE, out)
    ff, fe, g, _, nl = device_clip(ci.WIDE)
    with torch.no_grad():
        whole = module(ci.WIDE)(ff, fe, g, "video", nl)
    check(f"{ci.WIDE} (4, 4) vs forward()", out, whole.float().cpu().numpy(), 2 * ci.TOL)


# =============================================================================================================================
# state behaviour
# =============================================================================================================================
def test_finish_does_not_consume_the_state_and_the_clip_may_grow():
    key = ci.T12
    s = open_stream(key)
    views = push_all(s, key, (4, 4))
    first = finish(s).clone()
    again = finish(s)
    assert torch.equal(first, again), "finish() twice without a push"
    check("push 4+4, finish vs oracle on 8 frames", first, ci.oracle_output(key, frames=8))
    # the view push returned is the same rows of finish()'s result
    assert torch.equal(torch.cat(views), first[:-NG]) and views[1].data_ptr() == s.out[views[0].shape[0]:].data_ptr()
    views += push_all(s, key, (4,), t0=8)
    longer = finish(s)
    check("push, finish, push, finish vs oracle on 12 frames", longer, ci.oracle_output(key))
    assert torch.equal(torch.cat(views), longer[:-NG])
    assert s.frames == 12 and s.rows == longer.shape[0] - NG


def test_reset_replays_bit_for_bit_and_takes_a_new_guide():
    key = ci.T12
    s = open_stream(key)
    push_all(s, key, (4, 8))
    first = finish(s).clone()
    with torch.no_grad():
        s.reset()
    assert s.frames == 0
    push_all(s, key, (4, 8))
    assert torch.equal(finish(s), first), "reset() and replay"
    with torch.no_grad():
        s.reset(device_clip(key)[3])
    push_all(s, key, (4, 4, 4))
    check("reset(new guide) vs oracle with that guide", finish(s), ci.oracle_output(key, guide2=True))


def test_two_streams_on_one_projector_do_not_disturb_each_other():
    key = ci.T12
    ff, fe, *_ = device_clip(key)
    solo = []
    for guide2 in (False, True):
        s = open_stream(key, guide2)
        push_all(s, key, (4, 4, 4))
        solo.append(finish(s).clone())
    a, b = open_stream(key), open_stream(key, True)
    with torch.no_grad():
        for t0 in (0, 4, 8):                                  # interleaved: both use the module's one plan and its workspace
            a.push(ff[t0:t0 + 4], fe[t0:t0 + 4])
            b.push(ff[t0:t0 + 4], fe[t0:t0 + 4])
    out_b, out_a = finish(b), finish(a)
    assert torch.equal(out_a, solo[0]) and torch.equal(out_b, solo[1])
    check("second stream vs oracle with its guide", out_b, ci.oracle_output(key, guide2=True))


def test_equal_chunks_share_one_plan_and_push_allocates_nothing():
    key = ci.T12
    m = module(key)
    m.__dict__.pop(STORE, None)
    s = open_stream(key)
    push_all(s, key, (4,))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    push_all(s, key, (4, 4), t0=4)
    assert torch.cuda.memory_allocated() == before, "push allocated device memory"
    plans = m.__dict__[STORE]
    assert len(plans) == 1 and next(iter(plans.values())).hits == 3
    finish(s)
    s2 = open_stream(key)
    push_all(s2, key, (8,))
    assert len(m.__dict__[STORE]) == 2


def test_refusals_on_the_device():
    key = ci.T12
    s = open_stream(key, max_frames=8)
    ff, fe, *_ = device_clip(key)
    with torch.no_grad():
        with pytest.raises(ValueError, match="nothing has been pushed"):
            s.finish()
        with pytest.raises(ValueError, match="whole window groups"):
            s.push(ff[:3], fe[:3])
        s.push(ff[:4], fe[:4])
        with pytest.raises(ValueError, match="exceed max_frames"):
            s.push(ff[4:12], fe[4:12])
        with pytest.raises(ValueError, match="without frames_embed|with frames_embed"):
            s.push(ff[4:8], None)
        with pytest.raises(ValueError, match="opened for"):
            s.push(ff[4:8, :3], fe[4:8, :3])
        assert s.frames == 4
        s.push(ff[4:8], fe[4:8])
    check("after the refusals vs oracle on 8 frames", finish(s), ci.oracle_output(key, frames=8))
