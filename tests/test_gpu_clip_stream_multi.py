"""HIComProjector.open_stream_multi (GPU; hicom_amd/clip_stream.py: ClipStreamMulti, csrc/clip_stream.hip): ONE clip pushed in chunks for Q
guides against the CPU oracle per guide on the concatenated clip and against forward_multi_guide, the fold-set kernel alone against float64,
and what only a carried multi-guide state can break.

Inputs: the family of tests/clip_stream_multi_inputs.py (the clips of clip_stream_inputs -- every group of 4 frames times its own power of
two -- and guide q times its own power of two, so the guides have different running maxima and rescale events);
tests/test_clip_stream_multi_power.py shows on the CPU that the five faults of a chunked stream and the three of a multi-guide one (a
chunk's set folded into the neighbour's state, every guide's rows in plane 0, one maximum shared by the guides) move every (guide, region)
they can touch by >= 4 bars.

Bars.  Parity: <= 1e-3 max-abs on the fp32 output against oracle.projector_forward per guide and per region (local rows, the 32 global
rows), the project's bar (tests/test_gpu_parity.py).  Against forward_multi_guide on the concatenation: 2e-3 (each side within 1e-3 of the
oracle).  The 32 global rows of a guide are identical bit for bit, newline rows equal image_newline bit for bit.
Fold-set kernel: the bound of test_fold_kernel_against_fp64 in tests/test_gpu_clip_stream.py (its fold_ref, imported: the carried term and
ONE arriving term, nparts = 1): |err| <= ((1 + 8) 2^-23 + 2 TRANS) sum_i w_i |term_i| + sum_i w_i 2^-23 |m_i - M'| |term_i| for L' and every
ACC' element; M' exact; from the empty state the result is the set bit for bit."""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

import clip_stream_inputs as ci
import clip_stream_multi_inputs as cm
from clip_stream_inputs import fold_ref
from gpu_util import build_module, dev_bf16
from hicom_amd import clip_stream as cs
from hicom_amd import native as nv

pytestmark = pytest.mark.gpu

NG = cm.NG
NAN = float("nan")
STORE = cs.STORE_MULTI
EINVAL, EUNSUP = -1, -2


# =============================================================================================================================
# the fold-set kernel alone
# =============================================================================================================================
@pytest.mark.parametrize("R", [27, 45])
@pytest.mark.parametrize("carried", ["below", "above", "equal", "empty"])
def test_fold_set_kernel_against_fp64(R, carried):
    rng = np.random.default_rng(1000 * R + len(carried))
    E, PAD = 1152, 3
    sm = rng.normal(0.0, 3.0, R).astype(np.float32)
    sl = rng.uniform(1.0, 40.0, R).astype(np.float32)
    sa = rng.normal(0.0, 5.0, (R, E)).astype(np.float32)
    if carried == "empty":
        M, L, A = np.full(R, -np.inf, dtype=np.float32), np.zeros(R, dtype=np.float32), np.zeros((R, E), dtype=np.float32)
    else:
        M = (sm + {"below": -2.5, "above": 2.5, "equal": 0.0}[carried]).astype(np.float32)
        L = rng.uniform(1.0, 40.0, R).astype(np.float32)
        A = rng.normal(0.0, 5.0, (R, E)).astype(np.float32)
    d = lambda x: torch.from_numpy(x).cuda()
    set_ml = torch.stack([d(sm), d(sl)], dim=1).contiguous()                      # interleaved (M, L), as the merges write it
    ml_in = torch.stack([d(M), d(L)], dim=1).contiguous()
    ml_out = torch.full((R + PAD, 2), 7.5, dtype=torch.float32, device="cuda")    # canary rows behind R in both state buffers
    acc = torch.full((R + PAD, E), 7.5, dtype=torch.float32, device="cuda")
    acc[:R] = d(A)
    nv.stream_state_fold_set(set_ml, d(sa), ml_in, ml_out, acc, rows=R)
    torch.cuda.synchronize()
    Mn, Ln, An, l_tol, a_tol = fold_ref(sm[None], sl[None], sa[None], M, L, A)
    got_ml, got_acc = ml_out[:R].cpu().numpy().astype(np.float64), acc[:R].cpu().numpy().astype(np.float64)
    assert np.isfinite(got_ml).all() and np.isfinite(got_acc).all(), "NaN / Inf: -inf - -inf"
    l_err, a_err = np.abs(got_ml[:, 1] - Ln), np.abs(got_acc - An)
    print(f"CLIPSTREAM-MULTI fold set R={R} {carried}: L err={l_err.max():.3e} ratio={(l_err / l_tol).max():.3e}  "
          f"ACC err={a_err.max():.3e} ratio={(a_err / a_tol).max():.3e}")
    assert np.array_equal(got_ml[:, 0], Mn), "M' is a maximum: exact"
    assert (l_err <= l_tol).all() and (a_err <= a_tol).all()
    assert bool((ml_out[R:] == 7.5).all()) and bool((acc[R:] == 7.5).all()), "rows behind R were written"
    assert torch.equal(ml_in, torch.stack([d(M), d(L)], dim=1)), "the block that was read is left alone"
    if carried == "empty":
        assert torch.equal(ml_out[:R], set_ml) and torch.equal(acc[:R], d(sa)), "from the empty state the result is the set"


# =============================================================================================================================
# the stream against the oracle and forward_multi_guide
# =============================================================================================================================
@functools.lru_cache(maxsize=None)
def module(key):
    return build_module(ci.build(key))


@functools.lru_cache(maxsize=None)
def device_clip(key):
    c = ci.build(key)
    return dev_bf16(c.ff), dev_bf16(c.fe), dev_bf16(c.newline)


@functools.lru_cache(maxsize=None)
def device_guides(key, Q, second=False):
    return dev_bf16(cm.guides(key, Q, second))


def open_multi(key, Q, second=False, max_frames=None, guides=None):
    c = ci.build(key)
    with torch.no_grad():
        return module(key).open_stream_multi(device_guides(key, Q, second) if guides is None else guides, c.h, c.w, max_frames or c.T, device_clip(key)[2])


def push_all(s, key, chunking, with_fe=True, t0=0):
    ff, fe, _ = device_clip(key)
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


def check(what, got, want, tol=cm.TOL):
    got = got.detach().float().cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    errs = cm.region_errors(got, want)
    loc, glob = [errs[q, "local"] for q in range(got.shape[0])], [errs[q, "global"] for q in range(got.shape[0])]
    print(f"CLIPSTREAM-MULTI {what}: local {min(loc):.3e} .. {max(loc):.3e}  global {min(glob):.3e} .. {max(glob):.3e}  (bar {tol:.0e})")
    bad = [f"{what} guide {q} {r} rows: {v:.3e} > {tol:.0e}" for (q, r), v in errs.items() if not v <= tol]
    assert not bad, "; ".join(bad)


def check_rows(key, out):
    for q in range(out.shape[0]):
        glob = out[q, -NG:]
        assert torch.equal(glob, glob[:1].expand_as(glob)), f"guide {q}: the {NG} global rows differ"
    c = ci.build(key)
    if c.newline is not None:
        lay = module(key)._layout((c.T // ci.KT, c.h // ci.KS, c.w // ci.KS), "video", True, False)
        nl = device_clip(key)[2].float()
        assert lay.newline_rows and out.shape[1] == lay.n_rows + NG
        for r in lay.newline_rows:
            assert torch.equal(out[:, r], nl.expand(out.shape[0], -1)), f"newline row {r}"


def whole_clip(key, Q, with_fe=True):
    """forward_multi_guide on the concatenation: the resident-clip counterpart."""
    ff, fe, nl = device_clip(key)
    with torch.no_grad():
        out = module(key).forward_multi_guide(ff, fe if with_fe else None, device_guides(key, Q), "video", nl)
    torch.cuda.synchronize()
    return out


def parity(key, Q, chunking, with_fe):
    s = open_multi(key, Q)
    push_all(s, key, chunking, with_fe)
    out = finish(s)
    assert out.dtype == torch.float32 and out.stride(0) == s.out.stride(0)
    tag = f"{key} Q={Q} {chunking} fe={with_fe}"
    check(tag + " vs oracle", out, cm.oracle_guides(key, Q, with_fe))
    check_rows(key, out)
    whole = whole_clip(key, Q, with_fe)
    check(tag + " vs forward_multi_guide", out, whole.float().cpu().numpy(), 2 * cm.TOL)
    # the same local kernel, the same readout GEMMs on the same rows in another row order: held on the first MI355X run for all 27 cases
    assert torch.equal(out[:, :-NG], whole[:, :-NG]), "the local rows are those of forward_multi_guide bit for bit"
    return s, out, whole


PARITY = [(k, Q, ch, fe) for Q in (3, 5) for k, fe in ((cm.T12, True), (cm.T12, False), (cm.T12_GRID, True)) for ch in cm.T12_CHUNKINGS]


@pytest.mark.parametrize("key,Q,chunking,with_fe", PARITY,
                         ids=[f"Q{Q}-T12_{k[4] or 'plain'}-{'+'.join(map(str, ch))}-{'fe' if fe else 'no_fe'}" for k, Q, ch, fe in PARITY])
def test_parity_with_the_oracle_and_forward_multi_guide(key, Q, chunking, with_fe):
    """Q = 3: 27 folded rows, one 32-row pass of the stream kernel.  Q = 5: 45 rows, two passes, and guide 4 alone in the last group of the local
    kernel."""
    parity(key, Q, chunking, with_fe)


def test_wider_case_grid_9x9_hidden_896():
    """27 windows per chunk and guide at hidden 896: the readout's tile choice changes with the row count."""
    parity(cm.WIDE, 2, (4, 4), True)


def test_both_merge_forms_are_reached(monkeypatch):
    """The form is chosen once per plan (hicom_global_stream_has_marg, as the multi-guide step chooses it): in-kernel marginals for these
    chunk shapes; under HICOM_GLOBAL_NO_MARG=1, the switch of the many-row stream, a fresh plan takes the logit-tensor form.  Both against
    the same bars."""
    key, Q = cm.T12, 5
    m = module(key)
    m.__dict__.pop(STORE, None)
    s, out_marg, _ = parity(key, Q, (4, 8), True)
    forms = {p.args.marg for p in m.__dict__[STORE].values()}
    assert forms == {1}, "the chunks of 4 and 8 frames of a 6 x 6 grid have in-kernel marginals"
    monkeypatch.setenv("HICOM_GLOBAL_NO_MARG", "1")
    m.__dict__.pop(STORE, None)
    try:
        s, out_logit, _ = parity(key, Q, (4, 8), True)
        assert {p.args.marg for p in m.__dict__[STORE].values()} == {0}
    finally:
        m.__dict__.pop(STORE, None)                        # (later tests build their plans without the switch)
    d = float((out_marg - out_logit).abs().max())
    print(f"CLIPSTREAM-MULTI marginal form vs logit-tensor form: max-abs {d:.3e}")
    assert d <= 2 * cm.TOL


# =============================================================================================================================
# state behaviour
# =============================================================================================================================
def test_finish_does_not_consume_the_state_and_the_clip_may_grow():
    key, Q = cm.T12, 3
    s = open_multi(key, Q)
    views = push_all(s, key, (4, 4))
    first = finish(s).clone()
    assert torch.equal(first, finish(s)), "finish() twice without a push"
    check("push 4+4, finish vs oracle on 8 frames", first, cm.oracle_guides(key, Q, frames=8))
    assert torch.equal(torch.cat(views, dim=1), first[:, :-NG]) and views[1].data_ptr() == s.out[:, views[0].shape[1]:].data_ptr()
    views += push_all(s, key, (4,), t0=8)
    longer = finish(s)
    check("push, finish, push, finish vs oracle on 12 frames", longer, cm.oracle_guides(key, Q))
    assert torch.equal(longer[:, :first.shape[1] - NG], first[:, :-NG]), "the earlier prefix's local rows changed"
    assert torch.equal(torch.cat(views, dim=1), longer[:, :-NG])
    assert s.frames == 12 and s.rows == longer.shape[1] - NG


def test_reset_replays_bit_for_bit_and_takes_new_guides():
    key, Q = cm.T12, 3
    s = open_multi(key, Q)
    push_all(s, key, (4, 8))
    first = finish(s).clone()
    with torch.no_grad():
        s.reset()
    assert s.frames == 0
    push_all(s, key, (4, 8))
    assert torch.equal(finish(s), first), "reset() and replay"
    with torch.no_grad():
        s.reset(device_guides(key, Q, True))
        with pytest.raises(ValueError, match="opened for Q=3"):
            s.reset(device_guides(key, 2))
    push_all(s, key, (4, 4, 4))
    check("reset(new guides) vs oracle with those guides", finish(s), cm.oracle_guides(key, Q, second=True))


def test_two_streams_on_one_projector_do_not_disturb_each_other():
    key, Q = cm.T12, 3
    ff, fe, _ = device_clip(key)
    solo = []
    for second in (False, True):
        s = open_multi(key, Q, second)
        push_all(s, key, (4, 4, 4))
        solo.append(finish(s).clone())
    a, b = open_multi(key, Q), open_multi(key, Q, True)
    with torch.no_grad():
        for t0 in (0, 4, 8):                                  # interleaved: both use the module's one plan and its workspace
            a.push(ff[t0:t0 + 4], fe[t0:t0 + 4])
            b.push(ff[t0:t0 + 4], fe[t0:t0 + 4])
    out_b, out_a = finish(b), finish(a)
    assert torch.equal(out_a, solo[0]) and torch.equal(out_b, solo[1])
    check("second stream vs oracle with its guides", out_b, cm.oracle_guides(key, Q, second=True))


# =============================================================================================================================
# the guides do not leak into each other
# =============================================================================================================================
def test_replacing_one_guide_moves_only_its_output():
    key, Q = cm.T12, 3
    s = open_multi(key, Q)
    push_all(s, key, (4, 4, 4))
    before = finish(s).clone()
    g = device_guides(key, Q).clone()
    g[1] = device_guides(key, Q, True)[1]
    s2 = open_multi(key, Q, guides=g)
    push_all(s2, key, (4, 4, 4))
    after = finish(s2)
    for q in (0, 2):
        d = float((after[q] - before[q]).abs().max())
        print(f"CLIPSTREAM-MULTI guide 1 replaced: guide {q} moved by {d:.3e}")
        assert d <= 2 * cm.TOL
    assert float((after[1] - before[1]).abs().max()) > 4 * cm.TOL, "the replaced guide's output did not move"
    want = cm.oracle_guides(key, Q, second=True)[1]
    assert float(np.abs(after[1].cpu().numpy() - want).max()) <= cm.TOL


def test_one_guide_agrees_with_the_single_guide_stream():
    key = cm.T12
    g = device_guides(key, 3)[:1].contiguous()
    s = open_multi(key, 1, guides=g)
    push_all(s, key, (4, 8))
    multi = finish(s)
    with torch.no_grad():
        single = module(key).open_stream(g[0], 6, 6, 12, None)
    push_all(single, key, (4, 8))
    one = finish(single)
    d = float((multi[0] - one).abs().max())
    print(f"CLIPSTREAM-MULTI Q=1 vs ClipStream: max-abs {d:.3e}")
    assert tuple(multi.shape) == (1,) + tuple(one.shape) and d <= 2 * cm.TOL


# =============================================================================================================================
# plans, allocation, refusals on the device
# =============================================================================================================================
def test_equal_chunks_share_one_plan_and_push_allocates_nothing():
    key, Q = cm.T12, 3
    m = module(key)
    m.__dict__.pop(STORE, None)
    s = open_multi(key, Q)
    push_all(s, key, (4,))
    finish(s)
    before = torch.cuda.memory_allocated()
    push_all(s, key, (4, 4), t0=4)
    finish(s)
    assert torch.cuda.memory_allocated() == before, "push or finish allocated device memory"
    plans = m.__dict__[STORE]
    assert len(plans) == 1 and next(iter(plans.values())).hits == 3
    s2 = open_multi(key, Q)
    push_all(s2, key, (8,))
    assert len(plans) == 2
    s5 = open_multi(key, 5)
    push_all(s5, key, (4,))
    assert len(plans) == 3                                   # Q is part of the key


def test_the_c_entry_point_refuses_in_front_of_any_launch():
    """Argument checks on a real, filled block: a frame range outside the positional tables, overlapping (M, L) blocks, a NULL pointer,
    Q = 33.  None launches: the stream's buffers and state are what they were."""
    key, Q = cm.T12, 3
    m = module(key)
    s = open_multi(key, Q)
    push_all(s, key, (4,))
    torch.cuda.synchronize()
    plan = next(p for k, p in m.__dict__[STORE].items() if k[0] == Q and k[1] == 4)
    a = plan.args
    bits = lambda t: t.view(torch.int32)                      # (the untouched part of `out` is uninitialised memory: compare bits, not values)
    out0, ml0, acc0 = bits(s.out).clone(), bits(s.state_ml).clone(), bits(s.state_acc).clone()
    L = nv.lib()
    saved = {f: getattr(a, f) for f in ("t0", "state_ml_out", "ff", "Q", "set_acc")}
    try:
        for over, code, needle in ((dict(t0=a.y_index0), EINVAL, "outside the positional tables"),
                                   (dict(state_ml_out=a.state_ml_in), EINVAL, "overlap"),
                                   (dict(state_ml_out=a.state_ml_in + 8 * (Q * 9 - 1)), EINVAL, "overlap"),
                                   (dict(ff=None), EINVAL, "NULL pointer"), (dict(set_acc=None), EINVAL, "NULL pointer"),
                                   (dict(Q=33), EUNSUP, "1 <= Q <= 32")):
            for f, v in over.items():
                setattr(a, f, v)
            got = L.hicom_compressor_stream_push_multi(ctypes.byref(a))
            msg = L.hicom_last_error().decode()
            assert got == code and re.search(needle, msg), (over, got, msg)
            for f, v in saved.items():
                setattr(a, f, v)
    finally:
        for f, v in saved.items():
            setattr(a, f, v)
    torch.cuda.synchronize()
    assert torch.equal(bits(s.out), out0) and torch.equal(bits(s.state_ml), ml0) and torch.equal(bits(s.state_acc), acc0), "a refused call launched something"
    push_all(s, key, (4, 4), t0=4)                            # the block still serves
    check("after the refusals vs oracle", finish(s), cm.oracle_guides(key, Q))
