"""HIComProjector.open_stream_adapt (GPU; hicom_amd/clip_stream.py: ClipStreamAdapt, csrc/clip_stream.hip, csrc/multi_guide.hip): ONE clip
pushed in chunks for Q guides on the k / v adaptor recipe against the CPU oracle per guide on the concatenated clip, against prepare_clip +
forward_prepared on the resident clip, against a plain module through open_stream_multi, the local adapt entry point alone, and what only
planes that live for one push can break.

Inputs: tests/clip_stream_adapt_inputs.py (the clips and guides of the multi-guide stream's tests under the adaptkv weights of
many_item_inputs); tests/test_clip_stream_adapt_power.py shows on the CPU that the eight faults of a chunked multi-guide stream and the four of
a per-chunk adaptor stage (the previous push's planes read, the planes swapped, the blend skipped from the second push on, the k adaptor fed
frames_feature) move every (guide, region) they can touch by >= 4 bars.

Bars.  Parity: the rule of many_item_inputs, <= 1e-3 max-abs on the fp32 output against oracle.projector_forward per guide and per region.
Against forward_prepared on the concatenation: 2e-3 on the global rows (each side within 1e-3 of the oracle, the bar
tests/test_gpu_clip_stream_multi.py holds against forward_multi_guide); the local rows bit for bit -- the same window kernel on the same
planes, and a row of the dense GEMM that makes the planes does not depend on how many rows the call has.  Against a plain module with the same
weights through open_stream_multi: the 32 global rows of every guide bit for bit (the global stage of the recipe is the plain one)."""
import ctypes
import functools
import math
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import clip_stream_adapt_inputs as ca
from gpu_util import build_module, dev_bf16
from hicom_amd import clip_stream as cs
from hicom_amd import native as nv
from hicom_amd import prepared
from oracle import hicom_oracle as orc

pytestmark = pytest.mark.gpu

NG = ca.NG
STORE = cs.STORE_ADAPT
EINVAL, EUNSUP = -1, -2
KV, K_ONLY, V_ONLY = ca.ADAPTKV, ca.ADAPTK, ca.ADAPTV


@functools.lru_cache(maxsize=None)
def _module(key, recipe):
    return build_module(ca.build(key, recipe))


def module(key, recipe=KV):
    return _module(key, recipe)                                # (one cache entry per module, however it is asked for)


@functools.lru_cache(maxsize=None)
def plain_module(key):
    """The plain recipe with the weights the adaptkv module shares with it."""
    c = ca.build(key)
    cfg = SimpleNamespace(**{**vars(c.cfg), "mm_projector_type": ca.mi.PLAIN})
    return build_module(SimpleNamespace(cfg=cfg, sd={k: v for k, v in c.sd.items() if k in orc.param_shapes(cfg)}))


@functools.lru_cache(maxsize=None)
def device_clip(key):
    c = ca.build(key)
    return dev_bf16(c.ff), dev_bf16(c.fe), dev_bf16(c.newline)


@functools.lru_cache(maxsize=None)
def device_guides(key, Q, second=False):
    return dev_bf16(ca.guides(key, Q, second))


def open_adapt(key, Q, recipe=KV, second=False, guides=None, m=None):
    c = ca.build(key, recipe)
    with torch.no_grad():
        return (m or module(key, recipe)).open_stream_adapt(device_guides(key, Q, second) if guides is None else guides, c.h, c.w, c.T, device_clip(key)[2])


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


def check(what, got, want):
    """Per guide and region at the bar of many_item_inputs for that guide's oracle output."""
    got = got.detach().float().cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    errs = ca.region_errors(got, want)
    Q = got.shape[0]
    loc, glob = [errs[q, "local"] for q in range(Q)], [errs[q, "global"] for q in range(Q)]
    tol = [ca.tolerance(want[q]) for q in range(Q)]
    print(f"CLIPSTREAM-ADAPT {what}: local {min(loc):.3e} .. {max(loc):.3e}  global {min(glob):.3e} .. {max(glob):.3e}  (bar {max(tol):.0e})")
    bad = [f"{what} guide {q} {r} rows: {v:.3e} > {tol[q]:.0e}" for (q, r), v in errs.items() if not v <= tol[q]]
    assert not bad, "; ".join(bad)


def check_rows(key, out):
    for q in range(out.shape[0]):
        glob = out[q, -NG:]
        assert torch.equal(glob, glob[:1].expand_as(glob)), f"guide {q}: the {NG} global rows differ"
    c = ca.build(key)
    if c.newline is not None:
        lay = module(key)._layout((c.T // ca.KT, c.h // ca.KS, c.w // ca.KS), "video", True, False)
        nl = device_clip(key)[2].float()
        assert lay.newline_rows and out.shape[1] == lay.n_rows + NG
        for r in lay.newline_rows:
            assert torch.equal(out[:, r], nl.expand(out.shape[0], -1)), f"newline row {r}"


@functools.lru_cache(maxsize=None)
def resident(key, recipe, Q, with_fe):
    """prepare_clip + ONE forward_prepared on the concatenation: the resident-clip counterpart."""
    ff, fe, nl = device_clip(key)
    m = module(key, recipe)
    with torch.no_grad():
        clip = m.prepare_clip(ff, fe if with_fe else None, "video")
        out = m.forward_prepared(clip, device_guides(key, Q), nl)
    torch.cuda.synchronize()
    return out, clip


def parity(key, recipe, Q, chunking, with_fe):
    s = open_adapt(key, Q, recipe)
    assert type(s) is cs.ClipStreamAdapt
    push_all(s, key, chunking, with_fe)
    out = finish(s)
    assert out.dtype == torch.float32 and out.stride(0) == s.out.stride(0)
    tag = f"{key} {recipe.split('_')[1]} Q={Q} {chunking} fe={with_fe}"
    check(tag + " vs oracle", out, ca.oracle_guides(key, recipe, Q, with_fe))
    check_rows(key, out)
    whole = resident(key, recipe, Q, with_fe)[0]
    d_loc, d_glob = float((out[:, :-NG] - whole[:, :-NG]).abs().max()), float((out[:, -NG:] - whole[:, -NG:]).abs().max())
    print(f"CLIPSTREAM-ADAPT {tag} vs forward_prepared: local {d_loc:.3e}  global {d_glob:.3e}")
    assert d_glob <= 2 * ca.mi.TOL
    assert torch.equal(out[:, :-NG], whole[:, :-NG]), "the local rows are those of forward_prepared on the resident clip bit for bit"
    return s, out


PARITY = [(k, r, Q, fe, ch) for k, r, Q, fe, chs in ca.CASES if k != ca.WIDE for ch in chs]


@pytest.mark.parametrize("key,recipe,Q,with_fe,chunking", PARITY,
                         ids=[f"{r.split('_')[1]}-Q{Q}-T12_{k[4] or 'plain'}-{'+'.join(map(str, ch))}-{'fe' if fe else 'no_fe'}" for k, r, Q, fe, ch in PARITY])
def test_parity_with_the_oracle_and_forward_prepared(key, recipe, Q, with_fe, chunking):
    """Q = 4: one full group of the adapt local kernel; Q = 5: a full group and a remainder of one, two passes of the stream kernel; Q = 9:
    three groups, 81 folded rows.  adapt_k alone and adapt_v alone at Q = 3: the single-problem GEMMs and one NULL plane."""
    parity(key, recipe, Q, chunking, with_fe)


def test_wider_case_grid_9x9_hidden_896():
    """324 tokens and 27 windows per chunk at hidden 896."""
    parity(ca.WIDE, KV, 2, (4, 4), True)


def test_global_rows_are_those_of_a_plain_module_bit_for_bit():
    """The adaptors sit on the local stage only: the same weights without them, through open_stream_multi, give the same 32 global rows per
    guide, and other local rows."""
    key, Q = ca.T12, 5
    s = open_adapt(key, Q)
    push_all(s, key, (4, 8))
    out = finish(s)
    pm = plain_module(key)
    with torch.no_grad():
        routed = pm.open_stream_adapt(device_guides(key, Q), 6, 6, 12, None)
    assert type(routed) is cs.ClipStreamMulti, "a plain module gets open_stream_multi's object"
    push_all(routed, key, (4, 8))
    plain = finish(routed)
    assert torch.equal(out[:, -NG:], plain[:, -NG:]), "global rows"
    assert float((out[:, :-NG] - plain[:, :-NG]).abs().max()) > 4 * ca.mi.TOL, "the adaptors do not reach the local rows"


# =============================================================================================================================
# state behaviour: bit-equal checks
# =============================================================================================================================
def test_finish_does_not_consume_the_state_and_the_clip_may_grow():
    key, Q = ca.T12, 4
    s = open_adapt(key, Q)
    views = push_all(s, key, (4, 4))
    first = finish(s).clone()
    assert torch.equal(first, finish(s)), "finish() twice without a push"
    check("push 4+4, finish vs oracle on 8 frames", first, ca.oracle_guides(key, KV, Q, frames=8))
    assert torch.equal(torch.cat(views, dim=1), first[:, :-NG])
    views += push_all(s, key, (4,), t0=8)
    longer = finish(s)
    assert torch.equal(longer[:, :first.shape[1] - NG], first[:, :-NG]), "the earlier prefix's local rows changed"
    assert torch.equal(torch.cat(views, dim=1), longer[:, :-NG])
    one_go = open_adapt(key, Q)
    push_all(one_go, key, (4, 4, 4))
    assert torch.equal(longer, finish(one_go)), "push, finish, push, finish against the pushes alone"
    check("push, finish, push, finish vs oracle on 12 frames", longer, ca.oracle_guides(key, KV, Q))


def test_reset_replays_bit_for_bit_and_takes_new_guides():
    key, Q = ca.T12, 4
    s = open_adapt(key, Q)
    push_all(s, key, (4, 8))
    first = finish(s).clone()
    with torch.no_grad():
        s.reset()
    push_all(s, key, (4, 8))
    assert torch.equal(finish(s), first), "reset() and replay"
    fresh = open_adapt(key, Q, second=True)
    push_all(fresh, key, (4, 8))
    want = finish(fresh).clone()
    with torch.no_grad():
        s.reset(device_guides(key, Q, True))
    push_all(s, key, (4, 8))
    got = finish(s)
    assert torch.equal(got, want), "reset(new guides) and replay against a stream opened with them"
    check("reset(new guides) vs oracle with those guides", got, ca.oracle_guides(key, KV, Q, second=True))


def test_two_interleaved_streams_share_one_plan_and_its_planes():
    """Both streams use the module's one plan, so the SAME ky / vy planes: stream b pushes another part of the clip between a's pushes (the
    planes hold other tokens' MLP outputs when a pushes again)."""
    key, Q = ca.T12, 4
    m = module(key)
    ff, fe, _ = device_clip(key)
    order_a, order_b = (0, 4, 8), (8, 0, 4)                    # b sees the clip's groups in another order: a clip of its own
    solo = []
    for second, order in ((False, order_a), (True, order_b)):
        s = open_adapt(key, Q, second=second)
        with torch.no_grad():
            for t0 in order:
                s.push(ff[t0:t0 + 4], fe[t0:t0 + 4])
        solo.append(finish(s).clone())
    m.__dict__.pop(STORE, None)
    a, b = open_adapt(key, Q), open_adapt(key, Q, second=True)
    with torch.no_grad():
        for ta, tb in zip(order_a, order_b):
            a.push(ff[ta:ta + 4], fe[ta:ta + 4])
            b.push(ff[tb:tb + 4], fe[tb:tb + 4])
    out_b, out_a = finish(b), finish(a)
    assert len(m.__dict__[STORE]) == 1 and next(iter(m.__dict__[STORE].values())).hits == 6
    assert torch.equal(out_a, solo[0]) and torch.equal(out_b, solo[1])
    check("first stream vs oracle", out_a, ca.oracle_guides(key, KV, Q))


def test_replacing_one_guide_leaves_the_others_untouched():
    key, Q = ca.T12, 5
    s = open_adapt(key, Q)
    push_all(s, key, (4, 4, 4))
    before = finish(s).clone()
    g = device_guides(key, Q).clone()
    g[1] = device_guides(key, Q, True)[1]
    s2 = open_adapt(key, Q, guides=g)
    push_all(s2, key, (4, 4, 4))
    after = finish(s2)
    for q in (0, 2, 3, 4):
        assert torch.equal(after[q, :-NG], before[q, :-NG]), f"guide {q}: local rows moved"
        d = float((after[q] - before[q]).abs().max())
        print(f"CLIPSTREAM-ADAPT guide 1 replaced: guide {q} moved by {d:.3e}")
        assert d <= 2 * ca.mi.TOL
    assert float((after[1] - before[1]).abs().max()) > 4 * ca.mi.TOL, "the replaced guide's output did not move"
    want = ca.oracle_guides(key, KV, Q, second=True)[1]
    assert float(np.abs(after[1].cpu().numpy() - want).max()) <= ca.tolerance(want)


# =============================================================================================================================
# plans, allocation, the weights, the entry points
# =============================================================================================================================
def test_push_and_finish_allocate_nothing_after_the_first_push_of_a_shape():
    key, Q = ca.T12, 4
    m = module(key)
    m.__dict__.pop(STORE, None)
    s = open_adapt(key, Q)
    push_all(s, key, (4,))
    finish(s)
    before = torch.cuda.memory_allocated()
    push_all(s, key, (4, 4), t0=4)
    finish(s)
    assert torch.cuda.memory_allocated() == before, "push or finish allocated device memory"
    plans = m.__dict__[STORE]
    (plan,) = plans.values()
    assert plan.hits == 3
    args = plan.args
    lo, hi = plan.ws.data_ptr(), plan.ws.data_ptr() + plan.ws.numel()
    N = 4 * 6 * 6
    for p, n in ((args.ky, N * ca.D * 2), (args.vy, N * ca.D * 2), (args.adapt_ws, args.adapt_ws_bytes)):
        assert lo <= p and p + n <= hi and p % 256 == 0, "the planes and the hidden planes lie in the plan's one workspace"
    assert args.adapt_ws_bytes == nv.clip_adapt_prepare_workspace(N, ca.D, args.ak, args.av) == 2 * N * ca.D * 2
    assert args.base.ctx_f16 + Q * 4 * ca.D * 2 <= args.base.hid_f16 <= args.ky


def test_the_plan_follows_the_adaptor_weights():
    """A second layer written in place: the next push runs on the new weights (the plan's refresh rebuilds the fp16 copy its descriptor
    points at), and the old weights written back give the first result bit for bit."""
    key, Q = ca.T12, 4
    m = build_module(ca.build(key))                             # a module of its own: its weights move
    s = open_adapt(key, Q, m=m)
    push_all(s, key, (12,))
    first = finish(s).clone()
    w = m.local_compressor.v_proj[2].weight
    old = w.detach().clone()
    with torch.no_grad():
        w.mul_(0.5)
        s.reset()
    push_all(s, key, (12,))
    moved = finish(s).clone()
    assert float((moved[:, :-NG] - first[:, :-NG]).abs().max()) > ca.mi.TOL, "the stream did not follow the adaptor's weights"
    assert torch.equal(moved[:, -NG:], first[:, -NG:]), "the global rows do not read the adaptors"
    with torch.no_grad():
        w.copy_(old)
        s.reset()
    push_all(s, key, (12,))
    assert torch.equal(finish(s), first)


def test_local_adapt_entry_point_alone_leaves_the_contexts_of_forward_prepared():
    """hicom_multi_guide_local_adapt_fwd on a 4-frame 6 x 6 chunk against hicom_compressor_multiguide_adapt_fwd on the same tokens and the same
    planes: the fp16 contexts in the step's workspace, bit for bit.  The step's workspace ends with its regions ctx16 [Q windows, E] fp16,
    hid16 [Q windows, hidden] fp16 and loc [Q windows, hidden] of the output dtype, each rounded up to 256 bytes (csrc/segment_host.hpp)."""
    key, Q = ca.T12, 5
    m = module(key)
    ff, fe, _ = device_clip(key)
    g = device_guides(key, Q)
    m.__dict__.pop(prepared.STORE, None)
    with torch.no_grad():
        clip = m.prepare_clip(ff[:4], fe[:4], "video")
        m.forward_prepared(clip, g)
    torch.cuda.synchronize()
    (plan,) = m.__dict__[prepared.STORE].values()
    W, hidden = Q * 4, ca.build(key).hidden
    up = lambda n: (n + 255) // 256 * 256
    off = plan.ws.numel() - up(W * hidden * 4) - up(W * hidden * 2) - up(W * ca.D * 2)
    want = plan.ws[off:off + W * ca.D * 2].view(torch.float16).view(Q, 4, ca.D).clone()
    assert float(want.float().abs().max()) > 0.1
    a = plan.args
    got = torch.full((Q, 4, ca.D), float("nan"), dtype=torch.float16, device="cuda")
    nv.multi_guide_local_adapt(fe[:4].data_ptr(), ff[:4].data_ptr(), g.data_ptr(), clip.y_k.data_ptr(), clip.y_v.data_ptr(), a.ak, a.av, a.alpha_dt, a.eps,
                               Q, 4, 6, 6, ca.D, 4, 3, 1.0 / math.sqrt(ca.D), got.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    # one plane alone: the other stream is read raw -- other contexts, and finite ones
    nv.multi_guide_local_adapt(fe[:4].data_ptr(), ff[:4].data_ptr(), g.data_ptr(), None, clip.y_v.data_ptr(), a.ak, a.av, a.alpha_dt, a.eps,
                               Q, 4, 6, 6, ca.D, 4, 3, 1.0 / math.sqrt(ca.D), got.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()) and not torch.equal(got, want)


def test_the_c_entry_point_refuses_in_front_of_any_launch():
    """Argument checks on a real, filled block: none launches -- the stream's buffers, its state and the plan's planes are what they were."""
    key, Q = ca.T12, 4
    m = module(key)
    s = open_adapt(key, Q)
    push_all(s, key, (4,))
    torch.cuda.synchronize()
    plan = next(p for k, p in m.__dict__[STORE].items() if k[0] == Q and k[1] == 4)
    x, a = plan.args, plan.args.base
    bits = lambda t: t.view(torch.int32)                      # (the untouched part of `out` is uninitialised memory: compare bits, not values)
    out0, ml0, acc0, ws0 = bits(s.out).clone(), bits(s.state_ml).clone(), bits(s.state_acc).clone(), plan.ws.clone()
    L = nv.lib()
    cases_ = ((a, dict(t0=a.y_index0), EINVAL, "outside the positional tables"), (a, dict(state_ml_out=a.state_ml_in), EINVAL, "overlap"),
              (a, dict(ff=None), EINVAL, "NULL pointer"), (a, dict(Q=33), EUNSUP, "1 <= Q <= 32"),
              (x, dict(ky=None), EINVAL, "come together"), (x, dict(vy=x.vy + 8), EINVAL, "16-byte aligned planes"),
              (x, dict(adapt_ws_bytes=x.adapt_ws_bytes - 1), EINVAL, "workspace of"), (x, dict(alpha_dt=nv.DT_F16), EINVAL, "alpha dtype"))
    for block, over, code, needle in cases_:
        saved = {f: getattr(block, f) for f in over}
        try:
            for f, v in over.items():
                setattr(block, f, v)
            got = L.hicom_compressor_stream_push_multi_adapt(ctypes.byref(x))
            msg = L.hicom_last_error().decode()
            assert got == code and re.search(needle, msg), (over, got, msg)
        finally:
            for f, v in saved.items():
                setattr(block, f, v)
    torch.cuda.synchronize()
    assert torch.equal(bits(s.out), out0) and torch.equal(bits(s.state_ml), ml0) and torch.equal(bits(s.state_acc), acc0), "a refused call launched something"
    assert torch.equal(plan.ws, ws0), "a refused call wrote the plan's workspace"
    push_all(s, key, (4, 4), t0=4)                            # the block still serves
    check("after the refusals vs oracle", finish(s), ca.oracle_guides(key, KV, Q))
