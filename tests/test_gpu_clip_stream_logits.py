"""The logits form of the three clip stream pushes on the GPU: ClipStream, ClipStreamMulti and ClipStreamGroupMulti pushed
with local_logits in the place of frames_embed.

Inputs: the clip family of tests/clip_stream_inputs.py at E 1152, hidden 128, 6 x 6 (2 x 2 windows of 3 x 3 per window group, kt = 4), with
and without image_newline (`grid`); the guides of tests/clip_stream_multi_inputs.py.  The logits are exact: frames_embed . guide in float64
from the bf16 frames_embed, rounded to fp32 once, so both forms see the same scores up to rounding.  A chunk's logits are a VIEW of the
whole clip's [Q, T, H, W] tensor: the planes lie T H W floats apart, more than the chunk's Tc H W, and the chunk's first token is not the
tensor's first -- an absolute token index or a plane stride of Tc H W reads other cells.  The group's logits have NaN in every plane
q >= Q_i of an item's tokens and 30 000 in a gap behind the stack's tokens.

Bars.  ClipStreamMulti: local rows bit-equal to forward_multi_guide(local_logits=) on the concatenation, global rows bit-equal to the keyed
stream.  ClipStream: global rows bit-equal to the keyed stream; local rows within 2e-3 of forward(local_logits=) (the bar
tests/test_gpu_clip_stream.py holds keyed pushes to against forward()) and the whole output within 1e-3 of the oracle per region.
ClipStreamGroupMulti: every push's views bit-equal to forward_ragged_multi_guide(local_logits=)'s local rows, finish_many's global rows
bit-equal to a keyed group's, every slot's local rows bit-equal to ClipStreamMulti with logits on the slot's chunks.  End to end with a
small head (inter 200): head_scores + push(local_logits=) against siglip_head_embed + push(frames_embed), each against the float64 head
and the oracle on the concatenation; the new pipeline's largest error may be at most twice the parent's (the rule of DESIGN.md §3.18).
The same for one tick of the group with its slots out of order: g.head_scores leaves the planes q >= Q_i of an item uninitialised, as the
ragged scores kernel does."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import clip_stream_inputs as ci
import clip_stream_multi_inputs as cm
from gpu_util import DEV, build_module, dev_bf16
from hicom_amd import clip_stream as cs
from hicom_amd import clip_stream_group_multi as cgm
from hicom_amd import native as nv
from host_util import EINVAL
from ops_reference import up
from stream_blocks import group_multi_push_block, multi_push_block, single_push_block
from test_gpu_head_scores import SmallHead, head_fp64          # (as tests/test_gpu_ragged_multi_guide_logits.py takes them)

pytestmark = pytest.mark.gpu
NAN = float("nan")
NG = ci.NG
H = W = 6
HW = H * W
HIDDEN = 128
T16 = (16, 6, 6, HIDDEN, None)
T16_GRID = (16, 6, 6, HIDDEN, "grid")
T24 = (24, 6, 6, HIDDEN, None)
T24_GRID = (24, 6, 6, HIDDEN, "grid")
KEYS = [T16, T16_GRID]
CHUNKINGS = [(4, 8, 4), (8, 4)]
QS = [1, 3, 5]
TOL_FORWARD = 2 * ci.TOL            # tests/test_gpu_clip_stream.py: a keyed stream against forward() on the concatenation
COUNTS = (3, 1, 5)                  # the group: guides per slot
TICKS = (((2, 0), (8, 4)), ((1, 2, 0), (4, 4, 8)))          # (slots, chunk lengths) per tick: out of order, slot 1 absent from the first
kid = lambda k: f"T{k[0]}_{k[4] or 'plain'}"


@functools.lru_cache(maxsize=None)
def module(key):
    return build_module(ci.build(key))


@functools.lru_cache(maxsize=None)
def clip(key):
    c = ci.build(key)
    return dev_bf16(c.ff), dev_bf16(c.fe), dev_bf16(c.newline)


@functools.lru_cache(maxsize=None)
def guides9(key):
    """bf16 [9, D] on the device: the five guides of clip_stream_multi_inputs and four of its second set."""
    return dev_bf16(np.concatenate([cm.guides(key, 5), cm.guides(key, 5, True)])[:9])


def exact_logits(fe, g):
    """fp32 [Q, T, H, W]: frames_embed . g_q in float64, rounded once."""
    return torch.einsum("thwd,qd->qthw", up(fe.cpu()), up(g.cpu())).float().to(DEV)


def chunks_of(chunking):
    t0 = 0
    for n in chunking:
        yield t0, n
        t0 += n


# =============================================================================================================================
# ClipStreamMulti
# =============================================================================================================================
@pytest.mark.parametrize("chunking", CHUNKINGS, ids=lambda c: "+".join(map(str, c)))
@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("key", KEYS, ids=kid)
def test_multi_stream_with_logits_is_the_resident_logits_step_and_the_keyed_stream(key, Q, chunking):
    m = module(key)
    ff, fe, nl = clip(key)
    T = sum(chunking)
    g = guides9(key)[:Q].contiguous()
    L = exact_logits(fe[:T], g)
    with torch.no_grad():
        s, keyed = m.open_stream_multi(g, H, W, 16, nl), m.open_stream_multi(g, H, W, 16, nl)
        for t0, n in chunks_of(chunking):
            view = s.push(ff[t0:t0 + n], None, local_logits=L[:, t0:t0 + n])
            keyed.push(ff[t0:t0 + n], fe[t0:t0 + n])
            assert view.shape[0] == Q
        out, want_keyed = s.finish(), keyed.finish()
        whole = m.forward_multi_guide(ff[:T], None, g, "video", nl, local_logits=L)
    torch.cuda.synchronize()
    assert out.shape == whole.shape == want_keyed.shape and s.has_logits and s.has_fe is False
    assert torch.equal(out[:, :-NG], whole[:, :-NG]), "the local rows differ from forward_multi_guide(local_logits=) on the concatenation"
    assert torch.equal(out[:, -NG:], want_keyed[:, -NG:]), "the global rows differ from the keyed stream's"
    e = float((out[:, :-NG] - want_keyed[:, :-NG]).abs().max())
    print(f"CLIPSTREAM_LOGITS multi {kid(key)} Q={Q} {chunking}: local rows vs the keyed stream {e:.3e}")
    assert e <= TOL_FORWARD
    plans = m.__dict__[cs.STORE_MULTI]
    assert any(k[-1] == "logits" for k in plans) and any(k[-1] != "logits" for k in plans)


# =============================================================================================================================
# ClipStream
# =============================================================================================================================
@pytest.mark.parametrize("chunking", CHUNKINGS, ids=lambda c: "+".join(map(str, c)))
@pytest.mark.parametrize("key", KEYS, ids=kid)
def test_single_stream_with_logits_against_the_keyed_stream_forward_and_the_oracle(key, chunking):
    c = ci.build(key)
    m = module(key)
    ff, fe, nl = clip(key)
    T = sum(chunking)
    g = dev_bf16(c.g)
    L = exact_logits(fe[:T], g.view(1, -1))[0]
    with torch.no_grad():
        s, keyed = m.open_stream(g, H, W, 16, nl), m.open_stream(g, H, W, 16, nl)
        for t0, n in chunks_of(chunking):
            s.push(ff[t0:t0 + n], None, local_logits=L[t0:t0 + n])
            keyed.push(ff[t0:t0 + n], fe[t0:t0 + n])
        out, want_keyed = s.finish(), keyed.finish()
        whole = m(ff[:T], None, g, "video", nl, local_logits=L)
    torch.cuda.synchronize()
    assert torch.equal(out[-NG:], want_keyed[-NG:]), "the global rows differ from the keyed stream's"
    e_fwd = float((out[:-NG] - whole[:-NG]).abs().max())
    errs = ci.region_errors(out.float().cpu().numpy(), ci.oracle_output(key, True, frames=T))
    print(f"CLIPSTREAM_LOGITS single {kid(key)} {chunking}: local rows vs forward(local_logits=) {e_fwd:.3e}; vs the oracle local {errs['local']:.3e} "
          f"global {errs['global']:.3e}")
    assert e_fwd <= TOL_FORWARD
    assert errs["local"] <= ci.TOL and errs["global"] <= ci.TOL


# =============================================================================================================================
# ClipStreamGroupMulti
# =============================================================================================================================
def slot_frames(slot, t0, n):
    """Slot s follows the clip from frame 4 s on: the frames [t0, t0 + n) of its own clip."""
    return slice(4 * slot + t0, 4 * slot + t0 + n)


def tick_inputs(key, g, slots, sizes, frames, gap=0):
    """(stacked ff, stacked fe, gathered guides, counts, logits [q_max, sum Tc, H, W]): NaN in the planes q >= Q_i of an item's tokens; the
    planes lie sum N_i + gap floats apart with 30 000 in the gap."""
    ff, fe, _ = clip(key)
    pair0 = [sum(COUNTS[:s]) for s in range(len(COUNTS))]
    parts = [slot_frames(s, frames[s], n) for s, n in zip(slots, sizes)]
    sff, sfe = torch.cat([ff[p] for p in parts]), torch.cat([fe[p] for p in parts])
    counts = [COUNTS[s] for s in slots]
    gathered = torch.cat([g[pair0[s]:pair0[s] + COUNTS[s]] for s in slots])
    N = sum(sizes) * HW
    buf = torch.full((max(counts), N + gap), 30000.0, dtype=torch.float32, device=DEV)
    L = buf[:, :N].view(max(counts), sum(sizes), H, W)
    L.fill_(NAN)
    t = 0
    for s, n in zip(slots, sizes):
        L[:COUNTS[s], t:t + n] = exact_logits(sfe[t:t + n], g[pair0[s]:pair0[s] + COUNTS[s]])
        t += n
    return sff, sfe, gathered, counts, L


@pytest.mark.parametrize("key", [T24, T24_GRID], ids=kid)
def test_group_with_logits_is_the_ragged_logits_step_the_keyed_group_and_the_multi_stream(key):
    m = module(key)
    _, _, nl = clip(key)
    g = guides9(key)
    B = len(COUNTS)
    with torch.no_grad():
        grp = m.open_stream_group_multi(g, COUNTS, H, W, 16, nl)
        keyed = m.open_stream_group_multi(g, COUNTS, H, W, 16, nl)
        singles = [m.open_stream_multi(g[sum(COUNTS[:s]):sum(COUNTS[:s + 1])].contiguous(), H, W, 16, nl) for s in range(B)]
        frames = [0] * B
        for slots, sizes in TICKS:
            sff, sfe, gathered, counts, L = tick_inputs(key, g, slots, sizes, frames, gap=7)
            views = [v.clone() for v in grp.push(sff, None, sizes, list(slots), local_logits=L)]
            keyed.push(sff, sfe, sizes, list(slots))
            clean = torch.nan_to_num(L, nan=0.0).contiguous()                # (forward_ragged_multi_guide does not read those planes either)
            want = m.forward_ragged_multi_guide(sff, None, gathered, sizes, counts, "video", nl, local_logits=clean)
            t = 0
            for i, (s, n) in enumerate(zip(slots, sizes)):
                assert views[i].shape == want[i][:, :-NG].shape, (views[i].shape, want[i].shape)
                assert bool(torch.isfinite(views[i]).all()), f"slot {s}: an unread plane reached the output"
                assert torch.equal(views[i], want[i][:, :-NG]), f"tick {slots}: item {i} differs from forward_ragged_multi_guide(local_logits=)"
                singles[s].push(sff[t:t + n], None, local_logits=L[:COUNTS[s], t:t + n])
                frames[s] += n
                t += n
        outs, want_keyed = grp.finish_many(), keyed.finish_many()
        solo = [s.finish() for s in singles]
    torch.cuda.synchronize()
    assert grp.has_logits == [True] * B and grp.has_fe == [False] * B
    for s in range(B):
        assert torch.equal(outs[s][:, -NG:], want_keyed[s][:, -NG:]), f"slot {s}: the global rows differ from the keyed group's"
        assert torch.equal(outs[s][:, :-NG], solo[s][:, :-NG]), f"slot {s}: the local rows differ from ClipStreamMulti with logits"
        e = float((outs[s][:, -NG:] - solo[s][:, -NG:]).abs().max())
        assert e <= TOL_FORWARD, (s, e)


# =============================================================================================================================
# guards
# =============================================================================================================================
def test_the_gap_behind_a_plane_and_a_stale_frames_embed_are_not_read(monkeypatch):
    key = T16_GRID
    m = module(key)
    ff, fe, nl = clip(key)
    g = guides9(key)[:5].contiguous()
    L = exact_logits(fe, g)
    poison = torch.full((8 * HW * ci.D + 8,), NAN, dtype=torch.bfloat16, device=DEV)
    stale = poison.data_ptr() + 2                                            # valid memory full of NaN, not 16-byte aligned

    def run(gap, poisoned):
        with monkeypatch.context() as mp:
            if poisoned:                                                     # the block keeps an fe address, as after a keyed push
                for name in ("compressor_stream_push_multi_logits", "compressor_stream_push_logits"):
                    real = getattr(nv, name)
                    mp.setattr(nv, name, lambda a, *rest, real=real: (setattr(a, "fe", stale), real(a, *rest))[1])
            with torch.no_grad():
                s, one = m.open_stream_multi(g, H, W, 16, nl), m.open_stream(g[2], H, W, 16, nl)
                for t0, n in chunks_of((4, 8, 4)):
                    buf = torch.full((5, n * HW + gap), 30000.0, dtype=torch.float32, device=DEV)
                    Lc = buf[:, :n * HW].view(5, n, H, W)
                    Lc.copy_(L[:, t0:t0 + n])
                    s.push(ff[t0:t0 + n], None, local_logits=Lc)
                    one.push(ff[t0:t0 + n], None, local_logits=Lc[2])
                return s.finish().clone(), one.finish().clone()
    base = run(0, False)
    for gap, poisoned in ((5, False), (0, True)):
        got = run(gap, poisoned)
        torch.cuda.synchronize()
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), (gap, poisoned)
    assert bool(torch.isfinite(base[0]).all()) and bool(torch.isfinite(base[1]).all())


def test_group_a_stale_frames_embed_is_not_read(monkeypatch):
    key = T24
    m = module(key)
    g = guides9(key)
    slots, sizes = TICKS[0]
    sff, _, _, _, L = tick_inputs(key, g, slots, sizes, [0, 0, 0])
    poison = torch.full((sff.numel() + 8,), NAN, dtype=torch.bfloat16, device=DEV)
    outs = []
    for poisoned in (False, True):
        with monkeypatch.context() as mp:
            if poisoned:
                real = nv.compressor_stream_group_multi_push_logits
                mp.setattr(nv, "compressor_stream_group_multi_push_logits", lambda a, *rest: (setattr(a, "fe", poison.data_ptr() + 2), real(a, *rest))[1])
            with torch.no_grad():
                grp = m.open_stream_group_multi(g, COUNTS, H, W, 16, None)
                grp.push(sff, None, sizes, list(slots), local_logits=L)
                outs.append({s: o.clone() for s, o in grp.finish_many().items()})
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0][s], outs[1][s]) and bool(torch.isfinite(outs[0][s]).all()) for s in outs[0])


# =============================================================================================================================
# end to end with the head
# =============================================================================================================================
@pytest.mark.parametrize("Q", [1, 3])
def test_end_to_end_with_the_head_against_the_parent_pipeline(Q):
    from hicom_amd import siglip_head_embed
    from oracle import hicom_oracle as orc
    key = T16
    c = ci.build(key)
    m = module(key)
    head = SmallHead().to(torch.bfloat16).to(DEV).eval()
    x = clip(key)[0][:12]                                                    # the tower's output: frames_feature itself
    g = guides9(key)[:Q].contiguous()
    multi = Q > 1
    with torch.no_grad():
        opener = (lambda: m.open_stream_multi(g, H, W, 16, None)) if multi else (lambda: m.open_stream(g[0], H, W, 16, None))
        new, old = opener(), opener()
        for t0, n in chunks_of((4, 8)):
            xc = x[t0:t0 + n]
            new.push(xc, None, local_logits=new.head_scores(xc, head))
            old.push(xc, siglip_head_embed(xc, head))
        got_new, got_old = new.finish().float().cpu(), old.finish().float().cpu()
    torch.cuda.synchronize()
    fe64 = head_fp64(x, head)
    sd = {k: torch.from_numpy(np.asarray(v)).double() for k, v in c.sd.items()}
    want = torch.stack([orc.projector_forward(c.cfg, sd, up(x.cpu()), fe64, up(g[q].cpu()), "video", None) for q in range(Q)])
    if not multi:
        got_new, got_old = got_new[None], got_old[None]
    e_new, e_old = float((got_new.double() - want).abs().max()), float((got_old.double() - want).abs().max())
    print(f"CLIPSTREAM_LOGITS end-to-end Q={Q}: max-abs vs the float64 head + oracle: head_scores + push(local_logits=) {e_new:.3e}, "
          f"siglip_head_embed + push(frames_embed) {e_old:.3e}")
    assert e_new <= 2 * e_old, (e_new, e_old)


def test_group_end_to_end_with_the_head_against_the_parent_pipeline():
    from hicom_amd import siglip_head_embed
    from oracle import hicom_oracle as orc
    key = T24
    c = ci.build(key)
    m = module(key)
    head = SmallHead().to(torch.bfloat16).to(DEV).eval()
    g = guides9(key)
    slots, sizes = TICKS[0]
    x = tick_inputs(key, g, slots, sizes, [0, 0, 0])[0]                       # the tower's output: the stacked frames_feature itself
    with torch.no_grad():
        new, old = (m.open_stream_group_multi(g, COUNTS, H, W, 16, None) for _ in range(2))
        L = new.head_scores(x, head, sizes, list(slots))
        assert L.dtype == torch.float32 and tuple(L.shape) == (max(COUNTS[s] for s in slots), sum(sizes), H, W)
        new.push(x, None, sizes, list(slots), local_logits=L)
        old.push(x, siglip_head_embed(x, head), sizes, list(slots))
        got_new, got_old = new.finish_many(), old.finish_many()
    torch.cuda.synchronize()
    fe64 = head_fp64(x, head)
    sd = {k: torch.from_numpy(np.asarray(v)).double() for k, v in c.sd.items()}
    t = 0
    for s, n in zip(slots, sizes):
        p0 = sum(COUNTS[:s])
        want = torch.stack([orc.projector_forward(c.cfg, sd, up(x[t:t + n].cpu()), fe64[t:t + n], up(g[p0 + q].cpu()), "video", None) for q in range(COUNTS[s])])
        e_new = float((got_new[s].double().cpu() - want).abs().max())
        e_old = float((got_old[s].double().cpu() - want).abs().max())
        print(f"CLIPSTREAM_LOGITS end-to-end group slot {s} (Q={COUNTS[s]}, {n} frames): max-abs vs the float64 head + oracle: g.head_scores + push(local_logits=) "
              f"{e_new:.3e}, siglip_head_embed + push(frames_embed) {e_old:.3e}")
        assert bool(torch.isfinite(got_new[s]).all()) and e_new <= 2 * e_old, (s, e_new, e_old)
        t += n


# =============================================================================================================================
# the C entries
# =============================================================================================================================
def test_c_entries_refuse_null_logits_and_a_short_stride_without_launching():
    L = nv.lib()
    addr = torch.zeros(16, device=DEV).data_ptr()
    calls = (("compressor_stream_push_logits", lambda ll, qs: L.hicom_compressor_stream_push_logits(ctypes.byref(single_push_block()), ll), False),
             ("compressor_stream_push_multi_logits", lambda ll, qs: L.hicom_compressor_stream_push_multi_logits(ctypes.byref(multi_push_block()), ll, qs), 143),
             ("compressor_stream_group_multi_push_logits",
              lambda ll, qs: L.hicom_compressor_stream_group_multi_push_logits(ctypes.byref(group_multi_push_block()), ll, qs), 16 * 36 - 1))
    for who, call, short in calls:
        assert call(None, 1 << 20) == EINVAL
        msg = L.hicom_last_error().decode()
        assert msg.startswith(who + ": ") and "local_logits" in msg, msg
        assert call(addr + 2, 1 << 20) == EINVAL and L.hicom_last_error().decode().startswith(who + ": ")
        if short:
            assert call(addr, short) == EINVAL
            msg = L.hicom_last_error().decode()
            assert msg.startswith(who + ": ") and f"q_stride={short}" in msg, msg
    assert L.hicom_compressor_stream_push_logits(None, addr) == EINVAL and L.hicom_compressor_stream_push_multi_logits(None, addr, 144) == EINVAL
    assert L.hicom_compressor_stream_group_multi_push_logits(None, addr, 576) == EINVAL
    torch.cuda.synchronize()
