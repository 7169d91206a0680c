"""Power of tests/test_gpu_clip_stream_logits.py (CPU, float64): a model of the chunked local stage that takes its scores
from a logits buffer exactly as the three pushes address it, with the faults such an addressing can have planted in it.

The model: per chunk (per item of a tick) and guide, logit of chunk-local token n = buffer[plane * q_stride + first + n]; softmax over each
window of 4 x 3 x 3 tokens at scale 1 / sqrt(D); context from the value rows; the readout MLP (clip_stream_inputs._local_rows with the
scores given).  The buffers are those of the GPU test: for a single video the whole clip's [Q, T H W] tensor of which a chunk is a view
(first = t0 H W, q_stride = T H W > Tc H W); for the group a [q_max, sum N_i + gap] buffer with the items one behind the other, a sentinel
in the planes q >= Q_i of an item's tokens (the GPU test has NaN there: any read of it is caught) and in the gap.

Faults:
  absolute_index     the chunk's token n is looked up at its index in the CLIP (t0 H W + n behind the chunk's first cell)
  plane_stride_tc    guide q's plane is taken Tc H W floats behind guide 0's where q_stride is larger
  pair_plane         (group) plane pair0_slot + q of item i instead of q
  tok0_previous      (group) the first token of the previous item
  plane_Q            (group) guide Q_i - 1 of an item with Q_i < q_max reads plane Q_i

The bars of the GPU test are bit-equality and, at the most, 2e-3 (ClipStream's local rows against forward()).  Every fault moves a local
row of EVERY case it applies to by at least 4 x 2e-3 (the smallest: absolute_index with one guide and the (8, 4) chunking, 1.1e-2 = 5.4 bars);
ClipStream (Q = 1), the one object whose bar is 2e-3 and not bit-equality, is held to the four bars on its own.  The unfaulted model agrees
with the keyed float64 reference to the rounding of the fp32 logits.  (A model of the addressing: it runs none of the package's code.)"""
import math

import numpy as np
import pytest

import clip_stream_inputs as ci
import clip_stream_multi_inputs as cm

D, KT, KS, H, W = ci.D, ci.KT, ci.KS, 6, 6
HW = H * W
KEY = (16, 6, 6, 128, None)                  # the single-video clip of the GPU test
KEY_GROUP = (24, 6, 6, 128, None)            # the group's: slot s follows it from frame 4 s on
BAR = 2e-3                                   # the widest bar of the GPU test (TOL_FORWARD)
SENTINEL = 30000.0
CHUNKINGS = [(4, 8, 4), (8, 4)]
QS = [1, 3, 5]
COUNTS = (3, 1, 5)
TICKS = (((2, 0), (8, 4)), ((1, 2, 0), (4, 4, 8)))
SINGLE_FAULTS = ("absolute_index", "plane_stride_tc")
GROUP_FAULTS = ("pair_plane", "tok0_previous", "plane_Q")


def guides9(key=KEY):
    return np.concatenate([cm.guides(key, 5), cm.guides(key, 5, True)])[:9].astype(np.float64)


def rows_from_scores(c, ff, s):
    """Readout rows [windows, hidden] of one chunk from its raw scores s [Tc H W] (chunk-local token order)."""
    Tc = ff.shape[0]

    def win(x, d):
        x = x.reshape(Tc // KT, KT, H // KS, KS, W // KS, KS, d).transpose(0, 2, 4, 1, 3, 5, 6)
        return x.reshape(-1, KT * KS * KS, d)
    sw = win(s.reshape(Tc, H, W, 1), 1)[..., 0] / math.sqrt(D)
    p = np.exp(sw - sw.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    return ci._mlp(np.einsum("nk,nkd->nd", p, win(ff, D)), c.sd, "local_compressor.readout")


def read(buf, idx):
    """buffer cells at flat indices; an index outside the allocation reads the sentinel (the device would read foreign memory)."""
    idx = np.asarray(idx)
    ok = (idx >= 0) & (idx < buf.size)
    return np.where(ok, buf[np.clip(idx, 0, buf.size - 1)], SENTINEL)


def exact(fe, g):
    """fp32-rounded float64 [Q, N]: frames_embed . g_q."""
    return (fe.reshape(-1, D).astype(np.float64) @ g.T).T.astype(np.float32).astype(np.float64)


# ---- one video in chunks: ClipStream (Q = 1) and ClipStreamMulti ------------------------------------------------------------------------------
def single_model(chunking, Q, fault=None):
    c = ci.build(KEY)
    T = sum(chunking)
    g = guides9()[:Q]
    buf = exact(c.fe[:T], g).reshape(-1)                         # [Q, T HW] flat
    n_tok, out, t0 = np.arange, [], 0
    for Tc in chunking:
        n = n_tok(Tc * HW)
        first = t0 * HW + (t0 * HW if fault == "absolute_index" else 0)
        stride = Tc * HW if fault == "plane_stride_tc" else T * HW
        out.append(np.stack([rows_from_scores(c, c.ff[t0:t0 + Tc].astype(np.float64), read(buf, q * stride + first + n)) for q in range(Q)]))
        t0 += Tc
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("chunking", CHUNKINGS, ids=lambda c: "+".join(map(str, c)))
@pytest.mark.parametrize("Q", QS)
def test_single_video_model_and_its_faults(Q, chunking):
    c = ci.build(KEY)
    good = single_model(chunking, Q)
    t0, keyed = 0, []
    for Tc in chunking:
        keyed.append(np.stack([ci._local_rows(c, c.ff[t0:t0 + Tc].astype(np.float64), c.fe[t0:t0 + Tc].astype(np.float64), g) for g in guides9()[:Q]]))
        t0 += Tc
    assert np.abs(good - np.concatenate(keyed, axis=1)).max() <= 1e-5, "the model is not the keyed local stage"
    for fault in SINGLE_FAULTS:
        if fault == "plane_stride_tc" and Q == 1:
            continue                                            # one plane: its stride is never used
        move = np.abs(single_model(chunking, Q, fault) - good).max()
        print(f"CLIPSTREAM_LOGITS power Q={Q} {chunking} {fault}: moves a local row by {move:.3e} = {move / BAR:.1f} bars")
        assert move >= 4 * BAR, (fault, move)


def test_every_single_video_fault_has_four_bars_on_a_shape_of_the_gpu_test():
    # ClipStream (Q = 1) is the object whose bar is 2e-3: absolute_index has its four bars there; plane_stride_tc needs Q > 1
    moves = {("absolute_index", 1): max(np.abs(single_model(ch, 1, "absolute_index") - single_model(ch, 1)).max() for ch in CHUNKINGS)}
    for f in SINGLE_FAULTS:
        moves[f, "Q > 1"] = max(np.abs(single_model(ch, Q, f) - single_model(ch, Q)).max() for ch in CHUNKINGS for Q in QS if Q > 1)
    assert all(m >= 4 * BAR for m in moves.values()), moves
    assert any(len(ch) > 1 for ch in CHUNKINGS), "absolute_index needs a chunk with t0 > 0"
    assert any(Q > 1 for Q in QS) and all(Tc < sum(ch) for ch in CHUNKINGS for Tc in ch), "plane_stride_tc needs Q > 1 and Tc H W < q_stride"


# ---- the group: items of a tick one behind the other ------------------------------------------------------------------------------------------
def group_model(fault=None, gap=7):
    c = ci.build(KEY_GROUP)
    G = guides9(KEY_GROUP)
    pair0 = [sum(COUNTS[:s]) for s in range(len(COUNTS))]
    frames, out = [0] * len(COUNTS), []
    for slots, sizes in TICKS:
        N = sum(sizes) * HW
        q_max = max(COUNTS[s] for s in slots)
        buf = np.full((q_max, N + gap), SENTINEL)
        parts, tok0s, t = [], [], 0
        for s, n in zip(slots, sizes):
            sl = slice(4 * s + frames[s], 4 * s + frames[s] + n)
            buf[:COUNTS[s], t * HW:(t + n) * HW] = exact(c.fe[sl], G[pair0[s]:pair0[s] + COUNTS[s]])
            parts.append(sl)
            tok0s.append(t * HW)
            t += n
        flat, stride = buf.reshape(-1), N + gap
        for i, (s, n) in enumerate(zip(slots, sizes)):
            tok0 = tok0s[i - 1] if fault == "tok0_previous" and i > 0 else tok0s[i]
            rows = []
            for q in range(COUNTS[s]):
                plane = q
                if fault == "pair_plane":
                    plane = pair0[s] + q
                if fault == "plane_Q" and COUNTS[s] < q_max and q == COUNTS[s] - 1:
                    plane = COUNTS[s]
                rows.append(rows_from_scores(c, c.ff[parts[i]].astype(np.float64), read(flat, plane * stride + tok0 + np.arange(n * HW))))
            out.append(np.stack(rows))
            frames[s] += n
    return out


def test_group_model_and_its_faults():
    c = ci.build(KEY_GROUP)
    G = guides9(KEY_GROUP)
    good = group_model()
    assert all(np.isfinite(r).all() for r in good)
    # the unfaulted model is the keyed local stage of every item
    frames, k = [0] * len(COUNTS), 0
    for slots, sizes in TICKS:
        for s, n in zip(slots, sizes):
            sl = slice(4 * s + frames[s], 4 * s + frames[s] + n)
            p0 = sum(COUNTS[:s])
            want = np.stack([ci._local_rows(c, c.ff[sl].astype(np.float64), c.fe[sl].astype(np.float64), g) for g in G[p0:p0 + COUNTS[s]]])
            assert np.abs(good[k] - want).max() <= 1e-5, (slots, s)
            frames[s] += n
            k += 1
    for fault in GROUP_FAULTS:
        bad = group_model(fault)
        move = max(np.abs(b - a).max() for a, b in zip(good, bad))
        print(f"CLIPSTREAM_LOGITS power group {fault}: moves a local row by {move:.3e} = {move / BAR:.1f} bars")
        assert move >= 4 * BAR, (fault, move)


def test_every_group_fault_applies_to_the_ticks_of_the_gpu_test():
    pair0 = [sum(COUNTS[:s]) for s in range(len(COUNTS))]
    assert any(pair0[s] > 0 for slots, _ in TICKS for s in slots), "pair_plane needs an item whose slot does not own pair 0"
    assert all(len(slots) > 1 for slots, _ in TICKS), "tok0_previous needs a second item"
    assert any(COUNTS[s] < max(COUNTS[u] for u in slots) for slots, _ in TICKS for s in slots), "plane_Q needs an item with Q_i < q_max"
    assert any(set(range(len(COUNTS))) - set(slots) for slots, _ in TICKS) and any(len(set(sizes)) > 1 for _, sizes in TICKS)
