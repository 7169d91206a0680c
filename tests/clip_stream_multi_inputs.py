"""Inputs and the float64 reference of the multi-guide clip stream (HIComProjector.open_stream_multi, hicom_amd/clip_stream.py): ONE video
pushed in chunks of whole window groups, Q guides, the global softmax state of all heads x Q folded rows carried from chunk to chunk.

The clips, weights and newline rows are those of tests/clip_stream_inputs.py (GROUP_SCALES kept: the running maximum of the global softmax
rises when the second group of 4 frames arrives and not with the third).  Guide q is a synth guide of its own seed times its own power of two
(GUIDE_SCALES, exact in bf16): a guide's logits scale with it, so the guides have different running maxima and meet different rescale
events, and a state that mixes the guides up -- rows, planes or maxima -- cannot pass for the right one.

chunked_ref_multi is the numpy float64 restatement of what the stream computes for Q guides: per chunk every guide's local rows at their packed
offset in the guide's own plane, per chunk ONE un-normalised set (m, l, o) per guide and head (the merge of the chunk), folded into the
carried (M, L, O) of that guide and head, then the finish chain per guide.  `mutant` switches on the faults a chunked multi-guide
implementation can have: the five of clip_stream_inputs (applied to every guide) and

  guide_swap      the chunk's set rows of guide q are folded into the state of guide q + 1 (cyclically)
  plane_zero      every guide's chunk rows land in plane 0 of the output (the last guide's rows survive there, the other planes stay empty)
  shared_max      ONE carried M per head, the largest over the guides, while every guide's (L, O) stay relative to its own maximum

tests/test_clip_stream_multi_power.py holds chunked_ref_multi to oracle.projector_forward per guide on the concatenation and shows that every
mutant moves every (guide, region) it can touch by >= 4 bars of the GPU test; tests/test_gpu_clip_stream_multi.py takes its cases from here."""
import functools

import numpy as np
import torch

import clip_stream_inputs as ci
from hicom_amd import geometry as geo
from hicom_amd import synth
from oracle import hicom_oracle as orc
from oracle_util import to_t

D, NG, KT, KS, TOL = ci.D, ci.NG, ci.KT, ci.KS, ci.TOL
GUIDE_SCALES = (1.0, 2.0, 4.0, 2.0, 1.0)      # guide q (a synth guide of its own seed) times GUIDE_SCALES[q]: powers of two between 1 and 4, the
                                              # range in which every mutant keeps its power on these clips (test_clip_stream_multi_power: at 0.5 and
                                              # below the softmax is too flat for no_rescale, from 8 up too sharp for state_reset and l_last);
                                              # neighbours differ, and the largest sits in the middle of the first local group
MUTANTS = ci.MUTANTS + ("guide_swap", "plane_zero", "shared_max")

# (clip key of clip_stream_inputs, Q, chunkings): the parity cases of the GPU test
T12, T12_GRID, WIDE = ci.T12, ci.T12_GRID, ci.WIDE
T12_CHUNKINGS = ((4, 4, 4), (4, 8), (8, 4), (12,))
CASES = [(T12, 3, T12_CHUNKINGS), (T12_GRID, 3, T12_CHUNKINGS), (T12, 5, T12_CHUNKINGS), (T12_GRID, 5, T12_CHUNKINGS), (WIDE, 2, ((4, 4),))]


@functools.lru_cache(maxsize=None)
def guides(key, Q, second=False):
    """float32 [Q, D], exact in bf16; second: another set of Q guides (reset with new guides, a replaced guide)."""
    assert 1 <= Q <= len(GUIDE_SCALES)
    tag = "guideB" if second else "guide"
    g = np.stack([synth.synth_inputs(1, 3, 3, D, tag=f"{ci.TAG}:multi:{tag}{q}")["g"] * np.float32(GUIDE_SCALES[q]) for q in range(Q)])
    assert g.dtype == np.float32 and np.array_equal(synth.round_to_bf16(g), g)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def oracle_guides(key, Q, with_fe=True, frames=None, second=False, dtype=torch.float32):
    """oracle.projector_forward per guide on the clip's first `frames` frames (all by default): [Q, rows, hidden]; read-only."""
    c = ci.build(key)
    sd = {k: to_t(v, dtype) for k, v in c.sd.items()}
    n = c.T if frames is None else frames
    fe = c.fe[:n] if with_fe else None
    out = np.stack([orc.projector_forward(c.cfg, sd, to_t(c.ff[:n], dtype), to_t(fe, dtype), to_t(g, dtype), "video", to_t(c.newline, dtype)).numpy()
                    for g in guides(key, Q, second)])
    out.setflags(write=False)
    return out


def region_errors(got, want):
    """{(guide, region): max-abs} for got / want [Q, rows, hidden]."""
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    errs = {}
    for q in range(d.shape[0]):
        errs[q, "local"], errs[q, "global"] = float(d[q, :-NG].max()), float(d[q, -NG:].max())
    return errs


def top_guide(Q):
    return int(np.argmax(GUIDE_SCALES[:Q]))


def touches(mutant, chunking, Q):
    """The (guide, region) pairs `mutant` can touch when the clip is pushed as `chunking` for Q > 1 guides.  The five single-guide mutants:
    clip_stream_inputs.touches, for every guide.  guide_swap and plane_zero need no second push.  shared_max needs a carried state, and a
    guide whose own maximum is below the shared one: counted on for every guide but the one with the largest scale, which holds the
    largest maximum in most heads (it still moves in the others: UNCOUNTED says so, and the power test asks nothing of it)."""
    assert Q > 1
    every = range(Q)
    if mutant == "guide_swap":
        return {(q, "global") for q in every}
    if mutant == "plane_zero":
        return {(q, "local") for q in every}
    if mutant == "shared_max":
        return {(q, "global") for q in every if q != top_guide(Q)} if len(chunking) > 1 else set()
    return {(q, r) for q in every for r in ci.touches(mutant, chunking)}


def uncounted(mutant, chunking, Q):
    """(guide, region) pairs a mutant may move without `touches` counting on it."""
    return {(top_guide(Q), "global")} if mutant == "shared_max" and len(chunking) > 1 else set()


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------------
def chunked_ref_multi(key, chunking, Q, mutant=None, with_fe=True, second=False):
    """float64 [Q, local rows + 32, hidden]: the clip pushed as `chunking` (frames per push) for Q guides, then finish()."""
    assert mutant is None or mutant in MUTANTS
    f64 = ci._f64
    c = ci.build(key)
    sd, T, h, w = c.sd, sum(chunking), c.h, c.w
    G = f64(guides(key, Q, second))
    has_nl = c.newline is not None
    lay = geo.pack_layout(c.cfg.mm_patch_merge_type, c.cfg.mm_newline_position, "video", T // KT, h // KS, w // KS, has_nl, False)
    out = np.zeros((Q, lay.n_rows + NG, c.hidden))
    for r in lay.newline_rows:
        out[:, r] = f64(c.newline)
    a = "global_compressor.attn_layer."
    Wq, bq, Wk, bk, Wv, bv, Wo, bo = (f64(sd[a + n]) for n in ("q_proj.weight", "q_proj.bias", "k_proj.weight", "k_proj.bias", "v_proj.weight",
                                                             "v_proj.bias", "out_proj.weight", "out_proj.bias"))
    nh, hd = D // 128, 128
    qh = (G @ Wq.T + bq).reshape(Q, nh, hd)
    pt, ph, pw = (orc.pos_axis_table(n, D) for n in (T, h, w))
    M, L, O = np.full((Q, nh), -np.inf), np.zeros((Q, nh)), np.zeros((Q, nh, hd))
    t0 = 0
    for Tc in chunking:
        ff, fe = f64(c.ff[t0:t0 + Tc]), f64(c.fe[t0:t0 + Tc] if with_fe else c.ff[t0:t0 + Tc])
        # every guide's local rows at the packed offset of the chunk's first window, in the guide's own plane
        m0 = 0 if mutant == "rows_at_zero" else (t0 // KT) * (h // KS) * (w // KS)
        for q in range(Q):
            plane = 0 if mutant == "plane_zero" else q
            for i, row in enumerate(ci._local_rows(c, ff, fe, G[q])):
                out[plane, lay.row_of(m0 + i)] = row
        # the chunk's ONE un-normalised set per guide and head, absolute frame numbers in the positional term
        f0 = 0 if mutant == "frame_restart" else t0
        pos = (pt[f0:f0 + Tc, None, None, :] + ph[None, :, None, :] + pw[None, None, :, :]).astype(np.float32).astype(np.float64)
        x = (ff + pos).reshape(-1, D)
        k = (x @ Wk.T + bk).reshape(-1, nh, hd).transpose(1, 0, 2)
        v = (x @ Wv.T + bv).reshape(-1, nh, hd).transpose(1, 0, 2)
        s = np.einsum("qhd,hnd->qhn", qh, k) * hd ** -0.5
        mc = s.max(axis=2)
        p = np.exp(s - mc[:, :, None])
        lc, oc = p.sum(axis=2), np.einsum("qhn,hnd->qhd", p, v)
        if mutant == "guide_swap":
            mc, lc, oc = (np.roll(z, 1, axis=0) for z in (mc, lc, oc))
        # the fold of the set into the carried state
        if mutant == "state_reset":
            M, L, O = np.full((Q, nh), -np.inf), np.zeros((Q, nh)), np.zeros((Q, nh, hd))
        Mn = np.maximum(M, mc)
        a_old = np.ones((Q, nh)) if mutant == "no_rescale" else np.exp(M - Mn)
        a_new = np.exp(mc - Mn)
        L = (0.0 if mutant == "l_last" else L * a_old) + lc * a_new
        O = O * a_old[:, :, None] + oc * a_new[:, :, None]
        M = Mn
        if mutant == "shared_max":
            M = np.broadcast_to(M.max(axis=0), M.shape).copy()
        t0 += Tc
    for q in range(Q):
        att = Wo @ (O[q] / L[q][:, None]).reshape(D) + bo
        out[q, lay.n_rows:] = ci._mlp((G[q] + att)[None], sd, "global_compressor.readout")
    return out
