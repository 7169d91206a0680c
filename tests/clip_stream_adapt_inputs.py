"""Inputs and the float64 reference of the multi-guide clip stream on the k / v adaptor recipe (HIComProjector.open_stream_adapt,
hicom_amd/clip_stream.py: ClipStreamAdapt): ONE video pushed in chunks of whole window groups, Q guides, the adaptor MLPs run per chunk.

The clips and newline rows are those of tests/clip_stream_inputs.py (T = 12, 6 x 6, windows 4 x 3 x 3, GROUP_SCALES kept: the running
maximum of the global softmax rises when the second group of 4 frames arrives and not with the third).  The guides and their scales are those
of tests/clip_stream_multi_inputs.py; beyond its five guides (Q = 9: three groups of the adapt local kernel) the same law goes on, guide q
a synth guide of its own seed times 2, 4, 2, 4: neighbours still differ, the last guide and the first included (guide_swap hands guide 0
the set of the last guide; at equal scales it moved guide 0's global rows by 3.3 bars only).  The weights are the adaptkv state dict of
tests/many_item_inputs.py (alphas 0.5: half of an adapted key or value is LayerNorm of the MLP's output); a recipe with one adaptor loads
the part it has.

chunked_ref_adapt is the numpy float64 restatement of what the stream computes: tests/clip_stream_multi_inputs.py's chunked_ref_multi with the
adaptor blend in the local stage -- per chunk y_k = MLP_k(key tokens), y_v = MLP_v(frames_feature), key = (1 - a_k) x + a_k LN_k(y_k) and the
values likewise, the window softmax of every guide over the blended rows.  The global stage reads the raw tokens.  `mutant` switches on
the faults of chunked_ref_multi (all eight) and those a per-chunk adaptor stage can have:

  prev_planes      from the second push on the y planes read are those the PREVIOUS push wrote (token n of the chunk reads row n mod N_prev)
  planes_swapped   the key blend reads the value stream's plane and the value blend the key stream's
  blend_late_off   the blend is skipped from the second push on (raw keys and values, as the plain recipe)
  key_from_ff      the k adaptor's MLP reads frames_feature although frames_embed was given (the raw half of the key is still frames_embed)

tests/test_clip_stream_adapt_power.py holds chunked_ref_adapt to oracle.projector_forward per guide on the concatenation and shows that every
mutant moves every (guide, region) it can touch by >= 4 bars of the GPU test; tests/test_gpu_clip_stream_adapt.py takes its cases from here."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import clip_stream_inputs as ci
import clip_stream_multi_inputs as cm
import many_item_inputs as mi
from hicom_amd import geometry as geo
from hicom_amd import synth
from oracle import hicom_oracle as orc
from oracle_util import to_t

D, NG, KT, KS = ci.D, ci.NG, ci.KT, ci.KS
ADAPTKV, ADAPTK, ADAPTV = mi.ADAPTKV, mi.ADAPTK, mi.ADAPTV
ENTRY = mi.Entry("clip_stream_adapt", "adapt", (), "edge")           # the tolerance rule of many_item_inputs: the 1e-3 of `edge`
ADAPT_MUTANTS = ("prev_planes", "planes_swapped", "blend_late_off", "key_from_ff")
MUTANTS = cm.MUTANTS + ADAPT_MUTANTS
MAX_Q = 9

T12, T12_GRID, WIDE = ci.T12, ci.T12_GRID, ci.WIDE
T12_CHUNKINGS = ((4, 4, 4), (4, 8), (8, 4), (12,))
# (clip key, recipe, Q, with frames_embed, chunkings): the parity cases of the GPU test
CASES = ([(k, ADAPTKV, Q, fe, T12_CHUNKINGS) for Q in (4, 5, 9) for k, fe in ((T12, True), (T12, False), (T12_GRID, True))]
         + [(T12, ADAPTK, 3, True, ((4, 8),)), (T12, ADAPTV, 3, True, ((4, 8),)), (WIDE, ADAPTKV, 2, True, ((4, 4),))])


def tolerance(want):
    """The bar of the GPU test for one guide's output `want` (the oracle's): max-abs, the same for both regions."""
    return mi.tolerance(ENTRY, want)


def guide_scale(q):
    return cm.GUIDE_SCALES[q] if q < len(cm.GUIDE_SCALES) else (2.0, 4.0)[(q - len(cm.GUIDE_SCALES)) % 2]


@functools.lru_cache(maxsize=None)
def guides(key, Q, second=False):
    """float32 [Q, D], exact in bf16; the first five are clip_stream_multi_inputs.guides.  second: another set of Q guides."""
    assert 1 <= Q <= MAX_Q
    tag = "guideB" if second else "guide"
    g = np.stack([synth.synth_inputs(1, 3, 3, D, tag=f"{ci.TAG}:multi:{tag}{q}")["g"] * np.float32(guide_scale(q)) for q in range(Q)])
    assert g.dtype == np.float32 and np.array_equal(synth.round_to_bf16(g), g)
    n = min(Q, len(cm.GUIDE_SCALES))
    assert np.array_equal(g[:n], cm.guides(key, n, second))
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def build(key, recipe=ADAPTKV):
    """The clip of clip_stream_inputs under the weights of many_item_inputs' adaptor cases: cfg, sd, tokens, newline."""
    c = ci.build(key)
    cfg0, sd = mi._weights("adapt", recipe, c.hidden)
    cfg = SimpleNamespace(**{**vars(cfg0), "mm_newline_position": c.cfg.mm_newline_position})
    assert all(np.all(v == 0.5) for k, v in sd.items() if k.endswith("_alpha"))
    return SimpleNamespace(key=key, recipe=recipe, cfg=cfg, sd=sd, modal="video", newline=c.newline, ff=c.ff, fe=c.fe, T=c.T, h=c.h, w=c.w,
                           hidden=c.hidden, adapt_k=recipe in (ADAPTKV, ADAPTK), adapt_v=recipe in (ADAPTKV, ADAPTV))


@functools.lru_cache(maxsize=None)
def oracle_guides(key, recipe, Q, with_fe=True, frames=None, second=False, dtype=torch.float32):
    """oracle.projector_forward per guide on the clip's first `frames` frames (all by default): [Q, rows, hidden]; read-only."""
    c = build(key, recipe)
    sd = {k: to_t(v, dtype) for k, v in c.sd.items()}
    n = c.T if frames is None else frames
    fe = c.fe[:n] if with_fe else None
    out = np.stack([orc.projector_forward(c.cfg, sd, to_t(c.ff[:n], dtype), to_t(fe, dtype), to_t(g, dtype), "video", to_t(c.newline, dtype)).numpy()
                    for g in guides(key, Q, second)])
    out.setflags(write=False)
    return out


region_errors = cm.region_errors


def top_guides(Q):
    """The guides with the largest scale (more than one from Q = 7 on)."""
    s = [guide_scale(q) for q in range(Q)]
    return {q for q in range(Q) if s[q] == max(s)}


def touches(mutant, chunking, Q, with_fe=True):
    """The (guide, region) pairs `mutant` can touch when the clip is pushed as `chunking` for Q > 1 guides under the adaptkv recipe.  The
    eight mutants of clip_stream_multi_inputs as there (shared_max: every guide but those of the largest scale).  The adaptor mutants
    touch the local rows of every guide: prev_planes and blend_late_off from the second push on, planes_swapped always, key_from_ff when
    frames_embed is given."""
    assert Q > 1
    local = {(q, "local") for q in range(Q)}
    if mutant in ("prev_planes", "blend_late_off"):
        return local if len(chunking) > 1 else set()
    if mutant == "planes_swapped":
        return local
    if mutant == "key_from_ff":
        return local if with_fe else set()
    if mutant == "shared_max":
        return {(q, "global") for q in range(Q) if q not in top_guides(Q)} if len(chunking) > 1 else set()
    return {(q, r) for q in range(Q) for r in ci.touches(mutant, chunking)} if mutant in ci.MUTANTS else cm.touches(mutant, chunking, Q)


def uncounted(mutant, chunking, Q):
    """(guide, region) pairs a mutant may move without `touches` counting on it.  shared_max: the guides of the largest scale.  no_rescale
    under a chunking whose later chunks hold no larger group than an earlier one ((8, 4)): the groups' scales order the running maxima
    of most heads, not of all of them under these weights (a head's largest logit may still sit in the third group: guide 2 moves by
    2e-4), so nothing is counted on there and nothing is forbidden."""
    if mutant == "shared_max" and len(chunking) > 1:
        return {(q, "global") for q in top_guides(Q)}
    if mutant == "no_rescale" and len(chunking) > 1 and not ci.touches(mutant, chunking):
        return {(q, "global") for q in range(Q)}
    return set()


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------------
def _layer_norm(y, sd, p):
    mu = y.mean(axis=-1, keepdims=True)
    var = ((y - mu) ** 2).mean(axis=-1, keepdims=True)
    return (y - mu) / np.sqrt(var + orc.LN_EPS) * ci._f64(sd[p + ".weight"]) + ci._f64(sd[p + ".bias"])


@functools.lru_cache(maxsize=64)
def _plane(key, recipe, stream, source, t0, Tc):
    """y = MLP_stream(x) float64 [Tc h w, D] of the chunk's tokens x = the clip's `source` ("ff" / "fe") frames t0 .. t0 + Tc."""
    c = build(key, recipe)
    x = ci._f64(getattr(c, source)[t0:t0 + Tc]).reshape(-1, D)
    y = ci._mlp(x, c.sd, f"local_compressor.{stream}_proj")
    y.setflags(write=False)
    return y


def _blend(c, stream, x, y):
    a = float(c.sd[f"local_compressor.{stream}_alpha"][0])
    return (1.0 - a) * x + a * _layer_norm(y, c.sd, f"local_compressor.{stream}_norm").reshape(x.shape)


def _window_rows(c, key_t, val_t, g):
    """Readout rows [windows, hidden] of one chunk from its (blended) key and value tokens [Tc, h, w, D], window order (t1, h1, w1)."""
    Tc, h, w, _ = val_t.shape

    def win(x):
        x = x.reshape(Tc // KT, KT, h // KS, KS, w // KS, KS, D).transpose(0, 2, 4, 1, 3, 5, 6)
        return x.reshape(-1, KT * KS * KS, D)
    kw, vw = win(key_t), win(val_t)
    s = kw @ g / np.sqrt(D)
    p = np.exp(s - s.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    return ci._mlp(np.einsum("nk,nkd->nd", p, vw), c.sd, "local_compressor.readout")


def chunked_ref_adapt(key, chunking, Q, recipe=ADAPTKV, mutant=None, with_fe=True, second=False):
    """float64 [Q, local rows + 32, hidden]: the clip pushed as `chunking` (frames per push) for Q guides under `recipe`, then finish()."""
    assert mutant is None or mutant in MUTANTS
    assert mutant not in ADAPT_MUTANTS or recipe == ADAPTKV
    f64 = ci._f64
    c = build(key, recipe)
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
    key_src = "fe" if with_fe else "ff"
    t0, prev = 0, None
    for i, Tc in enumerate(chunking):
        ff, fe = f64(c.ff[t0:t0 + Tc]), f64(getattr(c, key_src)[t0:t0 + Tc])
        # the local stage: the adaptor MLPs over the chunk's tokens, the blend, every guide's windows
        yk = _plane(key, recipe, "k", "ff" if mutant == "key_from_ff" else key_src, t0, Tc) if c.adapt_k else None
        yv = _plane(key, recipe, "v", "ff", t0, Tc) if c.adapt_v else None
        planes = (yk, yv)
        if mutant == "prev_planes" and prev is not None:
            n = np.arange(Tc * h * w)
            yk, yv = (p[n % p.shape[0]] for p in prev)
        prev = planes
        if mutant == "planes_swapped":
            yk, yv = yv, yk
        off = mutant == "blend_late_off" and i > 0
        key_t = _blend(c, "k", fe, yk) if c.adapt_k and not off else fe
        val_t = _blend(c, "v", ff, yv) if c.adapt_v and not off else ff
        m0 = 0 if mutant == "rows_at_zero" else (t0 // KT) * (h // KS) * (w // KS)
        for q in range(Q):
            plane = 0 if mutant == "plane_zero" else q
            for j, row in enumerate(_window_rows(c, key_t, val_t, G[q])):
                out[plane, lay.row_of(m0 + j)] = row
        # the global stage on the raw tokens: the chunk's ONE un-normalised set per guide and head, absolute frame numbers
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
