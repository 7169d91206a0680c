"""Inputs and the float64 reference of the clip stream (HIComProjector.open_stream, hicom_amd/clip_stream.py): a video pushed in chunks of
whole window groups, the global softmax state carried from chunk to chunk.

The input family.  `synth` tokens and weights (the golden cases' law), every group of kt = 4 frames times its own power of two (exact in
bf16): GROUP_SCALES, repeated along the clip.  A group's logits scale with its tokens, so the running maximum of the global softmax RISES
when the second group arrives and the third group's maximum stays BELOW it: pushed as (4, 4, 4) the carried state is rescaled in the second
push and the arriving partials in the third; as (4, 8) the second push raises the maximum, as (8, 4) it does not.  The clip does not depend
on the chunking, so one oracle run serves every chunking of a case.

chunked_ref is a numpy float64 restatement of what the stream computes -- per chunk the local windows and their readout rows at their packed
offset, the online-softmax carry (M, L, O) of the global stage with ABSOLUTE frame numbers in the positional term, then the finish chain --
with a `mutant` switch for the faults a chunked implementation can have:

  no_rescale      the carried state is not rescaled when the running maximum rises
  frame_restart   the chunk's frame index restarts at 0 (the positional term of every chunk is that of the clip's first frames)
  state_reset     the state is emptied at every push (the result is the last chunk's alone)
  l_last          L is taken from the last chunk only
  rows_at_zero    a chunk's local rows land at row 0

tests/test_clip_stream_power.py holds chunked_ref to oracle.projector_forward on the concatenation and shows that every mutant moves every
region it can touch by >= 4 bars of the GPU test; tests/test_gpu_clip_stream.py takes its cases from here."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

import cases
from global_stream_inputs import EPS23, TRANS
from hicom_amd import geometry as geo
from hicom_amd import synth
from oracle import hicom_oracle as orc
from oracle_util import to_t

D = cases.D
NG = 32
KT, KS = 4, 3
TOL = 1e-3                                   # the bar of forward() against the oracle (tests/test_gpu_parity.py), per region
GROUP_SCALES = (0.25, 1.0, 0.5)              # per group of KT frames: the running maximum rises in the second group and not in the third;
                                             # at most 1, so no value exceeds the flat law the 1e-3 bar of forward() was set under
MUTANTS = ("no_rescale", "frame_restart", "state_reset", "l_last", "rows_at_zero")
TAG = "clipstream"

# (T, h, w, hidden, newline position or None): the cases of the GPU test
T12 = (12, 6, 6, 64, None)
T12_GRID = (12, 6, 6, 64, "grid")
T4 = (4, 6, 6, 64, None)
WIDE = (8, 9, 9, 896, None)
CHUNKINGS = {T12: ((4, 4, 4), (4, 8), (8, 4), (12,)), T12_GRID: ((4, 4, 4), (12,)), T4: ((4,),), WIDE: ((4, 4),)}


@functools.lru_cache(maxsize=None)
def build(key):
    T, h, w, hidden, nlpos = key
    over = {"hidden_size": hidden}
    if nlpos is not None:
        over["mm_newline_position"] = nlpos
    cfg = SimpleNamespace(**{**cases.DEFAULT_CFG, **over})
    sd = synth.synth_state_dict(orc.param_shapes(cfg), tag=TAG)
    x = synth.synth_inputs(T, h, w, D, tag=f"{TAG}:clip")
    s = np.array([GROUP_SCALES[(t // KT) % len(GROUP_SCALES)] for t in range(T)], dtype=np.float32)[:, None, None, None]
    ff, fe = x["ff"] * s, x["fe"] * s
    for a in (ff, fe, x["g"]):
        assert np.array_equal(synth.round_to_bf16(a), a)
    nl = synth.normal_like((hidden,), synth.seed_of(f"{TAG}:newline")) if nlpos is not None else None
    g2 = synth.synth_inputs(1, 3, 3, D, tag=f"{TAG}:guide2")["g"]
    return SimpleNamespace(key=key, cfg=cfg, sd=sd, modal="video", newline=nl, ff=ff, fe=fe, g=x["g"], g2=g2, T=T, h=h, w=w, hidden=hidden)


@functools.lru_cache(maxsize=None)
def oracle_output(key, with_fe=True, frames=None, guide2=False, dtype=torch.float32):
    """oracle.projector_forward on the clip's first `frames` frames (all of them by default); callers must not write into it."""
    c = build(key)
    sd = {k: to_t(v, dtype) for k, v in c.sd.items()}
    n = c.T if frames is None else frames
    fe = c.fe[:n] if with_fe else None
    out = orc.projector_forward(c.cfg, sd, to_t(c.ff[:n], dtype), to_t(fe, dtype), to_t(c.g2 if guide2 else c.g, dtype), "video",
                                to_t(c.newline, dtype)).numpy()
    out.setflags(write=False)
    return out


def region_errors(got, want):
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    return {"local": float(d[:-NG].max()), "global": float(d[-NG:].max())}


def touches(mutant, chunking):
    """The regions `mutant` can touch when the clip is pushed as `chunking`.  One push: none.  no_rescale needs a later chunk that raises
    the running maximum: with GROUP_SCALES every chunking but one whose later chunks are all made of groups no larger than an earlier one."""
    if len(chunking) < 2:
        return ()
    if mutant == "rows_at_zero":
        return ("local",)
    if mutant == "no_rescale":
        top, t, rises = 0.0, 0, False
        for i, n in enumerate(chunking):
            m = max(GROUP_SCALES[(u // KT) % len(GROUP_SCALES)] for u in range(t, t + n))
            rises |= i > 0 and m > top
            top, t = max(top, m), t + n
        return ("global",) if rises else ()
    return ("global",)


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------------
def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(x / math.sqrt(2.0))).numpy())


def _mlp(x, sd, p):
    h = _gelu(x @ _f64(sd[p + ".0.weight"]).T + _f64(sd[p + ".0.bias"]))
    return h @ _f64(sd[p + ".2.weight"]).T + _f64(sd[p + ".2.bias"])


def _local_rows(c, ff, fe, g):
    """Readout rows [windows, hidden] of one chunk, window order (t1, h1, w1) (reference projector.py:544-559 with the guide as query)."""
    Tc, h, w, _ = ff.shape
    def win(x):
        x = x.reshape(Tc // KT, KT, h // KS, KS, w // KS, KS, D).transpose(0, 2, 4, 1, 3, 5, 6)
        return x.reshape(-1, KT * KS * KS, D)
    kw, vw = win(fe), win(ff)
    s = kw @ g / math.sqrt(D)
    p = np.exp(s - s.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    return _mlp(np.einsum("nk,nkd->nd", p, vw), c.sd, "local_compressor.readout")


def chunked_ref(key, chunking, with_fe=True, mutant=None, guide2=False):
    """float64 [local rows + 32, hidden]: the clip pushed as `chunking` (frames per push), then finish()."""
    assert mutant is None or mutant in MUTANTS
    c = build(key)
    sd, T, h, w = c.sd, sum(chunking), c.h, c.w
    g = _f64(c.g2 if guide2 else c.g)
    has_nl = c.newline is not None
    merge, nlpos = c.cfg.mm_patch_merge_type, c.cfg.mm_newline_position
    lay = geo.pack_layout(merge, nlpos, "video", T // KT, h // KS, w // KS, has_nl, False)
    out = np.zeros((lay.n_rows + NG, c.hidden))
    for r in lay.newline_rows:
        out[r] = _f64(c.newline)
    a = "global_compressor.attn_layer."
    Wq, bq, Wk, bk, Wv, bv, Wo, bo = (_f64(sd[a + n]) for n in ("q_proj.weight", "q_proj.bias", "k_proj.weight", "k_proj.bias", "v_proj.weight",
                                                              "v_proj.bias", "out_proj.weight", "out_proj.bias"))
    nh, hd = D // 128, 128
    qh = (Wq @ g + bq).reshape(nh, hd)
    pt, ph, pw = (orc.pos_axis_table(n, D) for n in (T, h, w))
    M, L, O = np.full(nh, -np.inf), np.zeros(nh), np.zeros((nh, hd))
    t0 = 0
    for Tc in chunking:
        ff, fe = _f64(c.ff[t0:t0 + Tc]), _f64(c.fe[t0:t0 + Tc] if with_fe else c.ff[t0:t0 + Tc])
        # local rows at the packed offset of the chunk's first window
        rows = _local_rows(c, ff, fe, g)
        m0 = 0 if mutant == "rows_at_zero" else (t0 // KT) * (h // KS) * (w // KS)
        for i, row in enumerate(rows):
            out[lay.row_of(m0 + i)] = row
        # global carry: absolute frame numbers in the positional term (the fp32 table of the reference, projector.py:95-99, :606)
        f0 = 0 if mutant == "frame_restart" else t0
        pos = (pt[f0:f0 + Tc, None, None, :] + ph[None, :, None, :] + pw[None, None, :, :]).astype(np.float32).astype(np.float64)
        x = (ff + pos).reshape(-1, D)
        k = (x @ Wk.T + bk).reshape(-1, nh, hd).transpose(1, 0, 2)
        v = (x @ Wv.T + bv).reshape(-1, nh, hd).transpose(1, 0, 2)
        s = np.einsum("hd,hnd->hn", qh, k) * hd ** -0.5
        if mutant == "state_reset":
            M, L, O = np.full(nh, -np.inf), np.zeros(nh), np.zeros((nh, hd))
        Mn = np.maximum(M, s.max(axis=1))
        alpha = np.ones(nh) if mutant == "no_rescale" else np.exp(M - Mn)
        p = np.exp(s - Mn[:, None])
        L = (0.0 if mutant == "l_last" else L * alpha) + p.sum(axis=1)
        O = O * alpha[:, None] + np.einsum("hn,hnd->hd", p, v)
        M = Mn
        t0 += Tc
    att = Wo @ (O / L[:, None]).reshape(D) + bo
    out[lay.n_rows:] = _mlp((g + att)[None], sd, "global_compressor.readout")
    return out


# ---- the fold kernel alone: float64 reference and bounds (tests/test_gpu_clip_stream.py has the derivation) ---------------------------------
def fold_ref(pm, pl, pacc, M, L, A):
    """float64 (M', L', ACC') and the bounds of L' and ACC' (module docstring)."""
    R = M.shape[0]
    nparts = pm.shape[0]
    m = np.concatenate([M[None].astype(np.float64), pm[:, :R].astype(np.float64)])            # [1 + nparts, R]
    l = np.concatenate([L[None].astype(np.float64), pl[:, :R].astype(np.float64)])
    a = np.concatenate([A[None].astype(np.float64), pacc[:, :R].astype(np.float64)])          # [1 + nparts, R, E]
    Mn = m.max(axis=0)
    with np.errstate(invalid="ignore"):
        w = np.where(np.isinf(m), 0.0, np.exp(m - Mn))
        arg = np.where(np.isinf(m), 0.0, np.abs(m - Mn))
    rel = (nparts + 8) * EPS23 + 2 * TRANS
    Ln, An = (w * l).sum(0), (w[..., None] * a).sum(0)
    l_tol = rel * (w * np.abs(l)).sum(0) + (w * EPS23 * arg * np.abs(l)).sum(0)
    a_tol = rel * (w[..., None] * np.abs(a)).sum(0) + ((w * EPS23 * arg)[..., None] * np.abs(a)).sum(0)
    return Mn, Ln, An, l_tol, a_tol
