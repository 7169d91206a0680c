"""Inputs and the float64 reference of the clip stream group on the k / v adaptor recipe (HIComProjector.open_stream_group_adapt,
hicom_amd/clip_stream_group_adapt.py).

The clips, the guides and the schedule are those of tests/clip_stream_group_multi_inputs.py (per-slot clips with GROUP_SCALES rotated by the
slot, the guides `group_multi_guide{i}`, SCHEDULE) under the adaptkv weights of tests/many_item_inputs.py, alphas 0.5, as
tests/clip_stream_adapt_inputs.py takes them: B = 3 slots with COUNTS = (1, 2, 5) guides, a 6 x 6 grid, hidden 64, E = 1152, max_frames 16,
chunks of 4 and 8 frames.  Five guides: a full guide group of the adaptor window kernel (4) plus a remainder of 1, and 45 folded rows, a
second pass of the global stream.  The guides are scaled by GUIDE_SCALE (a power of two: exact in bf16): the window softmax then leans on a
few tokens, and a fault in the planes a window reads moves its local rows by more than 4 bars (tests/test_clip_stream_group_adapt_power.py).

adapt_ref is clip_stream_group_multi_inputs.multi_ref -- the schedule replayed in the device's row space -- with the adaptor blend in the
local stage: per PUSH y_k = MLP_k(key tokens) and y_v = MLP_v(frames_feature) over the stacked tokens of the call, an item's windows read the
rows of its own tokens; key = (1 - a_k) x + a_k LN_k(y_k), the values likewise.  The global stage reads the raw tokens.  `mutant`: the nine
faults of multi_ref and the faults a STACKED adaptor stage can have:

  plane_offset     an item reads the planes at the stack's first token (token n of the item reads plane row n of the stack)
  planes_swapped   the key blend reads the value stream's plane and the value blend the key stream's
  prev_planes      from the group's second push on the planes read are those the PREVIOUS push wrote (stack row n reads row n mod N_prev)
  blend_first_only the blend is skipped for every item but the first of a push (raw keys and values, as the plain recipe)
  key_from_ff      the k adaptor's MLP reads frames_feature although frames_embed was given (the raw half of the key is still frames_embed)

touches(mutant, schedule, counts) names the (finish, slot) whose pairs' local rows such a fault can move."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import clip_stream_adapt_inputs as ai
import clip_stream_group_multi_inputs as gm
import clip_stream_inputs as ci
import many_item_inputs as mi
from hicom_amd import geometry as geo
from hicom_amd import synth
from oracle import hicom_oracle as orc
from oracle_util import to_t

D, NG, KT, KS, NH = gm.D, gm.NG, gm.KT, gm.KS, gm.NH
ADAPTKV, ADAPTK, ADAPTV = mi.ADAPTKV, mi.ADAPTK, mi.ADAPTV
TOL = 1e-3                                   # against the oracle, per pair and region; 2 TOL against forward() (the project's bars for this recipe)
COUNTS = (1, 2, 5)
M = sum(COUNTS)
PAIR0 = tuple(sum(COUNTS[:s]) for s in range(len(COUNTS)))
GUIDE_SCALE = 4.0
ADAPT_MUTANTS = ("plane_offset", "planes_swapped", "prev_planes", "blend_first_only", "key_from_ff")
MUTANTS = gm.MUTANTS + ADAPT_MUTANTS
MAX_FRAMES = gm.MAX_FRAMES
G12, G12_GRID, G12_ONE, WIDE = gm.G12, gm.G12_GRID, gm.G12_ONE, gm.WIDE

# clip_stream_group_multi_inputs.SCHEDULE with the reset bringing the guides from index M on
SCHEDULE = tuple(("reset", op[1], M) if op[0] == "reset" else op for op in gm.SCHEDULE)
COUNTS_WIDE, SCHEDULE_WIDE = gm.COUNTS_WIDE, gm.SCHEDULE_WIDE
final_state = gm.final_state
_f64 = ci._f64


@functools.lru_cache(maxsize=None)
def build(key, recipe=ADAPTKV):
    """clip_stream_group_multi_inputs.build(key) under the adaptor weights: cfg, sd, per-slot clips gff / gfe, M + 2 guides mg."""
    c = gm.build(key)
    cfg0, sd = mi._weights("adapt", recipe, c.hidden)
    cfg = SimpleNamespace(**{**vars(cfg0), "mm_newline_position": c.cfg.mm_newline_position})
    assert all(np.all(v == 0.5) for k, v in sd.items() if k.endswith("_alpha"))
    mg = [synth.synth_inputs(1, 3, 3, D, tag=f"{ci.TAG}:group_multi_guide{i}")["g"] * np.float32(GUIDE_SCALE) for i in range(M + 2)]
    for a in mg:
        assert a.dtype == np.float32 and np.array_equal(synth.round_to_bf16(a), a)
    return SimpleNamespace(key=key, recipe=recipe, cfg=cfg, sd=sd, modal="video", newline=c.newline, gff=c.gff, gfe=c.gfe, mg=mg, h=c.h, w=c.w,
                           hidden=c.hidden, adapt_k=recipe in (ADAPTKV, ADAPTK), adapt_v=recipe in (ADAPTKV, ADAPTV))


def plain_state_dict(c):
    """The weights of `c` without the adaptors: a plain-recipe module with the same local readout and global stage."""
    return {k: v for k, v in c.sd.items() if not any(k.startswith(f"local_compressor.{s}_") for s in ("k", "v"))}


@functools.lru_cache(maxsize=None)
def oracle_output(key, recipe, slot, frames, guide, with_fe=True, dtype=torch.float32):
    """oracle.projector_forward on the first `frames` frames of slot `slot`'s clip with guide mg[guide]; callers must not write into it."""
    c = build(key, recipe)
    sd = {k: to_t(v, dtype) for k, v in c.sd.items()}
    fe = c.gfe[slot][:frames] if with_fe else None
    out = orc.projector_forward(c.cfg, sd, to_t(c.gff[slot][:frames], dtype), to_t(fe, dtype), to_t(c.mg[guide], dtype), "video",
                                to_t(c.newline, dtype)).numpy()
    out.setflags(write=False)
    return out


def pair_errors(got, want):
    """[{"local", "global"}] per pair of a slot ([Q, rows, hidden] both); NaN counts as infinite."""
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    d = np.where(np.isnan(d), np.inf, d)
    return [{"local": float(x[:-NG].max()), "global": float(x[-NG:].max())} for x in d]


def touches(mutant, schedule, counts=COUNTS, with_fe=True):
    """{(finish index, slot)}: the finishes whose local rows an adaptor-stage fault can move -- those that hold a chunk the fault reached."""
    assert mutant in ADAPT_MUTANTS
    hit, out, npush, nfin = [False] * len(counts), set(), 0, 0
    for op in schedule:
        if op[0] == "reset":
            hit[op[1]] = False
        elif op[0] == "push":
            for i, (s, _) in enumerate(op[1]):
                hit[s] |= {"plane_offset": i > 0, "blend_first_only": i > 0, "planes_swapped": True, "prev_planes": npush > 0,
                           "key_from_ff": with_fe}[mutant]
            npush += 1
        else:
            fin = final_state(schedule, counts)[nfin]
            out |= {(nfin, s) for s in fin if hit[s]}
            nfin += 1
    return out


def adapt_ref(key, schedule, counts=COUNTS, recipe=ADAPTKV, with_fe=True, mutant=None):
    """Per finish: {slot: float64 [Q_s, local rows so far + 32, hidden]} (module docstring)."""
    assert mutant is None or mutant in MUTANTS
    assert mutant not in ADAPT_MUTANTS or recipe == ADAPTKV
    c = build(key, recipe)
    sd, h, w = c.sd, c.h, c.w
    B, npairs = len(counts), sum(counts)
    pair0 = [sum(counts[:s]) for s in range(B)]
    wps = (h // KS) * (w // KS)
    has_nl = c.newline is not None
    merge, nlpos = c.cfg.mm_patch_merge_type, c.cfg.mm_newline_position
    cap = geo.pack_layout(merge, nlpos, "video", MAX_FRAMES // KT, h // KS, w // KS, has_nl, False)
    a = "global_compressor.attn_layer."
    Wq, bq, Wk, bk, Wv, bv, Wo, bo = (_f64(sd[a + n]) for n in ("q_proj.weight", "q_proj.bias", "k_proj.weight", "k_proj.bias", "v_proj.weight",
                                                              "v_proj.bias", "out_proj.weight", "out_proj.bias"))
    hd = D // NH
    pt, ph, pw = (orc.pos_axis_table(n, D) for n in (2 * MAX_FRAMES, h, w))
    guide = list(range(npairs))                                 # pair -> index into c.mg
    frames = [0] * B
    buf = [np.zeros((cap.n_rows + NG, c.hidden)) for _ in range(npairs)]
    for b in buf:
        for r in cap.newline_rows if cap.nl_group else ():     # chunk-local newline rows (`grid` / `frame`)
            b[r] = _f64(c.newline)
    Ms, Ls, ACC = np.full(npairs * NH, -np.inf), np.zeros(npairs * NH), np.zeros((npairs * NH, D))
    prev = None                                                 # the planes of the previous push

    def mlp(stream, x):
        return ci._mlp(x, sd, f"local_compressor.{stream}_proj")

    results = []
    for op in schedule:
        if op[0] == "reset":
            rows = slice(pair0[op[1]] * NH, (pair0[op[1]] + counts[op[1]]) * NH)
            Ms[rows], Ls[rows], ACC[rows] = -np.inf, 0.0, 0.0
            frames[op[1]] = 0
            if op[2] is not None:
                for q in range(counts[op[1]]):
                    guide[pair0[op[1]] + q] = op[2] + q
            continue
        if op[0] == "finish":
            named = [s for s in range(B) if frames[s]] if op[1] is None else list(op[1])
            lay = {s: geo.pack_layout(merge, nlpos, "video", frames[s] // KT, h // KS, w // KS, has_nl, False) for s in range(B) if frames[s]}
            tail_rows = {s: (list(lay[s].newline_rows) if (has_nl and not lay[s].nl_group) else []) for s in lay}
            row0 = {s: lay[s].n_rows - len(tail_rows[s]) for s in lay}
            written = list(named)
            if mutant == "unnamed_written":
                written += [s for s in range(B) if s not in named]
            for s in written:
                at = row0[s] if s in named else 0
                if mutant == "finish_wrong_row":
                    at = row0[named[0]]
                ntail = len(tail_rows[named[0]])
                for q in range(counts[s]):
                    p = pair0[s] + q
                    sp = pair0[s] if mutant == "state_shared" else p
                    rows = slice(sp * NH, sp * NH + NH)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        ctx = ACC[rows] / Ls[rows, None]                                          # [nh, E]
                        o = np.concatenate([Wv[hh * hd:(hh + 1) * hd] @ ctx[hh] + bv[hh * hd:(hh + 1) * hd] for hh in range(NH)])
                        att = Wo @ o + bo
                        tok = ci._mlp((_f64(c.mg[guide[p]]) + att)[None], sd, "global_compressor.readout")
                    for r in range(ntail):
                        buf[p][at + r] = _f64(c.newline)
                    buf[p][at + ntail:at + ntail + NG] = tok
            results.append({s: np.stack([buf[pair0[s] + q][:lay[s].n_rows + NG].copy() for q in range(counts[s])]) for s in named})
            continue
        # ---- a push: the adaptor MLPs over the STACK, then per item the blend, the windows of every guide and the global sets
        items = [(s, Tc, frames[s]) for s, Tc in op[1]]
        ffs = [_f64(c.gff[s][t0:t0 + Tc]) for s, Tc, t0 in items]
        kxs = [_f64(c.gfe[s][t0:t0 + Tc]) if with_fe else f for (s, Tc, t0), f in zip(items, ffs)]
        stack_k = np.concatenate([(f if mutant == "key_from_ff" else k).reshape(-1, D) for f, k in zip(ffs, kxs)])
        stack_v = np.concatenate([f.reshape(-1, D) for f in ffs])
        yk = mlp("k", stack_k) if c.adapt_k else None
        yv = mlp("v", stack_v) if c.adapt_v else None
        planes = (yk, yv)
        if mutant == "prev_planes" and prev is not None:
            n = np.arange(stack_v.shape[0])
            yk, yv = (p[n % p.shape[0]] for p in prev)
        prev = planes
        if mutant == "planes_swapped":
            yk, yv = yv, yk
        first_t0, tok0 = items[0][2], 0
        for i, ((s, Tc, t0), ff, fe) in enumerate(zip(items, ffs, kxs)):
            N, Q = Tc * h * w, counts[s]
            at = 0 if mutant == "plane_offset" else tok0
            off = mutant == "blend_first_only" and i > 0
            key_t = ai._blend(c, "k", fe, yk[at:at + N]) if c.adapt_k and not off else fe
            val_t = ai._blend(c, "v", ff, yv[at:at + N]) if c.adapt_v and not off else ff
            tok0 += N
            p0 = s if mutant == "wrong_pair0" else pair0[s]
            f0 = first_t0 if mutant == "t0_shared" else t0
            pos_e = (pt[f0:f0 + Tc, None, None, :] + ph[None, :, None, :] + pw[None, None, :, :]).astype(np.float32).astype(np.float64).reshape(-1, D)
            x = ff.reshape(-1, D)
            k = ((x + pos_e) @ Wk.T + bk).reshape(-1, NH, hd)
            R = NH * Q
            sc = np.zeros((R, x.shape[0]))
            for q in range(Q):
                gq = Q - 1 - q if mutant == "guides_swapped" else q
                g = _f64(c.mg[guide[p0 + gq]])
                rows = ai._window_rows(c, key_t, val_t, g)
                m0 = (t0 // KT) * wps
                for j, row in enumerate(rows):
                    buf[p0 + q][cap.row_of(m0 + j)] = row
                if cap.nl_group:                                # the push places the chunk's own newline rows as well
                    lo, hi = (geo.pack_layout(merge, nlpos, "video", n // KT, h // KS, w // KS, has_nl, False).n_rows if n else 0 for n in (t0, t0 + Tc))
                    for r in cap.newline_rows:
                        if lo <= r < hi:
                            buf[p0 + q][r] = _f64(c.newline)
                qh = (Wq @ g + bq).reshape(NH, hd)
                sc[q * NH:(q + 1) * NH] = np.einsum("hd,nhd->hn", qh, k) * hd ** -0.5
            Mc = sc.max(axis=1)
            pr = np.exp(sc - Mc[:, None])
            Lc, Atok = pr.sum(axis=1), pr @ x
            for r in range(R):
                src = r - 16 if (mutant == "rowgroup0" and (r & 31) >= 16) else r              # whose partials the merge takes
                lsrc = r - 32 if (mutant == "pass_logits" and r >= 32) else r                  # whose logits the positional term takes
                mc = Mc[src]
                acc_c = Atok[src] + np.exp(sc[lsrc] - mc) @ pos_e
                row = (p0 * NH + r % NH) if mutant == "state_shared" else p0 * NH + r
                mn = max(Ms[row], mc)
                w_o = 1.0 if mutant == "no_rescale" else (0.0 if Ms[row] == -np.inf else np.exp(Ms[row] - mn))
                w_c = np.exp(mc - mn)
                Ms[row], Ls[row], ACC[row] = mn, Ls[row] * w_o + Lc[src] * w_c, ACC[row] * w_o + acc_c * w_c
        for s, Tc, _ in items:
            frames[s] += Tc
    return results
