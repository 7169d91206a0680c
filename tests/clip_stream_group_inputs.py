"""Inputs and the float64 reference of the clip stream group (HIComProjector.open_stream_group, hicom_amd/clip_stream_group.py): B live
videos with one guide each, pushed together in chunks of whole window groups, every slot carrying its own global softmax state.

The input family is that of tests/clip_stream_inputs.py (its `build`, TOL, GROUP_SCALES and layout): slot s gets a guide of its own and the
family's clip with GROUP_SCALES rotated by s groups (powers of two: exact in bf16), so the slots differ in their tokens and the running
maximum of the global softmax rises at different pushes in different slots.

group_ref is a numpy float64 restatement of what the group computes.  It replays a SCHEDULE -- a list of
    ("push", ((slot, Tc), ...))      ("finish",)  [every slot that holds frames]      ("reset", slot, guide index or None)
-- and returns, per ("finish",), {slot: [local rows so far + 32, hidden]}.  A `mutant` switch restates the faults a many-slot push can have:

  t0_shared        every item of a push uses the first item's frame offset
  t0_restart       the frame offset of every item is 0
  slot_swap        an item folds into, takes the guide of and writes to the slot at its POSITION in the call, not its named slot
  row0_shared      every item's local rows land at the first item's row offset
  absent_touched   a slot that is absent from a push is emptied by it
  no_rescale       the carried state is not rescaled when the running maximum rises
  reset_all        a reset empties every slot
  marg_normalised  the positional term of a chunk's set is divided by L_c before the fold

`touches(mutant, schedule)` says which (finish, slot, region) entries a mutant can move under a schedule, by walking the schedule with the
rule of the mutant (no_rescale: every push behind a slot's first -- the positional term moves the maximum too, so the scales alone do not
say which push raises it; absent_touched empties the slot, and a slot that is never pushed again finishes as NaN: moved without bound); tests/test_clip_stream_group_power.py holds every other entry to zero movement.

The bound of the merge + fold kernel alone (hicom_stream_group_merge_fold_fwd; tests/test_gpu_clip_stream_group.py).  One (item, head) row:
    L' = w_o L + w_c L_c,   ACC' = w_o ACC + w_c ACC_c,   L_c = sum_p u_p l_p,   ACC_c = sum_p u_p acc_p + sum_s marg_s pe[s],
    u_p = e^(m_p - M_c),  w_o = e^(M - M'),  w_c = e^(M_c - M'),  marg_s = sum over the slot's tokens of e^(logit - M_c).
 (a) the merge of the partials, global_stream_inputs.forward_bounds' merge terms un-normalised: each u_p carries the device exponential
     (TRANS) and the rounding of its argument (2^-23 |m_p - M_c|); the nparts terms are summed: (nparts + 8) 2^-23.
 (b) the positional rows: each of the N = Tc H W weights e^(logit - M_c) carries TRANS and 2^-23 |logit - M_c|; a marginal sums <= N of them
     in two stages ((N + 8) 2^-23 covers every order); the T + H + W products marg_s pe[s] are accumulated by fma: (T + H + W) 2^-23.
 (c) the fold, one more term on the bound of tests/test_gpu_clip_stream.py's docstring: w_o and w_c carry TRANS and 2^-23 |m - M'| each, two
     terms summed with their products: 8 2^-23; the errors of (a) and (b) reach the result scaled by w_c.
With A_c = sum_p u_p |acc_p|, B_c = sum_s marg_s |pe[s]|, D_c = sum_p u_p 2^-23 |m_p - M_c| |acc_p|, G_c = sum_s (sum_n e_n 2^-23 |logit_n - M_c|)
|pe[s]| (the argument roundings, weighted):
    |err ACC'| <= (8 2^-23 + 2 TRANS) (w_o |ACC| + w_c (A_c + B_c)) + 2^-23 (|M - M'| w_o |ACC| + |M_c - M'| w_c (A_c + B_c))
                  + w_c [((nparts + 8) 2^-23 + TRANS) A_c + D_c + ((N + T + H + W + 8) 2^-23 + TRANS) B_c + G_c]
and the same for L' with l in the place of acc and no positional rows.  M' is a maximum: exact."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import clip_stream_inputs as ci
from global_stream_inputs import EPS23, TRANS
from hicom_amd import geometry as geo
from hicom_amd import synth
from oracle import hicom_oracle as orc
from oracle_util import to_t

D, NG, KT, KS, TOL = ci.D, ci.NG, ci.KT, ci.KS, ci.TOL
B = 3
MUTANTS = ("t0_shared", "t0_restart", "slot_swap", "row0_shared", "absent_touched", "no_rescale", "reset_all", "marg_normalised")

# (T, h, w, hidden, newline position or None): clip_stream_inputs' keys
G12 = ci.T12
G12_GRID = ci.T12_GRID
WIDE = ci.WIDE

# B = 3, at most 12 frames per slot: all slots with unequal chunks; a permuted subset whose items differ in t0 (8 and 4) AND in Tc (4 and 8);
# one slot alone; finish on every slot; reset(slot 0, a new guide) while the others go on; slot 0 at t0 = 0 next to slot 2 at t0 = 8
SCHEDULE = (("push", ((0, 4), (1, 8), (2, 4))), ("push", ((1, 4), (0, 8))), ("push", ((2, 4),)), ("finish",), ("reset", 0, 3),
            ("push", ((0, 4), (2, 4))), ("finish",))
# B = 2 on the wide case: chunks (4, 4), then (4,) into one slot only -- slot 0, whose second group raises the running maximum
SCHEDULE_WIDE = (("push", ((0, 4), (1, 4))), ("push", ((0, 4),)), ("finish",))


def scale_of(slot, t):
    return ci.GROUP_SCALES[(t // KT + slot) % len(ci.GROUP_SCALES)]


@functools.lru_cache(maxsize=None)
def build(key):
    """clip_stream_inputs.build(key) with per-slot clips ff[s], fe[s] (the family's clip, GROUP_SCALES rotated by s groups) and guides
    g[0 .. B] (g[B]: the guide reset() brings)."""
    c = ci.build(key)
    base = np.array([scale_of(0, t) for t in range(c.T)], dtype=np.float32)[:, None, None, None]
    ff, fe = [], []
    for s in range(B):
        r = np.array([scale_of(s, t) for t in range(c.T)], dtype=np.float32)[:, None, None, None] / base
        ff.append(c.ff * r)
        fe.append(c.fe * r)
    g = [c.g, c.g2] + [synth.synth_inputs(1, 3, 3, D, tag=f"{ci.TAG}:group_guide{i}")["g"] for i in range(2, B + 1)]
    for a in ff + fe + g:
        assert a.dtype == np.float32 and np.array_equal(synth.round_to_bf16(a), a)
    return SimpleNamespace(**vars(c), gff=ff, gfe=fe, gg=g)


def final_state(schedule, nslots=B):
    """Per ("finish",) of the schedule: {slot: (frames, guide index)} of the slots that hold frames."""
    frames, guide, out = [0] * nslots, list(range(nslots)), []
    for op in schedule:
        if op[0] == "push":
            for s, n in op[1]:
                frames[s] += n
        elif op[0] == "reset":
            frames[op[1]] = 0
            guide[op[1]] = guide[op[1]] if op[2] is None else op[2]
        else:
            out.append({s: (frames[s], guide[s]) for s in range(nslots) if frames[s]})
    return out


@functools.lru_cache(maxsize=None)
def oracle_output(key, slot, frames, guide, with_fe=True, dtype=torch.float32):
    """oracle.projector_forward on the first `frames` frames of slot `slot`'s clip with guide `guide`; callers must not write into it."""
    c = build(key)
    sd = {k: to_t(v, dtype) for k, v in c.sd.items()}
    fe = c.gfe[slot][:frames] if with_fe else None
    out = orc.projector_forward(c.cfg, sd, to_t(c.gff[slot][:frames], dtype), to_t(fe, dtype), to_t(c.gg[guide], dtype), "video",
                                to_t(c.newline, dtype)).numpy()
    out.setflags(write=False)
    return out


def stacked(key, items, t0s, with_fe=True):
    """The stacked chunk tensors of one push: items ((slot, Tc), ...) at the frame offsets t0s."""
    c = build(key)
    ff = np.concatenate([c.gff[s][t:t + n] for (s, n), t in zip(items, t0s)])
    fe = np.concatenate([c.gfe[s][t:t + n] for (s, n), t in zip(items, t0s)]) if with_fe else None
    return ff, fe


def touches(mutant, schedule, nslots=B):
    """The set of (finish index, slot, region) a mutant can move under `schedule` (module docstring)."""
    frames = [0] * nslots
    bad = {r: [False] * nslots for r in ("local", "global")}
    out, nfin = set(), 0
    for op in schedule:
        if op[0] == "push":
            named = [s for s, _ in op[1]]
            first_t0 = frames[named[0]]
            for s in range(nslots):
                if mutant == "absent_touched" and s not in named and frames[s]:
                    bad["global"][s] = True
            for pos, (s, n) in enumerate(op[1]):
                t0 = frames[s]
                if ((mutant == "t0_shared" and t0 != first_t0) or (mutant == "t0_restart" and t0) or mutant == "marg_normalised"
                        or (mutant == "no_rescale" and t0)):
                    bad["global"][s] = True
                if mutant == "row0_shared" and t0 != first_t0:
                    bad["local"][s] = True
                if mutant == "slot_swap" and pos != s:
                    for r in bad:
                        bad[r][s] = bad[r][pos] = True
            for s, n in op[1]:
                frames[s] += n
        elif op[0] == "reset":
            for s in range(nslots):
                if s == op[1]:
                    frames[s], bad["local"][s], bad["global"][s] = 0, False, False
                elif mutant == "reset_all" and frames[s]:
                    bad["global"][s] = True
        else:
            out |= {(nfin, s, r) for r in bad for s in range(nslots) if frames[s] and bad[r][s]}
            nfin += 1
    return out


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------------
_f64 = ci._f64


def group_ref(key, schedule, with_fe=True, mutant=None, nslots=B):
    """Per ("finish",): {slot: float64 [local rows so far + 32, hidden]} (module docstring)."""
    assert mutant is None or mutant in MUTANTS
    c = build(key)
    sd, h, w = c.sd, c.h, c.w
    wps = (h // KS) * (w // KS)
    has_nl = c.newline is not None
    merge, nlpos = c.cfg.mm_patch_merge_type, c.cfg.mm_newline_position
    cap = geo.pack_layout(merge, nlpos, "video", c.T // KT, h // KS, w // KS, has_nl, False)
    a = "global_compressor.attn_layer."
    Wq, bq, Wk, bk, Wv, bv, Wo, bo = (_f64(sd[a + n]) for n in ("q_proj.weight", "q_proj.bias", "k_proj.weight", "k_proj.bias", "v_proj.weight",
                                                              "v_proj.bias", "out_proj.weight", "out_proj.bias"))
    nh, hd = D // 128, 128
    pt, ph, pw = (orc.pos_axis_table(n, D) for n in (2 * c.T, h, w))       # (frame rows past T: what a mutant's wrong offset reaches)
    guide = list(range(nslots))
    frames = [0] * nslots
    buf = [np.zeros((cap.n_rows + NG, c.hidden)) for _ in range(nslots)]
    for b in buf:
        for r in cap.newline_rows:            # chunk-local newline rows (`grid` / `frame`): the rows of a prefix are those of the whole clip
            b[r] = _f64(c.newline)

    def empty():
        return [np.full(nh, -np.inf), np.zeros(nh), np.zeros((nh, hd))]
    state = [empty() for _ in range(nslots)]
    results = []
    for op in schedule:
        if op[0] == "reset":
            for s in range(nslots):
                if s == op[1] or mutant == "reset_all":
                    state[s] = empty()
            frames[op[1]] = 0
            if op[2] is not None:
                guide[op[1]] = op[2]
            continue
        if op[0] == "finish":
            res = {}
            for s in range(nslots):
                if not frames[s]:
                    continue
                lay = geo.pack_layout(merge, nlpos, "video", frames[s] // KT, h // KS, w // KS, has_nl, False)
                g = _f64(c.gg[guide[s]])
                M, L, O = state[s]
                out = buf[s][:lay.n_rows + NG].copy()
                for r in lay.newline_rows:
                    out[r] = _f64(c.newline)
                with np.errstate(invalid="ignore", divide="ignore"):
                    att = Wo @ (O / L[:, None]).reshape(D) + bo
                out[lay.n_rows:] = ci._mlp((g + att)[None], sd, "global_compressor.readout")
                res[s] = out
            results.append(res)
            continue
        named = [s for s, _ in op[1]]
        first_t0 = frames[named[0]]
        if mutant == "absent_touched":
            for s in range(nslots):
                if s not in named:
                    state[s] = empty()
        for pos, (s, Tc) in enumerate(op[1]):
            t0 = frames[s]
            dst = pos if mutant == "slot_swap" else s               # the slot the device works on: guide, state and output buffer
            g = _f64(c.gg[guide[dst]])
            ff, fe = _f64(c.gff[s][t0:t0 + Tc]), _f64(c.gfe[s][t0:t0 + Tc] if with_fe else c.gff[s][t0:t0 + Tc])
            rows = ci._local_rows(c, ff, fe, g)
            m0 = ((first_t0 if mutant == "row0_shared" else t0) // KT) * wps
            for i, row in enumerate(rows):
                buf[dst][cap.row_of(m0 + i)] = row
            f0 = {"t0_shared": first_t0, "t0_restart": 0}.get(mutant, t0)
            pos_e = (pt[f0:f0 + Tc, None, None, :] + ph[None, :, None, :] + pw[None, None, :, :]).astype(np.float32).astype(np.float64)
            qh = (Wq @ g + bq).reshape(nh, hd)
            x = (ff + pos_e).reshape(-1, D)
            k = (x @ Wk.T + bk).reshape(-1, nh, hd).transpose(1, 0, 2)
            v_tok = (ff.reshape(-1, D) @ Wv.T + bv).reshape(-1, nh, hd).transpose(1, 0, 2)
            v_pos = (pos_e.reshape(-1, D) @ Wv.T).reshape(-1, nh, hd).transpose(1, 0, 2)
            sc = np.einsum("hd,hnd->hn", qh, k) * hd ** -0.5
            Mc = sc.max(axis=1)
            p = np.exp(sc - Mc[:, None])
            Lc = p.sum(axis=1)
            O_pos = np.einsum("hn,hnd->hd", p, v_pos)
            Oc = np.einsum("hn,hnd->hd", p, v_tok) + (O_pos / Lc[:, None] if mutant == "marg_normalised" else O_pos)
            M, L, O = state[dst]
            Mn = np.maximum(M, Mc)
            w_o = np.ones(nh) if mutant == "no_rescale" else np.exp(M - Mn)
            w_c = np.exp(Mc - Mn)
            state[dst] = [Mn, L * w_o + Lc * w_c, O * w_o[:, None] + Oc * w_c[:, None]]
        for s, Tc in op[1]:
            frames[s] += Tc
    return results


def region_errors(got, want):
    return ci.region_errors(got, want)


# ---- the merge + fold kernels alone: the shapes of their tests, the float64 reference and its bounds -----------------------------------------
# =============================================================================================================================
# the merge + fold kernel alone
# =============================================================================================================================
ITEMS, R, RP, E, TC, H, W = 3, 9, 16, 1152, 4, 6, 6
N = TC * H * W
Y0, X0, P = 16, 22, 28
SLOTS, T0S, NSLOTS = (2, 0, 1), (8, 0, 4), 4             # a fourth slot is absent


def merge_fold_ref(nparts, pm, pl, pacc, s, pe, ml, acc):
    """float64 (M', L', ACC') per item and the bounds of L' and ACC' (clip_stream_group_inputs' docstring)."""
    out = []
    f = lambda x: np.asarray(x, dtype=np.float64)
    for i, (slot, t0) in enumerate(zip(SLOTS, T0S)):
        m, l, a = (f(x[i * nparts:(i + 1) * nparts, :R]) for x in (pm, pl, pacc))           # [nparts, R], [nparts, R, E]
        Mc = m.max(axis=0)
        u = np.exp(m - Mc)
        Lc, Lc_arg = (u * l).sum(0), (u * EPS23 * np.abs(m - Mc) * l).sum(0)
        A, A_abs = (u[..., None] * a).sum(0), (u[..., None] * np.abs(a)).sum(0)
        D_c = ((u * EPS23 * np.abs(m - Mc))[..., None] * np.abs(a)).sum(0)
        e = np.exp(f(s[i, :R]) - Mc[:, None]).reshape(R, TC, H, W)
        ea = e * EPS23 * np.abs(f(s[i, :R]).reshape(R, TC, H, W) - Mc[:, None, None, None])
        rows = np.concatenate([f(pe[t0:t0 + TC]), f(pe[Y0:Y0 + H]), f(pe[X0:X0 + W])])        # [T + H + W, E]
        marg = lambda w: np.concatenate([w.sum((2, 3)), w.sum((1, 3)), w.sum((1, 2))], axis=1)     # [R, T + H + W]
        Bc, B_abs, G_c = marg(e) @ rows, marg(e) @ np.abs(rows), marg(ea) @ np.abs(rows)
        M, L, ACC = f(ml[slot, :, 0]), f(ml[slot, :, 1]), f(acc[slot])
        Mn = np.maximum(M, Mc)
        with np.errstate(invalid="ignore"):
            w_o = np.where(np.isinf(M), 0.0, np.exp(M - Mn))
            arg_o = np.where(np.isinf(M), 0.0, np.abs(M - Mn))
        w_c, arg_c = np.exp(Mc - Mn), np.abs(Mc - Mn)
        Ln, An = w_o * L + w_c * Lc, w_o[:, None] * ACC + w_c[:, None] * (A + Bc)
        rel = 8 * EPS23 + 2 * TRANS
        k_m, k_p = (nparts + 8) * EPS23 + TRANS, (N + TC + H + W + 8) * EPS23 + TRANS
        l_tol = rel * (w_o * L + w_c * Lc) + EPS23 * (arg_o * w_o * L + arg_c * w_c * Lc) + w_c * (k_m * Lc + Lc_arg)
        a_mag = w_c[:, None] * (A_abs + B_abs)
        a_tol = (rel * (w_o[:, None] * np.abs(ACC) + a_mag) + EPS23 * (arg_o[:, None] * w_o[:, None] * np.abs(ACC) + arg_c[:, None] * a_mag)
                 + w_c[:, None] * (k_m * A_abs + D_c + k_p * B_abs + G_c))
        out.append((slot, Mn, Ln, An, l_tol, a_tol))
    return out
