"""Inputs and the float64 reference of the clip stream group with several guides per slot (HIComProjector.open_stream_group_multi,
hicom_amd/clip_stream_group_multi.py).

The input family is that of tests/clip_stream_group_inputs.py (per-slot clips with GROUP_SCALES rotated by the slot, TOL, the layout): slot s
has COUNTS[s] guides of its own, a PAIR is one (slot, guide), numbered slot-major then guide-major; `build(key).mg` holds the M = sum COUNTS
guides of the open call and, behind them, the guides a reset brings.

multi_ref is a numpy float64 restatement of the SCHEDULE the device runs.  It keeps the device's row space: an item with Q guides has the
folded rows R = nh q + h, streamed in passes of 32 rows and row groups of 16; a row's chunk set is (M_c, L_c, sum p x) from the partials of
its 16-row group plus the positional term from the row's logits; the fold goes into state row pair0 nh + R in E-space, and finish applies
v_proj per head, out_proj, the guide as residual and the readout per pair.  A SCHEDULE is a list of
    ("push", ((slot, Tc), ...))     ("finish", slots or None)  [None: every slot that holds frames]     ("reset", slot, first guide index or None)
and multi_ref returns, per finish, {slot: [Q_s, local rows so far + 32, hidden]}.  A `mutant` restates a fault of the many-pair schedule:

  guides_swapped    the guides of a slot are taken in reverse order (pair q works with guide Q - 1 - q)
  wrong_pair0       an item's first pair is its slot's INDEX, the first pair of a group with one guide per slot
  rowgroup0         rows >= 16 of a pass take row group 0's partials (row R merges the partials of row R - 16)
  pass_logits       pass 1 reads pass 0's logits (row R >= 32 takes the positional term from the logits of row R - 32)
  state_shared      all guides of a slot fold into, and finish from, the state of the slot's first guide
  t0_shared         every item of a push uses the first item's frame offset
  no_rescale        the carried state is not rescaled when the running maximum rises
  finish_wrong_row  finish_many places every named slot's rows at the first named slot's row
  unnamed_written   finish_many also writes the rows of the slots it was not given, at the row the host passes for them (0)

tests/test_clip_stream_group_multi_power.py holds every mutant to >= 4 bars of movement in some region of some finish."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import clip_stream_group_inputs as gi
import clip_stream_inputs as ci
from hicom_amd import geometry as geo
from hicom_amd import synth
from oracle import hicom_oracle as orc
from oracle_util import to_t

D, NG, KT, KS, TOL = ci.D, ci.NG, ci.KT, ci.KS, ci.TOL
NH = D // 128
COUNTS = (1, 2, 4)
M = sum(COUNTS)
PAIR0 = tuple(sum(COUNTS[:s]) for s in range(len(COUNTS)))
MUTANTS = ("guides_swapped", "wrong_pair0", "rowgroup0", "pass_logits", "state_shared", "t0_shared", "no_rescale", "finish_wrong_row", "unnamed_written")

G12 = ci.T12
G12_GRID = ci.T12_GRID
G12_ONE = (12, 6, 6, 64, "one_token")
WIDE = ci.WIDE
MAX_FRAMES = 16

# B = 3 with (1, 2, 4) guides, at most 12 frames per slot: all slots with unequal chunks; a permuted subset whose items differ in t0 (8 and 4)
# and in Tc; one slot alone; finish_many on a subset, then on every slot; reset(slot 1, two new guides: the guides from index M on) while the
# others go on; slot 1 at t0 = 0 next to slot 2 at t0 = 8; finish_many
SCHEDULE = (("push", ((0, 4), (1, 8), (2, 4))), ("push", ((1, 4), (0, 8))), ("push", ((2, 4),)), ("finish", (0, 2)), ("finish", None), ("reset", 1, M),
            ("push", ((1, 4), (2, 4))), ("finish", None))
# B = 2 with (2, 4) guides on the wide case: chunks (4, 4), then (4,) into slot 1 only
COUNTS_WIDE = (2, 4)
SCHEDULE_WIDE = (("push", ((0, 4), (1, 4))), ("push", ((1, 4),)), ("finish", None))


@functools.lru_cache(maxsize=None)
def build(key):
    """clip_stream_group_inputs.build(key) with `mg`: M + 2 guides (the last two: what reset(slot 1) brings)."""
    c = gi.build(key)
    mg = [synth.synth_inputs(1, 3, 3, D, tag=f"{ci.TAG}:group_multi_guide{i}")["g"] for i in range(M + 2)]
    for a in mg:
        assert a.dtype == np.float32 and np.array_equal(synth.round_to_bf16(a), a)
    return SimpleNamespace(**vars(c), mg=mg)


def final_state(schedule, counts=COUNTS):
    """Per finish of the schedule: {slot: (frames, first guide index)} of the slots it returns."""
    pair0 = [sum(counts[:s]) for s in range(len(counts))]
    frames, guide0, out = [0] * len(counts), list(pair0), []
    for op in schedule:
        if op[0] == "push":
            for s, n in op[1]:
                frames[s] += n
        elif op[0] == "reset":
            frames[op[1]] = 0
            guide0[op[1]] = guide0[op[1]] if op[2] is None else op[2]
        else:
            named = [s for s in range(len(counts)) if frames[s]] if op[1] is None else list(op[1])
            out.append({s: (frames[s], guide0[s]) for s in named})
    return out


@functools.lru_cache(maxsize=None)
def oracle_output(key, slot, frames, guide, with_fe=True, dtype=torch.float32):
    """oracle.projector_forward on the first `frames` frames of slot `slot`'s clip with guide mg[guide]; callers must not write into it."""
    c = build(key)
    sd = {k: to_t(v, dtype) for k, v in c.sd.items()}
    fe = c.gfe[slot][:frames] if with_fe else None
    out = orc.projector_forward(c.cfg, sd, to_t(c.gff[slot][:frames], dtype), to_t(fe, dtype), to_t(c.mg[guide], dtype), "video",
                                to_t(c.newline, dtype)).numpy()
    out.setflags(write=False)
    return out


_f64 = ci._f64


def multi_ref(key, schedule, counts=COUNTS, with_fe=True, mutant=None):
    """Per finish: {slot: float64 [Q_s, local rows so far + 32, hidden]} (module docstring)."""
    assert mutant is None or mutant in MUTANTS
    c = build(key)
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

    def clear(s):
        rows = slice(pair0[s] * NH, (pair0[s] + counts[s]) * NH)
        Ms[rows], Ls[rows], ACC[rows] = -np.inf, 0.0, 0.0

    results = []
    for op in schedule:
        if op[0] == "reset":
            clear(op[1])
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
        named = [s for s, _ in op[1]]
        first_t0 = frames[named[0]]
        for s, Tc in op[1]:
            t0, Q = frames[s], counts[s]
            p0 = s if mutant == "wrong_pair0" else pair0[s]
            ff, fe = _f64(c.gff[s][t0:t0 + Tc]), _f64(c.gfe[s][t0:t0 + Tc] if with_fe else c.gff[s][t0:t0 + Tc])
            f0 = first_t0 if mutant == "t0_shared" else t0
            pos_e = (pt[f0:f0 + Tc, None, None, :] + ph[None, :, None, :] + pw[None, None, :, :]).astype(np.float32).astype(np.float64).reshape(-1, D)
            x = ff.reshape(-1, D)
            k = ((x + pos_e) @ Wk.T + bk).reshape(-1, NH, hd)
            R = NH * Q
            sc = np.zeros((R, x.shape[0]))
            for q in range(Q):
                gq = Q - 1 - q if mutant == "guides_swapped" else q
                g = _f64(c.mg[guide[p0 + gq]])
                # the local rows of pair p0 + q
                rows = ci._local_rows(c, ff, fe, g)
                m0 = (t0 // KT) * wps
                for i, row in enumerate(rows):
                    buf[p0 + q][cap.row_of(m0 + i)] = row
                if cap.nl_group:                                # the push places the chunk's own newline rows as well
                    lo, hi = (geo.pack_layout(merge, nlpos, "video", n // KT, h // KS, w // KS, has_nl, False).n_rows if n else 0 for n in (t0, t0 + Tc))
                    for r in cap.newline_rows:
                        if lo <= r < hi:
                            buf[p0 + q][r] = _f64(c.newline)
                qh = (Wq @ g + bq).reshape(NH, hd)
                sc[q * NH:(q + 1) * NH] = np.einsum("hd,nhd->hn", qh, k) * hd ** -0.5
            # the stream's partials per row: (m, l, sum p x), relative to the row's own maximum
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
        for s, Tc in op[1]:
            frames[s] += Tc
    return results


def cs_prefix_rows(proj, frames, c):
    """Local rows of a prefix of `frames` frames without the rows that belong to finish (hicom_amd.clip_stream.prefix_layout)."""
    from hicom_amd import clip_stream
    return clip_stream.prefix_layout(proj, frames // KT, c.h // KS, c.w // KS, c.newline is not None)[0]


def region_errors(got, want):
    """{"local", "global"}: the largest error over the pairs of a slot ([Q, rows, hidden] both)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    d = np.where(np.isnan(d), np.inf, d)
    return {"local": float(d[:, :-NG].max()), "global": float(d[:, -NG:].max())}
