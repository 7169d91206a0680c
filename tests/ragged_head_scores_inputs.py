"""Inputs, float64 references and planted faults for the segmented scores kernel hicom_head_scores_ragged_fwd behind
hicom_head_guide_fold_many_fwd (csrc/head_scores.hip): B items stacked, item i with N_i tokens and its own Q_i guides.
Shared by tests/test_gpu_ragged_head_scores.py (the kernels against the references) and tests/test_ragged_head_scores_power.py (CPU: what
a wrong kernel would do to the references, against the same bounds).

Operands   as tests/head_scores_inputs.py draws them, over the whole stack: x bf16 [sum N_i, 1152], hid fp16 [sum N_i, ld] = |N(0, 1)| on
           columns < inter and SENTINEL on [inter, kpad) and in the pitch gap (`clean`: zero there -- the result must not move), guides bf16
           [sum Q_i, 1152], W2, b2.
Mixes      token counts are free at kernel level:
             n4        N (5, 36, 53, 729), Q (1, 3, 17, 2): an item inside one tile, tails of 4 and 21 tokens, 23 tiles of one item, both
                       row-group forms (max Q_i = 17)
             mix6      N (36, 144, 36, 288, 36), Q (1, 3, 5, 2, 4): the step's MIX6 (frames (1, 4, 1, 8, 1) of 6 x 6)
             q32       N (9, 9), Q (32, 1): a full tile of guide rows in front of a one-guide item whose tile reads 31 rows behind its own
             pitched   inter 4304 (kpad 4352, ld 4544): one item, N 144, Q 3
             pitched2  the same plane with two items, N (144, 40), Q (3, 17)
           inter 200 on the first three.
Reference  out[q, tok0_i + n] = x[n] . g + hid[n, :inter] . (W2^T g) + g . b2 with g = guide q of item i, float64, for q < Q_i; every other
           cell of the [max Q_i, sum N_i] buffer is NaN: the kernel does not write it.
Bound      the hs_tol formula of tests/head_scores_inputs.py (derived there from the formats and the summation structure) on the item's
           operands: `item_tol`; tests/test_ragged_head_scores_power.py holds it against hs_tol itself.
Faults     `MUTANTS`: what a kernel with one wrong index writes into that buffer (None where the fault computes the same function)."""
import functools
from types import SimpleNamespace
from typing import NamedTuple

import torch

import head_scores_inputs as hs
import window_attn_inputs as wi
from ops_reference import up

D = hs.D
NAN = float("nan")
TILE = 32


class Mix(NamedTuple):
    id: str
    N: tuple
    Q: tuple
    inter: int = 200


MIXES = (Mix("n4", (5, 36, 53, 729), (1, 3, 17, 2)), Mix("mix6", (36, 144, 36, 288, 36), (1, 3, 5, 2, 4)), Mix("q32", (9, 9), (32, 1)),
         Mix("pitched", (144,), (3,), 4304), Mix("pitched2", (144, 40), (3, 17), 4304))
BY_ID = {m.id: m for m in MIXES}


def prefix(v):
    out, s = [], 0
    for x in v:
        out.append(s)
        s += x
    return out


@functools.lru_cache(maxsize=None)
def build(mix):
    g = torch.Generator().manual_seed(wi._seed("ragged-head-scores-" + mix.id))
    rnd = lambda *s: torch.randn(*s, generator=g)
    kpad, ld = hs.kpad_ld(mix.inter)
    M, T = sum(mix.Q), sum(mix.N)
    hid = torch.full((T, ld), hs.SENTINEL)
    hid[:, :mix.inter] = rnd(T, mix.inter).abs()
    clean = hid.clone()
    clean[:, mix.inter:] = 0
    return SimpleNamespace(mix=mix, kpad=kpad, ld=ld, M=M, T=T, tok0=prefix(mix.N), pair0=prefix(mix.Q), x=rnd(T, D).bfloat16(), hid=hid.half(),
                           clean=clean.half(), guides=rnd(M, D).bfloat16(), w2=(0.03 * rnd(D, mix.inter)).bfloat16(), b2=(0.5 * rnd(D)).bfloat16())


def item_operands(b, i):
    """Item i as a case of head_scores_inputs (what hs_terms and the bound read): its tokens, its guides, the shared weights."""
    t, p = b.tok0[i], b.pair0[i]
    return SimpleNamespace(case=SimpleNamespace(inter=b.mix.inter), x=b.x[t:t + b.mix.N[i]], hid=b.hid[t:t + b.mix.N[i]], guides=b.guides[p:p + b.mix.Q[i]],
                           w2=b.w2, b2=b.b2)


def tol_of(c):
    """head_scores_inputs.hs_tol on the operands `c` (its lines, with hs_build(case) replaced by the argument)."""
    inter = c.case.inter
    x, h, g, w2, b2 = (up(t).abs() for t in (c.x, c.hid[:, :inter], c.guides, c.w2, c.b2))
    Uab = g @ w2
    U = hs.hs_terms(c)[3].abs()
    A = g @ x.T + U @ h.T + (g @ b2)[:, None]
    K = D + inter
    return ((2 * (K / 4 + 128) + 12) * hs.EPS24 * A + (D / 16 + 18) * hs.EPS24 * (Uab @ h.T)
            + 2.0 ** -21 * U.max(1).values[:, None] * h.sum(1)[None, :])


@functools.lru_cache(maxsize=None)
def item_tol(mix, i):
    return tol_of(item_operands(build(mix), i))


@functools.lru_cache(maxsize=None)
def item_reference(mix, i):
    gx, uh, cc, _ = hs.hs_terms(item_operands(build(mix), i))
    return gx + uh + cc[:, None]


@functools.lru_cache(maxsize=None)
def _all_rows(mix):
    """(g . x + U . hid, c) of EVERY guide row against EVERY token of the stack, [M + 64, T] and [M + 64], zero in the 64 rows behind M (the
    planes' pad rows and a zero guide): what a kernel with a wrong row or token index computes."""
    b = build(mix)
    gx, uh, cc, _ = hs.hs_terms(SimpleNamespace(case=SimpleNamespace(inter=mix.inter), x=b.x, hid=b.hid, guides=b.guides, w2=b.w2, b2=b.b2))
    pad = torch.zeros(64, b.T, dtype=torch.float64)
    return torch.cat([gx + uh, pad]), torch.cat([cc, pad[:, 0]])


def empty(mix):
    return torch.full((max(mix.Q), sum(mix.N)), NAN, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def reference(mix):
    """The [max Q_i, sum N_i] buffer as the kernel leaves it after a NaN pre-fill."""
    b, out = build(mix), empty(mix)
    for i, (n, q) in enumerate(zip(mix.N, mix.Q)):
        out[:q, b.tok0[i]:b.tok0[i] + n] = item_reference(mix, i)
    return out


MUTANTS = ("pair0_of_previous_item", "tile_runs_into_next_item", "q_of_item_0", "c_by_guide_number")


def mutant(mix, name):
    """The buffer under one planted fault, or None where the fault is not defined on the mix:
      pair0_of_previous_item    item i >= 1 takes the guide rows (and U, scale, c) that start at item i - 1's first pair   (B > 1)
      tile_runs_into_next_item  tiles of 32 counted over the stack, a tile's item that of its first token: the tokens behind an item's end
                                meet that item's guides   (some tile crosses an item boundary)
      q_of_item_0               every item stores item 0's number of guide rows   (some Q_i != Q_0)
      c_by_guide_number         c[q] instead of c[pair0 + q]   (B > 1)"""
    b, out = build(mix), empty(mix)
    s, c = _all_rows(mix)
    B = len(mix.N)
    span = lambda i: slice(b.tok0[i], b.tok0[i] + mix.N[i])
    if name == "pair0_of_previous_item":
        if B == 1:
            return None
        for i in range(B):
            p = b.pair0[max(i - 1, 0)] if i else 0
            out[:mix.Q[i], span(i)] = s[p:p + mix.Q[i], span(i)] + c[p:p + mix.Q[i], None]
        return out
    if name == "tile_runs_into_next_item":
        ends = [t + n for t, n in zip(b.tok0, mix.N)]
        if all(e % TILE == 0 for e in ends[:-1]):
            return None
        owner = lambda n: next(i for i, e in enumerate(ends) if n < e)
        for t0 in range(0, b.T, TILE):
            i = owner(t0)
            p, q = b.pair0[i], mix.Q[i]
            out[:q, t0:min(t0 + TILE, b.T)] = s[p:p + q, t0:min(t0 + TILE, b.T)] + c[p:p + q, None]
        return out
    if name == "q_of_item_0":
        if all(q == mix.Q[0] for q in mix.Q):
            return None
        q = mix.Q[0]
        for i in range(B):
            p = b.pair0[i]
            out[:q, span(i)] = s[p:p + q, span(i)] + c[p:p + q, None]
        return out
    if name == "c_by_guide_number":
        if B == 1:
            return None
        for i in range(B):
            p, q = b.pair0[i], mix.Q[i]
            out[:q, span(i)] = s[p:p + q, span(i)] + c[:q, None]
        return out
    raise KeyError(name)


def worst(mix, got):
    """The largest error / bound over the cells of every item's guides (a NaN there counts as infinite), infinite as well if any cell
    that the kernel must not write (q >= Q_i on item i's tokens) is not the NaN of the pre-fill.  got: [max Q_i, sum N_i]."""
    b, w = build(mix), 0.0
    for i, (n, q) in enumerate(zip(mix.N, mix.Q)):
        cells = got[:, b.tok0[i]:b.tok0[i] + n].double()
        err = (cells[:q] - item_reference(mix, i)).abs()
        err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
        w = max(w, float((err / item_tol(mix, i)).max()))
        if not bool(torch.isnan(cells[q:]).all()):
            w = float("inf")
    return w
