"""What the cases of tests/ragged_multi_guide_train_inputs.py can see (CPU, float64).

A model of the global stage's backward as the ragged multi-guide training step computes it -- per item, over its nh Q_i folded rows in the
item's row space (row R = nh q + h): folded queries, logits, (M, L), merged contexts, the tail per pair, then dctx, delta,
dS = p (dP - delta), dqt = sum_n dS x_n + sum_n dS pe_n, and from dqt the k_proj / q_proj gradients summed over the pairs -- written out in
float64 with the defects a two-row-group, multi-pass backward over pairs can have planted in it.  The model runs no code of the package's
hot path (only the oracle, the input generators and the bar), so this file says something about the TESTS, not about the kernels.

Unmutated, the model reproduces the yardstick (fp64 autograd through the oracle per pair) on the three parameters that dS and dqt reach,
far inside the bar.  For every GPU case, each mutant moves at least one of them past the bar of tests/test_gpu_ragged_multi_guide_train.py:
  neighbour_ml   a pair's softmax weights formed with the (M, L) of the next pair of the call
  pass0_rows     pass p > 0 streams pass 0's rows again (the 32 pass offset dropped): row R >= 32 gets what row R mod 32 gets
  group0_slots   the dq merge takes row group 1's partial sums at group 0's slots (gslots dropped): the x part of dqt of a row with
                 (R >> 4) odd is that of row R - 16; the positional part, from the row's own dS, stays
  item_rows      dY gathered with the item's rows instead of the pair's: every pair of an item gets the cotangent of its first pair
  pair_sum       a pair's global cotangent summed into another pair of the same item: pair (i, 1)'s lands in pair (i, 0), its own is zero
The test prints, per case and mutant, the largest error in units of the bar.  Smallest measured multiple of a bar over all cases and
mutants: 145 (pair_sum on rmg_mix9_chunks3, q_proj.bias; neighbour_ml is never under 7.6e3, the three others never under 380)."""
import functools
import math

import numpy as np
import pytest
import torch

import ragged_multi_guide_inputs as ri
import ragged_multi_guide_train_inputs as rmt
import ragged_train_inputs as rt
from oracle import hicom_oracle as orc
from oracle_util import to_t

A = "global_compressor.attn_layer."
G = "global_compressor.readout."
SEEN = (A + "k_proj.weight", A + "q_proj.weight", A + "q_proj.bias")
MUTANTS = ("neighbour_ml", "pass0_rows", "group0_slots", "item_rows", "pair_sum")
NG = ri.NG


def gelu_grad(z):
    return 0.5 * (1 + torch.erf(z / math.sqrt(2))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


@functools.lru_cache(maxsize=None)
def forward_state(id):
    """Per item, in float64 over its nh Q_i rows: what the forward leaves, and the function from a pair's global cotangent to its dctx."""
    c = ri.build(id)
    f64 = torch.float64
    sd = {k: to_t(v, f64) for k, v in c.sd.items() if k.startswith("global_compressor.")}
    Wq, bq, Wk = sd[A + "q_proj.weight"], sd[A + "q_proj.bias"], sd[A + "k_proj.weight"]
    Wv, bv, Wo, bo = sd[A + "v_proj.weight"], sd[A + "v_proj.bias"], sd[A + "out_proj.weight"], sd[A + "out_proj.bias"]
    G0, g0, G2 = sd[G + "0.weight"], sd[G + "0.bias"], sd[G + "2.weight"]
    E = Wq.shape[0]
    nh, hd = E // 128, 128
    rows_of = {p: o.shape[0] for p, o in ri.oracle_outputs(id).items()}
    items, k = [], 0
    for i in range(c.B):
        ff = c.ff[i]
        T, H, W, _ = ff.shape
        x = to_t(ff, f64).reshape(-1, E)
        xp = (to_t(ff, f64) + orc.pos_table(T, H, W, E).double()).reshape(-1, E)          # x_n + pe_n
        g = to_t(c.g[i], f64)                                                              # [Q, E]
        Q = g.shape[0]
        qp = (g @ Wq.t() + bq).view(Q, nh, hd)
        qt = (hd ** -0.5 * torch.einsum("hje,qhj->qhe", Wk.view(nh, hd, E), qp)).reshape(Q * nh, E)
        S = qt @ xp.t()
        M = S.max(1).values
        L = torch.exp(S - M[:, None]).sum(1)
        ctx = (torch.exp(S - M[:, None]) / L[:, None]) @ xp
        o = (torch.einsum("hje,qhe->qhj", Wv.view(nh, hd, E), ctx.view(Q, nh, E)) + bv.view(nh, hd)).reshape(Q, E)
        z = (o @ Wo.t() + bo + g) @ G0.t() + g0
        dtok = torch.stack([torch.from_numpy(rmt.cotangent(id, k + q, (rows_of[i, q], G2.shape[0]))).double()[-NG:].sum(0) for q in range(Q)])
        items.append(dict(x=x, xp=xp, g=g, qp=qp, S=S, M=M, L=L, ctx=ctx, z=z, dtok=dtok, Q=Q))
        k += Q

    def dctx_of(it, dtok):
        dpre = (gelu_grad(it["z"]) * (dtok @ G2)) @ G0
        do = (dpre @ Wo).view(it["Q"], nh, hd)
        return torch.einsum("hje,qhj->qhe", Wv.view(nh, hd, E), do).reshape(it["Q"] * nh, E)
    return dict(items=items, Wk=Wk.view(nh, hd, E), scale=hd ** -0.5, E=E, nh=nh, dctx_of=dctx_of)


def model_grads(id, mutant=None):
    st = forward_state(id)
    items, E, nh = st["items"], st["E"], st["nh"]
    hd = E // nh
    dWk = torch.zeros(E, E, dtype=torch.float64)
    dWq = torch.zeros(E, E, dtype=torch.float64)
    dbq = torch.zeros(E, dtype=torch.float64)
    all_M, all_L = torch.cat([it["M"] for it in items]), torch.cat([it["L"] for it in items])
    row0 = 0
    for it in items:
        nr, Q = it["S"].shape[0], it["Q"]
        M, L = it["M"], it["L"]
        if mutant == "neighbour_ml":                    # the next pair of the call: nh rows further, around the end
            idx = (row0 + nh + torch.arange(nr)) % all_M.numel()
            M, L = all_M[idx], all_L[idx]
        dtok = it["dtok"]
        if mutant == "item_rows":
            dtok = dtok[:1].expand(Q, -1)
        if mutant == "pair_sum" and Q > 1:
            dtok = dtok.clone()
            dtok[0] += dtok[1]
            dtok[1] = 0
        dctx = st["dctx_of"](it, dtok)
        delta = (dctx * it["ctx"]).sum(1)
        p = torch.exp(it["S"] - M[:, None]) / L[:, None]
        dS = p * (dctx @ it["xp"].t() - delta[:, None])
        R = torch.arange(nr)
        if mutant == "pass0_rows":
            dS = dS[R % 32]
        dqx, dqpos = dS @ it["x"], dS @ (it["xp"] - it["x"])
        if mutant == "group0_slots":
            dqx = dqx[torch.where((R >> 4) % 2 == 1, R - 16, R)]
        dqt = (dqx + dqpos).view(Q, nh, E)
        dWk += st["scale"] * torch.einsum("qhj,qhe->hje", it["qp"], dqt).reshape(E, E)
        dqp = st["scale"] * torch.einsum("hje,qhe->qhj", st["Wk"], dqt).reshape(Q, E)
        dWq += dqp.t() @ it["g"]
        dbq += dqp.sum(0)
        row0 += nr
    return {SEEN[0]: dWk, SEEN[1]: dWq, SEEN[2]: dbq}


def in_bars(id, grads):
    """{name: max-abs error against the yardstick in units of the parameter's bar} (inf for a gradient that is not finite)."""
    want, bar = rmt.yardstick(id), rt.bars(rmt.yardstick(id))
    out = {}
    for k in SEEN:
        err = float(np.abs(grads[k].numpy() - want[k]).max())
        out[k] = err / bar[k] if math.isfinite(err) else math.inf
    return out


@pytest.mark.parametrize("id", rmt.CASES)
def test_every_mutant_moves_a_gradient_past_the_bar(id):
    clean = in_bars(id, model_grads(id))
    print(f"{id} model vs yardstick: " + "  ".join(f"{k.split('.', 2)[2]} {v:.2e}" for k, v in clean.items()) + "  (bars)")
    assert max(clean.values()) <= 0.05, f"{id}: the model is not the yardstick's backward: {clean}"
    slipped = []
    for mutant in MUTANTS:
        moved = in_bars(id, model_grads(id, mutant))
        print(f"POWER {id} {mutant}: " + "  ".join(f"{k.split('.', 2)[2]} {v:.3g}" for k, v in moved.items()) + "  (bars)")
        if not max(moved.values()) > 1.0:
            slipped.append(f"{mutant}: at most {max(moved.values()):.3g} bars")
    assert not slipped, f"{id}: " + "; ".join(slipped)
