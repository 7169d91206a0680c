"""What the cases of tests/ragged_train_inputs.py can see (CPU, float64).

A model of the global stage's backward as the ragged training step computes it -- per item: folded queries, logits, (M, L), merged
contexts, the tail, then dctx, delta, dS = p (dP - delta), dqt = sum_n dS (x_n + pe_n), and from dqt the k_proj / q_proj gradients summed
over the items -- written out in float64 with the defects a segmented backward can have planted in it.  The model runs no code of the
package's hot path (only the oracle, the input generators and the bar), so this file also passes on the commit before the feature: it
says something about the TESTS, not about the kernels.

Unmutated, the model reproduces the yardstick (fp64 autograd through the oracle) on the three parameters that dS and dqt reach, far inside
the bar.  For every GPU case, each mutant moves at least one of them past the bar of tests/test_gpu_ragged_train.py:
  last_token     every item's last token dropped from dS
  neighbour_ml   the softmax weights of item i formed with the (M, L) of item i + 1
  no_delta       dS = p dP
  no_pos_marg    dqt without the positional marginals: sum_n dS x_n
  guide0         the rows of item 0's dctx (and pos_b) taken for every item's dP
The test prints, per case and mutant, the largest error in units of the bar."""
import functools
import math

import numpy as np
import pytest
import torch

import many_item_inputs as mi
import ragged_train_inputs as rt
from oracle import hicom_oracle as orc
from oracle_util import to_t

A = "global_compressor.attn_layer."
G = "global_compressor.readout."
SEEN = (A + "k_proj.weight", A + "q_proj.weight", A + "q_proj.bias")
MUTANTS = ("last_token", "neighbour_ml", "no_delta", "no_pos_marg", "guide0")
NG = mi.NG


def gelu_grad(z):
    return 0.5 * (1 + torch.erf(z / math.sqrt(2))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


@functools.lru_cache(maxsize=None)
def forward_state(id):
    """Per item, in float64: what the forward leaves and what the tail's backward hands the attention backward."""
    c = mi.build(id)
    f64 = torch.float64
    sd = {k: to_t(v, f64) for k, v in c.sd.items() if k.startswith("global_compressor.")}
    Wq, bq, Wk = sd[A + "q_proj.weight"], sd[A + "q_proj.bias"], sd[A + "k_proj.weight"]
    Wv, bv, Wo, bo = sd[A + "v_proj.weight"], sd[A + "v_proj.bias"], sd[A + "out_proj.weight"], sd[A + "out_proj.bias"]
    G0, g0, G2 = sd[G + "0.weight"], sd[G + "0.bias"], sd[G + "2.weight"]
    E = Wq.shape[0]
    nh, hd = E // 128, 128
    items = []
    for i, (ff, _, g, _) in enumerate(c.items):
        T, H, W, _ = ff.shape
        xp = (to_t(ff, f64) + orc.pos_table(T, H, W, E).double()).reshape(-1, E)          # x_n + pe_n
        x = to_t(ff, f64).reshape(-1, E)
        g = to_t(g, f64)
        qp = (Wq @ g + bq).view(nh, hd)
        qt = hd ** -0.5 * torch.einsum("hje,hj->he", Wk.view(nh, hd, E), qp)
        S = qt @ xp.t()
        M = S.max(1).values
        L = torch.exp(S - M[:, None]).sum(1)
        ctx = (torch.exp(S - M[:, None]) / L[:, None]) @ xp
        o = (torch.einsum("hje,he->hj", Wv.view(nh, hd, E), ctx) + bv.view(nh, hd)).reshape(E)
        pre = Wo @ o + bo + g
        z = G0 @ pre + g0
        n_rows = mi.oracle_outputs(id)[i].shape[0]
        dtok = torch.from_numpy(rt.cotangent(id, i, (n_rows, G2.shape[0]))).double()[-NG:].sum(0)
        dpre = G0.t() @ (gelu_grad(z) * (G2.t() @ dtok))
        do = (Wo.t() @ dpre).view(nh, hd)
        dctx = torch.einsum("hje,hj->he", Wv.view(nh, hd, E), do)
        items.append(dict(x=x, xp=xp, g=g, qp=qp, S=S, M=M, L=L, dctx=dctx, delta=(dctx * ctx).sum(1)))
    return dict(items=items, Wk=Wk.view(nh, hd, E), scale=hd ** -0.5, E=E)


def model_grads(id, mutant=None):
    st = forward_state(id)
    items, E = st["items"], st["E"]
    dWk = torch.zeros(E, E, dtype=torch.float64)
    dWq = torch.zeros(E, E, dtype=torch.float64)
    dbq = torch.zeros(E, dtype=torch.float64)
    for i, it in enumerate(items):
        M, L = it["M"], it["L"]
        if mutant == "neighbour_ml":
            nb = items[(i + 1) % len(items)]
            M, L = nb["M"], nb["L"]
        p = torch.exp(it["S"] - M[:, None]) / L[:, None]
        dctx = items[0]["dctx"] if mutant == "guide0" else it["dctx"]
        dP = dctx @ it["xp"].t()
        dS = p * (dP if mutant == "no_delta" else dP - it["delta"][:, None])
        if mutant == "last_token":
            dS[:, -1] = 0
        dqt = dS @ (it["x"] if mutant == "no_pos_marg" else it["xp"])
        dWk += st["scale"] * torch.einsum("hj,he->hje", it["qp"], dqt).reshape(E, E)
        dqp = st["scale"] * torch.einsum("hje,he->hj", st["Wk"], dqt).reshape(E)
        dWq += torch.outer(dqp, it["g"])
        dbq += dqp
    return {SEEN[0]: dWk, SEEN[1]: dWq, SEEN[2]: dbq}


def in_bars(id, grads):
    """{name: max-abs error against the yardstick in units of the parameter's bar} (inf for a gradient that is not finite)."""
    want, bar = rt.yardstick(id), rt.bars(rt.yardstick(id))
    out = {}
    for k in SEEN:
        err = float(np.abs(grads[k].numpy() - want[k]).max())
        out[k] = err / bar[k] if math.isfinite(err) else math.inf
    return out


@pytest.mark.parametrize("id", rt.CASES)
def test_every_mutant_moves_a_gradient_past_the_bar(id):
    clean = in_bars(id, model_grads(id))
    print(f"{id} model vs yardstick: " + "  ".join(f"{k.split('.', 2)[2]} {v:.2e}" for k, v in clean.items()) + "  (bars)")
    assert max(clean.values()) <= 0.05, f"{id}: the model is not the yardstick's backward: {clean}"
    slipped = []
    for mutant in MUTANTS:
        moved = in_bars(id, model_grads(id, mutant))
        print(f"{id} {mutant}: " + "  ".join(f"{k.split('.', 2)[2]} {v:.3g}" for k, v in moved.items()) + "  (bars)")
        if not max(moved.values()) > 1.0:
            slipped.append(f"{mutant}: at most {max(moved.values()):.3g} bars")
    assert not slipped, f"{id}: " + "; ".join(slipped)
