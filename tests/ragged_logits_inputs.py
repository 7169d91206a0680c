"""Inputs and references of the logits form of the ragged step and its training step (tests/test_gpu_ragged_logits.py,
tests/test_ragged_logits_power.py), on the cases, cotangents and yardsticks of tests/ragged_train_inputs.py and
tests/ragged_train_input_grads.py (imported, not edited).

Scores: what the GPU is handed is fp32(frames_embed_n . guide_item), the dot product formed in float64 on the host from the case's bf16
values, stacked [sum T_i, H, W].  The oracle, run with that frames_embed, is then the reference with nothing changed under oracle/.

References, from the oracle's fp64 autograd (ragged_train_input_grads.yardstick), computed once per process:
  d local_logits   in the plain recipe the loss depends on frames_embed only through l_n = fe_n . g, so d fe_n = dl_n g and
                   dl_n = (d_fe[n] . g) / (g . g);
  d guide_embeds   the oracle's total minus sum_n dl_n fe_n, the local share: in the logits form it flows through the scores into the
                   caller's graph, and the step hands back the global share only.
Bars: d local_logits per item under ragged_train_input_grads.item_bar on the item's own largest reference entry (the rule of the bf16 input
gradients: the fp32 result gets no wider bar than they do), d guide_embeds under ragged_train_input_grads.guide_bar."""
import functools

import numpy as np

import many_item_inputs as mi
import ragged_train_input_grads as ig
import ragged_train_inputs as rt

CASES = rt.CASES


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scores(id):
    """fp32 [sum T_i, H, W]: frames_embed_n . guide of the token's item, summed in float64, rounded once."""
    c = mi.build(id)
    per = [(fe.astype(np.float64).reshape(-1, fe.shape[-1]) @ g.astype(np.float64)).astype(np.float32).reshape(fe.shape[:3]) for _, fe, g, _ in c.items]
    return frozen(np.concatenate(per))


@functools.lru_cache(maxsize=None)
def dl_reference(id):
    """Per item, float64 [T_i, H, W]: dl_n = (d_fe[n] . g) / (g . g)."""
    c = mi.build(id)
    _, want_in = ig.yardstick(id)
    out = []
    for (_, _, g, _), dfe in zip(c.items, want_in["frames_embed"]):
        g = g.astype(np.float64)
        out.append(frozen((dfe.reshape(-1, g.shape[0]) @ g / (g @ g)).reshape(dfe.shape[:3])))
    return out


@functools.lru_cache(maxsize=None)
def dguide_reference(id):
    """float64 [B, E]: the oracle's d guide_embeds minus sum_n dl_n fe_n per item (the share that flows through the scores)."""
    c = mi.build(id)
    _, want_in = ig.yardstick(id)
    rows = []
    for (_, fe, _, _), dl, dg in zip(c.items, dl_reference(id), want_in["guide_embeds"]):
        rows.append(dg - dl.reshape(-1) @ fe.astype(np.float64).reshape(-1, fe.shape[-1]))
    return frozen(np.stack(rows))


def dl_errors(got, id, splits):
    """[(max-abs error, bar)] per item of a stacked d local_logits `got` [sum T_i, H, W] (a torch tensor) against dl_reference."""
    out, t0 = [], 0
    for T, want in zip(splits, dl_reference(id)):
        g = got[t0:t0 + T].double().cpu().numpy().reshape(want.shape)
        out.append((float(np.abs(g - want).max()), ig.item_bar(want)))
        t0 += T
    return out
