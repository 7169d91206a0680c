"""Yardstick and bars of the ragged training step's INPUT gradients (tests/test_gpu_ragged_train_inputs.py): fp64 autograd through
oracle.hicom_oracle.projector_forward per item with frames_feature, frames_embed and guide_embeds requiring grad, on the cases, cotangents
and parameter bars of tests/ragged_train_inputs.py (imported, not edited).

Bars, the project's own:
  parameters       ragged_train_inputs.bars
  d guide_embeds   the same rule on the fp32 [B, E] gradient, on its own largest entry
  bf16 inputs      per item, 2^-7 mx + 2e-3 mx + 1e-6 with mx the item's largest reference entry (tests/test_gpu_backward.py:243-244): one
                   rounding to bf16 of an entry up to mx, + the gradient tolerance
  sums             per item, |sum got - sum want| <= 2e-2 sum |want| + 1e-6 (tests/test_gpu_backward.py:245)"""
import functools

import numpy as np
import torch

import many_item_inputs as mi
import ragged_train_inputs as rt
from oracle import hicom_oracle as orc
from oracle_util import to_t

INPUTS = ("frames_feature", "frames_embed", "guide_embeds")


def oracle_grads(cfg, sd, items, cot, with_fe=True):
    """({parameter name: fp64 gradient or None}, {"frames_feature": [per item], "frames_embed": [per item] or None, "guide_embeds": [B, E]})
    of sum_i (oracle(item i) * cot(i, shape)).sum(); items: (ff, fe, g, modal)."""
    f64 = torch.float64
    sd64 = {k: to_t(v, f64).requires_grad_(True) for k, v in sd.items()}
    leaves = []
    total = 0.0
    for i, (ff, fe, g, modal) in enumerate(items):
        x = to_t(ff, f64).requires_grad_(True)
        k = to_t(fe, f64).requires_grad_(True) if with_fe else None
        q = to_t(g, f64).requires_grad_(True)
        leaves.append((x, k, q))
        out = orc.projector_forward(cfg, sd64, x, k, q, modal, None)
        total = total + (out * torch.from_numpy(cot(i, tuple(out.shape))).double()).sum()
    total.backward()
    params = {k: (None if v.grad is None else v.grad.numpy()) for k, v in sd64.items()}
    inputs = {"frames_feature": [x.grad.numpy() for x, _, _ in leaves],
              "frames_embed": [k.grad.numpy() for _, k, _ in leaves] if with_fe else None,
              "guide_embeds": np.stack([q.grad.numpy() for _, _, q in leaves])}
    return params, inputs


@functools.lru_cache(maxsize=None)
def yardstick(id, with_fe=True):
    """The reference gradients of case `id`, computed once per process; callers must not write into them."""
    c = mi.build(id)
    return oracle_grads(c.cfg, c.sd, c.items, lambda i, shape: rt.cotangent(id, i, shape), with_fe)


def guide_bar(params, dg):
    return rt.bars({**params, "__guide_embeds__": dg})["__guide_embeds__"]


def item_bar(want):
    mx = float(np.abs(want).max())
    return 2 ** -7 * mx + 2e-3 * mx + 1e-6


def item_errors(got, want_items, splits):
    """[(max-abs error, bar, |sum error|, sum bar)] per item of a stacked bf16 gradient `got` [sum T_i, ...] against the per-item references."""
    out, t0 = [], 0
    for T, want in zip(splits, want_items):
        g = got[t0:t0 + T].double().cpu().numpy().reshape(want.shape)
        out.append((float(np.abs(g - want).max()), item_bar(want), abs(float(g.sum()) - float(want.sum())), 2e-2 * float(np.abs(want).sum()) + 1e-6))
        t0 += T
    return out
