"""Cases, cotangents, yardstick and bar of the ragged training step's tests (tests/test_gpu_ragged_train.py).

Cases: the `ragged` and `batch` entries of tests/many_item_inputs.py at hidden 64 (families `edge`, `edge_outlier`, `item_scales`; a batch
entry runs as split_sizes = (T,) * B on the 4-D view).  Loss: sum_i (out_i * R_i).sum() with seeded fp32 cotangents R_i.
Yardstick: fp64 autograd through oracle.hicom_oracle.projector_forward per item, the gradients summed over the items, computed once per
process.  Bar (tests/test_gpu_backward.py's rule, on the fp32 gradients): 2e-3 of the parameter's largest reference entry, or 1e-5 of the
case's largest entry where that is larger, + 1e-6 absolute."""
import functools

import numpy as np
import torch

import many_item_inputs as mi
from hicom_amd import synth
from oracle import hicom_oracle as orc
from oracle_util import to_t

CASES = [e.id for e in mi.CASES if e.step in ("ragged", "batch") and e.hidden == 64]


def stacked(c):
    """(frames_feature [sum T_i, h, w, D], frames_embed, guides [B, D], split_sizes, modals) of a many_item_inputs case."""
    cat = (lambda a: a.reshape(-1, *a.shape[2:])) if c.entry.step == "batch" else np.concatenate
    return cat(c.ff), cat(c.fe), c.g, list(c.splits), list(c.modals)


def cotangent(id, item, shape):
    rng = np.random.default_rng(synth.seed_of(f"ragged_train:{id}:R{item}") % (2 ** 32))
    return rng.standard_normal(shape).astype(np.float32)


def oracle_grads(cfg, sd, items, newline, cot):
    """{parameter name | "image_newline": fp64 gradient or None} of sum_i (oracle(item i) * cot(i, shape)).sum(); items: (ff, fe, g, modal)."""
    f64 = torch.float64
    sd64 = {k: to_t(v, f64).requires_grad_(True) for k, v in sd.items()}
    nl = None if newline is None else to_t(newline, f64).requires_grad_(True)
    total = 0.0
    for i, (ff, fe, g, modal) in enumerate(items):
        out = orc.projector_forward(cfg, sd64, to_t(ff, f64), to_t(fe, f64), to_t(g, f64), modal, nl)
        total = total + (out * torch.from_numpy(cot(i, tuple(out.shape))).double()).sum()
    total.backward()
    grads = {k: (None if v.grad is None else v.grad.numpy()) for k, v in sd64.items()}
    if nl is not None:
        grads["image_newline"] = nl.grad.numpy()
    return grads


@functools.lru_cache(maxsize=None)
def yardstick(id):
    """The reference gradients of case `id`, computed once per process; callers must not write into them."""
    c = mi.build(id)
    return oracle_grads(c.cfg, c.sd, c.items, None, lambda i, shape: cotangent(id, i, shape))


def bars(want):
    """{name: bar} for the reference gradients `want` of one case."""
    mx_case = max(float(np.abs(v).max()) for v in want.values() if v is not None)
    return {k: max(2e-3 * float(np.abs(v).max()), 1e-5 * mx_case) + 1e-6 for k, v in want.items() if v is not None}


def errors(got, want):
    """{name: max-abs of the fp32 gradient against the reference}; a gradient that is missing counts as infinitely wrong."""
    return {k: (float(np.abs(got[k].double().cpu().numpy() - v).max()) if got.get(k) is not None else float("inf"))
            for k, v in want.items() if v is not None}
