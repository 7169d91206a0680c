"""Cases, cotangents and yardstick of the ragged multi-guide training step's tests (tests/test_gpu_ragged_multi_guide_train.py,
tests/test_ragged_multi_guide_train_power.py).

Cases: entries of tests/ragged_multi_guide_inputs.py at hidden 64 (MIX6 and MIX9, chunk overrides 1, 3 and 18, without frames_embed,
`edge_outlier`, `item_scales`; the two newline cases apart).  Loss: sum over the M = sum Q_i pairs of (out_pair * R_pair).sum() with seeded
fp32 cotangents R_pair, pairs numbered in the call's order.  Yardstick: fp64 autograd through the oracle per pair
(ragged_train_inputs.oracle_grads with the pair list as its items), the gradients summed over the pairs, computed once per process.
Bar: ragged_train_inputs.bars, the rule of tests/test_gpu_backward.py."""
import functools

import numpy as np

import ragged_multi_guide_inputs as ri
import ragged_train_inputs as rt
from hicom_amd import synth

CASES = ["rmg_mix6", "rmg_mix6_chunks1", "rmg_mix6_chunks3", "rmg_mix6_chunks18", "rmg_mix9", "rmg_mix9_chunks3", "rmg_mix6_no_fe", "rmg_mix6_outlier",
         "rmg_mix9_scales"]
NEWLINE_CASES = ["rmg_mix6_newline", "rmg_mix6_newline_grid"]


def cotangent(id, pair, shape):
    """The cotangent of pair number `pair` (the call's order) of case `id`."""
    rng = np.random.default_rng(synth.seed_of(f"ragged_multi_guide_train:{id}:R{pair}") % (2 ** 32))
    return rng.standard_normal(shape).astype(np.float32)


def pair_items(c):
    """The pair list as oracle_grads' items: (ff, fe, g, modal) per (item, guide)."""
    return [(c.ff[i], c.fe[i] if c.entry.with_fe else None, c.g[i][q], c.modals[i]) for i, q in c.pairs]


@functools.lru_cache(maxsize=None)
def yardstick(id):
    """The reference gradients of case `id` (with "image_newline" where the case has one), computed once per process; callers must not
    write into them."""
    c = ri.build(id)
    return rt.oracle_grads(c.cfg, c.sd, pair_items(c), c.newline, lambda k, shape: cotangent(id, k, shape))
