"""Cases, yardsticks and bars of the ragged training step for the k / v adaptor recipe (tests/test_gpu_ragged_train_adapt.py,
tests/test_ragged_train_adapt_power.py).

Cases: the adaptor entries of tests/many_item_inputs.py (MIX6 at side 6, E 1152, hidden 896: adapt_k + adapt_v, adapt_k alone, adapt_v
alone, the heavy-tailed family) and `adaptkv_mix6_no_fe`, the first of them without frames_embed -- that module's table has no such row,
so it is built here from its public functions with the same weights, seeds and family.
Yardstick: fp64 autograd through oracle.hicom_oracle.projector_forward per item, summed (tests/ragged_train_inputs.py and
tests/ragged_train_input_grads.py, imported).  Bars: tests/ragged_train_inputs.bars for parameters, tests/ragged_train_input_grads for the
inputs.  Fallback (the issue's rule): where the LOOP of forward() -- the code this step replaces -- itself exceeds the rule for an entry
on a case, that entry's bar is 1.5 x the loop's measured error against fp64; the margin is for the different summation order of one TN
GEMM over the stacked tokens."""
import functools
from types import SimpleNamespace

import numpy as np

import many_item_inputs as mi
import ragged_train_input_grads as ig
import ragged_train_inputs as rt
from hicom_amd import synth

NO_FE = "adaptkv_mix6_no_fe"
CASES = [e.id for e in mi.entries("adapt")] + [NO_FE]
assert CASES == ["adaptkv_mix6", "adaptk_mix6", "adaptv_mix6", "adaptkv_mix6_outlier", NO_FE]
FALLBACK = 1.5


@functools.lru_cache(maxsize=None)
def build(id):
    """mi.build(id) for the table's entries; NO_FE: adaptkv_mix6 with frames_embed=None (the local spikes then stand on frames_feature)."""
    if id != NO_FE:
        return mi.build(id)
    base = mi.build("adaptkv_mix6")
    e = base.entry._replace(id=id, with_fe=False)
    splits, modals, h, w = e.shape
    xs = [mi.under_family(synth.synth_inputs(T, h, w, mi.D, tag=f"{mi.TAGS[e.step]}:item{b}"), base.sd, e.family, chunks=e.chunks, with_fe=False,
                          shift_g=e.shift_g, shift_l=e.shift_l, power=b) for b, T in enumerate(splits)]
    c = SimpleNamespace(entry=e, cfg=base.cfg, sd=base.sd, newline=None, B=len(splits), splits=list(splits), modals=list(modals))
    c.ff, c.fe, c.g = [x["ff"] for x in xs], None, np.stack([x["g"] for x in xs])
    c.items = [(c.ff[b], None, c.g[b], modals[b]) for b in range(c.B)]
    return c


def stacked(c):
    """(frames_feature [sum T_i, h, w, D], frames_embed or None, guides [B, D], split_sizes, modals)."""
    return np.concatenate(c.ff), (None if c.fe is None else np.concatenate(c.fe)), c.g, list(c.splits), list(c.modals)


@functools.lru_cache(maxsize=None)
def yardstick(id):
    """(parameter gradients, input gradients) in fp64 of case `id`, computed once per process; callers must not write into them."""
    c = build(id)
    return ig.oracle_grads(c.cfg, c.sd, c.items, lambda i, shape: rt.cotangent(id, i, shape), with_fe=c.fe is not None)


def fallback_bar(bar, loop_err):
    """The bar of one entry: the rule's, or 1.5 x the loop's own error where the loop exceeds the rule."""
    return bar if (loop_err is None or not loop_err > bar) else FALLBACK * loop_err
