"""Wrong-softmax oracles (CPU, test infrastructure): `with wrong_softmax(name):` runs oracle.hicom_oracle with one of its two softmaxes
(mha: the global stage; local_context: the window attention) replaced by a subtly wrong one, through the oracle's module-level names
`softmax_mha` / `softmax_local` (and, for "pos_off", `global_forward`).  torch itself is never patched, and the oracle's names are put
back when the block ends, however it ends.

What they are for: tests/test_many_item_power.py asserts that every input family of tests/many_item_inputs.py moves the oracle's output
by several tolerances under each replacement, so that a kernel wrong in the same way cannot stay inside the tolerance of the GPU tests.
Each replacement stands for a fault a segmented online-softmax kernel can have:

  uniform          the logits never reach the exponent
  scale_0.9        a wrong logit scale (1/sqrt(d), a folded constant)
  drop_last        the item's / the window's last key lost: a tail-tile mask or a loop bound one short (weights NOT renormalised)
  drop_first       the first key lost: a pipeline prologue that skips its first tile or token
  drop_tile_edge   key 16 of the global stage lost: the first token behind the first 16-token tile boundary
  pos_off          the global stage without its positional term
"""
import contextlib
import functools

import torch

from oracle import hicom_oracle as orc

LOCAL, GLOBAL = "local", "global"


def _uniform(s, dim=-1):
    return torch.softmax(s * 0, dim=dim)


def _scaled(s, dim=-1):
    return torch.softmax(s * 0.9, dim=dim)


def _drop(index):
    def f(s, dim=-1):
        assert dim == -1
        p = torch.softmax(s, dim=dim).clone()
        if -p.shape[-1] <= index < p.shape[-1]:
            p[..., index] = 0
        return p
    return f


# name -> (replacement of softmax_mha or None, replacement of softmax_local or None, use_pos_emb of the global stage)
_TABLE = {
    "uniform": (_uniform, _uniform, True),
    "scale_0.9": (_scaled, _scaled, True),
    "drop_last": (_drop(-1), _drop(-1), True),
    "drop_first": (_drop(0), _drop(0), True),
    "drop_tile_edge": (_drop(16), None, True),
    "pos_off": (None, None, False),
}
MUTANTS = tuple(_TABLE)


def regions(name, n_tokens):
    """The output regions replacement `name` can touch on an item of n_tokens tokens."""
    mha, local, pos = _TABLE[name]
    if name == "drop_tile_edge" and n_tokens <= 16:
        return ()
    return ((LOCAL,) if local is not None else ()) + ((GLOBAL,) if mha is not None or not pos else ())


@contextlib.contextmanager
def wrong_softmax(name):
    mha, local, pos = _TABLE[name]
    saved = orc.softmax_mha, orc.softmax_local, orc.global_forward
    try:
        if mha is not None:
            orc.softmax_mha = mha
        if local is not None:
            orc.softmax_local = local
        if not pos:
            orc.global_forward = functools.partial(saved[2], use_pos_emb=False)
        yield
    finally:
        orc.softmax_mha, orc.softmax_local, orc.global_forward = saved
