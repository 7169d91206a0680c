"""The cases of HIComProjector.forward_ragged_multi_guide (B items of unequal length, item i with its own Q_i guides) under the input
families of tests/many_item_inputs.py, and the oracle's outputs for them, computed once per process and per (item, guide) pair.

An item with Q_i guides is spiked as the one clip of forward_multi_guide is (many_item_inputs.under_family with g = [Q_i, D]: the sums
over the item's guides of the global and the local spike), item b of `item_scales` is scaled by 4^b with all its guides.  Whether the
families do on these cases what they are for is asserted on the oracle alone by tests/test_ragged_multi_guide_power.py; the GPU tests
(tests/test_gpu_ragged_multi_guide.py) take their cases from the same table.

The two mixes are the smallest at which the step can go wrong:
  MIX6  grid 6 x 6, splits (1, 4, 1, 8, 1), guide counts (1, 3, 5, 2, 4): remainder groups of 1, 2 and 3 of the local kernel, one item
        across the group of four and the 32-row pass (Q = 5: 45 rows), a masked tail tile in the 36-token items, a 1-frame "video"
  MIX9  grid 9 x 9, splits (1, 4), counts (4, 8): 81 tokens end in a tail tile; Q = 8 is 72 rows, three passes, the last part-filled
"""
import functools
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np

import cases
import many_item_inputs as mi
from hicom_amd import synth
from oracle import hicom_oracle as orc
from oracle_util import to_t

D = cases.D
NG = mi.NG
TAG = "raggedmultiguide"
ITEM_TAG = mi.TAGS["ragged"]         # tokens (and each item's first guide) by the seeds of the ragged step's cases
MIX6 = ((1, 4, 1, 8, 1), ("image", "video", "video", "video", "image"), 6, 6, (1, 3, 5, 2, 4))
MIX9 = ((1, 4), ("image", "video"), 9, 9, (4, 8))


class Entry(NamedTuple):
    id: str
    shape: tuple                        # (splits, modals, h, w, guide counts)
    family: str
    chunks: Optional[int] = None
    hidden: int = 64
    with_fe: bool = True
    newline: Optional[str] = None       # mm_newline_position of a case with image_newline, None: no newline token
    shift_g: float = 5.0
    shift_l: float = 4.0


CASES = (
    Entry("rmg_mix6", MIX6, "edge"),
    Entry("rmg_mix6_chunks1", MIX6, "edge", chunks=1),
    Entry("rmg_mix6_chunks3", MIX6, "edge", chunks=3),
    Entry("rmg_mix6_chunks18", MIX6, "edge", chunks=18),
    Entry("rmg_mix9", MIX9, "edge"),
    Entry("rmg_mix9_chunks3", MIX9, "edge", chunks=3),
    Entry("rmg_mix6_newline", MIX6, "edge", newline="no_token"),     # (the default position: only the images carry a newline row)
    Entry("rmg_mix6_newline_grid", MIX6, "edge", newline="grid"),
    Entry("rmg_mix6_no_fe", MIX6, "edge", with_fe=False),
    Entry("rmg_mix6_h896", MIX6, "edge", hidden=896),
    Entry("rmg_mix6_outlier", MIX6, "edge_outlier", shift_g=8.0, shift_l=12.0),
    Entry("rmg_mix9_scales", MIX9, "item_scales"),
)
BY_ID = {e.id: e for e in CASES}
assert len(BY_ID) == len(CASES)


@functools.lru_cache(maxsize=None)
def _weights(hidden, newline):
    over = {"hidden_size": hidden}
    if newline is not None:
        over["mm_newline_position"] = newline
    cfg = SimpleNamespace(**{**cases.DEFAULT_CFG, **over})
    return cfg, mi._weights("ragged", None, hidden)[1]          # the ragged step's weights (the newline position is no weight)


@functools.lru_cache(maxsize=None)
def _torch_sd(hidden, newline):
    return {k: to_t(v) for k, v in _weights(hidden, newline)[1].items()}


def guide(i, q):
    """Guide 0 of item i is the ragged case's guide of that item: a single-guide item is the ragged step's item."""
    return synth.synth_inputs(1, 3, 3, D, tag=f"{ITEM_TAG}:item{i}" if q == 0 else f"{TAG}:item{i}:guide{q}")["g"]


@functools.lru_cache(maxsize=None)
def build(id):
    """The case of entry `id`: cfg, sd, newline, splits, modals, counts, the per-item arrays ff / fe (lists) and g ([Q_i, D] per item),
    and `pairs`, the list of (item, guide) in the call's order."""
    e = BY_ID[id]
    splits, modals, h, w, counts = e.shape
    cfg, sd = _weights(e.hidden, e.newline)
    outliers = mi.OUTLIERS if e.family == "edge_outlier" else None
    c = SimpleNamespace(entry=e, cfg=cfg, sd=sd, splits=list(splits), modals=list(modals), counts=list(counts), h=h, w=w, B=len(splits))
    c.newline = synth.normal_like((cfg.hidden_size,), synth.seed_of(f"{TAG}:newline")) if e.newline is not None else None
    c.ff, c.fe, c.g = [], [], []
    for i, (T, Q) in enumerate(zip(splits, counts)):
        x = synth.synth_inputs(T, h, w, D, tag=f"{ITEM_TAG}:item{i}", outliers=outliers)
        x["g"] = np.stack([guide(i, q) for q in range(Q)])
        x = mi.under_family(x, sd, e.family, chunks=e.chunks, with_fe=e.with_fe, shift_g=e.shift_g, shift_l=e.shift_l, power=i)
        c.ff.append(x["ff"]); c.fe.append(x["fe"]); c.g.append(x["g"])
    c.pairs = [(i, q) for i in range(c.B) for q in range(counts[i])]
    return c


def run_oracle(c, item, q, ff=None, g=None):
    """The oracle on item `item` alone with its guide q (ff / g: replacements of the item's tokens / of that guide)."""
    e = c.entry
    ff = c.ff[item] if ff is None else ff
    fe = c.fe[item] if e.with_fe else None
    g = c.g[item][q] if g is None else g
    return orc.projector_forward(c.cfg, _torch_sd(e.hidden, e.newline), to_t(ff), to_t(fe), to_t(g), c.modals[item], to_t(c.newline)).numpy()


@functools.lru_cache(maxsize=None)
def oracle_outputs(id):
    """{(item, guide): the oracle's output}, computed once per process; callers must not write into it."""
    c = build(id)
    outs = {p: run_oracle(c, *p) for p in c.pairs}
    for o in outs.values():
        o.setflags(write=False)
    return outs


def regions(c, item, rows):
    """{region: row indices} of one pair's `rows` packed rows: the local token rows, the newline rows, the NG global rows."""
    nl = set()
    if c.newline is not None:
        proj = _layout_module(c.entry.hidden, c.entry.newline)
        T, modal = c.splits[item], c.modals[item]
        at, ay, ax = proj.local_compressor.tilings(T, c.h, c.w, modal)
        nl = set(proj._layout((at.nwin, ay.nwin, ax.nwin), modal, True, False).newline_rows)
    loc = [r for r in range(rows - NG) if r not in nl]
    return {"local": loc, "newline": sorted(nl), "global": list(range(rows - NG, rows))}


@functools.lru_cache(maxsize=None)
def _layout_module(hidden, newline):
    import hicom_amd
    return hicom_amd.build_vision_projector(_weights(hidden, newline)[0])


def check_pair(c, what, got, want, item):
    """Prints the per-region max-abs of one pair against the oracle and returns the violations of its bar (many_item_inputs.tolerance:
    1e-3, HEAVY_REL x max |oracle out| under `edge_outlier`) as strings."""
    tol = mi.tolerance(c.entry, want)
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    errs = {r: float(d[idx].max()) for r, idx in regions(c, item, want.shape[0]).items() if idx}
    print(f"{c.entry.id} [{c.entry.family}] {what}: " + "  ".join(f"{r} {v:.3e}" for r, v in errs.items())
          + f"  (bar {tol:.3e}, max|out| {np.abs(want).max():.3f})")
    return [f"{what} {r} rows: {v:.3e} > {tol:.3e}" for r, v in errs.items() if not v <= tol]
