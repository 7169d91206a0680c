"""The cases tests/test_gpu_prepared_many.py holds to the oracle (HIComProjector.forward_prepared_many: B prepared clips, clip i with its
own Q_i guides, one call), under the input families of tests/many_item_inputs.py, and the oracle's outputs for them, computed once per
process and per (clip, guide) pair.

Families, weights law (the adaptkv state dict of the "adapt" step at hidden 896: a recipe with fewer adaptors, and the plain recipe, load
the part they have; alphas = 0.5) and tolerance rule are many_item_inputs'.  A clip with Q_i guides is spiked as the one clip of
forward_multi_guide is (under_family with g = [Q_i, D]).  An adapted key is (1 - a) fe + a LN(MLP(fe)), a = 0.5: shift_l is doubled
where the keys are adapted.  tests/test_prepared_many_power.py asserts, on the oracle alone, that every wrong softmax of
tests/softmax_mutants.py moves every region of every pair here by at least 4 bars.

The two mixes are those of tests/ragged_multi_guide_inputs.py, the smallest at which the step can go wrong:
  MIX6  grid 6 x 6, frames (1, 4, 1, 8, 1), guide counts (1, 3, 5, 2, 4): remainder groups of 1, 2 and 3 of the window kernels, one clip
        across the group of four and the 32-row pass (Q = 5: 45 rows), a masked tail tile in the 36-token clips, a 1-frame "video"
  MIX9  grid 9 x 9, frames (1, 4), counts (4, 8): 81 tokens end in a tail tile; Q = 8 is 72 rows, three passes, the last part-filled
"""
import functools
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np

import many_item_inputs as mi
import ragged_multi_guide_inputs as ri
from hicom_amd import synth
from oracle import hicom_oracle as orc
from oracle_util import to_t

D, NG, HIDDEN = mi.D, mi.NG, 896
TAG = "preparedmany"
MIX6, MIX9 = ri.MIX6, ri.MIX9


class Entry(NamedTuple):
    id: str
    shape: tuple                        # (frames per clip, modals, h, w, guide counts)
    family: str
    recipe: str = mi.ADAPTKV
    chunks: Optional[int] = None
    with_fe: bool = True
    newline: Optional[str] = None       # mm_newline_position of a case with image_newline, None: no newline token
    shift_g: float = 5.0
    shift_l: float = 8.0
    hidden: int = HIDDEN


CASES = (
    Entry("pm_mix6_adaptkv", MIX6, "edge"),
    Entry("pm_mix6_adaptk", MIX6, "edge", recipe=mi.ADAPTK),
    Entry("pm_mix6_adaptv", MIX6, "edge", recipe=mi.ADAPTV, shift_l=4.0),
    Entry("pm_mix6_no_fe", MIX6, "edge", with_fe=False),
    Entry("pm_mix6_newline_grid", MIX6, "edge", newline="grid"),
    Entry("pm_mix6_outlier", MIX6, "edge_outlier", shift_g=8.0, shift_l=24.0),
    Entry("pm_mix9_chunks3", MIX9, "edge", chunks=3),
    Entry("pm_mix6_plain", MIX6, "edge", recipe=mi.PLAIN, shift_l=4.0),
)
BY_ID = {e.id: e for e in CASES}
assert len(BY_ID) == len(CASES)


@functools.lru_cache(maxsize=None)
def _weights(recipe, newline):
    cfg, sd = mi._weights("adapt", recipe, HIDDEN)
    if newline is not None:
        cfg = SimpleNamespace(**{**vars(cfg), "mm_newline_position": newline})
    return cfg, sd


@functools.lru_cache(maxsize=None)
def _torch_sd(recipe):
    return {k: to_t(v) for k, v in _weights(recipe, None)[1].items()}


@functools.lru_cache(maxsize=None)
def build(id, recipe=None):
    """The case of entry `id`: cfg, sd, newline, frames, modals, counts, the per-clip arrays ff / fe (lists; fe[i] None without
    frames_embed) and g ([Q_i, D] per clip), and `pairs`, the list of (clip, guide) in the call's order.  `recipe`: the same inputs and
    the same weights under another recipe (the parts of the adaptkv state dict it has)."""
    e = BY_ID[id]
    frames, modals, h, w, counts = e.shape
    cfg, sd = _weights(recipe or e.recipe, e.newline)
    spike_sd = _weights(e.recipe, None)[1]
    outliers = mi.OUTLIERS if e.family == "edge_outlier" else None
    c = SimpleNamespace(entry=e, recipe=recipe or e.recipe, cfg=cfg, sd=sd, frames=list(frames), modals=list(modals), counts=list(counts), h=h, w=w,
                        B=len(frames))
    c.newline = synth.normal_like((cfg.hidden_size,), synth.seed_of(f"{TAG}:newline")) if e.newline is not None else None
    c.ff, c.fe, c.g = [], [], []
    for i, (T, Q) in enumerate(zip(frames, counts)):
        x = synth.synth_inputs(T, h, w, D, tag=f"{TAG}:item{i}", outliers=outliers)
        x["g"] = np.stack([synth.synth_inputs(1, 3, 3, D, tag=f"{TAG}:item{i}:guide{q}")["g"] for q in range(Q)])
        x = mi.under_family(x, spike_sd, e.family, chunks=e.chunks, with_fe=e.with_fe, shift_g=e.shift_g, shift_l=e.shift_l)
        c.ff.append(x["ff"]); c.fe.append(x["fe"]); c.g.append(x["g"])
    c.pairs = [(i, q) for i in range(c.B) for q in range(counts[i])]
    return c


def run_oracle(c, item, q, sd=None, ff=None, g=None):
    """The oracle on clip `item` alone with its guide q (sd: other weights (numpy) than the case's; ff / g: replacements of the clip's
    tokens / of that guide)."""
    tsd = _torch_sd(c.recipe) if sd is None else {k: to_t(v) for k, v in sd.items()}
    return orc.projector_forward(c.cfg, tsd, to_t(c.ff[item] if ff is None else ff), to_t(c.fe[item]), to_t(c.g[item][q] if g is None else g),
                                 c.modals[item], to_t(c.newline)).numpy()


@functools.lru_cache(maxsize=None)
def oracle_outputs(id, recipe=None):
    """{(clip, guide): the oracle's output}, computed once per process; callers must not write into it."""
    c = build(id, recipe)
    outs = {p: run_oracle(c, *p) for p in c.pairs}
    for o in outs.values():
        o.setflags(write=False)
    return outs


@functools.lru_cache(maxsize=None)
def _layout_module(recipe, newline):
    import hicom_amd
    return hicom_amd.build_vision_projector(_weights(recipe, newline)[0])


def regions(c, item, rows):
    """{region: row indices} of one pair's `rows` packed rows: the local token rows, the newline rows, the NG global rows."""
    nl = set()
    if c.newline is not None:
        proj = _layout_module(c.recipe, c.entry.newline)
        T, modal = c.frames[item], c.modals[item]
        at, ay, ax = proj.local_compressor.tilings(T, c.h, c.w, modal)
        nl = set(proj._layout((at.nwin, ay.nwin, ax.nwin), modal, True, False).newline_rows)
    loc = [r for r in range(rows - NG) if r not in nl]
    return {"local": loc, "newline": sorted(nl), "global": list(range(rows - NG, rows))}


def check_pair(c, what, got, want, item):
    """Prints the per-region max-abs of one pair against the oracle and returns the violations of its bar (many_item_inputs.tolerance:
    1e-3, HEAVY_REL x max |oracle out| under `edge_outlier`) as strings."""
    tol = mi.tolerance(c.entry, want)
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    errs = {r: float(d[idx].max()) for r, idx in regions(c, item, want.shape[0]).items() if idx}
    print(f"{c.entry.id} [{c.entry.family}] {what}: " + "  ".join(f"{r} {v:.3e}" for r, v in errs.items())
          + f"  (bar {tol:.3e}, max|out| {np.abs(want).max():.3f})")
    return [f"{what} {r} rows: {v:.3e} > {tol:.3e}" for r, v in errs.items() if not v <= tol]
