"""The cases tests/test_gpu_prepared_clip.py holds to the oracle (prepare_clip + forward_prepared: ONE clip under the k / v adaptor recipes,
Q guides per call), under the input families of tests/many_item_inputs.py, and the oracle's outputs for them (computed once per process).

Families, weights law (the adaptkv state dict of the "adapt" step: a recipe with fewer adaptors loads the part it has; alphas = 0.5) and
tolerance rule are many_item_inputs'; only the table is this file's.  tests/test_prepared_clip_power.py asserts, on the oracle alone, that
every wrong softmax of tests/softmax_mutants.py moves every region of every (case, guide) here by at least 4 bars.

Shapes: the smallest at which the window kernel for several guides can go wrong -- 36-token windows (6 x 6, T = 4 and T = 8: one and two
windows along t), 9-token windows (images), a 9 x 9 image with newline rows, keys from frames_feature.  Q: the kernel walks a window once
per group of guides and the remainder group is its own instantiation, so the Q values cover a full group, every remainder and three groups
for every group size up to 4: {1, 2, 3, 4, 5, 6, 7, 9}.  Width 1152, hidden 896."""
import functools
from types import SimpleNamespace

import numpy as np

import many_item_inputs as mi
from hicom_amd import synth
from oracle import hicom_oracle as orc
from oracle_util import to_t

D, NG, HIDDEN = mi.D, mi.NG, 896
TAG = "preparedclip"
Entry = mi.Entry

# shape: (Q, T, h, w, modal); an adapted key is (1 - a) fe + a LN(MLP(fe)), a = 0.5: shift_l is doubled where the keys are adapted
# (many_item_inputs.CASES, the "adapt" entries)
CASES = (
    Entry("pc_video_T4_Q4", "prepared", (4, 4, 6, 6, "video"), "edge", recipe=mi.ADAPTKV, hidden=HIDDEN, shift_l=8.0),
    Entry("pc_video_T8_Q9", "prepared", (9, 8, 6, 6, "video"), "edge", recipe=mi.ADAPTKV, hidden=HIDDEN, shift_l=8.0),
    Entry("pc_image_Q3", "prepared", (3, 1, 6, 6, "image"), "edge", recipe=mi.ADAPTKV, hidden=HIDDEN, shift_l=8.0),
    Entry("pc_image9_newline_Q5", "prepared", (5, 1, 9, 9, "image"), "edge", recipe=mi.ADAPTKV, hidden=HIDDEN, shift_l=8.0),
    Entry("pc_video_T4_no_fe_Q6", "prepared", (6, 4, 6, 6, "video"), "edge", recipe=mi.ADAPTKV, hidden=HIDDEN, with_fe=False, shift_l=8.0),
    Entry("pc_video_T4_adaptk_Q7", "prepared", (7, 4, 6, 6, "video"), "edge", recipe=mi.ADAPTK, hidden=HIDDEN, shift_l=8.0),
    Entry("pc_video_T4_adaptv_Q2", "prepared", (2, 4, 6, 6, "video"), "edge", recipe=mi.ADAPTV, hidden=HIDDEN),
    Entry("pc_video_T4_adaptv_Q1", "prepared", (1, 4, 6, 6, "video"), "edge", recipe=mi.ADAPTV, hidden=HIDDEN),
    Entry("pc_video_T4_outlier_Q3", "prepared", (3, 4, 6, 6, "video"), "edge_outlier", recipe=mi.ADAPTKV, hidden=HIDDEN, shift_g=8.0, shift_l=24.0),
)
BY_ID = {e.id: e for e in CASES}
NEWLINE = ("pc_image9_newline_Q5",)                             # cases with mm_newline_position = "grid": a newline row behind every row of windows


@functools.lru_cache(maxsize=None)
def build(id, recipe=None):
    """The case of entry `id`: cfg, sd, newline, Q, modal, the clip ff / fe (None without frames_embed), the guides g [Q, D].  `recipe`:
    the same inputs and the same weights under another recipe (the parts of the adaptkv state dict it has)."""
    e = BY_ID[id]
    cfg, sd = mi._weights("adapt", recipe or e.recipe, e.hidden)
    newline = None
    if id in NEWLINE:
        cfg = SimpleNamespace(**{**vars(cfg), "mm_newline_position": "grid"})
        newline = synth.normal_like((cfg.hidden_size,), synth.seed_of(f"{TAG}:newline"))
    Q, T, h, w, modal = e.shape
    clip = synth.synth_inputs(T, h, w, D, tag=f"{TAG}:clip", outliers=mi.OUTLIERS if e.family == "edge_outlier" else None)
    clip["g"] = np.stack([synth.synth_inputs(1, 3, 3, D, tag=f"{TAG}:guide{q}")["g"] for q in range(Q)])
    x = mi.under_family(clip, mi._weights("adapt", e.recipe, e.hidden)[1], e.family, chunks=e.chunks, with_fe=e.with_fe, shift_g=e.shift_g,
                        shift_l=e.shift_l)
    return SimpleNamespace(entry=e, cfg=cfg, sd=sd, newline=newline, Q=Q, modal=modal, ff=x["ff"], fe=x["fe"], g=x["g"], n_tokens=T * h * w)


def run_oracle(c, q, sd=None, g=None):
    """The oracle on the clip with guide q (or the guide row `g`); sd: other weights (numpy) than the case's."""
    tsd = {k: to_t(v) for k, v in (sd or c.sd).items()}
    return orc.projector_forward(c.cfg, tsd, to_t(c.ff), to_t(c.fe), to_t(c.g[q] if g is None else g), c.modal, to_t(c.newline)).numpy()


@functools.lru_cache(maxsize=None)
def oracle_outputs(id, recipe=None):
    """The oracle's output per guide, computed once per process; callers must not write into it."""
    c = build(id, recipe)
    outs = [run_oracle(c, q) for q in range(c.Q)]
    for o in outs:
        o.setflags(write=False)
    return outs
