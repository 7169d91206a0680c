"""Input families for the many-item steps (forward_batch, forward_ragged, their k / v adaptor forms, forward_multi_guide), the table of
cases the GPU tests hold to the oracle under them, and the oracle's outputs for those cases (computed once per process).

Why families: on the flat law (N(0, 1) tokens, N(0, .02) weights) both softmaxes of the compressor are nearly uniform, and an output
within 1e-3 of the oracle says little about the online softmax that produced it: a global stage with every logit 10 % off, or one that
loses an item's last token, moves the output by 5e-4 .. 7e-4 (tests/test_many_item_power.py prints the figures).  The families put
softmax mass, on purpose, where a segmented kernel can go wrong:

  edge          at the item's tokens n in {0, 15, 16, N - 1} (its first token, both sides of the first 16-token tile boundary, its last
                token) and, 0.6 times as high (spike_weight), at both sides of every chunk boundary when the step is run with chunks=:
                    ff[n] += a u,  u = W_k^T (W_q g + b_q) of the global attention, a such that the mean per-head logit shift is shift_g;
                    fe[n] += shift_l sqrt(D) g / (g . g): the local logit g . fe[n] / sqrt(D) rises by shift_l (on ff when there is no
                    frames_embed: the keys are frames_feature then).
                Several guides on one clip (forward_multi_guide): the sums over the guides of both terms.
  edge_outlier  `edge` on top of heavy-tailed channels, outliers = (12, 60.0) as the golden cases G13*.  The channels spread the flat
                logits over several units (global, per head) resp. tens of units (local), so the spikes are higher here (the table's
                shift_g / shift_l) and stand on levelled rows (below).
  item_scales   item b's tokens and guide x 4^b under `edge` (a power of two: exact in bf16): every logit of item b is 16^b times item
                0's, the running maxima of neighbouring items differ by that factor inside one launch, and each item is compared with
                the oracle of the scaled item.  Levelled rows as well.

Levelled rows (LEVELLED): a softmax over scaled or heavy-tailed logits is close to one-hot, and which of the spiked tokens won would be
left to the flat rows under the spikes -- the family would then test one of the edges per head, by chance.  So, in these two families,
the part of a spiked token's flat row that its own logits read (global: W_k,h^T q_h per head and guide; local: the guide) is replaced by
that of the item's mean token: every spiked token stands exactly its spike above the item's average logit, the spiked tokens share the
mass (up to their positional terms), and their VALUES still differ by the rest of their flat rows.

All values are bf16-representable (synth.round_to_bf16).  Whether a family does what it is for is asserted, on the CPU and on the
oracle alone, by tests/test_many_item_power.py for every entry of CASES; the GPU tests take their cases from the same table.
"""
import functools
import math
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np

import cases
from hicom_amd import synth
from oracle import hicom_oracle as orc
from oracle_util import to_t

D = cases.D
NG = 32                                                         # global rows per item (.._global32)
TOL = 1e-3                                                      # the bar of every forward path (tests/test_gpu_parity.py)
HEAVY_REL = 1e-3                                                # ... and of its heavy-tailed cases: HEAVY_REL x max |oracle out|
OUTLIERS = (12, 60.0)
PLAIN, ADAPTKV, ADAPTK, ADAPTV = "local43_global32", "local43_adaptkv_global32", "local43_adaptk_global32", "local43_adaptv_global32"
FAMILIES = ("edge", "edge_outlier", "item_scales")
LEVELLED = ("edge_outlier", "item_scales")                      # families whose spiked tokens start from levelled flat rows (see above)
TAGS = {"batch": "batch", "ragged": "ragged", "adapt": "segadapt", "multi_guide": "multiguide"}      # the seed tags of the four test files

MIX6 = ((1, 4, 1, 8, 1), ("image", "video", "video", "video", "image"), 6, 6)
MIX9 = ((1, 4), ("image", "video"), 9, 9)


class Entry(NamedTuple):
    """step "batch": shape (B, T, h, w, modal); "ragged" / "adapt": (splits, modals, h, w); "multi_guide": (Q, T, h, w, modal)."""
    id: str
    step: str
    shape: tuple
    family: str
    chunks: Optional[int] = None
    recipe: Optional[str] = None        # None: cases.DEFAULT_CFG's (the plain recipe)
    hidden: int = 64
    with_fe: bool = True
    shift_g: float = 5.0
    shift_l: float = 4.0


CASES = (
    # ---- forward_batch ----
    Entry("batch_video_T4", "batch", (3, 4, 6, 6, "video"), "edge"),                       # 144 tokens per item: 9 full tiles
    Entry("batch_image_81", "batch", (2, 1, 9, 9, "image"), "edge"),                       # 81 tokens: a masked tail tile
    Entry("batch_T8_chunks3", "batch", (2, 8, 6, 6, "video"), "edge", chunks=3),           # spikes on both sides of the chunk boundaries
    Entry("batch_T8_chunks18", "batch", (2, 8, 6, 6, "video"), "edge", chunks=18),         # ... of every tile boundary
    Entry("batch_image_81_outlier", "batch", (2, 1, 9, 9, "image"), "edge_outlier", shift_g=8.0, shift_l=12.0),
    Entry("batch_image_81_scales", "batch", (2, 1, 9, 9, "image"), "item_scales"),
    Entry("batch_video_T4_h896", "batch", (3, 4, 6, 6, "video"), "edge", hidden=896),
    Entry("batch_image_81_h3584", "batch", (2, 1, 9, 9, "image"), "edge", hidden=3584),    # the readout's 96- / 192-row tiles
    # ---- forward_ragged ----
    Entry("ragged_mix6", "ragged", MIX6, "edge"),
    Entry("ragged_mix9", "ragged", MIX9, "edge"),
    Entry("ragged_mix6_outlier", "ragged", MIX6, "edge_outlier", shift_g=8.0, shift_l=12.0),
    Entry("ragged_mix9_scales", "ragged", MIX9, "item_scales"),
    # ---- the k / v adaptor recipes (hidden 896 as tests/test_gpu_seg_adapt.py).  An adapted key is (1 - a) fe + a LN(MLP(fe)), a = 0.5:
    # half of the spike reaches the logit, so shift_l is doubled where the keys are adapted ----
    Entry("adaptkv_mix6", "adapt", MIX6, "edge", recipe=ADAPTKV, hidden=896, shift_l=8.0),
    Entry("adaptk_mix6", "adapt", MIX6, "edge", recipe=ADAPTK, hidden=896, shift_l=8.0),
    Entry("adaptv_mix6", "adapt", MIX6, "edge", recipe=ADAPTV, hidden=896),
    Entry("adaptkv_mix6_outlier", "adapt", MIX6, "edge_outlier", recipe=ADAPTKV, hidden=896, shift_g=8.0, shift_l=24.0),
    # ---- forward_multi_guide ----
    Entry("mg_video3", "multi_guide", (3, 4, 6, 6, "video"), "edge"),
    Entry("mg_video5", "multi_guide", (5, 8, 6, 6, "video"), "edge"),                      # crosses a local group and a stream pass
    Entry("mg_image8", "multi_guide", (8, 1, 9, 9, "image"), "edge"),
    Entry("mg_video3_no_fe", "multi_guide", (3, 4, 6, 6, "video"), "edge", with_fe=False),
    Entry("mg_video3_outlier", "multi_guide", (3, 4, 6, 6, "video"), "edge_outlier", shift_g=8.0, shift_l=12.0),
    Entry("mg_video3_h896", "multi_guide", (3, 4, 6, 6, "video"), "edge", hidden=896),
)
BY_ID = {e.id: e for e in CASES}
assert len(BY_ID) == len(CASES)


def entries(step):
    return [e for e in CASES if e.step == step]


# ---- the families ----------------------------------------------------------------------------------------------------------------
def edge_tokens(N, chunks=None):
    """The item-local tokens `edge` spikes: 0, 15, 16, N - 1 and, for a step run with chunks=, the last token in front of and the first
    token behind every chunk boundary (chunk c of nc starts at tile ntiles c // nc, nc = min(chunks, ntiles): csrc/batch.hip,
    hicom_amd/ragged.py:plan_tables)."""
    toks = {0, 15, 16, N - 1}
    if chunks:
        ntiles = (N + 15) // 16
        nc = max(1, min(chunks, ntiles))
        for c in range(1, nc):
            tb = ntiles * c // nc
            toks |= {16 * tb - 1, 16 * tb}
    return sorted(t for t in toks if 0 <= t < N)


def spike_weight(n, N):
    """The part of shift_g / shift_l token n gets: all of it at the four tokens every item spikes, 0.6 of it at a token that is spiked
    as a chunk boundary only.  With one tile per chunk every 16th token and its predecessor are spiked; at equal height they would share
    the softmax mass evenly among 36 tokens, which a wrong logit scale or one lost token moves little.  Two heights keep a tenth of the
    mass on each of the four tokens and make the mass of the two groups depend on the scale."""
    return 1.0 if n in (0, 15, 16, N - 1) else 0.6


def global_spike(sd, g, shift_g):
    """a u for one guide g (float64): u = W_k^T (W_q g + b_q), the direction of frames_feature that raises this guide's global logits in
    every head; a so that the mean over the heads of the logit shift q_h . W_k,h (a u) / sqrt(128) is shift_g.  Returns (a u, the shift
    per head)."""
    p = "global_compressor.attn_layer."
    Wq, bq, Wk = (sd[p + n].astype(np.float64) for n in ("q_proj.weight", "q_proj.bias", "k_proj.weight"))
    q = Wq @ g.astype(np.float64) + bq
    u = Wk.T @ q
    nh = q.shape[0] // 128
    per = np.array([q[128 * i:128 * (i + 1)] @ (Wk[128 * i:128 * (i + 1)] @ u) for i in range(nh)]) / math.sqrt(128)
    a = shift_g / per.mean()
    return a * u, per * a


def head_directions(sd, g):
    """[D, heads]: column h = W_k,h^T q_h, the direction of frames_feature that guide g's global logit of head h reads."""
    p = "global_compressor.attn_layer."
    Wq, bq, Wk = (sd[p + n].astype(np.float64) for n in ("q_proj.weight", "q_proj.bias", "k_proj.weight"))
    q = Wq @ g.astype(np.float64) + bq
    return np.stack([Wk[i:i + 128].T @ q[i:i + 128] for i in range(0, q.shape[0], 128)], axis=1)


def local_spike(g, shift_l):
    g = g.astype(np.float64)
    return shift_l * math.sqrt(g.shape[0]) * g / (g @ g)


def under_family(x, sd, family, chunks=None, with_fe=True, shift_g=5.0, shift_l=4.0, power=0):
    """The item x = synth_inputs(...) (flat law; drawn with outliers=OUTLIERS for "edge_outlier") under `family`: a dict ff [T, h, w, D],
    fe (None without frames_embed), g.  x["g"] is the item's guide [D], or [Q, D] for Q guides on the one clip.  `power`: the item's
    index b of "item_scales"."""
    assert family in FAMILIES
    T, h, w, dim = x["ff"].shape
    N = T * h * w
    guides = x["g"].reshape(-1, dim)
    ff = x["ff"].reshape(N, dim).astype(np.float64)
    fe = x["fe"].reshape(N, dim).astype(np.float64)
    add_g = sum(global_spike(sd, g, shift_g)[0] for g in guides)
    add_l = sum(local_spike(g, shift_l) for g in guides)
    flat_ff, flat_fe = ff.copy(), fe.copy()
    toks = edge_tokens(N, chunks)
    if family in LEVELLED:
        # the flat rows under the spikes, levelled: their own logits (global: per head and guide; local: per guide) are set to the mean
        # logit of the item's tokens, so a spiked token stands exactly its spike above the item's average token
        dirs = np.concatenate([head_directions(sd, g) for g in guides], axis=1)            # [D, 9 Q]
        gdir = guides.astype(np.float64).T                                                 # [D, Q]
        mean_ff, mean_fe = ff.mean(axis=0), fe.mean(axis=0)
        for n in toks:
            flat_ff[n] -= dirs @ np.linalg.lstsq(dirs, flat_ff[n] - mean_ff, rcond=None)[0]
            flat_fe[n] -= gdir @ np.linalg.lstsq(gdir, flat_fe[n] - mean_fe, rcond=None)[0]
    for n in toks:
        wt = spike_weight(n, N)
        ff[n] = flat_ff[n] + wt * add_g
        fe[n] = flat_fe[n] + wt * add_l
        if not with_fe:
            ff[n] = ff[n] + wt * add_l
    s = np.float32(4.0 ** power if family == "item_scales" else 1.0)
    ff, fe = (synth.round_to_bf16(a.astype(np.float32)).reshape(T, h, w, dim) * s for a in (ff, fe))
    return dict(ff=ff, fe=fe if with_fe else None, g=x["g"] * s)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights(step, recipe, hidden):
    over = {"hidden_size": hidden}
    if recipe is not None:
        over["mm_projector_type"] = recipe
    cfg = SimpleNamespace(**{**cases.DEFAULT_CFG, **over})
    if step == "adapt":            # the state dict is always the adaptkv one: a recipe with fewer adaptors loads the part it has
        full = SimpleNamespace(**{**vars(cfg), "mm_projector_type": ADAPTKV})
        sd_all = synth.synth_state_dict(orc.param_shapes(full), tag=TAGS[step])
        sd = {k: v for k, v in sd_all.items() if k in orc.param_shapes(cfg)}
    else:
        sd = synth.synth_state_dict(orc.param_shapes(cfg), tag=TAGS[step])
    return cfg, sd


@functools.lru_cache(maxsize=None)
def build(id):
    """The case of entry `id`: cfg, sd, newline (None), the step's item description and `items`, a list of (ff, fe, g, modal) per item
    (per guide for "multi_guide"), what the oracle is run on."""
    e = BY_ID[id]
    cfg, sd = _weights(e.step, e.recipe, e.hidden)
    tag = TAGS[e.step]
    outliers = OUTLIERS if e.family == "edge_outlier" else None
    kw = dict(chunks=e.chunks, with_fe=e.with_fe, shift_g=e.shift_g, shift_l=e.shift_l)
    c = SimpleNamespace(entry=e, cfg=cfg, sd=sd, newline=None)
    if e.step == "multi_guide":
        Q, T, h, w, modal = e.shape
        clip = synth.synth_inputs(T, h, w, D, tag=f"{tag}:clip", outliers=outliers)
        clip["g"] = np.stack([synth.synth_inputs(1, 3, 3, D, tag=f"{tag}:guide{q}")["g"] for q in range(Q)])
        x = under_family(clip, sd, e.family, **kw)
        c.Q, c.modal, c.ff, c.fe, c.g = Q, modal, x["ff"], x["fe"], x["g"]
        c.items = [(c.ff, c.fe, c.g[q], modal) for q in range(Q)]
        return c
    if e.step == "batch":
        B, T, h, w, modal = e.shape
        splits, modals = [T] * B, [modal] * B
    else:
        splits, modals, h, w = e.shape
    xs = [under_family(synth.synth_inputs(T, h, w, D, tag=f"{tag}:item{b}", outliers=outliers), sd, e.family, power=b, **kw)
          for b, T in enumerate(splits)]
    c.B, c.splits, c.modals = len(splits), list(splits), list(modals)
    c.ff, c.fe, c.g = [x["ff"] for x in xs], ([x["fe"] for x in xs] if e.with_fe else None), np.stack([x["g"] for x in xs])
    if e.step == "batch":
        c.modal, c.ff, c.fe = modals[0], np.stack(c.ff), (np.stack(c.fe) if e.with_fe else None)
    c.items = [(c.ff[b], None if c.fe is None else c.fe[b], c.g[b], modals[b]) for b in range(c.B)]
    return c


def run_oracle(c, item):
    ff, fe, g, modal = c.items[item]
    sd = _torch_sd(c.entry.step, c.entry.recipe, c.entry.hidden)
    return orc.projector_forward(c.cfg, sd, to_t(ff), to_t(fe), to_t(g), modal, None).numpy()


@functools.lru_cache(maxsize=None)
def _torch_sd(step, recipe, hidden):
    return {k: to_t(v) for k, v in _weights(step, recipe, hidden)[1].items()}


@functools.lru_cache(maxsize=None)
def oracle_outputs(id):
    """The oracle's output per item (per guide), computed once per process; callers must not write into it."""
    c = build(id)
    outs = [run_oracle(c, i) for i in range(len(c.items))]
    for o in outs:
        o.setflags(write=False)
    return outs


def tolerance(entry, want):
    """The bar of the GPU tests for one item's output `want` (the oracle's): max-abs, the same for both regions."""
    return HEAVY_REL * float(np.abs(want).max()) if entry.family == "edge_outlier" else TOL


def region_errors(got, want):
    """max-abs over the local rows and over the NG global rows."""
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    return {"local": float(d[:-NG].max()), "global": float(d[-NG:].max())}


def check_item(entry, what, got, want):
    """Prints the per-region max-abs of one item against the oracle and returns the violations of its bar as strings."""
    tol = tolerance(entry, want)
    errs = region_errors(got, want)
    print(f"{entry.id} [{entry.family}] {what}: local {errs['local']:.3e}  global {errs['global']:.3e}  (bar {tol:.3e}, max|out| {np.abs(want).max():.3f})")
    return [f"{what} {r} rows: {v:.3e} > {tol:.3e}" for r, v in errs.items() if not v <= tol]
