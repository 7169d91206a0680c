"""Inputs, float64 references and derived error bounds for the window bodies of the many-guide local stage, multi_window_ctx16<NV, NG>
and multi_window_adapt_ctx16<NV, NG> (csrc/multi_window.hpp; launched by multi_guide_local_kernel and multi_guide_local_adapt_kernel,
csrc/multi_guide.hip), and for the single-guide body local_window_ctx16 (csrc/segment_item.hpp) behind forward_batch / forward_ragged.
Shared by tests/test_gpu_multi_window.py (the kernels against the references) and tests/test_multi_window_power.py (CPU: what a wrong
kernel would do to the references, against the same bounds).  A layer on tests/window_attn_inputs.py (spike_positions, plant,
forward_bounds_of, ctx16_of) and tests/ops_reference.py (window_tokens, window_attention_ref, blend_rows, ln_fp32_tol).

The family
  guides     Q bf16 rows ~ N(0, 1) in 1152 dimensions: distinct, pairwise |cosine| below COS_MAX (asserted in build).  Adaptor form:
             guide q keeps that size on its own BLOCK of 96 columns and THIN = 0.05 of it on the others.  The adaptor's logit bound is
             4 D 2^-23 on the sum of ABSOLUTE terms, and what guide q' plants in a shared key row enters guide q's absolute terms
             with sum_j |q_j| |q'_j| / |q'|: among dense guides the bound of every weight grows by 1 % per further guide, and at Q = 9
             no two contexts of a window are 8 such bounds apart.  Every column still carries every guide.  On its block guide q also
             leans by +-0.5 (1 + q // 2 / 2), the sign alternating with q: cg = sum_j q_j gamma_j then differs between any two guides
             by a quarter of |q| at least (two random guides can have nearly the same cg, and a cg taken from guide 0 would not show).
  spikes     window positions of window_attn_inputs.spike_positions: 0, 3, 4 and WIN - 1 (lane 63 at WIN 64) at the full height, both
             sides of every multiple of 8 and of 12 at 0.6 of it.  A window of fewer than three such positions (WIN 1, WIN 3) spikes all
             of its positions, so that a pair of them stays live when one is left out; where all spikes would have one height (WIN 3,
             WIN 8) the second one stands at 0.85 of it, so that the logit scale owns a share of every window's weights.
  diversity  guide q of window w leaves out spike (w + q) mod k of the k spikes, so no two guides of a window and no two windows of a
             guide share a maximum or a weight pattern.  Guides q >= k (a small window under many guides) would repeat a pattern: guide
             q lowers spike (w + q + q // k) mod k to 0.85 of its height as well.  ONE window under ONE guide leaves nothing out (there is
             nothing to differ from, and its first position has to carry mass for a lost first token to show).
  planting   guide q plants its own spikes with window_attn_inputs.plant through the key rows along that guide (adaptor form: through
             the x stream, the (1 - a_k) factor divided out).  The key rows are shared by all guides, so what one guide plants leaks
             into the others by the guides' cosine; the references simply compute what results.  conditions() says what must still
             hold, and tests/test_multi_window_power.py asserts it.
  keys       the random part of a key row: N(0, 1 / 16) per column in the plain form (flat logits ~ N(0, 1 / 16): under N(0, 1) the flat
             part alone pushes a spike of some (guide, window) pairs below the live weight), N(0, 1) in the x stream of the adaptor form
             (its guides are thin outside their block).
  values     random rows.  Adaptor form: the x rows of the tokens at the second height are twenty times as large (window_attn_inputs.build
             has the reason: the adaptor's logit bound is wide, and the split of the mass between the heights has to own a share).
  planes     adaptor form: ky / vy are fp16 planes given directly, row n = s_n N(0, 1) + m_n with s_n = 10^U(-1, 1) (two decades) and
             m_n = s_n (0.4 + 0.6 |N(0, 1)|): the LayerNorm statistics of neighbouring rows differ by up to a factor of 100, so a mu / rstd taken
             from another row moves the result.  alpha_k = 0.4, alpha_v = 0.3, as bf16 or f32; `which` = key / value / both (the other
             plane is NULL).
  far        runs with `far`: every key row holds FAR_KEY in column J0 and every ODD guide FAR / (scale (1 - a_k) FAR_KEY) there (set
             behind the planting, which sees that column as zero): the logits of an odd guide lie FAR = 110 above those of its even
             neighbour, uniformly over a window, so the softmax of either is what it was.  expf(110) overflows fp32 and expf(-110) is
             zero: a guide that subtracts its neighbour's maximum turns non-finite.  (Without this no reference can see that fault:
             exp(s - c) / sum exp(s - c) does not depend on c.)  The logit bound grows with |s| -- these runs count that fault alone.

Geometries (T, H, W, kt, ks), E = 1152, exact partitions only (all the entry points admit): GEOMS.  Guide counts: every NG alone (1 .. 4),
a full group plus each remainder (5, 6, 7), two full groups plus one (9) at WIN 36 and at both WIN 64 grids; 1, 4, 5 at the others.

References: blend_rows on both streams (adaptor form), then window_attention_ref per guide, in float64, from the values as the kernel
received them.  The output is the fp16 plane [Q][windows][1152].

Bounds: window_attn_inputs.forward_bounds_of per guide, output ctx16 -- the logit error of a D-term fp32 dot product of bf16 / fp16
inputs (logit_tol), its effect on the weights (weight_rel), the (WIN + 4)-term fp32 accumulation, one rounding to fp16.  The bodies here
run the same arithmetic per guide as the kernels those bounds were written for (one wave instead of four: fewer partial sums, the same
count of terms).  One term is added for the blended KEY stream, the LayerNorm statistics' error on the logit, which logit_tol folds
into its 4 D 2^-23 on absolute terms without deriving it.  With per-token means and scales it is derived here from ln_fp32_tol: the
logit holds scale a_k sum_j q_j LN(y_n)_j, LN(y)_j = gamma_j (y_j - mu) rstd + beta_j computed with fp32 statistics is off by at most
ln_fp32_tol(y, gamma, beta, eps)_j, hence
        d_s += scale a_k sum_j |q_j| ln_fp32_tol(y_n, gamma_k, beta_k, eps)_j.
(The value stream's statistics are in forward_bounds_of already: its `drow` term.)  No constant here comes from a kernel's output.
"""
import functools
import math
from types import SimpleNamespace
from typing import NamedTuple

import torch

import ops_reference as R
import window_attn_inputs as wi
from ops_reference import up

D = 1152
EPS = 1e-6
COS_MAX = 0.2
BLOCK, THIN = 96, 0.05
SECOND_ROUND = 0.85
LIVE = 0.05                 # a position is live above this weight
APART = 8.0                 # two guides of a window differ by this many bounds somewhere
FAR, FAR_KEY, J0 = 110.0, 128.0, 7
F32_MAX, F32_TINY = 3.4028234663852886e38, 2.0 ** -149
AK, AV = 0.4, 0.3
FLAT = 0.25                 # size of a key row's random part: flat logits ~ N(0, 1 / 16)
LOW_ROWS = 20.0             # adaptor form: size of the x value rows at the second height
MEAN = (0.4, 0.6)           # a y row's mean in units of its scale: MEAN[0] + MEAN[1] |N(0, 1)|

GEOMS = {
    "w1": (1, 1, 1, 1, 1),            # WIN 1
    "w3": (3, 1, 1, 3, 1),            # WIN 3
    "w8": (2, 2, 2, 2, 2),            # WIN 8
    "w16": (4, 2, 2, 4, 2),           # WIN 16
    "w36": (8, 6, 6, 4, 3),           # WIN 36: 8 windows, the release shape in small
    "w64": (4, 8, 8, 4, 4),           # WIN 64: 4 windows, every lane live
    "w64_flat": (1, 8, 8, 1, 8),      # WIN 64: a single window, all lanes in one frame
    "w9_tail": (1, 3, 9, 1, 3),       # WIN 9: 3 windows, the last workgroup has one live wave of four (`win >= nwin`)
}
ALL_Q, FEW_Q = (1, 2, 3, 4, 5, 6, 7, 9), (1, 4, 5)
MANY = ("w36", "w64", "w64_flat")      # every guide count
WHICH = ("key", "value", "both")


class MRun(NamedTuple):
    form: str                     # "plain" | "adapt"
    geom: str
    Q: int
    which: str = "both"           # adapt: key | value | both
    alpha_dt: str = "bf16"
    far: bool = False

    @property
    def id(self):
        return "-".join([self.form, self.geom, f"Q{self.Q}"] + ([self.which, self.alpha_dt] if self.form == "adapt" else [])
                        + (["far"] if self.far else []))


def _runs():
    plain = [MRun("plain", g, q) for g in GEOMS for q in (ALL_Q if g in MANY else FEW_Q)]
    adapt, n = [], 0
    for g in GEOMS:
        for q in (ALL_Q if g in MANY else FEW_Q):
            for which in (WHICH if g in ("w36", "w64") else (WHICH[n % 3],)):       # WIN 36 and the 4-window WIN 64: all three
                adapt.append(MRun("adapt", g, q, which, ("bf16", "f32")[n % 2]))
                n += 1
    far = [MRun(form, g, q, "both", "f32" if q == 2 else "bf16", True) for form in ("plain", "adapt") for g in ("w36", "w64") for q in (2, 7)]
    return tuple(plain), tuple(adapt), tuple(far)


PLAIN_RUNS, ADAPT_RUNS, FAR_RUNS = _runs()
RUNS = PLAIN_RUNS + ADAPT_RUNS + FAR_RUNS
assert len({r.id for r in RUNS}) == len(RUNS)


def partner(q, Q):
    """The guide that shares guide q's register arrays as u ^ 1 in its group of kGuideGroup = 4 (q itself where the group has none)."""
    g0 = q // 4 * 4
    v = (q - g0) ^ 1
    return g0 + v if v < min(4, Q - g0) else q


# ---- the family -----------------------------------------------------------------------------------------------------------------
def positions(WIN):
    pos = wi.spike_positions(WIN)
    if len(pos) < 3:
        pos = {i: 1.0 for i in range(WIN)}
    if len(pos) > 1 and len(set(pos.values())) == 1:
        pos[list(pos)[1]] = SECOND_ROUND
    return pos


def multi_targets(Q, NW, WIN):
    """[Q, NW, WIN]: the height of position i's spike for guide q in window w."""
    pos = positions(WIN)
    keys, k = list(pos), len(pos)
    tgt = torch.zeros(Q, NW, WIN, dtype=torch.float64)
    for i, h in pos.items():
        tgt[:, :, i] = wi.SHIFT * h
    if Q * NW > 1:
        for q in range(Q):
            for w in range(NW):
                r = q // k
                if r:
                    tgt[q, w, keys[(w + q + r) % k]] *= SECOND_ROUND
                tgt[q, w, keys[(w + q) % k]] = 0.0
    return tgt


def _planes(N, rnd):
    s = 10.0 ** (2.0 * torch.rand(N, 1, generator=rnd.g) - 1.0)
    return (rnd(N, D) * s + s * (MEAN[0] + MEAN[1] * rnd(N, 1).abs())).half()


@functools.lru_cache(maxsize=None)
def build(run):
    """The tensors of `run` as the kernels receive them (CPU; callers must not write into them)."""
    T, H, W, kt, ks = geom = GEOMS[run.geom]
    N, Q = T * H * W, run.Q
    tok, _ = R.window_tokens(*geom)
    NW, WIN = tok.shape
    assert tok.numel() == N
    g = torch.Generator().manual_seed(wi._seed(run.id))
    rnd = lambda *s: torch.randn(*s, generator=g)
    rnd.g = g
    adapt = run.form == "adapt"
    c = SimpleNamespace(run=run, geom=geom, D=D, N=N, Q=Q, NW=NW, WIN=WIN, tok=tok, bias=0.0, eps=EPS)
    c.scale = 1.0 / math.sqrt(D)
    c.tgt = multi_targets(Q, NW, WIN)
    guides = rnd(Q, D)
    if adapt:                                 # (module docstring, `guides`)
        own = torch.arange(D)[None, :] // BLOCK == torch.arange(Q)[:, None]
        lean = torch.tensor([(-1.0) ** q * 0.5 * (1 + 0.5 * (q // 2)) for q in range(Q)])[:, None]
        guides = torch.where(own, guides + lean, guides * THIN)
    guides = guides.bfloat16()
    if run.far:
        guides[:, J0] = 0.0
    use_k, use_v = adapt and run.which in ("both", "key"), adapt and run.which in ("both", "value")
    adt = wi.DT[run.alpha_dt]
    c.ak, c.av = (torch.tensor([AK]).to(adt) if use_k else None), (torch.tensor([AV]).to(adt) if use_v else None)
    keep = 1.0 - (float(c.ak.double()) if use_k else 0.0)
    key = rnd(N, D).double() * (1.0 if adapt else FLAT)
    for q in range(Q):
        wi.plant(key, tok, up(guides[q]).expand(NW, D), c.tgt[q], c.scale, 0, False, divide=keep)
    if run.far:
        key[:, J0] = FAR_KEY / keep
        guides[1::2, J0] = FAR / (c.scale * FAR_KEY)
    c.guides = guides
    gd = up(guides)
    cos = (gd @ gd.T) / (gd.norm(dim=1)[:, None] * gd.norm(dim=1)[None, :]) - torch.eye(Q, dtype=torch.float64)
    assert float(cos.abs().max()) < (1.0 if run.far else COS_MAX), run.id
    value = rnd(N, D)
    if not adapt:
        c.key, c.value = key.float().bfloat16(), value.bfloat16()
        return c
    low = tok[:, [i for i, h in positions(WIN).items() if h < 1.0]].unique()
    value[low] *= LOW_ROWS
    c.kx, c.vx = key.float().bfloat16(), value.bfloat16()
    c.ky = _planes(N, rnd) if use_k else None
    c.vy = _planes(N, rnd) if use_v else None
    c.kg, c.kb, c.vg, c.vb = ((1 + 0.1 * rnd(D)).bfloat16(), (0.1 * rnd(D)).bfloat16(), (1 + 0.1 * rnd(D)).bfloat16(), (0.1 * rnd(D)).bfloat16())
    return c


# ---- references -------------------------------------------------------------------------------------------------------------------
def _stream(x, y, ga, be, a, src=None):
    """(rows, absolute terms, rstd mu) of one stream: blend_rows; src [N] plants the LayerNorm statistics of row src[n] on row n."""
    x = up(x)
    if y is None:
        return x, None, None
    y, ga, be, a = up(y), up(ga), up(be), float(a.double())
    mu, rstd = R.layer_norm_stats(y, EPS)
    if src is None:
        return R.blend_rows(x, y, ga, be, a, EPS)[0], R.ln_blend_ref(y, ga, be, x, a, EPS)[1], rstd * mu
    mu, rstd = mu[src], rstd[src]
    return (1 - a) * x + a * ((y - mu) * rstd * ga + be), None, rstd * mu


def streams(c, src=None):
    """((K, K_ab, rstd mu of ky), (V, V_ab, rstd mu of vy)) of a run, float64."""
    if c.run.form == "plain":
        return (up(c.key), None, None), (up(c.value), None, None)
    return _stream(c.kx, c.ky, c.kg, c.kb, c.ak, src), _stream(c.vx, c.vy, c.vg, c.vb, c.av, src)


@functools.lru_cache(maxsize=None)
def reference(run):
    """window_attention_ref per guide, stacked: ctx [Q, NW, D], s, p, s_ab [Q, NW, WIN], ...; `per_guide`: the dicts themselves."""
    c = build(run)
    (K, Kab, _), (V, Vab, _) = streams(c)
    per = [R.window_attention_ref(K, V, up(c.guides[q]).expand(c.NW, D), c.geom, c.scale, 0.0, key_ab=Kab, value_ab=Vab) for q in range(c.Q)]
    out = {k: torch.stack([fw[k] for fw in per]) for k in ("ctx", "s", "p", "mx", "s_ab", "ctx_ab")}
    out["per_guide"] = per
    return out


@functools.lru_cache(maxsize=None)
def bounds(run):
    """[Q, NW, D]: the bound of every element of the fp16 plane (module docstring)."""
    c = build(run)
    ref = reference(run)
    like = wi.Run("adapt" if run.form == "adapt" else "fwd", run.geom, D)
    more = 0.0
    tol_rows = None
    if run.form == "adapt" and c.ky is not None:
        tol_rows = R.ln_fp32_tol(up(c.ky), up(c.kg), up(c.kb), EPS)[c.tok]                       # [NW, WIN, D]
    out = []
    for q in range(c.Q):
        if tol_rows is not None:
            more = c.scale * float(c.ak.double()) * torch.einsum("wid,d->wi", tol_rows, up(c.guides[q]).abs())
        out.append(wi.forward_bounds_of(like, c, ref["per_guide"][q], more)["ctx16"])
    return torch.stack(out)


def want16(run):
    """What the fp16 plane stands for."""
    return wi.ctx16_of(reference(run)["ctx"])


def conditions(run):
    """(share of (guide, window) pairs with fewer than min(2, WIN) live positions, share of guide pairs of a window whose contexts lie
    closer than APART bounds everywhere).  The second is 0 by definition at WIN 1 (one token has weight 1 under every guide) and in
    the `far` runs (their bound is ten times as wide, and the one fault they count needs no two guides apart)."""
    c, ref, b = build(run), reference(run), bounds(run)
    live = (ref["p"] > LIVE).sum(-1) < min(2, c.WIN)
    close, pairs = 0, 0
    if c.WIN > 1 and not run.far:
        ctx = want16(run)
        for q in range(c.Q):
            for r in range(q + 1, c.Q):
                far_apart = ((ctx[q] - ctx[r]).abs() / torch.maximum(b[q], b[r])).max(-1).values >= APART
                close += int((~far_apart).sum())
                pairs += c.NW
    return float(live.float().mean()), (close / pairs if pairs else 0.0)


# ---- planted faults (tests/test_multi_window_power.py) ---------------------------------------------------------------------------
def _softmax(s, lost=(), mx_of=None):
    s = s.clone()
    s[..., list(lost)] = -math.inf
    mx = s.max(-1, keepdim=True).values
    if mx_of is None:
        e = torch.exp(s - mx)
    else:                                    # another guide's maximum: the exponentials at the range of fp32
        e = torch.exp((s - mx[mx_of]).clamp(max=700.0))
        e = torch.where(e > F32_MAX, torch.full_like(e, math.inf), torch.where(e < F32_TINY, torch.zeros_like(e), e))
    return e / e.sum(-1, keepdim=True)


def fault_names(run):
    """The faults that apply to `run`; why a fault does not apply is written at mutant()."""
    c = build(run)
    Q, WIN = c.Q, c.WIN
    paired = any(partner(q, Q) != q for q in range(Q))
    if run.far:
        return ["take_max"]
    out = ["drop_first", "drop_last"]
    if WIN > 1:
        out.append("scale_1.1")
        if paired:
            out.append("take_weights")
        if Q > 4 and Q % 4:
            out.append("prev_group_rows")
    if Q > 1:
        out.append("plane_stride")
    if run.form == "adapt":
        if WIN > 1:
            out += ["stats_prev", "stats_last"]
        if c.vy is not None:
            out.append("no_smu")
        if c.ky is not None and Q > 1 and WIN > 1:
            out.append("cg_of_guide_0")
    return out


def mutant(run, name):
    """The fp16 plane's float64 meaning [Q, NW, D] under one planted fault (non-finite where the fault empties a softmax):
      take_max          guide u of a group subtracts guide u ^ 1's maximum.  `far` runs only: elsewhere it computes the same function.
      take_weights      guide u takes guide u ^ 1's weights.  Q with a pair in a group, WIN > 1 (one token: weight 1 for all).
      prev_group_rows   the remainder group reads the guide rows of the group in front.  Q > 4 with a remainder, WIN > 1.
      plane_stride      guide q's plane is written (plane - D) q elements from the first (guide by guide into a NaN-filled buffer).  Q > 1.
      drop_last / drop_first   window position WIN - 1 (lane 63 at WIN 64) / 0 out of the softmax.  At WIN 1 the softmax is empty.
      scale_1.1         logits scaled by 1.1.  WIN > 1.
      stats_prev / stats_last   adaptor form: mu / rstd of the window's previous row (the first row keeps its own) / of its last row
                        for all of them, on every adapted stream.  WIN > 1.
      no_smu            adaptor form, values adapted: the - smu of the epilogue left out.
      cg_of_guide_0     adaptor form, keys adapted: the cg of guide 0 in every guide's logit.  Q > 1, WIN > 1."""
    c, ref = build(run), reference(run)
    tok, Q, NW, WIN = c.tok, c.Q, c.NW, c.WIN
    gd = up(c.guides)
    src = None
    if name in ("stats_prev", "stats_last"):
        src = torch.arange(c.N)
        src[tok.reshape(-1)] = (torch.cat([tok[:, :1], tok[:, :-1]], 1) if name == "stats_prev" else tok[:, -1:].expand(NW, WIN)).reshape(-1)
    (K, _, kmu), (V, _, vmu) = streams(c, src)
    rows = list(range(Q))
    if name == "prev_group_rows":
        g0 = Q // 4 * 4
        rows = [q - 4 if q >= g0 else q for q in range(Q)]
    s = ref["s"] if src is None and name != "prev_group_rows" else c.scale * torch.einsum("wid,qd->qwi", K[tok], gd[rows])
    if name == "scale_1.1":
        s = 1.1 * s
    if name == "cg_of_guide_0":
        cg = (gd * up(c.kg)).sum(1)
        s = s + c.scale * float(c.ak.double()) * kmu[tok].squeeze(-1)[None] * (cg - cg[0])[:, None, None]
    pair = [partner(q, Q) for q in range(Q)]
    lost = {"drop_first": (0,), "drop_last": (WIN - 1,)}.get(name, ())
    p = _softmax(s, lost, pair if name == "take_max" else None)
    if name == "take_weights":
        p = p[pair]
    ctx = torch.einsum("qwi,wid->qwd", p, V[tok])
    if name == "no_smu":
        ctx = ctx + float(c.av.double()) * up(c.vg) * torch.einsum("qwi,wi->qw", p, vmu[tok].squeeze(-1))[:, :, None]
    if name == "plane_stride":
        plane = NW * D
        flat = torch.full((Q * plane,), wi.NAN, dtype=torch.float64)
        for q in range(Q):
            flat[q * (plane - D):q * (plane - D) + plane] = ctx[q].reshape(-1)
        ctx = flat.view(Q, NW, D)
    return wi.ctx16_of(ctx)


def gamma_once_shift(run):
    """What folding gamma into the y row once per row (csrc/multi_window.hpp warns against it: `that would round differently`) does to
    the contexts, in bounds: every product gamma_j y_j formed in fp32 before it meets the guide.  In exact arithmetic it is the
    reference's own function and the products are exact in fp32, so the fault has no float64 form; what is left is where sums round."""
    c, ref = build(run), reference(run)
    assert run.form == "adapt" and c.ky is not None
    a = float(c.ak.double())
    y, ga = up(c.ky), up(c.kg)
    mu, rstd = R.layer_norm_stats(y, EPS)
    folded = (c.ky.float() * c.kg.float()).double()                                   # fp32 products, as one pass over the row leaves them
    K = (1 - a) * up(c.kx) + a * ((folded - mu * ga) * rstd + up(c.kb))
    s = c.scale * torch.einsum("wid,qd->qwi", K[c.tok], up(c.guides))
    (_, _, _), (V, _, _) = streams(c)
    ctx = torch.einsum("qwi,wid->qwd", _softmax(s), V[c.tok])
    return float(((wi.ctx16_of(ctx) - want16(run)).abs() / bounds(run)).max())


# ---- the single-guide body behind forward_batch / forward_ragged ---------------------------------------------------------------------
ITEM_CASES = {"batch": ((4, 4, 4), ("video",) * 3), "ragged": ((4, 8, 1), ("video", "video", "image"))}
ITEM_HW, ITEM_KT, ITEM_KS = 6, 4, 3


@functools.lru_cache(maxsize=None)
def item_case(name):
    """Items of T frames on a 6 x 6 grid, each with its own guide row and tokens, planted per item by the single-guide family
    (window_attn_inputs.spike_targets); the float64 contexts and their bounds per item, in the order the step stacks its windows."""
    Ts, modals = ITEM_CASES[name]
    g = torch.Generator().manual_seed(wi._seed("items-" + name))
    rnd = lambda *s: torch.randn(*s, generator=g)
    scale = 1.0 / math.sqrt(D)
    guides = rnd(len(Ts), D).bfloat16()
    like = wi.Run("fwd", "items", D)
    ff, fe, ctx, tol = [], [], [], []
    for i, (T, modal) in enumerate(zip(Ts, modals)):
        geom = (T, ITEM_HW, ITEM_HW, 1 if modal == "image" or T == 1 else ITEM_KT, ITEM_KS)
        tok, _ = R.window_tokens(*geom)
        NW, WIN = tok.shape
        q = up(guides[i]).expand(NW, D)
        key = rnd(T * ITEM_HW * ITEM_HW, D).double()
        wi.plant(key, tok, q, wi.spike_targets(NW, WIN), scale, 0, True)
        c = SimpleNamespace(D=D, WIN=WIN, bias=0.0, value=rnd(T * ITEM_HW * ITEM_HW, D).bfloat16(), key=key.float().bfloat16())
        fw = R.window_attention_ref(up(c.key), up(c.value), q, geom, scale, 0.0)
        ff.append(c.value), fe.append(c.key), ctx.append(wi.ctx16_of(fw["ctx"])), tol.append(wi.forward_bounds_of(like, c, fw)["ctx16"])
    return SimpleNamespace(Ts=Ts, modals=modals, scale=scale, guides=guides, ff=torch.cat(ff), fe=torch.cat(fe), ctx=ctx, tol=tol,
                           windows=sum(t.shape[0] for t in ctx))
