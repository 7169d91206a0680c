"""Inputs, float64 references and derived bounds for the logits form of the multi-guide step: the scores kernel
hicom_head_scores_multi_fwd behind hicom_head_guide_fold_fwd (csrc/head_scores.hip) and the local kernel
hicom_multi_guide_local_logits_fwd (csrc/multi_guide.hip, multi_window.hpp: multi_window_guides_logits_ctx16).  Shared by
tests/test_gpu_head_scores.py, tests/test_gpu_multi_guide_logits.py (the kernels against the references) and
tests/test_head_scores_power.py (CPU: what a wrong kernel would do to the references, against the same bounds).

Scores
  operands   x bf16 [M, 1152] ~ N(0, 1); hid fp16 [M, ld] = |N(0, 1)| on columns < inter (what a GELU leaves, mostly positive: the hidden
             term does not average out), zero on [inter, kpad) and in the pitch gap [kpad, ld) -- or SENTINEL there (`sentinel` cases: the
             result must not move); guides bf16 [Q, 1152] ~ N(0, 1); W2 bf16 [1152, inter] ~ N(0, 0.03^2); b2 bf16 [1152] ~ N(0, 0.25).
             So g . x ~ 34, U . hid ~ sqrt(1152) 0.03 inter 0.8 / sqrt(inter) ..., c ~ 17: each of the three terms is orders above the bound.
  reference  L[q, n] = x[n] . g_q + hid[n, :inter] . (W2^T g_q) + g_q . b2, float64, from the values as the kernels receive them.
  bound      per element, from the formats and the summation structure the header of csrc/head_scores.hip states (never from a result).
             With A[q, n] = sum |x||g| + sum_k |hid||U| + sum |g||b2| and Uab = |W2|^T |g|:
               (2 (K / 4 + 128) + 12) 2^-24 A    fp32 accumulation: K = 1152 + inter products are dealt to four waves in blocks of 128, so no
                                                 running sum holds more than K / 4 + 128 of them; a hidden product is two (hi and lo); the
                                                 four partial sums, the scale, c and the x part are a dozen more roundings
               + (1152 / 16 + 18) 2^-24 sum_k |hid[n, k]| Uab[q, k]     U[q, k] itself: an fp32 sum of 1152 products in 16 slices, the
                                                 slices added in order (every |product| is inside Uab)
               + 2^-21 max_k |U[q, k]| sum_k |hid[n, k]|                the hi + lo fp16 pair at the row's power of two: 2^-22 of the row's
                                                 largest scaled value, which is below twice max |U|
             The operands themselves are exact (bf16 guides and tokens, fp16 hidden values).

Local stage
  families   `spike`: the plain family of tests/multi_window_inputs.py (a dominant logit per window and guide, diversity between guides and
             windows: its builders on this file's geometries) on T = 1 windows of 9 tokens (w9_tail), 4 x 3 x 3 windows on 6 x 6 (w36) and on 27 x 27 (w27);
             `flat`: the same tokens with key rows of N(0, 1 / 16) and nothing planted -- near-equal logits, every weight about 1 / WIN.
             Q in 1, 4, 5, 32.  The kernel receives the EXACT logits key_n . g_q (float64, rounded to fp32 once), so its logit error is
             one fp32 rounding: inside the D-term logit bound of window_attn_inputs.forward_bounds_of, which is used unchanged (the bound
             multi_window_inputs.bounds is for the plain form).
"""
import functools
from types import SimpleNamespace
from typing import NamedTuple

import torch

import multi_window_inputs as mw
import ops_reference as R
import window_attn_inputs as wi
from ops_reference import up

D = 1152
SENTINEL = 30000.0
EPS24 = 2.0 ** -24


class HsCase(NamedTuple):
    M: int
    inter: int
    Q: int
    sentinel: bool = False

    @property
    def id(self):
        return f"M{self.M}-inter{self.inter}-Q{self.Q}" + ("-sentinel" if self.sentinel else "")


def kpad_ld(inter):
    kpad = (inter + 63) // 64 * 64
    return kpad, kpad + (192 if kpad > 2048 else 0)          # (encoder._head_cache's pitch rule)


# M = 144 (4 x 6 x 6), 729 (one frame of the release grid: 22 workgroups and a 25-token tail), 16 k + 5; every Q at the small head,
# the pitched plane at M = 144
HS_CASES = tuple([HsCase(M, 200, Q) for M in (144, 729, 16 * 3 + 5) for Q in (1, 3, 17, 32)]
                 + [HsCase(144, 4304, Q) for Q in (1, 3, 17, 32)]
                 + [HsCase(144, 4304, 3, True), HsCase(53, 200, 17, True)])


@functools.lru_cache(maxsize=None)
def hs_build(case):
    g = torch.Generator().manual_seed(wi._seed("head-scores-" + case.id))
    rnd = lambda *s: torch.randn(*s, generator=g)
    kpad, ld = kpad_ld(case.inter)
    hid = torch.full((case.M, ld), SENTINEL if case.sentinel else 0.0)
    hid[:, :case.inter] = rnd(case.M, case.inter).abs()
    return SimpleNamespace(case=case, kpad=kpad, ld=ld, x=rnd(case.M, D).bfloat16(), hid=hid.half(), guides=rnd(case.Q, D).bfloat16(),
                           w2=(0.03 * rnd(D, case.inter)).bfloat16(), b2=(0.5 * rnd(D)).bfloat16())


def hs_terms(c):
    """(g . x, U . hid, c) as float64 [Q, M], [Q, M], [Q], and U [Q, inter]."""
    x, h, g, w2, b2 = up(c.x), up(c.hid)[:, :c.case.inter], up(c.guides), up(c.w2), up(c.b2)
    U = g @ w2
    return g @ x.T, U @ h.T, g @ b2, U


@functools.lru_cache(maxsize=None)
def hs_reference(case):
    gx, uh, cc, _ = hs_terms(hs_build(case))
    return gx + uh + cc[:, None]


@functools.lru_cache(maxsize=None)
def hs_tol(case):
    c = hs_build(case)
    x, h, g, w2, b2 = (up(t).abs() for t in (c.x, c.hid[:, :case.inter], c.guides, c.w2, c.b2))
    Uab = g @ w2
    U = hs_terms(c)[3].abs()
    A = g @ x.T + U @ h.T + (g @ b2)[:, None]
    K = D + case.inter
    return ((2 * (K / 4 + 128) + 12) * EPS24 * A + (D / 16 + 18) * EPS24 * (Uab @ h.T)
            + 2.0 ** -21 * U.max(1).values[:, None] * h.sum(1)[None, :])


HS_MUTANTS = ("no_hidden", "no_c", "u_of_guide_0", "pitch_is_kpad")


def hs_mutant(case, name):
    """The reference under one planted fault, or None where the fault computes the same function:
      no_hidden       the hidden term dropped
      no_c            c[q] dropped
      u_of_guide_0    U of guide 0 in every guide's hidden term (Q > 1)
      pitch_is_kpad   token n's hidden row read at n kpad of the plane instead of n ld: the pitch gap read as data (ld != kpad)"""
    c = hs_build(case)
    gx, uh, cc, U = hs_terms(c)
    if name == "no_hidden":
        return gx + cc[:, None]
    if name == "no_c":
        return gx + uh
    if name == "u_of_guide_0":
        return None if case.Q == 1 else gx + (U[:1] @ up(c.hid)[:, :case.inter].T).expand(case.Q, -1) + cc[:, None]
    if name == "pitch_is_kpad":
        if c.ld == c.kpad:
            return None
        rows = up(c.hid).reshape(-1)[:case.M * c.kpad].view(case.M, c.kpad)[:, :case.inter]
        return gx + U @ rows.T + cc[:, None]
    raise KeyError(name)


# ---- local stage ------------------------------------------------------------------------------------------------------------------
LOCAL_GEOMS = {"w9_tail": mw.GEOMS["w9_tail"], "w36": mw.GEOMS["w36"], "w27": (4, 27, 27, 4, 3)}      # w27: WIN 36 on the release grid, 81 windows
LOCAL_Q = (1, 4, 5, 32)


class LRun(NamedTuple):
    family: str                   # "spike" | "flat"
    geom: str
    Q: int

    @property
    def id(self):
        return f"{self.family}-{self.geom}-Q{self.Q}"


LOCAL_RUNS = tuple([LRun("spike", g, q) for g in LOCAL_GEOMS for q in LOCAL_Q] + [LRun("flat", "w36", q) for q in LOCAL_Q]
                   + [LRun("flat", "w9_tail", 5)])


@functools.lru_cache(maxsize=None)
def local_build(run):
    """The plain family of multi_window_inputs.build on a geometry of this file (`spike`: every guide plants its own spikes through the key
    rows, multi_targets; `flat`: nothing planted).  value bf16 [N, D], logits f32 [Q, N] (exact dot products key_n . g_q, rounded
    once), the float64 contexts as fp16 stands for them and their bounds (window_attn_inputs.forward_bounds_of per guide, what
    multi_window_inputs.bounds is for the plain form), both [Q, NW, D]."""
    geom = LOCAL_GEOMS[run.geom]
    tok, _ = R.window_tokens(*geom)
    NW, WIN = tok.shape
    N, Q = tok.numel(), run.Q
    g = torch.Generator().manual_seed(wi._seed("logits-" + run.id))
    rnd = lambda *s: torch.randn(*s, generator=g)
    scale = 1.0 / D ** 0.5
    guides = rnd(Q, D).bfloat16()
    key = rnd(N, D).double() * mw.FLAT
    if run.family == "spike":
        tgt = mw.multi_targets(Q, NW, WIN)
        for q in range(Q):
            wi.plant(key, tok, up(guides[q]).expand(NW, D), tgt[q], scale, 0, False, divide=1.0)
    key, value = key.float().bfloat16(), rnd(N, D).bfloat16()
    like = wi.Run("fwd", run.geom, D)
    cc = SimpleNamespace(D=D, WIN=WIN, bias=0.0, value=value, key=key)
    per = [R.window_attention_ref(up(key), up(value), up(guides[q]).expand(NW, D), geom, scale, 0.0) for q in range(Q)]
    want = wi.ctx16_of(torch.stack([fw["ctx"] for fw in per]))
    tol = torch.stack([wi.forward_bounds_of(like, cc, fw)["ctx16"] for fw in per])
    s = torch.stack([fw["s"] for fw in per])
    logits = (up(guides) @ up(key).T).float()
    T, H, W, kt, ks = geom
    return SimpleNamespace(run=run, geom=geom, Q=Q, N=N, NW=NW, WIN=WIN, tok=tok, scale=scale, value=value, logits=logits, want=want, tol=tol, s=s,
                           axes=((T, kt, T // kt), (H, ks, H // ks), (W, ks, W // ks)))


LOCAL_MUTANTS = ("uniform", "logits_of_guide_0", "no_scale", "next_window")


def local_mutant(run, name):
    """The contexts under one planted fault (None where it computes the same function):
      uniform             weights 1 / WIN, the logits ignored (WIN > 1)
      logits_of_guide_0   guide 0's logits for every guide (Q > 1)
      no_scale            the 1 / sqrt(D) scale missing (WIN > 1)
      next_window         window w takes the logits of window w + 1 (the last one those of the first; more than one window)"""
    b = local_build(run)
    s = up(b.logits)[:, b.tok] * b.scale                                       # [Q, NW, WIN]
    if name == "uniform":
        s = torch.zeros_like(s)
    elif name == "logits_of_guide_0":
        if b.Q == 1:
            return None
        s = s[:1].expand_as(s)
    elif name == "no_scale":
        s = s / b.scale
    elif name == "next_window":
        if b.NW == 1:
            return None
        s = s.roll(-1, 1)
    else:
        raise KeyError(name)
    p = torch.softmax(s, -1)
    return wi.ctx16_of(torch.einsum("qwi,wid->qwd", p, up(b.value)[b.tok]))


def local_reference_from_logits(run):
    """The unmutated contexts from the logits the kernel receives (not from the keys): what the power test holds against `want`."""
    b = local_build(run)
    p = torch.softmax(up(b.logits)[:, b.tok] * b.scale, -1)
    return wi.ctx16_of(torch.einsum("qwi,wid->qwd", p, up(b.value)[b.tok]))

