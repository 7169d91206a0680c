"""Inputs, float64 references and derived error bounds for the window kernels of csrc/local_attn.hip (local_attn_kernel,
local_attn_adapt_kernel, local_attn_bwd_kernel) and trilinear_pool_kernel (csrc/rowwise_ops.hip).  Shared by
tests/test_gpu_window_attn.py (the kernels against the references) and tests/test_window_attn_power.py (CPU: what a wrong kernel
would do to the references, against the same bounds).

Why a family (the pattern of tests/global_stream_inputs.py): under N(0, 1) logits every weight of a window is about 1 / WIN, and a
kernel that loses a token at a pass boundary, takes its statistics over the first 64 scores only or skips the maximum stays inside
any honest bound.  Here the mass of every window sits where a window kernel can go wrong:

  spiked positions  window positions 0, 3, 4 and WIN - 1 at the full height SHIFT (the four waves take tokens w, w + 4, ...); at
                    0.6 SHIFT the last position before and the first behind every pass boundary -- multiples of 12 (forward, phase 2
                    of the backward) and of 8 (adaptor forward, phase 1 of the backward) -- and positions 63 and 64 (the second trip
                    of the 64-lane loops of softmax_stats and of the backward's dS loop).  Pass boundaries beyond position 128 are
                    spiked only at the last one of each pass length: for WIN <= 100 that is every boundary, and the 2401-token
                    window keeps its mass on a few tokens.  A window of 2 .. 7 tokens has no pass boundary inside: its last position
                    takes 0.6 SHIFT, so that it too has two heights (the split of the mass between them depends on the logit scale).
  window diversity  window w leaves out spike w mod k of its k spikes, so windows do not share a maximum.  A grid of ONE window leaves
                    none out (there is no other window, and its first position has to carry mass for a lost first token to show).
  planting          through the key rows along the window's query: k_n += target / scale q / |q|^2 before rounding to the stream
                    dtype (adaptor forward: through the x stream, the (1 - a_k) factor divided out).  With normalised key rows the
                    spike changes the row's norm: the coefficient c of k_n + c q / |q| that raises scale cos by the target is solved
                    for (bisection), scale = 30 (a clip-scale e^ls).  A token that several windows hold is seen by each of them; with
                    one shared query it is planted once.  The references simply compute what results.
  values            random rows: every spiked token's value row differs from the others.
  guards            tests/test_gpu_window_attn.py uploads every stream as an interior view of a larger buffer with a NaN row in front
                    and behind (guard_rows / guard_query here), and fills every output with NaN.

Geometries (T, H, W, kt, ks), window size, what they cover: GEOMS below.  RUNS lists what is run for each kernel (the option matrix).
"""
import functools
import math
from types import SimpleNamespace
from typing import NamedTuple

import torch

import ops_reference as R
from ops_reference import EPS23, sum_tol, up

SHIFT = 8.0
LOW = 0.6                   # spike_weight of tests/many_item_inputs.py / global_stream_inputs.py
TRANS = 2.0 ** -21          # a device transcendental (tests/test_gpu_ops_small.py)
BF16_RND, F16_RND, F16_SUB = 2.0 ** -8, 2.0 ** -10, 2.0 ** -24
CLIP_SCALE = 30.0
NAN = float("nan")
DT = {"bf16": torch.bfloat16, "f32": torch.float32, "f16": torch.float16}

GEOMS = {
    "w1": (1, 1, 1, 1, 1),            # WIN 1: one token
    "w3": (3, 1, 1, 3, 1),            # WIN 3: one wave idle
    "w8": (2, 2, 2, 2, 2),            # WIN 8: one 8-pass exactly
    "w12": (3, 2, 2, 3, 2),           # WIN 12: one 12-pass exactly
    "w16": (4, 2, 2, 4, 2),           # WIN 16: two 8-passes; 12 + 4
    "w18_all": (3, 7, 5, 2, 3),       # WIN 18: overlap on every axis (12 windows; y has two trailing windows)
    "w24": (6, 2, 2, 6, 2),           # WIN 24: full passes at both pass lengths
    "w36_mask7": (7, 7, 5, 4, 3),     # WIN 36: 12 windows, overlap on every axis: parity mask 7
    "w36_exact": (8, 6, 6, 4, 3),     # WIN 36: exact partition
    "w36_y": (4, 8, 3, 4, 3),         # WIN 36: only y overlaps (nfull = 2, one trailing window)
    "w36_t": (7, 3, 3, 4, 3),         # WIN 36: only t overlaps
    "w36_x": (4, 3, 5, 4, 3),         # WIN 36: only x overlaps
    "w72": (8, 6, 3, 8, 3),           # WIN 72: two windows; second trip of the 64-lane loops
    "w100": (4, 10, 5, 4, 5),         # WIN 100: two windows
    "w36_real": (4, 27, 27, 4, 3),    # WIN 36: one case of the real grid, D = 1152 only
    "w2401": (1, 49, 49, 1, 49),      # WIN 2401: many trips of softmax_stats; the backward's LDS does not fit (refused)
}


class Run(NamedTuple):
    kernel: str                   # "fwd" | "adapt" | "bwd"
    geom: str
    D: int
    key_dt: str = "bf16"
    value_dt: str = "bf16"
    l2norm: int = 0               # fwd: bits; bwd: 1 = l2norm_key
    query: str = "bf16_shared"    # bf16_shared (stride 0) | bf16_win | f32_win | f32_strided (stride D + 24)
    out: str = "ctx"              # fwd: ctx | ctx16 | both
    bias: float = 0.25
    big_value: bool = False       # fwd: one f32 value row holds 1e5 at the position that carries most of the window's mass
    which: str = "both"           # adapt: key | value | both
    alpha_dt: str = "bf16"
    value_is_key: bool = False    # bwd: dvalue alone, the key-side gradient added in; else dkey and dvalue

    @property
    def id(self):
        d = self._asdict()
        base = Run(self.kernel, self.geom, self.D)._asdict()
        return "-".join([self.kernel, self.geom, str(self.D)] + [f"{k}={v}" for k, v in d.items() if v != base[k]])


def _runs():
    fwd, adapt, bwd = [], [], []
    for name in GEOMS:
        if name == "w2401":
            continue
        for D in ((1152,) if name == "w36_real" else (768, 1152)):
            fwd.append(Run("fwd", name, D))
    fwd.append(Run("fwd", "w2401", 768))
    for kd in DT:                                                     # all 9 key x value dtype pairs at WIN 18
        for vd in DT:
            if (kd, vd) != ("bf16", "bf16"):
                fwd.append(Run("fwd", "w18_all", 768, key_dt=kd, value_dt=vd))
    for l2 in (1, 2, 3):
        fwd += [Run("fwd", "w18_all", 1152, l2norm=l2), Run("fwd", "w72", 768, l2norm=l2)]
    for q in ("bf16_win", "f32_win", "f32_strided"):
        fwd += [Run("fwd", "w16", 768, query=q), Run("fwd", "w36_mask7", 1152, query=q)]
    fwd += [Run("fwd", "w36_mask7", 768, out="ctx16"), Run("fwd", "w36_mask7", 768, out="both"),
            Run("fwd", "w3", 1152, out="both", value_dt="f32", big_value=True)]
    fwd += [Run("fwd", "w36_exact", 1152, bias=95.0), Run("fwd", "w100", 768, bias=95.0)]
    for i, name in enumerate(("w1", "w3", "w16", "w18_all", "w36_mask7", "w72")):
        for j, which in enumerate(("key", "value", "both")):
            D = (768, 1152)[(i + j) % 2]
            adapt.append(Run("adapt", name, D, which=which, alpha_dt=("bf16", "f32")[(i + j // 2) % 2],
                             query=("bf16_shared", "f32_win")[j % 2 if which != "both" else i % 2]))
    for i, name in enumerate(n for n in GEOMS if n != "w2401"):
        D = 1152 if name == "w36_real" else (768, 1152)[i % 2]
        bwd.append(Run("bwd", name, D, query=("bf16_shared", "f32_win")[i % 2]))
        bwd.append(Run("bwd", name, D, query=("f32_win", "bf16_shared")[i % 2], value_is_key=True))
    for name, D, q in (("w16", 1152, "bf16_win"), ("w36_mask7", 768, "bf16_shared"), ("w72", 1152, "f32_win")):
        bwd += [Run("bwd", name, D, l2norm=1, query=q), Run("bwd", name, D, l2norm=1, query=q, value_is_key=True)]
    return tuple(fwd), tuple(adapt), tuple(bwd)


FWD_RUNS, ADAPT_RUNS, BWD_RUNS = _runs()
RUNS = FWD_RUNS + ADAPT_RUNS + BWD_RUNS
assert len({r.id for r in RUNS}) == len(RUNS)

POOLS = (((7, 7, 5), (2, 3, 2)), ((4, 27, 27), (1, 9, 9)), ((8, 6, 6), (8, 6, 6)), ((1, 6, 6), (1, 2, 2)), ((5, 3, 2), (2, 1, 1)))
POOL_D = (1152, 768, 8)


# ---- the family -----------------------------------------------------------------------------------------------------------------
def spike_positions(WIN):
    """{position: height / SHIFT} of one window."""
    pos = {}
    for step in (12, 8):
        edges = [b for b in range(step, WIN, step)]
        for b in [b for b in edges if b <= 128] + edges[-1:]:
            pos[b - 1] = pos[b] = LOW
    if WIN > 64:
        pos[63] = pos[64] = LOW
    for i in (0, 3, 4, WIN - 1):
        if 0 <= i < WIN:
            pos[i] = 1.0
    if 1 < WIN < 8:                   # no pass boundary inside: the last position takes the second height
        pos[WIN - 1] = LOW
    return dict(sorted(pos.items()))


def spike_targets(NW, WIN):
    """[NW, WIN]: the height of position i's spike in window w; with more than one window, window w leaves out spike w mod k."""
    pos = spike_positions(WIN)
    tgt = torch.zeros(NW, WIN, dtype=torch.float64)
    for i, h in pos.items():
        tgt[:, i] = SHIFT * h
    if NW > 1:
        keys = list(pos)
        for w in range(NW):
            tgt[w, keys[w % len(keys)]] = 0.0
    return tgt


def _rise(rows, u, qlen, c, scale, qn, key_norm):
    """scale q . (k + c u) / (|k + c u| if key_norm) / qn for rows k [M, D], unit vector u, |q| = qlen, coefficients c [M]."""
    dot = (rows @ u) * qlen + c * qlen
    if key_norm:
        dot = dot / torch.sqrt((rows * rows).sum(1) + 2 * c * (rows @ u) + c * c)
    return scale * dot / qn


def plant(rows, tok, q, tgt, scale, l2norm, shared, divide=1.0):
    """Raises the logit of (window w, position i) by tgt[w, i] through rows[tok[w, i]] (float64, in place), window by window."""
    done = set()
    for w in range(tok.shape[0]):
        sel = [i for i in range(tok.shape[1]) if tgt[w, i] > 0 and not (shared and int(tok[w, i]) in done)]
        if not sel:
            continue
        t = tok[w, sel]
        done.update(t.tolist())
        qw = q[w]
        qlen = float(qw.norm())
        u, qn = qw / qlen, (qlen if l2norm & 2 else 1.0)
        want = tgt[w, sel]
        if l2norm & 1:
            k = rows[t]
            base = _rise(k, u, qlen, torch.zeros(len(sel), dtype=torch.float64), scale, qn, True)
            lo, hi = torch.zeros(len(sel), dtype=torch.float64), torch.full((len(sel),), 64.0, dtype=torch.float64) * k.norm(dim=1)
            assert bool((_rise(k, u, qlen, hi, scale, qn, True) - base > want).all()), "spike out of reach of scale cos"
            for _ in range(70):
                mid = 0.5 * (lo + hi)
                over = _rise(k, u, qlen, mid, scale, qn, True) - base > want
                hi, lo = torch.where(over, mid, hi), torch.where(over, lo, mid)
            c = 0.5 * (lo + hi)
        else:
            c = want * qn / (scale * qlen)
        rows[t] += (c / divide)[:, None] * u[None, :]


def _seed(id):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(id)) % (2 ** 31)


def _query(run, NW, D, rnd, small):
    """(q as uploaded: [1 | NW, D] in its dtype, stride)."""
    shared = run.query == "bf16_shared"
    q = rnd(1 if shared else NW, D) * ((1.0 / math.sqrt(D)) if small else 1.0)
    if run.kernel == "fwd" and run.l2norm & 2:
        q = q * 1.25                     # |q| away from 1: a query that is not normalised shows
    q = q.to(torch.bfloat16 if run.query.startswith("bf16") else torch.float32)
    return q, (0 if shared else (D + 24 if run.query == "f32_strided" else D))


@functools.lru_cache(maxsize=None)
def build(run):
    """The tensors of `run` as the kernels receive them (CPU; callers must not write into them)."""
    T, H, W, kt, ks = geom = GEOMS[run.geom]
    D, N = run.D, T * H * W
    tok, widx = R.window_tokens(*geom)
    NW, WIN = tok.shape
    g = torch.Generator().manual_seed(_seed(run.id))
    rnd = lambda *s: torch.randn(*s, generator=g)
    c = SimpleNamespace(run=run, geom=geom, D=D, N=N, NW=NW, WIN=WIN, tok=tok, bias=run.bias)
    c.exact = tok.numel() == N
    c.tgt = spike_targets(NW, WIN)
    shared = run.query == "bf16_shared"
    normed = run.l2norm != 0
    # plain: flat logits ~ N(0, 1).  Adaptor forward: a quarter of that -- its logit bound (four chained D-term sums) is four times
    # as wide, and the flat logits' absolute terms are most of it
    c.scale = CLIP_SCALE if normed else (0.25 if run.kernel == "adapt" else 1.0) / math.sqrt(D)
    c.q, c.q_stride = _query(run, NW, D, rnd, small=normed)
    qd = up(c.q).expand(NW, D)
    if run.kernel == "adapt":
        use_k, use_v = run.which in ("both", "key"), run.which in ("both", "value")
        adt = DT[run.alpha_dt]
        c.ak, c.av = (torch.tensor([0.4]).to(adt) if use_k else None), (torch.tensor([0.7]).to(adt) if use_v else None)
        kx = rnd(N, D).double()
        plant(kx, tok, qd, c.tgt, c.scale, 0, shared, divide=1.0 - (float(c.ak.double()) if use_k else 0.0))
        # the logit bound of this kernel is wide (four chained D-term sums): the value rows of the tokens at the second height are
        # ten times as large, so that the split of the mass between the two heights (scale_1.1) owns a share of the contexts
        vx = rnd(N, D)
        low = tok[(c.tgt > 0) & (c.tgt < SHIFT)].unique()
        vx[low] *= 10.0
        c.kx, c.vx = kx.float().bfloat16(), vx.bfloat16()
        c.ky = (rnd(N, D) * 1.5 + 0.3).half() if use_k else None
        c.vy = (rnd(N, D) * 0.7 - 0.2).half() if use_v else None
        c.kg, c.kb, c.vg, c.vb = ((1 + 0.1 * rnd(D)).bfloat16(), (0.1 * rnd(D)).bfloat16(), (1 + 0.1 * rnd(D)).bfloat16(),
                                  (0.1 * rnd(D)).bfloat16())
        return c
    key = rnd(N, D).double() * ((1.0 / math.sqrt(D)) if run.l2norm == 2 and run.kernel == "fwd" else 1.0)
    tgt = c.tgt
    if run.big_value:                       # the last token of window 0 carries most of the window's mass
        tgt = tgt.clone()
        tgt[0, WIN - 1] = SHIFT + 2.0
    plant(key, tok, qd, tgt, c.scale, run.l2norm if run.kernel == "fwd" else (1 if run.l2norm else 0), shared)
    c.key = key.float().to(DT[run.key_dt])
    if run.kernel == "bwd" and run.value_is_key:
        c.value = c.key
    else:
        value = rnd(N, D)
        if run.big_value:
            value[int(tok[0, WIN - 1]), 5] = 1.0e5
        c.value = value.to(DT[run.value_dt])
    if run.kernel == "bwd":
        # the upstream gradient has a component along the window's own context: delta = sum_j p_j dP_j is then as large as the dP
        # themselves, and a backward without it shows
        fw = R.window_attention_ref(up(c.key), up(c.value), qd, geom, c.scale, c.bias, l2norm=1 if run.l2norm else 0)
        c.dctx = (rnd(NW, D).double() + fw["ctx"]).float()
    return c


def guard_rows(t, device):
    """t [N, D] as rows 1 .. N of an [N + 2, D] device buffer whose first and last row are NaN (a dense interior view)."""
    buf = torch.full((t.shape[0] + 2, t.shape[1]), NAN, dtype=t.dtype, device=device)
    buf[1:-1] = t.to(device)
    return buf[1:-1]


def guard_query(q, stride, device):
    """q [rows, D] at row pitch max(stride, D) inside a NaN-filled flat device buffer, one NaN row in front and behind; the gaps of a
    strided query are NaN too.  Returns the flat view that starts at row 0 of q."""
    rows, D = q.shape
    pitch = max(stride, D)
    buf = torch.full(((rows + 2) * pitch,), NAN, dtype=q.dtype, device=device)
    buf[pitch:(rows + 1) * pitch].view(rows, pitch)[:, :D] = q.to(device)
    return buf[pitch:(rows + 1) * pitch]


# ---- references of a run ----------------------------------------------------------------------------------------------------------
def _adapt_rows(c):
    """Blended key and value rows of an adaptor run and their absolute terms."""
    def one(x, y, ga, be, a):
        x = up(x)
        if y is None:
            return x, x.abs()
        a = float(a.double())
        return (R.blend_rows(x, up(y), up(ga), up(be), a, 1e-6)[0],
                R.ln_blend_ref(up(y), up(ga), up(be), x, a, 1e-6)[1])
    return one(c.kx, c.ky, c.kg, c.kb, c.ak), one(c.vx, c.vy, c.vg, c.vb, c.av)


def forward_ref(run, scale_mul=1.0, l2norm=None, **faults):
    """window_attention_ref of a forward or adaptor-forward run; the keywords plant faults."""
    c = build(run)
    qd = up(c.q).expand(c.NW, c.D)
    if run.kernel == "adapt":
        (K, Kab), (V, Vab) = _adapt_rows(c)
        return R.window_attention_ref(K, V, qd, c.geom, c.scale * scale_mul, c.bias, key_ab=Kab, value_ab=Vab, **faults)
    return R.window_attention_ref(up(c.key), up(c.value), qd, c.geom, c.scale * scale_mul, c.bias,
                                  l2norm=run.l2norm if l2norm is None else l2norm, **faults)


def backward_ref(run, scale_mul=1.0, l2norm_key=None, **faults):
    c = build(run)
    return R.window_attention_bwd_ref(up(c.key), up(c.value), up(c.q).expand(c.NW, c.D), up(c.dctx), c.geom, c.scale * scale_mul, c.bias,
                                      l2norm_key=bool(run.l2norm) if l2norm_key is None else l2norm_key, value_is_key=run.value_is_key,
                                      **faults)


@functools.lru_cache(maxsize=None)
def reference(run):
    return backward_ref(run) if run.kernel == "bwd" else forward_ref(run)


def ctx16_of(ctx):
    """What ctx16 stands for: the context saturated at the fp16 range."""
    return ctx.clamp(-65504.0, 65504.0)


# ---- error bounds, from the references' own quantities ----------------------------------------------------------------------------
def _norm_rel(D):
    """Relative error of 1 / |row| in fp32: the D-term sum of squares (D 2^-23, halved by the square root), the square root and the
    division (up to 4 units each where they are not correctly rounded)."""
    return (D / 2 + 8) * EPS23


def logit_tol(run, c, s_ab):
    """|d s| of s = scale dot (/ norms) + bias, s_ab = scale sum |q_j| |k_j| (/ norms):
      plain      the D-term fp32 dot product, the product with scale and the addition of bias: (D + 2) 2^-23 s_ab + 2^-23 |bias|
                 (the last rounding is 2^-24 |s| <= 2^-24 (s_ab + |bias|), counted in both terms)
      l2norm     every set bit divides by a norm: + _norm_rel(D) s_ab per bit (bit 2 also rounds every q_j / |q|: one more unit)
      adaptor    four chained D-term sums (LayerNorm mean and variance, the x and the y dot product) bounded together by
                 4 D 2^-23 on the absolute terms of the blended expression, as tests/test_gpu_ops_small.py bounds the backward."""
    D = c.D
    if run.kernel == "adapt":
        return sum_tol(4 * D + 2, s_ab) + EPS23 * abs(c.bias)
    bits = (run.l2norm & 1) + ((run.l2norm >> 1) & 1) if run.kernel == "fwd" else (1 if run.l2norm else 0)
    return sum_tol(D + 2, s_ab) + bits * (_norm_rel(D) + EPS23) * s_ab + EPS23 * abs(c.bias)


def weight_rel(o, d_s, WIN):
    """Relative error of a softmax weight p_i = expf(s_i - mx) / sum_j expf(s_j - mx), [NW, WIN]:
      a logit error of at most d (the window's largest) moves it by at most e^(2 d) - 1;
      expf twice, numerator and sum: 2 TRANS;  the subtraction s - mx rounds to 2^-24 |s - mx| in the exponent, in the numerator and
      (weighted) in the sum: 2^-23 (|s_i - mx| + sum_j p_j |s_j - mx|) at most (weights below e^-104 are zero);
      the WIN-term sum and the reciprocal and product behind it: (WIN + 2) 2^-23."""
    d = d_s.max(1, keepdim=True).values
    span = (o["mx"] - o["s"]).clamp(0.0, 104.0)
    arg = EPS23 * (span + (o["p"] * span).sum(1, keepdim=True))
    return torch.expm1(2 * d) + 2 * TRANS + (WIN + 2) * EPS23 + arg


def forward_bounds(run, fw):
    """Bounds of ctx (and ctx16) of a forward / adaptor-forward run:
      ctx    sum_i p_i v_i: the weights' error (weight_rel) times p_i |v_i|, + the (WIN + 4)-term fp32 sum (WIN FMAs over the waves'
             tokens, the four partial rows): (WIN + 4) 2^-23 ctx_ab.
             Adaptor value path: v_i = (1 - a) x_i + a (gamma yhat_i + beta) is never formed; |v_i| stands for its absolute terms,
             yhat carries the LayerNorm statistics' error 2 D 2^-23 (|y| + |mu|) rstd (as in the adaptor backward's test), times
             a |gamma| p_i, and the blend of the two accumulators adds 6 roundings on ctx_ab.
      ctx16  the same, + one rounding to fp16 (2^-10 |ref|, 2^-24 in the subnormal range), of the value saturated at +-65504."""
    return forward_bounds_of(run, build(run), fw)


def forward_bounds_of(run, c, fw, d_s_more=0.0):
    """forward_bounds on tensors `c` of the caller's own (tests/multi_window_inputs.py: one guide of a multi-guide run); run: what
    logit_tol reads (kernel, l2norm).  d_s_more: a further term of the logit bound, [NW, WIN]."""
    d_s = logit_tol(run, c, fw["s_ab"]) + d_s_more
    rel = weight_rel(fw, d_s, c.WIN)
    tok = fw["tok"]
    if run.kernel == "adapt":
        (_, _), (_, Vab) = _adapt_rows(c)
    else:
        Vab = up(c.value).abs()
    tol = torch.einsum("wi,wid->wd", fw["p"] * rel, Vab[tok]) + sum_tol(c.WIN + 4, fw["ctx_ab"])
    if run.kernel == "adapt" and c.vy is not None:
        y = up(c.vy)
        mu, rstd = R.layer_norm_stats(y, 1e-6)
        drow = 2 * c.D * EPS23 * (y.abs() + mu.abs()) * rstd * up(c.vg).abs() * float(c.av.double())
        tol = tol + torch.einsum("wi,wid->wd", fw["p"], drow[tok]) + 6 * EPS23 * fw["ctx_ab"]
    return {"d_s": d_s, "p": rel * fw["p"], "ctx": tol, "ctx16": tol + F16_RND * ctx16_of(fw["ctx"]).abs() + F16_SUB}


def backward_bounds(run, bw):
    """Bounds of dq, dls, dkey, dvalue of a backward run (the derivation of test_local_attn_adapt_bwd_matches_fp64_reference, with the
    plain kernel's terms).  Per window, wsum(v) = sum_j v_j:
      s, dP   logit_tol;  dP_i = dctx . v_i, a D-term dot product: (D + 1) 2^-23 dP_ab
      p       weight_rel
      dS      p (dP - delta), delta = sum_j p_j dP_j: the weight's error on both terms, dP's error on both, 4 roundings:
              (p_rel + 4 2^-23) p (|dP| + wsum(p |dP|)) + p (d_P + wsum(p d_P)) + p wsum(p p_rel |dP|)
      dls     sum_i dS_i (s_i - bias): dS's error times |s_i - bias|, + |dS_i| times the error of s_i - bias (the logit's, + the
              subtraction's rounding 2^-23 (|s_i| + |bias|)), + the (WIN + 2)-term sum
      dsk     scale dS r, r = 1 / |k|: scale r (d_dS + |dS| (norm_rel + 3 2^-23))
      dq      sum_i dsk_i k_i: d_dsk |k_i|, + the (WIN + 4)-term sum
      dk_i    dsk q - kc k, kc = dsk (q . khat) r: d_dsk |q| + d_kc |k| + 2 roundings of the two terms,
              d_kc = d_dsk |sraw| r + |dsk| r (d_sraw + |sraw| (norm_rel + 3 2^-23)), d_sraw the logit's error / scale
      dv_i    p_i dctx (+ dk_i): p_rel p |dctx| + 2 roundings (+ d_dk_i)
      dkey / dvalue  the contributions arrive launch by launch (the reference's `steps`): each read-modify-write adds the contribution's
              own error, the fp32 addition's rounding, and one rounding to bf16 of the running sum, 2^-8 (|running sum| + its error so
              far).  A token written once (exact partition, or held by one window) sees exactly one rounding."""
    c = build(run)
    D, WIN, scale = c.D, c.WIN, c.scale
    q, g = up(c.q).expand(c.NW, D), up(c.dctx)
    K = up(c.key)[bw["tok"]]
    nr = _norm_rel(D) if run.l2norm else 0.0
    wsum = lambda v: v.sum(1, keepdim=True)
    d_s = logit_tol(run, c, bw["s_ab"])
    d_sraw = (d_s - EPS23 * abs(c.bias)) / scale
    d_P = sum_tol(D + 1, bw["dP_ab"])
    p, dP, dS = bw["p"], bw["dP"], bw["dS"]
    p_rel = weight_rel(bw, d_s, WIN)
    d_dS = (p_rel + 4 * EPS23) * p * (dP.abs() + wsum(p * dP.abs())) + p * (d_P + wsum(p * d_P)) + p * wsum(p * p_rel * dP.abs())
    sb = bw["s"] - c.bias
    out = {"dls": (d_dS * sb.abs() + dS.abs() * (d_s + EPS23 * (bw["s"].abs() + abs(c.bias)))).sum(1) + sum_tol(WIN + 2, bw["dls_ab"])}
    d_dsk = scale * bw["r"] * (d_dS + dS.abs() * (nr + 3 * EPS23))
    out["dq"] = torch.einsum("wi,wid->wd", d_dsk, K.abs()) + sum_tol(WIN + 4, bw["dq_ab"])
    d_kc = d_dsk * bw["sraw"].abs() * bw["r"] + bw["dsk"].abs() * bw["r"] * (d_sraw + bw["sraw"].abs() * (nr + 3 * EPS23))
    if not run.l2norm:
        d_kc = torch.zeros_like(d_kc)
    d_dk = d_dsk[:, :, None] * q.abs()[:, None, :] + d_kc[:, :, None] * K.abs()
    d_dv = (p_rel * p)[:, :, None] * g.abs()[:, None, :]
    if run.value_is_key:
        d_dv = d_dv + d_dk
    for name, rows_key, ab_key, d_rows in (("dkey", "dk", "dk_ab", d_dk), ("dvalue", "dv", "dv_ab", d_dv)):
        run_sum = torch.zeros(c.N, D, dtype=torch.float64)
        tol = torch.zeros(c.N, D, dtype=torch.float64)
        for st in bw["steps"]:
            t = st["tok"]
            e_tol = d_rows[st["win"]].reshape(-1, D) + 2 * EPS23 * st[ab_key]
            tol[t] += e_tol + EPS23 * (run_sum[t].abs() + st[rows_key].abs())
            run_sum[t] += st[rows_key]
            tol[t] += BF16_RND * (run_sum[t].abs() + tol[t])
        out[name] = tol
    return out


def bwd_outputs(run):
    return ("dq", "dls", "dvalue") if run.value_is_key else ("dq", "dls", "dkey", "dvalue")


# ---- pooled queries ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool_input(shape, D):
    g = torch.Generator().manual_seed(sum(shape) * 7 + D)
    return torch.randn(*shape, D, generator=g).bfloat16()


def pool_bounds(shape, ab, slopes):
    """out = nested lerps t, h, w of products tap * weight: 7 roundings on the absolute-weighted sum (3 levels of two products and one
    addition, the weights 1 - lam one more); the source index (i + 0.5) n_in / n_out - 0.5 is formed in fp32 and is below n_in:
    n_in 2^-23 per axis, times that axis' difference of neighbouring taps (on either side: a source index that should be a grid
    point may land just below it)."""
    return 7 * EPS23 * ab + sum(n * EPS23 * s for n, s in zip(shape, slopes))
