"""Inputs, float64 references and derived error bounds for the two global-stage stream kernels (csrc/global_stream.hip:
global_stream_kernel, the one-row-group "narrow" form, and global_stream_wide_kernel, the many-row "wide" form) and the merge behind
them (csrc/merge.hip).  Shared by tests/test_gpu_global_stream.py (the kernels against the references) and
tests/test_global_stream_power.py (CPU: what a wrong kernel would do to the references, against the same bounds).

Why a family (the pattern of tests/many_item_inputs.py): under N(0, 1) logits every softmax weight is about 1 / N and a chunked
kernel that loses a token, takes a token for the wrong frame or drops a positional term stays inside any honest bound.  Here the mass
sits, on purpose, where a chunked kernel can go wrong:

  spiked tokens   the clip's tokens 0, 15, 16 and N - 1 at the full height SHIFT; at 0.6 SHIFT (spike_weight, as many_item_inputs) the
                  last token in front of and the first token behind every chunk boundary -- of every chunk count the case is run with
                  -- and every frame boundary.  Two heights: the split of the mass between the two groups depends on the logit scale.
  chunk rule      chunk c of nparts covers the 16-token tiles [ntiles c // nparts, ntiles (c + 1) // nparts), ntiles = ceil(N / 16):
                  restated here from the kernels (`tb`, `te`), never taken from hicom_amd.
  row diversity   row r leaves out spike r mod k of the k spiked tokens, every row carries its own positional table, and a query is
                  the sum of a direction all rows share and one of its own: rows of one 16-row group do not share a maximum.
  forward         the spikes rise through q . x: x_n += Q^+ target_n (minimum-norm solution of q_r . add = target[r, n] for all rows),
                  so every spiked token's value row differs from every other's.
  backward        s_in is an input of the kernel and is spiked directly; (M, L) from it in float64, rounded to fp32; delta is the true
                  g_r . ctx_r of these inputs (every row of dS then sums to zero, and leaving delta out is visible).
  tables          pos_a ~ N(0, 0.7) per entry, three entries per logit, against flat dot products ~ N(0, 1); pos_b = g . pe^T as the
                  product forms it (same magnitude as g . x); pe ~ N(0, 0.5), max |pe| > 0.5.  The tables are wider than the columns
                  used (pos_stride > x_index0 + W) and the frame block starts at t_index0 = t0.  Rows >= R of pos_a / pos_b hold
                  finite garbage, rows >= R and columns >= N of s_in NaN: none of it may reach an output.

Which kernel form runs (restated from wide_ok / hicom_global_stream_has_marg; the GPU tests assert the native predicate agrees):
  wide    E = 1152, rows_pad a multiple of 32, H, W <= 64 and, with a positional table, a chunk spanning at most 8 frames:
          ceil((ceil(ntiles / nparts) + 1) 16 / HW) + 1 <= 8
  marg    wide, [frames | H | W] in at most 8 blocks of 16 columns, N = T H W, and room for the merge's weight record in the row's
          scratch: 2 + nparts + T + H + W <= T (H + W + 2)   (so never at T = 1)
"""
import functools
import math
from types import SimpleNamespace
from typing import NamedTuple

import torch

import ops_reference as R
from ops_reference import EPS23, sum_tol, up

SHIFT = 8.0
TRANS = 2.0 ** -21          # a device transcendental (tests/test_gpu_ops_small.py)
PSPLIT = 2.0 ** -16         # a weight handed to the matrix cores as bf16 hi + lo: |w - hi - lo| <= 2^-17 |w| (common.hpp split_bf16), doubled
CORE = 4                    # tokens 0, 15, 16, N - 1


class Entry(NamedTuple):
    id: str
    form: str               # "marg": wide with in-kernel marginals; "wide": wide, logit-tensor form; "narrow"; see the module docstring
    E: int
    grid: tuple             # (T, H, W)
    R: int
    nparts: tuple
    t0: int = 0
    pos: bool = True
    refuse_marg: bool = False      # the shape sits just outside hicom_global_stream_has_marg: asking for part_marg must be refused


# nparts: {2, the suggested count, one tile per chunk} where the predicates allow it.  The suggested count is ntiles // 4 at these
# sizes (hicom_global_stream_nparts: >= 4 tiles per chunk; the chip-filling count is never the smaller one here).
CASES = (
    # ---- wide form with in-kernel marginals, E = 1152 ----
    Entry("marg_8x6x6_r27", "marg", 1152, (8, 6, 6), 27, (2, 4, 18)),                   # N = 288: full tiles; rows_pad 32
    Entry("marg_8x6x6_r33", "marg", 1152, (8, 6, 6), 33, (2, 4, 18), t0=5),             # rows_pad 64: a half-filled group + a padding-only group
    Entry("marg_8x6x6_r288", "marg", 1152, (8, 6, 6), 288, (2, 4, 18), t0=5),           # 9 workgroups of two full groups
    Entry("marg_4x7x5_r27", "marg", 1152, (4, 7, 5), 27, (2, 9), t0=5),                 # N = 140: masked tail of 12 (suggested = 2)
    Entry("marg_4x7x5_r33", "marg", 1152, (4, 7, 5), 33, (2, 9)),
    Entry("marg_2x9x9_r27", "marg", 1152, (2, 9, 9), 27, (2, 11)),                      # N = 162: tail of 2, the frame boundary inside tile 5
    Entry("marg_2x9x9_r33", "marg", 1152, (2, 9, 9), 33, (2, 11), t0=5),
    # N = 544: H needs two marginal blocks, W exactly one.  One tile per chunk (34) leaves no room for the weight record
    # (2 + 34 + 2 + 33 > 70): 33 chunks, all of one tile but one, is the nearest allowed and sits exactly on that limit
    Entry("marg_2x17x16_r27", "marg", 1152, (2, 17, 16), 27, (2, 8, 33), t0=5),
    Entry("marg_2x17x16_r33", "marg", 1152, (2, 17, 16), 33, (2, 8, 33)),
    # ---- the 8-frame span of a chunk ----
    Entry("span_12x6x6_np2", "marg", 1152, (12, 6, 6), 27, (2,), t0=5),                 # (14 + 1) 16 / 36 -> 7 (+ 1) frames: exactly the limit
    Entry("span_13x6x6_np2", "narrow", 1152, (13, 6, 6), 27, (2,), refuse_marg=True),   # 8 (+ 1): falls out; narrow kernel, two row groups
    # ---- wide form without in-kernel marginals ----
    Entry("wide_1x12x12_r27", "wide", 1152, (1, 12, 12), 27, (2, 9), refuse_marg=True),  # T = 1: no room for the weight record
    Entry("wide_nopos_4x7x5_r27", "wide", 1152, (4, 7, 5), 27, (2, 9), pos=False),      # pos_a / pos_b NULL
    # ---- narrow form with the positional table on ----
    Entry("narrow_e1152_r9", "narrow", 1152, (4, 7, 5), 9, (1, 2, 3), t0=5),            # (suggested = 2)
    Entry("narrow_e768_r9", "narrow", 768, (4, 7, 5), 9, (1, 2, 3)),
    Entry("narrow_e768_r27", "narrow", 768, (2, 9, 9), 27, (1, 2, 3), t0=5),            # two row groups at E = 768
)
BY_ID = {e.id: e for e in CASES}
assert len(BY_ID) == len(CASES)


# ---- the kernels' chunking and shape predicates, restated -----------------------------------------------------------------------
def ntiles_of(N):
    return (N + 15) // 16


def chunk_tiles(N, nparts):
    """First tile of chunk c for c = 0 .. nparts (the last entry: ntiles)."""
    nt = ntiles_of(N)
    return [nt * c // nparts for c in range(nparts + 1)]


def chunk_token_ranges(N, nparts):
    tb = chunk_tiles(N, nparts)
    return [(16 * tb[c], min(16 * tb[c + 1], N)) for c in range(nparts)]


def chunk_first_frames(N, HW, nparts):
    return [16 * tb // HW for tb in chunk_tiles(N, nparts)[:-1]]


def suggested_nparts(N):
    return max(1, ntiles_of(N) // 4)


def wide_ok(N, E, rows_pad, H, W, nparts, pos=True):
    tiles_per_part = (ntiles_of(N) + nparts - 1) // nparts + 1
    span_ok = not pos or (tiles_per_part * 16 + H * W - 1) // (H * W) + 1 <= 8
    return E == 1152 and rows_pad > 16 and rows_pad % 32 == 0 and (not pos or (H <= 64 and W <= 64)) and span_ok


def has_marg(N, E, rows_pad, H, W, nparts):
    if N % (H * W):
        return False
    T = N // (H * W)
    room = 2 + nparts + T + H + W <= T * (H + W + 2)
    return room and wide_ok(N, E, rows_pad, H, W, nparts) and 1 + (H + 15) // 16 + (W + 15) // 16 <= 8


def form_of(e, nparts):
    T, H, W = e.grid
    N, rows_pad = T * H * W, rows_pad_of(e.R)
    if e.pos and has_marg(N, e.E, rows_pad, H, W, nparts):
        return "marg"
    return "wide" if wide_ok(N, e.E, rows_pad, H, W, nparts, e.pos) else "narrow"


def rows_pad_of(R_):
    """The row padding the product uses: 16 for up to 16 rows, else a multiple of 32 (two row groups per wide workgroup)."""
    return 16 if R_ <= 16 else (R_ + 31) // 32 * 32


# ---- the family -----------------------------------------------------------------------------------------------------------------
def spike_tokens(N, HW, nparts_list):
    toks = {0, 15, 16, N - 1}
    for nparts in nparts_list:
        for tb in chunk_tiles(N, nparts)[1:-1]:
            toks |= {16 * tb - 1, 16 * tb}
    for f in range(1, N // HW):
        toks |= {f * HW - 1, f * HW}
    return sorted(t for t in toks if 0 <= t < N)


def spike_weight(n, N):
    return 1.0 if n in (0, 15, 16, N - 1) else 0.6


def spike_targets(R_, N, toks):
    """[R, N]: the height of token n's spike in row r; row r leaves out spike r mod k."""
    tgt = torch.zeros(R_, N, dtype=torch.float64)
    for n in toks:
        tgt[:, n] = SHIFT * spike_weight(n, N)
    for r in range(R_):
        tgt[r, toks[r % len(toks)]] = 0.0
    return tgt


def split_planes(v, rows_pad):
    """bf16 hi / lo planes of f32 rows (the operands of the stream kernels), zero rows up to rows_pad."""
    hi = torch.zeros(rows_pad, v.shape[1], dtype=torch.bfloat16)
    lo = torch.zeros_like(hi)
    hi[:v.shape[0]] = v.bfloat16()
    lo[:v.shape[0]] = (v - hi[:v.shape[0]].float()).bfloat16()
    return hi, lo


@functools.lru_cache(maxsize=None)
def build(id):
    """The tensors of case `id` as the kernels receive them (CPU; callers must not write into them)."""
    e = BY_ID[id]
    T, H, W = e.grid
    N, E, R_ = T * H * W, e.E, e.R
    rows_pad, stride = rows_pad_of(R_), ntiles_of(N) * 16 + 16
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(id)))
    rnd = lambda *s: torch.randn(*s, generator=g)
    c = SimpleNamespace(entry=e, T=T, H=H, W=W, N=N, E=E, R=R_, rows_pad=rows_pad, stride=stride, t0=e.t0)
    cap = e.t0 + T + 2
    c.y0, c.x0, c.P = cap, cap + H, cap + H + W + 3
    c.toks = spike_tokens(N, H * W, e.nparts)
    tgt = spike_targets(R_, N, c.toks)
    # forward: queries = a shared direction + an own one (flat dot products ~ N(0, 1)), tokens spiked through the pseudo-inverse
    q = ((0.7 * rnd(1, E) + 0.7 * rnd(R_, E)) / math.sqrt(E)).contiguous()
    c.qhi, c.qlo = split_planes(q, rows_pad)
    qd = up(c.qhi)[:R_] + up(c.qlo)[:R_]
    x = rnd(N, E).double() + (torch.linalg.pinv(qd) @ tgt).t()
    c.x = x.float().bfloat16().contiguous()
    c.pe = (rnd(c.P, E) * 0.5).contiguous() if e.pos else None
    c.pos_a = c.pos_b = None
    if e.pos:
        c.pos_a = 3.0 + 2.0 * rnd(rows_pad, c.P)              # rows >= R: garbage of another magnitude
        c.pos_a[:R_] = 0.7 * rnd(R_, c.P)
    # backward
    gq = (0.05 * rnd(R_, E)).contiguous()
    c.dhi, c.dlo = split_planes(gq, rows_pad)
    gd = up(c.dhi)[:R_] + up(c.dlo)[:R_]
    if e.pos:
        c.pos_b = -2.0 + 3.0 * rnd(rows_pad, c.P)
        c.pos_b[:R_] = (gd @ up(c.pe).t()).float()
    c.s_in = torch.full((rows_pad, stride), float("nan"))
    c.s_in[:R_, :N] = (rnd(R_, N).double() + tgt).float()
    Sd = up(c.s_in)[:R_, :N]
    Md = Sd.max(1).values
    c.ml = torch.stack([Md, torch.exp(Sd - Md[:, None]).sum(1)], 1).float().contiguous()
    p = torch.exp(Sd - up(c.ml)[:, 0:1]) / up(c.ml)[:, 1:2]
    dP = R.stream_terms(gd, up(c.x), up(c.pos_b)[:R_] if e.pos else None, None, H, W, e.t0, c.y0, c.x0)[0]
    c.delta = (p * dP).sum(1).float().contiguous()
    return c


def fwd_args(c):
    """What the float64 references take: the up-cast values of the uploaded tensors, real rows only."""
    R_ = c.R
    return dict(q=up(c.qhi)[:R_] + up(c.qlo)[:R_], x=up(c.x), pos_a=up(c.pos_a)[:R_] if c.entry.pos else None,
                pe=up(c.pe) if c.entry.pos else None, H=c.H, W=c.W, t0i=c.t0, y0i=c.y0, x0i=c.x0)


def bwd_args(c):
    R_ = c.R
    return dict(g=up(c.dhi)[:R_] + up(c.dlo)[:R_], x=up(c.x), pos_b=up(c.pos_b)[:R_] if c.entry.pos else None, S=up(c.s_in), ml=up(c.ml),
                delta=up(c.delta), H=c.H, W=c.W, t0i=c.t0, y0i=c.y0, x0i=c.x0)


@functools.lru_cache(maxsize=None)
def forward_ref(id):
    return R.global_stream_ref(**fwd_args(build(id)))


@functools.lru_cache(maxsize=None)
def backward_ref(id):
    return R.global_stream_bwd_ref(**bwd_args(build(id)))


# ---- error bounds, from the references' own quantities ----------------------------------------------------------------------------
def forward_bounds(c, fw, nparts):
    """Bounds of the forward outputs (dict of tensors shaped like the outputs):
      S     2 E products over both bf16 planes accumulated in fp32 on the matrix cores + 3 positional terms, any order:
            (2 E + 3) 2^-23 sum |terms|.
      lse   M + log L.  A logit error of at most d (the row's largest S bound) moves it by at most d.  L: every weight carries the
            device exp (TRANS) and the rounding of its argument S - M and of the product with log2 e (2^-23 |S - M|, weights below e^-104
            are zero), summed over <= N tokens and nparts chunks with the rescales (k 2^-23), and the weight of the chunk in the merge
            (TRANS); the logarithm and the addition: 2 roundings of the result.
      ctx   a logit error d changes a softmax weight by at most e^(2 d) - 1 relative; the weights carry TRANS (exp) + TRANS (the
            chunk's weight) and the argument roundings as above; they reach the matrix cores as bf16 hi + lo (PSPLIT); the sums over
            the tokens, the chunks and the T + H + W positional rows of the merge, the rescales and the division by L: k 2^-23
            sum |terms|, k = N + nparts + T + H + W + 8."""
    e = c.entry
    s_tol = sum_tol(2 * c.E + 3, fw["S_ab"])
    d = s_tol.max(1, keepdim=True).values
    arg = fw["p"] * EPS23 * (fw["M"][:, None] - fw["S"]).clamp(0.0, 104.0)
    k = c.N + nparts + ((c.T + c.H + c.W) if e.pos else 0) + 8
    lse_tol = d[:, 0] + k * EPS23 + 2 * TRANS + arg.sum(1) + 2 * EPS23 * fw["lse"].abs()
    ctx_tol = (torch.expm1(2 * d) + k * EPS23 + 2 * TRANS + PSPLIT) * fw["ctx_ab"] + arg @ fw["vabs"]
    return {"S": s_tol, "lse": lse_tol, "ctx": ctx_tol}


def backward_bounds(c, bw, nparts):
    """Bounds of the backward outputs:
      dS    p (dP - delta).  dP: 2 E products + 3 positional terms + the subtraction, (2 E + 4) 2^-23 (sum |terms| + |delta|), times
            p; p = expf(S - M) / L from the given fp32 S, (M, L): TRANS, the rounding of S - M (2^-24 |S - M|), the reciprocal and the
            two products (3 roundings), times |dS|.
      dSx   sum_n dS x: the dS bounds times |x_n|, + dS as bf16 hi + lo on the matrix cores (PSPLIT) and the sums over <= N tokens
            and nparts chunks: (N + nparts + 8) 2^-23, times sum |dS| |x|.
      marg  the same over the tokens of a frame / grid row / grid column (one-hot matrix-core sums)."""
    S, ml = up(c.s_in)[:c.R, :c.N], up(c.ml)
    p_rel = TRANS + 3 * EPS23 + 2.0 ** -24 * (S - ml[:, 0:1]).abs()
    ds_tol = bw["p"] * sum_tol(2 * c.E + 4, bw["dP_ab"] + up(c.delta).abs()[:, None]) + p_rel * bw["dS"].abs()
    k_rel = (c.N + nparts + 8) * EPS23 + PSPLIT
    out = {"dS": ds_tol, "dSx": ds_tol @ up(c.x).abs() + k_rel * bw["dSx_ab"]}
    if c.entry.pos:
        out["marg"] = tuple(t + k_rel * ab for t, ab in zip(R.axis_marginals(ds_tol, c.H, c.W), bw["marg_ab"]))
    return out
