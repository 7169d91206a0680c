"""Inputs, dispatch predicates (restated) and derived error bounds for the kernels of csrc/merge.hip / csrc/merge_item.hpp: the merge of
streaming partials with the value-side positional term (hicom_global_merge_fwd, hicom_global_merge_marg_fwd), the cross-shard combine
(hicom_global_combine_fwd / _strided_fwd) and merge + v_proj (hicom_merge_vproj_fwd / _fixed_fwd / _sets_fwd).  Shared by
tests/test_gpu_merge.py (the kernels against tests/ops_reference.py: merge_ref, combine_ref, merge_vproj_ref) and
tests/test_merge_power.py (CPU: what a wrong kernel would do to the references, against the same bounds).

The partials are SYNTHETIC and made consistent with the logits, not taken from a stream kernel:
  logits      fp32 [rows_pad, stride], random, every (row, frame) with a level shift of its own (sigma 3: the frame maxima differ), spikes
              of 6 .. 8 on the first and the last token and, at T > 64, on both sides of the frame boundary 63 | 64.
  chunks      the stream kernels' rule (global_stream_inputs.chunk_tiles): chunk i of nparts covers the 16-token tiles
              [ntiles i // nparts, ntiles (i + 1) // nparts).  part_m = the chunk's maximum (exact in fp32), part_l = sum e^(s - m) in
              float64 rounded to fp32.  A chunk without tiles (nparts > ntiles) carries a state of its own: m up to 60 below the row's
              largest logit, l in [0.5, 1.5) -- weights that underflow beside weights of exactly 1.  Every frame maximum is <= M = max_p m_p
              (the kernel derives M from part_m alone); the builder asserts it.
  part_acc    l_p times a random fp32 row; every row r = 1 mod 4 carries +-30 entries of alternating sign over the partials (cancellation).
  pe          ~ N(0, 1), as large as the contexts; the t / y / x blocks start at t0, t0 + T + 2 and t0 + T + H + 5 of a taller table, the
              rows between and behind them are NaN (rows in front of t0 are finite: another shard's frames).
  padding     rows >= R of part_m / part_l / part_acc / part_marg and of the logits, and the logits' columns >= N, are NaN.
  part_marg   (marginal form) float64 sums of e^(s - m_i) over the chunk's tokens per frame / grid row / grid column, rounded to fp32, in
              the layout [8 frames from the chunk's first | pad to 16 | H | pad to 16 | W | pad to 16]; the pad columns are NaN.
  no pe       part_m = -60 U(0, 1) with two partials per row at exactly 0 and the last partial within 1 of the maximum.

Which kernels run (restated from the host code of csrc/merge.hip, never imported; tests/test_gpu_merge.py cannot see the choice directly,
so every case names the form it is built for and form_of() must agree -- a moved threshold fails the named case):
  marginals   wave   H <= 32 and W <= 32: frame_marginals_wave_kernel
              regs   otherwise, H W <= 1024: frame_marginals_kernel with the logits in registers;   reread: H W > 1024
              margw  the marginal form: merge_marg_weights_kernel
  merge       mode0      no pe: merge_ctx_kernel<0>, no positional term
              mode0_pos  pe, and the weight record nparts + T + H + W + 2 does not fit min(64, T) (H + W + 2): one kernel does it all
              mode1 + mode2 / apply8   otherwise: weights once per row, then the apply step: merge_ctx_apply_kernel<8> where
                         rows >= 64, nparts <= 32 and 8 (1024 + record) floats fit 64 KB of LDS, else merge_ctx_kernel<2>
  passes      ceil(T / 64) staging passes of the frame marginals (mode0_pos and mode1)

  case                       (T, H, W)      R / pad  nparts        E     t0  form  [marginal entry]
  nopos_p{1 .. 500}           -             9 / 16   1 31 32 33 224 225 256 257 300 500   1152   -  mode0 (8-deep batch from 225, tail, > 256;
                                                                            500: the 8-deep loop behind the prefetched batch)
  nopos_p33_e{768,100,36}     -             9 / 16   33          768 100 36  -  mode0; the c4 < E and c < E masks
  wave_3x27x27_p7            (3, 27, 27)    9 / 16   7           1152    0  wave mode1 mode2  [margw mode2]
  wave_2x32x32_p5            (2, 32, 32)    9 / 16   5           1152    0  wave mode1 mode2 (the full 32 x 32 wave)  [margw mode2]
  wave_4x7x5_p3              (4, 7, 5)      9 / 16   3           1152    5  wave mode1 mode2  [margw mode2]
  wave_1x5x3_p9              (1, 5, 3)      9 / 16   9           1152    0  wave mode0_pos (9 + 1 + 8 + 2 > 10)
  regs_2x33x4_p3             (2, 33, 4)     9 / 16   3           1152    5  regs mode1 mode2  [margw mode2: H in three blocks of 16]
  regs_2x4x40_p3             (2, 4, 40)     9 / 16   3           1152    0  regs mode1 mode2  [margw mode2: W in three blocks]
  reread_2x33x32_p3          (2, 33, 32)    9 / 16   3           1152    5  reread (H W = 1056) mode1 mode2  [margw mode2]
  stage_65x3x2_p4            (65, 3, 2)     9 / 16   4           1152    5  wave mode1 mode2, 2 passes (64 + 1 frames)
  stage_130x3x2_p4           (130, 3, 2)    9 / 16   4           1152    0  wave mode1 mode2, 3 passes (64 + 64 + 2); 135 positional rows
  stage_65x1x1_p200          (65, 1, 1)     9 / 16   200         1152    5  wave mode0_pos (200 + 65 + 4 > 256), 2 passes
  pos132_100x16x16_r9_p4     (100, 16, 16)  9 / 16   4           1152    5  wave mode1 mode2, 132 positional rows: the second j0 batch
  pos132_100x16x16_r9_p16    (100, 16, 16)  9 / 16   16          1152    0  the same  [margw mode2]
  a8_{4x7x5,100x16x16}_r{64,69}_p{1,16,17,32}_e{1152,100}   all 32;  64 / 64, 69 / 96;  t0 = 5 where R + nparts is odd
                                                                            wave mode1 apply8; 100x16x16: the j >= 128 tail  [margw apply8]
  m2_4x7x5_r63_p16           (4, 7, 5)      63 / 64  16          1152    5  wave mode1 mode2: rows = 63  [margw mode2]
  m2_4x7x5_r64_p33           (4, 7, 5)      64 / 64  33          1152    0  wave mode1 mode2: nparts = 33  [margw mode2, the third i0 trip]
  m2_1000x15x1_r64_p8        (1000, 15, 1)  64 / 64  8           1152    5  wave mode1 mode2: 8 (1024 + 1026) floats exceed 64 KB of LDS
  m0_1000x1x1_r64_p16        (1000, 1, 1)   64 / 64  16          1152    0  wave mode0_pos, 16 passes.  (At H = W = 1 a record fits the
                                                                            scratch only up to T = 250, where it is far below the LDS limit:
                                                                            this shape cannot reach mode2 through the logit form, and the
                                                                            marginal form cannot hold it -- a 16-token tile spans 16 frames.)
  marg_4x7x5_r{9,69}_p{1,2,15,16,17}  (4, 7, 5)  wave mode1 mode2 / apply8  [margw mode2 / apply8]

The marginal entry runs on EVERY positional case whose shape the part_marg layout can hold (marg_layout_ok; asserted below for the whole
table).  It cannot hold: wave_1x5x3_p9 (T = 1: no room for the record), the stage_* cases, m2_1000x15x1 and m0_1000x1x1 (H W < 16: one
tile spans more than 8 frames), pos132_100x16x16_r9_p4 (a chunk of 25 frames) and a8_100x16x16_*_p1_* (one chunk of 100 frames).

Branches of csrc/merge.hip that stay unreached, and why:
  ay[1..3] of merge_ctx_kernel (H + W > 256) -- the staging tile of 64 (H + W + 2) floats must fit smem2 <= 60000 bytes, which refuses
      H + W above 212 (at one partial); hicom_global_merge_marg_fwd caps H, W at 64.  The refusal is tested instead ((1, 110, 110)).
  The `H + W <= 1024` half of the E % 4 requirement -- shadowed by the same smem2 cap.
  merge_vproj_fixed_kernel<32, *> is never instantiated; the part_marg / vpe16 role of merge_item.hpp runs only inside the readout
      launch (tests/test_gpu_ops.py).

Bounds (merge_bounds, combine_bounds, vproj_bounds): term by term from the kernels' operations and the references' own magnitudes; see
their docstrings.  None is tuned to a measured error.
"""
import functools
from types import SimpleNamespace
from typing import NamedTuple

import torch

import ops_reference as R
from global_stream_inputs import TRANS, chunk_first_frames, chunk_token_ranges, ntiles_of, rows_pad_of
from ops_reference import EPS23, up

NAN = float("nan")
FIX = 2.0 ** -37            # half a unit of the 2^-36 fixed-point accumulators: one rintf per integer add (merge_item.hpp)


class Case(NamedTuple):
    id: str
    grid: tuple             # (T, H, W) or None: no positional term
    R: int
    nparts: int
    form: str               # what the host code must choose (module docstring)
    E: int = 1152
    t0: int = 0
    normalize: tuple = (0, 1)
    marg: str = ""          # the form of the marginal entry, where the case also runs through hicom_global_merge_marg_fwd


def _cases():
    M2, A8 = "margw mode2", "margw apply8"
    out = []
    for n in (1, 31, 32, 33, 224, 225, 256, 257, 300, 500):
        out.append(Case(f"nopos_p{n}", None, 9, n, "mode0"))
    for E in (768, 100, 36):
        out.append(Case(f"nopos_p33_e{E}", None, 9, 33, "mode0", E))
    out += [
        Case("wave_3x27x27_p7", (3, 27, 27), 9, 7, "wave mode1 mode2", marg=M2),
        Case("wave_2x32x32_p5", (2, 32, 32), 9, 5, "wave mode1 mode2", marg=M2),
        Case("wave_4x7x5_p3", (4, 7, 5), 9, 3, "wave mode1 mode2", t0=5, marg=M2),
        Case("wave_1x5x3_p9", (1, 5, 3), 9, 9, "wave mode0_pos"),
        Case("regs_2x33x4_p3", (2, 33, 4), 9, 3, "regs mode1 mode2", t0=5, marg=M2),
        Case("regs_2x4x40_p3", (2, 4, 40), 9, 3, "regs mode1 mode2", marg=M2),
        Case("reread_2x33x32_p3", (2, 33, 32), 9, 3, "reread mode1 mode2", t0=5, marg=M2),
        Case("stage_65x3x2_p4", (65, 3, 2), 9, 4, "wave mode1 mode2", t0=5),
        Case("stage_130x3x2_p4", (130, 3, 2), 9, 4, "wave mode1 mode2"),
        Case("stage_65x1x1_p200", (65, 1, 1), 9, 200, "wave mode0_pos", t0=5),
        Case("pos132_100x16x16_r9_p4", (100, 16, 16), 9, 4, "wave mode1 mode2", t0=5),
        Case("pos132_100x16x16_r9_p16", (100, 16, 16), 9, 16, "wave mode1 mode2", marg=M2),
    ]
    # the 8-row apply: every (grid, R, nparts, E) of the issue's list
    for grid in ((4, 7, 5), (100, 16, 16)):
        for r in (64, 69):
            for n in (1, 16, 17, 32):
                for E in (1152, 100):
                    marg = "" if (grid[0] == 100 and n == 1) else A8                  # (one chunk of 100 frames: no 8-frame block holds it)
                    out.append(Case(f"a8_{grid[0]}x{grid[1]}x{grid[2]}_r{r}_p{n}_e{E}", grid, r, n, "wave mode1 apply8", E, 5 if (r + n) % 2 else 0,
                                    (0, 1), marg))
    out += [
        Case("m2_4x7x5_r63_p16", (4, 7, 5), 63, 16, "wave mode1 mode2", t0=5, marg=M2),
        Case("m2_4x7x5_r64_p33", (4, 7, 5), 64, 33, "wave mode1 mode2", marg=M2),
        Case("m2_1000x15x1_r64_p8", (1000, 15, 1), 64, 8, "wave mode1 mode2", t0=5),
        Case("m0_1000x1x1_r64_p16", (1000, 1, 1), 64, 16, "wave mode0_pos"),
    ]
    for r in (9, 69):
        for n in (1, 2, 15, 16, 17):
            if r == 69 and n in (1, 16, 17):
                continue                                # (a8_4x7x5_r69_p{1,16,17}_e1152 above)
            out.append(Case(f"marg_4x7x5_r{r}_p{n}", (4, 7, 5), r, n, "wave mode1 " + ("apply8" if r == 69 else "mode2"), 1152, 5 if n % 2 else 0,
                            (0, 1), A8 if r == 69 else M2))
    return tuple(out)


CASES = _cases()
BY_ID = {e.id: e for e in CASES}
assert len(BY_ID) == len(CASES)
kTC = 64


# ---- the host code's choices, restated --------------------------------------------------------------------------------------------
def apply_form(T, H, W, rows, nparts):
    rec = 2 + nparts + T + H + W
    return "apply8" if (8 * 16 * 64 + 8 * rec) * 4 <= 64 * 1024 and rows >= 64 and nparts <= 32 else "mode2"


def two_kernel(T, H, W, nparts):
    return nparts + T + H + W + 2 <= min(kTC, T) * (H + W + 2)


def smem2_bytes(T, H, W, nparts, pos=True):
    return (nparts + ((2 * T + H + W + kTC * (H + W + 2)) if pos else 0) + 16 * 64 + 4) * 4


def refusal(T, H, W, nparts, E, pos=True):
    """The reason hicom_global_merge_fwd refuses the shape, in the order it checks, or None."""
    if pos and (H * W + H + 4) * 4 > 60000:
        return "too large for the marginal kernel"
    if E % 4 or (pos and H + W > 1024):
        return "global_merge: E"
    if smem2_bytes(T, H, W, nparts, pos) > 60000:
        return "too many partials/frames for one pass"
    return None


def form_of(e):
    if e.grid is None:
        return "mode0"
    T, H, W = e.grid
    assert refusal(T, H, W, e.nparts, e.E) is None
    mk = "wave" if H <= 32 and W <= 32 else ("regs" if H * W <= 1024 else "reread")
    return f"{mk} mode1 {apply_form(T, H, W, e.R, e.nparts)}" if two_kernel(T, H, W, e.nparts) else f"{mk} mode0_pos"


def marg_form_of(e):
    T, H, W = e.grid
    return "margw " + apply_form(T, H, W, e.R, e.nparts)


def marg_width(H, W):
    return 16 * (1 + (H + 15) // 16 + (W + 15) // 16)


def marg_layout_ok(N, H, W, nparts):
    """What the part_marg layout and hicom_global_merge_marg_fwd need: H, W <= 64, whole frames, a chunk within 8 frames of its first,
    and room for the weight record at the head of the row's scratch region."""
    if N % (H * W) or H > 64 or W > 64:
        return False
    T = N // (H * W)
    tiles_per_part = (ntiles_of(N) + nparts - 1) // nparts + 1
    return (tiles_per_part * 16 + H * W - 1) // (H * W) + 1 <= 8 and 2 + nparts + T + H + W <= T * (H + W + 2)


for _e in CASES:            # the marginal entry runs wherever its layout can hold the case, and nowhere else
    if _e.grid is not None:
        assert bool(_e.marg) == marg_layout_ok(_e.grid[0] * _e.grid[1] * _e.grid[2], _e.grid[1], _e.grid[2], _e.nparts), _e.id


# ---- the merge family -------------------------------------------------------------------------------------------------------------
def _gen(id):
    return torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(id)))


def spread_m(g, nparts, rows):
    """part_m without logits: -60 U(0, 1); per row two partials at exactly 0 (weight 1) and the last partial within 1 of the maximum."""
    m = -60.0 * torch.rand(nparts, rows, generator=g)
    for r in range(rows):
        for k in torch.randint(0, nparts, (2,), generator=g).tolist():
            m[k, r] = 0.0
    m[nparts - 1] = -torch.rand(rows, generator=g)
    m[torch.randint(0, nparts, (1,), generator=g).item(), 0] = 0.0
    return m


def value_rows(g, nparts, rows, E):
    v = torch.randn(nparts, rows, E, generator=g)
    sign = (1.0 - 2.0 * (torch.arange(nparts) % 2))[:, None, None]
    big = torch.arange(rows) % 4 == 1
    v[:, big] += 30.0 * sign * (1.0 + torch.rand(nparts, int(big.sum()), E, generator=g))
    return v


@functools.lru_cache(maxsize=None)
def build(id):
    """The tensors of merge case `id` as the kernels receive them (CPU; callers must not write into them)."""
    e = BY_ID[id]
    g = _gen(id)
    R_, E, nparts = e.R, e.E, e.nparts
    rows_pad = rows_pad_of(R_)
    c = SimpleNamespace(entry=e, R=R_, rows_pad=rows_pad, E=E, nparts=nparts, pos=e.grid is not None, T=0, H=1, W=1, N=0, t0=0, y0=0, x0=0,
                        scores=None, pe=None, pmarg=None)
    pm, pl = torch.full((nparts, rows_pad), NAN), torch.full((nparts, rows_pad), NAN)
    pacc = torch.full((nparts, rows_pad, E), NAN)
    if not c.pos:
        pm[:, :R_] = spread_m(g, nparts, R_)
        pl[:, :R_] = 0.5 + torch.rand(nparts, R_, generator=g)
    else:
        T, H, W = e.grid
        N, HW = T * H * W, H * W
        c.T, c.H, c.W, c.N, c.t0 = T, H, W, N, e.t0
        c.y0, c.x0 = e.t0 + T + 2, e.t0 + T + 2 + H + 3
        c.P, c.stride = c.x0 + W + 2, ntiles_of(N) * 16 + 16
        s = torch.randn(R_, N, generator=g) + (3.0 * torch.randn(R_, T, generator=g)).repeat_interleave(HW, 1)
        c.toks = sorted({0, N - 1} | ({64 * HW - 1, 64 * HW} if T > 64 else set()))
        for n in c.toks:
            s[:, n] += 6.0 + 2.0 * torch.rand(R_, generator=g)
        c.scores = torch.full((rows_pad, c.stride), NAN)
        c.scores[:R_, :N] = s
        sd = s.double()
        top = s.max(1).values
        c.ranges = chunk_token_ranges(N, nparts)
        for i, (lo, hi) in enumerate(c.ranges):
            if hi > lo:
                pm[i, :R_] = s[:, lo:hi].max(1).values
                pl[i, :R_] = torch.exp(sd[:, lo:hi] - pm[i, :R_, None].double()).sum(1).float()
            else:
                pm[i, :R_] = top - 60.0 * torch.rand(R_, generator=g)
                pl[i, :R_] = 0.5 + torch.rand(R_, generator=g)
        # the kernel takes M from part_m alone: every frame's maximum must be below it
        assert bool((s.reshape(R_, T, HW).max(2).values <= pm[:, :R_].max(0).values[:, None]).all())
        c.pe = torch.randn(c.P, E, generator=g)
        c.pe[e.t0 + T:c.y0] = NAN
        c.pe[c.y0 + H:c.x0] = NAN
        c.pe[c.x0 + W:] = NAN
        if e.marg:
            assert marg_layout_ok(N, H, W, nparts), id
            MS, ybase, xbase = marg_width(H, W), 16, 16 + 16 * ((H + 15) // 16)
            c.pmarg = torch.full((nparts, rows_pad, MS), NAN)
            t, y, x = R.token_axes(N, H, W)
            for i, ((lo, hi), ff) in enumerate(zip(c.ranges, chunk_first_frames(N, HW, nparts))):
                blk = torch.zeros(R_, MS, dtype=torch.float64)
                if hi > lo:
                    w = torch.exp(sd[:, lo:hi] - pm[i, :R_, None].double())
                    assert int(t[lo]) >= ff and int(t[hi - 1]) < ff + 8
                    blk.index_add_(1, t[lo:hi] - ff, w)
                    blk.index_add_(1, ybase + y[lo:hi], w)
                    blk.index_add_(1, xbase + x[lo:hi], w)
                c.pmarg[i, :R_] = blk.float()
            c.pmarg[:, :, 8:16] = NAN
            c.pmarg[:, :, ybase + H:xbase] = NAN
            c.pmarg[:, :, xbase + W:] = NAN
    pacc[:, :R_] = pl[:, :R_, None] * value_rows(g, nparts, R_, E)
    c.pm, c.pl, c.pacc = pm, pl, pacc
    return c


def ref_args(c):
    a = dict(part_m=up(c.pm), part_l=up(c.pl), part_acc=up(c.pacc), rows=c.R)
    if c.pos:
        a.update(scores=up(c.scores), N=c.N, H=c.H, W=c.W, pe=up(c.pe), t0i=c.t0, y0i=c.y0, x0i=c.x0)
    return a


@functools.lru_cache(maxsize=None)
def merge_reference(id, normalize):
    """{M, L, acc, acc_nope (the same without the positional term), ab (absolute terms, un-normalised)} of case `id`."""
    c = build(id)
    a = ref_args(c)
    M, L, acc = R.merge_ref(**a, normalize=bool(normalize))
    o = {"M": M, "L": L, "acc": acc, "ab": R.merge_ref(**a, absolute=True)[2]}
    if c.pos:
        o["acc_nope"] = R.merge_ref(**{**a, "scores": None, "pe": None}, normalize=bool(normalize))[2]
    return o


def weight_terms(pm, pl, rows):
    """(w, rel, L, relL): the partial weights e^(m_p - M), the relative error of each on the device -- one expf (TRANS) and the
    rounding of its argument, 2^-23 |m_p - M| (arguments below -104 give 0 either way) -- L, and the relative error of L: the weights'
    errors and an nparts-term fp32 sum."""
    m, l = up(pm)[:, :rows], up(pl)[:, :rows]
    d = m.max(0).values[None] - m
    w = torch.exp(-d)
    rel = TRANS + EPS23 * d.clamp(0.0, 104.0)
    L = (w * l).sum(0)
    return w, rel, L, (m.shape[0] + 8) * EPS23 + (w * l * rel).sum(0) / L


def merge_bounds(c, ref, normalize):
    """{"logL": [R], "acc": [R, E]}.
      acc   sum_p w_p acc_p + sum_j wpos_j pe_j, one fmaf per partial and per positional row and the reduction over the 16 / 32 column
            groups, any order: (nparts + T + H + W + 8) 2^-23 sum |terms| (the reference's own absolute sum).
            A partial weight: weight_terms.  A positional weight is a sum of e^(s_n - fmax_t) e^(fmax_t - M) over tokens: two expf
            (2 TRANS), their argument roundings 2^-23 (M - s_n) <= 2^-23 D_r (D_r the row's largest M - s_n, capped at 104), and the
            longest chain of additions any of the kernels runs for one weight: a y (x) weight sums the W (H) tokens of a grid row
            (column) and is folded over the T frames by fmaf; a t weight sums a frame as W then H terms (block kernel; the wave kernel:
            <= 16 per lane, then a tree) and takes one product: at most (H + W + T + 4) 2^-23, the 4 for the product, the cross-half
            add and the tree's last levels.  The marginal entry sums nparts chunks instead, two threads per weight: ceil(nparts / 2) + 1
            additions and the fp32 rounding of part_marg; the table keeps that within H + W + T + 4 (asserted), so both entries meet
            ONE bound.  All relative to sum_n e^(s_n - M) |pe rows of n|.
            normalize: divided by L, + the relative error of L and the division's rounding.
      logL  the relative error of L + the rounding of L to fp32 and of the comparison's own log.
    M is compared exactly."""
    w, rel, L, relL = weight_terms(c.pm, c.pl, c.R)
    npos = (c.T + c.H + c.W) if c.pos else 0
    ab_part = (w[:, :, None] * up(c.pacc)[:, :c.R].abs()).sum(0)
    tol = ((w * rel)[:, :, None] * up(c.pacc)[:, :c.R].abs()).sum(0) + R.sum_tol(c.nparts + npos + 8, ref["ab"])
    if c.pos:
        assert not c.entry.marg or (c.nparts + 1) // 2 + 2 <= c.H + c.W + c.T + 4
        D = (ref["M"][:, None] - up(c.scores)[:c.R, :c.N]).clamp(0.0, 104.0).max(1).values
        tol = tol + (2 * TRANS + EPS23 * D + (c.H + c.W + c.T + 4) * EPS23)[:, None] * (ref["ab"] - ab_part).clamp_min(0.0)
    if normalize:
        tol = tol / L[:, None] + ref["acc"].abs() * (relL + EPS23)[:, None]
    return {"logL": relL + 2 * EPS23, "acc": tol}


MERGE_FAULTS = ("lose_last_partial", "lose_partial_batch", "frame_max_unscaled", "lose_frames_from_64", "lose_pos_from_128", "ignore_t0",
                "swap_yx", "neighbour_record", "pad_leak", "unnormalised_L")


def fault_applies(e, name, normalize):
    T, H, W = e.grid or (0, 1, 1)
    pos = e.grid is not None
    return {"lose_last_partial": True, "lose_partial_batch": e.nparts >= 225, "frame_max_unscaled": pos and T > 1,
            "lose_frames_from_64": pos and T > 64, "lose_pos_from_128": pos and T + H + W > 128, "ignore_t0": pos and e.t0 != 0,
            "swap_yx": pos and H != W, "neighbour_record": e.R > 1 and (e.nparts > 1 or pos or bool(normalize)), "pad_leak": e.R < rows_pad_of(e.R),
            "unnormalised_L": bool(normalize) and e.nparts > 1}[name]


# ---- combine ----------------------------------------------------------------------------------------------------------------------
COMBINE_FAMILIES = ("equal", "low", "spread")
COMBINE_SHAPES = tuple((n, r, E) for n in (1, 2, 8) for r in (1, 9) for E in (100, 256, 260, 1152))


@functools.lru_cache(maxsize=None)
def build_combine(family, nsets, rows, E):
    """ml [nsets, rows, 2], acc [nsets, rows, E] (un-normalised: L times a random row, cancellation as in the merge family) and the
    packed strided buffer [nsets, stride] = [(M, L) pairs | acc | gap of NaN].  equal: every set at the same M; low: set 1 (set 0 of one)
    100 below the others -- its weight e^-100 is 0 in fp32; spread: M ~ 3 N(0, 1)."""
    g = _gen(f"combine_{family}_{nsets}_{rows}_{E}")
    M = 3.0 * torch.randn(nsets, rows, generator=g)
    if family == "equal":
        M = M[:1].expand(nsets, rows).clone()
    elif family == "low":
        M = M[:1].expand(nsets, rows).clone() + 0.25 * torch.randn(nsets, rows, generator=g)
        M[min(1, nsets - 1)] -= 100.0
    L = 0.5 + 40.0 * torch.rand(nsets, rows, generator=g)
    acc = (L[:, :, None] * value_rows(g, nsets, rows, E)).contiguous()
    ml = torch.stack([M, L], 2).contiguous()
    stride = 2 * rows + rows * E + 7
    packed = torch.full((nsets, stride), NAN)
    packed[:, :2 * rows] = ml.reshape(nsets, -1)
    packed[:, 2 * rows:2 * rows + rows * E] = acc.reshape(nsets, -1)
    return SimpleNamespace(ml=ml, acc=acc, packed=packed, stride=stride, nsets=nsets, rows=rows, E=E)


def combine_bounds(c, ctx):
    """fmaf chains of nsets terms for the numerator and for L, weights as in weight_terms, one division."""
    w, rel, L, relL = weight_terms(c.ml[:, :, 0], c.ml[:, :, 1], c.rows)
    a = up(c.acc).abs()
    return (((w * rel)[:, :, None] * a).sum(0) + R.sum_tol(c.nsets + 2, (w[:, :, None] * a).sum(0))) / L[:, None] + ctx.abs() * (relL + EPS23)[:, None]


# ---- merge + v_proj ---------------------------------------------------------------------------------------------------------------
VPROJ_SHAPES = ((1152, 9), (768, 6), (768, 12), (64, 1))          # head dims 128, 128, 64, 64
VPROJ_NPARTS = (1, 7, 255, 256)
VPROJ_FAULTS = ("head_off_by_one", "lose_last_slab")


@functools.lru_cache(maxsize=None)
def build_vproj(E, rows, nparts):
    """part_m (spread 60) / part_l / part_acc f32 [nparts, 16(, E)] with NaN rows >= rows; p16 = acc / l as f16 (the hot path's
    normalised contexts); w_v bf16 [E, E]; sets: the same states packed as [(M, L) pairs | acc | NaN gap] per partial, rows_pad = rows."""
    g = _gen(f"vproj_{E}_{rows}_{nparts}")
    pm, pl, pacc = torch.full((nparts, 16), NAN), torch.full((nparts, 16), NAN), torch.full((nparts, 16, E), NAN)
    pm[:, :rows] = spread_m(g, nparts, rows)
    pl[:, :rows] = 0.5 + torch.rand(nparts, rows, generator=g)
    vals = value_rows(g, nparts, rows, E)
    pacc[:, :rows] = pl[:, :rows, None] * vals
    p16 = torch.full((nparts, 16, E), NAN, dtype=torch.float16)
    p16[:, :rows] = (pacc[:, :rows] / pl[:, :rows, None]).half()
    wv = (0.05 * torch.randn(E, E, generator=g)).bfloat16()
    stride = 2 * rows + rows * E + 6
    sets = torch.full((nparts, stride), NAN)
    sets[:, 0:2 * rows:2], sets[:, 1:2 * rows:2] = pm[:, :rows], pl[:, :rows]
    sets[:, 2 * rows:2 * rows + rows * E] = pacc[:, :rows].reshape(nparts, -1)
    return SimpleNamespace(E=E, rows=rows, nparts=nparts, pm=pm, pl=pl, pacc=pacc, p16=p16, wv=wv, sets=sets)


@functools.lru_cache(maxsize=None)
def vproj_reference(E, rows, nparts, f16):
    c = build_vproj(E, rows, nparts)
    return R.merge_vproj_ref(up(c.pm), up(c.pl), up(c.p16 if f16 else c.pacc), rows, up(c.wv), normalised=f16)


def vproj_bounds(c, ref, f16, fixed):
    """{"logL", "ctx", "o"}.  ctx: as the normalised merge without a positional term (the f16 form weighs with w_p l_p: one more rounding
    per weight; the f16 quantisation itself is in the inputs).  o = W_v,h ctx_h: the ctx bound through |W_v|, + a chain of 32 fmaf and
    one lane exchange per 64-column slab and the E / 64 slab sums: (34 + E / 64) 2^-23 sum |W_v| |ctx|.  fixed: + 2^-37 for each of the
    E / 64 integer adds into one accumulator (one rintf(dot 2^36) per slab and output; every partial of a slab is merged in front of
    the conversion, so there is one partial group)."""
    M, L, ctx, o = ref
    w, rel, _, relL = weight_terms(c.pm, c.pl, c.rows)
    vals = up(c.p16 if f16 else c.pacc)[:, :c.rows].abs()
    wa = w * up(c.pl)[:, :c.rows] if f16 else w
    rel = rel + EPS23 if f16 else rel
    ctx_tol = (((wa * rel)[:, :, None] * vals).sum(0) + R.sum_tol(c.nparts + 8, (wa[:, :, None] * vals).sum(0))) / L[:, None]
    ctx_tol = ctx_tol + ctx.abs() * (relL + EPS23)[:, None]
    hd = c.E // c.rows
    wabs = up(c.wv).abs().reshape(c.rows, hd, c.E)
    o_tol = torch.einsum("hjc,hc->hj", wabs, ctx_tol).reshape(c.E) + R.sum_tol(34 + c.E // 64, torch.einsum("hjc,hc->hj", wabs, ctx.abs()).reshape(c.E))
    if fixed:
        o_tol = o_tol + (c.E // 64) * FIX
    return {"logL": relL + 2 * EPS23, "ctx": ctx_tol, "o": o_tol}
