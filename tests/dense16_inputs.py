"""Inputs, float64 references and error bounds for the dense 16-bit GEMM kernels of csrc/dense16.hip: dense16_gemm_kernel (NT form,
the general and the row-contiguous epilogue, the positional-table term `row_tab`) and dense16_tn_kernel (weight gradients).  Shared by
tests/test_gpu_dense16.py (the kernels against the references) and tests/test_dense16_power.py (CPU: what a wrong kernel would do to
the references, against the same bounds).

NT cases.  M = T H W rows walk the token grid; the table term of row m is tab[t0 + t] + tab[y0 + y] + tab[x0 + x].
  table     ~ 0.5 N(0, 1) per entry (a wrong table row moves a value by about 0.5 against bounds of about 1e-5), f32 [P, tab_ld]; the
            columns >= N of a table wider than N hold finite garbage of another magnitude
  bias      ~ 0.1 N(0, 1) in bf16 with |b[N - 1]| >= 0.05 (what a padded column of the last slice would add to ssq)
  operands  a ~ 0.5 N(0, 1), w ~ 0.05 N(0, 1) in the case's 16-bit type, as tests/test_gpu_head.py::test_dense16_gemm_matches_torch;
            lda = K + 64 and the pad columns are NaN
  residual  ~ N(0, 1) in bf16; dot vector ~ N(0, 1) in f32

  id               M     N     K    type  tab_ld  (t0, y0, x0)  P   what it reaches
  rows_4x7x5       140   136   128  bf16  144     (3, 11, 20)   32  row epilogue; H W = 35: the frame boundaries 35 / 70 / 105 fall inside
                                                                    16-row MFMA blocks, y changes every 5 rows; two row tiles (128 + 12: the
                                                                    row clamp); the last 64-slice holds 8 columns; table wider than N
  general_4x7x5    140   132   128  fp16  132     (3, 11, 20)   32  the same with N % 8 == 4: general epilogue
  wide_3x9x11      297   1152  64   fp16  1152    (0, 0, 0)     12  18 slices, 9 column tiles, three row tiles with a ragged last one, 27
                                                                    workgroups through the XCD remap
  tall_2x27x19     1026  72    64   bf16  80      (1, 4, 32)    52  nine row tiles: the second super-tile block (RM = 8) holds one row tile
  one_frame_1x6x6  36    64    64   fp16  64      (0, 2, 5)     12  T = 1, one partly filled tile

TN cases (Kt, M, N, lda, ldb, type, splits): the operands sit in allocations with extra rows (up to the next multiple of 64 and 8
more) and, where the pitch exceeds the width, extra columns, all NaN; the kernel gets the [:Kt] row view with its pitch.
  (1, 8, 8, 8, 8, bf16, 1)            one token row: the `kk = Kt - 1` clamp and 63 zeroed rows
  (40, 136, 72, 144, 80, fp16, 1)     Kt < 64, pitched, fp16 at a ragged Kt, two row tiles of the product
  (200, 136, 264, 136, 264, bf16, 3)  4 stages, 2 per split: the third split is empty (its partial must be exact zeros)
  (700, 264, 136, 272, 144, fp16, 8)  the multiple-of-8 block mapping with 6 tiles, 11 stages (ragged last one), splits 6 and 7 empty
  (1090, 136, 136, 136, 136, bf16, 16) 18 stages, 2 per split, ragged last stage: splits 9 .. 15 empty

Bounds (nt_bounds; the project's own from tests/test_gpu_head.py, and per-element bounds of the slice sums derived from them):
  y (f32)    d = 2e-5 max(1, max |pre|)
  val (fp16) 2^-11 max(1, max |pre|) + 1e-6          pre (fp16)  2^-10 max(1, max |pre|)
  ssq[s, m]  every pre of the slice is off by at most d: |(p + e)^2 - p^2| <= 2 d |p| + d^2 (second order, dropped), and the
             64 fused multiply-adds and 3 shuffle additions of the slice in fp32: 2 d sum |pre| + 64 2^-23 sum pre^2
  rdot[s, m] d sum |vec| + 64 2^-23 sum |vec y|  likewise
  TN         the formula of test_dense16_tn_matches_torch: 8e-6 sqrt(Kt) + 1e-5 max |want|
"""
import functools
from types import SimpleNamespace
from typing import NamedTuple

import torch

import ops_reference as R
from ops_reference import EPS23, up

NAN = float("nan")
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


class NT(NamedTuple):
    id: str
    grid: tuple             # (T, H, W)
    N: int
    K: int
    dtype: str
    tab_ld: int
    offs: tuple             # (t0, y0, x0)
    P: int                  # table rows


NT_CASES = (
    NT("rows_4x7x5", (4, 7, 5), 136, 128, "bf16", 144, (3, 11, 20), 32),
    NT("general_4x7x5", (4, 7, 5), 132, 128, "f16", 132, (3, 11, 20), 32),
    NT("wide_3x9x11", (3, 9, 11), 1152, 64, "f16", 1152, (0, 0, 0), 12),
    NT("tall_2x27x19", (2, 27, 19), 72, 64, "bf16", 80, (1, 4, 32), 52),
    NT("one_frame_1x6x6", (1, 6, 6), 64, 64, "f16", 64, (0, 2, 5), 12),
)
NT_BY_ID = {e.id: e for e in NT_CASES}
assert len(NT_BY_ID) == len(NT_CASES)


class TN(NamedTuple):
    Kt: int
    M: int
    N: int
    lda: int
    ldb: int
    dtype: str
    splits: int

    @property
    def id(self):
        return f"tn_{self.Kt}x{self.M}x{self.N}_{self.dtype}_s{self.splits}"


TN_CASES = (
    TN(1, 8, 8, 8, 8, "bf16", 1),
    TN(40, 136, 72, 144, 80, "f16", 1),
    TN(200, 136, 264, 136, 264, "bf16", 3),
    TN(700, 264, 136, 272, 144, "f16", 8),
    TN(1090, 136, 136, 136, 136, "bf16", 16),
)
TN_BY_ID = {e.id: e for e in TN_CASES}


def _seed(id):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(id))


# ---- NT ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def build(id):
    """The tensors of NT case `id` as the kernel receives them (CPU; callers must not write into them)."""
    e = NT_BY_ID[id]
    T, H, W = e.grid
    M, N, K, dt = T * H * W, e.N, e.K, DTYPES[e.dtype]
    g = torch.Generator().manual_seed(_seed(id))
    rnd = lambda *s: torch.randn(*s, generator=g)
    c = SimpleNamespace(entry=e, T=T, H=H, W=W, M=M, N=N, K=K, geom=(H, W) + e.offs, slices=(N + 63) // 64, npad=(N + 127) // 128 * 128)
    a = torch.full((M, K + 64), NAN)
    a[:, :K] = rnd(M, K) * 0.5
    c.a = a.to(dt)
    c.w = (rnd(N, K) * 0.05).to(dt)
    b = rnd(N) * 0.1
    if abs(float(b[N - 1])) < 0.05:
        b[N - 1] = 0.0625 if float(b[N - 1]) >= 0 else -0.0625
    c.b = b.bfloat16()
    c.tab = 3.0 + 2.0 * rnd(e.P, e.tab_ld)
    c.tab[:, :N] = 0.5 * rnd(e.P, N)
    c.res = rnd(M, N).bfloat16()
    c.vec = rnd(N).contiguous()
    assert abs(float(c.b[N - 1])) >= 0.05 and e.offs[0] + T <= e.P and e.offs[1] + H <= e.P and e.offs[2] + W <= e.P
    return c


def ref_args(c, table=True):
    """What dense16_ref takes for the everything-at-once launch: the up-cast values of the uploaded tensors."""
    kw = dict(a=up(c.a), w=up(c.w), b=up(c.b), K=c.K, act="gelu", res=up(c.res), dot_vec=up(c.vec))
    if table:
        kw.update(tab=up(c.tab), geom=c.geom)
    return kw


@functools.lru_cache(maxsize=None)
def reference(id, table=True):
    return R.dense16_ref(**ref_args(build(id), table))


def nt_bounds(c, ref):
    """Bounds of the NT outputs from the reference's own quantities (module docstring): scalars for y / val / pre, [slices, M] for the
    slice sums."""
    scale = max(1.0, float(ref["pre"].abs().max()))
    d = 2e-5 * scale
    vec = up(c.vec)[None, :]
    return {"y": torch.tensor(d, dtype=torch.float64), "val": torch.tensor(2.0 ** -11 * scale + 1e-6, dtype=torch.float64),
            "pre": torch.tensor(2.0 ** -10 * scale, dtype=torch.float64),
            "ssq": 2 * d * R.slice_sums(ref["pre"].abs()) + 64 * EPS23 * R.slice_sums(ref["pre"] ** 2),
            "rdot": d * R.slice_sums(vec.abs().expand_as(ref["y"])) + 64 * EPS23 * R.slice_sums((vec * ref["y"]).abs())}


def checked_outputs(c):
    """The outputs tests/test_gpu_dense16.py always checks for the case: pre and rdot need the row epilogue (N % 8 == 0)."""
    return ("ssq", "val", "y") + (("pre", "rdot") if c.N % 8 == 0 else ())


# ---- TN ---------------------------------------------------------------------------------------------------------------------------
def tn_stages(Kt):
    return (Kt + 63) // 64


def tn_live_splits(Kt, splits):
    """(stages per split, number of splits that own at least one stage): restated from dense16_tn_kernel (`per`, `s0 < ns_total`)."""
    per = (tn_stages(Kt) + splits - 1) // splits
    return per, (tn_stages(Kt) + per - 1) // per


@functools.lru_cache(maxsize=None)
def build_tn(id):
    """a_full [rows, lda], b_full [rows, ldb] with rows = 64 ceil(Kt / 64) + 8: NaN outside [:Kt, :M] / [:Kt, :N]."""
    e = TN_BY_ID[id]
    g = torch.Generator().manual_seed(_seed(id))
    rows, dt = 64 * tn_stages(e.Kt) + 8, DTYPES[e.dtype]
    a = torch.full((rows, e.lda), NAN)
    b = torch.full((rows, e.ldb), NAN)
    a[:e.Kt, :e.M] = torch.randn(e.Kt, e.M, generator=g) * 0.5
    b[:e.Kt, :e.N] = torch.randn(e.Kt, e.N, generator=g) * 0.5
    return SimpleNamespace(entry=e, a_full=a.to(dt), b_full=b.to(dt))


@functools.lru_cache(maxsize=None)
def reference_tn(id):
    c = build_tn(id)
    e = c.entry
    return R.dense16_tn_ref(up(c.a_full)[:e.Kt], up(c.b_full)[:e.Kt], e.M, e.N)


def tn_tol(Kt, want):
    return 2e-6 * Kt ** 0.5 * 4 + 1e-5 * float(want.abs().max())
