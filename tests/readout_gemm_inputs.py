"""Inputs, expected output images and error bounds for the three readout GEMMs: readout_gemm_kernel (csrc/readout_gemm.hip, "gemm":
fp32 activations split into bf16 hi + lo on the fly, 64 x 64 tiles, K loop in groups of three), planes_gemm_kernel<HAS_LO>
(csrc/planes_gemm.hip, "planes": bf16 hi / lo planes, 48 x 128 tiles, five-slot ring) and readout16_gemm_kernel in its 96 x 64 form
(csrc/readout16.hip, "r16": fp16 operands, eight-stage ring, row-line and general epilogue).  Shared by tests/test_gpu_readout_gemm.py
(the kernels against these images) and tests/test_readout_gemm_power.py (CPU: what a wrong kernel would do to the images).

Two input families per case (build):
  exact   every product and every partial sum in any order is exactly representable in fp32, so a correct kernel reproduces the
          float64 value bit for bit (bound zero).  Always run WITHOUT the activation.  Split forms: x = a + c 2^-9 with integers
          1 <= |a| <= 4, 1 <= |c| <= 3 of one sign (hi and lo are both nonzero multiples of 2^-9 everywhere and hi + lo == x exactly); fp16 form:
          nonzero integers / 8, |a| <= 4.  Weights: nonzero integers in [-6, 6] times 2^-4.  Bias: integers in [-31, 31] times 2^-6.
          build() asserts the condition: every term is a multiple of one power of two g and max sum |terms| / g < 2^24.  Cases with
          K > 704 (r16 only: 16 and 17 stages) do not run this family.
  round   seeded normal values that are not bf16-representable: x = N(0, 1) + 2^-10 N(0, 1) in f32 (split on the host exactly as
          split_bf16 of csrc/common.hpp does for the planes form), a16 = 0.7 N(0, 1) in fp16; w = 0.03 N(0, 1) in bf16 (r16: 0.02, cast
          to fp16); b = 0.1 N(0, 1) rounded to bf16 (an f32 bias holds the same values).  Run with the case's activation.
Both families are seeded by (kernel, M, N, K) alone, so two cases that differ only in layout see the same operands.

Outputs (expected): every output is an image [rows, ld] in float64 with NaN where the kernel must not write.  The test allocates it
NaN-filled with GUARD_FRONT rows in front; the image itself ends in GUARD_BACK rows that stay NaN, and its columns [N, ld) stay NaN.
  y       the packed rows in the case's type, at rows row0 + m + m // nl_group;   y32: the same launch with f32 rows, taken for every
          case whose rows are bf16 (so that a 16-bit rounding never is the only witness)
  hi, lo  (planes, exact family) the bf16 planes = split_bf16 of the value;   planes (round family): hi + lo
  p16     (r16) the fp16 plane
Bounds of the round family, elementwise (bounds): sum_tol(products + 1, sum |terms|) on the pre-activation; with GELU that times
max |GELU'| = GELU_SLOPE, plus the function's own error (ERF_AS_ERR + TRANS) |h| / 2 -- the stated error of the Abramowitz-Stegun
7.1.26 erf of gelu_erf (checked against float64 erf in tests/test_ops_references.py) and 2^-21 for its hardware reciprocal and exp2 --
plus three fp32 roundings; plus the output rounding: BF16_RND |ref| (bf16 rows), 2^-17 |ref| (hi + lo), F16_RND |ref| + F16_SUB (fp16).

Case fields: kernel, M, N, K, act (GELU in the round family), bias ("bf16" | "f32" | None), out ("y" | "plane" | "both"), ydt, lo (planes:
HAS_LO), ld_extra (ldy = N + ld_extra), (row0, nl_group), y_off / p_off / b_off (the tensor is a view that many elements into its
allocation: the scalar store / bias paths, and for r16 the general epilogue in place of the row-line one).  The table follows (id:
what the case reaches).
"""
import functools
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch

import ops_reference as R
from ops_reference import EPS23, up

NAN = float("nan")
BF16_RND, F16_RND, F16_SUB, TRANS = 2.0 ** -8, 2.0 ** -10, 2.0 ** -24, 2.0 ** -21
GUARD_FRONT, GUARD_BACK = 8, 2
EXACT_K_MAX = 704
TILES = {"gemm": (64, 64, 3), "planes": (48, 128, 5), "r16": (96, 64, 8)}        # rows, columns of a tile; ring depth / unroll group
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


class Case(NamedTuple):
    kernel: str
    M: int
    N: int
    K: int
    act: int
    bias: Optional[str]
    out: str
    ydt: Optional[str]
    what: str
    lo: bool = True
    ld_extra: int = 0
    row0: int = 0
    nl_group: int = 0
    y_off: int = 0
    p_off: int = 0
    b_off: int = 0

    @property
    def id(self):
        s = f"{self.kernel}{'' if self.lo else '_hi'}_k{self.K // 64}_m{self.M}_n{self.N}_{'gelu' if self.act else 'lin'}_b{self.bias}_{self.out}"
        s += f"_{self.ydt}" if self.ydt else ""
        s += f"_ld{self.ld_extra}" if self.ld_extra else ""
        s += f"_r{self.row0}g{self.nl_group}" if (self.row0 or self.nl_group) else ""
        for n, v in (("yoff", self.y_off), ("poff", self.p_off), ("boff", self.b_off)):
            s += f"_{n}{v}" if v else ""
        return s

    @property
    def has_y(self):
        return self.out in ("y", "both")

    @property
    def has_plane(self):
        return self.out in ("plane", "both")

    @property
    def ns(self):
        return self.K // 64

    @property
    def ld(self):
        return self.N + self.ld_extra


def _g(M, N, K64, act, bias, ydt, what, **kw):
    return Case("gemm", M, N, 64 * K64, act, bias, "y", ydt, what, **kw)


def _p(M, N, K64, act, bias, out, ydt, what, **kw):
    return Case("planes", M, N, 64 * K64, act, bias, out, ydt, what, **kw)


def _r(M, N, K64, act, bias, out, ydt, what, **kw):
    return Case("r16", M, N, 64 * K64, act, bias, out, ydt, what, **kw)


GEMM_CASES = (
    _g(1, 1, 1, 0, None, "f32", "ns = 1: both prologue clamps, every later load re-loads stage 0; one row, one column, no bias"),
    _g(63, 63, 2, 1, "bf16", "f32", "ns = 2: the `ns > 2` clamp; row and weight-row clamp by one; GELU; ldy > N; gaps of 9 behind 3 rows", ld_extra=8, row0=3, nl_group=9),
    _g(64, 64, 3, 0, "f32", "bf16", "ns = 3: one full group of three; exactly one tile; f32 bias; a gap behind every row", row0=2, nl_group=1),
    _g(65, 65, 4, 0, "bf16", "f32", "ns = 4: a group with two tail steps; one row and one column in the second tiles; group > M", nl_group=66),
    _g(130, 118, 5, 1, "f32", "bf16", "ns = 5: a group with one tail step; three row tiles; N % 64 = 54; GELU to bf16 rows", ld_extra=8, row0=3, nl_group=9),
    _g(65, 130, 6, 0, None, "bf16", "ns = 6: two full groups; three column tiles; no bias"),
    _g(130, 65, 7, 0, "bf16", "f32", "ns = 7: two groups and one stage", ld_extra=8, row0=2, nl_group=1),
    _g(513, 118, 2, 0, "bf16", "f32", "the ninth row block: second pass of the XCD tile order with nbx = 2", row0=3, nl_group=9),
    _g(1, 130, 3, 1, "f32", "f32", "one row against three column tiles; GELU with an f32 bias", row0=2, nl_group=1),
    _g(63, 1, 4, 0, "bf16", "bf16", "one column: every weight row of the tile clamps to row 0", ld_extra=8),
    _g(64, 118, 1, 1, None, "f32", "ns = 1 with a ragged second column tile; GELU without bias; group > M", nl_group=65),
    _g(65, 64, 5, 1, "bf16", "bf16", "ns = 5 with one row in the second row tile", row0=3, nl_group=9),
    _g(130, 63, 6, 0, "f32", "f32", "ns = 6, three row tiles, ragged single column tile, ldy > N", ld_extra=8),
    _g(63, 65, 7, 1, "bf16", "f32", "ns = 7 with GELU; one column in the second tile", row0=2, nl_group=1),
    _g(64, 130, 2, 0, "bf16", "bf16", "ns = 2 with three column tiles, the last of two columns", ld_extra=8, row0=3, nl_group=9),
    _g(130, 64, 3, 0, None, "f32", "ns = 3, M = 2 tiles + 2 rows; group > M", nl_group=131),
    _g(1, 63, 5, 0, "bf16", "bf16", "one row: every activation row of the tile clamps to row 0", row0=3, nl_group=9),
    _g(65, 1, 2, 1, "f32", "f32", "one column, two row tiles, GELU", ld_extra=8, row0=2, nl_group=1),
    _g(63, 118, 4, 0, "f32", "bf16", "ns = 4, ragged in both directions"),
    _g(64, 65, 1, 0, "bf16", "f32", "ns = 1, one column in the second tile, ldy > N", ld_extra=8, row0=3, nl_group=9),
)

PLANES_CASES = (
    _p(1, 1, 1, 0, None, "y", "f32", "ns = 1: prologue of one stage; one row, one column: every DMA row clamps; scalar stores"),
    _p(47, 3, 2, 1, "bf16", "both", "f32", "ns = 2: parity tail with a step; N % 4 != 0: scalar stores and scalar bias tail", ),
    _p(48, 4, 3, 0, "f32", "plane", None, "HAS_LO = false, ns = 3: draining loop once; exactly one row tile; one vector group", lo=False),
    _p(49, 127, 4, 0, "bf16", "y", "bf16", "ns = 4: prologue fills the ring; N = 127: the last group is partial; bf16 rows scalar", row0=3, nl_group=9),
    _p(97, 128, 5, 1, "f32", "both", "f32", "ns = 5: ring exactly full, no steady step; vector stores of planes and f32 rows; vector f32 bias", ld_extra=8, row0=2, nl_group=1),
    _p(48, 129, 6, 0, "bf16", "y", "f32", "HAS_LO = false, ns = 6: one steady pair; one column in the second column tile", lo=False),
    _p(49, 130, 7, 0, None, "both", "bf16", "ns = 7: one steady pair, odd tail; N % 4 = 2; no bias", row0=3, nl_group=9),
    _p(47, 257, 8, 1, "bf16", "plane", None, "ns = 8: two steady pairs; three column tiles, the last of one column"),
    _p(97, 4, 9, 0, "bf16", "both", "f32", "HAS_LO = false, ns = 9; ldy = N + 2: ldy % 4 != 0 takes the scalar stores at N % 4 == 0", lo=False, ld_extra=2),
    _p(48, 128, 10, 0, "bf16", "y", "f32", "ns = 10; y one element into its allocation: base off 16 bytes, scalar stores", y_off=1),
    _p(49, 128, 11, 0, "bf16", "both", "f32", "ns = 11: three steady pairs, odd tail; bias as b[1:] (bvec = 0)", b_off=1),
    _p(385, 130, 2, 0, "bf16", "y", "f32", "the ninth row block: second pass of the XCD tile order with nbx = 2", row0=3, nl_group=9),
    _p(47, 128, 5, 1, None, "y", "bf16", "HAS_LO = false, ns = 5, GELU without bias, bf16 rows as vectors, ldy > N", lo=False, ld_extra=8),
    _p(1, 130, 7, 0, "f32", "both", "f32", "HAS_LO = false, ns = 7, one row; f32 bias scalar tail", lo=False),
    _p(49, 3, 10, 0, "bf16", "y", "f32", "HAS_LO = false, ns = 10, N = 3", lo=False, row0=2, nl_group=1),
    _p(97, 127, 11, 1, "bf16", "plane", None, "HAS_LO = false, ns = 11, GELU, planes alone, scalar", lo=False),
    _p(97, 257, 6, 0, "f32", "y", "bf16", "ns = 6; f32 bias as b[1:]: 4 bytes off, bvec = 0; three row tiles x three column tiles", b_off=1),
    _p(1, 128, 9, 1, "bf16", "plane", None, "ns = 9 with GELU: planes alone, vector stores"),
    _p(385, 129, 2, 0, "bf16", "y", "f32", "HAS_LO = false on the ninth row block; group > M", lo=False, nl_group=386),
    _p(48, 4, 8, 0, None, "both", "f32", "ns = 8, N = 4 with ldy = N + 2: scalar stores; no bias", ld_extra=2),
    _p(47, 257, 1, 0, "bf16", "both", "bf16", "HAS_LO = false, ns = 1", lo=False),
    _p(48, 130, 4, 1, "f32", "y", "f32", "HAS_LO = false, ns = 4, GELU; y one element into its allocation", lo=False, y_off=1),
    _p(49, 1, 8, 0, "bf16", "plane", None, "HAS_LO = false, ns = 8, one column", lo=False),
    _p(97, 129, 3, 1, "bf16", "y", "f32", "ns = 3 with GELU, f32 rows, ldy > N", ld_extra=8, row0=3, nl_group=9),
)

R16_CASES = (
    _r(1, 1, 1, 0, None, "plane", None, "ns = 1; one row, one column; general epilogue, scalar store"),
    _r(95, 4, 2, 1, "bf16", "plane", None, "ns = 2; the plane alone with N % 8 != 0: general epilogue, 8-byte vectors"),
    _r(96, 8, 3, 0, "bf16", "plane", None, "ns = 3; N = 8: row-line form requested, but no whole 64-column tile: general epilogue"),
    _r(97, 64, 4, 0, "f32", "plane", None, "ns = 4; the plane alone through the row-line epilogue; one row in the second row tile"),
    _r(97, 64, 4, 0, "f32", "plane", None, "the same with the plane 8 bytes off a 16-byte base: general epilogue", p_off=4),
    _r(193, 200, 5, 1, "bf16", "y", "bf16", "ns = 5; bf16 rows alone: row-line for three column tiles, general for the fourth (8 columns)", row0=3, nl_group=9),
    _r(193, 200, 5, 1, "bf16", "y", "bf16", "the same with y 8 bytes off a 16-byte base: general epilogue, scalar stores", row0=3, nl_group=9, y_off=4),
    _r(96, 63, 6, 0, "bf16", "both", "f32", "ns = 6; plane + f32 rows, N = 63: scalar stores"),
    _r(95, 65, 7, 1, "f32", "both", "f32", "ns = 7: prologue exactly fills the ring; one column in the second column tile", ld_extra=8),
    _r(97, 100, 8, 0, "bf16", "both", "f32", "ns = 8: ring exactly full (first wrap of slot 0); ldy = N + 2: ldy % 4 != 0", ld_extra=2),
    _r(1, 64, 9, 0, "bf16", "y", "bf16", "ns = 9: one steady pair; bf16 rows alone, row-line, a gap behind every row", row0=2, nl_group=1),
    _r(1, 64, 9, 0, "bf16", "y", "bf16", "the same with y one element into its allocation: general epilogue", row0=2, nl_group=1, y_off=1),
    _r(193, 8, 10, 1, None, "plane", None, "ns = 10: one steady pair, even tail; three row tiles; no bias"),
    _r(96, 64, 16, 0, "bf16", "plane", None, "ns = 16: the ring wraps twice (round family only: K > 704)"),
    _r(97, 200, 17, 1, "bf16", "plane", None, "ns = 17 with GELU: row-line for three column tiles, general for the fourth (round family only)"),
    _r(769, 64, 2, 0, "bf16", "y", "bf16", "the ninth row tile; bf16 rows through the row-line epilogue", row0=3, nl_group=9),
    _r(193, 64, 8, 1, "bf16", "plane", None, "ns = 8 with GELU, row-line; bias as b[1:] (bvec = 0)", b_off=1),
    _r(95, 200, 7, 0, "f32", "y", "bf16", "ns = 7; bf16 rows with ldy = N + 8; group > M", ld_extra=8, nl_group=96),
    _r(96, 4, 9, 0, "bf16", "both", "f32", "ns = 9; N = 4: one vector group"),
    _r(97, 65, 10, 0, "f32", "both", "f32", "ns = 10; f32 bias scalar tail", row0=2, nl_group=1),
    _r(769, 100, 3, 1, "bf16", "both", "f32", "the ninth row tile with two column tiles, GELU"),
    _r(1, 200, 6, 0, None, "y", "bf16", "ns = 6; one row; no bias; row-line + general"),
    _r(193, 63, 2, 0, "bf16", "y", "bf16", "bf16 rows alone with N % 8 != 0: general epilogue, ldy > N", ld_extra=8),
    _r(95, 8, 1, 1, "f32", "plane", None, "ns = 1 with GELU and a vector f32 bias"),
)

CASES = GEMM_CASES + PLANES_CASES + R16_CASES
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
__doc__ += "\n".join(f"  {c.id}: {c.what}" for c in CASES) + "\n"


def families(c):
    return ("exact", "round") if c.K <= EXACT_K_MAX else ("round",)


def act_of(c, family):
    return "gelu" if (family == "round" and c.act) else "none"


def nterms(c):
    return 2 if (c.kernel == "gemm" or (c.kernel == "planes" and c.lo)) else 1


def y_rows(c):
    return int(R.packed_rows(c.M, c.row0, c.nl_group)[-1]) + 1 + GUARD_BACK


def _seed(c, family):
    return ({"gemm": 1, "planes": 2, "r16": 3}[c.kernel] * 1000003 + c.M * 10007 + c.N * 101 + c.K) * 2 + (family == "exact")


@functools.lru_cache(maxsize=None)
def build(id, family):
    """The tensors of case `id` as the kernel receives them (CPU; callers must not write into them) and their float64 values:
    x f32 (gemm) | hi, lo bf16 (planes; lo None without a lo plane) | a16 fp16 (r16); w bf16 (r16: fp16); b in the case's bias type or
    None; a_terms, w64, b64 for R.readout_gemm_ref."""
    c = BY_ID[id]
    M, N, K = c.M, c.N, c.K
    g = torch.Generator().manual_seed(_seed(c, family))
    d = SimpleNamespace(case=c, family=family, x=None, hi=None, lo=None, a16=None)
    if family == "exact":
        assert K <= EXACT_K_MAX
        ints = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
        sign = lambda *s: 1.0 - 2.0 * torch.randint(0, 2, s, generator=g).float()
        w = sign(N, K) * ints(1, 6, N, K) * 2.0 ** -4
        b = ints(-31, 31, N) * 2.0 ** -6
        if c.kernel == "r16":
            a = sign(M, K) * ints(1, 32, M, K) / 8
        else:
            a = sign(M, K) * (ints(1, 4, M, K) + ints(1, 3, M, K) * 2.0 ** -9)
    else:
        rnd = lambda *s: torch.randn(*s, generator=g)
        if c.kernel == "r16":
            a, w = rnd(M, K) * 0.7, (rnd(N, K) * 0.02).bfloat16().float()
        else:
            a = rnd(M, K)
            a, w = (a + rnd(M, K) * 2.0 ** -10).float(), rnd(N, K) * 0.03
        b = rnd(N) * 0.1
    b = b.bfloat16()
    d.b = None if c.bias is None else b.to(DTYPES[c.bias])
    d.b64 = None if c.bias is None else up(b)
    if c.kernel == "r16":
        d.a16, d.w = a.half(), w.half()
        d.a_terms = [up(d.a16)]
    else:
        d.w = w.bfloat16()
        hi, lo = R.split_bf16_ref(a)
        if c.kernel == "gemm":
            d.x = a
        else:
            d.hi, d.lo = hi, (lo if c.lo else None)
        d.a_terms = [up(hi), up(lo)] if nterms(c) == 2 else [up(hi)]
    d.w64 = up(d.w)
    if family == "exact":
        ga = 2.0 ** -3 if c.kernel == "r16" else 2.0 ** -9
        unit = ga * 2.0 ** -4
        whole = lambda t, q: bool((t / q == (t / q).round()).all())
        assert torch.equal(d.w64, w.double()) and whole(d.w64, 2.0 ** -4) and all(whole(t, ga) for t in d.a_terms)
        assert d.b64 is None or whole(d.b64, unit)
        assert c.kernel == "r16" or torch.equal(d.a_terms[0] + up(lo), a.double())          # x == hi + lo exactly
        val, ab, _ = R.readout_gemm_ref(d.a_terms, d.w64, d.b64)
        assert float(ab.max()) / unit < 2.0 ** 24, (id, float(ab.max()) / unit)
        assert torch.equal(val.float().double(), val) and float(val.abs().max()) < 65504.0
        for t in d.a_terms:                                                                  # every stage of every plane is live
            assert bool((t.reshape(M, K // 64, 64) != 0).all())
    return d


def base_tol(c, family, val, ab, pre):
    """The elementwise bound of the f32 value (module docstring); zeros in the exact family."""
    if family == "exact":
        return torch.zeros_like(val)
    t = R.sum_tol(nterms(c) * c.K + 1, ab)
    if act_of(c, family) == "gelu":
        _, derf = R.gelu_ref(pre)
        t = R.GELU_SLOPE * t + (R.ERF_AS_ERR + TRANS) * derf + 3 * EPS23 * (val.abs() + derf)
    return t


def stage_set(c):
    """Stages at which the per-stage faults are planted: 0, ns - 1 and one in every residue class of the ring depth."""
    return sorted({0, c.ns - 1} | set(range(min(TILES[c.kernel][2], c.ns))))


def faults(c, family):
    """name -> (keywords of R.readout_gemm_ref, layout faults) for every fault that applies to the case in this family."""
    TM, TN, _ = TILES[c.kernel]
    M, N, ns = c.M, c.N, c.ns
    m, n = torch.arange(M), torch.arange(N)
    f = {}
    for s in stage_set(c):
        if nterms(c) == 2:
            f[f"lo_stage_{s}"] = (dict(drop_lo_stage=s), {})
        if s >= 1:
            f[f"stale_stage_{s}"] = (dict(stale_stage=s), {})
    f["last_missing"] = (dict(drop_stage=ns - 1), {})
    f["last_twice"] = (dict(double_stage=ns - 1), {})
    if c.kernel == "planes":
        f["half_lost"] = (dict(lost_half=(ns - 1, 1, 16 * ((N - 1) // 16), N)), {})
    if M % TM >= 2:
        f["tail_rows"] = (dict(row_of=torch.where(m >= M // TM * TM, torch.full_like(m, M - 1), m)), {})
    if N % TN >= 2:
        f["tail_cols"] = (dict(col_of=torch.where(n >= N // TN * TN, torch.full_like(n, N - 1), n)), {})
    if c.bias is not None:
        if N >= 2:
            f["bias_shift4"] = (dict(bias_of=(n + 4).clamp(max=N - 1)), {})
        if N % 4 >= 2:
            f["bias_tail_group"] = (dict(bias_of=torch.where(n >= N // 4 * 4, torch.full_like(n, N - 1), n)), {})
        if act_of(c, family) == "gelu":
            f["gelu_before_bias"] = (dict(gelu_before_bias=True), {})
    if c.has_y:
        if c.nl_group > 0 and M >= c.nl_group:
            f["gap_late"] = ({}, dict(gap_late=True))
        if c.row0 > 0:
            f["row0_dropped"] = ({}, dict(row0_dropped=True))
        f["y32_is_bf16"] = ({}, dict(y32_is_bf16=True))
        if c.ld_extra > 0 and (M >= 2 or c.row0 > 0):
            f["pitch_is_N"] = ({}, dict(pitch_is_N=True))
    return f


FAULT_KINDS = ("lo_stage", "stale_stage", "last_missing", "last_twice", "half_lost", "tail_rows", "tail_cols", "bias_shift4", "bias_tail_group",
               "gelu_before_bias", "gap_late", "row0_dropped", "y32_is_bf16", "pitch_is_N")


def kind_of(name):
    return name.rsplit("_", 1)[0] if name.startswith(("lo_stage_", "stale_stage_")) else name


@functools.lru_cache(maxsize=None)
def expected(id, family, fault=None):
    """key -> (image, bound image) of every output tests/test_gpu_readout_gemm.py checks for the case (module docstring); `fault` names an
    entry of faults(c, family) to plant.  Exact family: the images hold the values as rounded to the output type and the bounds are zero."""
    c, d = BY_ID[id], build(id, family)
    ref_kw, lay = faults(c, family)[fault] if fault else ({}, {})
    val, ab, pre = R.readout_gemm_ref(d.a_terms, d.w64, d.b64, act_of(c, family), **ref_kw)
    exact = family == "exact"
    tol = base_tol(c, family, val, ab, pre)
    f32 = val.float()
    out = {}
    if c.has_y:
        orow = R.packed_rows(c.M, 0 if lay.get("row0_dropped") else c.row0, c.nl_group, gap_late=lay.get("gap_late", False))
        img = lambda v: R.place_rows(v, y_rows(c), c.ld, orow, c.N if lay.get("pitch_is_N") else None)
        v32 = up(f32.bfloat16()) if lay.get("y32_is_bf16") else (up(f32) if exact else val)
        if c.ydt == "f32":
            out["y"] = (img(v32), img(tol))
        else:
            out["y"] = (img(up(f32.bfloat16()) if exact else val), img(tol if exact else tol + BF16_RND * val.abs()))
            out["y32"] = (img(v32), img(tol))
    if c.has_plane:
        img = lambda v: R.place_rows(v, c.M + GUARD_BACK, c.N, torch.arange(c.M))
        if c.kernel == "r16":
            out["p16"] = (img(up(f32.half()) if exact else val), img(tol if exact else tol + F16_RND * val.abs() + F16_SUB))
        elif exact:
            hi, lo = R.split_bf16_ref(f32)
            out["hi"], out["lo"] = (img(up(hi)), img(tol)), (img(up(lo)), img(tol))
        else:
            out["planes"] = (img(val), img(tol + 2.0 ** -17 * val.abs()))
    return out


def moved(good, bad):
    """By how many bounds the planted fault moves the checked images at the least-forgiving element: inf where an element is live in one
    image and NaN in the other, or differs at a zero bound."""
    best = 0.0
    for k, (g, t) in good.items():
        b = bad[k][0]
        if not torch.equal(torch.isnan(g), torch.isnan(b)):
            return float("inf")
        live = ~torch.isnan(g)
        diff, t = (b[live] - g[live]).abs(), t[live]
        if bool(((t == 0) & (diff > 0)).any()):
            return float("inf")
        if bool((t > 0).any()):
            best = max(best, float((diff[t > 0] / t[t > 0]).max()))
    return best


# Faults that cannot reach POWER bounds in the round family of a case and are therefore witnessed by its exact family alone
# (tests/test_readout_gemm_power.py checks the exact family for them and holds this list to the pairs that need it).  The bound of
# the round family grows with K (sum_tol over 2 K + 1 terms) while one stage's lo plane contributes a few 1e-5 whatever K is.
_LO = lambda *s: tuple(f"lo_stage_{i}" for i in s)
EXACT_ONLY = {
    "gemm_k5_m130_n118_gelu_bf32_y_bf16_ld8_r3g9": _LO(0, 1, 2, 4),
    "gemm_k6_m65_n130_lin_bNone_y_bf16": _LO(0, 1, 2, 5),
    "gemm_k7_m130_n65_lin_bbf16_y_f32_ld8_r2g1": _LO(0, 1, 2, 6),
    "gemm_k3_m1_n130_gelu_bf32_y_f32_r2g1": _LO(0),
    "gemm_k4_m63_n1_lin_bbf16_y_bf16_ld8": _LO(0, 2, 3),
    "gemm_k5_m65_n64_gelu_bbf16_y_bf16_r3g9": _LO(0, 1, 2, 4),
    "gemm_k6_m130_n63_lin_bf32_y_f32_ld8": _LO(0, 1, 2, 5),
    "gemm_k7_m63_n65_gelu_bbf16_y_f32_r2g1": _LO(0, 1, 2, 6),
    "gemm_k5_m1_n63_lin_bbf16_y_bf16_r3g9": _LO(0, 1, 2, 4),
    "planes_k5_m97_n128_gelu_bf32_both_f32_ld8_r2g1": _LO(0, 1, 2, 3, 4),
    "planes_k7_m49_n130_lin_bNone_both_bf16_r3g9": _LO(0, 1, 2, 3, 4, 6),
    "planes_k8_m47_n257_gelu_bbf16_plane": _LO(0, 1, 2, 3, 4, 7),
    "planes_k10_m48_n128_lin_bbf16_y_f32_yoff1": _LO(0, 1, 2, 3, 4, 9),
    "planes_k11_m49_n128_lin_bbf16_both_f32_boff1": _LO(0, 1, 2, 3, 4, 10) + ("y32_is_bf16",),
    "planes_hi_k10_m49_n3_lin_bbf16_y_f32_r2g1": ("y32_is_bf16",),
    "planes_k6_m97_n257_lin_bf32_y_bf16_boff1": _LO(0, 1, 2, 3, 4, 5),
    "planes_k9_m1_n128_gelu_bbf16_plane": _LO(0, 1, 2, 3, 4, 8),
    "planes_k8_m48_n4_lin_bNone_both_f32_ld2": _LO(0, 1, 2, 3, 4, 7) + ("y32_is_bf16",),
}
assert set(EXACT_ONLY) <= set(BY_ID)
