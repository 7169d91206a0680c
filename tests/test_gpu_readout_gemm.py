"""The three readout GEMMs -- readout_gemm_kernel, planes_gemm_kernel<HAS_LO> and readout16_gemm_kernel (96 x 64 form, no role) --
against the float64 reference R.readout_gemm_ref on the case table of tests/readout_gemm_inputs.py (its docstring lists the cases, the
two input families and the bounds).  tests/test_readout_gemm_power.py shows on the reference alone that a kernel which drops or re-reads
a stage, loses a k half, clamps a whole tail tile, shifts the bias, applies GELU early or mis-places a row misses these checks.

Per case and family, every output is allocated NaN-filled with guard rows in front and behind (and guard columns where ldy > N) and
compared as a whole image: every live element is written; rows < row0, gap rows, trailing rows, columns [N, ldy), plane rows >= M and
the elements in front of an offset view keep their NaN.
  exact family (no activation)   f32 rows equal the float64 value; bf16 rows, the hi / lo planes and the fp16 plane equal its RNE
                                 rounding resp. split_bf16 -- bound zero
  round family (the case's act)  |got - ref| <= bound elementwise (gi.base_tol + the output rounding)
  cross-form identities          bf16 rows == (f32 rows of a second launch).bfloat16(); the other bias type (same values) gives the same
                                 bits; r16: the row-line and the general epilogue give the same bits
  refusals                       K % 64 != 0, ldy < N, negative row0, an activation or weight base off 16 bytes, no output at all:
                                 HicomNativeError (non-zero status), the NaN-filled outputs untouched
Every check prints `READOUT <name> err=<largest error> bound=<bound there> ratio=<largest error / bound>`.

Measured on an MI355X (all 68 cases; the range over the cases of the largest error / bound per output): no fault found.
  exact family       every output of every case bit for bit (err = 0)
  round family       gemm             planes           r16
  f32 rows (y)       8.3e-4 .. 1.1e-2  2.2e-4 .. 3.5e-3  6.8e-4 .. 3.9e-3   err <= 9.0e-07
  f32 rows (y32)     5.7e-4 .. 3.8e-3  4.8e-4 .. 7.1e-3  4.0e-4 .. 5.0e-3   err <= 8.9e-07
  bf16 rows          0.68 .. 0.95      0.81 .. 0.98      0.73 .. 0.98       err <= 7.4e-03
  hi + lo planes                       2.2e-3 .. 0.30                       err <= 1.5e-05
  fp16 plane                                             0.066 .. 0.43      err <= 4.9e-04
The f32 outputs sit two to three orders below their bound (sum_tol is a worst case over the order of 2 K + 1 terms); the 16-bit outputs
sit below one because their bound is the half-ulp rounding itself.  The whole file runs in about 3 s.
"""
import pytest
import torch

import readout_gemm_inputs as gi
from ops_reference import up
from hicom_amd import native as nv

pytestmark = pytest.mark.gpu

NAN = float("nan")
GF = gi.GUARD_FRONT
IDS = {k: [c.id for c in gi.CASES if c.kernel == k] for k in ("gemm", "planes", "r16")}
PLANE_DT = {"hi": torch.bfloat16, "lo": torch.bfloat16, "planes": torch.bfloat16, "p16": torch.float16}


class Buf:
    """A NaN-filled allocation of `off` elements + GF guard rows + `rows` rows of `ld`; `view` is what the kernel gets."""

    def __init__(self, rows, ld, dtype, off=0):
        self.flat = torch.full((off + (GF + rows) * ld,), NAN, dtype=dtype, device="cuda")
        self.off = off
        self.body = self.flat[off:].view(GF + rows, ld)
        self.view = self.body[GF:]
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == (off * self.flat.element_size()) % 16

    def front_untouched(self):
        return bool(torch.isnan(self.flat[:self.off + GF * self.body.shape[1]]).all())

    def untouched(self):
        return bool(torch.isnan(self.flat).all())


_DEV = {}


def device_inputs(id, family):
    """The case's operands on the device; the bias in both types (`b` the case's own, with its offset; `b_other` the same values in the
    other type, aligned)."""
    if (id, family) not in _DEV:
        c, d = gi.BY_ID[id], gi.build(id, family)
        o = {n: (None if getattr(d, n) is None else getattr(d, n).cuda()) for n in ("x", "hi", "lo", "a16", "w")}
        o["b"] = o["b_other"] = None
        if d.b is not None:
            hold = torch.zeros(c.N + c.b_off, dtype=d.b.dtype, device="cuda")
            hold[c.b_off:] = d.b.cuda()
            o["b"] = hold[c.b_off:]
            o["b_other"] = d.b.to(torch.float32 if d.b.dtype == torch.bfloat16 else torch.bfloat16).cuda()
            assert o["b"].data_ptr() % 16 == (c.b_off * d.b.element_size()) % 16
        _DEV[(id, family)] = o
    return _DEV[(id, family)]


def launch(c, dev, family, ydt, b, y_off=None, p_off=None):
    """One launch of the case's kernel with rows of type `ydt` (None: no rows) and the planes the case asks for: key -> Buf."""
    act = nv.ACT_GELU if gi.act_of(c, family) == "gelu" else nv.ACT_NONE
    y_off, p_off = (c.y_off if y_off is None else y_off), (c.p_off if p_off is None else p_off)
    o = {}
    if ydt is not None:
        o["y"] = Buf(gi.y_rows(c), c.ld, gi.DTYPES[ydt], y_off)
    y = o["y"].view if "y" in o else None
    planes = lambda *names: [o.setdefault(n, Buf(c.M + gi.GUARD_BACK, c.N, PLANE_DT[n], p_off)).view[:c.M] for n in names]
    if c.kernel == "gemm":
        nv.readout_gemm(dev["x"], dev["w"], b, y, act=act, row0=c.row0, nl_group=c.nl_group, M=c.M)
    elif c.kernel == "planes":
        hi, lo = planes("hi", "lo") if c.has_plane else (None, None)
        nv.planes_gemm(dev["hi"], dev["lo"], dev["w"], b, act=act, out_hi=hi, out_lo=lo, y=y, row0=c.row0, nl_group=c.nl_group)
    else:
        p16 = planes("p16")[0] if c.has_plane else None
        nv.readout16_gemm(dev["a16"], dev["w"], b, act=act, out_f16=p16, y=y, row0=c.row0, nl_group=c.nl_group)
    torch.cuda.synchronize()
    return o


def compare(name, buf, img, tol):
    """The whole image: NaN exactly where the reference image is NaN (and in front of it), |got - ref| <= tol elsewhere (tol 0: equal)."""
    got = up(buf.view)
    assert got.shape == img.shape, (name, got.shape, img.shape)
    assert buf.front_untouched(), f"{name}: an element in front of the output was written"
    live = ~torch.isnan(img)
    wrote = ~torch.isnan(got)
    assert bool((wrote | ~live).all()), f"{name}: {int((live & ~wrote).sum())} live elements were not written (or are NaN)"
    assert bool((live | ~wrote).all()), f"{name}: {int((wrote & ~live).sum())} elements outside the live rows and columns were written"
    err, t = (got[live] - img[live]).abs(), tol[live]
    assert bool(torch.isfinite(err).all()), f"{name}: non-finite values in the result"
    ratio = torch.where(t > 0, err / t.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    i = int(ratio.argmax())
    print(f"READOUT {name} err={float(err.max()):.3e} bound={float(t[i]):.3e} ratio={float(ratio[i]):.3e}")
    assert bool((err <= t).all()), f"{name}: {int((err > t).sum())} elements over their bound; worst error {float(err[i]):.3e} against {float(t[i]):.3e}"


def same_bits(a, b):
    return a.flat.dtype == b.flat.dtype and torch.equal(a.view.float().nan_to_num(nan=12345.0), b.view.float().nan_to_num(nan=12345.0))


def run_case(id):
    c = gi.BY_ID[id]
    for family in gi.families(c):
        dev, exp = device_inputs(id, family), gi.expected(id, family)
        o = launch(c, dev, family, c.ydt, dev["b"])
        chk = dict(o)
        if "planes" in exp:                                          # round family of the planes kernels: hi + lo as one value
            hi, lo = chk.pop("hi"), chk.pop("lo")
            assert hi.front_untouched() and lo.front_untouched()
            assert torch.equal(torch.isnan(hi.view), torch.isnan(lo.view)), "the hi and the lo plane are not written at the same elements"
            chk["planes"] = Buf(c.M + gi.GUARD_BACK, c.N, torch.float32)
            chk["planes"].view.copy_(hi.view.float() + lo.view.float())
        if c.ydt == "bf16":                                          # the same launch with f32 rows
            o32 = launch(c, dev, family, "f32", dev["b"])
            chk["y32"] = o32["y"]
            assert same_bits(o["y"], _as_bf16(o32["y"])), "bf16 rows != f32 rows .bfloat16()"
            for k in ("hi", "lo", "p16"):
                assert k not in o or same_bits(o[k], o32[k]), f"{k} depends on the type of the rows"
        assert set(chk) == set(exp), (set(chk), set(exp))
        for k, (img, tol) in exp.items():
            compare(f"{id} {family} {k}", chk[k], img, tol)
        if dev["b_other"] is not None:
            ob = launch(c, dev, family, c.ydt, dev["b_other"])
            for k, buf in ob.items():
                assert same_bits(buf, o[k]), f"{k}: the {dev['b_other'].dtype} bias gives other bits than the {dev['b'].dtype} bias"
        yield family, o, dev


def _as_bf16(buf):
    b = Buf(buf.view.shape[0], buf.view.shape[1], torch.bfloat16)
    b.view.copy_(buf.view.bfloat16())
    return b


@pytest.mark.parametrize("id", IDS["gemm"])
def test_readout_gemm_images(id):
    for _ in run_case(id):
        pass


@pytest.mark.parametrize("id", IDS["planes"])
def test_planes_gemm_images(id):
    for _ in run_case(id):
        pass


def row_line(c):
    """Whether r16_build sends the case's launch through the row-line epilogue (and a whole 64-column tile exists to take it)."""
    one16 = (c.out == "plane" and c.p_off % 8 == 0) or (c.out == "y" and c.ydt == "bf16" and c.y_off % 8 == 0 and c.ld % 8 == 0)
    return c.N % 8 == 0 and c.N >= 64 and one16


@pytest.mark.parametrize("id", IDS["r16"])
def test_readout16_gemm_images(id):
    c = gi.BY_ID[id]
    for family, o, dev in run_case(id):
        if row_line(c):
            # the same launch with the output 8 bytes off a 16-byte base: the general epilogue, the same bits
            g = launch(c, dev, family, c.ydt, dev["b"], y_off=4, p_off=4)
            for k, buf in g.items():
                assert buf.view.data_ptr() % 16 == 8 and buf.front_untouched()
                assert same_bits(buf, o[k]), f"{k}: the general epilogue gives other bits than the row-line epilogue"


def test_the_r16_table_takes_both_epilogues():
    r = [c for c in gi.CASES if c.kernel == "r16"]
    assert {c.out for c in r if row_line(c)} == {"plane", "y"} and any(not row_line(c) and c.N % 8 == 0 and (c.p_off or c.y_off) for c in r)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _off16(t, elems=1):
    """A copy of t that starts `elems` elements into its allocation."""
    hold = torch.zeros(t.numel() + elems, dtype=t.dtype, device="cuda")
    hold[elems:] = t.reshape(-1)
    return hold[elems:].view(t.shape)


@pytest.mark.parametrize("kernel", ["gemm", "planes", "r16"])
def test_refusals_write_nothing(kernel):
    M, N, K = 5, 8, 64
    g = torch.Generator().manual_seed(3)
    dt = torch.float16 if kernel == "r16" else torch.bfloat16
    a32 = torch.randn(M, K + 32, generator=g).cuda()
    w = torch.randn(N, K + 32, generator=g).cuda().to(dt)
    b = torch.randn(N, generator=g).cuda().bfloat16()
    cut = lambda t: t[:, :K].contiguous()
    act_of = {"gemm": lambda t: t, "planes": lambda t: t.bfloat16(), "r16": lambda t: t.half()}[kernel]

    def call(a, wt, y, row0=0, planes=None):
        if kernel == "gemm":
            nv.readout_gemm(a, wt, b, y, row0=row0)
        elif kernel == "planes":
            nv.planes_gemm(a, a, wt, b, out_hi=planes and planes[0].view[:M], out_lo=planes and planes[1].view[:M], y=y, row0=row0)
        else:
            nv.readout16_gemm(a, wt, b, out_f16=planes and planes[0].view[:M], y=y, row0=row0)

    a_ok, w_ok = act_of(cut(a32)), cut(w)
    bad = {"K % 64": dict(a=act_of(a32), wt=w), "ldy < N": dict(a=a_ok, wt=w_ok, ld=N - 1), "row0 < 0": dict(a=a_ok, wt=w_ok, row0=-1),
           "activation base": dict(a=_off16(a_ok), wt=w_ok), "weight base": dict(a=a_ok, wt=_off16(w_ok))}
    for what, kw in bad.items():
        y = Buf(M + 2, kw.get("ld", N), torch.float32)
        planes = None if kernel == "gemm" else [Buf(M + 2, N, dt), Buf(M + 2, N, dt)]
        assert what not in ("activation base", "weight base") or (kw["a"].data_ptr() % 16 or kw["wt"].data_ptr() % 16)
        with pytest.raises(nv.HicomNativeError):
            call(kw["a"], kw["wt"], y.view, kw.get("row0", 0), planes)
        torch.cuda.synchronize()
        assert y.untouched() and all(p.untouched() for p in planes or ()), what
    # no output at all
    if kernel == "gemm":
        status = nv.lib().hicom_readout_gemm_fwd(a_ok.data_ptr(), w_ok.data_ptr(), b.data_ptr(), nv.DT_BF16, M, N, K, nv.ACT_NONE, None, nv.DT_F32, N, 0, 0,
                                                 torch.cuda.current_stream().cuda_stream)
        assert status != 0
    else:
        with pytest.raises(nv.HicomNativeError):
            call(a_ok, w_ok, None)
    # ... and the accepted form of the same call writes
    y = Buf(M + 2, N, torch.float32)
    call(a_ok, w_ok, y.view, 0, None if kernel == "gemm" else [Buf(M + 2, N, dt), Buf(M + 2, N, dt)])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y.view[:M]).all()) and bool(torch.isnan(y.view[M:]).all()) and y.front_untouched()
