"""The segmented scores kernel on the GPU: hicom_head_guide_fold_many_fwd + hicom_head_scores_ragged_fwd
(csrc/head_scores.hip) on the mixes of tests/ragged_head_scores_inputs.py -- N (5, 36, 53, 729) with Q (1, 3, 17, 2), the step's MIX6
N (36, 144, 36, 288, 36) with Q (1, 3, 5, 2, 4), N (9, 9) with Q (32, 1), all at inter 200, and the pitched plane (inter 4304) with one
item of 144 tokens and with two items.

Fold    every row of the many-row fold against hicom_head_guide_fold_fwd on the item's guides, bit for bit; the pad rows zero, scale 1, c 0.
Scores  against hicom_head_scores_multi_fwd on each item's slice of the same operands with the item's rows of the same U planes copied
        out, bit for bit (the same tiling per item, the same arithmetic per row); against the float64 reference per item at the hs_tol
        bound on the item's operands (tests/test_ragged_head_scores_power.py: a kernel that takes the previous item's guide rows, lets a
        tile run on into the next item, stores item 0's Q rows for every item or indexes c by the guide's number misses it by a factor of
        4 at least on every mix where the fault is defined).  The logits [max Q_i][q_stride = sum N_i + 3] lie between two guard rows, all
        pre-filled with one NaN bit pattern: every cell with q >= Q_i, every cell behind sum N_i and both guard rows keep the pattern.  hid
        carries 30000 in its pad columns and its pitch gap: the result equals, bit for bit, that on zeros there.
B = 1   through the ragged entry equals the multi entry bit for bit.
Every mix runs once per process; the checks share the result.  Each prints `RAGGED_HEAD_SCORES <mix> item <i> err=... bound=... ratio=...`
before it asserts.

Measured on an MI355X: errors <= 2.2e-5 (inter 200) and <= 9.9e-5 (inter 4304), at most 2.4e-4 of the bound; every bit-for-bit comparison
holds."""
import functools
from types import SimpleNamespace

import pytest
import torch

import ragged_head_scores_inputs as rh
from gpu_util import DEV
from hicom_amd import encoder
from hicom_amd import native as nv

pytestmark = pytest.mark.gpu
PATTERN = 0x7FC01234                     # a quiet NaN with a payload: `untouched` is a comparison of bits
IDS = [m.id for m in rh.MIXES]


def nan_fill(*shape):
    return torch.full(shape, PATTERN, dtype=torch.int32, device=DEV).view(torch.float32)


def untouched(t):
    return bool((t.contiguous().view(torch.int32) == PATTERN).all())


def tables(N, Q):
    items, tile_item = encoder.ragged_score_tables(N, Q)
    return torch.from_numpy(items).to(DEV), torch.from_numpy(tile_item).to(DEV)


def scores(b, hid, planes, tabs):
    """The ragged kernel into a guarded, padded buffer: (whole buffer, the [max Q_i, stride] rows between the guards)."""
    buf = nan_fill(max(b.mix.Q) + 2, b.T + 3)
    out = buf[1:-1]
    nv.head_scores_ragged(b.dx, hid, b.kpad, b.dg, *planes, *tabs, max(b.mix.Q), out)
    torch.cuda.synchronize()
    return buf, out


@functools.lru_cache(maxsize=None)
def run(mix):
    b = rh.build(mix)
    dev = lambda t: t.to(DEV).contiguous()
    r = SimpleNamespace(mix=mix, kpad=b.kpad, T=b.T, tok0=b.tok0, pair0=b.pair0, dx=dev(b.x), dhid=dev(b.hid), dclean=dev(b.clean), dg=dev(b.guides),
                        dw2=dev(b.w2), db2=dev(b.b2))
    r.ldu = nv.head_fold_ldu(b.kpad)
    r.planes = nv.head_guide_fold_many(r.dw2, r.db2, r.dg, r.ldu)
    r.tabs = tables(mix.N, mix.Q)
    r.buf, r.out = scores(r, r.dhid, r.planes, r.tabs)
    return r


def item_slices(r, i):
    t, p = r.tok0[i], r.pair0[i]
    return slice(t, t + r.mix.N[i]), slice(p, p + r.mix.Q[i])


@pytest.mark.parametrize("mix", rh.MIXES, ids=IDS)
def test_fold_many_equals_the_fold_per_item_bit_for_bit(mix):
    r = run(mix)
    u_hi, u_lo, u_scale, c = r.planes
    M = sum(mix.Q)
    rows = (M + 15) // 16 * 16 + 32
    assert tuple(u_hi.shape) == tuple(u_lo.shape) == (rows, r.ldu) and tuple(u_scale.shape) == tuple(c.shape) == (rows,)
    for i, q in enumerate(mix.Q):
        _, ps = item_slices(r, i)
        one = nv.head_guide_fold(r.dw2, r.db2, r.dg[ps].contiguous(), r.ldu)
        torch.cuda.synchronize()
        for name, many, single in zip(("u_hi", "u_lo", "u_scale", "c"), r.planes, one):
            assert torch.equal(many[ps], single[:q]), f"{mix.id} item {i}: {name} differs from the single fold"
    assert not bool(u_hi[M:].any()) and not bool(u_lo[M:].any()) and not bool(c[M:].any()) and bool((u_scale[M:] == 1).all()), "pad rows"
    assert not bool(u_hi[:, mix.inter:].any()) and not bool(u_lo[:, mix.inter:].any())


@functools.lru_cache(maxsize=None)
def multi_per_item(mix):
    """hicom_head_scores_multi_fwd on each item's slice of the same operands, the item's rows of the same U planes copied out."""
    r = run(mix)
    outs = []
    for i, q in enumerate(mix.Q):
        ts, ps = item_slices(r, i)
        qpad = (q + 15) // 16 * 16
        own = []
        for plane, fill in zip(r.planes, (0, 0, 1, 0)):
            t = torch.full((qpad,) + tuple(plane.shape[1:]), fill, dtype=plane.dtype, device=DEV)
            t[:q] = plane[ps]
            own.append(t)
        out = nan_fill(q, mix.N[i])
        nv.head_scores_multi(r.dx[ts], r.dhid[ts], r.kpad, r.dg[ps].contiguous(), *own, out)
        outs.append(out)
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("mix", rh.MIXES, ids=IDS)
def test_scores_equal_the_multi_form_per_item_bit_for_bit(mix):
    r = run(mix)
    for i, (q, one) in enumerate(zip(mix.Q, multi_per_item(mix))):
        ts, _ = item_slices(r, i)
        assert bool(torch.isfinite(one).all())
        assert torch.equal(r.out[:q, ts], one), f"{mix.id} item {i}: {int((r.out[:q, ts] != one).sum())} cells differ from the multi form"


@pytest.mark.parametrize("mix", rh.MIXES, ids=IDS)
def test_scores_match_fp64_per_item_and_nothing_else_is_written(mix):
    r = run(mix)
    got = r.out[:, :r.T].cpu()
    for i, (n, q) in enumerate(zip(mix.N, mix.Q)):
        ts, _ = item_slices(r, i)
        cells = got[:q, ts].double()
        assert bool(torch.isfinite(cells).all()), f"{mix.id} item {i}: a cell of its guides was not written"
        err, tol = (cells - rh.item_reference(mix, i)).abs(), rh.item_tol(mix, i)
        ratio = err / tol
        k = int(ratio.argmax())
        print(f"RAGGED_HEAD_SCORES {mix.id} item {i} (N={n} Q={q}) err={float(err.max()):.3e} bound={float(tol.reshape(-1)[k]):.3e} "
              f"ratio={float(ratio.reshape(-1)[k]):.3e}")
        assert bool((err <= tol).all()), f"{mix.id} item {i}: error {float(err.reshape(-1)[k]):.3e} over its bound {float(tol.reshape(-1)[k]):.3e}"
        assert untouched(r.out[q:, ts]), f"{mix.id} item {i}: a cell with q >= Q_i was written"
    assert rh.worst(mix, got) <= 1.0
    assert untouched(r.out[:, r.T:]), "a cell behind sum N_i was written"
    assert untouched(r.buf[0]) and untouched(r.buf[-1]), "a guard row was written"


@pytest.mark.parametrize("mix", rh.MIXES, ids=IDS)
def test_the_sentinel_does_not_move_a_bit(mix):
    """30000 in hid's pad columns and pitch gap against zeros there."""
    r = run(mix)
    _, clean = scores(r, r.dclean, r.planes, r.tabs)
    for i, q in enumerate(mix.Q):
        ts, _ = item_slices(r, i)
        assert torch.equal(r.out[:q, ts], clean[:q, ts]), f"{mix.id} item {i}"


SINGLE = [("n4", 3), ("n4", 2), ("n4", 0), ("q32", 0), ("mix6", 3), ("pitched", 0)]       # N 729 / 53 / 5 / 9 / 288 / 144, Q 2 / 17 / 1 / 32 / 2 / 3


@pytest.mark.parametrize("mix_id,i", SINGLE, ids=[f"{m}-item{i}" for m, i in SINGLE])
def test_one_item_through_the_ragged_entry_equals_the_multi_entry(mix_id, i):
    """B = 1: the tiling is the multi form's.  Both entries on the same operands and the same planes (hicom_head_guide_fold_fwd: the 16 or
    32 rows the ragged kernel reads from pair 0 are the rows the multi kernel reads)."""
    mix = rh.BY_ID[mix_id]
    r = run(mix)
    ts, ps = item_slices(r, i)
    n, q = mix.N[i], mix.Q[i]
    x, hid, g = r.dx[ts], r.dhid[ts], r.dg[ps].contiguous()
    planes = nv.head_guide_fold(r.dw2, r.db2, g, r.ldu)
    a, b = nan_fill(q + 2, n + 3), nan_fill(q + 2, n + 3)
    nv.head_scores_multi(x, hid, r.kpad, g, *planes, a[1:-1])
    nv.head_scores_ragged(x, hid, r.kpad, g, *planes, *tables((n,), (q,)), q, b[1:-1])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a[1:-1, :n]).all())
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{mix_id} item {i}: the two entries differ"
    assert torch.equal(b[1:-1, :n], r.out[:q, ts]), "the item alone differs from the item in its batch"
