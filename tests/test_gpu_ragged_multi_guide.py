"""HIComProjector.forward_ragged_multi_guide (GPU): B items of unequal length, item i with its own Q_i instructions, in one native call
(csrc/ragged_multi_guide.hip) against the CPU oracle run once per (item, guide) pair, plus what only this step can break: pairs that
alias one item's tokens, remainder groups of the local kernel, part-filled 32-row passes of the two-row-group stream, the slot order the
merge walks, isolation between the guides of an item and between items, plans, refusals.

Cases and input families: tests/ragged_multi_guide_inputs.py (MIX6, MIX9; `edge`, one `edge_outlier`, one `item_scales` case);
tests/test_ragged_multi_guide_power.py shows on the oracle alone that a wrong softmax moves every region of every pair by >= 4 bars.
Bar: 1e-3 max-abs on the fp32 output per pair and per region (local rows, newline rows, global rows), HEAVY_REL x max |oracle out| under
`edge_outlier`; 2e-3 against the sibling steps and forward() (each side is held to 1e-3).  The test prints every figure before it asserts.
Measured on an MI355X: `edge` local 3.7e-5 .. 1.8e-4, global 8.3e-7 .. 2.3e-6 (newline rows 0); hidden 896 local 2.2e-4 .. 6.5e-4, global
5.2e-6 .. 8.1e-6; `edge_outlier` local 3.0e-4 .. 9.7e-4 of bars of 2.0e-3 .. 3.3e-3, global 3.0e-6 .. 6.6e-6; `item_scales` local 8.8e-5 ..
7.2e-4, global 9.2e-7 .. 8.1e-6.  All Q_i = 1 against forward_ragged: 0 (bit-identical); B = 1 against forward_multi_guide 2.4e-6; every pair
against forward() 9.8e-7 .. 1.1e-4."""
import numpy as np
import pytest
import torch

import hicom_amd
import many_item_inputs as mi
import ragged_multi_guide_inputs as ri
from gpu_util import build_module, dev_bf16
from hicom_amd import ragged_multi_guide as rmg
from hicom_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-3
D = ri.D
NG = ri.NG
STORE = "_ragged_multi_guide_plans"


def tensors(c, ff=None, g=None):
    ff = c.ff if ff is None else ff
    g = c.g if g is None else g
    fe = dev_bf16(np.concatenate(c.fe)) if c.entry.with_fe else None
    return dev_bf16(np.concatenate(ff)), fe, dev_bf16(np.concatenate(g))


def run(c, m=None, ff=None, g=None, splits=None, counts=None, modals=None, fe=None, chunks="entry"):
    m = m or build_module(c)
    tff, tfe, tg = tensors(c, ff, g)
    if fe is not None:
        tfe = dev_bf16(np.concatenate(fe))
    kw = {"chunks": c.entry.chunks if chunks == "entry" else chunks}
    with torch.no_grad():
        out = m.forward_ragged_multi_guide(tff, tfe, tg, splits or c.splits, counts or c.counts, modals or c.modals, dev_bf16(c.newline), **kw)
    torch.cuda.synchronize()
    return out


def check_views(out, counts):
    """The B outputs are [Q_i, rows_i, hidden] views that tile one storage in item-major, then guide-major order."""
    hidden, off = out[0].shape[2], 0
    for i, o in enumerate(out):
        assert o.dim() == 3 and o.shape[0] == counts[i] and o.is_contiguous()
        assert o.untyped_storage().data_ptr() == out[0].untyped_storage().data_ptr() and o.storage_offset() == off
        off += o.numel()
    assert out[0].untyped_storage().nbytes() == off * out[0].element_size() and hidden == out[-1].shape[2]


def check_against_oracle(id, chunks="entry"):
    c, want = ri.build(id), ri.oracle_outputs(id)
    out = run(c, chunks=chunks)
    assert isinstance(out, list) and len(out) == c.B
    check_views(out, c.counts)
    bad = []
    for (i, q), w in want.items():
        got = out[i][q]
        assert got.dtype == torch.float32 and tuple(got.shape) == w.shape, (i, q, tuple(got.shape), w.shape)
        assert torch.equal(got[-NG:], got[-1:].expand(NG, -1)), f"pair ({i}, {q}): the {NG} global rows differ"
        bad += ri.check_pair(c, f"pair ({i}, {q})", got.cpu().numpy(), w, i)
    assert not bad, f"{id}: " + "; ".join(bad)
    return c, out


# ---- parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", [e.id for e in ri.CASES])
def test_input_families_per_pair_and_region_against_oracle(id):
    """Every case of the table: MIX6 (remainder groups of 1, 2 and 3, Q = 5 across the local group and the 32-row pass, masked tail tiles,
    a 1-frame "video") with chunks None / 1 / 3 / 18, with image_newline in both positions, without frames_embed, at hidden 896, under
    `edge_outlier`; MIX9 (Q = 8: three passes, the last part-filled; 81 tokens: a tail tile) under `edge` and `item_scales`."""
    c, out = check_against_oracle(id)
    if c.newline is not None:
        nl = torch.from_numpy(c.newline).cuda()
        seen = 0
        for i in range(c.B):
            for r in ri.regions(c, i, out[i].shape[1])["newline"]:
                assert torch.equal(out[i][:, r], nl.expand(c.counts[i], -1)), f"item {i} row {r}: not the newline vector"      # bit for bit
                seen += 1
        assert seen >= 2 and (c.entry.newline != "grid" or seen > 2)          # the images always; under "grid" the clips as well


@pytest.mark.parametrize("chunks", [None, 1, 3, 18])
def test_chunks_on_the_flat_edges(chunks):
    """The `edge` inputs of MIX6 (no chunk-boundary spikes) under every chunk count: the division must not show."""
    check_against_oracle("rmg_mix6", chunks=chunks)


# ---- reductions to the sibling steps ------------------------------------------------------------------------------------------------
def test_single_guides_reduce_to_forward_ragged():
    c = ri.build("rmg_mix6")
    m = build_module(c)
    g0 = [g[:1] for g in c.g]
    out = run(c, m, g=g0, counts=[1] * c.B, chunks=3)
    tff, tfe, tg = tensors(c, g=g0)
    with torch.no_grad():
        rag = m.forward_ragged(tff, tfe, tg, c.splits, c.modals, chunks=3)
    diffs = [float((out[i][0] - rag[i]).abs().max()) for i in range(c.B)]
    print(f"all Q_i = 1 vs forward_ragged: max-abs per item {['%.3e' % d for d in diffs]}")
    assert max(diffs) <= 2 * TOL


def test_one_item_reduces_to_forward_multi_guide():
    c = ri.build("rmg_mix6")
    m = build_module(c)
    i = 2                                           # the 1-frame "video" with five guides
    out = run(c, m, ff=[c.ff[i]], fe=[c.fe[i]], g=[c.g[i]], splits=[c.splits[i]], counts=[c.counts[i]], modals=[c.modals[i]])
    with torch.no_grad():
        mg = m.forward_multi_guide(dev_bf16(c.ff[i]), dev_bf16(c.fe[i]), dev_bf16(c.g[i]), c.modals[i])
    d = float((out[0] - mg).abs().max())
    print(f"B = 1, Q = 5 vs forward_multi_guide: max-abs {d:.3e}")
    assert out[0].shape == mg.shape and d <= 2 * TOL


@pytest.mark.parametrize("id", ["rmg_mix6_newline_grid", "rmg_mix9"])
def test_agrees_with_forward_per_pair(id):
    c = ri.build(id)
    m = build_module(c)
    out = run(c, m)
    diffs = []
    with torch.no_grad():
        for i, q in c.pairs:
            one = m(dev_bf16(c.ff[i]), dev_bf16(c.fe[i]), dev_bf16(c.g[i][q]), c.modals[i], dev_bf16(c.newline))
            assert one.shape == out[i][q].shape and one.dtype == out[i].dtype
            diffs.append(float((one - out[i][q]).abs().max()))
    print(f"{id} vs forward(): max-abs per pair {['%.3e' % d for d in diffs]}")
    assert max(diffs) <= 2 * TOL


# ---- bit-for-bit invariances inside the step, chunks fixed ---------------------------------------------------------------------------
CH = 3


def intruder(tag, scale=4.0):
    return synth.synth_inputs(1, 3, 3, D, tag=f"{ri.TAG}:{tag}")["g"] * scale


def test_permuted_guides_permute_an_items_outputs():
    c = ri.build("rmg_mix6")
    m = build_module(c)
    base = [o.clone() for o in run(c, m, chunks=CH)]
    perm = [4, 2, 0, 3, 1]                          # item 2: guide 4 leaves the group of one and the second pass
    g = list(c.g)
    g[2] = c.g[2][perm]
    out = run(c, m, g=g, chunks=CH)
    for k, q in enumerate(perm):
        assert torch.equal(out[2][k], base[2][q]), f"position {k} (guide {q})"
    for i in (0, 1, 3, 4):
        assert torch.equal(out[i], base[i]), f"item {i} moved"


def test_a_replaced_or_repeated_guide_leaves_its_neighbours():
    c = ri.build("rmg_mix6")
    m = build_module(c)
    base = [o.clone() for o in run(c, m, chunks=CH)]
    g = [x.copy() for x in c.g]
    g[2][1] = intruder("intruder")                  # other softmax maxima inside the shared 32-row pass
    g[4][3] = g[4][0]                               # the same guide twice in one item (another local group slot, another row group)
    out = run(c, m, g=g, chunks=CH)
    for i in range(c.B):
        for q in range(c.counts[i]):
            if (i, q) in ((2, 1), (4, 3)):
                assert not torch.equal(out[i][q], base[i][q])
            else:
                assert torch.equal(out[i][q], base[i][q]), f"pair ({i}, {q}) moved"
    assert torch.equal(out[4][3], out[4][0])


def test_other_items_and_an_appended_item_leave_a_pair():
    c = ri.build("rmg_mix6")
    m = build_module(c)
    base = [o.clone() for o in run(c, m, chunks=CH)]
    ff, g = list(c.ff), [x.copy() for x in c.g]
    ff[1] = ff[1] * np.float32(4.0)                 # item 1: other tokens, other running maxima
    g[3][:] = intruder("intruder2")                 # item 3: other guides
    out = run(c, m, ff=ff, g=g, chunks=CH)
    for i in (0, 2, 4):
        assert torch.equal(out[i], base[i]), f"item {i} moved"
    assert not torch.equal(out[1], base[1]) and not torch.equal(out[3], base[3])
    more = run(c, m, ff=c.ff + [c.ff[1]], fe=c.fe + [c.fe[1]], g=c.g + [c.g[2][:2]], splits=c.splits + [4], counts=c.counts + [2],
               modals=c.modals + ["video"], chunks=CH)
    for i in range(c.B):
        assert torch.equal(more[i], base[i]), f"item {i} moved when an item was appended"


def test_two_calls_and_a_side_stream_give_the_same_bits():
    c = ri.build("rmg_mix9")
    m = build_module(c)
    first = [o.clone() for o in run(c, m)]
    second = run(c, m)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert len(m.__dict__[STORE]) == 1 and next(iter(m.__dict__[STORE].values())).hits == 2          # the second call hit the cached plan
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run(c, m)
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, third))
    assert len(m.__dict__[STORE]) == 2                                                              # the stream is part of the key


@pytest.mark.parametrize("id,chunks", [("rmg_mix6", None), ("rmg_mix6", 3), ("rmg_mix9", 18)])
def test_device_tables_equal_the_host_mirror(id, chunks):
    c = ri.build(id)
    m = build_module(c)
    run(c, m, chunks=chunks)
    plan, = m.__dict__[STORE].values()
    want = rmg.table_image(plan.tables)
    got = plan.ws[:want.size * 4].cpu().numpy().view(np.int32)
    assert np.array_equal(got, want)
    t = plan.tables
    assert len(t.units) == sum(p * n for p, n in zip(t.passes, t.chunks)) and t.slots == 2 * len(t.units)
    if chunks is None:
        assert len(t.units) <= 2 * torch.cuda.get_device_properties(0).multi_processor_count + sum(t.passes)


# ---- plans ----------------------------------------------------------------------------------------------------------------------------
def test_plan_key_weight_update_and_allocations():
    """guide_counts is part of the key; an in-place weight update (x -1 on the local readout's second Linear, exact in bf16) is followed
    under the same plan; after warm-up a call allocates its output and nothing token-sized."""
    c = ri.build("rmg_mix6")
    m = build_module(c)
    tff, tfe, tg = tensors(c)
    with torch.no_grad():
        before = [o.clone() for o in m.forward_ragged_multi_guide(tff, tfe, tg, c.splits, c.counts, c.modals)]
        m.forward_ragged_multi_guide(tff, tfe, tg[:c.B * 3].contiguous(), c.splits, [3] * c.B, c.modals)
        assert len(m.__dict__[STORE]) == 2
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        out = m.forward_ragged_multi_guide(tff, tfe, tg, c.splits, c.counts, c.modals)
        grown = torch.cuda.memory_allocated() - base
        out_bytes = sum(o.numel() for o in out) * 4
        print(f"allocated by a warm call: {grown} bytes (output {out_bytes}, tokens {tff.numel() * 2})")
        assert out_bytes <= grown < out_bytes + 4096 and grown < tff.numel() * 2
        del out
        m.local_compressor.readout[2].weight.data.mul_(-1.0)
        after = m.forward_ragged_multi_guide(tff, tfe, tg, c.splits, c.counts, c.modals)
    torch.cuda.synchronize()
    plans = m.__dict__[STORE]
    assert len(plans) == 2 and next(iter(plans.values())).hits == 3
    flipped = {**c.sd, "local_compressor.readout.2.weight": -c.sd["local_compressor.readout.2.weight"]}
    m2 = build_module(type(c)(**{**vars(c), "sd": flipped}))
    want = run(c, m2, chunks=None)
    for i in range(c.B):
        assert torch.equal(after[i], want[i]), f"item {i}: the plan did not follow the weight update"
        assert not torch.equal(after[i][:, :-NG], before[i][:, :-NG])


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_no_plan():
    c = ri.build("rmg_mix9")
    m = build_module(c)
    ff, fe, g = tensors(c)
    call = lambda mod, *a, **k: mod.forward_ragged_multi_guide(*a, **k)
    ok = (c.splits, c.counts, c.modals)
    modules = [m]
    with torch.no_grad():
        for over in ({"mm_projector_type": "local43_adaptkv_global32"}, {"use_guide": "coarse"}):
            cfg = type(c.cfg)(**{**vars(c.cfg), **over})
            other = hicom_amd.build_vision_projector(cfg).to(torch.bfloat16).cuda().eval()
            modules.append(other)
            with pytest.raises(NotImplementedError, match="plain release recipe"):
                call(other, ff, fe, g, *ok)
        half = hicom_amd.build_vision_projector(c.cfg).to(torch.float16).cuda().eval()
        modules.append(half)
        with pytest.raises(NotImplementedError, match="float16"):
            call(half, ff.half(), fe.half(), g.half(), *ok)
        with pytest.raises(NotImplementedError):
            call(m, ff.half(), fe.half(), g.half(), *ok)                    # fp16 tokens into a bf16 module
        with pytest.raises(NotImplementedError):
            call(m, {"base": None, "patch": ff[0]}, None, g, *ok)
        with pytest.raises(ValueError, match=r"\[sum Q_i, E\]"):
            call(m, ff, fe, g[:-1].contiguous(), *ok)                       # sum(guide_counts) != guide_embeds.shape[0]
        with pytest.raises(ValueError, match="guide counts for"):
            call(m, ff, fe, g, c.splits, c.counts + [1], c.modals)
        for bad in ([0, 12], [33, 8]):
            with pytest.raises(ValueError, match="Q_i <= 32"):
                call(m, ff, fe, g, c.splits, bad, c.modals)
        with pytest.raises(ValueError, match="split_sizes"):
            call(m, ff, fe, g, [1, 3], c.counts, c.modals)
        odd = dev_bf16(np.zeros((5, 7, 7, D), np.float32))                  # 7 is no multiple of the 3 x 3 window
        with pytest.raises(NotImplementedError, match="partition"):
            call(m, odd, odd, g, *ok)
    m.requires_grad_(True)
    with pytest.raises(RuntimeError, match="autograd"):
        call(m, ff, fe, g, *ok)
    m.requires_grad_(False)
    for mod in modules:
        assert not mod.__dict__.get(STORE), "a refusal left a plan behind"
    out = call(m, ff, fe, g, *ok)
    assert out[0].grad_fn is None and len(m.__dict__[STORE]) == 1
    torch.cuda.synchronize()
