"""HIComProjector.forward_prepared_many (GPU): B prepared clips, clip i with its own Q_i instructions, in one native call
(csrc/ragged_multi_guide.hip: clips_local_kernel, clips_local_adapt_kernel, clips_stream_kernel behind hicom_compressor_clips_multiguide_fwd)
against the CPU oracle run once per (clip, guide) pair, plus what only this step can break: the pointer table (a wrong column, a stale
row, a table rewritten under a running call), clips at fresh addresses under one plan, the window groups and remainders over clips that
live apart, staleness per clip, refusals.

Cases and input families: tests/prepared_many_inputs.py (MIX6, MIX9; the three adaptor recipes and the plain one at hidden 896);
tests/test_prepared_many_power.py shows on the oracle alone that a wrong softmax moves every region of every pair by >= 4 bars.  Every
clip is its OWN allocation, never a view of a stack.  Bar: 1e-3 max-abs on the fp32 output per pair and per region (local rows, newline
rows, global rows), HEAVY_REL x max |oracle out| under `edge_outlier`; 2e-3 against the sibling steps and forward() (each side is held to
1e-3 by its own test).  The tests print every figure before they assert.
Measured on an MI355X: `edge` local 1.2e-4 .. 7.1e-4, global 5.1e-6 .. 7.6e-6, newline rows 0; `edge_outlier` local 1.3e-3 .. 2.1e-3 of bars
of 4.6e-3 .. 5.5e-3, global 1.7e-5 .. 2.6e-5; the plain recipe local 2.8e-4 .. 6.3e-4.  B = 1 against forward_prepared 6.0e-6 / 7.5e-6; all
Q_i = 1 against forward_ragged 0; every pair against forward() 5.8e-6 .. 1.4e-4."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import many_item_inputs as mi
import prepared_many_inputs as pmi
from gpu_util import build_module, dev_bf16
from hicom_amd import prepared, synth

pytestmark = pytest.mark.gpu

TOL = 1e-3
D, NG = pmi.D, pmi.NG
STORE = "_prepared_many_plans"
BASE = "pm_mix6_adaptkv"
CH = 3


def clips_of(c, m, ff=None, idx=None):
    """prepare_clip per clip, every clip from tensors of its own."""
    ff = c.ff if ff is None else ff
    with torch.no_grad():
        return [m.prepare_clip(dev_bf16(ff[i]), dev_bf16(c.fe[i]), c.modals[i]) for i in (range(c.B) if idx is None else idx)]


def guides_of(g):
    return dev_bf16(np.concatenate(g))


def run(c, m, clips, g=None, counts=None, chunks="entry", sync=True):
    kw = {"chunks": c.entry.chunks if chunks == "entry" else chunks}
    with torch.no_grad():
        out = m.forward_prepared_many(clips, guides_of(c.g if g is None else g), c.counts if counts is None else counts, dev_bf16(c.newline), **kw)
    if sync:
        torch.cuda.synchronize()
    return out


def keep(out):
    return [o.clone() for o in out]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def check_views(out, counts):
    """The B outputs are [Q_i, rows_i, hidden] views that tile one storage in item-major, then guide-major order."""
    hidden, off = out[0].shape[2], 0
    for i, o in enumerate(out):
        assert o.dim() == 3 and o.shape[0] == counts[i] and o.is_contiguous()
        assert o.untyped_storage().data_ptr() == out[0].untyped_storage().data_ptr() and o.storage_offset() == off
        off += o.numel()
    assert out[0].untyped_storage().nbytes() == off * out[0].element_size() and hidden == out[-1].shape[2]


def check_pairs(c, out, wants, what=""):
    bad = []
    for (i, q), w in wants.items():
        got = out[i][q]
        assert got.dtype == torch.float32 and tuple(got.shape) == w.shape, (i, q, tuple(got.shape), w.shape)
        assert torch.equal(got[-NG:], got[-1:].expand(NG, -1)), f"pair ({i}, {q}): the {NG} global rows differ"
        bad += pmi.check_pair(c, f"{what}pair ({i}, {q})", got.cpu().numpy(), w, i)
    return bad


# ---- 1: parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", [e.id for e in pmi.CASES])
def test_parity_per_pair_and_region_against_oracle(id):
    c, wants = pmi.build(id), pmi.oracle_outputs(id)
    m = build_module(c)
    clips = clips_of(c, m)
    lc = m.local_compressor
    for clip in clips:
        assert (clip.y_k is not None) == bool(lc.adapt_k) and (clip.y_v is not None) == bool(lc.adapt_v)
    assert len({clip.ff.untyped_storage().data_ptr() for clip in clips}) == c.B               # every clip its own allocation
    out = run(c, m, clips)
    assert isinstance(out, list) and len(out) == c.B
    check_views(out, c.counts)
    bad = check_pairs(c, out, wants)
    assert not bad, f"{id}: " + "; ".join(bad)
    if c.newline is not None:
        nl = torch.from_numpy(c.newline).cuda()
        seen = 0
        for i in range(c.B):
            for r in pmi.regions(c, i, out[i].shape[1])["newline"]:
                assert torch.equal(out[i][:, r], nl.expand(c.counts[i], -1)), f"clip {i} row {r}: not the newline vector"      # bit for bit
                seen += 1
        assert seen > 2                                                                         # under "grid" the clips as well as the images


# ---- 2: a plain module: the kernels of forward_ragged_multi_guide behind another address source ---------------------------------------
@pytest.mark.parametrize("chunks", [CH, None])
def test_plain_module_has_the_bits_of_forward_ragged_multi_guide(chunks):
    c = pmi.build("pm_mix6_plain")
    m = build_module(c)
    clips = clips_of(c, m)
    assert all(clip.y_k is None and clip.y_v is None and clip.nbytes == 0 for clip in clips)
    out = run(c, m, clips, chunks=chunks)
    with torch.no_grad():
        want = m.forward_ragged_multi_guide(dev_bf16(np.concatenate(c.ff)), dev_bf16(np.concatenate(c.fe)), guides_of(c.g), c.frames, c.counts, c.modals,
                                            chunks=chunks)
    torch.cuda.synchronize()
    for i in range(c.B):
        assert out[i].shape == want[i].shape and torch.equal(out[i], want[i]), f"clip {i}"
    assert len(m.__dict__[STORE]) == 1 and len(m.__dict__["_ragged_multi_guide_plans"]) == 1


# ---- 3: the sibling steps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [2, 3])
def test_one_clip_agrees_with_forward_prepared(i):
    """B = 1: the 1-frame "video" with five guides (a full group and a remainder of one), the 8-frame clip with two."""
    c = pmi.build(BASE)
    m = build_module(c)
    clip, = clips_of(c, m, idx=[i])
    out = run(c, m, [clip], g=[c.g[i]], counts=[c.counts[i]])
    with torch.no_grad():
        one = m.forward_prepared(clip, dev_bf16(c.g[i]))
    torch.cuda.synchronize()
    d = float((out[0] - one).abs().max())
    print(f"B = 1 (clip {i}, Q = {c.counts[i]}) vs forward_prepared: max-abs {d:.3e}")
    assert out[0].shape == one.shape and d <= 2 * TOL


def test_single_guides_agree_with_forward_ragged_on_the_stacked_tokens():
    c = pmi.build(BASE)
    m = build_module(c)
    g0 = [g[:1] for g in c.g]
    out = run(c, m, clips_of(c, m), g=g0, counts=[1] * c.B, chunks=CH)
    with torch.no_grad():
        rag = m.forward_ragged(dev_bf16(np.concatenate(c.ff)), dev_bf16(np.concatenate(c.fe)), guides_of(g0), c.frames, c.modals, chunks=CH)
    torch.cuda.synchronize()
    diffs = [float((out[i][0] - rag[i]).abs().max()) for i in range(c.B)]
    print(f"all Q_i = 1 vs forward_ragged (adaptor recipe): max-abs per clip {['%.3e' % d for d in diffs]}")
    assert max(diffs) <= 2 * TOL


def test_every_pair_agrees_with_forward():
    c = pmi.build("pm_mix6_newline_grid")
    m = build_module(c)
    out = run(c, m, clips_of(c, m))
    diffs = []
    with torch.no_grad():
        for i, q in c.pairs:
            one = m(dev_bf16(c.ff[i]), dev_bf16(c.fe[i]), dev_bf16(c.g[i][q]), c.modals[i], dev_bf16(c.newline))
            assert one.shape == out[i][q].shape and one.dtype == out[i].dtype
            diffs.append(float((one - out[i][q]).abs().max()))
    print(f"pm_mix6_newline_grid vs forward(): max-abs per pair {['%.3e' % d for d in diffs]}")
    assert max(diffs) <= 2 * TOL


# ---- 4: bit-for-bit invariances, chunks fixed ------------------------------------------------------------------------------------------
def intruder(tag, scale=4.0):
    return synth.synth_inputs(1, 3, 3, D, tag=f"{pmi.TAG}:{tag}")["g"] * scale


def test_permuted_guides_permute_a_clips_outputs():
    c = pmi.build(BASE)
    m = build_module(c)
    clips = clips_of(c, m)
    base = keep(run(c, m, clips, chunks=CH))
    perm = [4, 2, 0, 3, 1]                          # clip 2: guide 4 leaves the group of one and the second pass
    g = list(c.g)
    g[2] = c.g[2][perm]
    out = run(c, m, clips, g=g, chunks=CH)
    for k, q in enumerate(perm):
        assert torch.equal(out[2][k], base[2][q]), f"position {k} (guide {q})"
    for i in (0, 1, 3, 4):
        assert torch.equal(out[i], base[i]), f"clip {i} moved"


def test_a_replaced_guide_leaves_its_neighbours():
    c = pmi.build(BASE)
    m = build_module(c)
    clips = clips_of(c, m)
    base = keep(run(c, m, clips, chunks=CH))
    g = [x.copy() for x in c.g]
    g[2][1] = intruder("intruder")                  # other softmax maxima inside its window group and the shared 32-row pass
    g[4][3] = g[4][0]                               # the same guide twice in one clip
    out = run(c, m, clips, g=g, chunks=CH)
    for i in range(c.B):
        for q in range(c.counts[i]):
            if (i, q) in ((2, 1), (4, 3)):
                assert not torch.equal(out[i][q], base[i][q])
            else:
                assert torch.equal(out[i][q], base[i][q]), f"pair ({i}, {q}) moved"
    assert torch.equal(out[4][3], out[4][0])


def test_other_clips_tokens_an_appended_clip_and_a_permutation_leave_a_pair():
    c = pmi.build(BASE)
    m = build_module(c)
    clips = clips_of(c, m)
    base = keep(run(c, m, clips, chunks=CH))
    ff = list(c.ff)
    ff[1] = ff[1] * np.float32(4.0)                 # clip 1: other tokens, other planes, other running maxima
    other = clips_of(c, m, ff=ff, idx=[1])[0]
    out = run(c, m, [clips[0], other] + clips[2:], chunks=CH)
    for i in (0, 2, 3, 4):
        assert torch.equal(out[i], base[i]), f"clip {i} moved"
    assert not torch.equal(out[1], base[1])
    more = run(c, m, clips + [clips[1]], g=c.g + [c.g[2][:2]], counts=c.counts + [2], chunks=CH)     # (a clip may appear more than once)
    for i in range(c.B):
        assert torch.equal(more[i], base[i]), f"clip {i} moved when a clip was appended"
    order = [3, 0, 4, 2, 1]
    out = run(c, m, [clips[i] for i in order], g=[c.g[i] for i in order], counts=[c.counts[i] for i in order], chunks=CH)
    for k, i in enumerate(order):
        assert torch.equal(out[k], base[i]), f"position {k} (clip {i})"


def moved_copy(clip):
    """The clip with its tokens and planes cloned to fresh addresses."""
    twin = prepared.PreparedClip(clip.proj, clip.ff.clone(), None if clip.fe is None else clip.fe.clone(), clip.modal)
    twin.y_k = None if clip.y_k is None else clip.y_k.clone()
    twin.y_v = None if clip.y_v is None else clip.y_v.clone()
    twin.sig, twin.epoch, twin.mark, twin.event, twin.stream = clip.sig, clip.epoch, clip.mark, clip.event, clip.stream
    return twin


def test_clips_at_fresh_addresses_give_the_same_bits_on_the_same_plan():
    c = pmi.build(BASE)
    m = build_module(c)
    clips = clips_of(c, m)
    base = keep(run(c, m, clips, chunks=CH))
    plan, = m.__dict__[STORE].values()
    torch.cuda.synchronize()
    twins = [moved_copy(clip) for clip in clips]
    for a, b in zip(clips, twins):
        assert a.ff.data_ptr() != b.ff.data_ptr() and a.y_k.data_ptr() != b.y_k.data_ptr() and a.y_v.data_ptr() != b.y_v.data_ptr()
    for k in (0, 2, 5):                             # some, then all of the clips moved
        out = run(c, m, twins[:k] + clips[k:], chunks=CH)
        assert same(out, base), f"{k} clips moved"
    now, = m.__dict__[STORE].values()
    assert now is plan and plan.hits == 4           # the addresses are not in the key: no rebuild


def test_two_calls_and_a_side_stream_give_the_same_bits():
    c = pmi.build("pm_mix9_chunks3")
    m = build_module(c)
    clips = clips_of(c, m)
    first = keep(run(c, m, clips))
    assert same(first, run(c, m, clips))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                   # the clips were made on another stream: their events are waited for on the device
        third = run(c, m, clips, sync=False)
    side.synchronize()
    assert same(first, third)
    assert len(m.__dict__[STORE]) == 2              # the stream is part of the key


# ---- 5: the pointer-table protocol ------------------------------------------------------------------------------------------------------
def test_back_to_back_calls_with_other_clips_each_equal_their_own_call():
    """Two calls on one plan with DIFFERENT clip sets and no synchronisation in between: the second call's table rows must not reach the
    first call's kernels, and the first call's rows must not survive into the second."""
    c = pmi.build(BASE)
    m = build_module(c)
    a = clips_of(c, m)
    b = clips_of(c, m, ff=[np.ascontiguousarray(x[:, ::-1]) for x in c.ff])         # the same shapes, other tokens and planes
    want_a = keep(run(c, m, a, chunks=CH))
    want_b = keep(run(c, m, b, chunks=CH))
    assert not any(torch.equal(x, y) for x, y in zip(want_a, want_b))
    plan, = m.__dict__[STORE].values()
    for first, second, w1, w2 in ((a, b, want_a, want_b), (b, a, want_b, want_a)):
        out1 = run(c, m, first, chunks=CH, sync=False)
        out2 = run(c, m, second, chunks=CH, sync=False)
        out3 = run(c, m, first[:2] + second[2:], chunks=CH, sync=False)
        torch.cuda.synchronize()
        assert same(out1, w1), "the first call saw another call's table"
        assert same(out2, w2), "the second call saw a stale table"
        assert same(out3, w1[:2] + w2[2:])
    assert len(m.__dict__[STORE]) == 1 and next(iter(m.__dict__[STORE].values())) is plan


# ---- 6: plans ------------------------------------------------------------------------------------------------------------------------
def test_plan_hits_weight_refresh_and_allocations():
    c = pmi.build(BASE)
    m = build_module(c)
    a = clips_of(c, m)
    b = clips_of(c, m, ff=[np.ascontiguousarray(x[:, ::-1]) for x in c.ff])
    g = guides_of(c.g)
    with torch.no_grad():
        before = keep(m.forward_prepared_many(a, g, c.counts))
        m.forward_prepared_many(b, g, c.counts)
        plans = m.__dict__[STORE]
        assert len(plans) == 1 and next(iter(plans.values())).hits == 2                 # the same mix, other clips: a hit
        m.forward_prepared_many(a, g[:c.B * 3].contiguous(), [3] * c.B)
        assert len(plans) == 2                                                          # guide_counts is part of the key
        m.local_compressor.readout[2].weight.data.mul_(-1.0)                            # eval mode, through `.data`: exact in bf16
        after = m.forward_prepared_many(a, g, c.counts)
    torch.cuda.synchronize()
    assert len(plans) == 2 and next(iter(plans.values())).hits == 3                     # refreshed in place under the same plan
    flipped = {**c.sd, "local_compressor.readout.2.weight": -c.sd["local_compressor.readout.2.weight"]}
    m2 = build_module(SimpleNamespace(cfg=c.cfg, sd=flipped))
    want = run(c, m2, clips_of(c, m2), chunks=None)
    for i in range(c.B):
        assert torch.equal(after[i], want[i]), f"clip {i}: the plan did not follow the weight update"
        assert not torch.equal(after[i][:, :-NG], before[i][:, :-NG])


def test_a_warm_call_allocates_its_output_and_nothing_token_sized():
    """Two clips, five pairs: the output stays below 1 MiB, where the caching allocator's block is the request rounded up to 512 bytes (as
    in the sibling tests; above it the block sizes are the allocator's business).  The call before it on the plan had other clips, so the
    measured call writes its table."""
    c = pmi.build(BASE)
    m = build_module(c)
    idx = [1, 3]
    a = clips_of(c, m, idx=idx)
    b = clips_of(c, m, ff=[np.ascontiguousarray(x[:, ::-1]) for x in c.ff], idx=idx)
    g, counts = guides_of([c.g[i] for i in idx]), [c.counts[i] for i in idx]
    with torch.no_grad():
        m.forward_prepared_many(a, g, counts)
        m.forward_prepared_many(b, g, counts)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        out = m.forward_prepared_many(a, g, counts)
        grown = torch.cuda.memory_allocated() - base
    torch.cuda.synchronize()
    out_bytes = sum(o.numel() for o in out) * 4
    smallest = min(clip.ff.numel() for clip in a) * 2                                   # the tokens of the smaller clip = one of its planes
    print(f"allocated by a warm call: {grown} bytes (output {out_bytes}, the smaller clip's tokens {smallest})")
    assert out_bytes < (1 << 20) and out_bytes <= grown < out_bytes + min(4096, smallest)
    assert len(m.__dict__[STORE]) == 1


def test_a_moved_adaptor_weight_names_the_stale_clip_until_refresh():
    c = pmi.build(BASE)
    m = build_module(c)
    idx = [1, 3]                                                # the 4-frame clip with three guides, the 8-frame clip with two
    clips = clips_of(c, m, idx=idx)
    g, counts = [c.g[i] for i in idx], [c.counts[i] for i in idx]
    before = keep(run(c, m, clips, g=g, counts=counts))
    name = "local_compressor.v_proj.2.weight"
    assert name in c.sd
    m.local_compressor.v_proj[2].weight.data.mul_(-1.0)
    with pytest.raises(RuntimeError, match=r"clip 0 is stale.*clip\.refresh\(\)"):
        run(c, m, clips, g=g, counts=counts)
    clips[0].refresh()
    with pytest.raises(RuntimeError, match=r"clip 1 is stale.*clip\.refresh\(\)"):
        run(c, m, clips, g=g, counts=counts)
    clips[1].refresh()
    after = run(c, m, clips, g=g, counts=counts)
    sd = {**c.sd, name: -c.sd[name]}
    bad = []
    for k, i in enumerate(idx):
        for q in range(counts[k]):
            want = pmi.run_oracle(c, i, q, sd=sd)
            assert np.abs(want[:-NG] - pmi.oracle_outputs(BASE)[(i, q)][:-NG]).max() > 4 * TOL        # (no output is within the bar of both)
            bad += pmi.check_pair(c, f"after refresh: pair ({i}, {q})", after[k][q].cpu().numpy(), want, i)
    assert not bad, "; ".join(bad)
    assert not same(before, after) and len(m.__dict__[STORE]) == 1


# ---- 7: refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_with_device_tensors_leave_no_plan():
    c = pmi.build("pm_mix9_chunks3")
    m, other = build_module(c), build_module(c)
    clips, foreign = clips_of(c, m), clips_of(c, other)
    g = guides_of(c.g)
    nl = dev_bf16(np.zeros((pmi.HIDDEN,), np.float32))
    call = lambda *a, **k: m.forward_prepared_many(*a, **k)
    with torch.no_grad():
        with pytest.raises(ValueError, match="clip 1 was prepared by another module"):
            call([clips[0], foreign[1]], g, c.counts)
        with pytest.raises(ValueError, match="clip 1 has no frames_embed"):
            call([clips[0], m.prepare_clip(clips[1].ff, None, "video")], g, c.counts)
        with pytest.raises(ValueError, match=r"clip 1 is 6 x 6 x 1152"):
            call([clips[0], m.prepare_clip(dev_bf16(np.zeros((4, 6, 6, D), np.float32)), dev_bf16(np.zeros((4, 6, 6, D), np.float32)), "video")], g, c.counts)
        with pytest.raises(ValueError, match=r"\[sum Q_i, E\]"):
            call(clips, g[:-1].contiguous(), c.counts)
        with pytest.raises(ValueError, match="guide counts for 2 clips"):
            call(clips, g, c.counts + [1])
        for bad in ([0, 12], [33, 8]):
            with pytest.raises(ValueError, match="Q_i <= 32"):
                call(clips, g, bad)
        with pytest.raises(NotImplementedError, match="float16"):
            call(clips, g.half(), c.counts)
        with pytest.raises(NotImplementedError, match="float16"):
            call(clips, g, c.counts, nl.half())
        with pytest.raises(ValueError, match="prepare_clip returned"):
            call([clips[0], clips[1].ff], g, c.counts)
    m.requires_grad_(True)
    with pytest.raises(RuntimeError, match="autograd"):
        call(clips, g, c.counts)
    m.requires_grad_(False)
    for mod in (m, other):
        assert not mod.__dict__.get(STORE), "a refusal left a plan behind"
    out = call(clips, g, c.counts, chunks=3)
    assert out[0].grad_fn is None and len(m.__dict__[STORE]) == 1
    torch.cuda.synchronize()
