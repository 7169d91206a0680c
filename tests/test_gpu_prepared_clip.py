"""HIComProjector.prepare_clip / forward_prepared (GPU): the k / v adaptor recipes with the adaptor MLPs run once per clip and Q guides
per call (csrc/multi_window.hpp: multi_window_adapt_ctx16, csrc/multi_guide.hip) against the CPU oracle run once per guide, plus what only
this path can break: the guides' isolation inside a group of the window kernel, the bits it shares with the batched adaptor step and
the plain multi-guide step, reuse of one clip, staleness, streams, refusals.

Cases, families and bars: tests/prepared_clip_inputs.py (6 x 6 and 9 x 9 grids, T = 1 / 4 / 8, width 1152, hidden 896; Q in {1, 2, 3, 4,
5, 6, 7, 9}: a full group of the kernel's 4 guides, every remainder, three groups).  Bar: 1e-3 max-abs on the fp32 output per guide and
per region (local rows, the 32 global rows), HEAVY_REL x max |oracle out| under `edge_outlier`; tests/test_prepared_clip_power.py shows
on the oracle alone that a wrong softmax moves every region by at least 4 bars.  The tests print what they measure.
Measured on an MI355X (max |out| 1.2 .. 1.9; 3.5 with newline rows): `edge` local 1.1e-4 .. 6.9e-4, global 8.6e-7 .. 8.5e-6;
`edge_outlier` local 1.1e-3 .. 1.5e-3 of bars of 4.6e-3 .. 4.9e-3, global 1.8e-5 .. 2.3e-5."""
import numpy as np
import pytest
import torch

import many_item_inputs as mi
import prepared_clip_inputs as pci
from gpu_util import build_module, dev_bf16
from hicom_amd import synth
from oracle_util import to_t

pytestmark = pytest.mark.gpu

NG = mi.NG
STORE, PREPARE_STORE = "_prepared_plans", "_prepare_plans"
BASE = "pc_video_T4_Q4"


def inputs(c):
    return dev_bf16(c.ff), dev_bf16(c.fe), dev_bf16(c.g), dev_bf16(c.newline)


def prepared(c, m=None):
    m = m or build_module(c)
    ff, fe, g, nl = inputs(c)
    with torch.no_grad():
        clip = m.prepare_clip(ff, fe, c.modal)
    return m, clip, g, nl


def run(m, clip, g, nl=None, **kw):
    with torch.no_grad():
        out = m.forward_prepared(clip, g, nl, **kw)
    torch.cuda.synchronize()
    return out


def check(c, out, wants, what):
    bad = []
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(wants),) + wants[0].shape, (tuple(out.shape), wants[0].shape)
    for q, want in enumerate(wants):
        assert torch.equal(out[q][-NG:], out[q][-1:].expand(NG, -1)), f"guide {q}: the {NG} global rows differ"
        bad += mi.check_item(c.entry, f"{what} guide {q}", out[q].cpu().numpy(), want)
    return bad


# ---- 1: parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", [e.id for e in pci.CASES])
def test_parity_per_guide_and_region_against_oracle(id):
    c, wants = pci.build(id), pci.oracle_outputs(id)
    m, clip, g, nl = prepared(c)
    lc = m.local_compressor
    assert (clip.y_k is not None) == bool(lc.adapt_k) and (clip.y_v is not None) == bool(lc.adapt_v)
    for y in (clip.y_k, clip.y_v):
        assert y is None or (y.dtype == torch.float16 and tuple(y.shape) == (c.n_tokens, pci.D))
    out = run(m, clip, g, nl)
    bad = check(c, out, wants, "forward_prepared")
    assert not bad, f"{id}: " + "; ".join(bad)
    if c.newline is not None:
        rows = m._layout((1, 3, 3), c.modal, True, False).newline_rows
        assert rows and out.shape[1] == 9 + len(rows) + NG
        for r in rows:
            assert torch.equal(out[:, r], nl.float().expand(c.Q, -1)), f"newline row {r}"


# ---- 2: bits -----------------------------------------------------------------------------------------------------------------------
def test_permuting_the_guides_permutes_the_outputs_bit_for_bit():
    c = pci.build("pc_video_T8_Q9")
    m, clip, g, _ = prepared(c)
    perm = [8, 3, 0, 5, 1, 7, 2, 6, 4]          # (guide 8 leaves the group of one for a group of four, every guide changes its place)
    base = run(m, clip, g).clone()
    out = run(m, clip, g[perm].contiguous())
    for i, q in enumerate(perm):
        assert torch.equal(out[i], base[q]), f"position {i} (guide {q})"


def test_replacing_one_guide_leaves_the_others_bit_identical_and_twins_agree():
    c = pci.build("pc_video_T8_Q9")
    m, clip, g, _ = prepared(c)
    first = run(m, clip, g).clone()
    g2 = g.clone()
    g2[1] = dev_bf16(synth.synth_inputs(1, 3, 3, pci.D, tag="preparedclip:intruder")["g"] * 4)      # other softmax maxima in its group
    second = run(m, clip, g2).clone()
    for q in range(c.Q):
        assert torch.equal(first[q], second[q]) == (q != 1), f"guide {q}"
    g3 = g.clone()
    g3[6] = g[0]                                 # the same guide in two groups, at two places
    third = run(m, clip, g3)
    assert torch.equal(third[0], third[6]) and torch.equal(third[0], first[0]) and not torch.equal(third[0], third[1])


@pytest.mark.parametrize("id", ["pc_video_T4_adaptv_Q1", "pc_video_T4_Q4", "pc_video_T4_adaptk_Q7"])
def test_one_guide_has_the_local_bits_of_forward_batch(id):
    """Q = 1: the planes, the blend code and the readout are those of the batched adaptor step on the [1, T, H, W, E] view."""
    c = pci.build(id)
    m, clip, g, _ = prepared(c)
    ff, fe, _, _ = inputs(c)
    for q in range(min(c.Q, 2)):
        out = run(m, clip, g[q:q + 1])
        with torch.no_grad():
            want = m.forward_batch(ff[None], None if fe is None else fe[None], g[q:q + 1], c.modal)
        torch.cuda.synchronize()
        assert out.shape == want.shape
        assert torch.equal(out[0, :-NG], want[0, :-NG]), f"guide {q}: local rows"


@pytest.mark.parametrize("id,chunks", [(BASE, None), ("pc_video_T8_Q9", 3)])
def test_global_rows_are_those_of_forward_multi_guide_on_a_plain_module(id, chunks):
    """The global stage of this recipe is plain: the same launches on the same non-adaptor weights at the same Q and chunks=."""
    c, p = pci.build(id), pci.build(id, mi.PLAIN)
    m, clip, g, _ = prepared(c)
    plain = build_module(p)
    ff, fe, _, _ = inputs(c)
    kw = {} if chunks is None else {"chunks": chunks}
    out = run(m, clip, g, **kw)
    with torch.no_grad():
        want = plain.forward_multi_guide(ff, fe, g, c.modal, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out[:, -NG:], want[:, -NG:])
    assert not torch.equal(out[:, :-NG], want[:, :-NG])


# ---- 3: reuse ----------------------------------------------------------------------------------------------------------------------
def test_one_clip_serves_successive_calls_and_two_clips_share_one_plan():
    c, wants = pci.build("pc_video_T8_Q9"), pci.oracle_outputs("pc_video_T8_Q9")
    m, clip, g, _ = prepared(c)
    planes = [clip.y_k.clone(), clip.y_v.clone()]
    sets = ([0, 1, 2, 3, 4], [7], [8, 2, 5])
    guides = [g[s].contiguous() for s in sets]
    for gs in guides:                           # (the three plans and their workspaces exist: a plan is per Q)
        run(m, clip, gs)
    before = torch.cuda.memory_allocated()
    bad, outs = [], []
    for s, gs in zip(sets, guides):
        outs.append(run(m, clip, gs))
        bad += check(c, outs[-1], [wants[q] for q in s], f"reuse {s}")
    assert not bad, "; ".join(bad)
    out_bytes = sum(o.numel() * o.element_size() for o in outs)
    grown = torch.cuda.memory_allocated() - before
    print(f"allocated between the calls: {grown} bytes, outputs {out_bytes}, one plane {c.n_tokens * pci.D * 2}")
    assert out_bytes <= grown <= out_bytes + 512 * len(outs)               # the outputs (the allocator rounds a block up to 512 bytes), nothing else
    assert torch.equal(clip.y_k, planes[0]) and torch.equal(clip.y_v, planes[1])
    plans = m.__dict__[STORE]
    assert len(plans) == 3 and len(m.__dict__[PREPARE_STORE]) == 1
    ff, fe, _, _ = inputs(c)
    with torch.no_grad():
        twin = m.prepare_clip(ff.clone(), fe.clone(), c.modal)
    out = run(m, twin, g[sets[2]].contiguous())
    assert torch.equal(out, outs[2])
    assert len(plans) == 3 and len(m.__dict__[PREPARE_STORE]) == 1          # two clips of one shape: one plan, one prepare plan
    assert torch.equal(twin.y_k, clip.y_k) and twin.y_k.data_ptr() != clip.y_k.data_ptr()


# ---- 4: staleness ------------------------------------------------------------------------------------------------------------------
def oracle_with(c, over):
    sd = {k: (over[k](v) if k in over else v) for k, v in c.sd.items()}
    return [pci.run_oracle(c, q, sd=sd) for q in range(c.Q)]


def test_an_adaptor_mlp_update_makes_the_clip_stale_until_refresh():
    c = pci.build(BASE)
    m, clip, g, _ = prepared(c)
    before = run(m, clip, g).clone()
    name = "local_compressor.v_proj.2.weight"
    assert name in c.sd
    m.local_compressor.v_proj[2].weight.data.mul_(-1.0)          # eval mode, through `.data`: exact in bf16
    with pytest.raises(RuntimeError, match="stale"):
        run(m, clip, g)
    with pytest.raises(RuntimeError, match="stale"):
        run(m, clip, g)                                          # ... and stays so
    clip.refresh()
    after = run(m, clip, g)
    wants = oracle_with(c, {name: lambda v: -v})
    assert np.abs(wants[0][:-NG] - pci.oracle_outputs(BASE)[0][:-NG]).max() > 4 * mi.TOL        # (no output is within the bar of both references)
    bad = check(c, after, wants, "after refresh")
    assert not bad, "; ".join(bad)
    assert not torch.equal(before, after) and len(m.__dict__[STORE]) == 1


def test_other_weights_are_followed_without_staleness_under_the_same_plan_and_clip():
    c = pci.build(BASE)
    m, clip, g, _ = prepared(c)
    run(m, clip, g)
    planes = [clip.y_k.clone(), clip.y_v.clone()]
    lc = m.local_compressor
    lc.readout[2].weight.data.mul_(-1.0)
    lc.k_alpha.data.mul_(0.5)                                    # 0.5 -> 0.25: exact
    lc.v_norm.weight.data.mul_(2.0)
    out = run(m, clip, g)
    wants = oracle_with(c, {"local_compressor.readout.2.weight": lambda v: -v, "local_compressor.k_alpha": lambda v: v * 0.5,
                            "local_compressor.v_norm.weight": lambda v: v * 2})
    assert np.abs(wants[0][:-NG] - pci.oracle_outputs(BASE)[0][:-NG]).max() > 4 * mi.TOL
    bad = check(c, out, wants, "readout / alpha / gamma updated")
    assert not bad, "; ".join(bad)
    plans = m.__dict__[STORE]
    assert len(plans) == 1 and next(iter(plans.values())).hits == 2
    assert torch.equal(clip.y_k, planes[0]) and torch.equal(clip.y_v, planes[1]) and not clip.is_stale()


# ---- 5: streams --------------------------------------------------------------------------------------------------------------------
def test_prepare_on_one_stream_call_on_another_without_host_synchronisation():
    c = pci.build(BASE)
    m, clip0, g, _ = prepared(c)
    same = run(m, clip0, g).clone()
    ff, fe, _, _ = inputs(c)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.no_grad():
        with torch.cuda.stream(s1):
            clip = m.prepare_clip(ff, fe, c.modal)
        with torch.cuda.stream(s2):                              # no host wait in between: the call waits for the clip's event on the device
            out = m.forward_prepared(clip, g)
    assert clip.stream == s1
    s2.synchronize()
    assert torch.equal(out, same)


# ---- 6: a plain-recipe module -------------------------------------------------------------------------------------------------------
def test_plain_module_goes_to_forward_multi_guide():
    p = pci.build(BASE, mi.PLAIN)
    m, clip, g, _ = prepared(p)
    assert clip.y_k is None and clip.y_v is None and clip.nbytes == 0 and not m.__dict__.get(PREPARE_STORE)
    out = run(m, clip, g)
    ff, fe, _, _ = inputs(p)
    with torch.no_grad():
        want = m.forward_multi_guide(ff, fe, g, p.modal)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert not m.__dict__.get(STORE) and len(m.__dict__["_multi_guide_plans"]) == 1


# ---- 7: refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_with_device_tensors_leave_no_plan():
    c = pci.build("pc_image_Q3")
    m = build_module(c)
    other = build_module(c)
    ff, fe, g, _ = inputs(c)

    def no_plans(*mods):
        return not any(mod.__dict__.get(s) for mod in mods for s in (STORE, PREPARE_STORE, "_multi_guide_plans"))
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="float16"):
            m.prepare_clip(ff.half(), fe.half(), "image")                              # fp16 tokens into a bf16 module
        odd = dev_bf16(np.zeros((1, 7, 7, pci.D), np.float32))
        with pytest.raises(NotImplementedError, match="partition"):
            m.prepare_clip(odd, odd, "image")
        with pytest.raises(ValueError, match="single frame"):
            m.prepare_clip(ff.expand(2, -1, -1, -1).contiguous(), None, "image")
    m.requires_grad_(True)
    with pytest.raises(RuntimeError, match="autograd"):
        m.prepare_clip(ff, fe, "image")
    m.requires_grad_(False)
    assert no_plans(m, other)
    clip = m.prepare_clip(ff, fe, "image")                                              # nothing trainable: nothing to detach from
    assert len(m.__dict__[PREPARE_STORE]) == 1
    with torch.no_grad():
        with pytest.raises(ValueError, match="another module"):
            other.forward_prepared(clip, g)
        for bad in (g[:, :-1].contiguous(), g[0], g[:0], g[:1].expand(33, -1).contiguous()):
            with pytest.raises(ValueError, match=r"\[Q, E\]|Q <= 32"):
                m.forward_prepared(clip, bad)
        with pytest.raises(NotImplementedError, match="float16"):
            m.forward_prepared(clip, g.half())
    m.requires_grad_(True)
    with pytest.raises(RuntimeError, match="autograd"):
        m.forward_prepared(clip, g)
    m.requires_grad_(False)
    assert not m.__dict__.get(STORE) and no_plans(other)
    out = m.forward_prepared(clip, g)
    assert out.grad_fn is None and len(m.__dict__[STORE]) == 1
    torch.cuda.synchronize()
