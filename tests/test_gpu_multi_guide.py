"""HIComProjector.forward_multi_guide (GPU): Q instructions on ONE clip in one native call (csrc/multi_guide.hip) against the CPU oracle
run once per guide, plus what only a many-guide kernel can break: isolation of the guides' softmax states, independence of a guide's
result from its place in a group of the local kernel and in a 32-row pass of the stream, masked tail tiles, several token chunks,
plan-cache behaviour, refusals.

Tolerance: <= 1e-3 max-abs on the fp32 output against the oracle, the bar tests/test_gpu_parity.py holds forward() to.  Against forward()
itself (each side within 1e-3 of the oracle) the bar is 2e-3; measured on an MI355X: 1.2e-5 .. 3.2e-5 against the oracle, 9.0e-7 .. 2.3e-5
against forward().

Input families (tests/many_item_inputs.py: `edge`, `edge_outlier`, `item_scales`): the same bar per item and per region (local rows, the
32 global rows), HEAVY_REL x max |oracle out| under `edge_outlier`; tests/test_many_item_power.py shows on the oracle alone that a wrong
softmax moves every region by at least 4 bars under them.  The test prints the per-region max-abs of every item.
Measured on an MI355X: `edge` local 2.8e-5 .. 1.9e-4, global 1.0e-6 .. 2.2e-6; hidden 896 local 4.2e-4 .. 5.1e-4, global 5.8e-6 .. 7.0e-6;
`edge_outlier` local 4.9e-4 .. 6.1e-4 of bars of 1.5e-3 .. 1.9e-3, global 2.9e-6 .. 5.2e-6."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cases
import hicom_amd
import many_item_inputs as mi
from gpu_util import build_module, dev_bf16
from hicom_amd import synth
from oracle import hicom_oracle as orc
from oracle_util import to_t

pytestmark = pytest.mark.gpu

TOL = 1e-3
D = cases.D
NG = 32
STORE = "_multi_guide_plans"


@functools.lru_cache(maxsize=None)
def mg_case(Q, T, h, w, modal="video", newline=False, cfg_over=()):
    """Weights by the golden cases' law, one clip, every guide from its own seed tag."""
    cfg = SimpleNamespace(**{**cases.DEFAULT_CFG, **dict(cfg_over)})
    sd = synth.synth_state_dict(orc.param_shapes(cfg), tag="multiguide")
    clip = synth.synth_inputs(T, h, w, D, tag="multiguide:clip")
    g = np.stack([synth.synth_inputs(1, 3, 3, D, tag=f"multiguide:guide{q}")["g"] for q in range(Q)])
    nl = synth.normal_like((cfg.hidden_size,), synth.seed_of("multiguide:newline")) if newline else None
    return SimpleNamespace(cfg=cfg, sd=sd, modal=modal, newline=nl, Q=Q, ff=clip["ff"], fe=clip["fe"], g=g)


@functools.lru_cache(maxsize=None)
def oracle_guides(key, with_fe=True):
    """The oracle's output per guide; with_fe False: the key stream is frames_feature."""
    c = mg_case(*key)
    sd = {k: to_t(v) for k, v in c.sd.items()}
    fe = c.fe if with_fe else c.ff
    return [orc.projector_forward(c.cfg, sd, to_t(c.ff), to_t(fe), to_t(c.g[q]), c.modal, to_t(c.newline)).numpy() for q in range(c.Q)]


def run_mg(c, m=None, g=None, with_fe=True, **kw):
    m = m or build_module(c)
    with torch.no_grad():
        out = m.forward_multi_guide(dev_bf16(c.ff), dev_bf16(c.fe) if with_fe else None, dev_bf16(c.g if g is None else g), c.modal,
                                    dev_bf16(c.newline), **kw)
    torch.cuda.synchronize()
    return out


def check_against_oracle(key, with_fe=True, **kw):
    c = mg_case(*key)
    want = oracle_guides(key, with_fe)
    out = run_mg(c, with_fe=with_fe, **kw)
    assert out.dtype == torch.float32 and tuple(out.shape) == (c.Q,) + want[0].shape
    got = out.cpu().numpy()
    errs = [float(np.abs(got[q] - want[q]).max()) for q in range(c.Q)]
    print(f"forward_multi_guide {key} fe={with_fe} {kw}: max-abs per guide {['%.3e' % e for e in errs]}")
    for q in range(c.Q):
        glob = out[q, -NG:]
        assert torch.equal(glob, glob[:1].expand_as(glob)), f"guide {q}: the {NG} global rows differ"
    assert max(errs) <= TOL, f"{key}: max-abs {max(errs):.3e}"
    return out


IMAGE3 = (3, 1, 6, 6, "image", False)
VIDEO3_NL = (3, 4, 6, 6, "video", True, (("mm_newline_position", "grid"),))        # a newline row behind every row of windows: rows 2 and 5
VIDEO3 = (3, 4, 6, 6, "video", False)
VIDEO1 = (1, 4, 6, 6, "video", False)
VIDEO5 = (5, 8, 6, 6, "video", False)
IMAGE8 = (8, 1, 9, 9, "image", False)


# ---- parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [IMAGE3, VIDEO3_NL, VIDEO1], ids=["Q3_image", "Q3_video_newline", "Q1_video"])
def test_parity_per_guide_against_oracle(key):
    out = check_against_oracle(key)
    if key[5]:
        c = mg_case(*key)
        nl = torch.from_numpy(c.newline).cuda()
        rows = build_module(c)._layout((1, 2, 2), "video", True, False).newline_rows
        assert rows == [2, 5] and out.shape[1] == 6 + NG
        for r in rows:
            assert torch.equal(out[:, r], nl.expand(key[0], -1)), f"newline row {r}"          # bit for bit


@pytest.mark.parametrize("chunks", [None, 3, 18])
def test_five_guides_cross_a_local_group_and_a_stream_pass(chunks):
    """Q = 5: a local group of four and one of one; 45 folded rows, more than one 32-row pass.  288 tokens = 18 tiles: the stream's own
    choice, 3 chunks of 6 tiles, one tile per chunk."""
    check_against_oracle(VIDEO5, **({} if chunks is None else {"chunks": chunks}))


def test_eight_guides_tail_tile_81_tokens():
    """81 tokens = 5 tiles + 1 token: the tail tile is masked.  72 folded rows."""
    check_against_oracle(IMAGE8)


def test_without_frames_embed_the_keys_are_frames_feature():
    want_fe, want_ff = oracle_guides(VIDEO3), oracle_guides(VIDEO3, False)
    # not vacuous: the two references lie further apart than two tolerances, so no output is within TOL of both
    assert np.abs(want_fe[0][:-NG] - want_ff[0][:-NG]).max() > 2 * TOL
    check_against_oracle(VIDEO3, with_fe=False)


@pytest.mark.parametrize("id", [e.id for e in mi.entries("multi_guide")])
def test_input_families_per_item_and_region_against_oracle(id):
    """The cases of tests/many_item_inputs.py for this step under the families `edge`, `edge_outlier`, `item_scales`: softmax mass on an
    item's first token, both sides of its first tile boundary, of its chunk boundaries and its last token (tests/test_many_item_power.py:
    a wrong softmax moves each region by >= 4 bars).  Per item and per region (local rows, the 32 global rows); bar: TOL, and
    HEAVY_REL x max |oracle out| under `edge_outlier`."""
    c, want = mi.build(id), mi.oracle_outputs(id)
    out = run_mg(c, with_fe=c.entry.with_fe)
    bad = []
    for b in range(c.Q):
        assert out[b].dtype == torch.float32 and tuple(out[b].shape) == want[b].shape, (b, tuple(out[b].shape), want[b].shape)
        assert torch.equal(out[b][-NG:], out[b][-1:].expand(NG, -1)), f"guide {b}: the {NG} global rows differ"
        bad += mi.check_item(c.entry, f"guide {b}", out[b].cpu().numpy(), want[b])
    assert not bad, f"{id}: " + "; ".join(bad)


# ---- isolation and position independence ---------------------------------------------------------------------------------------------
def test_guides_are_isolated():
    """Guide 1 replaced by another guide x 4 (other softmax maxima): outputs 0, 2, 3, 4 do not move by a bit, output 1 does."""
    c = mg_case(*VIDEO5)
    m = build_module(c)
    first = run_mg(c, m).clone()
    g2 = c.g.copy()
    g2[1] = synth.synth_inputs(1, 3, 3, D, tag="multiguide:intruder")["g"] * 4
    second = run_mg(c, m, g=g2)
    for q in (0, 2, 3, 4):
        assert torch.equal(first[q], second[q]), f"guide {q} moved"
    assert not torch.equal(first[1], second[1])


def test_same_guide_twice_gives_the_same_bits():
    c = mg_case(*VIDEO3)
    out = run_mg(c, g=np.stack([c.g[0], c.g[1], c.g[0]]))
    assert torch.equal(out[0], out[2])
    assert not torch.equal(out[0], out[1])


def test_permuted_guides_permute_the_outputs():
    c = mg_case(*VIDEO5)
    m = build_module(c)
    perm = [4, 2, 0, 3, 1]            # (guide 4 leaves the group of one for the group of four, rows cross the 32-row pass)
    base = run_mg(c, m).clone()
    out = run_mg(c, m, g=c.g[perm])
    for i, q in enumerate(perm):
        assert torch.equal(out[i], base[q]), f"position {i} (guide {q})"


# ---- agreement with forward() ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [VIDEO3_NL, VIDEO5, IMAGE8], ids=["Q3_video_newline", "Q5_video", "Q8_image"])
def test_agrees_with_forward_per_guide(key):
    c = mg_case(*key)
    m = build_module(c)
    out = run_mg(c, m)
    ff, fe, nl = dev_bf16(c.ff), dev_bf16(c.fe), dev_bf16(c.newline)
    diffs = []
    with torch.no_grad():
        for q in range(c.Q):
            one = m(ff, fe, dev_bf16(c.g[q]), c.modal, nl)
            assert one.shape == out[q].shape and one.dtype == out.dtype
            diffs.append(float((one - out[q]).abs().max()))
    print(f"forward_multi_guide vs forward() {key}: max-abs per guide {['%.3e' % d for d in diffs]}")
    assert max(diffs) <= 2 * TOL


# ---- module behaviour ------------------------------------------------------------------------------------------------------------------
def test_output_dtype_follows_the_module():
    c = mg_case(*IMAGE3)
    m = build_module(c, fp32_out=False)
    out = run_mg(c, m)
    assert out.dtype == torch.bfloat16
    with torch.no_grad():
        one = m(dev_bf16(c.ff), dev_bf16(c.fe), dev_bf16(c.g[1]), c.modal, None)
    assert out[1].shape == one.shape and one.dtype == torch.bfloat16


def test_plan_reuse_and_key():
    c = mg_case(*VIDEO3)
    m = build_module(c)
    ff, fe, g = dev_bf16(c.ff), dev_bf16(c.fe), dev_bf16(c.g)
    with torch.no_grad():
        a = m.forward_multi_guide(ff, fe, g, "video")
        b = m.forward_multi_guide(ff.clone(), fe.clone(), g.clone(), "video")          # other pointers, same shape
        assert torch.equal(a, b)
        plans = m.__dict__[STORE]
        assert len(plans) == 1 and next(iter(plans.values())).hits == 2
        two = m.forward_multi_guide(ff, fe, g[:2], "video")
        assert len(plans) == 2 and tuple(two.shape) == (2,) + tuple(a.shape[1:])       # Q is part of the key
    torch.cuda.synchronize()


def test_in_place_weight_update_is_followed_under_the_same_plan():
    """p.data.mul_(-1) on the local readout's second Linear in eval mode (exact in bf16): the cached fp16 copy is rebuilt into its
    buffer, the plan stays."""
    c = mg_case(*VIDEO3)
    m = build_module(c)
    before = run_mg(c, m).clone()
    name = "local_compressor.readout.2.weight"
    assert name in c.sd
    m.local_compressor.readout[2].weight.data.mul_(-1.0)
    sd = {k: to_t(-v if k == name else v) for k, v in c.sd.items()}
    want = [orc.projector_forward(c.cfg, sd, to_t(c.ff), to_t(c.fe), to_t(c.g[q]), c.modal, None).numpy() for q in range(c.Q)]
    assert np.abs(want[0][:-NG] - oracle_guides(VIDEO3)[0][:-NG]).max() > 2 * TOL      # (no output is within TOL of both references)
    after = run_mg(c, m)
    plans = m.__dict__[STORE]
    assert len(plans) == 1 and next(iter(plans.values())).hits == 2
    errs = [float(np.abs(after[q].cpu().numpy() - want[q]).max()) for q in range(c.Q)]
    print(f"forward_multi_guide after the in-place update: max-abs per guide {['%.3e' % e for e in errs]}")
    assert max(errs) <= TOL
    assert not torch.equal(before[0], after[0])


def test_side_stream_gives_the_same_bits():
    c = mg_case(*VIDEO3)
    m = build_module(c)
    first = run_mg(c, m).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = run_mg(c, m)
    side.synchronize()
    assert torch.equal(first, second)
    assert len(m.__dict__[STORE]) == 2                                                 # the stream is part of the key: its own workspace


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_no_plan():
    c = mg_case(*IMAGE3)
    m = build_module(c)
    ff, fe, g = dev_bf16(c.ff), dev_bf16(c.fe), dev_bf16(c.g)
    modules = [m]
    with torch.no_grad():
        adapt = build_module(mg_case(*IMAGE3, (("mm_projector_type", "local43_adaptkv_global32"),)))
        coarse = build_module(mg_case(*IMAGE3, (("use_guide", "coarse"),)))
        modules += [adapt, coarse]
        for other in (adapt, coarse):
            with pytest.raises(NotImplementedError, match="plain release recipe"):
                other.forward_multi_guide(ff, fe, g, "image")
        half = hicom_amd.build_vision_projector(c.cfg).to(torch.float16).cuda().eval()
        modules.append(half)
        with pytest.raises(NotImplementedError, match="float16"):
            half.forward_multi_guide(ff.half(), fe.half(), g.half(), "image")
        with pytest.raises(NotImplementedError):
            m.forward_multi_guide(ff.half(), fe.half(), g.half(), "image")            # fp16 tokens into a bf16 module
        with pytest.raises(NotImplementedError):
            m.forward_multi_guide({"base": None, "patch": ff[0]}, None, g, "image")
        odd = dev_bf16(np.zeros((1, 7, 7, D), np.float32))                             # 7 is no multiple of the 3 x 3 window
        with pytest.raises(NotImplementedError, match="partition"):
            m.forward_multi_guide(odd, odd, g, "image")
        with pytest.raises(ValueError, match=r"\[Q, E\]"):
            m.forward_multi_guide(ff, fe, g[:, :-1].contiguous(), "image")
        with pytest.raises(ValueError, match=r"\[Q, E\]"):
            m.forward_multi_guide(ff, fe, g[0], "image")
        with pytest.raises(ValueError, match="Q <= 32"):
            m.forward_multi_guide(ff, fe, g[:1].expand(33, -1).contiguous(), "image")
        with pytest.raises(ValueError, match="Q <= 32"):
            m.forward_multi_guide(ff, fe, g[:0], "image")
        with pytest.raises((NotImplementedError, ValueError)):
            m.forward_multi_guide(ff.float(), fe.float(), g, "image")
    m.requires_grad_(True)
    with pytest.raises(RuntimeError, match="autograd"):
        m.forward_multi_guide(ff, fe, g, "image")
    m.requires_grad_(False)
    for mod in modules:
        assert not mod.__dict__.get(STORE), "a refusal left a plan behind"
    out = m.forward_multi_guide(ff, fe, g, "image")                                   # nothing trainable: nothing to detach from
    assert out.grad_fn is None and len(m.__dict__[STORE]) == 1
