"""HIComProjector.forward_batch (GPU): B equal-shaped items in one native call (csrc/batch.hip) against the CPU oracle run on each
item alone, plus the properties that only a batched kernel can break: isolation of the items' softmax states, the positional frame
index restarting per item, masked tail tiles, several chunks per item, replay / view / plan-cache behaviour, refusals.

Tolerance: <= 1e-3 max-abs on the fp32 output, the bar tests/test_gpu_parity.py holds forward() to.

Input families (tests/many_item_inputs.py: `edge`, `edge_outlier`, `item_scales`): the same bar per item and per region (local rows, the
32 global rows), HEAVY_REL x max |oracle out| under `edge_outlier`; tests/test_many_item_power.py shows on the oracle alone that a wrong
softmax moves every region by at least 4 bars under them.  The test prints the per-region max-abs of every item.
Measured on an MI355X: hidden 64, `edge` / `item_scales` local 3.7e-5 .. 8.9e-5 (3.6e-4 on the x 4 item), global 9.2e-7 .. 4.7e-6;
`edge_outlier` local 5.6e-4 / 9.7e-4 of a bar of 1.5e-3 / 2.5e-3, global 3.2e-6 .. 5.1e-6; hidden 896 local 1.6e-4 .. 2.6e-4, global 5.7e-6 ..
7.3e-6; hidden 3584 local 6.3e-4 / 8.2e-4 (max |out| 2.5 / 2.7), global 1.1e-5 / 1.3e-5."""
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


@functools.lru_cache(maxsize=None)
def batch_case(B, T, h, w, modal="video", newline=False, cfg_over=()):
    """Weights by the golden cases' law, every item its own tokens and guide (a seed tag per item); the oracle's output per item."""
    cfg = SimpleNamespace(**{**cases.DEFAULT_CFG, **dict(cfg_over)})
    sd = synth.synth_state_dict(orc.param_shapes(cfg), tag="batch")
    items = [synth.synth_inputs(T, h, w, D, tag=f"batch:item{b}") for b in range(B)]
    nl = synth.normal_like((cfg.hidden_size,), synth.seed_of("batch:newline")) if newline else None
    return SimpleNamespace(cfg=cfg, sd=sd, modal=modal, newline=nl, B=B,
                           ff=np.stack([x["ff"] for x in items]), fe=np.stack([x["fe"] for x in items]), g=np.stack([x["g"] for x in items]))


@functools.lru_cache(maxsize=None)
def oracle_items(*key):
    c = batch_case(*key)
    sd = {k: to_t(v) for k, v in c.sd.items()}
    return [orc.projector_forward(c.cfg, sd, to_t(c.ff[b]), to_t(c.fe[b]), to_t(c.g[b]), c.modal, to_t(c.newline)).numpy() for b in range(c.B)]


def run_batch(c, m=None, **kw):
    m = m or build_module(c)
    with torch.no_grad():
        out = m.forward_batch(dev_bf16(c.ff), dev_bf16(c.fe), dev_bf16(c.g), c.modal, dev_bf16(c.newline), **kw)
    torch.cuda.synchronize()
    return out


def check_against_oracle(key, **kw):
    c = batch_case(*key)
    want = oracle_items(*key)
    out = run_batch(c, **kw)
    assert out.dtype == torch.float32 and tuple(out.shape) == (c.B,) + want[0].shape
    got = out.cpu().numpy()
    errs = [float(np.abs(got[b] - want[b]).max()) for b in range(c.B)]
    print(f"forward_batch {key} {kw}: max-abs per item {['%.3e' % e for e in errs]}")
    ng = 32
    for b in range(c.B):
        glob = out[b, -ng:]
        assert torch.equal(glob, glob[:1].expand_as(glob)), f"item {b}: the {ng} global rows differ"
    assert max(errs) <= TOL, f"{key}: max-abs {max(errs):.3e}"
    return out


@pytest.mark.parametrize("key", [(3, 1, 6, 6, "image", False), (3, 1, 6, 6, "image", True), (3, 4, 6, 6, "video", False)],
                         ids=["image", "image_newline", "video_T4"])
def test_parity_per_item_against_oracle(key):
    out = check_against_oracle(key)
    if key[5]:
        nl = torch.from_numpy(batch_case(*key).newline).cuda()
        assert torch.equal(out[:, -33], nl.expand(key[0], -1))          # the newline row in front of the global rows, bit for bit


@pytest.mark.parametrize("id", [e.id for e in mi.entries("batch")])
def test_input_families_per_item_and_region_against_oracle(id):
    """The cases of tests/many_item_inputs.py for this step under the families `edge`, `edge_outlier`, `item_scales`: softmax mass on an
    item's first token, both sides of its first tile boundary, of its chunk boundaries and its last token (tests/test_many_item_power.py:
    a wrong softmax moves each region by >= 4 bars).  Per item and per region (local rows, the 32 global rows); bar: TOL, and
    HEAVY_REL x max |oracle out| under `edge_outlier`."""
    c, want = mi.build(id), mi.oracle_outputs(id)
    out = run_batch(c, **({} if c.entry.chunks is None else {"chunks": c.entry.chunks}))
    bad = []
    for b in range(c.B):
        assert out[b].dtype == torch.float32 and tuple(out[b].shape) == want[b].shape, (b, tuple(out[b].shape), want[b].shape)
        assert torch.equal(out[b][-NG:], out[b][-1:].expand(NG, -1)), f"item {b}: the {NG} global rows differ"
        bad += mi.check_item(c.entry, f"item {b}", out[b].cpu().numpy(), want[b])
    assert not bad, f"{id}: " + "; ".join(bad)


def test_output_dtype_follows_the_module():
    c = batch_case(3, 1, 6, 6, "image", False)
    m = build_module(c, fp32_out=False)
    out = run_batch(c, m)
    assert out.dtype == torch.bfloat16
    with torch.no_grad():
        one = m(dev_bf16(c.ff[1]), dev_bf16(c.fe[1]), dev_bf16(c.g[1]), c.modal, None)
    assert out[1].shape == one.shape


def test_tail_tile_81_tokens():
    """81 tokens per item = 5 tiles + 1 token: the tail tile is masked, not filled from the next item."""
    check_against_oracle((2, 1, 9, 9, "image", False))


@pytest.mark.parametrize("chunks", [None, 3, 18])
def test_several_chunks_per_item(chunks):
    """288 tokens per item = 18 tiles: the heuristic's choice, 3 chunks of 6 tiles, one tile per chunk."""
    check_against_oracle((2, 8, 6, 6, "video", False), **({} if chunks is None else {"chunks": chunks}))


def test_tail_tile_and_chunks_together():
    check_against_oracle((2, 1, 9, 9, "image", False), chunks=4)


@pytest.mark.parametrize("key,chunks", [((3, 1, 6, 6, "image", False), None), ((3, 4, 6, 6, "video", False), 3)], ids=["image", "video_chunks3"])
def test_items_are_isolated(key, chunks):
    """Item 1 replaced (other tokens and guide, x4: other softmax maxima): items 0 and 2 must not move by a bit."""
    c = batch_case(*key)
    m = build_module(c)
    kw = {} if chunks is None else {"chunks": chunks}
    first = run_batch(c, m, **kw).clone()
    other = synth.synth_inputs(key[1], key[2], key[3], D, tag="batch:intruder")
    c2 = SimpleNamespace(**vars(c))
    c2.ff, c2.fe, c2.g = c.ff.copy(), c.fe.copy(), c.g.copy()
    c2.ff[1], c2.fe[1], c2.g[1] = other["ff"] * 4, other["fe"] * 4, other["g"] * 4
    second = run_batch(c2, m, **kw)
    assert torch.equal(first[0], second[0]) and torch.equal(first[2], second[2])
    assert not torch.equal(first[1], second[1])


def test_positional_index_restarts_per_item():
    """Three copies of one clip: a frame index that ran on through the stack would give three different outputs."""
    c = batch_case(3, 4, 6, 6, "video", False)
    c2 = SimpleNamespace(**vars(c))
    c2.ff, c2.fe, c2.g = (np.stack([a[0]] * 3) for a in (c.ff, c.fe, c.g))
    out = run_batch(c2)
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2])
    want = oracle_items(3, 4, 6, 6, "video", False)[0]
    assert np.abs(out[2].cpu().numpy() - want).max() <= TOL


def test_replay_views_and_plan_reuse():
    c = batch_case(3, 4, 6, 6, "video", False)
    m = build_module(c)
    ff, fe, g = dev_bf16(c.ff), dev_bf16(c.fe), dev_bf16(c.g)
    with torch.no_grad():
        a = m.forward_batch(ff, fe, g, "video")
        b = m.forward_batch(ff, fe, g, "video")
        assert torch.equal(a, b)
        plans = m.__dict__["_batch_plans"]
        assert len(plans) == 1
        # what frames_features.split(...) yields for a uniform batch: a [B T, H, W, E] tensor viewed 5-D, no copy
        stack_ff, stack_fe = ff.reshape(-1, *ff.shape[2:]).clone(), fe.reshape(-1, *fe.shape[2:]).clone()
        v_ff, v_fe = stack_ff.view(ff.shape), stack_fe.view(fe.shape)
        assert v_ff.data_ptr() == stack_ff.data_ptr()
        v = m.forward_batch(v_ff, v_fe, g.clone(), "video")
        assert torch.equal(a, v)
        assert len(plans) == 1 and next(iter(plans.values())).hits == 3          # other pointers, same shape: the plan is reused
        m.forward_batch(ff[:2], fe[:2], g[:2], "video")
        assert len(plans) == 2                                                    # B is part of the key
    torch.cuda.synchronize()


def test_refusals():
    c = batch_case(3, 1, 6, 6, "image", False)
    m = build_module(c)
    ff, fe, g = dev_bf16(c.ff), dev_bf16(c.fe), dev_bf16(c.g)
    with torch.no_grad():
        coarse = build_module(batch_case(3, 1, 6, 6, "image", False, (("use_guide", "coarse"),)))
        with pytest.raises(NotImplementedError, match="release recipe"):
            coarse.forward_batch(ff, fe, g, "image")
        two = torch.cat([ff, ff], 1)
        with pytest.raises((NotImplementedError, ValueError)):
            m.forward_batch(two, two, g, "image")
        half = hicom_amd.build_vision_projector(c.cfg).to(torch.float16).cuda().eval()
        with pytest.raises(NotImplementedError, match="float16"):
            half.forward_batch(ff.half(), fe.half(), g.half(), "image")
        with pytest.raises(NotImplementedError):
            m.forward_batch(ff.half(), fe.half(), g.half(), "image")              # fp16 tokens into a bf16 module
        for bad in (g[0], g[:2], g[:, :-1].contiguous()):
            with pytest.raises((NotImplementedError, ValueError)):
                m.forward_batch(ff, fe, bad, "image")
        odd = dev_bf16(np.zeros((2, 1, 7, 7, D), np.float32))                     # 7 is no multiple of the 3 x 3 window
        with pytest.raises(NotImplementedError, match="partition"):
            m.forward_batch(odd, odd, g[:2], "image")
        with pytest.raises(NotImplementedError):
            m.forward_batch({"base": None, "patch": ff[0, 0]}, None, g, "image")


def test_refuses_to_return_a_detached_tensor_in_grad_mode():
    c = batch_case(3, 1, 6, 6, "image", False)
    m = build_module(c)
    m.requires_grad_(True)
    with pytest.raises(RuntimeError, match="autograd"):
        m.forward_batch(dev_bf16(c.ff), dev_bf16(c.fe), dev_bf16(c.g), "image")
    m.requires_grad_(False)
    out = m.forward_batch(dev_bf16(c.ff), dev_bf16(c.fe), dev_bf16(c.g), "image")     # nothing trainable: nothing to detach from
    assert out.grad_fn is None
