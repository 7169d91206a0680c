"""HIComProjector.forward_ragged (GPU): items of unequal length and mixed modality in one native call (csrc/ragged.hip) against the CPU
oracle run on each item alone, plus what only a ragged kernel can break: item offsets that are no multiple of a tile, a temporal window
that changes between neighbours, per-item packing, isolation, permutation, the positional frame index restarting per item, the work
division, replay / view / plan-cache behaviour, refusals.

Tolerance: <= 1e-3 max-abs on the fp32 output, the bar tests/test_gpu_parity.py holds forward() and tests/test_gpu_batch.py holds
forward_batch to.

Input families (tests/many_item_inputs.py: `edge`, `edge_outlier`, `item_scales`): the same bar per item and per region (local rows, the
32 global rows), HEAVY_REL x max |oracle out| under `edge_outlier`; tests/test_many_item_power.py shows on the oracle alone that a wrong
softmax moves every region by at least 4 bars under them.  The test prints the per-region max-abs of every item.
Measured on an MI355X: `edge` local 4.4e-5 .. 8.5e-5, global 9.1e-7 .. 1.4e-6; `item_scales` local 6.9e-5 and 4.1e-4 (the x 4 item), global
1.0e-6 / 5.8e-6; `edge_outlier` local 5.4e-4 .. 8.6e-4 of bars of 1.7e-3 .. 2.4e-3, global 2.6e-6 .. 6.0e-6."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cases
import hicom_amd
import many_item_inputs as mi
from gpu_util import build_module, dev_bf16
from hicom_amd import ragged, synth
from oracle import hicom_oracle as orc
from oracle_util import to_t

pytestmark = pytest.mark.gpu

TOL = 1e-3
D = cases.D
NG = 32                                                         # global rows per item (local43_global32)
MIX6 = ((1, 4, 1, 8, 1), ("image", "video", "video", "video", "image"), 6, 6)          # token offsets 36, 180, 216, 504
MIX9 = ((1, 4), ("image", "video"), 9, 9)


@functools.lru_cache(maxsize=None)
def ragged_case(splits, modals, h, w, newline=False, cfg_over=()):
    """Weights by the golden cases' law, every item its own tokens and guide (a seed tag per item)."""
    cfg = SimpleNamespace(**{**cases.DEFAULT_CFG, **dict(cfg_over)})
    sd = synth.synth_state_dict(orc.param_shapes(cfg), tag="ragged")
    items = [synth.synth_inputs(T, h, w, D, tag=f"ragged:item{b}") for b, T in enumerate(splits)]
    nl = synth.normal_like((cfg.hidden_size,), synth.seed_of("ragged:newline")) if newline else None
    return SimpleNamespace(cfg=cfg, sd=sd, splits=list(splits), modals=list(modals), newline=nl, B=len(splits),
                           ff=[x["ff"] for x in items], fe=[x["fe"] for x in items], g=np.stack([x["g"] for x in items]))


@functools.lru_cache(maxsize=None)
def oracle_items(*key):
    c = ragged_case(*key)
    sd = {k: to_t(v) for k, v in c.sd.items()}
    return [orc.projector_forward(c.cfg, sd, to_t(c.ff[b]), to_t(c.fe[b]), to_t(c.g[b]), c.modals[b], to_t(c.newline)).numpy() for b in range(c.B)]


def run_ragged(c, m=None, **kw):
    m = m or build_module(c)
    with torch.no_grad():
        out = m.forward_ragged(dev_bf16(np.concatenate(c.ff)), dev_bf16(np.concatenate(c.fe)), dev_bf16(c.g), c.splits, c.modals,
                               dev_bf16(c.newline), **kw)
    torch.cuda.synchronize()
    return out


def check_against_oracle(key, **kw):
    c = ragged_case(*key)
    want = oracle_items(*key)
    out = run_ragged(c, **kw)
    assert isinstance(out, list) and len(out) == c.B
    errs = []
    for b in range(c.B):
        assert out[b].dtype == torch.float32 and tuple(out[b].shape) == want[b].shape, (b, tuple(out[b].shape), want[b].shape)
        errs.append(float(np.abs(out[b].cpu().numpy() - want[b]).max()))
    print(f"forward_ragged {key[:4]} {kw}: max-abs per item {['%.3e' % e for e in errs]}")
    for b in range(c.B):
        glob = out[b][-NG:]
        assert torch.equal(glob, glob[:1].expand_as(glob)), f"item {b}: the {NG} global rows differ"
    # the views tile one storage, in item order
    hidden = out[0].shape[1]
    row = 0
    for b in range(c.B):
        assert out[b].is_contiguous() and out[b].untyped_storage().data_ptr() == out[0].untyped_storage().data_ptr()
        assert out[b].storage_offset() == row * hidden
        row += out[b].shape[0]
    assert out[0].untyped_storage().nbytes() == row * hidden * 4
    assert max(errs) <= TOL, f"{key[:4]}: max-abs per item {errs}"
    return out


def test_mixed_parity_6x6():
    """Offsets 36 / 180 / 216 / 504 tokens, a masked tail tile in every item, kt 1 / 4 / 1 / 4 / 1, item 2 a 1-frame "video"."""
    out = check_against_oracle(MIX6)
    assert [o.shape[0] for o in out] == [36, 36, 36, 40, 36]


@pytest.mark.parametrize("id", [e.id for e in mi.entries("ragged")])
def test_input_families_per_item_and_region_against_oracle(id):
    """The cases of tests/many_item_inputs.py for this step under the families `edge`, `edge_outlier`, `item_scales`: softmax mass on an
    item's first token, both sides of its first tile boundary, of its chunk boundaries and its last token (tests/test_many_item_power.py:
    a wrong softmax moves each region by >= 4 bars).  Per item and per region (local rows, the 32 global rows); bar: TOL, and
    HEAVY_REL x max |oracle out| under `edge_outlier`."""
    c, want = mi.build(id), mi.oracle_outputs(id)
    out = run_ragged(c)
    bad = []
    for b in range(c.B):
        assert out[b].dtype == torch.float32 and tuple(out[b].shape) == want[b].shape, (b, tuple(out[b].shape), want[b].shape)
        assert torch.equal(out[b][-NG:], out[b][-1:].expand(NG, -1)), f"item {b}: the {NG} global rows differ"
        bad += mi.check_item(c.entry, f"item {b}", out[b].cpu().numpy(), want[b])
    assert not bad, f"{id}: " + "; ".join(bad)


def test_device_tables_equal_the_host_mirror():
    """The workspace's table region, as hicom_compressor_ragged_prepare wrote it, word for word against ragged.plan_tables."""
    c = ragged_case(*MIX6)
    m = build_module(c)
    run_ragged(c, m)
    plan, = m.__dict__["_ragged_plans"].values()
    want = ragged.table_image(plan.tables)
    got = plan.ws[:want.size * 4].cpu().numpy().view(np.int32)
    assert np.array_equal(got, want)
    assert sum(plan.tables.chunks) <= 2 * torch.cuda.get_device_properties(0).multi_processor_count + c.B


@pytest.mark.parametrize("cfg_over", [(), (("mm_newline_position", "grid"),)], ids=["default_position", "grid"])
def test_mixed_parity_with_newline_9x9(cfg_over):
    """An image and a 4-frame clip with image_newline.  Default position (no_token): only the image carries a newline row.  "grid"
    (cases.DEFAULT_CFG's merge type is spatial_unpad already): the clip has one after every grid row of 3 tokens, stride 4, the
    image one at its end -- other row counts, other newline strides."""
    key = MIX9 + (True, cfg_over)
    out = check_against_oracle(key)
    c = ragged_case(*key)
    nl = torch.from_numpy(c.newline).cuda()
    m = build_module(c)
    nl_rows = []
    for b in range(c.B):
        desc = ragged.item_descriptors(m, c.splits, c.modals, 9, 9, True)[0][b]
        rows = [desc[4] + k * desc[5] for k in range(desc[3])]
        nl_rows.append(rows)
        for r in rows:
            assert torch.equal(out[b][r], nl), f"item {b} row {r}: not the newline vector"
    assert nl_rows[0] == [9]
    assert nl_rows[1] == ([3, 7, 11] if cfg_over else []) and out[1].shape[0] == (12 if cfg_over else 9) + NG
    # bf16-out mode: shapes equal to forward()'s
    mb = build_module(c, fp32_out=False)
    outb = run_ragged(c, mb)
    with torch.no_grad():
        for b in range(c.B):
            one = mb(dev_bf16(c.ff[b]), dev_bf16(c.fe[b]), dev_bf16(c.g[b]), c.modals[b], dev_bf16(c.newline))
            assert outb[b].dtype == torch.bfloat16 and outb[b].shape == one.shape
            # the same fp32 values rounded once to bf16.  bf16 keeps 8 significant bits, so in [2^e, 2^(e+1)) an ulp is 2^(e-7) and
            # round-to-nearest moves a value by at most half of it, 2^(e-8) <= 2^-8 |x| (no subnormals at |out| ~ 1): the bound
            # tests/test_gpu_parity.py gives the bf16 rows of forward()
            rel = float(((outb[b].float() - out[b]).abs() / out[b].abs().clamp_min(2.0 ** -100)).max())
            print(f"forward_ragged bf16-out item {b}: max |bf16 - fp32| / |fp32| = {rel:.3e} (2^-8 = {2.0 ** -8:.3e})")
            assert bool(((outb[b].float() - out[b]).abs() <= 2.0 ** -8 * out[b].abs()).all())
            for r in nl_rows[b]:
                assert torch.equal(outb[b][r], nl.to(torch.bfloat16))
    torch.cuda.synchronize()


@pytest.mark.parametrize("chunks", [None, 1, 3, 18])
def test_chunks_6x6(chunks):
    """18: one tile per unit on the 8-frame item, clamped to 3 on the images."""
    check_against_oracle(MIX6, **({} if chunks is None else {"chunks": chunks}))


def test_chunks_9x9():
    check_against_oracle(MIX9, chunks=4)


@pytest.mark.parametrize("T,modal", [(4, "video"), (1, "image")], ids=["video_T4", "image"])
@pytest.mark.parametrize("chunks", [1, 3])
def test_equal_shapes_reduce_to_forward_batch_bit_for_bit(T, modal, chunks):
    c = ragged_case((T,) * 3, (modal,) * 3, 6, 6)
    m = build_module(c)
    ff, fe, g = dev_bf16(np.concatenate(c.ff)), dev_bf16(np.concatenate(c.fe)), dev_bf16(c.g)
    with torch.no_grad():
        rag = m.forward_ragged(ff, fe, g, c.splits, modal, chunks=chunks)
        bat = m.forward_batch(ff.view(3, T, 6, 6, D), fe.view(3, T, 6, 6, D), g, modal, chunks=chunks)
    torch.cuda.synchronize()
    for b in range(3):
        assert torch.equal(rag[b], bat[b]), f"item {b}"


def test_items_are_isolated():
    """Item 1 replaced (other tokens and guide, x4: other softmax maxima): items 0, 2, 3 and 4 must not move by a bit."""
    c = ragged_case(*MIX6)
    m = build_module(c)
    first = [o.clone() for o in run_ragged(c, m)]
    other = synth.synth_inputs(4, 6, 6, D, tag="ragged:intruder")
    c2 = SimpleNamespace(**vars(c))
    c2.ff, c2.fe, c2.g = list(c.ff), list(c.fe), c.g.copy()
    c2.ff[1], c2.fe[1], c2.g[1] = other["ff"] * 4, other["fe"] * 4, other["g"] * 4
    second = run_ragged(c2, m)
    for b in (0, 2, 3, 4):
        assert torch.equal(first[b], second[b]), f"item {b} moved"
    assert not torch.equal(first[1], second[1])


def test_permutation():
    """The item order reversed, heuristic work division: the outputs are the reversed list, bit for bit."""
    c = ragged_case(*MIX6)
    m = build_module(c)
    fwd = [o.clone() for o in run_ragged(c, m)]
    c2 = SimpleNamespace(**vars(c))
    c2.ff, c2.fe, c2.g, c2.splits, c2.modals = c.ff[::-1], c.fe[::-1], c.g[::-1].copy(), c.splits[::-1], c.modals[::-1]
    rev = run_ragged(c2, m)
    for b in range(c.B):
        assert torch.equal(fwd[b], rev[c.B - 1 - b]), f"item {b}"


def test_positional_index_restarts_per_item():
    """Three copies of one clip behind a 1-frame image: a frame index that ran on through the stack would give three different outputs."""
    key = ((1, 4, 4, 4), ("image", "video", "video", "video"), 6, 6)
    c = ragged_case(*key)
    c2 = SimpleNamespace(**vars(c))
    c2.ff, c2.fe = [c.ff[0]] + [c.ff[1]] * 3, [c.fe[0]] + [c.fe[1]] * 3
    c2.g = np.stack([c.g[0]] + [c.g[1]] * 3)
    out = run_ragged(c2)
    assert torch.equal(out[1], out[2]) and torch.equal(out[1], out[3])
    want = oracle_items(*key)[1]
    err = float(np.abs(out[3].cpu().numpy() - want).max())
    print(f"forward_ragged copies of one clip: max-abs {err:.3e}")
    assert err <= TOL


def test_replay_views_and_plan_reuse():
    c = ragged_case(*MIX6)
    m = build_module(c)
    ff, fe, g = dev_bf16(np.concatenate(c.ff)), dev_bf16(np.concatenate(c.fe)), dev_bf16(c.g)
    with torch.no_grad():
        a = m.forward_ragged(ff, fe, g, c.splits, c.modals)
        b = m.forward_ragged(ff, fe, g, c.splits, c.modals)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        plans = m.__dict__["_ragged_plans"]
        assert len(plans) == 1
        # a non-owning view of a larger tensor (the vision tower's output with other frames around), other pointers
        pad = torch.zeros((2,) + tuple(ff.shape[1:]), dtype=ff.dtype, device=ff.device)
        big_ff, big_fe = torch.cat([pad, ff, pad]), torch.cat([pad, fe, pad])
        v_ff, v_fe = big_ff[2:2 + ff.shape[0]], big_fe[2:2 + ff.shape[0]]
        assert v_ff.data_ptr() != big_ff.data_ptr() and v_ff.untyped_storage().data_ptr() == big_ff.untyped_storage().data_ptr()
        v = m.forward_ragged(v_ff, v_fe, g.clone(), tuple(c.splits), tuple(c.modals))
        assert all(torch.equal(x, y) for x, y in zip(a, v))
        assert len(plans) == 1 and next(iter(plans.values())).hits == 3          # other pointers, same split_sizes: the plan is reused
        m.forward_ragged(ff[:6], fe[:6], g[:3], c.splits[:3], c.modals[:3])
        assert len(plans) == 2                                                    # split_sizes are part of the key
    torch.cuda.synchronize()


def test_refusals():
    c = ragged_case(*MIX6)
    m = build_module(c)
    ff, fe, g = dev_bf16(np.concatenate(c.ff)), dev_bf16(np.concatenate(c.fe)), dev_bf16(c.g)
    S, M = c.splits, c.modals
    with torch.no_grad():
        with pytest.raises(ValueError, match="sum"):
            m.forward_ragged(ff, fe, g, [1, 4, 1, 8, 2], M)
        with pytest.raises(ValueError, match="modals"):
            m.forward_ragged(ff, fe, g, S, M[:4])
        with pytest.raises(ValueError, match="image"):
            m.forward_ragged(ff, fe, g, [2, 4, 1, 7, 1], M)                       # an "image" item of two frames
        with pytest.raises(NotImplementedError, match=r"item 1.*partition"):
            m.forward_ragged(ff, fe, g, [1, 6, 1, 6, 1], M)                       # 6 frames, temporal window 4
        odd = dev_bf16(np.zeros((2, 7, 7, D), np.float32))                        # 7 is no multiple of the 3 x 3 window
        with pytest.raises(NotImplementedError, match=r"item 0.*partition"):
            m.forward_ragged(odd, odd, g[:2], [1, 1], "image")
        coarse = build_module(ragged_case(*MIX6, False, (("use_guide", "coarse"),)))
        with pytest.raises(NotImplementedError, match="release recipe"):
            coarse.forward_ragged(ff, fe, g, S, M)
        half = hicom_amd.build_vision_projector(c.cfg).to(torch.float16).cuda().eval()
        with pytest.raises(NotImplementedError, match="float16"):
            half.forward_ragged(ff.half(), fe.half(), g.half(), S, M)
        with pytest.raises(NotImplementedError):
            m.forward_ragged(ff.half(), fe.half(), g.half(), S, M)                # fp16 tokens into a bf16 module
        with pytest.raises(NotImplementedError):
            m.forward_ragged({"base": None, "patch": ff[0]}, None, g, S, M)
        for bad in (g[0], g[:2], g[:, :-1].contiguous()):
            with pytest.raises((NotImplementedError, ValueError)):
                m.forward_ragged(ff, fe, bad, S, M)
    assert not m.__dict__.get("_ragged_plans")                                    # no refusal left a plan behind


def test_refuses_to_return_a_detached_tensor_in_grad_mode():
    c = ragged_case((1, 4), ("image", "video"), 6, 6)
    m = build_module(c)
    args = (dev_bf16(np.concatenate(c.ff)), dev_bf16(np.concatenate(c.fe)), dev_bf16(c.g), c.splits, c.modals)
    m.requires_grad_(True)
    with pytest.raises(RuntimeError, match="autograd"):
        m.forward_ragged(*args)
    m.requires_grad_(False)
    out = m.forward_ragged(*args)                                                 # nothing trainable: nothing to detach from
    assert all(o.grad_fn is None for o in out)
