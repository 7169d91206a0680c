"""forward_batch / forward_ragged on the k / v adaptor recipe `local43_adaptkv_global32` (GPU): the adaptor MLPs as dense GEMMs over all
tokens of the call and the LayerNorm + alpha blend fused into the per-item window kernel (csrc/segment_item.hpp:
local_window_adapt_ctx16), against the CPU oracle run on each item alone.

Tolerance: <= 1e-3 max-abs on the fp32 output, the bar tests/test_gpu_parity.py, test_gpu_batch.py and test_gpu_ragged.py hold every
forward path to.  Grids are 6x6 / 9x9, width 1152, hidden 896.  The helpers restate those of test_gpu_ragged.py / test_gpu_batch.py.

Input families (tests/many_item_inputs.py: `edge`, `edge_outlier`, `item_scales`): the same bar per item and per region (local rows, the
32 global rows), HEAVY_REL x max |oracle out| under `edge_outlier`; tests/test_many_item_power.py shows on the oracle alone that a wrong
softmax moves every region by at least 4 bars under them.  The test prints the per-region max-abs of every item.
Measured on an MI355X (hidden 896, max |out| 1.1 .. 1.8): `edge` local 1.4e-4 .. 3.7e-4, global 4.9e-6 .. 6.5e-6; `edge_outlier` local
1.1e-3 .. 1.8e-3 of bars of 3.5e-3 .. 5.7e-3, global 1.5e-5 .. 2.4e-5."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cases
import hicom_amd
import many_item_inputs as mi
from gpu_util import build_module, dev_bf16
from hicom_amd import native as nv
from hicom_amd import ragged, synth
from oracle import hicom_oracle as orc
from oracle_util import to_t

pytestmark = pytest.mark.gpu

TOL = 1e-3
D = cases.D
NG = 32                                                         # global rows per item
HIDDEN = 896
ADAPTKV, ADAPTK, ADAPTV, PLAIN = "local43_adaptkv_global32", "local43_adaptk_global32", "local43_adaptv_global32", "local43_global32"
MIX6 = ((1, 4, 1, 8, 1), ("image", "video", "video", "video", "image"), 6, 6)          # token offsets 36, 180, 216, 504
MIX9 = ((1, 4), ("image", "video"), 9, 9)
# hicom_compressor_{ragged,batch}_workspace_bytes of the PLAIN entry points as the parent commit of this feature computed them (its
# library, called on the host): MIX6 resp. B = 3 clips of 4 frames at 6x6, E = 1152, hidden = 896, 9 heads, P = 28 positional rows
# (16 frames + 6 + 6), chunks = 3, fp32 output, no newline
PARENT_RAGGED_WS_BYTES = 1855744
PARENT_BATCH_WS_BYTES = 1099776


@functools.lru_cache(maxsize=None)
def case_of(splits, modals, h, w, recipe=ADAPTKV, newline=False, cfg_over=(), with_fe=True):
    """Weights by the golden cases' law (alphas = 0.5, as G5_adaptkv), every item its own tokens and guide (a seed tag per item).  The
    state dict is always the adaptkv one: a recipe with fewer adaptors loads the part it has."""
    cfg = SimpleNamespace(**{**cases.DEFAULT_CFG, "hidden_size": HIDDEN, "mm_projector_type": recipe, **dict(cfg_over)})
    full = SimpleNamespace(**{**vars(cfg), "mm_projector_type": ADAPTKV})
    sd_all = synth.synth_state_dict(orc.param_shapes(full), tag="segadapt")
    assert float(sd_all["local_compressor.k_alpha"][0]) == float(sd_all["local_compressor.v_alpha"][0]) == 0.5
    sd = {k: v for k, v in sd_all.items() if k in orc.param_shapes(cfg)}
    items = [synth.synth_inputs(T, h, w, D, tag=f"segadapt:item{b}") for b, T in enumerate(splits)]
    nl = synth.normal_like((cfg.hidden_size,), synth.seed_of("segadapt:newline")) if newline else None
    return SimpleNamespace(cfg=cfg, sd=sd, splits=list(splits), modals=list(modals), newline=nl, B=len(splits),
                           ff=[x["ff"] for x in items], fe=[x["fe"] for x in items] if with_fe else None, g=np.stack([x["g"] for x in items]))


def oracle_of(c, sd=None):
    sd = {k: to_t(v) for k, v in (sd or c.sd).items()}
    return [orc.projector_forward(c.cfg, sd, to_t(c.ff[b]), None if c.fe is None else to_t(c.fe[b]), to_t(c.g[b]), c.modals[b],
                                  to_t(c.newline)).numpy() for b in range(c.B)]


@functools.lru_cache(maxsize=None)
def oracle_items(*key):
    return oracle_of(case_of(*key))


def run_ragged(c, m=None, **kw):
    m = m or build_module(c)
    with torch.no_grad():
        out = m.forward_ragged(dev_bf16(np.concatenate(c.ff)), None if c.fe is None else dev_bf16(np.concatenate(c.fe)), dev_bf16(c.g), c.splits,
                               c.modals, dev_bf16(c.newline), **kw)
    torch.cuda.synchronize()
    return out


def errors(out, want, what):
    errs = []
    for b in range(len(want)):
        assert out[b].dtype == torch.float32 and tuple(out[b].shape) == want[b].shape, (b, tuple(out[b].shape), want[b].shape)
        errs.append(float(np.abs(out[b].cpu().numpy() - want[b]).max()))
    print(f"{what}: max-abs per item {['%.3e' % e for e in errs]}")
    return errs


def check_ragged(key, **kw):
    c = case_of(*key)
    want = oracle_items(*key)
    out = run_ragged(c, **kw)
    assert isinstance(out, list) and len(out) == c.B
    errs = errors(out, want, f"forward_ragged {key[4] if len(key) > 4 else ADAPTKV} {key[:4]} {kw}")
    for b in range(c.B):
        glob = out[b][-NG:]
        assert torch.equal(glob, glob[:1].expand_as(glob)), f"item {b}: the {NG} global rows differ"
    assert max(errs) <= TOL, f"{key}: max-abs per item {errs}"
    return out


def check_not_vacuous(key):
    """On the CPU: the oracle's local rows with the adaptors against the oracle on the SAME weights under local43_global32."""
    c = case_of(*key)
    with_ad = oracle_items(*key)
    plain = SimpleNamespace(**vars(c))
    plain.cfg = SimpleNamespace(**{**vars(c.cfg), "mm_projector_type": PLAIN})
    without = oracle_of(plain)
    gaps = [float(np.abs(a[:-NG] - b[:-NG]).max()) for a, b in zip(with_ad, without)]
    print(f"oracle local rows, {c.cfg.mm_projector_type} vs {PLAIN} on the same weights: max-abs per item {['%.3e' % g for g in gaps]}")
    assert min(gaps) >= 10 * TOL, gaps
    for a, b in zip(with_ad, without):
        assert np.array_equal(a[-NG:], b[-NG:])                   # the global stage of this recipe is plain


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
def test_mixed_parity_6x6():
    """Offsets 36 / 180 / 216 / 504 tokens, windows of 9 tokens (kt = 1) beside windows of 36 (kt = 4), item 2 a 1-frame "video"."""
    check_not_vacuous(MIX6)
    out = check_ragged(MIX6)
    assert [o.shape[0] for o in out] == [36, 36, 36, 40, 36]


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe", [ADAPTK, ADAPTV])
def test_one_adaptor_only(recipe):
    """The NULL-stream branches of the window kernel and the single-problem GEMM launches."""
    check_not_vacuous(MIX6 + (recipe,))
    check_ragged(MIX6 + (recipe,))


@pytest.mark.parametrize("id", [e.id for e in mi.entries("adapt")])
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


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def test_frames_embed_none():
    """The k adaptor then reads frames_feature."""
    key = MIX6 + (ADAPTKV, False, (), False)
    check_not_vacuous(key)
    out = check_ragged(key)
    with_fe = run_ragged(case_of(*MIX6))
    assert not torch.equal(out[1], with_fe[1])


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_over", [(), (("mm_newline_position", "grid"),)], ids=["default_position", "grid"])
def test_parity_with_newline_9x9(cfg_over):
    key = MIX9 + (ADAPTKV, True, cfg_over)
    check_not_vacuous(key)
    out = check_ragged(key)
    c = case_of(*key)
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
    # bf16-out mode: the same fp32 values rounded once to bf16.  bf16 keeps 8 significant bits: round-to-nearest moves a value by at
    # most half an ulp, 2^-8 |x| (no subnormals at |out| ~ 1), the bound tests/test_gpu_ragged.py gives the plain recipe
    outb = run_ragged(c, build_module(c, fp32_out=False))
    for b in range(c.B):
        assert outb[b].dtype == torch.bfloat16 and outb[b].shape == out[b].shape
        rel = float(((outb[b].float() - out[b]).abs() / out[b].abs().clamp_min(2.0 ** -100)).max())
        print(f"forward_ragged adaptkv bf16-out item {b}: max |bf16 - fp32| / |fp32| = {rel:.3e} (2^-8 = {2.0 ** -8:.3e})")
        assert bool(((outb[b].float() - out[b]).abs() <= 2.0 ** -8 * out[b].abs()).all())
        for r in nl_rows[b]:
            assert torch.equal(outb[b][r], nl.to(torch.bfloat16))


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,modal", [(1, "image"), (4, "video")], ids=["image", "video_T4"])
def test_forward_batch_parity(T, modal):
    key = ((T,) * 3, (modal,) * 3, 6, 6)
    check_not_vacuous(key)
    c = case_of(*key)
    m = build_module(c)
    with torch.no_grad():
        out = m.forward_batch(dev_bf16(np.stack(c.ff)), dev_bf16(np.stack(c.fe)), dev_bf16(c.g), modal)
    torch.cuda.synchronize()
    want = oracle_items(*key)
    assert tuple(out.shape) == (3,) + want[0].shape
    errs = errors(out, want, f"forward_batch adaptkv B=3 T={T}")
    for b in range(3):
        assert torch.equal(out[b, -NG:], out[b, -1:].expand(NG, -1))
    assert max(errs) <= TOL, errs


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,modal", [(4, "video"), (1, "image")], ids=["video_T4", "image"])
@pytest.mark.parametrize("chunks", [1, 3])
def test_equal_shapes_reduce_to_forward_batch_bit_for_bit(T, modal, chunks):
    c = case_of((T,) * 3, (modal,) * 3, 6, 6)
    m = build_module(c)
    ff, fe, g = dev_bf16(np.concatenate(c.ff)), dev_bf16(np.concatenate(c.fe)), dev_bf16(c.g)
    with torch.no_grad():
        rag = m.forward_ragged(ff, fe, g, c.splits, modal, chunks=chunks)
        bat = m.forward_batch(ff.view(3, T, 6, 6, D), fe.view(3, T, 6, 6, D), g, modal, chunks=chunks)
    torch.cuda.synchronize()
    for b in range(3):
        assert torch.equal(rag[b], bat[b]), f"item {b}"


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def test_items_are_isolated():
    """Item 1 replaced (other tokens and guide, x4): items 0, 2, 3 and 4 must not move by a bit."""
    c = case_of(*MIX6)
    m = build_module(c)
    first = [o.clone() for o in run_ragged(c, m)]
    other = synth.synth_inputs(4, 6, 6, D, tag="segadapt:intruder")
    c2 = SimpleNamespace(**vars(c))
    c2.ff, c2.fe, c2.g = list(c.ff), list(c.fe), c.g.copy()
    c2.ff[1], c2.fe[1], c2.g[1] = other["ff"] * 4, other["fe"] * 4, other["g"] * 4
    second = run_ragged(c2, m)
    for b in (0, 2, 3, 4):
        assert torch.equal(first[b], second[b]), f"item {b} moved"
    assert not torch.equal(first[1], second[1])


# ---- 8 -------------------------------------------------------------------------------------------------------------------------
def test_permutation():
    c = case_of(*MIX6)
    m = build_module(c)
    fwd = [o.clone() for o in run_ragged(c, m)]
    c2 = SimpleNamespace(**vars(c))
    c2.ff, c2.fe, c2.g, c2.splits, c2.modals = c.ff[::-1], c.fe[::-1], c.g[::-1].copy(), c.splits[::-1], c.modals[::-1]
    rev = run_ragged(c2, m)
    for b in range(c.B):
        assert torch.equal(fwd[b], rev[c.B - 1 - b]), f"item {b}"


# ---- 9 -------------------------------------------------------------------------------------------------------------------------
def test_plain_recipe_is_untouched():
    """A local43_global32 module runs the plain entry points on the plain workspace layout: no adaptor region, the parent's size."""
    c = case_of(*MIX6 + (PLAIN,))
    m = build_module(c)
    out = run_ragged(c, m, chunks=3)
    plan, = m.__dict__["_ragged_plans"].values()
    assert type(plan.args) is nv.CompressorRaggedArgs and plan.io is plan.args and plan.adapt_bytes == 0
    a = plan.args
    assert (a.B, a.H, a.W, a.E, a.hidden, a.ks, a.nh, a.P, a.chunks, a.out_dt) == (5, 6, 6, D, HIDDEN, 3, 9, 28, 3, nv.DT_F32)
    assert plan.ws.numel() == a.ws_bytes == nv.compressor_ragged_workspace(a) == PARENT_RAGGED_WS_BYTES
    errs = errors(out, oracle_items(*MIX6 + (PLAIN,)), "forward_ragged plain recipe")
    assert max(errs) <= TOL
    cb = case_of((4,) * 3, ("video",) * 3, 6, 6, PLAIN)
    mb = build_module(cb)
    with torch.no_grad():
        mb.forward_batch(dev_bf16(np.stack(cb.ff)), dev_bf16(np.stack(cb.fe)), dev_bf16(cb.g), "video", chunks=3)
    torch.cuda.synchronize()
    planb, = mb.__dict__["_batch_plans"].values()
    assert type(planb.args) is nv.CompressorBatchArgs and planb.io is planb.args and planb.adapt_bytes == 0
    b = planb.args
    assert (b.B, b.T, b.H, b.W, b.E, b.hidden, b.kt, b.ks, b.nh, b.P, b.chunks, b.out_dt) == (3, 4, 6, 6, D, HIDDEN, 4, 3, 9, 28, 3, nv.DT_F32)
    assert planb.ws.numel() == b.ws_bytes == nv.compressor_batch_workspace(b) == PARENT_BATCH_WS_BYTES
    # the adaptor recipe: the same layout in front, one hidden plane and one y plane per adapted stream behind it (fp16 [tokens, E])
    ca = case_of(*MIX6)
    ma = build_module(ca)
    run_ragged(ca, ma, chunks=3)
    pa, = ma.__dict__["_ragged_plans"].values()
    assert type(pa.args) is nv.CompressorRaggedAdaptArgs
    assert pa.adapt_bytes == 4 * 540 * D * 2 and pa.ws.numel() == PARENT_RAGGED_WS_BYTES + pa.adapt_bytes


# ---- 10 ------------------------------------------------------------------------------------------------------------------------
def test_in_place_weight_update_is_followed_under_the_same_plan():
    """p.data.mul_(-1) on the v adaptor's second Linear in eval mode (exact in bf16; LayerNorm does not absorb a sign): the cached fp16
    copy is rebuilt into its buffer, the plan stays."""
    c = case_of(*MIX6)
    m = build_module(c)
    before = [o.clone() for o in run_ragged(c, m)]
    name = "local_compressor.v_proj.2.weight"
    m.local_compressor.v_proj[2].weight.data.mul_(-1.0)
    sd = dict(c.sd)
    sd[name] = -c.sd[name]
    want = oracle_of(c, sd)
    moved = [float(np.abs(a[:-NG] - b[:-NG]).max()) for a, b in zip(want, oracle_items(*MIX6))]
    print(f"oracle local rows, new vs old v adaptor weight: max-abs per item {['%.3e' % g for g in moved]}")
    assert min(moved) >= 10 * TOL
    after = run_ragged(c, m)
    plans = m.__dict__["_ragged_plans"]
    assert len(plans) == 1 and next(iter(plans.values())).hits == 2
    errs = errors(after, want, "forward_ragged after the in-place update")
    assert max(errs) <= TOL, errs
    assert not torch.equal(before[0], after[0])


# ---- 11 ------------------------------------------------------------------------------------------------------------------------
def test_refusals_stay():
    c = case_of(*MIX6)
    ff, fe, g = dev_bf16(np.concatenate(c.ff)), dev_bf16(np.concatenate(c.fe)), dev_bf16(c.g)
    bff, bfe = ff[:3].reshape(3, 1, 6, 6, D), fe[:3].reshape(3, 1, 6, 6, D)

    def module(**over):
        cfg = SimpleNamespace(**{**vars(c.cfg), **over})
        m = hicom_amd.build_vision_projector(cfg)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in c.sd.items()}, strict=False)      # (the adaptkv state dict)
        return m.to(torch.bfloat16).cuda().eval()
    with torch.no_grad():
        for m in (module(mm_projector_type="local43_adaptqkvg_global32_adaptg"), module(use_guide="coarse")):
            with pytest.raises(NotImplementedError, match="release recipe"):
                m.forward_ragged(ff, fe, g, c.splits, c.modals)
            with pytest.raises(NotImplementedError, match="release recipe"):
                m.forward_batch(bff, bfe, g[:3], "image")
            assert not m.__dict__.get("_ragged_plans") and not m.__dict__.get("_batch_plans")
    m = build_module(c)
    m.requires_grad_(True)
    with pytest.raises(RuntimeError, match="autograd"):
        m.forward_ragged(ff, fe, g, c.splits, c.modals)
    with pytest.raises(RuntimeError, match="autograd"):
        m.forward_batch(bff, bfe, g[:3], "image")
