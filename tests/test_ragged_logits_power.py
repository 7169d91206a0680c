"""What the cases of tests/ragged_logits_inputs.py can see of the window backward of the logits form (CPU, float64).

A model of hicom_compressor_ragged_local_logits_bwd as the training step uses it -- per item and window: p = softmax(scale l) over the
window's tokens from the fp32 scores the GPU is handed, dctx_w from fp64 autograd through the oracle's readout and packing with the
case's cotangent, dp_n = dctx_w . v_n, then
    dl_n = scale p_n (dp_n - sum_m p_m dp_m),    dv_n = p_n dctx_w
-- written out in float64 with the defects such a kernel can have planted in it.  The model runs no code of the package's hot path (only
the oracle, the input generators and the bars), so this file also passes on the commit before the feature: it says something about the
TESTS, not about the kernel.

Unmutated, the model reproduces dl_reference (from the oracle's autograd d frames_embed) far inside the bar: at most 3.1e-5 bars
(the scores are rounded to fp32).  The value-side share dv is held as a displacement: the mutant's dv minus the clean model's, in units of
the item bar of the oracle's whole d frames_feature.  For every GPU case, each mutant moves d local_logits or d frames_feature of at least
one item by several bars (asserted: more than 3).  Measured, the smallest over the ten cases of the larger of the two:
  no_scale       `scale` dropped from dl                                            3.31e+03 bars (d frames_feature does not move)
  no_delta       the sum_m p_m dp_m term dropped                                    95.2 bars (batch_video_T4; d frames_feature does not move)
  item_off_one   the window -> item map off by one item (scores of the next item)   54.6 bars (batch_video_T4; d frames_feature 35.1)
  wrong_window   the softmax taken over the next window's scores                    97.6 bars (batch_T8_chunks3; d local_logits 97.3)
The test prints, per case and mutant, the largest displacement of both in units of the bars."""
import functools
import math

import numpy as np
import pytest
import torch

import many_item_inputs as mi
import ragged_logits_inputs as li
import ragged_train_input_grads as ig
import ragged_train_inputs as rt
from oracle import hicom_oracle as orc
from oracle_util import to_t

MUTANTS = ("no_scale", "no_delta", "item_off_one", "wrong_window")
NG = mi.NG
SEVERAL = 3.0


@functools.lru_cache(maxsize=None)
def state(id):
    """Per item, float64: the window index, the scores, the value rows and dctx per window."""
    c = mi.build(id)
    f64 = torch.float64
    sd = {k: to_t(v, f64) for k, v in c.sd.items() if k.startswith("local_compressor.")}
    spec = orc.parse_projector_type(c.cfg.mm_projector_type)["local"]
    mode = orc.resolve_guide_mode(c.cfg, spec["force_use_guide"])
    ll = torch.from_numpy(np.asarray(li.scores(id))).double()
    items, t0 = [], 0
    for i, (ff, fe, g, modal) in enumerate(c.items):
        T, H, W, D = ff.shape
        ctx, _ = orc.local_context(spec, mode, sd, "local_compressor", to_t(ff, f64), to_t(fe, f64), to_t(g, f64), modal, None, None)
        ctx = ctx.detach().requires_grad_(True)
        loc = orc.post_process(c.cfg, orc.mlp2(ctx, sd, "local_compressor.readout"), modal, None, False)
        n_rows = mi.oracle_outputs(id)[i].shape[0]
        cot = torch.from_numpy(rt.cotangent(id, i, (n_rows, loc.shape[-1]))).double()[:-NG]
        (loc * cot.view(loc.shape)).sum().backward()
        kt = 1 if (modal == "image" or T == 1) else spec["kt"]
        idx = orc.window_token_index(T, H, W, kt, spec["ks"])
        items.append(dict(idx=idx, l=ll[t0:t0 + T].reshape(-1), v=to_t(ff, f64).reshape(-1, D), dctx=ctx.grad.reshape(-1, D), scale=1.0 / math.sqrt(D),
                          shape=(T, H, W)))
        t0 += T
    return items


def model(id, mutant=None):
    """[(dl [T, H, W], dv [T H W, D])] per item."""
    items, out = state(id), []
    for i, it in enumerate(items):
        idx, scale = it["idx"], it["scale"]
        l = it["l"]
        if mutant == "item_off_one":                            # the scores at the next item's first token + the window's token, wrapped
            nxt = items[(i + 1) % len(items)]["l"]
            l = nxt[torch.arange(l.numel()) % nxt.numel()]
        lw = l[idx]
        if mutant == "wrong_window":
            lw = lw.roll(-1, 0)
        p = torch.softmax(scale * lw, dim=-1)
        dp = torch.einsum("nd,nkd->nk", it["dctx"], it["v"][idx])
        delta = 0.0 if mutant == "no_delta" else (p * dp).sum(-1, keepdim=True)
        dlw = (1.0 if mutant == "no_scale" else scale) * p * (dp - delta)
        dl = torch.zeros_like(it["l"])
        dl[idx.reshape(-1)] = dlw.reshape(-1)
        dv = torch.zeros_like(it["v"])
        dv[idx.reshape(-1)] = (p[:, :, None] * it["dctx"][:, None, :]).reshape(-1, dv.shape[1])
        out.append((dl.reshape(it["shape"]).numpy(), dv.numpy()))
    return out


def in_bars(id, got, clean):
    """(largest dl error against dl_reference, largest dv displacement against the clean model) over the items, each in its item bar."""
    _, want_in = ig.yardstick(id)
    e_dl = max(float(np.abs(dl - want).max()) / ig.item_bar(want) for (dl, _), want in zip(got, li.dl_reference(id)))
    e_dv = max(float(np.abs(dv - dv0).max()) / ig.item_bar(w) for (_, dv), (_, dv0), w in zip(got, clean, want_in["frames_feature"]))
    return e_dl, e_dv


@pytest.mark.parametrize("id", li.CASES)
def test_every_planted_defect_moves_a_gradient_by_several_bars(id):
    clean = model(id)
    e_dl, _ = in_bars(id, clean, clean)
    print(f"{id} model vs dl_reference: {e_dl:.2e} bars")
    assert e_dl <= 0.05, f"{id}: the model is not the oracle's backward: {e_dl:.3g} bars"
    slipped = []
    for mutant in MUTANTS:
        m_dl, m_dv = in_bars(id, model(id, mutant), clean)
        print(f"{id} {mutant}: d local_logits {m_dl:.3g}  d frames_feature {m_dv:.3g}  (bars)")
        if not max(m_dl, m_dv) > SEVERAL:
            slipped.append(f"{mutant}: at most {max(m_dl, m_dv):.3g} bars")
    assert not slipped, f"{id}: " + "; ".join(slipped)
