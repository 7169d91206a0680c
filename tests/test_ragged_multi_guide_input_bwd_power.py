"""CPU: the float64 references of tests/ragged_multi_guide_input_bwd_reference.py against autograd gradients of a small fp64 model of the two
stages, on the item / guide-count structure of the GPU cases (MIX6 and MIX9 of tests/ragged_multi_guide_inputs.py, channels cut to 32), and
the five defects a multi-guide input backward can have, planted through the references' keywords.  Each defect must move an input gradient
of every mix by many bars (ragged_train_input_grads.item_bar on the item's reference: the bar the GPU test holds the step to); the smallest
factor is printed.

  1  guide q's dS paired with guide q + 1's row          (shifted_dS: d frames_embed)
  2  the `32 pass` row offset dropped in d x             (drop_pass_offset: d frames_feature, global share)
  3  only the first guide group's share in dkey          (first_group_only: d frames_embed)
  4  a pair's dq summed into its neighbour's             (dq_into_neighbour: d guide_embeds)
  5  no key-side term without frames_embed               (key_grad_in_dvalue=False: d frames_feature)"""
import functools

import pytest
import torch

import ops_reference as R
import ragged_multi_guide_input_bwd_reference as mr
import ragged_train_input_grads as ig

D, NH, KS = 32, 9, 3
SCALE = D ** -0.5
# (grid side, splits, guide counts): the two mixes of the GPU cases
MIXES = {"mix6": (6, (1, 4, 1, 8, 1), (1, 3, 5, 2, 4)), "mix9": (9, (1, 4), (4, 8))}
MANY = 10.0


def items_of(splits):
    return [(T, 4 if T % 4 == 0 else 1) for T in splits]


@functools.lru_cache(maxsize=None)
def model(mix):
    """Leaves, cotangents and the autograd gradients of the small model: local stage per (item, guide, window) softmax attention with the
    guide as the query; global stage per item nh Q_i folded rows of softmax attention over the item's tokens."""
    side, splits, counts = MIXES[mix]
    g = torch.Generator().manual_seed(2024 + side)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    items = items_of(splits)
    tok0, N, nw, pair0, row0 = mr.pair_offsets(items, counts, side, side, KS)
    M = sum(counts)
    m = dict(items=items, counts=counts, side=side, N=N, tok0=tok0, nw=nw, pair0=pair0, row0=row0)
    m["key"], m["value"], m["guides"] = rnd(sum(N), D).requires_grad_(True), rnd(sum(N), D).requires_grad_(True), rnd(M, D).requires_grad_(True)
    m["dctx_l"], m["qt"], m["dctx_g"] = 0.3 * rnd(sum(q * w for q, w in zip(counts, nw)), D), 0.5 * rnd(M * NH, D), 0.3 * rnd(M * NH, D)
    return m


def local_loss(m, key, value, guides):
    total = 0.0
    for i, ((T, kt), Q) in enumerate(zip(m["items"], m["counts"])):
        tok, _ = R.window_tokens(T, m["side"], m["side"], kt, KS)
        K, V = key[m["tok0"][i] + tok], value[m["tok0"][i] + tok]                 # [NW, WIN, D]
        for q in range(Q):
            p = m["pair0"][i] + q
            w = torch.softmax(SCALE * torch.einsum("wid,d->wi", K, guides[p]), 1)
            total = total + (torch.einsum("wi,wid->wd", w, V) * m["dctx_l"][m["row0"][p]:m["row0"][p] + m["nw"][i]]).sum()
    return total


def global_state(m, x):
    """Per item (S, dS) of its nh Q_i rows and the stacked (M, L), as the backward stream leaves them; and the loss whose d x they describe."""
    S, dS, ml, total, row = [], [], [], 0.0, 0
    for i, Q in enumerate(m["counts"]):
        nr = NH * Q
        xi = x[m["tok0"][i]:m["tok0"][i] + m["N"][i]]
        s = m["qt"][row:row + nr] @ xi.t()
        p = torch.softmax(s, 1)
        ctx = p @ xi
        total = total + (ctx * m["dctx_g"][row:row + nr]).sum()
        with torch.no_grad():
            dP = m["dctx_g"][row:row + nr] @ xi.t()
            S.append(s.detach()); dS.append(p * (dP - (p * dP).sum(1, keepdim=True)))
            mx = s.max(1).values
            ml.append(torch.stack([mx, torch.exp(s - mx[:, None]).sum(1)], 1))
        row += nr
    return S, dS, torch.cat(ml), total


def refs(m, value_is_key=False, **defect):
    key = m["value"] if value_is_key else m["key"]
    loc = {k: v for k, v in defect.items() if k != "drop_pass_offset"}
    with torch.no_grad():
        o = mr.rmg_local_bwd_ref(key.detach(), m["value"].detach(), m["guides"].detach(), m["dctx_l"], m["items"], m["counts"], m["side"], m["side"], KS,
                                 SCALE, value_is_key=value_is_key, **loc)
        S, dS, ml, _ = global_state(m, m["value"].detach())
        dx, _, _ = mr.rmg_global_dx_ref(S, dS, ml, m["qt"], m["dctx_g"], m["N"], m["counts"], NH, dx0=o["dvalue"],
                                        drop_pass_offset=defect.get("drop_pass_offset", False))
    return {"frames_feature": dx, "frames_embed": None if value_is_key else o["dkey"], "guide_local": o["dq_pair"]}


def autograd(m, value_is_key=False):
    for t in (m["key"], m["value"], m["guides"]):
        t.grad = None
    key = m["value"] if value_is_key else m["key"]
    (local_loss(m, key, m["value"], m["guides"]) + global_state(m, m["value"])[3]).backward()
    return {"frames_feature": m["value"].grad.clone(), "frames_embed": None if value_is_key else m["key"].grad.clone(), "guide_local": m["guides"].grad.clone()}


@pytest.mark.parametrize("vik", [False, True], ids=["keyed", "value_is_key"])
@pytest.mark.parametrize("mix", sorted(MIXES))
def test_references_are_the_autograd_gradients_of_the_small_model(mix, vik):
    m = model(mix)
    want, got = autograd(m, vik), refs(m, vik)
    for name in want:
        if want[name] is not None:
            err = float((got[name] - want[name]).abs().max())
            assert err <= 1e-11 * max(1.0, float(want[name].abs().max())), (name, err)


def moved(m, name, got, want):
    """The smallest over the items (pairs' items for the guide) of max |got - want| / item_bar(want item)."""
    out = []
    for i, Q in enumerate(m["counts"]):
        rows = slice(m["pair0"][i], m["pair0"][i] + Q) if name == "guide_local" else slice(m["tok0"][i], m["tok0"][i] + m["N"][i])
        out.append((float((got[name][rows] - want[name][rows]).abs().max()) / ig.item_bar(want[name][rows].numpy()), Q))
    return out


# defect -> (keyword, the gradient it must move, value_is_key, which items it can reach: a predicate of the item's guide count)
DEFECTS = {
    "1 dS of guide q with guide q+1's row": (dict(shifted_dS=True), "frames_embed", False, lambda Q: Q >= 2),
    "2 the 32-pass row offset dropped in d x": (dict(drop_pass_offset=True), "frames_feature", False, lambda Q: NH * Q > 32),
    "3 only the first guide group in dkey": (dict(first_group_only=True), "frames_embed", False, lambda Q: Q > mr.GUIDE_GROUP),
    "4 a pair's dq into its neighbour's": (dict(dq_into_neighbour=True), "guide_local", False, lambda Q: True),
    "5 no key-side term without frames_embed": (dict(key_grad_in_dvalue=False), "frames_feature", True, lambda Q: True),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defects_move_an_input_gradient_by_many_bars(defect):
    kw, name, vik, reach = DEFECTS[defect]
    smallest = float("inf")
    for mix in sorted(MIXES):
        m = model(mix)
        want, wrong = refs(m, vik), refs(m, vik, **kw)
        hit = [f for f, Q in moved(m, name, wrong, want) if reach(Q)]
        assert hit, f"{defect}: {mix} has no item the defect can reach"
        smallest = min(smallest, min(hit))
        # ... and nothing else: the items the defect cannot reach keep their gradient
        assert all(f == 0.0 for f, Q in moved(m, name, wrong, want) if not reach(Q) and not kw.get("dq_into_neighbour"))
    print(f"POWER {defect}: smallest factor over the reachable items of both mixes {smallest:.1f} bars")
    assert smallest > MANY
