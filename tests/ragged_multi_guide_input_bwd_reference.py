"""Plain float64 restatements of the three entry points behind forward_ragged_multi_guide_train(input_grads=True) (torch on the CPU; no call
into hicom_amd), built on the per-item references of tests/ops_reference.py:

  rmg_local_bwd_ref    hicom_compressor_ragged_multiguide_local_bwd + _dq_pair: ops_reference.window_attention_bwd_ref per (item, guide) on the
                       item's own grid, its tokens at tok0_i, guide q's row as the query of all its windows and the pair's rows of dctx;
                       dq pair-major, dkey / dvalue summed over the item's guides
  rmg_global_dx_ref    hicom_compressor_ragged_multiguide_global_dx: ops_reference.global_dx_ref per item on ALL nh Q_i rows of the item's row
                       space (the rows nh pair0_i .. of ml / qt / dctx)

Shared by tests/test_gpu_ragged_multi_guide_input_bwd.py (the kernels against these) and tests/test_ragged_multi_guide_input_bwd_power.py
(these against float64 autograd of a small model of the two stages, and the defects a multi-guide kernel can have, planted through the
keywords)."""
import torch

import ops_reference as R
from ragged_input_bwd_reference import offsets

GUIDE_GROUP = 4          # csrc/multi_window.hpp: kGuideGroup
PASS_ROWS = 32           # rows of one pass of the stream


def pair_offsets(items, counts, H, W, ks):
    """(tok0, N, windows per item, pair0 per item, first dq row per pair) ; items: (T, kt) pairs."""
    tok0, N, _, nw = offsets(items, H, W, ks)
    pair0 = [sum(counts[:i]) for i in range(len(counts))]
    rows, first = [], 0
    for w, Q in zip(nw, counts):
        for _ in range(Q):
            rows.append(first)
            first += w
    return tok0, N, nw, pair0, rows


def rmg_local_bwd_ref(key, value, guides, dctx, items, counts, H, W, ks, scale, value_is_key=False, shifted_dS=False, first_group_only=False,
                      dq_into_neighbour=False, key_grad_in_dvalue=True):
    """key, value [sum N_i, D], guides [M, D], dctx [sum Q_i w_i, D] pair-major, all float64.  Returns a dict: dq [sum Q_i w_i, D], dq_pair
    [M, D], dkey, dvalue [sum N_i, D] (dkey zero with value_is_key: the key-side rows are in dvalue) and `per_pair`, the per-pair dicts of
    window_attention_bwd_ref (for the bounds).  The keywords plant defects:
      shifted_dS          guide q's dS is paired with guide q + 1's row (of the guides in dkey, of the keys' weights in dq) -- cyclic in the item
      first_group_only    only the first group of GUIDE_GROUP guides enters dkey (and the key-side term of dvalue)
      dq_into_neighbour   pair p's dq rows are summed into pair p + 1's dq_pair (cyclic over all pairs)
      key_grad_in_dvalue  False: the key-side term is missing from dvalue under value_is_key"""
    tok0, N, nw, pair0, row0 = pair_offsets(items, counts, H, W, ks)
    total, M, D = key.shape[0], guides.shape[0], key.shape[1]
    z = lambda n: torch.zeros(n, D, dtype=torch.float64)
    out = {"dq": z(dctx.shape[0]), "dq_pair": z(M), "dkey": z(total), "dvalue": z(total), "per_pair": []}
    for i, ((T, kt), Q) in enumerate(zip(items, counts)):
        idx = tok0[i] + torch.arange(N[i])
        per = []
        for q in range(Q):
            p = pair0[i] + q
            rows = slice(row0[p], row0[p] + nw[i])
            per.append(R.window_attention_bwd_ref(key[idx], value[idx], guides[p].expand(nw[i], D), dctx[rows], (T, H, W, kt, ks), scale, 0.0))
        out["per_pair"].extend(per)
        for q, o in enumerate(per):
            p = pair0[i] + q
            rows = slice(row0[p], row0[p] + nw[i])
            src = per[(q + 1) % Q] if shifted_dS else o
            K = key[idx][o["tok"]]
            out["dq"][rows] = torch.einsum("wi,wid->wd", src["dsk"] if shifted_dS else o["dsk"], K)
            out["dq_pair"][(p + 1) % M if dq_into_neighbour else p] += out["dq"][rows].sum(0)
            tokens = idx[o["tok"].reshape(-1)]
            dk = (o["dsk"][:, :, None] * guides[pair0[i] + (q + 1) % Q if shifted_dS else p][None, None, :]).reshape(-1, D)
            if first_group_only and q >= GUIDE_GROUP:
                dk = torch.zeros_like(dk)
            dv = (o["p"][:, :, None] * dctx[rows][:, None, :]).reshape(-1, D)
            if value_is_key:
                out["dvalue"][tokens] += dv + (dk if key_grad_in_dvalue else 0.0)
            else:
                out["dkey"][tokens] += dk
                out["dvalue"][tokens] += dv
    return out


def rmg_global_dx_ref(S, dS, ml, qt, dctx, N, counts, nh, dx0=None, drop_pass_offset=False):
    """S, dS: per item [>= nh Q_i, >= N_i] float64 (the item's row space); ml [M nh, 2], qt, dctx [M nh, E] pair-major; N the items' token
    counts.  Returns (dx [sum N_i, E], abs_terms, p per item).  drop_pass_offset plants the defect of the `32 pass` row offset dropped: row
    R of an item reads the coefficients of row R % 32 (the first pass's)."""
    dxs, abs_, ps, row = [], [], [], 0
    for i, (n, Q) in enumerate(zip(N, counts)):
        nr = nh * Q
        rows = slice(row, row + nr)
        Si, dSi = S[i][:nr], dS[i][:nr]
        if drop_pass_offset:
            fold = torch.arange(nr) % PASS_ROWS
            Si, dSi = Si[fold], dSi[fold]
        dx, ab, p = R.global_dx_ref(Si, dSi, ml[rows], qt[rows], dctx[rows], n)
        dxs.append(dx); abs_.append(ab); ps.append(p)
        row += nr
    dx, ab = torch.cat(dxs), torch.cat(abs_)
    if dx0 is not None:
        dx, ab = dx + dx0, ab + dx0.abs()
    return dx, ab, ps
