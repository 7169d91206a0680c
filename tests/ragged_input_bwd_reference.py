"""Plain float64 restatements of the two entry points behind forward_ragged_train(input_grads=True) (torch on the CPU; no call into
hicom_amd), beside tests/ops_reference.py, whose per-item references they are built on:

  ragged_local_bwd_ref    hicom_compressor_ragged_local_bwd: ops_reference.window_attention_bwd_ref per item on the item's own grid
                          (T_i, H, W, kt_i, ks), its tokens at tok0_i, its guide row as the query of all its windows
  ragged_global_dx_ref    hicom_compressor_ragged_global_dx: ops_reference.global_dx_ref per item on the item's rows i nh .. (i + 1) nh

Shared by tests/test_gpu_ragged_input_bwd.py (the kernels against these) and tests/test_ragged_input_bwd_power.py (these against float64
autograd of a small model of the two stages, and the defects a segmented kernel can have, planted through the keywords)."""
import torch

import ops_reference as R


def offsets(items, H, W, ks):
    """(tok0, N, win0, windows) per item; items: (T, kt) pairs."""
    wps = (H // ks) * (W // ks)
    N = [T * H * W for T, _ in items]
    w = [(T // kt) * wps for T, kt in items]
    pre = lambda v: [sum(v[:i]) for i in range(len(v))]
    return pre(N), N, pre(w), w


def ragged_local_bwd_ref(key, value, guides, dctx, items, H, W, ks, scale, value_is_key=False, neighbour_guide=False, drop_tok0=False,
                         clip_kt=None, key_grad_in_dvalue=True):
    """key, value [sum N_i, D], guides [B, D], dctx [sum w_i, D], all float64.  Returns a dict: dq [sum w_i, D], dq_item [B, D], dkey,
    dvalue [sum N_i, D] (dkey zero with value_is_key: the key-side rows are in dvalue) and `per_item`, the per-item dicts of
    window_attention_bwd_ref (for the bounds).  The keywords plant defects:
      neighbour_guide     item i's windows take the guide of item i + 1
      drop_tok0           the item's rows are read from (and its gradients written to) the stack's first tokens
      clip_kt             an item shorter than clip_kt frames has its window geometry built with that temporal window (and as many frames):
                          its windows run on into the next item's tokens (wrapping at the stack's end)
      key_grad_in_dvalue  False: the key-side term is missing from dvalue under value_is_key"""
    tok0, N, win0, nw = offsets(items, H, W, ks)
    total, B, D = key.shape[0], len(items), key.shape[1]
    out = {"dq": torch.zeros(sum(nw), D, dtype=torch.float64), "dq_item": torch.zeros(B, D, dtype=torch.float64),
           "dkey": torch.zeros(total, D, dtype=torch.float64), "dvalue": torch.zeros(total, D, dtype=torch.float64), "per_item": []}
    for i, (T, kt) in enumerate(items):
        first = 0 if drop_tok0 else tok0[i]
        Tg, ktg = (clip_kt, clip_kt) if (clip_kt is not None and T < clip_kt) else (T, kt)
        idx = (first + torch.arange(Tg * H * W)) % total
        q = guides[(i + 1) % B if neighbour_guide else i]
        nwin = (Tg // ktg) * (H // ks) * (W // ks)
        o = R.window_attention_bwd_ref(key[idx], value[idx], q.expand(nwin, D), dctx[win0[i]:win0[i] + nwin], (Tg, H, W, ktg, ks), scale, 0.0,
                                       value_is_key=value_is_key, key_grad_in_dvalue=key_grad_in_dvalue)
        out["dq"][win0[i]:win0[i] + nwin] = o["dq"]
        out["dq_item"][i] = o["dq"].sum(0)
        if not value_is_key:
            out["dkey"][idx] = o["dkey"]
        out["dvalue"][idx] = o["dvalue"]
        out["per_item"].append(o)
    return out


def ragged_global_dx_ref(S, dS, ml, qt, dctx, N, nh, dx0=None, flat_tiles=None):
    """S, dS: per item [>= nh, >= N_i] float64; ml [B nh, 2], qt, dctx [B nh, E]; N the items' token counts.  Returns (dx [sum N_i, E],
    abs_terms, p per item).  flat_tiles=64 plants the defect of tiles counted from the STACK's first token: the tile that straddles an item
    edge keeps the rows (qt, dctx, M, L) of the item it started in, and its tail reads the next item's coefficients."""
    dxs, abs_, ps = [], [], []
    for i, n in enumerate(N):
        rows = slice(i * nh, (i + 1) * nh)
        dx, ab, p = R.global_dx_ref(S[i], dS[i], ml[rows], qt[rows], dctx[rows], n)
        dxs.append(dx); abs_.append(ab); ps.append(p)
    dx, ab = torch.cat(dxs), torch.cat(abs_)
    if flat_tiles:
        t0 = 0
        for i, n in enumerate(N[:-1]):
            edge = t0 + n                                          # first token of item i + 1
            tail_end = min((edge + flat_tiles - 1) // flat_tiles * flat_tiles, edge + N[i + 1])
            if edge % flat_tiles and tail_end > edge:
                k = tail_end - edge                                # tokens of item i + 1 inside item i's last tile
                rows = slice(i * nh, (i + 1) * nh)
                p = torch.exp(S[i + 1][:nh, :k] - ml[rows][:, 0:1]) / ml[rows][:, 1:2]
                dx[edge:tail_end] = dS[i + 1][:nh, :k].t() @ qt[rows] + p.t() @ dctx[rows]
            t0 = edge
    if dx0 is not None:
        dx, ab = dx + dx0, ab + dx0.abs()
    return dx, ab, ps


def tile_walk(N, tile=64):
    """Brute force: for every token of the stack, (item, first token of its tile inside the item), token by token."""
    out = []
    for i, n in enumerate(N):
        for t in range(n):
            out.append((i, t - t % tile))
    return out
