"""Helpers that run the HIP product path on a golden case (GPU tests / smoke)."""
import numpy as np
import torch

import hicom_amd
import window_attn_inputs as wi
from ops_reference import up


def dev_bf16(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).cuda()


def build_module(case, fp32_out=True):
    m = hicom_amd.build_vision_projector(case.cfg)
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in case.sd.items()}, strict=False)
    # (a clip-scale projector also owns `*_logit_scale` / `*_logit_bias`, reference projector.py:655-670: the synthetic state dicts do
    # not carry them, the tests give them through set_clip_logits())
    assert not unexpected and all("_logit_" in k for k in missing), (missing, unexpected)
    m = m.to(torch.bfloat16).cuda().eval()
    m.return_fp32 = fp32_out
    for sub in (m.local_compressor, m.global_compressor):
        if sub is not None:
            sub.return_fp32 = fp32_out
    return m


def run_native(case, fp32_out=True):
    m = build_module(case, fp32_out)
    ff, fe, g, nl = dev_bf16(case.ff), dev_bf16(case.fe), dev_bf16(case.g), dev_bf16(case.newline)
    with torch.no_grad():
        if case.logit is not None:
            ls, lb = (torch.tensor(v, device="cuda") for v in case.logit["local"])
            lo = m.local_compressor(ff, fe, g, case.modal, ls, lb)
            return {"local": lo}
        if case.anyres is not None:
            a = case.anyres
            fdict = {"base": None if a["no_base"] else ff[0], "patch": dev_bf16(a["patch_ff"])}
            edict = {"base": None if a["no_base"] else fe[0], "patch": dev_bf16(a["patch_fe"])}
            out = m(fdict, edict, g, case.modal, nl)
        else:
            out = m(ff, fe, g, case.modal, nl)
    torch.cuda.synchronize()
    return {"out": out}


def check_table_region(block, workspace, prepare, want):
    """prepare(block) on a real workspace filled with 0xff writes exactly `want` to its head: the ints behind it keep the fill."""
    n = workspace(block)
    ws = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    block.ws, block.ws_bytes, block.stream = ws.data_ptr(), n, torch.cuda.current_stream().cuda_stream
    prepare(block)
    got = ws[:4 * (len(want) + 64)].view(torch.int32).tolist()
    assert got[:len(want)] == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert got[len(want):] == [-1] * 64, "the table region is longer than the parent's"


# ---- raw launches of the multi-guide window kernels (tests/test_gpu_multi_window.py, tests/test_gpu_clip_stream_group_adapt.py) ---------------
DEV = "cuda"


def check(name, got, ref, tol):
    """|got - ref| <= tol elementwise (float64 on the CPU); the figures are printed first."""
    got, ref, tol = up(got), ref.double(), tol.double()
    assert got.shape == ref.shape == tol.shape, (name, got.shape, ref.shape, tol.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values in the result"
    err = (got - ref).abs()
    ratio = err / tol.clamp_min(1e-300)
    i = int(ratio.argmax())
    print(f"MULTI_WINDOW {name} err={float(err.max()):.3e} bound={float(tol.reshape(-1)[i]):.3e} ratio={float(ratio.reshape(-1)[i]):.3e}")
    assert bool((err <= tol).all()), f"{name}: error {float(err.reshape(-1)[i]):.3e} over its bound {float(tol.reshape(-1)[i]):.3e}"


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(t):
    """t [rows, D] as an interior view of a device buffer with a NaN row in front and behind (2304 bytes: 16-byte aligned); None stays."""
    if t is None:
        return None
    v = wi.guard_rows(t, DEV)
    assert v.data_ptr() % 16 == 0
    return v


def ptr(t):
    return None if t is None else t.data_ptr()


class SiglipHead(torch.nn.Module):
    """Stand-in with the attribute names of HF's SiglipMultiheadAttentionPoolingHead that encoder.py:284-285 touches."""
    def __init__(self, sd):
        super().__init__()
        import make_golden_head as mh                              # (tests/golden: the widths of the head's fixture)
        D, I = mh.D, mh.INTER
        self.layernorm = torch.nn.LayerNorm(D, eps=1e-6)
        self.mlp = torch.nn.Module()
        self.mlp.fc1 = torch.nn.Linear(D, I)
        self.mlp.fc2 = torch.nn.Linear(I, D)
        self.load_state_dict({k[len("head."):]: torch.from_numpy(v.copy()) for k, v in sd.items()})
