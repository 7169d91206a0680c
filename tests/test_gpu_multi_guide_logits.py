"""The logits form of the multi-guide step on the GPU: hicom_multi_guide_local_logits_fwd against the float64 window
softmax, and HIComProjector.forward_multi_guide(local_logits=) against forward(local_logits=) per guide and against the keyed form.

Local kernel: the runs of tests/head_scores_inputs.py -- T = 1 windows of 9 tokens (three windows: one live wave in the last workgroup),
4 x 3 x 3 windows on 6 x 6 and on 27 x 27, Q = 1, 4, 5, 32, a family with a dominant logit per window and guide and one with near-equal
logits -- at the bounds tests/test_gpu_multi_window.py uses for its fp16 context planes (multi_window_inputs.bounds /
window_attn_inputs.forward_bounds_of).  The kernel receives the exact logits key_n . g_q rounded to fp32; the value rows are an interior
view between NaN rows, the logit planes lie q_stride = N + 5 floats apart with NaN between them, the output between two NaN guard planes.
tests/test_head_scores_power.py: uniform weights, guide 0's logits for all, a missing scale or the neighbouring window's logits miss these
bounds by a factor of 4 at least.

Step: 4 x 6 x 6 and 8 x 6 x 6, Q = 3, with and without image_newline; L[q] = frames_embed . g_q in float64, rounded to fp32.  out[q]
against forward(frames_feature, None, g_q, modal, nl, local_logits=L[q]) and against forward_multi_guide with frames_embed, both at the
2e-3 that tests/test_gpu_multi_guide.py holds the step to against forward(); the global rows equal the keyed form's bit for bit; the keyed
form called afterwards hits its own plan.

Measured on an MI355X: local kernel errors <= 9.8e-4, at most 0.19 of the bound; the step 1.0e-5 .. 2.3e-5 against forward(local_logits=) and
1.1e-7 .. 8.9e-6 against the keyed form."""
import pytest
import torch

import head_scores_inputs as hs
from gpu_util import DEV, check, guarded
from hicom_amd import native as nv
from ops_reference import up
from test_gpu_multi_guide import NG, STORE, VIDEO3, VIDEO3_NL, build_module, dev_bf16, mg_case

pytestmark = pytest.mark.gpu
NAN = float("nan")
D = hs.D
TOL_FORWARD = 2e-3


@pytest.mark.parametrize("run", hs.LOCAL_RUNS, ids=[r.id for r in hs.LOCAL_RUNS])
def test_local_logits_kernel_matches_the_fp64_window_softmax(run):
    b = hs.local_build(run)
    value = guarded(b.value)
    stride = b.N + 5
    lbuf = torch.full((b.Q, stride), NAN, dtype=torch.float32, device=DEV)
    lbuf[:, :b.N] = b.logits.to(DEV)
    buf = torch.full((b.Q + 2, b.NW, D), NAN, dtype=torch.float16, device=DEV)
    out = buf[1:-1]
    at, ay, ax = (nv.Axis(n, k, w, w) for n, k, w in b.axes)
    nv.multi_guide_local_logits(value.data_ptr(), lbuf.data_ptr(), stride, at, ay, ax, b.Q, b.NW, b.scale, out.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    check(f"logits.ctx16[{run.id}]", out, b.want, b.tol)
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all()), f"{run.id}: a guard plane was written"


def exact_logits(c):
    """[Q, T, H, W] fp32: frames_embed . g_q in float64, rounded once."""
    fe, g = up(torch.from_numpy(c.fe).bfloat16()), up(torch.from_numpy(c.g).bfloat16())
    return torch.einsum("thwd,qd->qthw", fe, g).float().to(DEV)


VIDEO3_T8 = (3, 8, 6, 6, "video", False)
VIDEO3_T8_NL = (3, 8, 6, 6, "video", True, (("mm_newline_position", "grid"),))


@pytest.mark.parametrize("key", [VIDEO3, VIDEO3_NL, VIDEO3_T8, VIDEO3_T8_NL], ids=["4x6x6", "4x6x6_newline", "8x6x6", "8x6x6_newline"])
def test_step_with_logits_against_forward_and_the_keyed_form(key):
    c = mg_case(*key)
    m = build_module(c)
    ff, fe, g, nl = dev_bf16(c.ff), dev_bf16(c.fe), dev_bf16(c.g), dev_bf16(c.newline)
    L = exact_logits(c)
    with torch.no_grad():
        keyed = m.forward_multi_guide(ff, fe, g, c.modal, nl)
        out = m.forward_multi_guide(ff, None, g, c.modal, nl, local_logits=L)
        plans = dict(m.__dict__[STORE])
        assert len(plans) == 2 and sum(k[-1] == "logits" for k in plans) == 1
        hits = {k: p.hits for k, p in plans.items()}
        again = m.forward_multi_guide(ff, fe, g, c.modal, nl)
        stored = dict(m.__dict__[STORE])
        # (forward() comes last: its executor plan may move the module's cached tables, which rebuilds every plan of every step)
        single = torch.stack([m(ff, None, g[q], c.modal, nl, local_logits=L[q]) for q in range(c.Q)])
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.shape == keyed.shape == single.shape
    e_single = [float((out[q] - single[q]).abs().max()) for q in range(c.Q)]
    e_keyed = [float((out[q] - keyed[q]).abs().max()) for q in range(c.Q)]
    print(f"forward_multi_guide(local_logits=) {key[:4]} newline={key[5]}: max-abs per guide vs forward(local_logits=) {['%.3e' % e for e in e_single]}, "
          f"vs the keyed form {['%.3e' % e for e in e_keyed]}")
    assert max(e_single) <= TOL_FORWARD and max(e_keyed) <= TOL_FORWARD
    assert torch.equal(out[:, -NG:], keyed[:, -NG:]), "the global rows changed"
    assert torch.equal(again, keyed)
    (keyed_key,) = [k for k in plans if k[-1] != "logits"]
    assert len(stored) == 2 and stored[keyed_key] is plans[keyed_key]
    assert plans[keyed_key].hits == hits[keyed_key] + 1 and [p.hits for k, p in plans.items() if k != keyed_key] == [hits[k] for k in plans if k != keyed_key]


def test_refusals_on_the_new_keyword_are_those_of_the_keyed_call():
    c = mg_case(*VIDEO3)
    m = build_module(c)
    ff, g = dev_bf16(c.ff), dev_bf16(c.g)
    L = exact_logits(c)
    with pytest.raises(RuntimeError, match="autograd"):
        m.forward_multi_guide(ff, None, g, c.modal, None, local_logits=L)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="float16"):
            m.forward_multi_guide(ff.half(), None, g, c.modal, None, local_logits=L)
        with pytest.raises(NotImplementedError, match="float16"):
            m.forward_multi_guide(ff, None, g.half(), c.modal, None, local_logits=L)
        with pytest.raises(ValueError, match="float32"):
            m.forward_multi_guide(ff, None, g, c.modal, None, local_logits=L.double())
        with pytest.raises(ValueError, match="device tensor"):
            m.forward_multi_guide(ff, None, g, c.modal, None, local_logits=L.cpu())
        with pytest.raises(ValueError, match="frames_embed=None"):
            m.forward_multi_guide(ff, dev_bf16(c.fe), g, c.modal, None, local_logits=L)
    assert STORE not in m.__dict__ or not m.__dict__[STORE], "a refused call built a plan"
