"""CPU checks of the host side of the multi-guide clip stream on the k / v adaptor recipe (hicom_amd/clip_stream.py: ClipStreamAdapt,
csrc/clip_stream.hip, csrc/multi_guide.hip, hicom_amd/native.py): the new symbols and the unchanged ABI version, the layout of the new
argument block as the host C compiler sees it, the C refusals of both new entry points (every one an argument check in front of the first
launch), every Python refusal in front of any native call, the routing of a plain module, the plan key, the per-push patching and the
plan's refresh.

As in tests/test_clip_stream_multi_host.py the push-time checks and the plan cache need a stream object and no device: `host` opens one with
the device methods replaced by recorders and `nv` as clip_stream sees it replaced by an object that fails the test when any native function
is called."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import cases
import hicom_amd
from hicom_amd import clip_stream as cs
from hicom_amd import native as nv
from hicom_amd import segments as seg
from host_util import ADDR, EINVAL, EUNSUP, NoNative, module, tokens
from stream_blocks import ADAPTKV, ADAPT_REFUSALS, MULTI_REFUSALS as PLAIN_REFUSALS, adapt_block, adaptor, guides, multi_push_block as plain_block


# ---- C refusals: none launches ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(ADAPT_REFUSALS))
def test_c_push_adapt_refusals_of_the_new_parts_in_front_of_any_device_call(name):
    over, code, needle = ADAPT_REFUSALS[name]
    got = nv.lib().hicom_compressor_stream_push_multi_adapt(ctypes.byref(adapt_block(**over)))
    msg = nv.lib().hicom_last_error().decode()
    assert got == code and needle in msg, (got, msg)


@pytest.mark.parametrize("name", list(PLAIN_REFUSALS))
def test_c_push_adapt_makes_every_refusal_of_the_plain_push(name):
    """The shared body: the table of tests/test_clip_stream_multi_host.py against the adaptor entry, under the adaptor entry's name."""
    over, code, needle = PLAIN_REFUSALS[name]
    got = nv.lib().hicom_compressor_stream_push_multi_adapt(ctypes.byref(adapt_block(base=over)))
    msg = nv.lib().hicom_last_error().decode()
    assert got == code and msg.startswith("compressor_stream_push_multi_adapt: ") and needle in msg, (got, msg)


def test_c_push_adapt_null_arguments_and_the_plain_entry_keeps_its_name():
    L = nv.lib()
    assert L.hicom_compressor_stream_push_multi_adapt(None) == EINVAL
    assert L.hicom_last_error().decode() == "compressor_stream_push_multi_adapt: NULL arguments"
    assert L.hicom_compressor_stream_push_multi(None) == EINVAL
    assert L.hicom_last_error().decode() == "compressor_stream_push_multi: NULL arguments"
    assert L.hicom_compressor_stream_push_multi(ctypes.byref(plain_block(Q=33))) == EUNSUP
    assert L.hicom_last_error().decode().startswith("compressor_stream_push_multi: Q=33")


def test_c_local_adapt_refusals_in_front_of_any_device_call():
    L = nv.lib()
    ak, av = adaptor(), adaptor()
    order = (("key", ADDR), ("value", ADDR), ("guide", ADDR), ("ky", ADDR), ("vy", ADDR), ("ak", ctypes.byref(ak)), ("av", ctypes.byref(av)),
             ("alpha_dt", nv.DT_BF16), ("eps", ctypes.c_float(1e-6)), ("Q", 3), ("T", 4), ("H", 6), ("W", 6), ("E", 1152), ("kt", 4), ("ks", 3),
             ("scale", ctypes.c_float(0.03)), ("ctx", ADDR), ("stream", None))
    local = lambda **kw: L.hicom_multi_guide_local_adapt_fwd(*[kw.get(k, d) for k, d in order])
    for kw, code, needle in ((dict(key=None), EINVAL, "NULL pointer"), (dict(ctx=None), EINVAL, "NULL pointer"), (dict(ak=None), EINVAL, "NULL arguments"),
                             (dict(ky=None, vy=None), EINVAL, "neither stream has a prepared plane"), (dict(ky=ADDR + 8), EINVAL, "16-byte aligned planes"),
                             (dict(Q=33), EUNSUP, "1 <= Q <= 32"), (dict(Q=0), EUNSUP, "1 <= Q <= 32"), (dict(E=768), EUNSUP, "only 1152"),
                             (dict(T=6), EUNSUP, "exact partition"), (dict(T=8, kt=8), EUNSUP, "<= 64 tokens"), (dict(guide=ADDR + 2), EINVAL, "16-byte aligned inputs"),
                             (dict(alpha_dt=nv.DT_F16), EINVAL, "alpha dtype"), (dict(av=ctypes.byref(adaptor(beta=None))), EINVAL, "adaptor weights")):
        got = local(**kw)
        msg = L.hicom_last_error().decode()
        assert got == code and msg.startswith("multi_guide_local_adapt: ") and needle in msg, (kw, got, msg)
    # a stream without plane needs no LayerNorm parameters: the check passes them by (nothing is launched: the next refusal is reached)
    assert local(ky=None, ak=ctypes.byref(adaptor(gamma=None)), Q=33) == EUNSUP


# ---- Python refusals, routing, the plan key and the per-push patching without a device ---------------------------------------------------
@pytest.fixture
def host(monkeypatch):
    """Patches clip_stream for device-less streams of both multi-guide classes; returns the list of launches (class, t0, row0, nl_group,
    newline rows, the (M, L) block read)."""
    launches = []
    monkeypatch.setattr(cs, "nv", NoNative())
    monkeypatch.setattr(cs, "_require_bf16_cuda", lambda name, t: None)
    M = cs.ClipStreamMulti
    monkeypatch.setattr(M, "_allocate", lambda self, rows: setattr(self, "out", torch.zeros((self.Q, rows, self.hidden))))
    monkeypatch.setattr(M, "_prepare", lambda self, g: (setattr(self, "guides", g), setattr(self, "cur", 0)))
    monkeypatch.setattr(M, "_finish_device", lambda self, row0, tail: launches.append(("finish", row0, tail, self.cur)))
    for cls in (M, cs.ClipStreamAdapt):
        monkeypatch.setattr(cls, "_build_plan", lambda self, Tc, has_fe: cs.StreamPlan(None, None, [], lambda: None))
        monkeypatch.setattr(cls, "_launch", lambda self, plan, ff, fe, t0, row0, nl_group, nl_rows, stream:
                            launches.append((type(self).__name__, t0, row0, nl_group, nl_rows, self.cur)))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: SimpleNamespace(cuda_stream=0))
    return launches


def test_open_refusals_come_before_any_native_call(monkeypatch):
    monkeypatch.setattr(cs, "nv", NoNative())
    with torch.no_grad():
        for m in (module(ADAPTKV, use_guide="coarse"), module(ADAPTKV, use_clip_scale="local"), module("local43_adaptqkv_global32", use_guide="coarse"),
                  module("local43_adaptkv_global32_adaptg"), module("local43_global32_adaptg")):
            with pytest.raises(NotImplementedError, match="open_stream_adapt is built for the two release recipes only"):
                m.open_stream_adapt(guides(3), 6, 6, 16)
            assert cs.STORE_ADAPT not in m.__dict__
        for dt in (torch.float16, torch.float32):
            with pytest.raises(NotImplementedError, match=str(dt)):
                module(ADAPTKV, dtype=dt).open_stream_adapt(guides(3, dt), 6, 6, 16)
        m = module(ADAPTKV)
        for bad in (guides(0), guides(33)):
            with pytest.raises(ValueError, match=r"open_stream_adapt: .*1 <= Q <= 32"):
                m.open_stream_adapt(bad, 6, 6, 16)
        with pytest.raises(ValueError, match=r"guide_embeds is \[Q, E\]"):
            m.open_stream_adapt(guides(3)[0], 6, 6, 16)
        with pytest.raises(NotImplementedError, match="guide_embed dtype"):
            m.open_stream_adapt(guides(3, torch.float32), 6, 6, 16)
        with pytest.raises(NotImplementedError, match="partition the grid"):
            m.open_stream_adapt(guides(3), 7, 6, 16)
        with pytest.raises(ValueError, match="multiple of the temporal window"):
            m.open_stream_adapt(guides(3), 6, 6, 10)
        with pytest.raises(ValueError, match="needs image_newline"):
            module(ADAPTKV, mm_newline_position="grid").open_stream_adapt(guides(3), 6, 6, 16)
        with pytest.raises(NotImplementedError, match="frame of logits in LDS"):
            m.open_stream_adapt(guides(3), 150, 150, 16)
        with pytest.raises(nv.HicomNativeError, match="GPU only"):                  # everything in scope: the device check is the last one
            m.open_stream_adapt(guides(3), 6, 6, 16)
        # the earlier entries keep their refusals of the adaptor recipe word for word
        with pytest.raises(NotImplementedError, match="open_stream_multi is built for the plain release recipe only"):
            m.open_stream_multi(guides(3), 6, 6, 16)
        with pytest.raises(NotImplementedError, match="open_stream is built for the plain release recipe only"):
            m.open_stream(guides(3)[0], 6, 6, 16)
    with pytest.raises(RuntimeError, match="builds no autograd graph"):             # autograd on, trainable parameters
        module(ADAPTKV).open_stream_adapt(guides(3), 6, 6, 16)


def test_adaptor_widths_and_the_chunk_limit_are_checked_on_the_host(host):
    with torch.no_grad():
        m = module(ADAPTKV)
        lin = m.local_compressor.k_proj[0]
        lin.weight = torch.nn.Parameter(torch.zeros((cases.D, cases.D - 32), dtype=torch.bfloat16))
        with pytest.raises(NotImplementedError, match="adaptor widths must be multiples of 64"):
            m.open_stream_adapt(guides(3), 6, 6, 16)
        # 4 frames of 1026 x 1026 tokens of 1152 channels are 2^32.2 elements.  (With the positional term the merge's LDS limits on a chunk
        # bind first at every grid; without it they do not apply.)
        big = module(ADAPTKV)
        big.global_compressor.use_pos_emb = False
        with pytest.raises(NotImplementedError, match="below 2\\^32 elements"):
            big.open_stream_adapt(guides(2), 1026, 1026, 8)
        s = big.open_stream_adapt(guides(2), 510, 510, 16)                          # 4 frames fit (2^30.2), 16 frames do not
        huge = torch.zeros((1, 1, 1, 1), dtype=torch.bfloat16).expand(16, 510, 510, cases.D)
        with pytest.raises(NotImplementedError, match="ClipStreamAdapt.push: .*push shorter chunks"):
            s.push(huge, None)
    assert not host


def test_a_plain_module_is_routed_to_the_multi_guide_stream(host):
    with torch.no_grad():
        s = module().open_stream_adapt(guides(3), 6, 6, 8)
        assert type(s) is cs.ClipStreamMulti and s.WHAT == "open_stream_multi"
        a = module(ADAPTKV).open_stream_adapt(guides(3), 6, 6, 8)
        assert type(a) is cs.ClipStreamAdapt and a.RECIPE == "adaptkv" and s.RECIPE == "plain"
        for ptype in ("local43_adaptk_global32", "local43_adaptv_global32"):
            assert type(module(ptype).open_stream_adapt(guides(3), 6, 6, 8)) is cs.ClipStreamAdapt
        s.push(tokens(4), None)
        a.push(tokens(4), None)
    assert [l[0] for l in host] == ["ClipStreamMulti", "ClipStreamAdapt"]
    assert cs.STORE_MULTI in s.proj.__dict__ and cs.STORE_ADAPT not in s.proj.__dict__
    assert cs.STORE_ADAPT in a.proj.__dict__ and cs.STORE_MULTI not in a.proj.__dict__


def test_push_refusals_and_a_module_that_leaves_the_recipe(host):
    m = module(ADAPTKV)
    with torch.no_grad():
        s = m.open_stream_adapt(guides(3), 6, 6, 8)
        with pytest.raises(ValueError, match="ClipStreamAdapt.finish: nothing has been pushed"):
            s.finish()
        for bad, exc, needle in ((tokens(3), ValueError, "whole window groups"), (tokens(4, H=3), ValueError, "opened for"),
                                 (tokens(12), ValueError, "exceed max_frames=8 of open_stream_adapt"),
                                 (tokens(4, dtype=torch.float16), NotImplementedError, "float16"),
                                 ({"base": None, "patch": tokens(4)[0]}, NotImplementedError, "anyres")):
            with pytest.raises(exc, match=needle):
                s.push(bad, None)
        assert not host and s.frames == 0 and cs.STORE_ADAPT not in m.__dict__
        s.push(tokens(4), tokens(4))
        with pytest.raises(ValueError, match="with frames_embed so far"):
            s.push(tokens(4), None)
        with pytest.raises(ValueError, match="opened for Q=3"):
            s.reset(guides(2))
        m.local_compressor.adapt_k = m.local_compressor.adapt_v = False             # the module turns into the plain recipe
        with pytest.raises(NotImplementedError, match=r"left the scope of open_stream_adapt \(the k / v adaptor release recipe, bfloat16\)"):
            s.push(tokens(4), tokens(4))
    assert len(host) == 1 and s.frames == 4


def test_plan_key_patching_and_sharing(host):
    m = module(ADAPTKV, mm_newline_position="grid")
    nl = torch.zeros((64,), dtype=torch.bfloat16)
    with torch.no_grad():
        s = m.open_stream_adapt(guides(3), 6, 6, 16, nl)
        for _ in range(3):
            s.push(tokens(4), tokens(4))
        plans = m.__dict__[cs.STORE_ADAPT]
        (key,) = plans
        assert key[:2] == (3, 4) and key[-2:] == (True, True), "ClipStreamMulti's key, then the adaptor set"
        assert key[:-2] == cs.ClipStreamMulti._plan_key(s, 4, True, 0)
        assert len(plans) == 1 and plans[key].hits == 3
        assert [(t0, row0) for _, t0, row0, *_ in host] == [(0, 0), (4, 6), (8, 12)]          # t0 and row0 are call arguments, not key
        assert host[1][3:5] == (2, [8, 11])
        assert [cur for *_, cur in host] == [0, 1, 0]                                         # the (M, L) block read alternates per push
        s.finish()
        assert host[-1] == ("finish", 18, 0, 1)
        other = m.open_stream_adapt(guides(3), 6, 6, 16, nl)                                  # a second stream of the module shares the plan
        other.push(tokens(4), tokens(4))
        assert len(plans) == 1 and plans[key].hits == 4 and host[-1][-1] == 0
        m.open_stream_adapt(guides(5), 6, 6, 16, nl).push(tokens(4), tokens(4))               # another Q
        other.push(tokens(8), tokens(8))                                                      # another chunk length
        s.reset()
        s.push(tokens(4), None)                                                               # without frames_embed
        assert len(plans) == 4 and host[-1][1:3] == (0, 0)
        m.local_compressor.adapt_v = False                                                    # another adaptor set: a key of its own
        s.reset()
        s.push(tokens(4), None)
        assert len(plans) == 5 and sorted(k[-2:] for k in plans)[0] == (True, False)
        assert cs.STORE not in m.__dict__ and cs.STORE_MULTI not in m.__dict__
    m._invalidate_plans()
    assert cs.STORE_ADAPT not in m.__dict__


def test_build_plan_fills_the_adaptor_block_and_its_refresh_reaches_refresh_adaptors(monkeypatch):
    """_build_plan and _launch themselves, with the three native functions and the allocation they use replaced: the planes and the hidden
    planes lie behind the parent's regions in ONE workspace, a stream without adaptor has no plane, refresh rebuilds the readout copies
    and the adaptors' fp16 copies, and a push patches the plain block inside the adaptor block."""
    calls, pushed = [], []
    fake = SimpleNamespace(**{n: getattr(nv, n) for n in ("StreamPushMultiAdaptArgs", "StreamPushMultiArgs", "DT_F32", "DT_BF16")},
                           global_stream_nparts=lambda N, RP: 4, global_stream_has_marg=lambda *a: 1, global_stream_marg_width=lambda H, W: 16,
                           clip_adapt_prepare_workspace=lambda N, E, ak, av, what: (bool(ak.w0) + bool(av.w0)) * N * E * 2,
                           compressor_stream_push_multi_adapt=lambda args: pushed.append(args))
    monkeypatch.setattr(cs, "nv", fake)
    monkeypatch.setattr(cs, "_require_bf16_cuda", lambda name, t: None)
    monkeypatch.setattr(cs.ClipStreamMulti, "_allocate", lambda self, rows: setattr(self, "out", torch.zeros((self.Q, rows, self.hidden))))
    monkeypatch.setattr(cs.ClipStreamMulti, "_prepare", lambda self, g: (setattr(self, "guides", g), setattr(self, "cur", 0)))

    def fill(a, lc, what, ptr):
        calls.append(("fill", what))
        a.ak.w0 = ADDR if lc.adapt_k else None
        a.av.w0 = ADDR if lc.adapt_v else None
        a.alpha_dt, a.eps = nv.DT_BF16, 1e-6
    monkeypatch.setattr(seg, "fill_adaptors", fill)
    monkeypatch.setattr(seg, "refresh_adaptors", lambda lc: calls.append(("refresh_adaptors", lc)))
    monkeypatch.setattr(hicom_amd.projector, "_linear_params", lambda lin: (lin.weight, lin.bias))
    for ptype, has_k, has_v in ((ADAPTKV, True, True), ("local43_adaptk_global32", True, False), ("local43_adaptv_global32", False, True)):
        m = module(ptype)
        lc = m.local_compressor
        monkeypatch.setattr(type(lc), "readout_f16", lambda self: (calls.append(("readout_f16",)), (torch.zeros(1), torch.zeros(1)))[1])
        with torch.no_grad():
            s = m.open_stream_adapt(guides(3), 6, 6, 16)
            s.device, s.pos_a, s.pe, s.P, s.y0, s.x0 = "cpu", None, None, 0, 0, 0
            s.q_hi = s.q_lo = s.state_acc = torch.zeros(4)
            s.state_ml = torch.zeros((2, 27, 2))
            del calls[:]
            plan = s._build_plan(4, True)
        args = plan.args
        assert isinstance(args, nv.StreamPushMultiAdaptArgs) and calls[0] == ("fill", "open_stream_adapt")
        a, plane, base0 = args.base, 144 * cases.D * 2, plan.ws.data_ptr()
        assert (a.Q, a.Tc, a.nh, a.hidden) == (3, 4, 9, 64)
        regions = [args.ky if has_k else None, args.vy if has_v else None, args.adapt_ws]
        assert (args.ky is not None) == has_k and (args.vy is not None) == has_v
        assert args.adapt_ws_bytes == (has_k + has_v) * plane
        at = a.loc + 3 * 4 * 64 * 2                                                  # behind the parent's last region ([Q windows, hidden] bf16)
        for r, n in zip(regions, (plane * has_k, plane * has_v, args.adapt_ws_bytes)):
            if r is not None:
                assert r >= at and (r - base0) % 256 == 0 and r + n <= base0 + plan.ws.numel(), "an adaptor region inside the one workspace"
                at = r + n
        del calls[:]
        plan.refresh()
        assert calls == [("readout_f16",), ("refresh_adaptors", lc)]
        ff, fe = tokens(4), tokens(4)
        s.cur = 1
        s._launch(plan, ff, fe, 8, 12, 0, [], 7)
        assert pushed[-1] is args and (a.ff, a.fe, a.t0, a.row0, a.stream) == (ff.data_ptr(), fe.data_ptr(), 8, 12, 7)
        assert a.state_ml_in == s.state_ml[1].data_ptr() and a.state_ml_out == s.state_ml[0].data_ptr() and a.q_stride == s.out.stride(0)
