"""CPU checks of the host side of the multi-guide clip stream (hicom_amd/clip_stream.py: ClipStreamMulti, csrc/clip_stream.hip,
hicom_amd/native.py): the new symbols and the unchanged ABI version, the layout of the push argument block as the host C compiler sees it,
the C refusals (every one an argument check in front of the first launch), every Python refusal in front of any native call, the chunk row
offsets against HIComProjector._layout of the prefixes, the plan cache, and the (M, L) ping-pong.

As in tests/test_clip_stream_host.py the push-time checks and the plan cache need a stream object and no device: `host` opens one with the
device methods of ClipStreamMulti (_allocate, _prepare, _build_plan, _launch) replaced by recorders, and `nv` as clip_stream sees it replaced
by an object that fails the test when any native function is called."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import cases
from hicom_amd import clip_stream as cs
from hicom_amd import native as nv
from host_util import ADDR, EINVAL, EUNSUP, NoNative, module, tokens
from stream_blocks import MULTI_REFUSALS as C_REFUSALS, guides, multi_push_block as push_block


# ---- C refusals: none launches ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(C_REFUSALS))
def test_c_push_multi_refusals_in_front_of_any_device_call(name):
    over, code, needle = C_REFUSALS[name]
    got = nv.lib().hicom_compressor_stream_push_multi(ctypes.byref(push_block(**over)))
    msg = nv.lib().hicom_last_error().decode()
    assert got == code and msg.startswith("compressor_stream_push_multi: ") and needle in msg, (got, msg)
    assert nv.lib().hicom_compressor_stream_push_multi(None) == EINVAL


def test_c_fold_set_local_and_placement_refusals_in_front_of_any_device_call():
    L = nv.lib()
    fold = lambda **kw: L.hicom_stream_state_fold_set_fwd(*[kw.get(k, d) for k, d in (("ml", ADDR), ("acc", ADDR), ("rows", 27), ("E", 1152), ("ml_in", ADDR + 8192),
                                                                                    ("ml_out", ADDR + 4096), ("state", ADDR), ("stream", None))])
    for kw, needle in ((dict(ml=None), "NULL pointer"), (dict(rows=0), "bad shape"), (dict(E=1150), "bad shape"), (dict(acc=ADDR + 4), "aligned"),
                       (dict(ml_out=ADDR + 8192), "overlap"), (dict(ml_out=ADDR + 8192 + 208), "overlap")):
        assert fold(**kw) == EINVAL and needle in L.hicom_last_error().decode(), kw
    local = lambda **kw: L.hicom_multi_guide_local_fwd(*[kw.get(k, d) for k, d in (("key", ADDR), ("value", ADDR), ("guide", ADDR), ("Q", 3), ("T", 4), ("H", 6), ("W", 6),
                                                                                 ("E", 1152), ("kt", 4), ("ks", 3), ("scale", ctypes.c_float(0.03)), ("ctx", ADDR), ("stream", None))])
    for kw, code in ((dict(key=None), EINVAL), (dict(Q=33), EUNSUP), (dict(E=768), EUNSUP), (dict(T=6), EUNSUP), (dict(guide=ADDR + 2), EINVAL)):
        assert local(**kw) == code and L.hicom_last_error().decode().startswith("multi_guide_local: "), kw
    place = lambda **kw: L.hicom_stream_place_rows_fwd(*[kw.get(k, d) for k, d in (("loc", ADDR), ("tok", None), ("newline", None), ("Q", 3), ("windows", 4), ("hidden", 64),
                                                                                 ("nl_group", 0), ("nl_count", 0), ("nl_first", 0), ("nl_step", 1), ("rows", 4), ("global_row0", 4),
                                                                                 ("out", ADDR), ("out_dt", nv.DT_F32), ("ldo", 64), ("q_stride", 64 * 48), ("row0", 0),
                                                                                 ("stream", None))])
    for kw, code in ((dict(out=None), EINVAL), (dict(Q=33), EUNSUP), (dict(rows=6), EINVAL),            # global rows without their source
                     (dict(loc=None), EINVAL), (dict(row0=45), EINVAL), (dict(global_row0=3), EINVAL), (dict(out_dt=nv.DT_F16), EUNSUP)):
        assert place(**kw) == code and L.hicom_last_error().decode().startswith("stream_place_rows: "), kw


# ---- Python refusals, row offsets and the plan cache without a device ----------------------------------------------------------------------
@pytest.fixture
def host(monkeypatch):
    """Patches clip_stream for a device-less multi-guide stream; returns the list of launches (t0, row0, nl_group, newline rows, the (M, L)
    block read)."""
    launches = []
    M = cs.ClipStreamMulti
    monkeypatch.setattr(cs, "nv", NoNative())
    monkeypatch.setattr(cs, "_require_bf16_cuda", lambda name, t: None)
    monkeypatch.setattr(M, "_allocate", lambda self, rows: setattr(self, "out", torch.zeros((self.Q, rows, self.hidden))))
    monkeypatch.setattr(M, "_prepare", lambda self, g: (setattr(self, "guides", g), setattr(self, "cur", 0)))
    monkeypatch.setattr(M, "_build_plan", lambda self, Tc, has_fe: cs.StreamPlan(None, None, [], lambda: None))
    monkeypatch.setattr(M, "_launch", lambda self, plan, ff, fe, t0, row0, nl_group, nl_rows, stream: launches.append((t0, row0, nl_group, nl_rows, self.cur)))
    monkeypatch.setattr(M, "_finish_device", lambda self, row0, tail: launches.append(("finish", row0, tail, self.cur)))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: SimpleNamespace(cuda_stream=0))
    return launches


def test_open_refusals_come_before_any_native_call(monkeypatch):
    monkeypatch.setattr(cs, "nv", NoNative())
    with torch.no_grad():
        for m in (module(use_guide="coarse"), module("local43_adaptkv_global32"), module("local43_global32_adaptg"), module(use_clip_scale="local")):
            with pytest.raises(NotImplementedError, match="open_stream_multi is built for the plain release recipe"):
                m.open_stream_multi(guides(3), 6, 6, 16)
            assert cs.STORE_MULTI not in m.__dict__
        for dt in (torch.float16, torch.float32):
            with pytest.raises(NotImplementedError, match=str(dt)):
                module(dtype=dt).open_stream_multi(guides(3, dt), 6, 6, 16)
        m = module()
        for bad in (guides(0), guides(33)):
            with pytest.raises(ValueError, match=r"1 <= Q <= 32"):
                m.open_stream_multi(bad, 6, 6, 16)
        with pytest.raises(ValueError, match=r"guide_embeds is \[Q, E\]"):
            m.open_stream_multi(guides(3)[0], 6, 6, 16)                             # an [E] guide belongs to open_stream
        with pytest.raises(ValueError, match=r"guide_embeds is \[Q, E\]"):
            m.open_stream_multi(guides(3)[:, :-1], 6, 6, 16)
        with pytest.raises(NotImplementedError, match="guide_embed dtype"):
            m.open_stream_multi(guides(3, torch.float32), 6, 6, 16)
        with pytest.raises(NotImplementedError, match="partition the grid"):
            m.open_stream_multi(guides(3), 7, 6, 16)
        with pytest.raises(ValueError, match="multiple of the temporal window"):
            m.open_stream_multi(guides(3), 6, 6, 10)
        with pytest.raises(ValueError, match="needs image_newline"):
            module(mm_newline_position="grid").open_stream_multi(guides(3), 6, 6, 16)
        with pytest.raises(NotImplementedError, match="frame of logits in LDS"):
            m.open_stream_multi(guides(3), 150, 150, 16)                            # the merge kernels' limit on the grid
        with pytest.raises(nv.HicomNativeError, match="GPU only"):                  # everything in scope: the device check is the last one
            m.open_stream_multi(guides(3), 6, 6, 16)
        with pytest.raises(ValueError, match=r"guide_embed is \[E\]"):              # open_stream is as it was: a [Q, E] guide raises
            m.open_stream(guides(3), 6, 6, 16)
    m = module()
    with pytest.raises(RuntimeError, match="builds no autograd graph"):             # autograd on, trainable parameters
        m.open_stream_multi(guides(3), 6, 6, 16)


def test_push_finish_and_reset_refusals_come_before_any_native_call(host):
    m = module()
    with torch.no_grad():
        s = m.open_stream_multi(guides(3), 6, 6, 8)
        with pytest.raises(ValueError, match="ClipStreamMulti.finish: nothing has been pushed"):
            s.finish()
        for bad, exc, needle in ((tokens(3), ValueError, "whole window groups"), (tokens(6), ValueError, "whole window groups"),
                                 (tokens(4, H=3), ValueError, "opened for"), (tokens(12), ValueError, "exceed max_frames=8 of open_stream_multi"),
                                 (tokens(4, dtype=torch.float16), NotImplementedError, "float16"),
                                 ({"base": None, "patch": tokens(4)[0]}, NotImplementedError, "anyres")):
            with pytest.raises(exc, match=needle):
                s.push(bad, None)
        assert not host and s.frames == 0 and cs.STORE_MULTI not in m.__dict__
        s.push(tokens(4), tokens(4))
        with pytest.raises(ValueError, match="with frames_embed so far"):           # mixed with / without frames_embed
            s.push(tokens(4), None)
        with pytest.raises(ValueError, match="exceed max_frames"):
            s.push(tokens(8), tokens(8))
        for Q in (2, 4):
            with pytest.raises(ValueError, match="opened for Q=3"):
                s.reset(guides(Q))
        with pytest.raises(ValueError, match=r"guide_embeds is \[Q, E\]"):
            s.reset(guides(3)[0])
        assert len(host) == 1 and s.frames == 4
        s.reset(guides(3))                                                          # the same Q: a new clip
        assert s.frames == 0 and s.has_fe is None
        s.push(tokens(4), None)
    with pytest.raises(RuntimeError, match="builds no autograd graph"):
        s.push(tokens(4), None)
    with pytest.raises(RuntimeError, match="builds no autograd graph"):
        s.reset()
    assert len(host) == 2 and s.frames == 4
    long = module()
    with torch.no_grad():
        far = long.open_stream_multi(guides(2), 102, 102, 400)
        huge = torch.zeros((1, 1, 1, 1), dtype=torch.bfloat16).expand(168, 102, 102, cases.D)      # (a view: no memory behind it)
        with pytest.raises(NotImplementedError, match="push shorter chunks"):        # the merge kernels' limit on a chunk's frames: 164 at 102 x 102
            far.push(huge, None)
    assert len(host) == 2


@pytest.mark.parametrize("pos", ["grid", "frame", "one_token", "no_token"])
@pytest.mark.parametrize("chunking", [(4, 4, 4), (4, 8), (8, 4), (12,)])
def test_row_offsets_per_push_are_the_layout_of_the_prefixes(host, pos, chunking):
    m = module(mm_newline_position=pos)
    nl = None if pos == "no_token" else torch.zeros((64,), dtype=torch.bfloat16)
    with torch.no_grad():
        s = m.open_stream_multi(guides(3), 6, 6, 12, nl)
        assert tuple(s.out.shape) == (3, m._layout((3, 2, 2), "video", nl is not None, False).n_rows + 32, 64)
        groups = 0
        for n in chunking:
            view = s.push(tokens(n), None)
            before = m._layout((groups, 2, 2), "video", nl is not None, False) if groups else None
            after = m._layout((groups + n // 4, 2, 2), "video", nl is not None, False)
            tail = lambda lay: len(lay.newline_rows) if lay.nl_group == 0 else 0       # the whole-clip newline row belongs to finish()
            row0 = before.n_rows - tail(before) if before else 0
            row1 = after.n_rows - tail(after)
            t0, got_row0, nl_group, nl_rows, _ = host[-1]
            assert (t0, got_row0, nl_group) == (groups * 4, row0, after.nl_group)
            assert nl_rows == ([r for r in after.newline_rows if row0 <= r < row1] if after.nl_group else [])
            assert tuple(view.shape) == (3, row1 - row0, 64) and view.data_ptr() == s.out[:, row0:].data_ptr() and view.stride(0) == s.out.stride(0)
            groups += n // 4
        out = s.finish()
        whole = m._layout((3, 2, 2), "video", nl is not None, False)
        assert tuple(out.shape) == (3, whole.n_rows + 32, 64) and s.rows == whole.n_rows
        assert host[-1][:3] == ("finish", whole.n_rows - (1 if pos == "one_token" else 0), 1 if pos == "one_token" else 0)


def test_plans_are_shared_by_equal_chunks_and_streams_and_keyed_by_Q(host):
    m = module(mm_newline_position="grid")
    nl = torch.zeros((64,), dtype=torch.bfloat16)
    with torch.no_grad():
        s = m.open_stream_multi(guides(3), 6, 6, 16, nl)
        for _ in range(3):
            s.push(tokens(4), tokens(4))
        plans = m.__dict__[cs.STORE_MULTI]
        assert len(plans) == 1 and next(iter(plans.values())).hits == 3
        assert [(t0, row0) for t0, row0, *_ in host] == [(0, 0), (4, 6), (8, 12)]             # t0 and row0 are call arguments, not key
        assert host[1][2:4] == (2, [8, 11])
        assert [cur for *_, cur in host] == [0, 1, 0]                                         # the (M, L) block read alternates per push
        s.finish()
        assert host[-1] == ("finish", 18, 0, 1)                                               # finish() reads the block the last push wrote
        other = m.open_stream_multi(guides(3), 6, 6, 16, nl)                                  # a second stream of the module shares the plan
        other.push(tokens(4), tokens(4))
        assert len(plans) == 1 and next(iter(plans.values())).hits == 4 and host[-1][-1] == 0
        five = m.open_stream_multi(guides(5), 6, 6, 16, nl)                                   # another Q: a plan of its own
        five.push(tokens(4), tokens(4))
        assert len(plans) == 2
        other.push(tokens(8), tokens(8))                                                      # another chunk length
        assert len(plans) == 3
        s.reset()
        assert s.cur == 0
        s.push(tokens(4), None)                                                               # without frames_embed: a key of its own
        assert len(plans) == 4 and host[-1][:2] == (0, 0)
        assert cs.STORE not in m.__dict__                                                     # the single-guide stream's store is another one
    m._invalidate_plans()
    assert cs.STORE_MULTI not in m.__dict__
