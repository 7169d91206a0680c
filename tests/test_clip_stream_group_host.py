"""CPU checks of the host side of the clip stream group (hicom_amd/clip_stream_group.py, csrc/clip_stream_group.hip, hicom_amd/native.py):
the new symbols and the unchanged ABI version, the layout of the push block as the host C compiler sees it, every refusal in front of any
device work -- of the C entry points with made-up aligned addresses that nothing reads before a launch, of the Python object with `nv`
replaced by an object that fails the test when a native function is called -- and the plan cache keyed by the tuple of chunk lengths."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from hicom_amd import clip_stream as cs
from hicom_amd import clip_stream_group as csg
from hicom_amd import native as nv
from host_util import ADDR, EINVAL, EUNSUP, NoNative, module, tokens
from stream_blocks import GROUP_REFUSALS as C_REFUSALS, group_push_block as push_block, guides


# ---- C refusals: none launches ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(C_REFUSALS))
def test_c_push_refusals_in_front_of_any_device_call(name):
    over, code, needle = C_REFUSALS[name]
    L = nv.lib()
    got = L.hicom_compressor_stream_group_push(ctypes.byref(push_block(over)))
    msg = L.hicom_last_error().decode()
    assert got == code and msg.startswith("compressor_stream_group: ") and needle in msg, (got, msg)
    assert L.hicom_compressor_stream_group_push(None) == EINVAL and L.hicom_compressor_stream_group_prepare(None) == EINVAL


def test_workspace_bytes_follow_the_tuple_and_refuse_like_the_push():
    L = nv.lib()
    one = L.hicom_compressor_stream_group_workspace_bytes(ctypes.byref(push_block()))
    two = L.hicom_compressor_stream_group_workspace_bytes(ctypes.byref(push_block({("tc", 1): 4})))
    assert one > two > 0 and one % 256 == 0
    assert one == L.hicom_compressor_stream_group_workspace_bytes(ctypes.byref(push_block({("slot", 0): 1, ("t0", 2): 4})))   # not the per-push fields
    assert L.hicom_compressor_stream_group_workspace_bytes(ctypes.byref(push_block({"B": 33}))) == EUNSUP
    assert L.hicom_compressor_stream_group_workspace_bytes(None) == EINVAL


def test_merge_fold_refusals_in_front_of_any_device_call():
    L = nv.lib()
    ia = lambda *v: (ctypes.c_int32 * len(v))(*v)
    order = (("pm", ADDR), ("pl", ADDR), ("pa", ADDR), ("scores", ADDR), ("items", 3), ("nparts", 3), ("rows", 9), ("E", 1152), ("Tc", 4), ("H", 6), ("W", 6),
             ("pe", ADDR), ("P", 28), ("y0", 16), ("x0", 22), ("slot", ia(2, 0, 1)), ("t0", ia(8, 0, 4)), ("B", 4), ("ml", ADDR), ("acc", ADDR), ("stream", None))
    fold = lambda **kw: L.hicom_stream_group_merge_fold_fwd(*[kw.get(k, d) for k, d in order])
    for kw, code, needle in ((dict(pm=None), EINVAL, "NULL pointer"), (dict(rows=17), EINVAL, "bad shape"), (dict(E=1150), EINVAL, "bad shape"),
                             (dict(nparts=0), EINVAL, "bad shape"), (dict(B=33), EUNSUP, "1 <= B <= 32"), (dict(items=5), EINVAL, "bad shape"),
                             (dict(pa=ADDR + 4), EINVAL, "aligned"), (dict(scores=None), EINVAL, "needs the logits"),
                             (dict(slot=ia(2, 0, 2)), EINVAL, "appears twice"), (dict(slot=ia(2, 0, 4)), EINVAL, "0 <= slot < B = 4"),
                             (dict(t0=ia(8, 0, 16)), EINVAL, "outside the positional tables"), (dict(P=27), EINVAL, "outside the positional tables"),
                             (dict(Tc=1024, H=32, W=32, y0=4096, x0=4128, P=4160), EUNSUP, "marginal sums in LDS")):
        got = fold(**kw)
        assert got == code and needle in L.hicom_last_error().decode(), (kw, got, L.hicom_last_error().decode())


# ---- Python refusals and the plan cache without a device -------------------------------------------------------------------------------
@pytest.fixture
def host(monkeypatch):
    """Patches the group for a device-less object; returns the list of launches (slots, t0s, row0s) and of the plans built (tuples)."""
    launches, built = [], []
    monkeypatch.setattr(csg, "nv", NoNative())
    monkeypatch.setattr(cs, "nv", NoNative())
    monkeypatch.setattr(cs, "_require_bf16_cuda", lambda name, t: None)
    G = csg.ClipStreamGroup
    monkeypatch.setattr(G, "_allocate", lambda self, rows: setattr(self, "out", torch.zeros((self.Q, rows, self.hidden))))
    monkeypatch.setattr(G, "_prepare", lambda self, guides, slot=None: setattr(self, "guides", guides) if slot is None else None)
    monkeypatch.setattr(G, "_build_plan", lambda self, tcs, has_fe, stream=None: (built.append(tcs), cs.StreamPlan(None, None, [], lambda: None))[1])
    monkeypatch.setattr(G, "_launch", lambda self, plan, ff, fe, slots, t0s, row0s, stream: launches.append((tuple(slots), tuple(t0s), tuple(row0s))))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: SimpleNamespace(cuda_stream=0))
    return SimpleNamespace(launches=launches, built=built)


def test_open_refusals_come_before_any_native_call(monkeypatch):
    monkeypatch.setattr(csg, "nv", NoNative())
    monkeypatch.setattr(cs, "nv", NoNative())
    with torch.no_grad():
        for m in (module(use_guide="coarse"), module("local43_adaptkv_global32"), module("local43_global32_adaptg"), module(use_clip_scale="local")):
            with pytest.raises(NotImplementedError, match="open_stream_group is built for the plain release recipe only"):
                m.open_stream_group(guides(3), 6, 6, 16)
            assert csg.STORE_GROUP not in m.__dict__
        for dt in (torch.float16, torch.float32):
            with pytest.raises(NotImplementedError, match=str(dt)):
                module(dtype=dt).open_stream_group(guides(3).to(dt), 6, 6, 16)
        m = module()
        for B in (0, 33):
            with pytest.raises(ValueError, match=f"Q={B} guides"):
                m.open_stream_group(guides(B), 6, 6, 16)
        with pytest.raises(ValueError, match=r"guide_embeds is \[Q, E\]"):
            m.open_stream_group(guides(3)[0], 6, 6, 16)
        with pytest.raises(NotImplementedError, match="guide_embed dtype"):
            m.open_stream_group(guides(3).float(), 6, 6, 16)
        with pytest.raises(NotImplementedError, match="partition the grid"):
            m.open_stream_group(guides(3), 7, 6, 16)
        with pytest.raises(ValueError, match="multiple of the temporal window"):
            m.open_stream_group(guides(3), 6, 6, 10)
        with pytest.raises(ValueError, match="needs image_newline"):
            module(mm_newline_position="grid").open_stream_group(guides(3), 6, 6, 16)
        with pytest.raises(nv.HicomNativeError, match="GPU only"):                  # everything in scope: the device check is the last one
            m.open_stream_group(guides(3), 6, 6, 16)
    with pytest.raises(RuntimeError, match="builds no autograd graph"):
        module().open_stream_group(guides(3), 6, 6, 16)


def test_push_finish_and_reset_refusals_come_before_any_native_call(host):
    m = module()
    with torch.no_grad():
        g = m.open_stream_group(guides(3), 6, 6, 8)
        with pytest.raises(ValueError, match="nothing has been pushed into slot 1"):
            g.finish(1)
        for args, exc, needle in (((tokens(12), None, [4, 4, 4], [0, 1, 1]), ValueError, "at most once per push"),
                                  ((tokens(12), None, [4, 4, 4], [0, 1, 3]), ValueError, "0 <= slot < B = 3"),
                                  ((tokens(8), None, [4, 4]), ValueError, "slots names the slot"),
                                  ((tokens(16), None, [4, 4, 4, 4]), ValueError, "4 items"),
                                  ((tokens(4), None, []), ValueError, "0 items"),
                                  ((tokens(12), None, [4, 4, 8]), ValueError, "add up to 16 frames, frames_feature has 12"),
                                  ((tokens(11), None, [4, 4, 3]), ValueError, "whole window groups"),
                                  ((tokens(16), None, [12, 4], [0, 1]), ValueError, r"0 \+ 12 frames exceed max_frames=8"),
                                  ((tokens(12, H=3), None, [4, 4, 4]), ValueError, "opened for"),
                                  ((tokens(12)[0], None, [4, 4, 4]), ValueError, "sum Tc, H, W, E"),
                                  ((tokens(12, dtype=torch.float16), None, [4, 4, 4]), NotImplementedError, "float16"),
                                  ((tokens(12), tokens(8), [4, 4, 4]), ValueError, "frames_embed .* vs frames_feature"),
                                  (({"base": None}, None, [4]), NotImplementedError, "anyres")):
            with pytest.raises(exc, match=needle):
                g.push(*args)
        assert not host.launches and g.frames == [0, 0, 0] and csg.STORE_GROUP not in m.__dict__
        g.push(tokens(8), tokens(8), [4, 4], [2, 0])
        with pytest.raises(ValueError, match="with frames_embed so far"):           # mixed frames_embed within slot 2's clip
            g.push(tokens(8), None, [4, 4], [1, 2])
        g.push(tokens(4), None, [4], [1])                                           # ... slot 1 has not begun: its clip may come without
        with pytest.raises(ValueError, match=r"4 \+ 8 frames exceed max_frames=8"):
            g.push(tokens(12), tokens(12), [4, 8], [0, 2])
        assert len(host.launches) == 2 and g.frames == [4, 4, 4] and g.has_fe == [True, False, True]
        g.reset(2)
        g.push(tokens(4), None, [4], [2])                                           # a new clip in slot 2 decides again
        with pytest.raises(ValueError, match="slot 3"):
            g.reset(3)
        with pytest.raises(ValueError, match=r"guide_embed is \[E\]"):
            g.reset(0, guides(2))
    for call in (lambda: g.push(tokens(4), None, [4], [1]), lambda: g.reset(0), lambda: g.finish(0)):
        with pytest.raises(RuntimeError, match="builds no autograd graph"):
            call()
    assert g.frames == [4, 4, 4]


def test_the_plan_key_is_the_tuple_of_chunk_lengths(host):
    m = module(mm_newline_position="grid")
    nl = torch.zeros((64,), dtype=torch.bfloat16)
    with torch.no_grad():
        g = m.open_stream_group(guides(3), 6, 6, 16, nl)
        g.push(tokens(12), tokens(12), [4, 4, 4])
        g.push(tokens(12), tokens(12), [4, 4, 4], [2, 0, 1])                                 # the same tuple at other t0 and slots: a hit
        plans = m.__dict__[csg.STORE_GROUP]
        assert len(plans) == 1 and next(iter(plans.values())).hits == 2 and host.built == [(4, 4, 4)]
        assert next(iter(plans))[1] == (4, 4, 4), "the key holds the tuple of chunk lengths"
        assert host.launches == [((0, 1, 2), (0, 0, 0), (0, 0, 0)), ((2, 0, 1), (4, 4, 4), (6, 6, 6))]   # slot, t0, row0: arguments, not key
        g.push(tokens(12), tokens(12), [4, 8], [1, 0])                                       # another tuple: another plan
        g.push(tokens(12), tokens(12), [8, 4], [2, 1])                                       # ... and its permutation is a third
        assert host.built == [(4, 4, 4), (4, 8), (8, 4)] and host.launches[-1] == ((2, 1), (8, 12), (12, 18))
        assert g.frames == [16, 16, 16] and g.rows(0) == 24
        other = m.open_stream_group(guides(2), 6, 6, 16, nl)                                 # B is in the key (the base's Q)
        other.push(tokens(8), tokens(8), [4, 8][:1] + [4])
        assert len(plans) == 4
    m._invalidate_plans()
    assert csg.STORE_GROUP not in m.__dict__
