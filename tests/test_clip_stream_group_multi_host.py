"""CPU checks of the host side of the clip stream group with several guides per slot (hicom_amd/clip_stream_group_multi.py,
csrc/clip_stream_group_multi.hip, hicom_amd/native.py): the new symbols and the unchanged ABI version, the layout of the push block as the
host C compiler sees it and the unchanged sizes of the earlier blocks, every refusal in front of any device work -- of the C entry points
with made-up aligned addresses that nothing reads before a launch, of the Python object with `nv` replaced by an object that fails the test
when a native function is called -- and the plan cache keyed by the tuple of (chunk length, guide count)."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import hicom_amd
from hicom_amd import clip_stream as cs
from hicom_amd import clip_stream_group as csg
from hicom_amd import clip_stream_group_multi as cgm
from hicom_amd import native as nv
from host_util import ADDR, EINVAL, EUNSUP, NoNative, module, tokens
from stream_blocks import GROUP_MULTI_REFUSALS as C_REFUSALS, group_multi_push_block as push_block, guides


def test_the_feature_is_there():
    assert hasattr(hicom_amd.HIComProjector, "open_stream_group_multi")


# ---- C refusals: none launches ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(C_REFUSALS))
def test_c_push_refusals_in_front_of_any_device_call(name):
    over, code, needle = C_REFUSALS[name]
    L = nv.lib()
    got = L.hicom_compressor_stream_group_multi_push(ctypes.byref(push_block(over)))
    msg = L.hicom_last_error().decode()
    assert got == code and msg.startswith("compressor_stream_group_multi: ") and needle in msg, (got, msg)
    assert L.hicom_compressor_stream_group_multi_push(None) == EINVAL and L.hicom_compressor_stream_group_multi_prepare(None) == EINVAL


def test_workspace_bytes_follow_the_tuple_and_refuse_like_the_push():
    L = nv.lib()
    size = lambda over=None: L.hicom_compressor_stream_group_multi_workspace_bytes(ctypes.byref(push_block(over)))
    one = size()
    assert one > size({("tc", 1): 4}) > 0 and one % 256 == 0
    assert size({("q", 1): 4}) > one > size({("q", 0): 3}), "an item's guide count is part of the plan"
    assert one == size({("slot", 0): 1, ("t0", 2): 4, ("pair0", 0): 0, ("row0", 1): 9})                  # not the per-push fields
    assert size({"B": 33}) == EUNSUP and size({("q", 2): 40}) == EUNSUP
    assert L.hicom_compressor_stream_group_multi_workspace_bytes(None) == EINVAL


def test_merge_fold_refusals_in_front_of_any_device_call():
    L = nv.lib()
    ia = lambda *v: (ctypes.c_int32 * len(v))(*v)
    order = (("pm", ADDR), ("pl", ADDR), ("pa", ADDR), ("scores", ADDR), ("items", 3), ("nparts", 3), ("rows", 9), ("Q", 2), ("E", 1152), ("Tc", 4), ("H", 6),
             ("W", 6), ("pe", ADDR), ("P", 28), ("y0", 16), ("x0", 22), ("pair0", ia(4, 0, 2)), ("t0", ia(8, 0, 4)), ("M", 8), ("ml", ADDR), ("acc", ADDR),
             ("stream", None))
    fold = lambda **kw: L.hicom_stream_group_multi_merge_fold_fwd(*[kw.get(k, d) for k, d in order])
    for kw, code, needle in ((dict(pm=None), EINVAL, "NULL pointer"), (dict(rows=17), EINVAL, "bad shape"), (dict(E=1150), EINVAL, "bad shape"),
                             (dict(nparts=0), EINVAL, "bad shape"), (dict(Q=0), EUNSUP, "1 <= Q <= 32"), (dict(Q=33), EUNSUP, "1 <= Q <= 32"),
                             (dict(items=33), EINVAL, "bad shape"), (dict(pa=ADDR + 4), EINVAL, "aligned"), (dict(scores=None), EINVAL, "needs the logits"),
                             (dict(pair0=ia(4, 0, 1)), EINVAL, "share a pair"), (dict(pair0=ia(4, 0, 7)), EINVAL, "outside the group's 8 pairs"),
                             (dict(t0=ia(8, 0, 16)), EINVAL, "outside the positional tables"), (dict(P=27), EINVAL, "outside the positional tables"),
                             (dict(Tc=1024, H=32, W=32, y0=4096, x0=4128, P=4160), EINVAL, "bad shape"),
                             (dict(Tc=1000, H=8, W=8, y0=1024, x0=1032, P=1040), EUNSUP, "marginal sums in LDS")):
        got = fold(**kw)
        msg = L.hicom_last_error().decode()
        assert got == code and msg.startswith("stream_group_multi_merge_fold: ") and needle in msg, (kw, got, msg)


def test_place_global_refusals_in_front_of_any_device_call():
    L = nv.lib()
    ia = lambda *v: (ctypes.c_int32 * len(v))(*v)
    order = (("tok", ADDR), ("newline", ADDR), ("B", 3), ("counts", ia(1, 2, 4)), ("row0", ia(8, 4, 12)), ("named", 0b101), ("tail", 1), ("n_rows", 32),
             ("hidden", 64), ("out", ADDR), ("out_dt", nv.DT_F32), ("ldo", 64), ("pair_stride", 64 * 48), ("pair_rows", 48), ("stream", None))
    place = lambda **kw: L.hicom_stream_group_place_global_fwd(*[kw.get(k, d) for k, d in order])
    for kw, code, needle in ((dict(tok=None), EINVAL, "NULL pointer"), (dict(B=33), EUNSUP, "1 <= B <= 32"), (dict(out_dt=nv.DT_F16), EUNSUP, "output dtype"),
                             (dict(tail=2), EINVAL, "bad shape"), (dict(ldo=63), EINVAL, "bad shape"), (dict(pair_stride=64 * 47), EINVAL, "bad shape"),
                             (dict(newline=None), EINVAL, "no newline token"), (dict(named=0), EINVAL, "non-empty set"), (dict(named=0b1001), EINVAL, "non-empty set"),
                             (dict(counts=ia(1, 0, 4)), EUNSUP, "slot 1: Q=0 guides"), (dict(row0=ia(8, 4, 16)), EINVAL, "slot 2: rows 16 .. 49 outside"),
                             (dict(row0=ia(-1, 4, 12)), EINVAL, "slot 0: rows -1")):
        got = place(**kw)
        msg = L.hicom_last_error().decode()
        assert got == code and msg.startswith("stream_group_place_global: ") and needle in msg, (kw, got, msg)


# ---- Python refusals and the plan cache without a device -------------------------------------------------------------------------------
COUNTS = (1, 2, 4)


@pytest.fixture
def host(monkeypatch):
    """Patches the group for a device-less object; returns the launches (slots, t0s, row0s), the plans built and the finishes (slots, row0s, tail)."""
    launches, built, finishes = [], [], []
    for mod in (cgm, csg, cs):
        monkeypatch.setattr(mod, "nv", NoNative())
    monkeypatch.setattr(cs, "_require_bf16_cuda", lambda name, t: None)
    G = cgm.ClipStreamGroupMulti
    monkeypatch.setattr(G, "_allocate", lambda self, rows: setattr(self, "out", torch.zeros((self.M, rows, self.hidden))))
    monkeypatch.setattr(G, "_prepare", lambda self, guides, slot=None: setattr(self, "guides", guides) if slot is None else None)
    monkeypatch.setattr(G, "_build_plan", lambda self, tcqs, has_fe, stream=None: (built.append(tcqs), cs.StreamPlan(None, None, [], lambda: None))[1])
    monkeypatch.setattr(G, "_launch", lambda self, plan, ff, fe, slots, t0s, row0s, stream: launches.append((tuple(slots), tuple(t0s), tuple(row0s))))
    monkeypatch.setattr(G, "_finish_device", lambda self, slots, row0s, tail: finishes.append((tuple(slots), tuple(row0s), tail)))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: SimpleNamespace(cuda_stream=0))
    return SimpleNamespace(launches=launches, built=built, finishes=finishes)


def test_open_refusals_come_before_any_native_call(monkeypatch):
    for mod in (cgm, csg, cs):
        monkeypatch.setattr(mod, "nv", NoNative())
    with torch.no_grad():
        for m in (module(use_guide="coarse"), module("local43_adaptkv_global32"), module("local43_global32_adaptg"), module(use_clip_scale="local")):
            with pytest.raises(NotImplementedError, match="open_stream_group_multi is built for the plain release recipe only"):
                m.open_stream_group_multi(guides(7), COUNTS, 6, 6, 16)
            assert cgm.STORE_GROUP_MULTI not in m.__dict__
        for dt in (torch.float16, torch.float32):
            with pytest.raises(NotImplementedError, match=str(dt)):
                module(dtype=dt).open_stream_group_multi(guides(7).to(dt), COUNTS, 6, 6, 16)
        m = module()
        for counts, needle in (((), "B=0 slots"), ((1,) * 33, "B=33 slots"), ((1, 0, 4), "slot 1: Q=0 guides"), ((1, 33), "slot 1: Q=33 guides"),
                               ((1, 2.0, 4), "list of the B ints"), (3, "list of the B ints"), ((1, True), "list of the B ints")):
            with pytest.raises(ValueError, match=needle):
                m.open_stream_group_multi(guides(7), counts, 6, 6, 16)
        for M in (6, 8):
            with pytest.raises(ValueError, match=rf"guide_embeds has {M} rows, guide_counts \[1, 2, 4\] add up to 7"):
                m.open_stream_group_multi(guides(M), COUNTS, 6, 6, 16)
        with pytest.raises(ValueError, match=r"guide_embeds is \[Q, E\]"):
            m.open_stream_group_multi(guides(7)[0], COUNTS, 6, 6, 16)
        with pytest.raises(NotImplementedError, match="guide_embed dtype"):
            m.open_stream_group_multi(guides(7).float(), COUNTS, 6, 6, 16)
        with pytest.raises(NotImplementedError, match="partition the grid"):
            m.open_stream_group_multi(guides(7), COUNTS, 7, 6, 16)
        with pytest.raises(ValueError, match="multiple of the temporal window"):
            m.open_stream_group_multi(guides(7), COUNTS, 6, 6, 10)
        with pytest.raises(ValueError, match="needs image_newline"):
            module(mm_newline_position="grid").open_stream_group_multi(guides(7), COUNTS, 6, 6, 16)
        with pytest.raises(nv.HicomNativeError, match="GPU only"):                  # everything in scope: the device check is the last one
            m.open_stream_group_multi(guides(7), COUNTS, 6, 6, 16)
        with pytest.raises(nv.HicomNativeError, match="GPU only"):                  # more than 32 guides in all is in scope: the limit is per slot
            m.open_stream_group_multi(guides(40), (20, 20), 6, 6, 16)
    with pytest.raises(RuntimeError, match="builds no autograd graph"):
        module().open_stream_group_multi(guides(7), COUNTS, 6, 6, 16)


def test_push_finish_and_reset_refusals_come_before_any_native_call(host):
    m = module()
    with torch.no_grad():
        g = m.open_stream_group_multi(guides(7), COUNTS, 6, 6, 8)
        assert g.guide_counts == COUNTS and g.pair0 == [0, 1, 3] and g.out.shape[0] == 7
        with pytest.raises(ValueError, match="nothing has been pushed into slot 1"):
            g.finish(1)
        with pytest.raises(ValueError, match="nothing has been pushed into any slot"):
            g.finish_many()
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
        assert not host.launches and g.frames == [0, 0, 0] and cgm.STORE_GROUP_MULTI not in m.__dict__
        views = g.push(tokens(8), tokens(8), [4, 4], [2, 0])
        assert [tuple(v.shape) for v in views] == [(4, 4, 64), (1, 4, 64)], "one view per item: [Q_slot, chunk rows, hidden]"
        with pytest.raises(ValueError, match="with frames_embed so far"):           # mixed frames_embed within slot 2's clip
            g.push(tokens(8), None, [4, 4], [1, 2])
        with pytest.raises(ValueError, match="nothing has been pushed into slot 1"):         # an empty slot named explicitly
            g.finish_many([0, 1])
        with pytest.raises(ValueError, match="distinct slots"):
            g.finish_many([0, 0])
        with pytest.raises(ValueError, match="distinct slots"):
            g.finish_many([])
        with pytest.raises(ValueError, match="slot 3"):
            g.finish_many([3])
        assert not host.finishes
        outs = g.finish_many()                                                      # the default skips the empty slot 1
        assert sorted(outs) == [0, 2] and tuple(outs[2].shape) == (4, 4 + 32, 64) and tuple(outs[0].shape) == (1, 36, 64)
        assert host.finishes == [((0, 2), (4, 0, 4), 0)]
        assert tuple(g.finish(2).shape) == (4, 36, 64) and host.finishes[-1] == ((2,), (0, 0, 4), 0), "finish(slot) is finish_many([slot])"
        g.push(tokens(4), None, [4], [1])                                           # ... slot 1 has not begun: its clip may come without
        with pytest.raises(ValueError, match=r"4 \+ 8 frames exceed max_frames=8"):
            g.push(tokens(12), tokens(12), [4, 8], [0, 2])
        assert len(host.launches) == 2 and g.frames == [4, 4, 4] and g.has_fe == [True, False, True]
        g.reset(2)
        g.push(tokens(4), None, [4], [2])                                           # a new clip in slot 2 decides again
        with pytest.raises(ValueError, match="slot 3"):
            g.reset(3)
        with pytest.raises(ValueError, match="2 guides for slot 2, which was opened with Q=4"):
            g.reset(2, guides(2))
        with pytest.raises(ValueError, match=r"guide_embeds is \[Q, E\]"):
            g.reset(0, guides(1)[0])
        g.reset(1, guides(2))
        assert g.frames == [4, 0, 4]
    for call in (lambda: g.push(tokens(4), None, [4], [1]), lambda: g.reset(0), lambda: g.finish(0), lambda: g.finish_many()):
        with pytest.raises(RuntimeError, match="builds no autograd graph"):
            call()
    assert g.frames == [4, 0, 4]


def test_two_groups_of_other_guide_counts_share_a_plan_and_each_push_carries_its_own_group(monkeypatch):
    """Plans live on the module.  Groups A (counts (2, 2), M = 4) and B (counts (4, 2), M = 6) both push [4] into slot 1: one (Tc, Q) tuple,
    one plan, built by A.  The block that reaches the C entry must carry the pushing group's B, M and first pair: with A's M = 4 left in it,
    B's pairs 4 .. 6 would be refused.  The real _build_plan and _launch run against a recording `nv`; the block then goes through the
    real C checks with made-up addresses and a workspace too small, the first check behind the pair ranges' own (shape) checks."""
    pushed = []

    class Recorder(NoNative):
        StreamGroupMultiPushArgs = nv.StreamGroupMultiPushArgs
        DT_F32, DT_BF16 = nv.DT_F32, nv.DT_BF16

        def compressor_stream_group_multi_workspace(self, a):
            return 4096

        def compressor_stream_group_multi_prepare(self, a):
            pass

        def compressor_stream_group_multi_push(self, a):
            pushed.append((a.B, a.M, a.items, a.q[0], a.slot[0], a.pair0[0], a.t0[0]))
    monkeypatch.setattr(cgm, "nv", Recorder())
    for mod in (csg, cs):
        monkeypatch.setattr(mod, "nv", NoNative())
    monkeypatch.setattr(cs, "_require_bf16_cuda", lambda name, t: None)
    G = cgm.ClipStreamGroupMulti

    def allocate(self, rows):
        self.out = torch.zeros((self.M, rows, self.hidden))
        self.q_hi = self.q_lo = self.state_ml = self.state_acc = torch.zeros((16,))
        self.pos_a = self.pe = None
        self.P = self.y0 = self.x0 = 0
    monkeypatch.setattr(G, "_allocate", allocate)
    monkeypatch.setattr(G, "_prepare", lambda self, guides, slot=None: setattr(self, "guides", guides) if slot is None else None)
    monkeypatch.setattr(G, "_fill_common", lambda self, a, Tc, nparts, sizes: (torch.zeros((sizes[0],), dtype=torch.uint8), [ADDR], []))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: SimpleNamespace(cuda_stream=0))
    m = module()
    with torch.no_grad():
        ga = m.open_stream_group_multi(guides(4), (2, 2), 6, 6, 16)
        gb = m.open_stream_group_multi(guides(6), (4, 2), 6, 6, 16)
        ga.push(tokens(4), None, [4], [1])
        gb.push(tokens(4), None, [4], [1])
        ga.push(tokens(4), None, [4], [1])
    plans = m.__dict__[cgm.STORE_GROUP_MULTI]
    assert len(plans) == 1 and next(iter(plans.values())).hits == 3, "one (Tc, Q) tuple, one plan for both groups"
    assert pushed == [(2, 4, 1, 2, 1, 2, 0), (2, 6, 1, 2, 1, 4, 0), (2, 4, 1, 2, 1, 2, 4)], "B, M and the first pair are the pushing group's"
    # the shared block as group B left it passes the C entry's pair checks (M = 6: pairs 4 .. 6 are inside); with A's M = 4 it is refused
    a = next(iter(plans.values())).args
    with torch.no_grad():
        gb.reset(1)
        gb.push(tokens(4), None, [4], [1])
    for f in ("ff", "guide", "q_hi", "q_lo", "state_ml", "state_acc", "lw0_f16", "lb0", "lw2_f16", "lb2", "out"):
        setattr(a, f, ADDR)
    a.l_scale, a.ldo, a.ws_bytes = 0.03, 64, 1 << 30
    L = nv.lib()
    a.out_dt, a.pair_rows, a.pair_stride = nv.DT_F32, 48, 64 * 48
    a.ws = ADDR + 16                                         # (refused at the workspace's alignment: nothing is launched)
    assert L.hicom_compressor_stream_group_multi_workspace_bytes(ctypes.byref(a)) > 0
    a.ws_bytes = 0
    assert L.hicom_compressor_stream_group_multi_push(ctypes.byref(a)) == EINVAL and "workspace of" in L.hicom_last_error().decode()
    a.ws, a.ws_bytes, a.out = ADDR, 1 << 30, None            # ... and past the workspace the next refusal is the NULL pointer, not the pairs
    assert L.hicom_compressor_stream_group_multi_push(ctypes.byref(a)) == EINVAL and "NULL pointer" in L.hicom_last_error().decode()
    a.out, a.M, a.ldo = ADDR, 4, 63                          # group A's M under group B's pairs: refused for the pairs, in front of the layout
    assert L.hicom_compressor_stream_group_multi_push(ctypes.byref(a)) == EINVAL
    assert "pairs 4 .. 6 outside the group's 4 pairs" in L.hicom_last_error().decode()
    a.M = 6                                                  # group B's own M: the pairs pass, the layout (ldo < hidden) refuses
    assert L.hicom_compressor_stream_group_multi_push(ctypes.byref(a)) == EINVAL and "output layout" in L.hicom_last_error().decode()


def test_guide_counts_may_be_any_integers_but_not_bools_or_floats(host):
    import numpy as np
    m = module()
    with torch.no_grad():
        g = m.open_stream_group_multi(guides(7), np.array([1, 2, 4]), 6, 6, 8)
        assert g.guide_counts == (1, 2, 4) and all(type(q) is int for q in g.guide_counts)
        g = m.open_stream_group_multi(guides(7), torch.tensor([1, 2, 4]), 6, 6, 8)
        assert g.guide_counts == (1, 2, 4) and g.pair0 == [0, 1, 3]


def test_the_plan_key_is_the_tuple_of_chunk_lengths_and_guide_counts(host):
    m = module(mm_newline_position="grid")
    nl = torch.zeros((64,), dtype=torch.bfloat16)
    with torch.no_grad():
        g = m.open_stream_group_multi(guides(8), (2, 2, 4), 6, 6, 16, nl)
        g.push(tokens(8), tokens(8), [4, 4], [0, 2])
        g.push(tokens(8), tokens(8), [4, 4], [1, 2])                                         # the same (Tc, Q) tuple at another slot and t0: a hit
        plans = m.__dict__[cgm.STORE_GROUP_MULTI]
        assert len(plans) == 1 and next(iter(plans.values())).hits == 2 and host.built == [((4, 2), (4, 4))]
        assert next(iter(plans))[1] == ((4, 2), (4, 4)), "the key holds the tuple of (chunk length, guide count)"
        assert host.launches == [((0, 2), (0, 0), (0, 0)), ((1, 2), (0, 4), (0, 6))]         # slot, t0, row0: arguments, not key
        g.push(tokens(8), tokens(8), [4, 4], [2, 0])                                         # the same chunk lengths routed to slots of other Q
        assert host.built == [((4, 2), (4, 4)), ((4, 4), (4, 2))] and len(plans) == 2
        g.push(tokens(12), tokens(12), [4, 8], [1, 0])                                       # another tuple of lengths: another plan
        assert host.built[-1] == ((4, 2), (8, 2)) and host.launches[-1] == ((1, 0), (4, 8), (6, 12))
        assert g.frames == [16, 8, 12] and g.rows(0) == 24
        other = m.open_stream_group_multi(guides(4), (2, 2), 6, 6, 16, nl)                   # B is in the key (the base's Q)
        other.push(tokens(8), tokens(8), [4, 4])
        assert len(plans) == 4
        assert csg.STORE_GROUP not in m.__dict__, "the single-guide group's store is its own"
    m._invalidate_plans()
    assert cgm.STORE_GROUP_MULTI not in m.__dict__
