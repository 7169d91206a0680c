"""CPU checks of the host side of the logits form of the clip streams (hicom_amd/clip_stream.py, clip_stream_group.py,
clip_stream_group_multi.py, native.py, csrc/clip_stream.hip, csrc/clip_stream_group_multi.hip): the three new symbols on the unchanged ABI
version, their refusals in front of any launch (made-up aligned addresses that nothing reads), every Python refusal of push(local_logits=) in
front of any native call, the three forms of a clip and of a slot, the plan keys, the classes outside the feature, and the guide gather of
ClipStreamGroupMulti.head_scores.

As in tests/test_clip_stream_multi_host.py the stream objects are opened with their device methods replaced by recorders and `nv` as the
stream modules see it replaced by an object that fails the test when a native function is called."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from hicom_amd import clip_stream as cs
from hicom_amd import clip_stream_group as csg
from hicom_amd import clip_stream_group_adapt as cga
from hicom_amd import clip_stream_group_multi as cgm
from hicom_amd import encoder
from hicom_amd import native as nv
from host_util import ADDR, EINVAL, HEADER, NoNative, module, tokens
from stream_blocks import ADAPTKV, group_multi_push_block, guides, multi_push_block, single_push_block

NEW = ("hicom_compressor_stream_push_logits", "hicom_compressor_stream_push_multi_logits", "hicom_compressor_stream_group_multi_push_logits")
COUNTS = (3, 1, 5)


def logits(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


# ---- the C surface ---------------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_on_the_unchanged_abi():
    raw = ctypes.CDLL(nv.LIB_PATH)
    for name in NEW:
        assert name in nv.SIGNATURES and hasattr(raw, name) and f"int {name}(" in HEADER
    assert nv.ABI_VERSION == 16
    assert nv.SIGNATURES[NEW[0]][1] == [ctypes.POINTER(nv.StreamPushArgs), ctypes.c_void_p]
    assert nv.SIGNATURES[NEW[1]][1] == [ctypes.POINTER(nv.StreamPushMultiArgs), ctypes.c_void_p, ctypes.c_int64]
    assert nv.SIGNATURES[NEW[2]][1] == [ctypes.POINTER(nv.StreamGroupMultiPushArgs), ctypes.c_void_p, ctypes.c_int64]


def test_c_entries_refuse_in_front_of_any_launch():
    L = nv.lib()
    single = lambda ll, qs=0, **over: L.hicom_compressor_stream_push_logits(ctypes.byref(single_push_block(**over)), ll)
    multi = lambda ll, qs=144, **over: L.hicom_compressor_stream_push_multi_logits(ctypes.byref(multi_push_block(**over)), ll, qs)
    group = lambda ll, qs=576, **over: L.hicom_compressor_stream_group_multi_push_logits(ctypes.byref(group_multi_push_block(over)), ll, qs)
    for who, call, tokens_ in (("compressor_stream_push_logits", single, None), ("compressor_stream_push_multi_logits", multi, 144),
                               ("compressor_stream_group_multi_push_logits", group, 576)):
        err = lambda: L.hicom_last_error().decode()
        assert call(None) == EINVAL and err().startswith(who + ": ") and "local_logits" in err(), err()
        assert call(ADDR + 2) == EINVAL and err().startswith(who + ": ") and "local_logits" in err(), err()
        if tokens_:
            assert call(ADDR, tokens_ - 1) == EINVAL and err().startswith(who + ": ") and f"q_stride={tokens_ - 1}" in err(), err()
        # the checks of the keyed entry still run, under the new entry's name; fe is not looked at (an unaligned leftover does not refuse)
        assert call(ADDR, tokens_ or 0, E=768) == -2 and err().startswith(who + ": ") and "only 1152" in err(), err()
        assert call(ADDR, tokens_ or 0, fe=ADDR + 2, ff=None) == EINVAL and "NULL pointer" in err(), err()
    assert L.hicom_compressor_stream_push_logits(None, ADDR) == EINVAL and L.hicom_compressor_stream_push_multi_logits(None, ADDR, 144) == EINVAL
    assert L.hicom_compressor_stream_group_multi_push_logits(None, ADDR, 576) == EINVAL
    # the keyed entries keep their names and their rule on fe
    assert L.hicom_compressor_stream_push(ctypes.byref(single_push_block(fe=ADDR + 2))) == EINVAL
    assert L.hicom_last_error().decode().startswith("compressor_stream_push: ")


# ---- the Python surface without a device ----------------------------------------------------------------------------------------------------
@pytest.fixture
def host(monkeypatch):
    """Device-less streams and groups of every class; returns the recorded launches: (class name, has logits, ...)."""
    rec = SimpleNamespace(launches=[], built=[])
    for mod in (cs, csg, cgm, cga):
        monkeypatch.setattr(mod, "nv", NoNative())
    monkeypatch.setattr(cs, "_require_bf16_cuda", lambda name, t: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: SimpleNamespace(cuda_stream=0))

    def plan(self, *a, **k):
        rec.built.append(type(self).__name__)
        return cs.StreamPlan(None, None, [], lambda: None)
    for K in (cs.ClipStream, cs.ClipStreamMulti, cs.ClipStreamAdapt):
        monkeypatch.setattr(K, "_allocate", lambda self, rows: setattr(self, "out", torch.zeros((self.Q, rows, self.hidden) if self.MULTI else (rows, self.hidden))))
        monkeypatch.setattr(K, "_prepare", lambda self, g: (setattr(self, "guides" if self.MULTI else "guide", g), setattr(self, "cur", 0)))
        monkeypatch.setattr(K, "_build_plan", plan)
        monkeypatch.setattr(K, "_launch", lambda self, plan, ff, fe, t0, row0, nl_group, nl_rows, stream, local_logits=None:
                            rec.launches.append((type(self).__name__, local_logits is not None, fe is not None, t0)))
    for K in (csg.ClipStreamGroup, cgm.ClipStreamGroupMulti, cga.ClipStreamGroupAdapt):
        monkeypatch.setattr(K, "_allocate", lambda self, rows: setattr(self, "out", torch.zeros((self.Q, rows, self.hidden))))
        monkeypatch.setattr(K, "_prepare", lambda self, g, slot=None: setattr(self, "guides", g) if slot is None else None)
        monkeypatch.setattr(K, "_build_plan", plan)
        monkeypatch.setattr(K, "_launch", lambda self, plan, ff, fe, slots, t0s, row0s, stream, local_logits=None:
                            rec.launches.append((type(self).__name__, local_logits is not None, fe is not None, tuple(slots))))
    monkeypatch.setattr(cs, "adaptor_widths", lambda what, lc: None)
    return rec


def cuda_ok(monkeypatch):
    monkeypatch.setattr(cs, "_require_f32_cuda", lambda name, t: None)


@pytest.mark.parametrize("multi", [False, True], ids=["ClipStream", "ClipStreamMulti"])
def test_push_refusals_of_the_logits_come_before_any_native_call(host, monkeypatch, multi):
    m = module()
    lead = (3,) if multi else ()
    with torch.no_grad():
        s = m.open_stream_multi(guides(3), 6, 6, 16) if multi else m.open_stream(guides(1)[0], 6, 6, 16)
        with pytest.raises(ValueError, match="float32"):                                       # dtype, with the real check
            s.push(tokens(4), None, local_logits=logits(*lead, 4, 6, 6, dtype=torch.bfloat16))
        with pytest.raises(ValueError, match="device tensor"):                                 # device, with the real check
            s.push(tokens(4), None, local_logits=logits(*lead, 4, 6, 6))
        cuda_ok(monkeypatch)
        with pytest.raises(ValueError, match="frames_embed=None"):
            s.push(tokens(4), tokens(4), local_logits=logits(*lead, 4, 6, 6))
        for bad in (logits(*lead, 8, 6, 6), logits(*lead, 4, 6), logits(*lead, 4, 6, 5), logits(2, 4, 6, 6), "x"):
            with pytest.raises(ValueError, match="local_logits is"):
                s.push(tokens(4), None, local_logits=bad)
        with pytest.raises(ValueError, match="contiguous in its last three"):
            s.push(tokens(4), None, local_logits=logits(*lead, 4, 6, 12)[..., ::2])
        if multi:
            with pytest.raises(ValueError, match="floats apart"):
                s.push(tokens(4), None, local_logits=logits(1, 4, 6, 6).expand(3, 4, 6, 6))
        with pytest.raises(RuntimeError, match="requires grad"):
            s.push(tokens(4), None, local_logits=logits(*lead, 4, 6, 6).requires_grad_())
        with pytest.raises(ValueError, match="whole window groups"):                           # the chunk's own checks still run
            s.push(tokens(3), None, local_logits=logits(*lead, 3, 6, 6))
        assert not host.launches and not host.built and s.frames == 0 and s.has_logits is None
    with pytest.raises(RuntimeError, match="builds no autograd graph"):                        # grad mode, trainable parameters
        s.push(tokens(4), None, local_logits=logits(*lead, 4, 6, 6))
    assert not host.launches


def test_the_three_forms_of_a_clip_do_not_mix_and_reset_clears_the_form(host, monkeypatch):
    cuda_ok(monkeypatch)
    m = module()
    with torch.no_grad():
        s = m.open_stream_multi(guides(3), 6, 6, 16)
        L = logits(3, 4, 6, 6)
        s.push(tokens(4), None, local_logits=L)
        assert (s.has_fe, s.has_logits) == (False, True) and host.launches[-1] == ("ClipStreamMulti", True, False, 0)
        for fe in (tokens(4), None):
            with pytest.raises(ValueError, match="came with local_logits so far"):
                s.push(tokens(4), fe)
        s.push(tokens(4), None, local_logits=L[:, :4])
        assert s.frames == 8
        for fe, form in ((tokens(4), "with frames_embed"), (None, "without frames_embed")):
            s.reset()
            assert (s.frames, s.has_fe, s.has_logits) == (0, None, None)
            s.push(tokens(4), fe)
            assert s.has_logits is False
            with pytest.raises(ValueError, match=f"came {form} so far"):
                s.push(tokens(4), None, local_logits=L)
        assert [l[1] for l in host.launches] == [True, True, False, False]


def test_plan_keys_the_old_forms_keep_theirs_and_the_logits_form_has_its_own(host, monkeypatch):
    cuda_ok(monkeypatch)
    m = module()
    with torch.no_grad():
        for opener, store, lead in ((lambda: m.open_stream(guides(1)[0], 6, 6, 16), cs.STORE, ()), (lambda: m.open_stream_multi(guides(3), 6, 6, 16), cs.STORE_MULTI, (3,))):
            s = opener()
            old = [s._plan_key(4, True, 0), s._plan_key(4, False, 0)]
            assert old == [(s.Q, 4, 6, 6, 1152, has_fe, None, s.out_dtype, 0) for has_fe in (True, False)]
            s.push(tokens(4), tokens(4))
            s.reset()
            s.push(tokens(4), None)
            s.reset()
            s.push(tokens(4), None, local_logits=logits(*lead, 4, 6, 6))
            s.push(tokens(4), None, local_logits=logits(*lead, 4, 6, 6))
            keys = list(m.__dict__[store])
            assert keys == old + [old[1] + ("logits",)], keys
            assert m.__dict__[store][keys[2]].hits == 2
        g = m.open_stream_group_multi(guides(9), COUNTS, 6, 6, 16)
        items = ((8, 5), (4, 3))
        g.push(tokens(12), None, (8, 4), [2, 0])
        g.reset(2), g.reset(0)
        g.push(tokens(12), None, (8, 4), [2, 0], local_logits=logits(5, 12, 6, 6))
        keys = list(m.__dict__[cgm.STORE_GROUP_MULTI])
        assert keys == [g._plan_key(items, False, 0), g._plan_key(items, False, 0) + ("logits",)]


def test_group_refusals_forms_per_slot_and_reset(host, monkeypatch):
    m = module()
    with torch.no_grad():
        g = m.open_stream_group_multi(guides(9), COUNTS, 6, 6, 16)
        push = lambda ll, fe=None, sizes=(8, 4), slots=(2, 0): g.push(tokens(sum(sizes)), fe, sizes, list(slots), local_logits=ll)
        with pytest.raises(ValueError, match="float32"):
            push(logits(5, 12, 6, 6, dtype=torch.float16))
        with pytest.raises(ValueError, match="device tensor"):
            push(logits(5, 12, 6, 6))
        cuda_ok(monkeypatch)
        with pytest.raises(ValueError, match="frames_embed=None"):
            push(logits(5, 12, 6, 6), tokens(12))
        for bad in (logits(9, 12, 6, 6), logits(3, 12, 6, 6), logits(5, 8, 6, 6), logits(12, 6, 6)):       # q_max is that of the TICK's slots: 5
            with pytest.raises(ValueError, match=r"local_logits is \[max Q over the tick's slots"):
                push(bad)
        with pytest.raises(ValueError, match=r"= \[3, 8, 6, 6\]"):                                         # slots 0 and 1: q_max = 3
            push(logits(5, 8, 6, 6), None, (4, 4), (0, 1))
        with pytest.raises(ValueError, match="contiguous in its last three"):
            push(logits(5, 12, 6, 12)[..., ::2])
        with pytest.raises(ValueError, match="floats apart"):
            push(logits(1, 12, 6, 6).expand(5, 12, 6, 6))
        with pytest.raises(RuntimeError, match="requires grad"):
            push(logits(5, 12, 6, 6).requires_grad_())
        assert not host.launches and not host.built and g.frames == [0, 0, 0]
        push(logits(5, 12, 6, 6))
        assert g.has_logits == [True, None, True] and g.has_fe == [False, None, False] and host.launches[-1] == ("ClipStreamGroupMulti", True, False, (2, 0))
        with pytest.raises(ValueError, match="came with local_logits so far"):                             # slot 0 has the logits form, slot 1 is free
            g.push(tokens(8), None, (4, 4), [0, 1])
        g.push(tokens(4), tokens(4), (4,), [1])                                                           # slot 1: with frames_embed
        with pytest.raises(ValueError, match="came with frames_embed so far"):
            g.push(tokens(8), None, (4, 4), [1, 2], local_logits=logits(5, 8, 6, 6))
        g.reset(1)
        assert (g.frames[1], g.has_fe[1], g.has_logits[1]) == (0, None, None)
        g.push(tokens(8), None, (4, 4), [1, 2], local_logits=logits(5, 8, 6, 6))
        assert g.has_logits == [True, True, True] and g.frames == [4, 4, 12]
    with pytest.raises(RuntimeError, match="builds no autograd graph"):
        g.push(tokens(4), None, (4,), [0], local_logits=logits(3, 4, 6, 6))


def test_the_classes_outside_the_feature_raise(host, monkeypatch):
    cuda_ok(monkeypatch)
    with torch.no_grad():
        a = module(ADAPTKV).open_stream_adapt(guides(3), 6, 6, 16)
        with pytest.raises(NotImplementedError, match="not linear"):
            a.push(tokens(4), None, local_logits=logits(3, 4, 6, 6))
        with pytest.raises(NotImplementedError, match="not linear"):
            a.head_scores(tokens(4), None)
        ga = module(ADAPTKV).open_stream_group_adapt(guides(9), COUNTS, 6, 6, 16)
        with pytest.raises(NotImplementedError, match="not linear"):
            ga.push(tokens(4), None, (4,), [0], local_logits=logits(3, 4, 6, 6))
        with pytest.raises(NotImplementedError, match="not linear"):
            ga.head_scores(tokens(4), None, (4,), [0])
        g1 = module().open_stream_group(guides(3), 6, 6, 16)
        with pytest.raises(NotImplementedError, match=r"open_stream_group_multi\(guide_counts=\(1,\) \* B\)"):
            g1.push(tokens(4), None, (4,), [0], local_logits=logits(1, 4, 6, 6))
        assert not hasattr(g1, "head_scores")
        a.push(tokens(4), None)                                                                           # the keyed pushes are what they were
        ga.push(tokens(4), None, (4,), [0])
        g1.push(tokens(4), None, (4,), [0])
    assert [l[:2] for l in host.launches] == [("ClipStreamAdapt", False), ("ClipStreamGroupAdapt", False), ("ClipStreamGroup", False)]


def test_head_scores_helpers_pass_the_streams_guides_and_the_group_gathers_in_item_order(host, monkeypatch):
    calls = []
    monkeypatch.setattr(encoder, "siglip_head_scores", lambda x, head, g, act=None: calls.append(("one", g)) or "L1")
    monkeypatch.setattr(encoder, "siglip_head_scores_multi", lambda x, head, g, act=None: calls.append(("multi", g)) or "LQ")
    monkeypatch.setattr(encoder, "siglip_head_scores_ragged", lambda x, head, g, splits, counts, act=None: calls.append(("ragged", g, splits, counts)) or "LR")
    m = module()
    G = torch.arange(9, dtype=torch.float32)[:, None].expand(9, 1152).to(torch.bfloat16).contiguous()    # guide row p holds p
    with torch.no_grad():
        s1, sq = m.open_stream(G[4], 6, 6, 16), m.open_stream_multi(G[2:5], 6, 6, 16)
        g = m.open_stream_group_multi(G, COUNTS, 6, 6, 16)
        assert s1.head_scores(tokens(4), "head") == "L1" and calls[-1][0] == "one" and torch.equal(calls[-1][1], G[4])
        assert sq.head_scores(tokens(4), "head") == "LQ" and calls[-1][0] == "multi" and torch.equal(calls[-1][1], G[2:5])
        assert g.head_scores(tokens(12), "head", (8, 4), [2, 0]) == "LR"
        kind, got, splits, counts = calls[-1]
        assert kind == "ragged" and tuple(splits) == (8, 4) and list(counts) == [5, 3]
        assert got[:, 0].tolist() == [4, 5, 6, 7, 8, 0, 1, 2], "the guides of slot 2, then those of slot 0: the tick's item order"
        g.head_scores(tokens(12), "head", (4, 4, 4))                                                      # default: range(B)
        assert calls[-1][1][:, 0].tolist() == list(range(9)) and list(calls[-1][3]) == list(COUNTS)
        with pytest.raises(ValueError, match="slots names the slot"):
            g.head_scores(tokens(8), "head", (4, 4))
    assert not host.launches
