"""CPU checks of the host side of the clip stream group on the k / v adaptor recipe (hicom_amd/clip_stream_group_adapt.py,
csrc/clip_stream_group_multi.hip: the flavour Adapt, hicom_amd/native.py): the new symbols and the unchanged ABI version, the layout of the
new block as the host C compiler sees it and the unchanged sizes of the earlier blocks, every refusal in front of any device work -- of the
C entry points with made-up aligned addresses that nothing reads before a launch, of the Python object with `nv` replaced by an object that
fails the test when a native function is called -- the plan key and the store."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import cases
import hicom_amd
from hicom_amd import clip_stream as cs
from hicom_amd import clip_stream_group as csg
from hicom_amd import clip_stream_group_adapt as cga
from hicom_amd import clip_stream_group_multi as cgm
from hicom_amd import native as nv
from host_util import ADDR, EINVAL, EUNSUP, NoNative, module, tokens
from stream_blocks import ADAPTKV, adaptor, group_multi as gmh, guides

PLANE = (4 + 8 + 4) * 36 * 1152 * 2          # one fp16 plane over the 576 stacked tokens of gmh.push_block()


def test_the_feature_is_there():
    assert hasattr(hicom_amd.HIComProjector, "open_stream_group_adapt")
    assert issubclass(cga.ClipStreamGroupAdapt, cgm.ClipStreamGroupMulti) and cga.ClipStreamGroupAdapt.RECIPE == "adaptkv"
    assert cga.ClipStreamGroupAdapt.RECIPE_WORDS == "the k / v adaptor release recipe"


# ---- C refusals: none launches ----------------------------------------------------------------------------------------------------------
def adapt_block(base=None, **over):
    """gmh.push_block (three items of 4 / 8 / 4 frames of 6 x 6 with 4 / 1 / 2 guides) with both adaptors."""
    x = nv.StreamGroupAdaptPushArgs()
    x.base = gmh.push_block(base)
    x.ak, x.av, x.alpha_dt, x.eps = adaptor(), adaptor(), nv.DT_BF16, 1e-6
    for k, v in over.items():
        setattr(x, k, v)
    return x


def big_stack():
    """32 items of 24 frames of 72 x 72: 3981312 stacked tokens x 1152 >= 2^32, every plain limit of the tuple kept."""
    base = {"B": 32, "M": 32, "items": 32, "H": 72, "W": 72, "y_index0": 64, "x_index0": 136, "P": 208}
    for i in range(32):
        base.update({("tc", i): 24, ("q", i): 1, ("slot", i): i, ("pair0", i): i, ("t0", i): 0, ("row0", i): 0})
    return base


def plain_bytes(base=None):
    return nv.lib().hicom_compressor_stream_group_multi_workspace_bytes(ctypes.byref(gmh.push_block(base)))


ADAPT_REFUSALS = {
    "no adaptor at all": (None, dict(ak=adaptor(w0=None), av=adaptor(w0=None)), EINVAL, "neither stream has an adaptor"),
    "NULL second layer": (None, dict(av=adaptor(w2_f16=None)), EINVAL, "adaptor weights"),
    "NULL LayerNorm weight": (None, dict(ak=adaptor(gamma=None)), EINVAL, "adaptor weights"),
    "NULL alpha": (None, dict(av=adaptor(alpha=None)), EINVAL, "adaptor weights"),
    "alpha dtype": (None, dict(alpha_dt=nv.DT_F16), EINVAL, "alpha dtype"),
    "stacked tokens x E >= 2^32": (big_stack(), {}, EUNSUP, "3981312 tokens: the adaptor GEMMs take operands below 2^32 elements"),
    "workspace without the planes": ({"ws_bytes": plain_bytes()}, {}, EINVAL, "workspace of"),
    "workspace one byte short": ({"ws_bytes": plain_bytes() + 4 * PLANE - 1}, {}, EINVAL, f"workspace of {plain_bytes() + 4 * PLANE} bytes"),
    "misaligned workspace": ({"ws": ADDR + 128}, {}, EINVAL, "256-byte aligned"),
    "misaligned frames_embed": ({"fe": ADDR + 8}, {}, EINVAL, "16-byte aligned"),
}


@pytest.mark.parametrize("name", list(ADAPT_REFUSALS))
def test_c_push_refusals_of_the_adaptor_stage_in_front_of_any_device_call(name):
    base, over, code, needle = ADAPT_REFUSALS[name]
    L = nv.lib()
    got = L.hicom_compressor_stream_group_adapt_push(ctypes.byref(adapt_block(base, **over)))
    msg = L.hicom_last_error().decode()
    assert got == code and needle in msg, (got, msg)
    for f in (L.hicom_compressor_stream_group_adapt_push, L.hicom_compressor_stream_group_adapt_prepare, L.hicom_compressor_stream_group_adapt_workspace_bytes):
        assert f(None) == EINVAL


@pytest.mark.parametrize("name", list(gmh.C_REFUSALS))
def test_c_push_makes_every_refusal_of_the_plain_group_push(name):
    over, code, needle = gmh.C_REFUSALS[name]
    L = nv.lib()
    got = L.hicom_compressor_stream_group_adapt_push(ctypes.byref(adapt_block(over)))
    msg = L.hicom_last_error().decode()
    assert got == code and msg.startswith("compressor_stream_group_adapt: ") and needle in msg, (got, msg)


def test_workspace_bytes_are_the_plain_ones_plus_the_planes_and_refuse_like_the_push():
    L = nv.lib()
    size = lambda base=None, **over: L.hicom_compressor_stream_group_adapt_workspace_bytes(ctypes.byref(adapt_block(base, **over)))
    plain = plain_bytes()
    assert plain > 0 and PLANE % 256 == 0
    assert size() == plain + 4 * PLANE, "behind the plain regions: two planes and two hidden planes of layer 1, 4 x 2304 bytes per token"
    assert size(ak=adaptor(w0=None)) == size(av=adaptor(w0=None)) == plain + 2 * PLANE
    short = {("tc", 1): 4}
    assert size(short) == plain_bytes(short) + 4 * PLANE * 12 // 16, "the planes follow the STACK's tokens"
    assert size() == size({("slot", 0): 1, ("t0", 2): 4, ("pair0", 0): 0, ("row0", 1): 9})                  # not the per-push fields
    assert size(big_stack()) == EUNSUP and "below 2^32" in L.hicom_last_error().decode()
    assert plain_bytes(big_stack()) > 0, "... which the plain group takes"
    assert size(alpha_dt=nv.DT_F16) == EINVAL and size({"B": 33}) == EUNSUP and size({("q", 2): 40}) == EUNSUP
    assert size(ak=adaptor(w0=None), av=adaptor(w0=None)) == EINVAL


def test_local_adapt_refusals_in_front_of_any_device_call():
    L = nv.lib()
    ia = lambda *v: (ctypes.c_int32 * len(v))(*v)
    order = (("key", ADDR), ("value", ADDR), ("guide", ADDR), ("ky", ADDR), ("vy", ADDR), ("ak", ctypes.byref(adaptor())), ("av", ctypes.byref(adaptor())),
             ("alpha_dt", nv.DT_BF16), ("eps", ctypes.c_float(1e-6)), ("items", 3), ("Q", 2), ("Tc", 4), ("H", 6), ("W", 6), ("E", 1152), ("kt", 4), ("ks", 3),
             ("scale", ctypes.c_float(0.03)), ("pair0", ia(4, 0, 2)), ("M", 8), ("ctx", ADDR), ("stream", None))
    local = lambda **kw: L.hicom_stream_group_local_adapt_fwd(*[kw.get(k, d) for k, d in order])
    for kw, code, needle in ((dict(pair0=None), EINVAL, "NULL pointer"), (dict(items=0), EINVAL, "bad shape"), (dict(items=33), EINVAL, "bad shape"),
                             (dict(M=0), EINVAL, "bad shape"), (dict(key=None), EINVAL, "NULL pointer"), (dict(ky=None, vy=None), EINVAL, "neither stream"),
                             (dict(Q=33), EUNSUP, "1 <= Q <= 32"), (dict(E=1024), EUNSUP, "only 1152"), (dict(Tc=6), EUNSUP, "exact partition"),
                             (dict(vy=ADDR + 2), EINVAL, "16-byte aligned planes"), (dict(alpha_dt=nv.DT_F16), EINVAL, "alpha dtype"),
                             (dict(ak=ctypes.byref(adaptor(beta=None))), EINVAL, "adaptor weights"),
                             (dict(pair0=ia(4, 0, 1)), EINVAL, "share a pair"), (dict(pair0=ia(4, 0, 7)), EINVAL, "outside the group's 8 pairs")):
        got = local(**kw)
        msg = L.hicom_last_error().decode()
        assert got == code and needle in msg, (kw, got, msg)


# ---- Python refusals, the plan key and the store, without a device -------------------------------------------------------------------------
COUNTS = (1, 2, 5)


@pytest.fixture
def host(monkeypatch):
    """Patches the group for a device-less object; returns the launches (slots, t0s, row0s) and the plans built."""
    launches, built = [], []
    for mod in (cga, cgm, csg, cs):
        monkeypatch.setattr(mod, "nv", NoNative())
    monkeypatch.setattr(cs, "_require_bf16_cuda", lambda name, t: None)
    for G in (cga.ClipStreamGroupAdapt, cgm.ClipStreamGroupMulti):
        monkeypatch.setattr(G, "_allocate", lambda self, rows: setattr(self, "out", torch.zeros((self.M, rows, self.hidden))))
        monkeypatch.setattr(G, "_prepare", lambda self, guides, slot=None: setattr(self, "guides", guides) if slot is None else None)
        monkeypatch.setattr(G, "_build_plan", lambda self, tcqs, has_fe, stream=None: (built.append(tcqs), cs.StreamPlan(None, None, [], lambda: None))[1])
        monkeypatch.setattr(G, "_launch", lambda self, plan, ff, fe, slots, t0s, row0s, stream: launches.append((tuple(slots), tuple(t0s), tuple(row0s))))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: SimpleNamespace(cuda_stream=0))
    return SimpleNamespace(launches=launches, built=built)


def test_open_refusals_come_before_any_native_call(monkeypatch):
    for mod in (cga, cgm, csg, cs):
        monkeypatch.setattr(mod, "nv", NoNative())
    with torch.no_grad():
        for m in (module(ADAPTKV, use_guide="coarse"), module(ADAPTKV, use_clip_scale="local"), module("local43_adaptkv_global32_adaptg"),
                  module("local43_global32_adaptg")):
            with pytest.raises(NotImplementedError, match="open_stream_group_adapt is built for the two release recipes only"):
                m.open_stream_group_adapt(guides(8), COUNTS, 6, 6, 16)
            assert cga.STORE_GROUP_ADAPT not in m.__dict__
        m = module(ADAPTKV)
        for counts, needle in (((), "B=0 slots"), ((1, 0, 5), "slot 1: Q=0 guides"), ((1, 33), "slot 1: Q=33 guides"), (3, "list of the B ints")):
            with pytest.raises(ValueError, match=needle):
                m.open_stream_group_adapt(guides(8), counts, 6, 6, 16)
        with pytest.raises(ValueError, match=r"guide_embeds has 7 rows, guide_counts \[1, 2, 5\] add up to 8"):
            m.open_stream_group_adapt(guides(7), COUNTS, 6, 6, 16)
        with pytest.raises(NotImplementedError, match="partition the grid"):
            m.open_stream_group_adapt(guides(8), COUNTS, 7, 6, 16)
        with pytest.raises(nv.HicomNativeError, match="GPU only"):                  # everything in scope: the device check is the last one
            m.open_stream_group_adapt(guides(8), COUNTS, 6, 6, 16)
        # the earlier entries keep their refusals of the adaptor recipe word for word
        with pytest.raises(NotImplementedError, match="open_stream_group_multi is built for the plain release recipe only \\(local \\+ global compressor, "
                                                      "use_guide='direct', no adaptors, no clip scale\\); everything else goes through forward\\(\\) on the whole clip"):
            m.open_stream_group_multi(guides(8), COUNTS, 6, 6, 16)
        with pytest.raises(NotImplementedError, match="open_stream_group is built for the plain release recipe only \\(local \\+ global compressor, "
                                                      "use_guide='direct', no adaptors, no clip scale\\); everything else goes through forward\\(\\) on the whole clip"):
            m.open_stream_group(guides(3), 6, 6, 16)
    with pytest.raises(RuntimeError, match="builds no autograd graph"):
        module(ADAPTKV).open_stream_group_adapt(guides(8), COUNTS, 6, 6, 16)


def test_a_plain_module_is_routed_to_the_multi_guide_group(host):
    with torch.no_grad():
        g = module().open_stream_group_adapt(guides(8), COUNTS, 6, 6, 8)
        assert type(g) is cgm.ClipStreamGroupMulti and g.WHAT == "open_stream_group_multi" and g.RECIPE == "plain"
        a = module(ADAPTKV).open_stream_group_adapt(guides(8), COUNTS, 6, 6, 8)
        assert type(a) is cga.ClipStreamGroupAdapt and a.guide_counts == COUNTS and a.pair0 == [0, 1, 3] and a.out.shape[0] == 8
        for ptype in ("local43_adaptk_global32", "local43_adaptv_global32"):
            assert type(module(ptype).open_stream_group_adapt(guides(3), (1, 1, 1), 6, 6, 8)) is cga.ClipStreamGroupAdapt


def test_adaptor_widths_and_the_stacked_token_limit_are_checked_on_the_host(host):
    with torch.no_grad():
        m = module(ADAPTKV)
        lin = m.local_compressor.k_proj[0]
        lin.weight = torch.nn.Parameter(torch.zeros((cases.D, cases.D - 32), dtype=torch.bfloat16))
        with pytest.raises(NotImplementedError, match="open_stream_group_adapt: adaptor widths must be multiples of 64"):
            m.open_stream_group_adapt(guides(8), COUNTS, 6, 6, 16)
        # 8 frames of 510 x 510 tokens of 1152 channels are 2^31.2 elements: one chunk fits, a stack of two does not.  (With the positional
        # term the merge's LDS limit on a chunk binds first at this grid; without it it does not apply.)
        big = module(ADAPTKV)
        big.global_compressor.use_pos_emb = False
        with pytest.raises(NotImplementedError, match="open_stream_group_adapt: .*below 2\\^32 elements"):
            big.open_stream_group_adapt(guides(2), (1, 1), 1026, 1026, 8)
        g = big.open_stream_group_adapt(guides(2), (1, 1), 510, 510, 16)
        frames = lambda n: torch.zeros((1, 1, 1, 1), dtype=torch.bfloat16).expand(n, 510, 510, cases.D)
        with pytest.raises(NotImplementedError, match="ClipStreamGroupAdapt.push: Tc=16 .*push shorter chunks"):
            g.push(frames(16), None, [16], [0])
        with pytest.raises(NotImplementedError, match="ClipStreamGroupAdapt.push: 16 stacked frames of 510x510: .*over the whole stack"):
            g.push(frames(16), None, [8, 8])
        g.push(frames(8), None, [8], [1])
    assert host.launches == [((1,), (0,), (0,))] and g.frames == [0, 8]


def test_push_and_reset_refusals_are_the_parents_under_the_adaptor_recipe(host):
    m = module(ADAPTKV)
    with torch.no_grad():
        g = m.open_stream_group_adapt(guides(8), COUNTS, 6, 6, 8)
        with pytest.raises(ValueError, match="nothing has been pushed into slot 1"):
            g.finish(1)
        for args, exc, needle in (((tokens(12), None, [4, 4, 4], [0, 1, 1]), ValueError, "at most once per push"),
                                  ((tokens(12), None, [4, 4, 8]), ValueError, "add up to 16 frames, frames_feature has 12"),
                                  ((tokens(16), None, [12, 4], [0, 1]), ValueError, r"0 \+ 12 frames exceed max_frames=8 of open_stream_group_adapt"),
                                  ((tokens(12, dtype=torch.float16), None, [4, 4, 4]), NotImplementedError, "float16")):
            with pytest.raises(exc, match=needle):
                g.push(*args)
        assert not host.launches
        views = g.push(tokens(8), tokens(8), [4, 4], [2, 0])
        assert [tuple(v.shape) for v in views] == [(5, 4, 64), (1, 4, 64)]
        with pytest.raises(ValueError, match="ClipStreamGroupAdapt.reset: 2 guides for slot 2, which was opened with Q=5"):
            g.reset(2, guides(2))
        with pytest.raises(ValueError, match=r"ClipStreamGroupAdapt.reset: guide_embeds is \[Q, E\]"):
            g.reset(0, guides(1)[0])
        g.reset(2, guides(5))                                                       # new guides pass the scope check under the adaptor recipe
        assert g.frames == [4, 0, 0]
        m.local_compressor.adapt_k = m.local_compressor.adapt_v = False            # the module leaves the recipe behind the group's back
        with pytest.raises(NotImplementedError, match="left the scope of open_stream_group_adapt \\(the k / v adaptor release recipe, bfloat16\\)"):
            g.push(tokens(4), None, [4], [1])
        with pytest.raises(NotImplementedError, match="ClipStreamGroupAdapt.reset is built for the two release recipes only"):
            g.reset(1, guides(2))


def test_the_plan_key_carries_the_adaptor_set_and_the_store_is_the_classes_own(host):
    m = module(ADAPTKV)
    with torch.no_grad():
        g = m.open_stream_group_adapt(guides(8), COUNTS, 6, 6, 16)
        g.push(tokens(8), tokens(8), [4, 4], [0, 2])
        g.push(tokens(8), tokens(8), [4, 4], [0, 2])                                # the same (Tc, Q) tuple at another t0: a hit
        plans = m.__dict__[cga.STORE_GROUP_ADAPT]
        assert cga.STORE_GROUP_ADAPT == "_clip_stream_group_adapt_plans" and len(plans) == 1 and next(iter(plans.values())).hits == 2
        key = next(iter(plans))
        assert key[1] == ((4, 1), (4, 5)) and key[-2:] == (True, True), "the parent's key plus (adapt_k, adapt_v)"
        assert key[:-2] == cgm.ClipStreamGroupMulti._plan_key(g, ((4, 1), (4, 5)), True, 0)
        assert host.built == [((4, 1), (4, 5))] and host.launches == [((0, 2), (0, 0), (0, 0)), ((0, 2), (4, 4), (4, 4))]
        assert cgm.STORE_GROUP_MULTI not in m.__dict__ and cs.STORE_ADAPT not in m.__dict__
        k_only = module("local43_adaptk_global32")
        gk = k_only.open_stream_group_adapt(guides(8), COUNTS, 6, 6, 16)
        assert gk._plan_key(((4, 1),), True, 0)[-2:] == (True, False)
    m._invalidate_plans()
    assert cga.STORE_GROUP_ADAPT not in m.__dict__
