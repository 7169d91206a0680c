"""CPU pins of the host side of the many-item steps (csrc/segment_host.hpp, batch.hip, ragged.hip; hicom_amd/segments.py): the workspace
sizes, every refusal in front of the first launch with its status code and message, and the plan-cache protocol.

With chunks > 0 the workspace functions and every check in front of the first launch are pure host code (the number of compute units is
not asked for), so nothing here needs a device: pointer fields are made-up aligned addresses that nothing reads before a launch, and every
*_fwd case breaks exactly one rule, so none launches.

The expected sizes, codes and messages are literals recorded from a build of commit 8633699 ("forward_batch / forward_ragged: k / v
adaptor recipe, 14 launches"), the last commit with one host implementation per step, by running these same argument blocks through its
library on the host.  Not pinned: "adaptor width %d (multiple of 64)" -- E is held to 1152 in front of it, no argument block reaches it."""
import ctypes
from types import SimpleNamespace

import pytest

from hicom_amd import engine, native as nv, segments

ADDR = 0x7F0000001000                # a made-up address, 4096-byte aligned
IMG, IMG_NL = (1, 1, 0, 0, 0, 1, 32), (1, 1, 3, 3, 3, 4, 32)          # hicom_ragged_item: T, kt, nl_group, nl_count, nl_first, nl_step, n_global_rows
CLIP4, CLIP8 = (4, 4, 0, 0, 0, 1, 32), (8, 4, 0, 0, 0, 1, 32)
POINTERS = ("ff", "fe", "guide", "out", "newline", "lw0_f16", "lb0", "lw2_f16", "lb2", "wq", "bq", "wk", "wv", "bv", "wo", "bo", "gw0", "gb0", "gw2", "gb2",
            "pe", "kpe")
ADAPTOR_POINTERS = ("w0", "b0", "w2_f16", "b2", "gamma", "beta", "alpha")


def block(step, adapt="", items=(IMG, CLIP4, IMG, CLIP8), fwd=False, **over):
    """A valid argument block of `step` ("batch" / "ragged"; adapt: "", "k", "v" or "kv" picks the adaptor recipe and its streams).  fwd: every
    pointer, the packed-row layout and the workspace are filled in as well.  `over`: fields to overwrite, "ak.gamma" reaches into an
    adaptor, "item0.T" into an item, "args.eps" is a field of the adaptor recipe's block."""
    ragged = step == "ragged"
    args = (nv.CompressorRaggedAdaptArgs if ragged else nv.CompressorBatchAdaptArgs)() if adapt else (nv.CompressorRaggedArgs if ragged else nv.CompressorBatchArgs)()
    a = args.base if adapt else args
    a.H, a.W, a.E, a.hidden, a.ks, a.nh, a.P, a.chunks, a.out_dt, a.l_scale = 6, 6, 1152, 896, 3, 9, 0, 1, nv.DT_F32, 0.125
    keep = [args]
    if ragged and items is None:
        a.B = 4                      # ... and a NULL items pointer
    elif ragged:
        arr = (nv.RaggedItem * len(items))(*[nv.RaggedItem(*it) for it in items])
        keep.append(arr)
        a.B, a.items = len(items), arr
    else:
        a.B, a.T, a.kt = 3, 4, 4
    for s in adapt:
        d = getattr(args, "a" + s)
        d.w0 = ADDR
        if fwd:
            for f in ADAPTOR_POINTERS:
                setattr(d, f, ADDR)
    if adapt:
        args.alpha_dt, args.eps = nv.DT_BF16, 1e-5
    if fwd:
        for f in POINTERS:
            setattr(a, f, ADDR)
        a.P, a.t_index0, a.y_index0, a.x_index0 = 28, 0, 16, 22
        a.ldo, a.ws, a.ws_bytes = a.hidden, ADDR, 1 << 40
        if not ragged:
            a.global_row0, a.n_global_rows, a.item_rows = 4, 32, 36          # 4 windows per item, no newline rows
    for k, v in over.items():
        obj, _, field = k.rpartition(".")
        tgt = a if not obj else args if obj == "args" else arr[int(obj[4:])] if obj.startswith("item") else getattr(args, obj)
        setattr(tgt, field, v)
    return args, keep


def call(step, fn, args):
    """(result, hicom_last_error) of hicom_compressor_<step>[_adapt]_<fn>; args None: the plain entry point on a NULL block."""
    adapt = isinstance(args, (nv.CompressorBatchAdaptArgs, nv.CompressorRaggedAdaptArgs))
    f = getattr(nv.lib(), f"hicom_compressor_{step}_{'adapt_' if adapt else ''}{fn}")
    r = f(None if args is None else ctypes.byref(args))
    return int(r), nv.lib().hicom_last_error().decode()


# ---- workspace sizes ------------------------------------------------------------------------------------------------------------------------
WS_CASES = {
    "batch plain B=3 T=4 6x6 f32": ("batch", dict()),
    "batch plain bf16 P=28 chunks=3": ("batch", dict(out_dt=nv.DT_BF16, P=28, chunks=3)),
    "batch plain B=1 image 9x9": ("batch", dict(B=1, T=1, kt=1, H=9, W=9)),
    "batch plain B=5 image 9x9 P=19 chunks=3": ("batch", dict(B=5, T=1, kt=1, H=9, W=9, P=19, chunks=3)),
    "batch plain B=2 T=8 kt=4 chunks=3": ("batch", dict(B=2, T=8, chunks=3)),
    "batch ak": ("batch", dict(adapt="k")),
    "batch ak+av bf16 chunks=3": ("batch", dict(adapt="kv", out_dt=nv.DT_BF16, chunks=3)),
    "batch ak+av B=5 image 9x9": ("batch", dict(adapt="kv", B=5, T=1, kt=1, H=9, W=9)),
    "ragged plain (1, 4, 1, 8) 6x6 f32": ("ragged", dict()),
    "ragged plain bf16 P=28 chunks=3": ("ragged", dict(out_dt=nv.DT_BF16, P=28, chunks=3)),
    "ragged plain B=1 image 9x9": ("ragged", dict(items=(IMG,), H=9, W=9)),
    "ragged plain B=2 9x9 image with newline rows + clip kt=1": ("ragged", dict(items=(IMG_NL, (4, 1, 0, 0, 0, 1, 32)), H=9, W=9, chunks=3)),
    "ragged plain B=5 with newline rows 6x6": ("ragged", dict(items=((1, 1, 2, 2, 2, 3, 32), CLIP4, IMG, CLIP8, IMG), P=28)),
    "ragged ak": ("ragged", dict(adapt="k")),
    "ragged ak+av bf16 chunks=3": ("ragged", dict(adapt="kv", out_dt=nv.DT_BF16, chunks=3)),
    "ragged ak+av B=2 9x9 newline": ("ragged", dict(adapt="kv", items=(IMG_NL, CLIP4), H=9, W=9)),
}
WS_BYTES = {'batch plain B=3 T=4 6x6 f32': 653568,
 'batch plain bf16 P=28 chunks=3': 1078272,
 'batch plain B=1 image 9x9': 253696,
 'batch plain B=5 image 9x9 P=19 chunks=3': 2007552,
 'batch plain B=2 T=8 kt=4 chunks=3': 811264,
 'batch ak': 2644224,
 'batch ak+av bf16 chunks=3': 5056768,
 'batch ak+av B=5 image 9x9': 4998400,
 'ragged plain (1, 4, 1, 8) 6x6 f32': 900352,
 'ragged plain bf16 P=28 chunks=3': 1459200,
 'ragged plain B=1 image 9x9': 254720,
 'ragged plain B=2 9x9 image with newline rows + clip kt=1': 1026048,
 'ragged plain B=5 with newline rows 6x6': 1117440,
 'ragged ak': 3222784,
 'ragged ak+av bf16 chunks=3': 6100224,
 'ragged ak+av B=2 9x9 newline': 4255744}


@pytest.mark.parametrize("name", list(WS_CASES))
def test_workspace_bytes_are_the_parents(name):
    step, kw = WS_CASES[name]
    args, keep = block(step, **kw)
    n, msg = call(step, "workspace_bytes", args)
    assert n == WS_BYTES[name], (n, msg)


# ---- refusals in front of the first launch -----------------------------------------------------------------------------------------------
BIG = (8192, 1, 0, 0, 0, 1, 32)
# name -> (step, entry point, block arguments); in BOTH: once per step, with each prefix
BOTH = {
    "bad shape": ("workspace_bytes", dict(hidden=0)),
    "too many items": ("workspace_bytes", dict(B=4097)),
    "E": ("workspace_bytes", dict(E=1024)),
    "heads": ("workspace_bytes", dict(nh=17)),
    "hidden": ("workspace_bytes", dict(hidden=100)),
    "spatial partition": ("workspace_bytes", dict(H=7)),
    "output dtype": ("workspace_bytes", dict(out_dt=nv.DT_F16)),
    "pe without kpe": ("workspace_bytes", dict(pe=ADDR, P=28)),
    "neither stream adapted": ("workspace_bytes", dict(adapt="kv", **{"ak.w0": None, "av.w0": None})),
    "alpha dtype": ("workspace_bytes", dict(adapt="k", **{"args.alpha_dt": nv.DT_F16})),
    "fwd: NULL input": ("fwd", dict(fwd=True, ff=None)),
    "fwd: NULL output": ("fwd", dict(fwd=True, out=None)),
    "fwd: NULL workspace": ("fwd", dict(fwd=True, ws=None)),
    "fwd: NULL weight": ("fwd", dict(fwd=True, gw2=None)),
    "fwd: adaptor weights": ("fwd", dict(fwd=True, adapt="kv", **{"av.gamma": None})),
    "fwd: workspace too small": ("fwd", dict(fwd=True, ws_bytes=4096)),
    "fwd: workspace misaligned": ("fwd", dict(fwd=True, ws=ADDR + 128)),
    "fwd: misaligned input": ("fwd", dict(fwd=True, fe=ADDR + 8)),
    "fwd: misaligned guide, adaptor recipe": ("fwd", dict(fwd=True, adapt="v", guide=ADDR + 2)),
    "fwd: output layout (ldo)": ("fwd", dict(fwd=True, ldo=895)),
}
REFUSALS = {f"{step}: {name}": (step, fn, kw) for name, (fn, kw) in BOTH.items() for step in ("batch", "ragged")}
REFUSALS.update({
    "batch: NULL arguments": ("batch", "workspace_bytes", None),
    "batch: NULL arguments, fwd": ("batch", "fwd", None),
    "batch: B = 0": ("batch", "workspace_bytes", dict(B=0)),
    "batch: temporal partition": ("batch", "workspace_bytes", dict(T=5)),
    "batch: windows over 64 tokens": ("batch", "workspace_bytes", dict(T=8, kt=8)),
    "batch: too many tokens": ("batch", "workspace_bytes", dict(B=4096, H=96, W=96)),
    "batch: merge LDS": ("batch", "workspace_bytes", dict(B=1, T=64, H=96, W=96)),
    "batch: adaptor GEMM operands": ("batch", "workspace_bytes", dict(adapt="kv", B=4096, H=18, W=18)),
    "batch: fwd: no global rows": ("batch", "fwd", dict(fwd=True, n_global_rows=0, item_rows=4)),
    "batch: fwd: item_rows": ("batch", "fwd", dict(fwd=True, item_rows=37)),
    "batch: fwd: newline group": ("batch", "fwd", dict(fwd=True, nl_group=3, global_row0=5, item_rows=37)),
    "batch: fwd: newline rows without a token": ("batch", "fwd", dict(fwd=True, nl_group=2, nl_count=2, nl_first=2, nl_step=3, global_row0=6, item_rows=38,
                                                                     newline=None)),
    "batch: fwd: newline rows past the local rows": ("batch", "fwd", dict(fwd=True, nl_group=2, nl_count=2, nl_first=2, nl_step=4, global_row0=6, item_rows=38)),
    "batch: fwd: local rows": ("batch", "fwd", dict(fwd=True, global_row0=5, item_rows=37)),
    "ragged: NULL arguments": ("ragged", "workspace_bytes", None),
    "ragged: NULL arguments, prepare": ("ragged", "prepare", None),
    "ragged: NULL arguments, fwd": ("ragged", "fwd", None),
    "ragged: no items": ("ragged", "workspace_bytes", dict(items=None)),
    "ragged: item bad shape": ("ragged", "workspace_bytes", {"item2.n_global_rows": 0}),
    "ragged: item temporal partition": ("ragged", "workspace_bytes", {"item3.T": 6}),
    "ragged: item windows over 64 tokens": ("ragged", "workspace_bytes", {"item1.T": 8, "item1.kt": 8}),
    "ragged: item too many tokens": ("ragged", "workspace_bytes", dict(items=(IMG, (16384, 1, 0, 0, 0, 1, 32)), H=96, W=96)),
    "ragged: item output layout": ("ragged", "workspace_bytes", {"item0.nl_group": 3}),
    "ragged: item newline rows": ("ragged", "workspace_bytes", {"item0.nl_group": 2, "item0.nl_count": 2, "item0.nl_first": 2, "item0.nl_step": 0}),
    "ragged: too many tokens": ("ragged", "workspace_bytes", dict(items=(BIG, BIG), H=96, W=96)),
    "ragged: merge LDS": ("ragged", "workspace_bytes", dict(items=(IMG, (64, 4, 0, 0, 0, 1, 32)), H=96, W=96)),
    "ragged: adaptor GEMM operands": ("ragged", "workspace_bytes", dict(adapt="k", items=(CLIP4,) * 4096, H=18, W=18)),
    "ragged: prepare: workspace too small": ("ragged", "prepare", dict(fwd=True, ws_bytes=4096)),
    "ragged: prepare: bad shape, adaptor recipe": ("ragged", "prepare", dict(fwd=True, adapt="kv", ks=0)),
    "ragged: fwd: newline rows without a token": ("ragged", "fwd", dict(fwd=True, newline=None, **{"item2.nl_group": 2, "item2.nl_count": 2,
                                                                                                  "item2.nl_first": 2, "item2.nl_step": 3})),
})
REFUSED = {'batch: bad shape': (-1, 'compressor_batch: bad shape'),
 'ragged: bad shape': (-1, 'compressor_ragged: bad shape'),
 'batch: too many items': (-2, 'compressor_batch: B=4097 items (<= 4096 per call)'),
 'ragged: too many items': (-2, 'compressor_ragged: B=4097 items (<= 4096 per call)'),
 'batch: E': (-2, 'compressor_batch: E=1024 (only 1152)'),
 'ragged: E': (-2, 'compressor_ragged: E=1024 (only 1152)'),
 'batch: heads': (-2, 'compressor_batch: 17 heads (<= 16 folded rows per item)'),
 'ragged: heads': (-2, 'compressor_ragged: 17 heads (<= 16 folded rows per item)'),
 'batch: hidden': (-2, 'compressor_batch: hidden=100 (multiple of 64: fp16 readout planes)'),
 'ragged: hidden': (-2, 'compressor_ragged: hidden=100 (multiple of 64: fp16 readout planes)'),
 'batch: spatial partition': (-2, 'compressor_batch: needs an exact window partition (T=4 H=7 W=6, windows 4x3x3)'),
 'ragged: spatial partition': (-2, 'compressor_ragged: needs an exact window partition (H=7 W=6, windows 3x3)'),
 'batch: output dtype': (-2, 'compressor_batch: output dtype 2 (bf16 | f32)'),
 'ragged: output dtype': (-2, 'compressor_ragged: output dtype 2 (bf16 | f32)'),
 'batch: pe without kpe': (-1, 'compressor_batch: pe and kpe come together'),
 'ragged: pe without kpe': (-1, 'compressor_ragged: pe and kpe come together'),
 'batch: neither stream adapted': (-1, 'compressor_batch: neither stream has an adaptor (the plain entry point runs that recipe)'),
 'ragged: neither stream adapted': (-1, 'compressor_ragged: neither stream has an adaptor (the plain entry point runs that recipe)'),
 'batch: alpha dtype': (-1, 'compressor_batch: alpha dtype 2 (bf16 | f32)'),
 'ragged: alpha dtype': (-1, 'compressor_ragged: alpha dtype 2 (bf16 | f32)'),
 'batch: fwd: NULL input': (-1, 'compressor_batch: NULL pointer'),
 'ragged: fwd: NULL input': (-1, 'compressor_ragged: NULL pointer'),
 'batch: fwd: NULL output': (-1, 'compressor_batch: NULL pointer'),
 'ragged: fwd: NULL output': (-1, 'compressor_ragged: NULL pointer'),
 'batch: fwd: NULL workspace': (-1, 'compressor_batch: NULL pointer'),
 'ragged: fwd: NULL workspace': (-1, 'compressor_ragged: workspace of 904192 bytes, 256-byte aligned'),
 'batch: fwd: NULL weight': (-1, 'compressor_batch: NULL weight'),
 'ragged: fwd: NULL weight': (-1, 'compressor_ragged: NULL weight'),
 'batch: fwd: adaptor weights': (-1, 'compressor_batch: adaptor weights'),
 'ragged: fwd: adaptor weights': (-1, 'compressor_ragged: adaptor weights'),
 'batch: fwd: workspace too small': (-1, 'compressor_batch: workspace of 656384 bytes, 256-byte aligned'),
 'ragged: fwd: workspace too small': (-1, 'compressor_ragged: workspace of 904192 bytes, 256-byte aligned'),
 'batch: fwd: workspace misaligned': (-1, 'compressor_batch: workspace of 656384 bytes, 256-byte aligned'),
 'ragged: fwd: workspace misaligned': (-1, 'compressor_ragged: workspace of 904192 bytes, 256-byte aligned'),
 'batch: fwd: misaligned input': (-1, 'compressor_batch: 16-byte aligned inputs'),
 'ragged: fwd: misaligned input': (-1, 'compressor_ragged: 16-byte aligned inputs'),
 'batch: fwd: misaligned guide, adaptor recipe': (-1, 'compressor_batch: 16-byte aligned inputs'),
 'ragged: fwd: misaligned guide, adaptor recipe': (-1, 'compressor_ragged: 16-byte aligned inputs'),
 'batch: fwd: output layout (ldo)': (-1, 'compressor_batch: output layout'),
 'ragged: fwd: output layout (ldo)': (-1, 'compressor_ragged: output layout'),
 'batch: NULL arguments': (-1, 'compressor_batch: NULL arguments'),
 'batch: NULL arguments, fwd': (-1, 'compressor_batch: NULL arguments'),
 'batch: B = 0': (-1, 'compressor_batch: bad shape'),
 'batch: temporal partition': (-2, 'compressor_batch: needs an exact window partition (T=5 H=6 W=6, windows 4x3x3)'),
 'batch: windows over 64 tokens': (-2, 'compressor_batch: windows of 72 tokens (<= 64)'),
 'batch: too many tokens': (-2, 'compressor_batch: too many tokens in one call'),
 'batch: merge LDS': (-2, 'compressor_batch: T=64 frames of 96x96: the merge keeps T (H + W) marginal sums in LDS'),
 'batch: adaptor GEMM operands': (-2, 'compressor_batch: 5308416 tokens: the adaptor GEMMs take operands below 2^32 elements'),
 'batch: fwd: no global rows': (-1, 'compressor_batch: output layout'),
 'batch: fwd: item_rows': (-1, 'compressor_batch: output layout'),
 'batch: fwd: newline group': (-1, 'compressor_batch: output layout'),
 'batch: fwd: newline rows without a token': (-1, 'compressor_batch: newline rows'),
 'batch: fwd: newline rows past the local rows': (-1, 'compressor_batch: newline rows'),
 'batch: fwd: local rows': (-1, 'compressor_batch: 5 local rows for 4 tokens + 0 newline rows'),
 'ragged: NULL arguments': (-1, 'compressor_ragged: NULL arguments'),
 'ragged: NULL arguments, prepare': (-1, 'compressor_ragged: NULL arguments'),
 'ragged: NULL arguments, fwd': (-1, 'compressor_ragged: NULL arguments'),
 'ragged: no items': (-1, 'compressor_ragged: bad shape'),
 'ragged: item bad shape': (-1, 'compressor_ragged: item 2: bad shape'),
 'ragged: item temporal partition': (-2, 'compressor_ragged: item 3 needs an exact window partition (T=6, temporal window 4)'),
 'ragged: item windows over 64 tokens': (-2, 'compressor_ragged: item 1: windows of 72 tokens (<= 64)'),
 'ragged: item too many tokens': (-2, 'compressor_ragged: item 1: too many tokens'),
 'ragged: item output layout': (-1, 'compressor_ragged: item 0: output layout'),
 'ragged: item newline rows': (-1, 'compressor_ragged: item 0: newline rows'),
 'ragged: too many tokens': (-2, 'compressor_ragged: too many tokens in one call'),
 'ragged: merge LDS': (-2, 'compressor_ragged: T=64 frames of 96x96: the merge keeps T (H + W) marginal sums in LDS'),
 'ragged: adaptor GEMM operands': (-2, 'compressor_ragged: 5308416 tokens: the adaptor GEMMs take operands below 2^32 elements'),
 'ragged: prepare: workspace too small': (-1, 'compressor_ragged: workspace of 904192 bytes, 256-byte aligned'),
 'ragged: prepare: bad shape, adaptor recipe': (-1, 'compressor_ragged: bad shape'),
 'ragged: fwd: newline rows without a token': (-1, 'compressor_ragged: item 2 has newline rows and there is no newline token')}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_in_front_of_the_first_launch(name):
    step, fn, kw = REFUSALS[name]
    args, keep = (None, None) if kw is None else block(step, **kw)
    code, msg = call(step, fn, args)
    assert code < 0, "a block that passes every check must not be in this table: it would launch"
    assert (code, msg) == REFUSED[name]


def test_every_case_is_pinned():
    assert sorted(WS_BYTES) == sorted(WS_CASES) and sorted(REFUSED) == sorted(REFUSALS)
    assert all(n > 0 for n in WS_BYTES.values()) and all(code in (-1, -2) for code, _ in REFUSED.values())
    for step in ("batch", "ragged"):
        assert all(msg.startswith(f"compressor_{step}: ") for name, (_, msg) in REFUSED.items() if name.startswith(step))


# ---- the plan-cache protocol -------------------------------------------------------------------------------------------------------------
def test_cached_plan_protocol(monkeypatch):
    """segments.cached_plan: a hit on an unchanged signature, refresh without rebuild on a content change, rebuild on a signature change,
    eviction of the oldest plan at the seventeenth key."""
    state = SimpleNamespace(sig=("sig", 0), content=("content", 0))
    monkeypatch.setattr(engine, "plan_sig", lambda proj: state.sig)
    monkeypatch.setattr(engine, "content_sig", lambda proj: state.content)
    proj = SimpleNamespace()
    log = []

    def build(tag="k0"):
        plan = segments.SegPlan(object(), None, 1, 1)
        assert plan.items is None and plan.tables is None           # a batch plan
        plan.refresh = lambda: log.append(("refresh", tag))
        log.append(("build", tag))
        return plan

    def get(key="k0"):
        return segments.cached_plan(proj, "_batch_plans", key, lambda: build(key))
    first = get()
    assert log == [("build", "k0")] and first.hits == 1 and first.sig == ("sig", 0) and first.fresh == ("content", 0)
    assert list(proj._batch_plans) == ["k0"] and not hasattr(proj, "_ragged_plans")
    assert get() is first and first.hits == 2 and log == [("build", "k0")]                    # unchanged: a hit
    state.content = ("content", 1)                                                             # weights changed in place
    assert get() is first and first.hits == 3 and log == [("build", "k0"), ("refresh", "k0")]
    assert first.fresh == ("content", 1)
    assert get() is first and len(log) == 2                                                    # ... refreshed once
    # refresh() reallocates a cached table: the signature read AFTER it no longer matches the plan's, which is rebuilt
    state.content = ("content", 2)
    first.refresh = lambda: (log.append(("refresh", "k0")), setattr(state, "sig", ("sig", 1)))
    second = get()
    assert second is not first and log[2:] == [("refresh", "k0"), ("build", "k0")] and second.hits == 1
    assert second.sig == ("sig", 1) and second.fresh == ("content", 2) and proj._batch_plans == {"k0": second}
    state.sig = ("sig", 2)                                                                     # parameters replaced: rebuild, no refresh
    third = get()
    assert third is not second and log[4:] == [("build", "k0")] and proj._batch_plans == {"k0": third}
    # building moves the signature (the positional tables are (re)built): the plan takes the one read after build()
    del log[:]

    def moving_build():
        state.sig = ("sig", 3)
        return build("k1")
    fourth = segments.cached_plan(proj, "_batch_plans", "k1", moving_build)
    assert fourth.sig == ("sig", 3)
    for i in range(2, segments.MAX_PLANS):
        get(f"k{i}")
    assert segments.MAX_PLANS == 16 and list(proj._batch_plans) == [f"k{i}" for i in range(16)]
    get("k16")                                                                                 # the seventeenth key evicts the oldest
    assert list(proj._batch_plans) == [f"k{i}" for i in range(1, 17)]
    other = segments.cached_plan(proj, "_ragged_plans", "k0", build)                           # the stores are separate
    assert list(proj._ragged_plans) == ["k0"] and other.hits == 1 and len(proj._batch_plans) == 16


def test_cached_plan_eviction_releases_and_a_failed_build_stores_nothing(monkeypatch):
    """engine.cached_plan on the executor's store: the seventeenth key evicts the oldest plan and calls its release() exactly once, a plan
    without release() goes silently, and a build() that raises leaves no plan behind and the other plans alone."""
    monkeypatch.setattr(engine, "plan_sig", lambda proj: "sig")
    monkeypatch.setattr(engine, "content_sig", lambda proj: "content")
    proj = SimpleNamespace()
    released = []

    class Fake:
        def __init__(self, tag):
            self.tag, self.hits, self.sig, self.fresh, self.refresh = tag, 0, None, None, None

    class Releasing(Fake):
        def release(self):
            released.append(self.tag)

    def get(key, cls=Releasing):
        return engine.cached_plan(proj, "_engine_plans", key, lambda: cls(key))
    assert engine.cached_plan is segments.cached_plan and engine.MAX_PLANS == segments.MAX_PLANS == 16
    first = get("k0")
    get("k1", Fake)
    for i in range(2, 16):
        get(f"k{i}")
    assert get("k0") is first and first.hits == 2 and not released and len(proj._engine_plans) == 16

    def failing():
        raise NotImplementedError("refused in front of the workspace")
    before = dict(proj._engine_plans)
    with pytest.raises(NotImplementedError):
        engine.cached_plan(proj, "_engine_plans", "bad", failing)
    assert proj._engine_plans == before and list(proj._engine_plans) == list(before) and not released      # nothing stored, nothing evicted
    get("k16")
    assert released == ["k0"] and list(proj._engine_plans) == [f"k{i}" for i in range(1, 17)]
    get("k17")                                                                                 # k1 has no release(): evicted silently
    assert released == ["k0"] and list(proj._engine_plans) == [f"k{i}" for i in range(2, 18)]
    get("k18")
    assert released == ["k0", "k2"]
    # a stale plan whose rebuild is refused is gone, the others stay
    monkeypatch.setattr(engine, "plan_sig", lambda proj: "sig2")
    with pytest.raises(NotImplementedError):
        engine.cached_plan(proj, "_engine_plans", "k5", failing)
    assert list(proj._engine_plans) == [f"k{i}" for i in range(3, 19) if i != 5] and released == ["k0", "k2"]


def test_patch_guide_reaches_the_nested_injector_blocks():
    """engine.patch_guide on a bare argument block: slots on a top-level field and on `guide` of the nested inj_l / inj_g views, taken once
    as build_args takes them -- ctypes views of a nested structure alias the parent's memory, so the block reads every address back."""
    a = nv.CompressorArgs()
    slots = [(a, "lq"), (a.inj_l, "guide"), (a, "gq"), (a.inj_g, "guide")]

    def read():
        return a.lq, a.inj_l.guide, a.gq, a.inj_g.guide
    assert read() == (None,) * 4
    for addr in (ADDR, ADDR + 0x2000):
        engine.patch_guide(slots, addr)
        assert read() == (addr,) * 4
    assert (a.inj_l.visual, a.inj_g.visual, a.ff, a.fe) == (None,) * 4                       # ... and nothing beside them moved
