"""CPU checks of the host side of the clip stream group (hicom_amd/clip_stream_group.py, csrc/clip_stream_group.hip, hicom_amd/native.py):
the new symbols and the unchanged ABI version, the layout of the push block as the host C compiler sees it, every refusal in front of any
device work -- of the C entry points with made-up aligned addresses that nothing reads before a launch, of the Python object with `nv`
replaced by an object that fails the test when a native function is called -- and the plan cache keyed by the tuple of chunk lengths."""
import ctypes
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import pytest
import torch

import cases
import hicom_amd
from hicom_amd import clip_stream as cs
from hicom_amd import clip_stream_group as csg
from hicom_amd import native as nv
from test_clip_stream_host import ADDR, EINVAL, EUNSUP, NoNative, module, tokens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hicom_compressor_stream_group_workspace_bytes", "hicom_compressor_stream_group_prepare", "hicom_compressor_stream_group_push",
           "hicom_stream_group_merge_fold_fwd")


def test_symbols_are_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "hicom_hip.h")).read()
    declared = set(re.findall(r"\b(hicom_[a-z0-9_]+)\s*\(", header))
    L = nv.lib()
    for name in SYMBOLS:
        assert name in declared and name in nv.EXPORTS and hasattr(L, name)
    assert declared == set(nv.EXPORTS), "header and native.EXPORTS name the same entry points"
    assert L.hicom_compressor_stream_group_workspace_bytes.restype is ctypes.c_int64
    assert "typedef struct hicom_stream_group_push_args" in header
    assert nv.ABI_VERSION == L.hicom_abi_version() == 16
    assert hasattr(hicom_amd.HIComProjector, "open_stream_group")


def test_push_args_layout_matches_the_header_field_for_field(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no host C compiler")
    names = [n for n, _ in nv.StreamGroupPushArgs._fields_]
    src = tmp_path / "abi.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hicom_hip.h"\nint main(void) {\n'
                   '    printf("%d %zu", HICOM_ABI_VERSION, sizeof(hicom_stream_group_push_args));\n'
                   + "".join(f'    printf(" %zu", offsetof(hicom_stream_group_push_args, {n}));\n' for n in names)
                   + '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "abi"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    ver, size, *offs = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert ver == nv.ABI_VERSION == 16
    assert size == ctypes.sizeof(nv.StreamGroupPushArgs)
    assert offs == [getattr(nv.StreamGroupPushArgs, n).offset for n in names]
    assert names[-1] == "stream" and nv.StreamGroupPushArgs.tc.size == 4 * nv.GROUP_MAX == 128


# ---- C refusals: none launches ----------------------------------------------------------------------------------------------------------
def push_block(over=None):
    """Three items (4, 8, 4 frames) of a 6 x 6 grid for the slots (2, 0, 1) of a group of 3; `over`: fields, or (array, index) -> value."""
    a = nv.StreamGroupPushArgs()
    a.B, a.items, a.H, a.W, a.E, a.kt, a.ks, a.nh, a.hidden, a.chunks = 3, 3, 6, 6, 1152, 4, 3, 9, 64, 2
    for f in ("ff", "fe", "guide", "q_hi", "q_lo", "pos_a", "pe", "ws", "state_ml", "state_acc", "lw0_f16", "lb0", "lw2_f16", "lb2", "out"):
        setattr(a, f, ADDR)
    a.P, a.y_index0, a.x_index0, a.l_scale, a.out_dt, a.ldo, a.slot_rows, a.slot_stride = 28, 16, 22, 0.03, nv.DT_F32, 64, 48, 64 * 48
    for i, (tc, slot, t0, row0) in enumerate(((4, 2, 0, 0), (8, 0, 4, 4), (4, 1, 8, 8))):
        a.tc[i], a.slot[i], a.t0[i], a.row0[i] = tc, slot, t0, row0
    a.ws_bytes = 1 << 30
    for k, v in (over or {}).items():
        if isinstance(k, tuple):
            getattr(a, k[0])[k[1]] = v
        else:
            setattr(a, k, v)
    return a


C_REFUSALS = {
    "B = 0": ({"B": 0}, EUNSUP, "1 <= B <= 32"),
    "B = 33": ({"B": 33}, EUNSUP, "1 <= B <= 32"),
    "more items than slots": ({"items": 4}, EINVAL, "a slot appears at most once"),
    "E = 768": ({"E": 768}, EUNSUP, "only 1152"),
    "17 heads": ({"nh": 17}, EUNSUP, "<= 16 folded rows"),
    "hidden = 100": ({"hidden": 100}, EUNSUP, "multiple of 64"),
    "Tc % kt": ({("tc", 1): 6}, EUNSUP, "item 1 needs an exact window partition"),
    "H % ks": ({"H": 7}, EUNSUP, "exact window partition"),
    "window of 72 tokens": ({"kt": 8, ("tc", 0): 8, ("tc", 2): 8}, EUNSUP, "<= 64"),
    "output dtype": ({"out_dt": nv.DT_F16}, EUNSUP, "output dtype"),
    "workspace too small": ({"ws_bytes": 4096}, EINVAL, "workspace of"),
    "NULL ff": ({"ff": None}, EINVAL, "NULL pointer"),
    "NULL state": ({"state_acc": None}, EINVAL, "NULL pointer"),
    "NULL weight": ({"lw2_f16": None}, EINVAL, "NULL weight"),
    "pe without pos_a": ({"pos_a": None}, EINVAL, "come together"),
    "unaligned ff": ({"ff": ADDR + 8}, EINVAL, "16-byte aligned"),
    "duplicate slot": ({("slot", 2): 0}, EINVAL, "slot 0 appears twice"),
    "slot out of range": ({("slot", 0): 3}, EINVAL, "0 <= slot < B = 3"),
    "negative slot": ({("slot", 0): -1}, EINVAL, "0 <= slot < B = 3"),
    "t0 inside a window group": ({("t0", 1): 2}, EINVAL, "whole window groups"),
    "frames past the tables": ({("t0", 1): 12}, EINVAL, "item 1: frames 12 .. 20, grid 6x6 outside the positional tables"),
    "rows past the slot's buffer": ({("row0", 1): 41}, EINVAL, "item 1: rows 41 .. 49 outside the slot's buffer of 48 rows"),
    "negative row": ({("row0", 0): -1}, EINVAL, "outside the slot's buffer"),
    "slots closer than their rows": ({"slot_stride": 64 * 47}, EINVAL, "output layout"),
    "ldo < hidden": ({"ldo": 63}, EINVAL, "output layout"),
    "newline rows without a pointer": ({"nl_group": 2}, EINVAL, "no newline token"),
}


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


def guides(B):
    return torch.zeros((B, cases.D), dtype=torch.bfloat16)


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
