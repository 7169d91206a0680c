"""CPU checks of the host side of the clip stream (hicom_amd/clip_stream.py, csrc/clip_stream.hip, hicom_amd/native.py): the new symbols and the
unchanged ABI version, the layout of the push argument block as the host C compiler sees it, the chunk row offsets against
HIComProjector._layout of the whole clip, every refusal in front of any native call, and the plan cache.

The push-time checks and the plan cache need a stream object and no device: `host_stream` opens one with the three device methods of
ClipStream (_allocate, _prepare, _launch) and the plan's workspace replaced by recorders, and `nv` as clip_stream sees it replaced by an object
that fails the test when any native function is called."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import cases
from hicom_amd import clip_stream as cs
from hicom_amd import native as nv
from host_util import ADDR, EINVAL, NoNative, module, tokens
from stream_blocks import SINGLE_REFUSALS as C_REFUSALS, single_push_block as push_block


# ---- C refusals: none launches ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(C_REFUSALS))
def test_c_push_refusals_in_front_of_any_device_call(name):
    over, code, needle = C_REFUSALS[name]
    got = nv.lib().hicom_compressor_stream_push(ctypes.byref(push_block(**over)))
    msg = nv.lib().hicom_last_error().decode()
    assert got == code and msg.startswith("compressor_stream_push: ") and needle in msg, (got, msg)
    assert nv.lib().hicom_compressor_stream_push(None) == EINVAL


def test_c_fold_refusals_in_front_of_any_device_call():
    L = nv.lib()
    fold = lambda **kw: L.hicom_stream_state_fold_fwd(*[kw.get(k, d) for k, d in (("pm", ADDR), ("pl", ADDR), ("pa", ADDR), ("nparts", 3), ("rows", 9), ("rows_pad", 16),
                                                                              ("E", 1152), ("ml_in", ADDR), ("ml_out", ADDR + 4096), ("acc", ADDR), ("stream", None))])
    for kw, needle in ((dict(pm=None), "NULL pointer"), (dict(rows=17), "bad shape"), (dict(E=1150), "bad shape"), (dict(nparts=0), "bad shape"),
                       (dict(pa=ADDR + 4), "aligned"), (dict(ml_out=ADDR), "overlap"), (dict(ml_out=ADDR + 64), "overlap")):
        assert fold(**kw) == EINVAL and needle in L.hicom_last_error().decode(), kw
    assert L.hicom_stream_state_clear_fwd(None, 18, ADDR, 1152, None) == EINVAL
    assert L.hicom_stream_state_clear_fwd(ADDR, 18, ADDR, 1150, None) == EINVAL


# ---- row offsets ----------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("pos", ["grid", "frame", "one_token", "no_token"])
@pytest.mark.parametrize("has_nl", [True, False])
@pytest.mark.parametrize("grid", [6, 9])
@pytest.mark.parametrize("chunking", [(4, 4, 4), (4, 8), (8, 4), (12,)])
def test_chunk_rows_concatenated_are_the_layout_of_the_whole_clip(pos, has_nl, grid, chunking):
    m = module(mm_newline_position=pos)
    g = grid // 3
    if pos != "no_token" and not has_nl:
        with pytest.raises(ValueError, match="needs image_newline"):
            cs.chunk_rows(m, 0, 1, g, g, False)
        return
    whole = m._layout((3, g, g), "video", has_nl, False)
    token_rows, newline_rows, t, at = [], [], 0, 0
    for n in chunking:
        row0, nl_group, nl_rows, row1 = cs.chunk_rows(m, t, n // 4, g, g, has_nl)
        assert row0 == at and nl_group == whole.nl_group
        windows = (n // 4) * g * g
        token_rows += [row0 + i + (i // nl_group if nl_group else 0) for i in range(windows)]       # hicom_readout16_gemm_fwd's out_row(m)
        newline_rows += nl_rows
        assert sorted(token_rows[-windows:] + nl_rows) == list(range(row0, row1)), "a chunk's rows tile [row0, row1)"
        t, at = t + n // 4, row1
    tail, lay = cs.prefix_layout(m, 3, g, g, has_nl)
    assert tail == at and lay == whole
    newline_rows += list(range(tail, whole.n_rows))                                                 # finish(): the rows of the whole clip
    assert token_rows == [whole.row_of(i) for i in range(whole.n_tokens)]
    assert newline_rows == whole.newline_rows
    assert len(token_rows) + len(newline_rows) == whole.n_rows


# ---- Python refusals and the plan cache without a device -------------------------------------------------------------------------------


@pytest.fixture
def host(monkeypatch):
    """Patches clip_stream for a device-less stream; returns the list of launches (t0, row0, nl_group, newline rows)."""
    launches = []
    monkeypatch.setattr(cs, "nv", NoNative())
    monkeypatch.setattr(cs, "_require_bf16_cuda", lambda name, t: None)
    monkeypatch.setattr(cs.ClipStream, "_allocate", lambda self, rows: setattr(self, "out", torch.zeros((rows, self.hidden))))
    monkeypatch.setattr(cs.ClipStream, "_prepare", lambda self, guide: (setattr(self, "guide", guide), setattr(self, "cur", 0)))
    monkeypatch.setattr(cs.ClipStream, "_build_plan", lambda self, Tc, has_fe: cs.StreamPlan(None, None, [], lambda: None))
    monkeypatch.setattr(cs.ClipStream, "_launch", lambda self, plan, ff, fe, t0, row0, nl_group, nl_rows, stream: launches.append((t0, row0, nl_group, nl_rows)))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: SimpleNamespace(cuda_stream=0))
    return launches


GUIDE = torch.zeros((cases.D,), dtype=torch.bfloat16)


def test_open_refusals_come_before_any_native_call(monkeypatch):
    monkeypatch.setattr(cs, "nv", NoNative())
    with torch.no_grad():
        for m in (module(use_guide="coarse"), module("local43_adaptkv_global32"), module("local43_adaptqkv_global32", "fine"), module("local43_global32_adaptg"),
                  module(use_clip_scale="local")):
            with pytest.raises(NotImplementedError, match="plain release recipe"):
                m.open_stream(GUIDE, 6, 6, 16)
            assert cs.STORE not in m.__dict__
        for dt in (torch.float16, torch.float32):
            with pytest.raises(NotImplementedError, match=str(dt)):
                module(dtype=dt).open_stream(GUIDE.to(dt), 6, 6, 16)
        m = module()
        with pytest.raises(ValueError, match=r"guide_embed is \[E\]"):
            m.open_stream(torch.zeros((2, cases.D), dtype=torch.bfloat16), 6, 6, 16)
        with pytest.raises(NotImplementedError, match="guide_embed dtype"):
            m.open_stream(GUIDE.float(), 6, 6, 16)
        with pytest.raises(NotImplementedError, match="partition the grid"):
            m.open_stream(GUIDE, 7, 6, 16)
        with pytest.raises(NotImplementedError, match="16 .. 64 tokens"):
            module("local49_global32").open_stream(GUIDE, 9, 9, 16)                 # 4 x 9 x 9 windows: 324 tokens
        with pytest.raises(ValueError, match="multiple of the temporal window"):
            m.open_stream(GUIDE, 6, 6, 10)
        with pytest.raises(ValueError, match="positive ints"):
            m.open_stream(GUIDE, 6, 6, 0)
        with pytest.raises(ValueError, match="needs image_newline"):
            module(mm_newline_position="grid").open_stream(GUIDE, 6, 6, 16)
        with pytest.raises(ValueError, match=r"image_newline is \[hidden\]"):
            module(mm_newline_position="grid").open_stream(GUIDE, 6, 6, 16, torch.zeros((65,), dtype=torch.bfloat16))
        with pytest.raises(nv.HicomNativeError, match="GPU only"):                  # everything in scope: the device check is the last one
            m.open_stream(GUIDE, 6, 6, 16)
    m = module()
    with pytest.raises(RuntimeError, match="builds no autograd graph"):             # autograd on, trainable parameters
        m.open_stream(GUIDE, 6, 6, 16)


def test_push_and_finish_refusals_come_before_any_native_call(host):
    m = module()
    with torch.no_grad():
        s = m.open_stream(GUIDE, 6, 6, 8)
        with pytest.raises(ValueError, match="nothing has been pushed"):
            s.finish()
        for bad, exc, needle in ((tokens(3), ValueError, "whole window groups"), (tokens(0), ValueError, "whole window groups"),
                                 (tokens(4, H=3), ValueError, "opened for"), (tokens(4, E=768), ValueError, "opened for"),
                                 (tokens(4)[0], ValueError, r"\[Tc, H, W, E\]"), (tokens(12), ValueError, "exceed max_frames"),
                                 (tokens(4, dtype=torch.float16), NotImplementedError, "float16"),
                                 ({"base": None, "patch": tokens(4)[0]}, NotImplementedError, "anyres")):
            with pytest.raises(exc, match=needle):
                s.push(bad, None)
        with pytest.raises(ValueError, match="frames_embed .* vs frames_feature"):
            s.push(tokens(4), tokens(8))
        with pytest.raises(NotImplementedError, match="frames_embed dtype"):
            s.push(tokens(4), tokens(4, dtype=torch.float32))
        assert not host and s.frames == 0 and cs.STORE not in m.__dict__
        s.push(tokens(4), tokens(4))
        with pytest.raises(ValueError, match="with frames_embed so far"):           # a mismatch between the chunks of one clip
            s.push(tokens(4), None)
        with pytest.raises(ValueError, match="exceed max_frames"):
            s.push(tokens(8), tokens(8))
        assert len(host) == 1 and s.frames == 4
    with pytest.raises(RuntimeError, match="builds no autograd graph"):
        s.push(tokens(4), tokens(4))
    with pytest.raises(RuntimeError, match="builds no autograd graph"):
        s.reset()
    assert len(host) == 1 and s.frames == 4


def test_equal_chunks_at_different_offsets_share_one_plan(host):
    m = module(mm_newline_position="grid")
    nl = torch.zeros((64,), dtype=torch.bfloat16)
    with torch.no_grad():
        s = m.open_stream(GUIDE, 6, 6, 16, nl)
        for _ in range(3):
            s.push(tokens(4), tokens(4))
        plans = m.__dict__[cs.STORE]
        assert len(plans) == 1 and next(iter(plans.values())).hits == 3
        assert [(t0, row0) for t0, row0, _, _ in host] == [(0, 0), (4, 6), (8, 12)]           # t0 and row0 are call arguments, not key
        assert host[1][2:] == (2, [8, 11])
        other = m.open_stream(GUIDE, 6, 6, 16, nl)                                            # a second stream of the module shares the plan
        other.push(tokens(4), tokens(4))
        assert len(plans) == 1 and next(iter(plans.values())).hits == 4
        s.push(tokens(4), tokens(4))
        assert s.frames == 16 and s.rows == 24
        other.push(tokens(8), tokens(8))                                                      # another chunk length: another plan
        assert len(plans) == 2
        s.reset()
        s.push(tokens(4), None)                                                               # without frames_embed: a key of its own
        assert len(plans) == 3 and host[-1][:2] == (0, 0)
    m._invalidate_plans()
    assert cs.STORE not in m.__dict__
