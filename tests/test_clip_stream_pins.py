"""CPU pins of the host side of the three clip streams (hicom_amd/clip_stream.py, csrc/clip_stream.hip) and of the list of plan stores
(engine.cached_plan, HIComProjector._invalidate_plans).

Refusals: every C refusal case of tests/test_clip_stream_host.py, test_clip_stream_multi_host.py and test_clip_stream_adapt_host.py, and
the refusals of the fold, clear and placement entry points, with the status code and the COMPLETE hicom_last_error() text.  The argument
blocks are those tables', by import; the pointers are made-up aligned addresses that nothing reads before a launch, and every case breaks
a rule in front of the first launch, so nothing here needs a device.

Blocks: the argument block of a push of each class as the real _build_plan and _launch / _patch fill it on CPU tensors, with `nv` as
clip_stream sees it replaced by a recorder: every scalar field by value, every pointer field by what it addresses (a tensor of the stream,
an offset into the plan's workspace, NULL), and the workspace size.

The expected values are literals recorded from a build of commit 8d2d40b ("Window attention: fp64 tests of forward, adaptor forward,
backward, pool"), the last commit with one host body per stream class, by running these same cases through it.  Two fields of the
single-guide block were unified with the multi-guide rule after that commit; UNIFIED has them, with the reason."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import cases
import hicom_amd
from hicom_amd import clip_stream as cs
from hicom_amd import engine, multi_guide, native as nv, prepared, prepared_many, ragged_multi_guide
from hicom_amd import segments as seg
from host_util import ADDR, module, tokens
from stream_blocks import ADAPTKV, adapt, multi, single



# ---- refusals in front of the first launch -----------------------------------------------------------------------------------------------
def _args(order, kw):
    return [kw.get(k, d) for k, d in order]


FOLD = (("pm", ADDR), ("pl", ADDR), ("pa", ADDR), ("nparts", 3), ("rows", 9), ("rows_pad", 16), ("E", 1152), ("ml_in", ADDR), ("ml_out", ADDR + 4096),
        ("acc", ADDR), ("stream", None))
FOLD_SET = (("ml", ADDR), ("acc", ADDR), ("rows", 27), ("E", 1152), ("ml_in", ADDR + 8192), ("ml_out", ADDR + 4096), ("state", ADDR), ("stream", None))
CLEAR = (("ml", ADDR), ("ml_rows", 18), ("acc", ADDR), ("acc_floats", 1152), ("stream", None))
PLACE = (("loc", ADDR), ("tok", None), ("newline", None), ("Q", 3), ("windows", 4), ("hidden", 64), ("nl_group", 0), ("nl_count", 0), ("nl_first", 0),
         ("nl_step", 1), ("rows", 4), ("global_row0", 4), ("out", ADDR), ("out_dt", nv.DT_F32), ("ldo", 64), ("q_stride", 64 * 48), ("row0", 0), ("stream", None))
ENTRY_CASES = {
    "hicom_stream_state_fold_fwd": (FOLD, {"NULL partials": dict(pm=None), "rows > rows_pad": dict(rows=17), "E % 4": dict(E=1150), "no partials": dict(nparts=0),
                                           "misaligned partial accumulators": dict(pa=ADDR + 4), "misaligned (M, L)": dict(ml_in=ADDR + 4),
                                           "the same (M, L) block": dict(ml_out=ADDR), "(M, L) blocks overlap": dict(ml_out=ADDR + 64)}),
    "hicom_stream_state_fold_set_fwd": (FOLD_SET, {"NULL set": dict(ml=None), "no rows": dict(rows=0), "rows past the grid": dict(rows=65536), "E % 4": dict(E=1150),
                                                   "misaligned set accumulators": dict(acc=ADDR + 4), "misaligned set (M, L)": dict(ml=ADDR + 4),
                                                   "the same (M, L) block": dict(ml_out=ADDR + 8192), "(M, L) blocks overlap": dict(ml_out=ADDR + 8192 + 208)}),
    "hicom_stream_state_clear_fwd": (CLEAR, {"NULL (M, L)": dict(ml=None), "ACC % 4 floats": dict(acc_floats=1150), "misaligned ACC": dict(acc=ADDR + 8)}),
    "hicom_stream_place_rows_fwd": (PLACE, {"NULL out": dict(out=None), "Q = 33": dict(Q=33), "global rows without their source": dict(rows=6), "NULL loc": dict(loc=None),
                                            "rows past the guide's block": dict(row0=45), "global_row0 off the rows": dict(global_row0=3),
                                            "output dtype": dict(out_dt=nv.DT_F16), "newline rows without a pointer": dict(nl_count=1, nl_first=4, rows=5, global_row0=5)}),
}


def refusal_cases():
    """name -> a function that makes the call and returns its status code."""
    L = nv.lib()
    out = {}

    def add(name, fn, *args):
        out[name] = lambda: fn(*args)
    for name, (over, _, _) in single.C_REFUSALS.items():
        add(f"push: {name}", lambda o: L.hicom_compressor_stream_push(ctypes.byref(single.push_block(**o))), over)
    for name, (over, _, _) in multi.C_REFUSALS.items():
        add(f"push_multi: {name}", lambda o: L.hicom_compressor_stream_push_multi(ctypes.byref(multi.push_block(**o))), over)
        add(f"push_multi_adapt: plain: {name}", lambda o: L.hicom_compressor_stream_push_multi_adapt(ctypes.byref(adapt.adapt_block(base=o))), over)
    for name, (over, _, _) in adapt.ADAPT_REFUSALS.items():
        add(f"push_multi_adapt: {name}", lambda o: L.hicom_compressor_stream_push_multi_adapt(ctypes.byref(adapt.adapt_block(**o))), over)
    for entry in ("hicom_compressor_stream_push", "hicom_compressor_stream_push_multi", "hicom_compressor_stream_push_multi_adapt"):
        add(f"{entry[len('hicom_compressor_stream_'):]}: NULL arguments", getattr(L, entry), None)
    for entry, (order, table) in ENTRY_CASES.items():
        for name, kw in table.items():
            add(f"{entry[len('hicom_stream_'):-len('_fwd')]}: {name}", getattr(L, entry), *_args(order, kw))
    return out


REFUSED = {
    'push: E = 768': (-2, 'compressor_stream_push: E=768 (only 1152)'),
    'push: 13 rows': (-2, 'compressor_stream_push: 13 folded rows (<= 12)'),
    'push: hidden = 100': (-2, 'compressor_stream_push: hidden=100 (multiple of 64: fp16 readout planes)'),
    'push: Tc % kt': (-2, 'compressor_stream_push: needs an exact window partition (Tc=6 H=6 W=6, windows 4x3x3)'),
    'push: window of 72 tokens': (-2, 'compressor_stream_push: windows of 72 tokens (16 .. 64)'),
    'push: output dtype': (-2, 'compressor_stream_push: output dtype 2 (bf16 | f32)'),
    'push: NULL ff': (-1, 'compressor_stream_push: NULL pointer'),
    'push: NULL weight': (-1, 'compressor_stream_push: NULL weight'),
    'push: pe without pos_a': (-1, 'compressor_stream_push: pos_a, pe_hi and pe_lo come together'),
    'push: t0 inside a window group': (-1, 'compressor_stream_push: t0=2 (whole window groups of 4 frames)'),
    'push: frames past the tables': (-1, 'compressor_stream_push: frames 16 .. 20, grid 6x6 outside the positional tables (t < 16, y at 16, x at 22, 28 rows)'),
    'push: unaligned ff': (-1, 'compressor_stream_push: 16-byte aligned inputs'),
    'push: ldo < hidden': (-1, 'compressor_stream_push: output layout'),
    'push: newline rows without a pointer': (-1, 'compressor_stream_push: newline rows'),
    'push_multi: Q = 33': (-2, 'compressor_stream_push_multi: Q=33 guides (1 <= Q <= 32 per stream)'),
    'push_multi_adapt: plain: Q = 33': (-2, 'compressor_stream_push_multi_adapt: Q=33 guides (1 <= Q <= 32 per stream)'),
    'push_multi: Q = 0': (-2, 'compressor_stream_push_multi: Q=0 guides (1 <= Q <= 32 per stream)'),
    'push_multi_adapt: plain: Q = 0': (-2, 'compressor_stream_push_multi_adapt: Q=0 guides (1 <= Q <= 32 per stream)'),
    'push_multi: E = 768': (-2, 'compressor_stream_push_multi: E=768 (only 1152)'),
    'push_multi_adapt: plain: E = 768': (-2, 'compressor_stream_push_multi_adapt: E=768 (only 1152)'),
    'push_multi: 17 heads': (-2, 'compressor_stream_push_multi: 17 heads (<= 16 folded rows per guide)'),
    'push_multi_adapt: plain: 17 heads': (-2, 'compressor_stream_push_multi_adapt: 17 heads (<= 16 folded rows per guide)'),
    'push_multi: hidden = 100': (-2, 'compressor_stream_push_multi: hidden=100 (multiple of 64: fp16 readout planes)'),
    'push_multi_adapt: plain: hidden = 100': (-2, 'compressor_stream_push_multi_adapt: hidden=100 (multiple of 64: fp16 readout planes)'),
    'push_multi: Tc % kt': (-2, 'compressor_stream_push_multi: needs an exact window partition (Tc=6 H=6 W=6, windows 4x3x3)'),
    'push_multi_adapt: plain: Tc % kt': (-2, 'compressor_stream_push_multi_adapt: needs an exact window partition (Tc=6 H=6 W=6, windows 4x3x3)'),
    'push_multi: window of 72 tokens': (-2, 'compressor_stream_push_multi: windows of 72 tokens (<= 64)'),
    'push_multi_adapt: plain: window of 72 tokens': (-2, 'compressor_stream_push_multi_adapt: windows of 72 tokens (<= 64)'),
    'push_multi: output dtype': (-2, 'compressor_stream_push_multi: output dtype 2 (bf16 | f32)'),
    'push_multi_adapt: plain: output dtype': (-2, 'compressor_stream_push_multi_adapt: output dtype 2 (bf16 | f32)'),
    'push_multi: more chunks than tiles': (-1, 'compressor_stream_push_multi: 10 token chunks (<= 9 tiles of 16 tokens, <= 256)'),
    'push_multi_adapt: plain: more chunks than tiles': (-1, 'compressor_stream_push_multi_adapt: 10 token chunks (<= 9 tiles of 16 tokens, <= 256)'),
    'push_multi: NULL ff': (-1, 'compressor_stream_push_multi: NULL pointer'),
    'push_multi_adapt: plain: NULL ff': (-1, 'compressor_stream_push_multi_adapt: NULL pointer'),
    'push_multi: NULL guide': (-1, 'compressor_stream_push_multi: NULL pointer'),
    'push_multi_adapt: plain: NULL guide': (-1, 'compressor_stream_push_multi_adapt: NULL pointer'),
    'push_multi: NULL set': (-1, 'compressor_stream_push_multi: NULL pointer'),
    'push_multi_adapt: plain: NULL set': (-1, 'compressor_stream_push_multi_adapt: NULL pointer'),
    'push_multi: NULL state': (-1, 'compressor_stream_push_multi: NULL pointer'),
    'push_multi_adapt: plain: NULL state': (-1, 'compressor_stream_push_multi_adapt: NULL pointer'),
    'push_multi: NULL weight': (-1, 'compressor_stream_push_multi: NULL weight'),
    'push_multi_adapt: plain: NULL weight': (-1, 'compressor_stream_push_multi_adapt: NULL weight'),
    'push_multi: pe without pos_a': (-1, 'compressor_stream_push_multi: pos_a, pe and scratch come together'),
    'push_multi_adapt: plain: pe without pos_a': (-1, 'compressor_stream_push_multi_adapt: pos_a, pe and scratch come together'),
    'push_multi: t0 inside a window group': (-1, 'compressor_stream_push_multi: t0=2 (whole window groups of 4 frames)'),
    'push_multi_adapt: plain: t0 inside a window group': (-1, 'compressor_stream_push_multi_adapt: t0=2 (whole window groups of 4 frames)'),
    'push_multi: frames past the tables': (-1, 'compressor_stream_push_multi: frames 16 .. 20, grid 6x6 outside the positional tables (t < 16, y at 16, x at 22, 28 rows)'),
    'push_multi_adapt: plain: frames past the tables': (-1, 'compressor_stream_push_multi_adapt: frames 16 .. 20, grid 6x6 outside the positional tables (t < 16, y at 16, x at 22, 28 rows)'),
    'push_multi: last frame past the tables': (-1, 'compressor_stream_push_multi: frames 12 .. 20, grid 6x6 outside the positional tables (t < 16, y at 16, x at 22, 28 rows)'),
    'push_multi_adapt: plain: last frame past the tables': (-1, 'compressor_stream_push_multi_adapt: frames 12 .. 20, grid 6x6 outside the positional tables (t < 16, y at 16, x at 22, 28 rows)'),
    'push_multi: x rows past the tables': (-1, 'compressor_stream_push_multi: frames 0 .. 4, grid 6x6 outside the positional tables (t < 16, y at 16, x at 22, 27 rows)'),
    'push_multi_adapt: plain: x rows past the tables': (-1, 'compressor_stream_push_multi_adapt: frames 0 .. 4, grid 6x6 outside the positional tables (t < 16, y at 16, x at 22, 27 rows)'),
    'push_multi: unaligned ff': (-1, 'compressor_stream_push_multi: 16-byte aligned inputs, planes and accumulators, 8-byte aligned (M, L)'),
    'push_multi_adapt: plain: unaligned ff': (-1, 'compressor_stream_push_multi_adapt: 16-byte aligned inputs, planes and accumulators, 8-byte aligned (M, L)'),
    'push_multi: (M, L) blocks overlap: the same block': (-1, 'compressor_stream_push_multi: state_ml_in and state_ml_out overlap'),
    'push_multi_adapt: plain: (M, L) blocks overlap: the same block': (-1, 'compressor_stream_push_multi_adapt: state_ml_in and state_ml_out overlap'),
    'push_multi: (M, L) blocks overlap: 27 rows need 216 bytes': (-1, 'compressor_stream_push_multi: state_ml_in and state_ml_out overlap'),
    'push_multi_adapt: plain: (M, L) blocks overlap: 27 rows need 216 bytes': (-1, 'compressor_stream_push_multi_adapt: state_ml_in and state_ml_out overlap'),
    'push_multi: marginal form without pos-emb': (-2, 'compressor_stream_push_multi: no in-kernel marginals for a chunk of 4x6x6, 32 rows, 2 token chunks (hicom_global_stream_has_marg)'),
    'push_multi_adapt: plain: marginal form without pos-emb': (-2, 'compressor_stream_push_multi_adapt: no in-kernel marginals for a chunk of 4x6x6, 32 rows, 2 token chunks (hicom_global_stream_has_marg)'),
    'push_multi: short score stride': (-1, 'compressor_stream_push_multi: score_stride=128 (>= 144, % 4)'),
    'push_multi_adapt: plain: short score stride': (-1, 'compressor_stream_push_multi_adapt: score_stride=128 (>= 144, % 4)'),
    'push_multi: ldo < hidden': (-1, 'compressor_stream_push_multi: output layout (4 rows per guide at row 0, 4 token rows + 0 newline rows, row length 63, guides 3072 elements apart)'),
    'push_multi_adapt: plain: ldo < hidden': (-1, 'compressor_stream_push_multi_adapt: output layout (4 rows per guide at row 0, 4 token rows + 0 newline rows, row length 63, guides 3072 elements apart)'),
    'push_multi: guides closer than their rows': (-1, 'compressor_stream_push_multi: output layout (4 rows per guide at row 46, 4 token rows + 0 newline rows, row length 64, guides 3072 elements apart)'),
    'push_multi_adapt: plain: guides closer than their rows': (-1, 'compressor_stream_push_multi_adapt: output layout (4 rows per guide at row 46, 4 token rows + 0 newline rows, row length 64, guides 3072 elements apart)'),
    'push_multi: newline rows without a pointer': (-1, 'compressor_stream_push_multi: newline rows (one behind every 2 token rows)'),
    'push_multi_adapt: plain: newline rows without a pointer': (-1, 'compressor_stream_push_multi_adapt: newline rows (one behind every 2 token rows)'),
    'push_multi: newline rows off the packing': (-1, 'compressor_stream_push_multi: newline rows (one behind every 2 token rows)'),
    'push_multi_adapt: plain: newline rows off the packing': (-1, 'compressor_stream_push_multi_adapt: newline rows (one behind every 2 token rows)'),
    'push_multi_adapt: both planes NULL': (-1, 'multi_guide_local_adapt: neither stream has a prepared plane (the plain entry point runs that recipe)'),
    'push_multi_adapt: a plane without its adaptor': (-1, 'compressor_stream_push_multi_adapt: a plane and its adaptor come together (ky with ak.w0, vy with av.w0)'),
    'push_multi_adapt: an adaptor without its plane': (-1, 'compressor_stream_push_multi_adapt: a plane and its adaptor come together (ky with ak.w0, vy with av.w0)'),
    'push_multi_adapt: workspace one byte short': (-1, 'clip_adapt_prepare: workspace of 663552 bytes, 256-byte aligned'),
    'push_multi_adapt: NULL workspace': (-1, 'clip_adapt_prepare: workspace of 663552 bytes, 256-byte aligned'),
    'push_multi_adapt: workspace off its 256 bytes': (-1, 'clip_adapt_prepare: workspace of 663552 bytes, 256-byte aligned'),
    'push_multi_adapt: misaligned key plane': (-1, 'multi_guide_local_adapt: 16-byte aligned planes'),
    'push_multi_adapt: misaligned value plane': (-1, 'multi_guide_local_adapt: 16-byte aligned planes'),
    'push_multi_adapt: alpha dtype': (-1, 'multi_guide_local_adapt: alpha dtype 2 (bf16 | f32)'),
    'push_multi_adapt: NULL LayerNorm weight': (-1, 'multi_guide_local_adapt: adaptor weights'),
    'push_multi_adapt: NULL alpha': (-1, 'multi_guide_local_adapt: adaptor weights'),
    'push_multi_adapt: NULL second layer': (-1, 'clip_adapt_prepare: adaptor weights'),
    'push: NULL arguments': (-1, 'compressor_stream_push: NULL arguments'),
    'push_multi: NULL arguments': (-1, 'compressor_stream_push_multi: NULL arguments'),
    'push_multi_adapt: NULL arguments': (-1, 'compressor_stream_push_multi_adapt: NULL arguments'),
    'state_fold: NULL partials': (-1, 'stream_state_fold: NULL pointer'),
    'state_fold: rows > rows_pad': (-1, 'stream_state_fold: bad shape (nparts=3 rows=17 rows_pad=16 E=1152; E % 4)'),
    'state_fold: E % 4': (-1, 'stream_state_fold: bad shape (nparts=3 rows=9 rows_pad=16 E=1150; E % 4)'),
    'state_fold: no partials': (-1, 'stream_state_fold: bad shape (nparts=0 rows=9 rows_pad=16 E=1152; E % 4)'),
    'state_fold: misaligned partial accumulators': (-1, 'stream_state_fold: 16-byte aligned accumulators, 8-byte aligned (M, L)'),
    'state_fold: misaligned (M, L)': (-1, 'stream_state_fold: 16-byte aligned accumulators, 8-byte aligned (M, L)'),
    'state_fold: the same (M, L) block': (-1, 'stream_state_fold: state_ml_in and state_ml_out overlap'),
    'state_fold: (M, L) blocks overlap': (-1, 'stream_state_fold: state_ml_in and state_ml_out overlap'),
    'state_fold_set: NULL set': (-1, 'stream_state_fold_set: NULL pointer'),
    'state_fold_set: no rows': (-1, 'stream_state_fold_set: bad shape (rows=0 E=1152; E % 4)'),
    'state_fold_set: rows past the grid': (-1, 'stream_state_fold_set: bad shape (rows=65536 E=1152; E % 4)'),
    'state_fold_set: E % 4': (-1, 'stream_state_fold_set: bad shape (rows=27 E=1150; E % 4)'),
    'state_fold_set: misaligned set accumulators': (-1, 'stream_state_fold_set: 16-byte aligned accumulators, 8-byte aligned (M, L)'),
    'state_fold_set: misaligned set (M, L)': (-1, 'stream_state_fold_set: 16-byte aligned accumulators, 8-byte aligned (M, L)'),
    'state_fold_set: the same (M, L) block': (-1, 'stream_state_fold_set: state_ml_in and state_ml_out overlap'),
    'state_fold_set: (M, L) blocks overlap': (-1, 'stream_state_fold_set: state_ml_in and state_ml_out overlap'),
    'state_clear: NULL (M, L)': (-1, 'stream_state_clear: NULL pointer'),
    'state_clear: ACC % 4 floats': (-1, 'stream_state_clear: bad shape or alignment (ACC a multiple of 4 floats, 16-byte aligned)'),
    'state_clear: misaligned ACC': (-1, 'stream_state_clear: bad shape or alignment (ACC a multiple of 4 floats, 16-byte aligned)'),
    'place_rows: NULL out': (-1, 'stream_place_rows: NULL pointer'),
    'place_rows: Q = 33': (-2, 'stream_place_rows: Q=33 guides (1 <= Q <= 32)'),
    'place_rows: global rows without their source': (-1, 'stream_place_rows: NULL pointer'),
    'place_rows: NULL loc': (-1, 'stream_place_rows: NULL pointer'),
    "place_rows: rows past the guide's block": (-1, 'stream_place_rows: output layout (4 rows per guide at row 45, 4 token rows + 0 newline rows, row length 64, guides 3072 elements apart)'),
    'place_rows: global_row0 off the rows': (-1, 'stream_place_rows: output layout (4 rows per guide at row 0, 4 token rows + 0 newline rows, row length 64, guides 3072 elements apart)'),
    'place_rows: output dtype': (-2, 'stream_place_rows: output dtype 2 (bf16 | f32)'),
    'place_rows: newline rows without a pointer': (-1, 'stream_place_rows: newline rows (behind the token rows)'),
}


@pytest.mark.parametrize("name", list(refusal_cases()))
def test_refusals_are_the_parents_code_and_text(name):
    code = int(refusal_cases()[name]())
    msg = nv.lib().hicom_last_error().decode()
    assert code < 0, "a block that passes every check must not be in this table: it would launch"
    assert (code, msg) == REFUSED[name]


# ---- the argument block of a push -----------------------------------------------------------------------------------------------------------
def describe(block, names, ws, prefix=""):
    """{field: value} of a ctypes block, nested structures flattened as "ak.w0"; a pointer field by what it addresses."""
    out = {}
    for f, t in block._fields_:
        v = getattr(block, f)
        if isinstance(v, ctypes.Structure):
            out.update(describe(v, names, ws, f"{prefix}{f}."))
        elif t is ctypes.c_void_p and v is not None and f != "stream":
            off = v - ws.data_ptr()
            out[prefix + f] = names.get(v) or (("ws", off) if 0 <= off < ws.numel() else hex(v))
        else:
            out[prefix + f] = v
    return out


def t(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def recorded(monkeypatch, kind):
    """A stream of class `kind` on the geometry of the host tests (6 x 6 grid, kt = 4, ks = 3, hidden 64, 16 frames, `grid` newline rows)
    whose tensors live on the CPU, the plan of a chunk of 4 frames as the real _build_plan builds it, and `push(...)`: the real _launch on
    that plan -> the description of the block the native push was handed."""
    pushed = []
    fake = SimpleNamespace(**{n: getattr(nv, n) for n in ("StreamPushArgs", "StreamPushMultiArgs", "StreamPushMultiAdaptArgs", "DT_F32", "DT_BF16")},
                           fused_stream_nparts=lambda nw: 3, global_stream_nparts=lambda N, RP: 4, global_stream_has_marg=lambda *a: 1,
                           global_stream_marg_width=lambda H, W: 16,
                           clip_adapt_prepare_workspace=lambda N, E, ak, av, what: (bool(ak.w0) + bool(av.w0)) * N * E * 2,
                           compressor_stream_push=pushed.append, compressor_stream_push_multi=pushed.append,
                           compressor_stream_push_multi_adapt=pushed.append)
    monkeypatch.setattr(cs, "nv", fake)
    monkeypatch.setattr(cs, "_require_bf16_cuda", lambda name, x: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(hicom_amd.projector, "_linear_params", lambda lin: (lin.weight, lin.bias))

    def fill(a, lc, what, ptr):
        a.ak.w0, a.av.w0, a.alpha_dt, a.eps = ADDR, ADDR + 4096, nv.DT_BF16, 1e-6
    monkeypatch.setattr(seg, "fill_adaptors", fill)
    cls = {"single": cs.ClipStream, "multi": cs.ClipStreamMulti, "adapt": cs.ClipStreamAdapt}[kind]
    base = cs.ClipStream if kind == "single" else cs.ClipStreamMulti

    def allocate(self, rows):
        self.out = t(rows, self.hidden) if kind == "single" else t(self.Q, rows, self.hidden)
        R = self.nh if kind == "single" else self.R
        self.state_ml, self.state_acc = t(2, R, 2), t(1, R, self.E)
        self.q_hi, self.q_lo, self.pos_a = t(16, 8), t(16, 8), t(16, 28)
        self.pe_hi, self.pe_lo, self.pe = t(28, 8), t(28, 8), t(28, 8)
        self.P, self.y0, self.x0 = 28, 16, 22

    def prepare(self, guide):
        self.guide = self.guides = guide
        self.cur = 0
    monkeypatch.setattr(base, "_allocate", allocate)
    monkeypatch.setattr(base, "_prepare", prepare)
    m = module("local43_global32" if kind != "adapt" else ADAPTKV, mm_newline_position="grid")
    lc = m.local_compressor
    w0h, w2h = t(4), t(4)
    monkeypatch.setattr(type(lc), "readout_f16", lambda self: (w0h, w2h))
    nl = t(64, dtype=torch.bfloat16)
    guide = t(cases.D, dtype=torch.bfloat16) if kind == "single" else t(3, cases.D, dtype=torch.bfloat16)
    ff, fe = tokens(4), tokens(4)
    with torch.no_grad():
        s = getattr(m, {"single": "open_stream", "multi": "open_stream_multi", "adapt": "open_stream_adapt"}[kind])(guide, 6, 6, 16, nl)
        s.device = "cpu"
        plan = s._build_plan(4, True)
    names = {x.data_ptr(): n for n, x in (("ff", ff), ("fe", fe), ("guide", guide), ("q_hi", s.q_hi), ("q_lo", s.q_lo), ("pos_a", s.pos_a), ("pe_hi", s.pe_hi),
                                          ("pe_lo", s.pe_lo), ("pe", s.pe), ("state_ml[0]", s.state_ml[0]), ("state_ml[1]", s.state_ml[1]),
                                          ("state_acc", s.state_acc), ("out", s.out), ("newline", s.newline), ("readout_f16()[0]", w0h), ("readout_f16()[1]", w2h),
                                          ("readout[0].bias", lc.readout[0].bias), ("readout[2].bias", lc.readout[2].bias))}
    assert len(names) == 18, "the tensors a block may point at have addresses of their own"

    def push(cur, with_fe, t0, row0, nl_group, nl_rows):
        s.cur = cur
        s._launch(plan, ff, fe if with_fe else None, t0, row0, nl_group, nl_rows, 7)
        assert pushed[-1] is plan.args
        return describe(plan.args, names, plan.ws)
    return plan, push


# name -> (class, the pushes on ONE plan: (the (M, L) block read, with frames_embed, t0, row0, nl_group, the chunk's newline rows); the last is pinned)
GRID = (1, True, 4, 6, 2, [8, 11])                        # the second chunk of 4 frames with `grid` newline rows
BLOCK_CASES = {
    "single: grid newline rows": ("single", [GRID]),
    "single: no newline rows behind a push with some": ("single", [GRID, (0, False, 8, 12, 0, [])]),
    "single: one newline row": ("single", [GRID, (0, True, 0, 0, 4, [4])]),
    "multi Q=3: grid newline rows": ("multi", [GRID]),
    "multi Q=3: no newline rows behind a push with some": ("multi", [GRID, (0, False, 8, 12, 0, [])]),
    "adapt Q=3, both adaptors: grid newline rows": ("adapt", [GRID]),
}
WS_BYTES = {'single': 231424, 'multi': 771840, 'adapt': 2098944}
BLOCKS = {
    'single: grid newline rows': {
        'ff': 'ff', 'fe': 'fe', 'Tc': 4, 'H': 6, 'W': 6, 'E': 1152, 'kt': 4, 'ks': 3, 't0': 4, 'rows': 9, 'q_hi': 'q_hi', 'q_lo': 'q_lo', 'pos_a': 'pos_a',
        'pe_hi': 'pe_hi', 'pe_lo': 'pe_lo', 'P': 28, 'y_index0': 16, 'x_index0': 22, 'l_scale': 0.02946278266608715, 'part_m': ('ws', 0), 'part_l': ('ws', 256),
        'part_acc': ('ws', 512), 'ctx_f16': ('ws', 221696), 'hid_f16': ('ws', 230912), 'nparts': 3, 'hidden': 64, 'state_ml_in': 'state_ml[1]', 'state_ml_out':
        'state_ml[0]', 'state_acc': 'state_acc', 'lw0_f16': 'readout_f16()[0]', 'lb0': 'readout[0].bias', 'lw2_f16': 'readout_f16()[1]', 'lb2':
        'readout[2].bias', 'out': 'out', 'out_dt': 0, 'nl_group': 2, 'ldo': 64, 'row0': 6, 'newline': 'newline', 'nl_first': 8, 'nl_step': 3, 'nl_count': 2,
        'reserved_': 0, 'stream': 7},
    'single: no newline rows behind a push with some': {
        'ff': 'ff', 'fe': None, 'Tc': 4, 'H': 6, 'W': 6, 'E': 1152, 'kt': 4, 'ks': 3, 't0': 8, 'rows': 9, 'q_hi': 'q_hi', 'q_lo': 'q_lo', 'pos_a': 'pos_a',
        'pe_hi': 'pe_hi', 'pe_lo': 'pe_lo', 'P': 28, 'y_index0': 16, 'x_index0': 22, 'l_scale': 0.02946278266608715, 'part_m': ('ws', 0), 'part_l': ('ws', 256),
        'part_acc': ('ws', 512), 'ctx_f16': ('ws', 221696), 'hid_f16': ('ws', 230912), 'nparts': 3, 'hidden': 64, 'state_ml_in': 'state_ml[0]', 'state_ml_out':
        'state_ml[1]', 'state_acc': 'state_acc', 'lw0_f16': 'readout_f16()[0]', 'lb0': 'readout[0].bias', 'lw2_f16': 'readout_f16()[1]', 'lb2':
        'readout[2].bias', 'out': 'out', 'out_dt': 0, 'nl_group': 0, 'ldo': 64, 'row0': 12, 'newline': None, 'nl_first': 8, 'nl_step': 3, 'nl_count': 0,
        'reserved_': 0, 'stream': 7},
    'single: one newline row': {
        'ff': 'ff', 'fe': 'fe', 'Tc': 4, 'H': 6, 'W': 6, 'E': 1152, 'kt': 4, 'ks': 3, 't0': 0, 'rows': 9, 'q_hi': 'q_hi', 'q_lo': 'q_lo', 'pos_a': 'pos_a',
        'pe_hi': 'pe_hi', 'pe_lo': 'pe_lo', 'P': 28, 'y_index0': 16, 'x_index0': 22, 'l_scale': 0.02946278266608715, 'part_m': ('ws', 0), 'part_l': ('ws', 256),
        'part_acc': ('ws', 512), 'ctx_f16': ('ws', 221696), 'hid_f16': ('ws', 230912), 'nparts': 3, 'hidden': 64, 'state_ml_in': 'state_ml[0]', 'state_ml_out':
        'state_ml[1]', 'state_acc': 'state_acc', 'lw0_f16': 'readout_f16()[0]', 'lb0': 'readout[0].bias', 'lw2_f16': 'readout_f16()[1]', 'lb2':
        'readout[2].bias', 'out': 'out', 'out_dt': 0, 'nl_group': 4, 'ldo': 64, 'row0': 0, 'newline': 'newline', 'nl_first': 4, 'nl_step': 1, 'nl_count': 1,
        'reserved_': 0, 'stream': 7},
    'multi Q=3: grid newline rows': {
        'ff': 'ff', 'fe': 'fe', 'guide': 'guide', 'Q': 3, 'Tc': 4, 'H': 6, 'W': 6, 'E': 1152, 'kt': 4, 'ks': 3, 'nh': 9, 't0': 4, 'marg': 1, 'q_hi': 'q_hi',
        'q_lo': 'q_lo', 'pos_a': 'pos_a', 'pe': 'pe', 'P': 28, 'y_index0': 16, 'x_index0': 22, 'l_scale': 0.02946278266608715, 'part_m': ('ws', 0), 'part_l':
        ('ws', 512), 'part_acc': ('ws', 1024), 'scores': ('ws', 590848), 'scratch': ('ws', 609280), 'set_ml': ('ws', 616448), 'set_acc': ('ws', 616704),
        'ctx_f16': ('ws', 741120), 'hid_f16': ('ws', 768768), 'loc': ('ws', 770304), 'nparts': 4, 'hidden': 64, 'score_stride': 144, 'state_ml_in':
        'state_ml[1]', 'state_ml_out': 'state_ml[0]', 'state_acc': 'state_acc', 'lw0_f16': 'readout_f16()[0]', 'lb0': 'readout[0].bias', 'lw2_f16':
        'readout_f16()[1]', 'lb2': 'readout[2].bias', 'out': 'out', 'out_dt': 0, 'nl_group': 2, 'ldo': 64, 'q_stride': 3584, 'row0': 6, 'newline': 'newline',
        'nl_first': 8, 'nl_step': 3, 'nl_count': 2, 'reserved_': 0, 'stream': 7},
    'multi Q=3: no newline rows behind a push with some': {
        'ff': 'ff', 'fe': None, 'guide': 'guide', 'Q': 3, 'Tc': 4, 'H': 6, 'W': 6, 'E': 1152, 'kt': 4, 'ks': 3, 'nh': 9, 't0': 8, 'marg': 1, 'q_hi': 'q_hi',
        'q_lo': 'q_lo', 'pos_a': 'pos_a', 'pe': 'pe', 'P': 28, 'y_index0': 16, 'x_index0': 22, 'l_scale': 0.02946278266608715, 'part_m': ('ws', 0), 'part_l':
        ('ws', 512), 'part_acc': ('ws', 1024), 'scores': ('ws', 590848), 'scratch': ('ws', 609280), 'set_ml': ('ws', 616448), 'set_acc': ('ws', 616704),
        'ctx_f16': ('ws', 741120), 'hid_f16': ('ws', 768768), 'loc': ('ws', 770304), 'nparts': 4, 'hidden': 64, 'score_stride': 144, 'state_ml_in':
        'state_ml[0]', 'state_ml_out': 'state_ml[1]', 'state_acc': 'state_acc', 'lw0_f16': 'readout_f16()[0]', 'lb0': 'readout[0].bias', 'lw2_f16':
        'readout_f16()[1]', 'lb2': 'readout[2].bias', 'out': 'out', 'out_dt': 0, 'nl_group': 0, 'ldo': 64, 'q_stride': 3584, 'row0': 12, 'newline': None,
        'nl_first': 0, 'nl_step': 1, 'nl_count': 0, 'reserved_': 0, 'stream': 7},
    'adapt Q=3, both adaptors: grid newline rows': {
        'base.ff': 'ff', 'base.fe': 'fe', 'base.guide': 'guide', 'base.Q': 3, 'base.Tc': 4, 'base.H': 6, 'base.W': 6, 'base.E': 1152, 'base.kt': 4, 'base.ks':
        3, 'base.nh': 9, 'base.t0': 4, 'base.marg': 1, 'base.q_hi': 'q_hi', 'base.q_lo': 'q_lo', 'base.pos_a': 'pos_a', 'base.pe': 'pe', 'base.P': 28,
        'base.y_index0': 16, 'base.x_index0': 22, 'base.l_scale': 0.02946278266608715, 'base.part_m': ('ws', 0), 'base.part_l': ('ws', 512), 'base.part_acc':
        ('ws', 1024), 'base.scores': ('ws', 590848), 'base.scratch': ('ws', 609280), 'base.set_ml': ('ws', 616448), 'base.set_acc': ('ws', 616704),
        'base.ctx_f16': ('ws', 741120), 'base.hid_f16': ('ws', 768768), 'base.loc': ('ws', 770304), 'base.nparts': 4, 'base.hidden': 64, 'base.score_stride':
        144, 'base.state_ml_in': 'state_ml[1]', 'base.state_ml_out': 'state_ml[0]', 'base.state_acc': 'state_acc', 'base.lw0_f16': 'readout_f16()[0]',
        'base.lb0': 'readout[0].bias', 'base.lw2_f16': 'readout_f16()[1]', 'base.lb2': 'readout[2].bias', 'base.out': 'out', 'base.out_dt': 0, 'base.nl_group':
        2, 'base.ldo': 64, 'base.q_stride': 3584, 'base.row0': 6, 'base.newline': 'newline', 'base.nl_first': 8, 'base.nl_step': 3, 'base.nl_count': 2,
        'base.reserved_': 0, 'base.stream': 7, 'ak.w0': '0x7f0000001000', 'ak.b0': None, 'ak.w2_f16': None, 'ak.b2': None, 'ak.gamma': None, 'ak.beta': None,
        'ak.alpha': None, 'av.w0': '0x7f0000002000', 'av.b0': None, 'av.w2_f16': None, 'av.b2': None, 'av.gamma': None, 'av.beta': None, 'av.alpha': None, 'ky':
        ('ws', 771840), 'vy': ('ws', 1103616), 'adapt_ws': ('ws', 1435392), 'adapt_ws_bytes': 663552, 'alpha_dt': 0, 'eps': 9.999999974752427e-07},
}
# The single-guide patch left nl_first / nl_step of the previous push in a shared plan when a chunk has no newline rows, and gave nl_step = 1
# for ONE newline row where the multi-guide patch gives nl_group + 1.  Both classes now set (0, 1) and nl_group + 1: with nl_count == 0
# hicom_compressor_stream_push returns in front of hicom_scatter_rows_fwd and its check stops at nl_count == 0; with nl_count == 1 the
# scatter kernel multiplies the step by the row's index, 0, and the check asks for a positive step only.
UNIFIED = {"single: no newline rows behind a push with some": dict(nl_first=0, nl_step=1), "single: one newline row": dict(nl_step=5)}


@pytest.mark.parametrize("name", list(BLOCK_CASES))
def test_push_blocks_are_the_parents_field_for_field(monkeypatch, name):
    kind, pushes = BLOCK_CASES[name]
    plan, push = recorded(monkeypatch, kind)
    for p in pushes:
        got = push(*p)
    assert plan.ws.numel() == WS_BYTES[kind]
    want = {**BLOCKS[name], **UNIFIED.get(name, {})}
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}


def test_every_case_is_pinned():
    assert sorted(REFUSED) == sorted(refusal_cases()) and sorted(BLOCKS) == sorted(BLOCK_CASES)
    assert all(code in (-1, -2) for code, _ in REFUSED.values())
    assert set(UNIFIED) <= set(BLOCKS) and all(BLOCKS[n][k] != v for n, d in UNIFIED.items() for k, v in d.items())
    for b in BLOCKS.values():                                         # every pointer of a block is named: none is a bare address but the adaptors'
        assert all(not isinstance(v, str) or not v.startswith("0x") or k in ("ak.w0", "av.w0") for k, v in b.items())


# ---- one list of plan stores ----------------------------------------------------------------------------------------------------------------
def test_invalidate_plans_drops_every_store_cached_plan_was_handed(monkeypatch):
    """Whatever store name engine.cached_plan is handed is recorded on the module and dropped by _invalidate_plans (.to(), load_state_dict),
    with the two that do not go through cached_plan: dist.py's `_shard_plans` and the generation of the parameter list."""
    monkeypatch.setattr(engine, "plan_sig", lambda proj: "sig")
    monkeypatch.setattr(engine, "content_sig", lambda proj: "content")

    class Fake:
        def __init__(self):
            self.hits, self.sig, self.fresh, self.refresh = 0, None, None, None
    constants = [v for mod in (cs, multi_guide, ragged_multi_guide, prepared, prepared_many) for k, v in sorted(vars(mod).items())
                 if "STORE" in k and isinstance(v, str)]
    assert {cs.STORE, cs.STORE_MULTI, cs.STORE_ADAPT, "_prepared_many_plans", "_prepare_plans"} <= set(constants) and len(constants) == 8
    stores = ["_a_store_no_list_names", "_engine_plans", "_batch_plans", "_ragged_plans"] + constants
    m = module()
    for store in stores:
        plan = engine.cached_plan(m, store, "k", Fake)
        assert m.__dict__[store] == {"k": plan}                       # the stores stay where they were
    m.__dict__["_shard_plans"] = {"k": Fake()}
    gen = m.__dict__.get("_engine_params_gen", 0)
    m._invalidate_plans()
    assert [s for s in stores + ["_shard_plans"] if s in m.__dict__] == []
    assert m.__dict__["_engine_params_gen"] == gen + 1
    again = engine.cached_plan(m, prepared_many.STORE, "k", Fake)      # ... and a store comes back on its next use, recorded again
    assert m.__dict__[prepared_many.STORE] == {"k": again}
    m.load_state_dict(m.state_dict())
    assert prepared_many.STORE not in m.__dict__
