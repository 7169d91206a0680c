"""CPU checks of the host side of the multi-guide step (csrc/multi_guide.hip on csrc/segment_host.hpp, hicom_amd/native.py): the symbols,
the layout of the argument block as the host C compiler sees it, the workspace arithmetic DESIGN.md §3.8 states, and the refusals of the C
entry points in front of any device call -- by substring, and pinned exactly (workspace sizes, status codes, whole messages) as literals
recorded from a build of commit b2cec2a ("Add forward_multi_guide: one clip, Q instructions, tokens read once"), the last commit whose
multi-guide step had a host implementation of its own.

As in tests/test_seg_host_pins.py: with chunks > 0 the workspace function and every check in front of the first launch are pure host
code, pointer fields are made-up aligned addresses that nothing reads before a launch, and every *_fwd case breaks one rule, so none
launches."""
import ctypes

import pytest

from hicom_amd import native as nv
from host_util import ADDR, EINVAL, EUNSUP

POINTERS = ("ff", "fe", "guide", "out", "newline", "lw0_f16", "lb0", "lw2_f16", "lb2", "wq", "bq", "wk", "wv", "bv", "wo", "bo", "gw0", "gb0", "gw2", "gb2",
            "pe", "kpe")


def block(fwd=False, **over):
    """A valid argument block: Q = 3 guides on a 4 x 6 x 6 clip, windows 4 x 3 x 3 (4 of them), hidden 896, fp32 rows, 3 token chunks."""
    a = nv.CompressorMultiGuideArgs()
    a.Q, a.T, a.H, a.W, a.E, a.hidden, a.kt, a.ks, a.nh, a.P = 3, 4, 6, 6, 1152, 896, 4, 3, 9, 0
    a.chunks, a.out_dt, a.l_scale = 3, nv.DT_F32, 0.125
    if fwd:
        for f in POINTERS:
            setattr(a, f, ADDR)
        a.P, a.t_index0, a.y_index0, a.x_index0 = 28, 0, 16, 22
        a.ldo, a.ws, a.ws_bytes = a.hidden, ADDR, 1 << 40
        a.global_row0, a.n_global_rows, a.item_rows = 4, 32, 36
    for k, v in over.items():
        setattr(a, k, v)
    return a


def call(fn, a):
    r = getattr(nv.lib(), f"hicom_compressor_multiguide_{fn}")(None if a is None else ctypes.byref(a))
    return int(r), nv.lib().hicom_last_error().decode()


def _up(n):
    return (n + 255) // 256 * 256


def per_guide_bytes(Q, windows, E, hidden, odt):
    """The Q-sized regions of DESIGN.md §3.8, each rounded up to 256 bytes: qp, o, pre (E floats per guide), hid, tok (hidden floats per
    guide), and per guide and window the fp16 context row, the fp16 hidden row and the readout row of the output dtype."""
    return (3 * _up(Q * E * 4) + 2 * _up(Q * hidden * 4)
            + _up(Q * windows * E * 2) + _up(Q * windows * hidden * 2) + _up(Q * windows * hidden * odt))


@pytest.mark.parametrize("over", [dict(), dict(out_dt=nv.DT_BF16, P=28), dict(T=1, kt=1, H=9, W=9)], ids=["clip_f32", "clip_bf16_pos", "image_9x9"])
def test_workspace_arithmetic(over):
    sizes = [call("workspace_bytes", block(Q=q, **over))[0] for q in range(1, 33)]
    assert all(n > 0 for n in sizes)
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), "workspace_bytes is monotone in Q"
    a = block(**over)
    windows = (a.T // a.kt) * (a.H // a.ks) * (a.W // a.ks)
    odt = 4 if a.out_dt == nv.DT_F32 else 2
    # Q = 1 and Q = 2 share one 32-row pass: every row-sized region (and the logits) is the same, only the per-guide regions grow
    assert sizes[1] - sizes[0] == per_guide_bytes(2, windows, a.E, a.hidden, odt) - per_guide_bytes(1, windows, a.E, a.hidden, odt)
    # the fourth guide opens a second pass of 32 rows: the row-sized regions grow as well
    assert sizes[3] - sizes[2] > per_guide_bytes(4, windows, a.E, a.hidden, odt) - per_guide_bytes(3, windows, a.E, a.hidden, odt)


REFUSALS = {
    "Q = 0": ("workspace_bytes", dict(Q=0), EUNSUP, "1 <= Q <= 32"),
    "Q = 33": ("workspace_bytes", dict(Q=33), EUNSUP, "1 <= Q <= 32"),
    "hidden = 100": ("workspace_bytes", dict(hidden=100), EUNSUP, "multiple of 64"),
    "E = 768": ("workspace_bytes", dict(E=768), EUNSUP, "only 1152"),
    "window of 72 tokens": ("workspace_bytes", dict(T=8, kt=8), EUNSUP, "<= 64"),
    "inexact partition": ("workspace_bytes", dict(H=7), EUNSUP, "exact window partition"),
    "NULL block": ("workspace_bytes", None, EINVAL, "NULL arguments"),
    "fwd: Q = 0": ("fwd", dict(fwd=True, Q=0), EUNSUP, "1 <= Q <= 32"),
    "fwd: Q = 33": ("fwd", dict(fwd=True, Q=33), EUNSUP, "1 <= Q <= 32"),
    "fwd: hidden = 100": ("fwd", dict(fwd=True, hidden=100, ldo=100), EUNSUP, "multiple of 64"),
    "fwd: E = 768": ("fwd", dict(fwd=True, E=768), EUNSUP, "only 1152"),
    "fwd: window of 72 tokens": ("fwd", dict(fwd=True, T=8, kt=8), EUNSUP, "<= 64"),
    "fwd: NULL ff": ("fwd", dict(fwd=True, ff=None), EINVAL, "NULL pointer"),
    "fwd: NULL weight": ("fwd", dict(fwd=True, gw2=None), EINVAL, "NULL weight"),
    "fwd: workspace too small": ("fwd", dict(fwd=True, ws_bytes=4096), EINVAL, "workspace of"),
    "fwd: output layout": ("fwd", dict(fwd=True, item_rows=37), EINVAL, "output layout"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_c_entry_refusals_in_front_of_any_device_call(name):
    fn, kw, code, needle = REFUSALS[name]
    got, msg = call(fn, None if kw is None else block(**kw))
    assert got == code, (got, msg)
    assert msg.startswith("compressor_multiguide: ") and needle in msg, msg


# ---- exact pins ------------------------------------------------------------------------------------------------------------------------------
# The expected sizes, codes and messages below were recorded by running these same argument blocks through the library of commit b2cec2a on the
# host (as tests/test_seg_host_pins.py did for 8633699).
#
# WS_BLOCKS: the three blocks of test_workspace_arithmetic and "clip_f32_chunks9", a block whose marginal region is larger than its logits:
# on the 4 x 6 x 6 clip the logits are rows_pad x 144 floats and the marginals chunks x rows_pad x 48 (marg width of a 6 x 6 grid), equal at the
# file's 3 chunks and larger from 4 on; 9 chunks is the clip's tile count.
#
# PINNED: every refusal in front of the first launch.  Each block breaks one rule of those tested up to the refusal; "too many tokens" and
# "grid 126 x 126" cannot be reached without also exceeding the merge-LDS limits tested BEHIND them (65 (H + W) + 2 T <= 13588 floats bounds
# every grid that passes those to 2.6 M tokens), so the order of the rules is part of what is pinned there.  None launches.
WS_QS = (1, 2, 3, 4, 5, 8, 32)
WS_BLOCKS = {"clip_f32": dict(), "clip_bf16_pos": dict(out_dt=nv.DT_BF16, P=28), "image_9x9": dict(T=1, kt=1, H=9, W=9), "clip_f32_chunks9": dict(chunks=9)}
WS_BYTES = {'clip_f32': {1: 816128, 2: 867840, 3: 919552, 4: 1734912, 5: 1786624, 8: 2706176, 32: 8531456},
 'clip_bf16_pos': {1: 812288, 2: 856832, 3: 901376, 4: 1713152, 5: 1757696, 8: 2659072, 32: 8333056},
 'image_9x9': {1: 849920, 2: 940032, 3: 1030144, 4: 1879296, 5: 1969408, 8: 2999552, 32: 9718784},
 'clip_f32_chunks9': {1: 1739264, 2: 1790976, 3: 1842688, 4: 3581184, 5: 3632896, 8: 5475584, 32: 16839680}}

NL_ROWS = dict(nl_group=2, nl_count=2, nl_first=2, nl_step=3, global_row0=6, item_rows=38)      # a newline row behind every two windows: rows 2 and 5
PINS = {
    "NULL block": ("workspace_bytes", None),
    "NULL block, fwd": ("fwd", None),
    "Q = 0": ("workspace_bytes", dict(Q=0)),
    "Q = 33": ("workspace_bytes", dict(Q=33)),
    "bad shape": ("workspace_bytes", dict(hidden=0)),
    "E = 768": ("workspace_bytes", dict(E=768)),
    "nh = 32": ("workspace_bytes", dict(nh=32)),
    "nh = 7": ("workspace_bytes", dict(nh=7)),
    "hidden = 100": ("workspace_bytes", dict(hidden=100)),
    "output dtype": ("workspace_bytes", dict(out_dt=nv.DT_F16)),
    "pe without kpe": ("workspace_bytes", dict(pe=ADDR, P=28)),
    "inexact partition": ("workspace_bytes", dict(H=7)),
    "temporal partition": ("workspace_bytes", dict(T=5)),
    "window of 72 tokens": ("workspace_bytes", dict(T=8, kt=8)),
    "too many tokens": ("workspace_bytes", dict(H=6000, W=6000)),
    "too many tokens x guides": ("workspace_bytes", dict(Q=32, H=1026, W=1026)),
    "H + W > 1024": ("workspace_bytes", dict(H=516, W=516)),
    "grid 126 x 126": ("workspace_bytes", dict(H=126, W=126)),
    "T = 6800 frames": ("workspace_bytes", dict(T=6800)),
    "fwd: Q = 0": ("fwd", dict(fwd=True, Q=0)),
    "fwd: Q = 33": ("fwd", dict(fwd=True, Q=33)),
    "fwd: hidden = 100": ("fwd", dict(fwd=True, hidden=100, ldo=100)),
    "fwd: E = 768": ("fwd", dict(fwd=True, E=768)),
    "fwd: window of 72 tokens": ("fwd", dict(fwd=True, T=8, kt=8)),
    "fwd: NULL ff": ("fwd", dict(fwd=True, ff=None)),
    "fwd: NULL guide": ("fwd", dict(fwd=True, guide=None)),
    "fwd: NULL out": ("fwd", dict(fwd=True, out=None)),
    "fwd: NULL weight": ("fwd", dict(fwd=True, gw2=None)),
    "fwd: NULL workspace": ("fwd", dict(fwd=True, ws=None)),
    "fwd: workspace too small": ("fwd", dict(fwd=True, ws_bytes=4096)),
    "fwd: workspace misaligned": ("fwd", dict(fwd=True, ws=ADDR + 128)),
    "fwd: unaligned ff": ("fwd", dict(fwd=True, ff=ADDR + 8)),
    "fwd: unaligned fe": ("fwd", dict(fwd=True, fe=ADDR + 8)),
    "fwd: unaligned guide": ("fwd", dict(fwd=True, guide=ADDR + 2)),
    "fwd: output layout": ("fwd", dict(fwd=True, item_rows=37)),
    "fwd: output layout (no global rows)": ("fwd", dict(fwd=True, n_global_rows=0, item_rows=4)),
    "fwd: output layout (ldo < hidden)": ("fwd", dict(fwd=True, ldo=895)),
    "fwd: output layout (nl_group does not divide the windows)": ("fwd", dict(fwd=True, nl_group=3, global_row0=5, item_rows=37)),
    "fwd: newline rows without a newline pointer": ("fwd", dict(fwd=True, newline=None, **NL_ROWS)),
    "fwd: newline rows past the local rows": ("fwd", dict(fwd=True, **{**NL_ROWS, "nl_step": 4})),
    "fwd: local rows": ("fwd", dict(fwd=True, global_row0=5, item_rows=37)),
}
PINNED = {'NULL block': (-1, 'compressor_multiguide: NULL arguments'),
 'NULL block, fwd': (-1, 'compressor_multiguide: NULL arguments'),
 'Q = 0': (-2, 'compressor_multiguide: Q=0 guides (1 <= Q <= 32 per call)'),
 'Q = 33': (-2, 'compressor_multiguide: Q=33 guides (1 <= Q <= 32 per call)'),
 'bad shape': (-1, 'compressor_multiguide: bad shape'),
 'E = 768': (-2, 'compressor_multiguide: E=768 (only 1152)'),
 'nh = 32': (-2, 'compressor_multiguide: 32 heads (<= 16 folded rows per guide)'),
 'nh = 7': (-2, 'compressor_multiguide: 7 heads (<= 16 folded rows per guide)'),
 'hidden = 100': (-2, 'compressor_multiguide: hidden=100 (multiple of 64: fp16 readout planes)'),
 'output dtype': (-2, 'compressor_multiguide: output dtype 2 (bf16 | f32)'),
 'pe without kpe': (-1, 'compressor_multiguide: pe and kpe come together'),
 'inexact partition': (-2, 'compressor_multiguide: needs an exact window partition (T=4 H=7 W=6, windows 4x3x3)'),
 'temporal partition': (-2, 'compressor_multiguide: needs an exact window partition (T=5 H=6 W=6, windows 4x3x3)'),
 'window of 72 tokens': (-2, 'compressor_multiguide: windows of 72 tokens (<= 64)'),
 'too many tokens': (-2, 'compressor_multiguide: too many tokens in one call'),
 'too many tokens x guides': (-2, 'compressor_multiguide: too many tokens in one call'),
 'H + W > 1024': (-2, 'compressor_multiguide: a 516x516 grid: the merge keeps a frame of logits in LDS'),
 'grid 126 x 126': (-2, 'compressor_multiguide: a 126x126 grid: the merge keeps a frame of logits in LDS'),
 'T = 6800 frames': (-2, "compressor_multiguide: T=6800 frames of 6x6: the merge keeps the row's T + H + W weights and 64 frames of marginals in LDS"),
 'fwd: Q = 0': (-2, 'compressor_multiguide: Q=0 guides (1 <= Q <= 32 per call)'),
 'fwd: Q = 33': (-2, 'compressor_multiguide: Q=33 guides (1 <= Q <= 32 per call)'),
 'fwd: hidden = 100': (-2, 'compressor_multiguide: hidden=100 (multiple of 64: fp16 readout planes)'),
 'fwd: E = 768': (-2, 'compressor_multiguide: E=768 (only 1152)'),
 'fwd: window of 72 tokens': (-2, 'compressor_multiguide: windows of 72 tokens (<= 64)'),
 'fwd: NULL ff': (-1, 'compressor_multiguide: NULL pointer'),
 'fwd: NULL guide': (-1, 'compressor_multiguide: NULL pointer'),
 'fwd: NULL out': (-1, 'compressor_multiguide: NULL pointer'),
 'fwd: NULL weight': (-1, 'compressor_multiguide: NULL weight'),
 'fwd: NULL workspace': (-1, 'compressor_multiguide: workspace of 922880 bytes, 256-byte aligned'),
 'fwd: workspace too small': (-1, 'compressor_multiguide: workspace of 922880 bytes, 256-byte aligned'),
 'fwd: workspace misaligned': (-1, 'compressor_multiguide: workspace of 922880 bytes, 256-byte aligned'),
 'fwd: unaligned ff': (-1, 'compressor_multiguide: 16-byte aligned inputs'),
 'fwd: unaligned fe': (-1, 'compressor_multiguide: 16-byte aligned inputs'),
 'fwd: unaligned guide': (-1, 'compressor_multiguide: 16-byte aligned inputs'),
 'fwd: output layout': (-1, 'compressor_multiguide: output layout'),
 'fwd: output layout (no global rows)': (-1, 'compressor_multiguide: output layout'),
 'fwd: output layout (ldo < hidden)': (-1, 'compressor_multiguide: output layout'),
 'fwd: output layout (nl_group does not divide the windows)': (-1, 'compressor_multiguide: output layout'),
 'fwd: newline rows without a newline pointer': (-1, 'compressor_multiguide: newline rows'),
 'fwd: newline rows past the local rows': (-1, 'compressor_multiguide: newline rows'),
 'fwd: local rows': (-1, 'compressor_multiguide: 5 local rows for 4 tokens + 0 newline rows')}


@pytest.mark.parametrize("name", list(WS_BLOCKS))
def test_workspace_bytes_are_the_parents(name):
    got = {q: call("workspace_bytes", block(Q=q, **WS_BLOCKS[name]))[0] for q in WS_QS}
    assert got == WS_BYTES[name]


@pytest.mark.parametrize("name", list(PINS))
def test_refusals_are_the_parents(name):
    fn, kw = PINS[name]
    code, msg = call(fn, None if kw is None else block(**kw))
    assert code < 0, "a block that passes every check must not be in this table: it would launch"
    assert (code, msg) == PINNED[name]


def test_every_case_is_pinned():
    assert sorted(WS_BYTES) == sorted(WS_BLOCKS) and sorted(PINNED) == sorted(PINS)
    assert all(sorted(v) == sorted(WS_QS) and all(n > 0 for n in v.values()) for v in WS_BYTES.values())
    assert all(code in (EINVAL, EUNSUP) and msg.startswith("compressor_multiguide: ") for code, msg in PINNED.values())
    for name, (fn, kw, code, needle) in REFUSALS.items():           # the substring table above is a subset of the pins
        assert PINNED[name][0] == code and needle in PINNED[name][1]
