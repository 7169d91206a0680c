"""CPU pins of the host side of the two clip stream groups (hicom_amd/clip_stream_group.py, clip_stream_group_multi.py,
csrc/stream_group_host.hpp): one guide per slot and several.

Refusals: every C refusal case of tests/test_clip_stream_group_host.py and test_clip_stream_group_multi_host.py (their tables, by import),
the refusal cases of the two merge + fold entries and of the finish placement, NULL argument blocks, and per flavour one block that breaks
two rules at once (a duplicate slot and a first row past the buffer: the check order decides which is reported) -- each with the status code
and the COMPLETE hicom_last_error() text.  The pointers are made-up aligned addresses that nothing reads before a launch, and every case
breaks a rule in front of the first launch, so nothing here needs a device.

Sizes: ..._workspace_bytes of both flavours with chunks = 2 (explicit chunks: the division does not ask for the CU count).

Blocks: the argument block of two pushes of each class as the real _build_plan and _launch fill it on CPU tensors, with `nv` as the modules
see it replaced by a recorder: every scalar field by value, every pointer field by what it addresses (a tensor of the group, the workspace,
NULL), the per-item arrays up to the item count.

The expected values are literals recorded from a build of commit 740012d ("Add open_stream_group_multi: Q_s guides per slot, batched
finish_many"), the last commit with one host copy per flavour, by running these same cases through it."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import cases
import hicom_amd
from hicom_amd import clip_stream as cs
from hicom_amd import clip_stream_group as csg
from hicom_amd import clip_stream_group_multi as cgm
from hicom_amd import native as nv
from host_util import ADDR, module, tokens
from stream_blocks import group as single, group_multi as multi

FLAVOURS = {"group": (single, "hicom_compressor_stream_group"), "group_multi": (multi, "hicom_compressor_stream_group_multi")}


def ia(*v):
    return (ctypes.c_int32 * len(v))(*v)


# ---- refusals in front of the first launch -----------------------------------------------------------------------------------------------
FOLD = (("pm", ADDR), ("pl", ADDR), ("pa", ADDR), ("scores", ADDR), ("items", 3), ("nparts", 3), ("rows", 9), ("E", 1152), ("Tc", 4), ("H", 6), ("W", 6),
        ("pe", ADDR), ("P", 28), ("y0", 16), ("x0", 22), ("slot", ia(2, 0, 1)), ("t0", ia(8, 0, 4)), ("B", 4), ("ml", ADDR), ("acc", ADDR), ("stream", None))
FOLD_MULTI = (("pm", ADDR), ("pl", ADDR), ("pa", ADDR), ("scores", ADDR), ("items", 3), ("nparts", 3), ("rows", 9), ("Q", 2), ("E", 1152), ("Tc", 4),
              ("H", 6), ("W", 6), ("pe", ADDR), ("P", 28), ("y0", 16), ("x0", 22), ("pair0", ia(4, 0, 2)), ("t0", ia(8, 0, 4)), ("M", 8), ("ml", ADDR),
              ("acc", ADDR), ("stream", None))
PLACE = (("tok", ADDR), ("newline", ADDR), ("B", 3), ("counts", ia(1, 2, 4)), ("row0", ia(8, 4, 12)), ("named", 0b101), ("tail", 1), ("n_rows", 32),
         ("hidden", 64), ("out", ADDR), ("out_dt", nv.DT_F32), ("ldo", 64), ("pair_stride", 64 * 48), ("pair_rows", 48), ("stream", None))
BIG = dict(Tc=1024, H=32, W=32, y0=4096, x0=4128, P=4160)
ENTRY_CASES = {
    "hicom_stream_group_merge_fold_fwd": (FOLD, {
        "NULL partials": dict(pm=None), "NULL slots": dict(slot=None), "17 rows": dict(rows=17), "E % 4": dict(E=1150), "no partials": dict(nparts=0),
        "B = 33": dict(B=33), "more items than slots": dict(items=5), "misaligned partial accumulators": dict(pa=ADDR + 4),
        "misaligned (M, L)": dict(ml=ADDR + 4), "pe without the logits": dict(scores=None), "duplicate slot": dict(slot=ia(2, 0, 2)),
        "slot out of range": dict(slot=ia(2, 0, 4)), "negative t0": dict(t0=ia(8, -4, 4)), "frames past the tables": dict(t0=ia(8, 0, 16)),
        "x rows past the tables": dict(P=27), "a chunk past the merge's LDS": BIG}),
    "hicom_stream_group_multi_merge_fold_fwd": (FOLD_MULTI, {
        "NULL partials": dict(pm=None), "NULL pairs": dict(pair0=None), "17 rows": dict(rows=17), "E % 4": dict(E=1150), "no partials": dict(nparts=0),
        "Q = 0": dict(Q=0), "Q = 33": dict(Q=33), "33 items": dict(items=33), "M = 0": dict(M=0), "misaligned partial accumulators": dict(pa=ADDR + 4),
        "misaligned (M, L)": dict(ml=ADDR + 4), "pe without the logits": dict(scores=None), "two items on one pair": dict(pair0=ia(4, 0, 1)),
        "pairs past M": dict(pair0=ia(4, 0, 7)), "negative t0": dict(t0=ia(8, -4, 4)), "frames past the tables": dict(t0=ia(8, 0, 16)),
        "x rows past the tables": dict(P=27), "too many tokens for M pairs": BIG,
        "a chunk past the merge's LDS": dict(Tc=1000, H=8, W=8, y0=1024, x0=1032, P=1040)}),
    "hicom_stream_group_place_global_fwd": (PLACE, {
        "NULL tok": dict(tok=None), "B = 33": dict(B=33), "output dtype": dict(out_dt=nv.DT_F16), "two tail rows": dict(tail=2), "ldo < hidden": dict(ldo=63),
        "pairs closer than their rows": dict(pair_stride=64 * 47), "a newline row without a pointer": dict(newline=None), "no slot named": dict(named=0),
        "a slot past B named": dict(named=0b1001), "Q = 0": dict(counts=ia(1, 0, 4)), "rows past the pair's buffer": dict(row0=ia(8, 4, 16)),
        "negative row": dict(row0=ia(-1, 4, 12))}),
}
TWO_RULES = {("slot", 2): 0, ("row0", 1): 41}             # a duplicate slot and item 1's rows past the buffer


def refusal_cases():
    """name -> a function that makes the call and returns its status code."""
    L = nv.lib()
    out = {}

    def add(name, fn, *args):
        out[name] = lambda: fn(*args)
    for flavour, (mod, entry) in FLAVOURS.items():
        push = getattr(L, entry + "_push")
        for name, (over, _, _) in mod.C_REFUSALS.items():
            add(f"{flavour}: {name}", lambda o, m=mod, f=push: f(ctypes.byref(m.push_block(o))), over)
        add(f"{flavour}: a duplicate slot and rows past the buffer", lambda m=mod, f=push: f(ctypes.byref(m.push_block(TWO_RULES))))
        add(f"{flavour}: push: NULL arguments", push, None)
        add(f"{flavour}: prepare: NULL arguments", getattr(L, entry + "_prepare"), None)
    for entry, (order, table) in ENTRY_CASES.items():
        for name, kw in table.items():
            add(f"{entry[len('hicom_stream_'):-len('_fwd')]}: {name}", getattr(L, entry), *[kw.get(k, d) for k, d in order])
    return out


TABLES = '(t < 16, y at 16, x at 22, 28 rows)'
REFUSED = {
    'group: B = 0': (-2, 'compressor_stream_group: B=0 slots (1 <= B <= 32 per group)'),
    'group: B = 33': (-2, 'compressor_stream_group: B=33 slots (1 <= B <= 32 per group)'),
    'group: more items than slots': (-1, 'compressor_stream_group: 4 items in one push (1 .. B = 3: a slot appears at most once)'),
    'group: E = 768': (-2, 'compressor_stream_group: E=768 (only 1152)'),
    'group: 17 heads': (-2, 'compressor_stream_group: 17 heads (<= 16 folded rows per slot)'),
    'group: hidden = 100': (-2, 'compressor_stream_group: hidden=100 (multiple of 64: fp16 readout planes)'),
    'group: Tc % kt': (-2, 'compressor_stream_group: item 1 needs an exact window partition (Tc=6, temporal window 4)'),
    'group: H % ks': (-2, 'compressor_stream_group: needs an exact window partition (H=7 W=6, windows 4x3x3)'),
    'group: window of 72 tokens': (-2, 'compressor_stream_group: windows of 72 tokens (<= 64)'),
    'group: output dtype': (-2, 'compressor_stream_group: output dtype 2 (bf16 | f32)'),
    'group: workspace too small': (-1, 'compressor_stream_group: workspace of 524288 bytes, 256-byte aligned'),
    'group: NULL ff': (-1, 'compressor_stream_group: NULL pointer'),
    'group: NULL state': (-1, 'compressor_stream_group: NULL pointer'),
    'group: NULL weight': (-1, 'compressor_stream_group: NULL weight'),
    'group: pe without pos_a': (-1, 'compressor_stream_group: pos_a and pe come together'),
    'group: unaligned ff': (-1, 'compressor_stream_group: 16-byte aligned inputs, planes and accumulators, 8-byte aligned (M, L)'),
    'group: duplicate slot': (-1, 'compressor_stream_group: item 2: slot 0 appears twice in one push (its state is updated in place)'),
    'group: slot out of range': (-1, 'compressor_stream_group: item 0: slot 3 (0 <= slot < B = 3)'),
    'group: negative slot': (-1, 'compressor_stream_group: item 0: slot -1 (0 <= slot < B = 3)'),
    'group: t0 inside a window group': (-1, 'compressor_stream_group: item 1: t0=2 (whole window groups of 4 frames)'),
    'group: frames past the tables': (-1, 'compressor_stream_group: item 1: frames 12 .. 20, grid 6x6 outside the positional tables ' + TABLES),
    "group: rows past the slot's buffer": (-1, "compressor_stream_group: item 1: rows 41 .. 49 outside the slot's buffer of 48 rows"),
    'group: negative row': (-1, "compressor_stream_group: item 0: rows -1 .. 3 outside the slot's buffer of 48 rows"),
    'group: slots closer than their rows': (-1, 'compressor_stream_group: output layout (48 rows per slot, row length 64, slots 3008 elements apart)'),
    'group: ldo < hidden': (-1, 'compressor_stream_group: output layout (48 rows per slot, row length 63, slots 3072 elements apart)'),
    'group: newline rows without a pointer': (-1, 'compressor_stream_group: newline rows (one behind every 2 token rows) and there is no newline token'),
    'group: a duplicate slot and rows past the buffer': (-1, 'compressor_stream_group: item 2: slot 0 appears twice in one push (its state is updated in place)'),
    'group: push: NULL arguments': (-1, 'compressor_stream_group: NULL arguments'),
    'group: prepare: NULL arguments': (-1, 'compressor_stream_group: NULL arguments'),
    'group_multi: B = 0': (-2, 'compressor_stream_group_multi: B=0 slots (1 <= B <= 32 per group)'),
    'group_multi: B = 33': (-2, 'compressor_stream_group_multi: B=33 slots (1 <= B <= 32 per group)'),
    'group_multi: fewer pairs than slots': (-1, 'compressor_stream_group_multi: M=2 (slot, guide) pairs for 3 slots (B <= M <= 1024)'),
    'group_multi: more items than slots': (-1, 'compressor_stream_group_multi: 4 items in one push (1 .. B = 3: a slot appears at most once)'),
    'group_multi: E = 768': (-2, 'compressor_stream_group_multi: E=768 (only 1152)'),
    'group_multi: 17 heads': (-2, 'compressor_stream_group_multi: 17 heads (<= 16 folded rows per pair)'),
    'group_multi: hidden = 100': (-2, 'compressor_stream_group_multi: hidden=100 (multiple of 64: fp16 readout planes)'),
    'group_multi: Q = 0': (-2, 'compressor_stream_group_multi: item 1: Q=0 guides (1 <= Q <= 32 per slot)'),
    'group_multi: Q = 33': (-2, 'compressor_stream_group_multi: item 0: Q=33 guides (1 <= Q <= 32 per slot)'),
    'group_multi: Tc % kt': (-2, 'compressor_stream_group_multi: item 1 needs an exact window partition (Tc=6, temporal window 4)'),
    'group_multi: H % ks': (-2, 'compressor_stream_group_multi: needs an exact window partition (H=7 W=6, windows 4x3x3)'),
    'group_multi: window of 72 tokens': (-2, 'compressor_stream_group_multi: windows of 72 tokens (<= 64)'),
    'group_multi: output dtype': (-2, 'compressor_stream_group_multi: output dtype 2 (bf16 | f32)'),
    "group_multi: a chunk past the merge's LDS": (-2, 'compressor_stream_group_multi: T=1024 frames of 30x30: the merge keeps T (H + W) marginal sums in LDS'),
    'group_multi: workspace too small': (-1, 'compressor_stream_group_multi: workspace of 1360896 bytes, 256-byte aligned'),
    'group_multi: unaligned workspace': (-1, 'compressor_stream_group_multi: workspace of 1360896 bytes, 256-byte aligned'),
    'group_multi: NULL ff': (-1, 'compressor_stream_group_multi: NULL pointer'),
    'group_multi: NULL state': (-1, 'compressor_stream_group_multi: NULL pointer'),
    'group_multi: NULL weight': (-1, 'compressor_stream_group_multi: NULL weight'),
    'group_multi: pe without pos_a': (-1, 'compressor_stream_group_multi: pos_a and pe come together'),
    'group_multi: unaligned ff': (-1, 'compressor_stream_group_multi: 16-byte aligned inputs, planes and accumulators, 8-byte aligned (M, L)'),
    'group_multi: unaligned (M, L)': (-1, 'compressor_stream_group_multi: 16-byte aligned inputs, planes and accumulators, 8-byte aligned (M, L)'),
    'group_multi: duplicate slot': (-1, 'compressor_stream_group_multi: item 2: slot 0 appears twice in one push (its state is updated in place)'),
    'group_multi: slot out of range': (-1, 'compressor_stream_group_multi: item 0: slot 3 (0 <= slot < B = 3)'),
    'group_multi: negative slot': (-1, 'compressor_stream_group_multi: item 0: slot -1 (0 <= slot < B = 3)'),
    'group_multi: pairs past M': (-1, "compressor_stream_group_multi: item 0: pairs 4 .. 8 outside the group's 7 pairs"),
    'group_multi: negative pair': (-1, "compressor_stream_group_multi: item 1: pairs -1 .. 0 outside the group's 7 pairs"),
    'group_multi: two items on one pair': (-1, 'compressor_stream_group_multi: items 0 and 2 share a pair (3 .. 7 and 2 .. 4: a state is updated in place)'),
    'group_multi: t0 inside a window group': (-1, 'compressor_stream_group_multi: item 1: t0=2 (whole window groups of 4 frames)'),
    'group_multi: frames past the tables': (-1, 'compressor_stream_group_multi: item 1: frames 12 .. 20, grid 6x6 outside the positional tables ' + TABLES),
    "group_multi: rows past the pair's buffer": (-1, "compressor_stream_group_multi: item 1: rows 41 .. 49 outside the pair's buffer of 48 rows"),
    'group_multi: negative row': (-1, "compressor_stream_group_multi: item 0: rows -1 .. 3 outside the pair's buffer of 48 rows"),
    'group_multi: pairs closer than their rows': (-1, 'compressor_stream_group_multi: output layout (48 rows per pair, row length 64, pairs 3008 elements apart)'),
    'group_multi: ldo < hidden': (-1, 'compressor_stream_group_multi: output layout (48 rows per pair, row length 63, pairs 3072 elements apart)'),
    'group_multi: newline rows without a pointer': (-1, 'compressor_stream_group_multi: newline rows (one behind every 2 token rows) and there is no newline token'),
    'group_multi: a duplicate slot and rows past the buffer': (-1, 'compressor_stream_group_multi: item 2: slot 0 appears twice in one push (its state is updated in '
                                                                   'place)'),
    'group_multi: push: NULL arguments': (-1, 'compressor_stream_group_multi: NULL arguments'),
    'group_multi: prepare: NULL arguments': (-1, 'compressor_stream_group_multi: NULL arguments'),
    'group_merge_fold: NULL partials': (-1, 'stream_group_merge_fold: NULL pointer'),
    'group_merge_fold: NULL slots': (-1, 'stream_group_merge_fold: NULL pointer'),
    'group_merge_fold: 17 rows': (-1, 'stream_group_merge_fold: bad shape (items=3 nparts=3 rows=17 E=1152 Tc=4 H=6 W=6)'),
    'group_merge_fold: E % 4': (-1, 'stream_group_merge_fold: bad shape (items=3 nparts=3 rows=9 E=1150 Tc=4 H=6 W=6)'),
    'group_merge_fold: no partials': (-1, 'stream_group_merge_fold: bad shape (items=3 nparts=0 rows=9 E=1152 Tc=4 H=6 W=6)'),
    'group_merge_fold: B = 33': (-2, 'stream_group_merge_fold: B=33 slots (1 <= B <= 32 per group)'),
    'group_merge_fold: more items than slots': (-1, 'stream_group_merge_fold: bad shape (items=5 nparts=3 rows=9 E=1152 Tc=4 H=6 W=6)'),
    'group_merge_fold: misaligned partial accumulators': (-1, 'stream_group_merge_fold: 16-byte aligned accumulators, 8-byte aligned (M, L)'),
    'group_merge_fold: misaligned (M, L)': (-1, 'stream_group_merge_fold: 16-byte aligned accumulators, 8-byte aligned (M, L)'),
    'group_merge_fold: pe without the logits': (-1, 'stream_group_merge_fold: the positional term needs the logits'),
    'group_merge_fold: duplicate slot': (-1, 'stream_group_merge_fold: item 2: slot 2 appears twice in one push (its state is updated in place)'),
    'group_merge_fold: slot out of range': (-1, 'stream_group_merge_fold: item 2: slot 4 (0 <= slot < B = 4)'),
    'group_merge_fold: negative t0': (-1, 'stream_group_merge_fold: item 1: t0=-4'),
    'group_merge_fold: frames past the tables': (-1, 'stream_group_merge_fold: item 2: frames 16 .. 20, grid 6x6 outside the positional tables ' + TABLES),
    'group_merge_fold: x rows past the tables': (-1, 'stream_group_merge_fold: item 0: frames 8 .. 12, grid 6x6 outside the positional tables (t < 16, y at 16, x at 22, '
                                                     '27 rows)'),
    "group_merge_fold: a chunk past the merge's LDS": (-2, 'stream_group_merge_fold: Tc=1024 frames of 32x32: the merge keeps Tc (H + W) marginal sums in LDS'),
    'group_multi_merge_fold: NULL partials': (-1, 'stream_group_multi_merge_fold: NULL pointer'),
    'group_multi_merge_fold: NULL pairs': (-1, 'stream_group_multi_merge_fold: NULL pointer'),
    'group_multi_merge_fold: 17 rows': (-1, 'stream_group_multi_merge_fold: bad shape (items=3 M=8 nparts=3 rows=17 E=1152 Tc=4 H=6 W=6)'),
    'group_multi_merge_fold: E % 4': (-1, 'stream_group_multi_merge_fold: bad shape (items=3 M=8 nparts=3 rows=9 E=1150 Tc=4 H=6 W=6)'),
    'group_multi_merge_fold: no partials': (-1, 'stream_group_multi_merge_fold: bad shape (items=3 M=8 nparts=0 rows=9 E=1152 Tc=4 H=6 W=6)'),
    'group_multi_merge_fold: Q = 0': (-2, 'stream_group_multi_merge_fold: Q=0 guides (1 <= Q <= 32 per slot)'),
    'group_multi_merge_fold: Q = 33': (-2, 'stream_group_multi_merge_fold: Q=33 guides (1 <= Q <= 32 per slot)'),
    'group_multi_merge_fold: 33 items': (-1, 'stream_group_multi_merge_fold: bad shape (items=33 M=8 nparts=3 rows=9 E=1152 Tc=4 H=6 W=6)'),
    'group_multi_merge_fold: M = 0': (-1, 'stream_group_multi_merge_fold: bad shape (items=3 M=0 nparts=3 rows=9 E=1152 Tc=4 H=6 W=6)'),
    'group_multi_merge_fold: misaligned partial accumulators': (-1, 'stream_group_multi_merge_fold: 16-byte aligned accumulators, 8-byte aligned (M, L)'),
    'group_multi_merge_fold: misaligned (M, L)': (-1, 'stream_group_multi_merge_fold: 16-byte aligned accumulators, 8-byte aligned (M, L)'),
    'group_multi_merge_fold: pe without the logits': (-1, 'stream_group_multi_merge_fold: the positional term needs the logits'),
    'group_multi_merge_fold: two items on one pair': (-1, 'stream_group_multi_merge_fold: items 1 and 2 share a pair (0 .. 2 and 1 .. 3: a state is updated in place)'),
    'group_multi_merge_fold: pairs past M': (-1, "stream_group_multi_merge_fold: item 2: pairs 7 .. 9 outside the group's 8 pairs"),
    'group_multi_merge_fold: negative t0': (-1, 'stream_group_multi_merge_fold: item 1: t0=-4'),
    'group_multi_merge_fold: frames past the tables': (-1, 'stream_group_multi_merge_fold: item 2: frames 16 .. 20, grid 6x6 outside the positional tables ' + TABLES),
    'group_multi_merge_fold: x rows past the tables': (-1, 'stream_group_multi_merge_fold: item 0: frames 8 .. 12, grid 6x6 outside the positional tables (t < 16, y at '
                                                           '16, x at 22, 27 rows)'),
    'group_multi_merge_fold: too many tokens for M pairs': (-1, 'stream_group_multi_merge_fold: bad shape (items=3 M=8 nparts=3 rows=9 E=1152 Tc=1024 H=32 W=32)'),
    "group_multi_merge_fold: a chunk past the merge's LDS": (-2, 'stream_group_multi_merge_fold: Tc=1000 frames of 8x8: the merge keeps Tc (H + W) marginal sums in '
                                                                 'LDS'),
    'group_place_global: NULL tok': (-1, 'stream_group_place_global: NULL pointer'),
    'group_place_global: B = 33': (-2, 'stream_group_place_global: B=33 slots (1 <= B <= 32 per group)'),
    'group_place_global: output dtype': (-2, 'stream_group_place_global: output dtype 2 (bf16 | f32)'),
    'group_place_global: two tail rows': (-1, 'stream_group_place_global: bad shape (hidden=64, 32 global rows behind 2 newline rows, 48 rows per pair of 64 elements, '
                                              'pairs 3072 elements apart)'),
    'group_place_global: ldo < hidden': (-1, 'stream_group_place_global: bad shape (hidden=64, 32 global rows behind 1 newline rows, 48 rows per pair of 63 elements, '
                                             'pairs 3072 elements apart)'),
    'group_place_global: pairs closer than their rows': (-1, 'stream_group_place_global: bad shape (hidden=64, 32 global rows behind 1 newline rows, 48 rows per pair '
                                                             'of 64 elements, pairs 3008 elements apart)'),
    'group_place_global: a newline row without a pointer': (-1, 'stream_group_place_global: a newline row and there is no newline token'),
    'group_place_global: no slot named': (-1, 'stream_group_place_global: named slots 0 (a non-empty set of the 3 slots)'),
    'group_place_global: a slot past B named': (-1, 'stream_group_place_global: named slots 0x9 (a non-empty set of the 3 slots)'),
    'group_place_global: Q = 0': (-2, 'stream_group_place_global: slot 1: Q=0 guides (1 <= Q <= 32 per slot)'),
    "group_place_global: rows past the pair's buffer": (-1, "stream_group_place_global: slot 2: rows 16 .. 49 outside the pair's buffer of 48 rows"),
    'group_place_global: negative row': (-1, "stream_group_place_global: slot 0: rows -1 .. 32 outside the pair's buffer of 48 rows"),
}


@pytest.mark.parametrize("name", list(refusal_cases()))
def test_refusals_are_the_parents_code_and_text(name):
    code = int(refusal_cases()[name]())
    msg = nv.lib().hicom_last_error().decode()
    assert code < 0, "a block that passes every check must not be in this table: it would launch"
    assert (code, msg) == REFUSED[name]


# ---- workspace sizes ---------------------------------------------------------------------------------------------------------------------
def size_block(mod, tcs, qs=None):
    """The host tests' block (chunks = 2) with the items `tcs` in the slots 0 .. and, for the multi flavour, the guide counts `qs`."""
    over = {"B": len(tcs), "items": len(tcs)}
    for i, n in enumerate(tcs):
        over[("tc", i)] = n
    if qs is not None:
        over["M"] = sum(qs)
        for i, q in enumerate(qs):
            over[("q", i)] = q
    return mod.push_block(over)


SIZE_CASES = {
    "group: the host tests' block": ("group", (4, 8, 4), None),
    "group: one item": ("group", (8,), None),
    "group: 32 items of 4 frames": ("group", (4,) * 32, None),
    "group_multi: the host tests' block": ("group_multi", (4, 8, 4), (4, 1, 2)),
    "group_multi: the host tests' block, one guide each": ("group_multi", (4, 8, 4), (1, 1, 1)),
    "group_multi: one item, q = 1": ("group_multi", (8,), (1,)),
    "group_multi: one item, q = 16": ("group_multi", (8,), (16,)),                 # nh q = 144: 4.5 passes of 32 rows
    "group_multi: one item, q = 17": ("group_multi", (8,), (17,)),
    "group_multi: one item, q = 32": ("group_multi", (8,), (32,)),
    "group_multi: one item, q = 3": ("group_multi", (8,), (3,)),                   # nh q = 27: one pass
    "group_multi: one item, q = 4": ("group_multi", (8,), (4,)),                   # nh q = 36: two
    "group_multi: 32 items of 4 frames, one guide each": ("group_multi", (4,) * 32, (1,) * 32),
    "group_multi: 32 items of 4 frames, q = 3": ("group_multi", (4,) * 32, (3,) * 32),
}
SIZES = {
    "group: the host tests' block": 524288,
    'group: one item': 188928,
    'group: 32 items of 4 frames': 5369344,
    "group_multi: the host tests' block": 1360896,
    "group_multi: the host tests' block, one guide each": 1004032,
    'group_multi: one item, q = 1': 354816,
    'group_multi: one item, q = 16': 2007040,
    'group_multi: one item, q = 17': 2028800,
    'group_multi: one item, q = 32': 3681024,
    'group_multi: one item, q = 3': 397824,
    'group_multi: one item, q = 4': 751616,
    'group_multi: 32 items of 4 frames, one guide each': 10392576,
    'group_multi: 32 items of 4 frames, q = 3': 11081728,
}


@pytest.mark.parametrize("name", list(SIZE_CASES))
def test_workspace_bytes_are_the_parents(name):
    flavour, tcs, qs = SIZE_CASES[name]
    mod, entry = FLAVOURS[flavour]
    a = size_block(mod, tcs, qs)
    assert a.chunks == 2
    assert getattr(nv.lib(), entry + "_workspace_bytes")(ctypes.byref(a)) == SIZES[name]


# ---- the argument block of a push -----------------------------------------------------------------------------------------------------------
ARRAYS = ("tc", "q", "slot", "t0", "row0", "pair0")
WS_BYTES = 65536
PUSHES = (((0, 4), (1, 8), (2, 4)), ((1, 4), (0, 8)))      # (slot, frames) per item; the second push: t0, row0 and a slot order other than range(B)
COUNTS = (1, 2, 4)


def describe(block, names, ws):
    """{field: value} of a push block: a pointer field by what it addresses, a per-item array as the tuple of its first `items` entries."""
    out = {}
    for f, t in block._fields_:
        v = getattr(block, f)
        if f in ARRAYS:
            out[f] = tuple(v[:block.items])
        elif t is ctypes.c_void_p and v is not None and f != "stream":
            out[f] = names.get(v) or ("ws" if v == ws.data_ptr() else hex(v))
        else:
            out[f] = v
    return out


def t(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def recorded(monkeypatch, kind):
    """A group of class `kind` with three slots on the geometry of the host tests (6 x 6 grid, kt = 4, ks = 3, hidden 64, 16 frames, `grid`
    newline rows) whose tensors live on the CPU, pushed twice (PUSHES) through the real push, _build_plan and _launch -> the descriptions of
    the two blocks the native push was handed."""
    blocks, tensors = [], {}

    def push(a):
        g = tensors["group"]
        names = {x.data_ptr(): n for n, x in tensors.items() if isinstance(x, torch.Tensor)}
        names.update({x.data_ptr(): n for n, x in (("guides", g.guides), ("q_hi", g.q_hi), ("q_lo", g.q_lo), ("pos_a", g.pos_a), ("pe", g.pe),
                                                   ("state_ml", g.state_ml), ("state_acc", g.state_acc), ("out", g.out), ("newline", g.newline))})
        assert len(names) == 15, "the tensors a block may point at have addresses of their own"
        plan = next(p for p in g.proj.__dict__[g.STORE].values() if p.args is a)
        assert plan.ws.numel() == WS_BYTES
        blocks.append(describe(a, names, plan.ws))
    fake = SimpleNamespace(StreamGroupPushArgs=nv.StreamGroupPushArgs, StreamGroupMultiPushArgs=nv.StreamGroupMultiPushArgs, DT_F32=nv.DT_F32, DT_BF16=nv.DT_BF16,
                           GROUP_MAX=nv.GROUP_MAX, compressor_stream_group_workspace=lambda a: WS_BYTES, compressor_stream_group_multi_workspace=lambda a: WS_BYTES,
                           compressor_stream_group_prepare=lambda a: None, compressor_stream_group_multi_prepare=lambda a: None,
                           compressor_stream_group_push=push, compressor_stream_group_multi_push=push)
    for mod in (cs, csg, cgm):
        monkeypatch.setattr(mod, "nv", fake)
    monkeypatch.setattr(cs, "_require_bf16_cuda", lambda name, x: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: SimpleNamespace(cuda_stream=7))
    monkeypatch.setattr(hicom_amd.projector, "_linear_params", lambda lin: (lin.weight, lin.bias))
    G = csg.ClipStreamGroup if kind == "group" else cgm.ClipStreamGroupMulti

    def allocate(self, rows):
        units = self.Q                                           # slots of the single class, pairs of the multi class: the guide rows
        self.out = t(units, rows, self.hidden)
        self.state_ml, self.state_acc = t(units * self.nh, 2), t(units * self.nh, self.E)
        self.q_hi, self.q_lo, self.pos_a, self.pe = t(64, 8), t(64, 8), t(64, 28), t(28, 8)
        self.P, self.y0, self.x0 = 28, 16, 22
    monkeypatch.setattr(G, "_allocate", allocate)
    monkeypatch.setattr(G, "_prepare", lambda self, guides, slot=None: setattr(self, "guides", guides))
    m = module(mm_newline_position="grid")
    lc = m.local_compressor
    tensors.update({"readout_f16()[0]": t(4), "readout_f16()[1]": t(4), "readout[0].bias": lc.readout[0].bias, "readout[2].bias": lc.readout[2].bias,
                    "ff": tokens(16), "fe": tokens(16)})
    monkeypatch.setattr(type(lc), "readout_f16", lambda self: (tensors["readout_f16()[0]"], tensors["readout_f16()[1]"]))
    nl = t(64, dtype=torch.bfloat16)
    with torch.no_grad():
        if kind == "group":
            g = m.open_stream_group(t(3, cases.D, dtype=torch.bfloat16), 6, 6, 16, nl)
        else:
            g = m.open_stream_group_multi(t(sum(COUNTS), cases.D, dtype=torch.bfloat16), COUNTS, 6, 6, 16, nl)
        tensors["group"] = g
        for i, items in enumerate(PUSHES):
            n = sum(tc for _, tc in items)
            g.push(tensors["ff"][:n], tensors["fe"][:n], [tc for _, tc in items], [s for s, _ in items])
    return blocks


# what the four blocks agree on (a plan's block holds chunks = 0: the share of the CUs, which a real workspace call would ask for)
SHARED = {'ff': 'ff', 'fe': 'fe', 'guide': 'guides', 'B': 3, 'H': 6, 'W': 6, 'E': 1152, 'kt': 4, 'ks': 3, 'nh': 9, 'hidden': 64, 'chunks': 0, 'q_hi': 'q_hi',
          'q_lo': 'q_lo', 'pos_a': 'pos_a', 'pe': 'pe', 'P': 28, 'y_index0': 16, 'x_index0': 22, 'l_scale': 0.02946278266608715, 'ws': 'ws', 'ws_bytes': 65536,
          'state_ml': 'state_ml', 'state_acc': 'state_acc', 'lw0_f16': 'readout_f16()[0]', 'lb0': 'readout[0].bias', 'lw2_f16': 'readout_f16()[1]',
          'lb2': 'readout[2].bias', 'out': 'out', 'out_dt': 0, 'nl_group': 2, 'ldo': 64, 'newline': 'newline', 'stream': 7}
SINGLE = {**SHARED, 'slot_stride': 3584, 'slot_rows': 56}
MULTI = {**SHARED, 'M': 7, 'reserved_': 0, 'pair_stride': 3584, 'pair_rows': 56}
BLOCKS = {
    'group': [{**SINGLE, 'items': 3, 'tc': (4, 8, 4), 'slot': (0, 1, 2), 't0': (0, 0, 0), 'row0': (0, 0, 0)},
              {**SINGLE, 'items': 2, 'tc': (4, 8), 'slot': (1, 0), 't0': (8, 4), 'row0': (12, 6)}],
    'group_multi': [{**MULTI, 'items': 3, 'tc': (4, 8, 4), 'q': (1, 2, 4), 'slot': (0, 1, 2), 't0': (0, 0, 0), 'row0': (0, 0, 0), 'pair0': (0, 1, 3)},
                    {**MULTI, 'items': 2, 'tc': (4, 8), 'q': (2, 1), 'slot': (1, 0), 't0': (8, 4), 'row0': (12, 6), 'pair0': (1, 0)}],
}


@pytest.mark.parametrize("kind", ["group", "group_multi"])
def test_push_blocks_are_the_parents_field_for_field(monkeypatch, kind):
    got = recorded(monkeypatch, kind)
    want = BLOCKS[kind]
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert g == w, {k: (g.get(k), w.get(k)) for k in set(g) | set(w) if g.get(k) != w.get(k)}


def test_every_case_is_pinned():
    assert sorted(REFUSED) == sorted(refusal_cases()) and sorted(SIZES) == sorted(SIZE_CASES)
    assert all(code in (-1, -2) for code, _ in REFUSED.values()) and all(n > 0 and n % 256 == 0 for n in SIZES.values())
    for flavour, first in (("group", "slot 0 appears twice"), ("group_multi", "slot 0 appears twice")):      # the slot check is in front of the rows' check
        assert first in REFUSED[f"{flavour}: a duplicate slot and rows past the buffer"][1]
    for b in (b for pair in BLOCKS.values() for b in pair):            # every pointer of a block is named: none is a bare address
        assert all(not isinstance(v, str) or not v.startswith("0x") for v in b.values())
