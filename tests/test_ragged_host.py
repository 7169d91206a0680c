"""CPU checks of the ragged step's surface (header, binding and module agree on the new entry points) and of its table arithmetic:
hicom_amd.ragged.plan_tables restates what hicom_compressor_ragged_prepare writes into the workspace's table region
(tests/test_gpu_ragged.py holds the device's copy against it)."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest

import cases
import hicom_amd
from hicom_amd import native, ragged
from hicom_amd.projector import HIComProjector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "hicom_hip.h")).read()
NEW = ("hicom_compressor_ragged_workspace_bytes", "hicom_compressor_ragged_prepare", "hicom_compressor_ragged_fwd")
N_CUS = 256              # the stated CU count of the division tests (MI355X)


def test_ragged_entry_points_are_declared_exported_and_bound():
    lib = ctypes.CDLL(native.LIB_PATH)                 # loading needs no GPU; no compute call is made
    for name in NEW:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", HEADER)
        assert m, f"{name} is not declared in include/hicom_hip.h"
        assert name in native.EXPORTS and hasattr(lib, name)
        n_declared = len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(native.lib(), name).argtypes) == n_declared == 1
    assert native.lib().hicom_compressor_ragged_workspace_bytes.restype is ctypes.c_int64
    assert native.lib().hicom_compressor_ragged_fwd.restype is ctypes.c_int
    assert native.ABI_VERSION == 16 and "#define HICOM_ABI_VERSION 16" in HEADER


def declared_fields(struct):
    body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        head = re.match(r"(const\s+)?(\w+)", stmt)
        base = head.group(2)
        for var in stmt[head.end():].split(","):
            var = var.strip()
            if var.startswith("*"):
                kind = ctypes.POINTER(native.RaggedItem) if base == "hicom_ragged_item" else ctypes.c_void_p
            else:
                kind = ctype[base]
            out.append((var.lstrip("* "), kind))
    return out


def test_ragged_structs_match_the_header_field_for_field():
    assert list(native.RaggedItem._fields_) == declared_fields("hicom_ragged_item")
    assert [n for n, _ in native.RaggedItem._fields_] == ["T", "kt", "nl_group", "nl_count", "nl_first", "nl_step", "n_global_rows"]
    assert list(native.CompressorRaggedArgs._fields_) == declared_fields("hicom_compressor_ragged_args")


def test_projector_has_forward_ragged_and_the_package_exports_are_unchanged():
    assert callable(getattr(HIComProjector, "forward_ragged"))
    assert not any("ragged" in n.lower() for n in getattr(hicom_amd, "__all__"))


# ---- table arithmetic ------------------------------------------------------------------------------------------------------------
def projector(hidden=64, **over):
    return hicom_amd.build_vision_projector(SimpleNamespace(**{**cases.DEFAULT_CFG, "hidden_size": hidden, **over}))


MIXES = {
    "6x6": (6, [1, 4, 1, 8, 1], ["image", "video", "video", "video", "image"], {}, False),
    "27x27": (27, [1, 64] + [1] * 14, ["image", "video"] + ["image"] * 14, {"max_num_frames": 64}, False),
    "9x9_grid_newline": (9, [1, 4], ["image", "video"], {"mm_newline_position": "grid"}, True),
}


@pytest.fixture(scope="module", params=sorted(MIXES))
def mix(request):
    side, splits, modals, over, newline = MIXES[request.param]
    proj = projector(**over)
    desc, ks = ragged.item_descriptors(proj, splits, modals, side, side, newline)
    return SimpleNamespace(name=request.param, side=side, splits=splits, modals=modals, proj=proj, desc=desc, ks=ks, newline=newline,
                           tables=ragged.plan_tables(desc, side, side, ks, N_CUS))


def test_work_units_cover_each_items_tiles_once_in_order(mix):
    t = mix.tables
    assert [u[3] for u in t.units] == list(range(len(t.units)))                 # slot = position in the list
    for i, ntiles in enumerate(t.ntiles):
        mine = [u for u in t.units if u[0] == i]
        assert len(mine) == t.chunks[i] and [u[3] for u in mine] == list(range(t.slot0[i], t.slot0[i] + t.chunks[i]))
        assert mine[0][1] == 0 and mine[-1][2] == ntiles                        # the item's tiles, counted from ITS first token
        assert all(a[2] == b[1] for a, b in zip(mine, mine[1:]))                # no gap, no overlap, in order
        assert all(u[1] < u[2] for u in mine)                                   # no empty unit; none spans two items by construction
        assert ntiles == (mix.splits[i] * mix.side * mix.side + 15) // 16


def test_unit_count_is_bounded(mix):
    t = mix.tables
    B = len(mix.splits)
    assert len(t.units) <= 2 * N_CUS + B
    assert all(1 <= c <= min(n, 64) for c, n in zip(t.chunks, t.ntiles))
    if mix.name == "27x27":
        assert t.ntiles[1] == 2916 and t.chunks[1] == 64                        # the 64-frame item: capped
        assert len(set(t.chunks[2:])) == 1                                      # equal items, equal shares


def test_chunks_override_is_clamped_per_item():
    proj = projector()
    desc, ks = ragged.item_descriptors(proj, [1, 4, 1, 8, 1], ["image", "video", "video", "video", "image"], 6, 6, False)
    assert ragged.plan_tables(desc, 6, 6, ks, N_CUS, 18).chunks == [3, 9, 3, 18, 3]
    assert ragged.plan_tables(desc, 6, 6, ks, N_CUS, 1).chunks == [1] * 5


def test_division_is_a_function_of_the_item_and_the_totals_only():
    """Permuting the items permutes the division."""
    proj = projector()
    splits, modals = [1, 4, 1, 8, 1], ["image", "video", "video", "video", "image"]
    fwd = ragged.plan_tables(ragged.item_descriptors(proj, splits, modals, 6, 6, False)[0], 6, 6, 3, N_CUS)
    rev = ragged.plan_tables(ragged.item_descriptors(proj, splits[::-1], modals[::-1], 6, 6, False)[0], 6, 6, 3, N_CUS)
    assert rev.chunks == fwd.chunks[::-1]


def test_offsets_are_prefix_sums_of_layout_and_tilings(mix):
    t, proj = mix.tables, mix.proj
    tok = win = row = 0
    for i, (T, modal) in enumerate(zip(mix.splits, mix.modals)):
        at, ay, ax = proj.local_compressor.tilings(T, mix.side, mix.side, modal)
        lay = proj._layout((at.nwin, ay.nwin, ax.nwin), modal, mix.newline, False)
        assert mix.desc[i][1] == at.k == (1 if (modal == "image" or T == 1) else proj.local_compressor.temporal_kernel_size)
        assert (t.tok0[i], t.win0[i], t.row0[i]) == (tok, win, row)
        assert t.N[i] == T * mix.side * mix.side and t.windows[i] == at.nwin * ay.nwin * ax.nwin == lay.n_tokens
        assert t.global_row0[i] == lay.n_rows and t.rows[i] == lay.n_rows + proj.global_compressor.num_queries
        assert t.score_off[i] == sum(16 * n for n in t.ntiles[:i])
        # the three newline integers reproduce the layout's newline rows, and every other local row a token
        _, _, nl_group, nl_count, nl_first, nl_step, _ = mix.desc[i]
        assert [nl_first + k * nl_step for k in range(nl_count)] == lay.newline_rows and nl_group == lay.nl_group
        token_rows = [r for r in range(lay.n_rows) if r not in set(lay.newline_rows)]
        assert token_rows == [lay.row_of(m) for m in range(lay.n_tokens)]
        assert [r - r // (nl_group + 1) if nl_group else r for r in token_rows] == list(range(lay.n_tokens))
        assert list(t.win_item[win:win + t.windows[i]]) == [i] * t.windows[i] and list(t.row_item[row:row + t.rows[i]]) == [i] * t.rows[i]
        tok, win, row = tok + t.N[i], win + t.windows[i], row + t.rows[i]
    assert len(t.win_item) == win and len(t.row_item) == row
    if mix.name == "6x6":
        assert t.tok0 == [0, 36, 180, 216, 504] and all(x % 16 for x in t.tok0[1:])
    if mix.name == "9x9_grid_newline":
        assert t.rows[0] != t.rows[1] and mix.desc[0][5] != mix.desc[1][5]      # other row counts, other newline strides


def test_workspace_function_refuses_without_a_device_call():
    """hicom_compressor_ragged_workspace_bytes is host arithmetic: a video item whose T is no multiple of its window is HICOM_EUNSUP."""
    a = native.CompressorRaggedArgs()
    items = (native.RaggedItem * 2)(native.RaggedItem(1, 1, 0, 0, 0, 1, 32), native.RaggedItem(6, 4, 0, 0, 0, 1, 32))
    a.B, a.H, a.W, a.E, a.hidden, a.ks, a.nh, a.chunks, a.items = 2, 6, 6, 1152, 64, 3, 9, 1, items
    with pytest.raises(NotImplementedError, match="item 1.*partition"):
        native.compressor_ragged_workspace(a)
    items[1].T = 8
    n1 = native.compressor_ragged_workspace(a)
    a.chunks = 3
    assert 0 < n1 < native.compressor_ragged_workspace(a)                         # more units, more partial states
