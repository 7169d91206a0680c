"""CPU checks of the host side of the ragged multi-guide step (csrc/ragged_multi_guide.hip on csrc/segment_host.hpp, hicom_amd/native.py,
hicom_amd/ragged_multi_guide.py): the symbols, the layout of the new argument block as the host C compiler sees it, the workspace
arithmetic, the table arithmetic of the host mirror, and every refusal in front of any device call, by code and message.

As in tests/test_multi_guide_host.py: with chunks > 0 the workspace function and every check in front of the first launch are pure host
code, pointer fields are made-up aligned addresses that nothing reads before a launch, and every *_fwd / *_prepare case breaks one rule, so
none launches or copies."""
import ctypes
import hashlib
from types import SimpleNamespace

import pytest
import torch

import cases
import hicom_amd
from hicom_amd import native as nv
from hicom_amd import ragged
from hicom_amd import ragged_multi_guide as rmg
from host_util import ADDR, EINVAL, EUNSUP

N_CUS = 256
IMAGE, CLIP4, CLIP8 = (1, 1, 0, 0, 0, 1, 32), (4, 4, 0, 0, 0, 1, 32), (8, 4, 0, 0, 0, 1, 32)
MIX6 = [IMAGE, CLIP4, IMAGE, CLIP8, IMAGE]


def block(items=MIX6, counts=(1, 3, 5, 2, 4), n_counts=None, **over):
    """A valid argument block: the MIX6 batch on a 6 x 6 grid, windows of 3 x 3, hidden 64, fp32 rows, 3 token chunks."""
    a = nv.CompressorRaggedMultiGuideArgs()
    a._items = (nv.RaggedItem * len(items))(*[nv.RaggedItem(*d) for d in items])
    a._counts = (ctypes.c_int32 * len(counts))(*counts)
    a.B, a.H, a.W, a.E, a.hidden, a.ks, a.nh, a.P = len(items), 6, 6, 1152, 64, 3, 9, 0
    a.chunks, a.out_dt, a.l_scale = 3, nv.DT_F32, 0.125
    a.items, a.guide_counts, a.n_guide_counts = a._items, a._counts, len(counts) if n_counts is None else n_counts
    for k, v in over.items():
        setattr(a, k, v)
    return a


def call(fn, a):
    r = getattr(nv.lib(), f"hicom_compressor_ragged_multiguide_{fn}")(None if a is None else ctypes.byref(a))
    return int(r), nv.lib().hicom_last_error().decode()


# ---- workspace --------------------------------------------------------------------------------------------------------------------------
def _up(n):
    return (n + 255) // 256 * 256


def per_pair_bytes(M, ctx_rows, rows_out, nh, E, hidden, P, odt):
    """The regions sized by the pairs, each rounded up to 256 bytes: the pair table and the row -> pair lookup; qp, o, pre (E floats per
    pair), hid, tok (hidden floats); per folded row the hi / lo query planes, the positional table and the merged context; per pair and
    window the fp16 context row, the fp16 hidden row and the readout row."""
    R = M * nh
    return (_up(M * 16) + _up(rows_out * 4) + 3 * _up(M * E * 4) + 2 * _up(M * hidden * 4) + 2 * _up(R * E * 2) + _up(R * max(P, 1) * 4) + _up(R * E * 4)
            + _up(ctx_rows * E * 2) + _up(ctx_rows * hidden * 2) + _up(ctx_rows * hidden * odt))


@pytest.mark.parametrize("over", [dict(), dict(out_dt=nv.DT_BF16, P=28, hidden=896)], ids=["f32", "bf16_pos_h896"])
def test_workspace_grows_with_passes_not_with_guides_inside_a_pass(over):
    """One 4-frame clip (4 windows and 4 + 32 rows per pair) with Q = 1 .. 32 guides: inside a pass of 32 folded rows (Q <= 3, 4 .. 7, ...)
    only the pair-sized regions grow; a guide that opens a pass adds the pass's logits and partial states."""
    sizes = {q: call("workspace_bytes", block([CLIP4], (q,), **over))[0] for q in range(1, 33)}
    assert all(n > 0 for n in sizes.values())
    a = block([CLIP4], (1,), **over)
    odt = 4 if a.out_dt == nv.DT_F32 else 2
    pp = lambda q: per_pair_bytes(q, q * 4, q * (4 + 32), a.nh, a.E, a.hidden, a.P, odt)
    ntiles, chunks = 9, 3

    def pass_sized(p):
        """The regions sized by the passes: the work units (32 bytes each), the logits (32 rows per pass), part_m / part_l / part_acc (two
        16-row slots per unit)."""
        return _up(p * chunks * 32) + _up(p * 32 * ntiles * 16 * 4) + 2 * _up(2 * p * chunks * 16 * 4) + _up(2 * p * chunks * 16 * a.E * 4)
    for q in range(2, 33):
        passes, prev = rmg.item_passes(a.nh, q), rmg.item_passes(a.nh, q - 1)
        grown = sizes[q] - sizes[q - 1] - (pp(q) - pp(q - 1))
        assert grown == pass_sized(passes) - pass_sized(prev), (q, grown)
        assert (grown == 0) == (passes == prev)
    assert [rmg.item_passes(9, q) for q in (1, 3, 4, 7, 8, 32)] == [1, 1, 2, 2, 3, 9]


def test_table_region_and_every_region_are_256_byte_aligned():
    """The table region of the host mirror is what the C side puts in front of its regions: sizes differ by whole 256-byte regions, and
    the mirror's image is a whole number of 64-int blocks per table."""
    t = rmg.plan_tables(MIX6, (1, 3, 5, 2, 4), 6, 6, 3, 9, N_CUS, 3)
    img = rmg.table_image(t)
    assert img.size % 64 == 0
    sizes = [call("workspace_bytes", block(chunks=ch))[0] for ch in (1, 2, 3, 18)]
    assert all(n > 0 and n % 256 == 0 for n in sizes) and sizes == sorted(sizes)
    # one more chunk per item and pass: 2 slots of 16 rows (m, l, ACC) and one 32-byte unit per (item, pass); MIX6 has 7 passes in all
    t1, t2 = (rmg.plan_tables(MIX6, (1, 3, 5, 2, 4), 6, 6, 3, 9, N_CUS, ch) for ch in (1, 2))
    assert sum(t1.passes) == 7 and (len(t1.units), len(t2.units)) == (7, 14) and (t1.slots, t2.slots) == (14, 28)
    assert sizes[1] - sizes[0] == _up(28 * 16 * 1152 * 4) - _up(14 * 16 * 1152 * 4) + 2 * (_up(28 * 64) - _up(14 * 64)) + _up(14 * 32) - _up(7 * 32)


# ---- pinned values: the workspace function and the host mirror's table image, recorded before the host walk was shared -----------------
PIN_CASES = {"mix6": (MIX6, (1, 3, 5, 2, 4)), "ones": (MIX6, (1,) * 5), "q32": ([CLIP4], (32,))}
PIN_OVER = {"f32": dict(), "bf16_pos_h896": dict(out_dt=nv.DT_BF16, P=28, hidden=896)}
# (case, chunks) -> workspace bytes (f32, bf16_pos_h896), ints of the table image, first 16 hex digits of its SHA-256 (little-endian int32)
PINS = {
    ("mix6", 1): (2766592, 3098624, 896, "c5f4793c21d15a17"),
    ("mix6", 3): (4835072, 5167104, 1024, "d8c9328a93962cac"),
    ("mix6", 18): (7937536, 8269568, 1216, "5caa2c7971c90e7d"),
    ("ones", 1): (1365760, 1480704, 512, "f4cd85455c6790ad"),
    ("ones", 3): (2843136, 2958080, 576, "a9d4d3826643cfc3"),
    ("ones", 18): (5945600, 6060544, 768, "1cf94ec2c3837f3e"),
    ("q32", 1): (4960000, 5613568, 1536, "e3406d3f95114e43"),
    ("q32", 3): (7619328, 8272896, 1664, "3628efd9b0f678e2"),
    ("q32", 18): (15597568, 16251136, 2112, "4369d903f742e8a7"),
}


@pytest.mark.parametrize("case,chunks", list(PINS))
def test_workspace_bytes_and_table_image_are_pinned(case, chunks):
    """chunks > 0, so no device count enters either figure."""
    items, counts = PIN_CASES[case]
    f32, bf16, ints, digest = PINS[case, chunks]
    got = [call("workspace_bytes", block(items, counts, chunks=chunks, **over))[0] for over in PIN_OVER.values()]
    assert got == [f32, bf16]
    img = rmg.table_image(rmg.plan_tables(items, counts, 6, 6, 3, 9, N_CUS, chunks))
    assert (img.size, hashlib.sha256(img.astype("<i4").tobytes()).hexdigest()[:16]) == (ints, digest)


def projector(hidden=64, **over):
    return hicom_amd.build_vision_projector(SimpleNamespace(**{**cases.DEFAULT_CFG, "hidden_size": hidden, **over}))


@pytest.mark.parametrize("chunks", [0, 1, 3, 18])
def test_single_guides_have_the_ragged_steps_units(chunks):
    proj = projector()
    splits, modals = [1, 4, 1, 8, 1], ["image", "video", "video", "video", "image"]
    desc, ks = ragged.item_descriptors(proj, splits, modals, 6, 6, False, "forward_ragged_multi_guide")
    assert (desc, ks) == ragged.item_descriptors(proj, splits, modals, 6, 6, False)
    t = rmg.plan_tables(desc, [1] * 5, 6, 6, ks, 9, N_CUS, chunks)
    r = ragged.plan_tables(desc, 6, 6, ks, N_CUS, chunks)
    assert t.chunks == r.chunks and t.tok0 == r.tok0 and t.win0 == r.win0 and t.row0 == r.row0 and t.global_row0 == r.global_row0
    assert [u[:3] for u in t.units] == [u[:3] for u in r.units]                                    # item and tile fields
    assert [u[3] for u in t.units] == [0] * len(r.units)                                           # one pass
    assert [u[4] for u in t.units] == [r.slot0[u[0]] * 2 + (u[3] - r.slot0[u[0]]) for u in r.units]      # two row groups per unit
    assert list(t.win_item) == list(r.win_item) and list(t.row_pair) == list(r.row_item)


def test_slots_are_ordered_item_pass_row_group_chunk():
    t = rmg.plan_tables(MIX6, (1, 3, 5, 2, 4), 6, 6, 3, 9, N_CUS, 3)
    assert t.passes == [1, 1, 2, 1, 2] and t.chunks == [3, 3, 3, 3, 3]
    seen = []
    for i, tb, te, p, slot in t.units:
        c = slot - t.slot0[i] - 2 * p * t.chunks[i]
        assert 0 <= c < t.chunks[i] and (tb, te) == (t.ntiles[i] * c // t.chunks[i], t.ntiles[i] * (c + 1) // t.chunks[i])
        seen += [slot, slot + t.chunks[i]]                          # row group 0, row group 1
    assert sorted(seen) == list(range(t.slots))
    assert t.pairs[4] == (2, 0, t.ctx_row0[2], t.row0[2]) and t.pairs[5][2] - t.pairs[4][2] == t.windows[2]
    assert len(t.row_pair) == sum(q * r for q, r in zip(t.Q, t.rows)) and len(t.win_item) == sum(t.windows)


# ---- C refusals ------------------------------------------------------------------------------------------------------------------------
def fwd_block(**over):
    a = block()
    for f in ("ff", "fe", "guide", "out", "lw0_f16", "lb0", "lw2_f16", "lb2", "wq", "bq", "wk", "wv", "bv", "wo", "bo", "gw0", "gb0", "gw2", "gb2"):
        setattr(a, f, ADDR)
    a.ldo, a.ws, a.ws_bytes = a.hidden, ADDR, 1 << 40
    for k, v in over.items():
        setattr(a, k, v)
    return a


BIG = (3000, 4, 0, 0, 0, 1, 32)             # 3000 frames of 200 x 200: 1.2e8 tokens
REFUSALS = {
    "Q_i = 0": (lambda: block(counts=(1, 0, 5, 2, 4)), EUNSUP, "compressor_ragged_multiguide: item 1: Q=0 guides (1 <= Q <= 32 per item)"),
    "Q_i = 33": (lambda: block(counts=(1, 3, 5, 2, 33)), EUNSUP, "compressor_ragged_multiguide: item 4: Q=33 guides (1 <= Q <= 32 per item)"),
    "count array of the wrong length": (lambda: block(n_counts=4), EINVAL, "compressor_ragged_multiguide: 4 guide counts for 5 items (one per item)"),
    "no count array": (lambda: block(guide_counts=None), EINVAL, "compressor_ragged_multiguide: bad shape"),
    "inexact spatial partition": (lambda: block(H=7), EUNSUP, "compressor_ragged_multiguide: needs an exact window partition (H=7 W=6, windows 3x3)"),
    "inexact temporal partition": (lambda: block([IMAGE, (6, 4, 0, 0, 0, 1, 32)], (1, 2)), EUNSUP,
                                   "compressor_ragged_multiguide: item 1 needs an exact window partition (T=6, temporal window 4)"),
    "windows of 72 tokens": (lambda: block([(8, 8, 0, 0, 0, 1, 32)], (2,)), EUNSUP, "compressor_ragged_multiguide: item 0: windows of 72 tokens (<= 64)"),
    "E = 768": (lambda: block(E=768), EUNSUP, "compressor_ragged_multiguide: E=768 (only 1152)"),
    "hidden = 100": (lambda: block(hidden=100), EUNSUP, "compressor_ragged_multiguide: hidden=100 (multiple of 64: fp16 readout planes)"),
    "too many tokens in an item": (lambda: block([(4000, 4, 0, 0, 0, 1, 32)], (1,), H=201, W=201, ks=3), EUNSUP,
                                   "compressor_ragged_multiguide: item 0: too many tokens"),
    "too many tokens": (lambda: block([BIG, BIG], (1, 1), H=200, W=200, ks=4), EUNSUP, "compressor_ragged_multiguide: too many tokens in one call"),
    "too many token x guide products": (lambda: block([BIG], (2,), H=200, W=200, ks=4), EUNSUP,
                                        "compressor_ragged_multiguide: too many token x guide products in one call (240000000, < 2^27)"),
    "too many pairs": (lambda: block([IMAGE] * 200, (32,) * 200), EUNSUP, "compressor_ragged_multiguide: 6400 (item, guide) pairs (<= 4096 per call)"),
    "NULL block": (lambda: None, EINVAL, "compressor_ragged_multiguide: NULL arguments"),
}
FWD_REFUSALS = {
    "fwd: Q_i = 33": (lambda: fwd_block(_counts=None) and block(counts=(1, 3, 5, 2, 33)), EUNSUP, "Q=33 guides"),
    "fwd: NULL ff": (lambda: fwd_block(ff=None), EINVAL, "compressor_ragged_multiguide: NULL pointer"),
    "fwd: NULL weight": (lambda: fwd_block(gw2=None), EINVAL, "compressor_ragged_multiguide: NULL weight"),
    "fwd: workspace too small": (lambda: fwd_block(ws_bytes=4096), EINVAL, "compressor_ragged_multiguide: workspace of"),
    "fwd: workspace misaligned": (lambda: fwd_block(ws=ADDR + 128), EINVAL, "256-byte aligned"),
    "fwd: unaligned guide": (lambda: fwd_block(guide=ADDR + 2), EINVAL, "compressor_ragged_multiguide: 16-byte aligned inputs"),
    "fwd: output layout": (lambda: fwd_block(ldo=63), EINVAL, "compressor_ragged_multiguide: output layout"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
@pytest.mark.parametrize("fn", ["workspace_bytes", "prepare", "fwd"])
def test_c_refusals_by_code_and_message(fn, name):
    make, code, msg = REFUSALS[name]
    got, text = call(fn, make())
    assert (got, text) == (code, msg)


@pytest.mark.parametrize("name", list(FWD_REFUSALS))
def test_c_fwd_refusals_in_front_of_the_first_launch(name):
    make, code, needle = FWD_REFUSALS[name]
    got, text = call("fwd", make())
    assert got == code and needle in text and text.startswith("compressor_ragged_multiguide: "), (got, text)


def test_prepare_refuses_a_missing_workspace_before_it_copies():
    got, text = call("prepare", block())
    assert got == EINVAL and text.startswith("compressor_ragged_multiguide: workspace of") and "256-byte aligned" in text


def test_newline_rows_need_a_newline_token():
    items = [(1, 1, 4, 1, 4, 1, 32)] + MIX6[1:]                 # the first image ends in a newline row
    got, text = call("fwd", fwd_block(items=(nv.RaggedItem * 5)(*[nv.RaggedItem(*d) for d in items])))
    assert (got, text) == (EINVAL, "compressor_ragged_multiguide: item 0 has newline rows and there is no newline token")


# ---- Python refusals that need no device ------------------------------------------------------------------------------------------------
def test_python_refusals_in_front_of_any_tensor_work_leave_no_plan():
    """The module-level refusals come first and need no device: the non-plain recipes, an fp16 module, anyres dicts.  (What needs CUDA
    tensors to get that far -- fp16 tokens into a bf16 module, grad mode, sum(guide_counts) != guide_embeds.shape[0] -- is refused in
    tests/test_gpu_ragged_multi_guide.py.)"""
    ff = torch.zeros((5, 6, 6, 1152), dtype=torch.bfloat16)
    g = torch.zeros((7, 1152), dtype=torch.bfloat16)
    args = (ff, ff, g, [1, 4], [3, 4], ["image", "video"])
    mods = []
    for over in (dict(mm_projector_type="local43_adaptkv_global32"), dict(mm_projector_type="local43_adaptk_global32"), dict(use_guide="coarse")):
        m = projector(**over).to(torch.bfloat16)
        mods.append(m)
        with pytest.raises(NotImplementedError, match="plain release recipe"):
            m.forward_ragged_multi_guide(*args)
    half = projector().to(torch.float16)
    mods.append(half)
    with pytest.raises(NotImplementedError, match="float16"):
        half.forward_ragged_multi_guide(ff.half(), ff.half(), g.half(), *args[3:])
    plain = projector().to(torch.bfloat16)
    mods.append(plain)
    with pytest.raises(NotImplementedError, match="anyres dict"):
        plain.forward_ragged_multi_guide({"base": None, "patch": ff[0]}, None, g, *args[3:])
    with pytest.raises(nv.HicomNativeError, match="GPU only"):
        plain.forward_ragged_multi_guide(*args)
    for m in mods:
        assert not m.__dict__.get(rmg.STORE), "a refusal left a plan behind"
