"""Valid argument blocks of the clip stream entry points, and the tables of the one-field changes that each entry point refuses: what the
host tests of the stream classes, of the groups and the pinned-refusal tests share.  Pointer fields are made-up aligned addresses that
nothing reads before a launch, and every table row breaks one rule, so none launches.

`single`, `multi`, `adapt`, `group` and `group_multi` at the end name each entry point's block builder and table the same way."""
from types import SimpleNamespace

import torch

import cases
from hicom_amd import native as nv
from host_util import ADDR, EINVAL, EUNSUP

ADAPTKV = "local43_adaptkv_global32"


def guides(Q, dtype=torch.bfloat16):
    return torch.zeros((Q, cases.D), dtype=dtype)


# ---- hicom_compressor_stream_push ----------------------------------------------------------------------------------------------------------
def single_push_block(**over):
    a = nv.StreamPushArgs()
    a.Tc, a.H, a.W, a.E, a.kt, a.ks, a.t0, a.rows, a.hidden, a.nparts = 4, 6, 6, 1152, 4, 3, 0, 9, 64, 1
    for f in ("ff", "fe", "q_hi", "q_lo", "pos_a", "pe_hi", "pe_lo", "part_m", "part_l", "part_acc", "ctx_f16", "hid_f16", "state_ml_in", "state_acc",
              "lw0_f16", "lb0", "lw2_f16", "lb2", "out"):
        setattr(a, f, ADDR)
    a.state_ml_out = ADDR + 4096
    a.P, a.y_index0, a.x_index0, a.l_scale, a.out_dt, a.ldo = 28, 16, 22, 0.03, nv.DT_F32, 64
    for k, v in over.items():
        setattr(a, k, v)
    return a


SINGLE_REFUSALS = {
    "E = 768": (dict(E=768), EUNSUP, "only 1152"),
    "13 rows": (dict(rows=13), EUNSUP, "<= 12"),
    "hidden = 100": (dict(hidden=100), EUNSUP, "multiple of 64"),
    "Tc % kt": (dict(Tc=6), EUNSUP, "exact window partition"),
    "window of 72 tokens": (dict(Tc=8, kt=8), EUNSUP, "16 .. 64"),
    "output dtype": (dict(out_dt=nv.DT_F16), EUNSUP, "output dtype"),
    "NULL ff": (dict(ff=None), EINVAL, "NULL pointer"),
    "NULL weight": (dict(lw2_f16=None), EINVAL, "NULL weight"),
    "pe without pos_a": (dict(pos_a=None), EINVAL, "come together"),
    "t0 inside a window group": (dict(t0=2), EINVAL, "whole window groups"),
    "frames past the tables": (dict(t0=16), EINVAL, "outside the positional tables"),
    "unaligned ff": (dict(ff=ADDR + 8), EINVAL, "16-byte aligned"),
    "ldo < hidden": (dict(ldo=63), EINVAL, "output layout"),
    "newline rows without a pointer": (dict(nl_count=2, nl_first=2, nl_step=3), EINVAL, "newline rows"),
}


# ---- hicom_compressor_stream_push_multi ----------------------------------------------------------------------------------------------------
MULTI_POINTERS = ("ff", "fe", "guide", "q_hi", "q_lo", "pos_a", "pe", "part_m", "part_l", "part_acc", "scores", "scratch", "set_ml", "set_acc", "ctx_f16",
            "hid_f16", "loc", "state_ml_in", "state_acc", "lw0_f16", "lb0", "lw2_f16", "lb2", "out")


def multi_push_block(**over):
    """A chunk of 4 frames of 6 x 6 for Q = 3 guides at hidden 64: 4 windows, 27 folded rows; tables for 16 frames."""
    a = nv.StreamPushMultiArgs()
    a.Q, a.Tc, a.H, a.W, a.E, a.kt, a.ks, a.nh, a.t0, a.hidden, a.nparts, a.marg = 3, 4, 6, 6, 1152, 4, 3, 9, 0, 64, 2, 0
    for f in MULTI_POINTERS:
        setattr(a, f, ADDR)
    a.state_ml_out = ADDR + 4096
    a.P, a.y_index0, a.x_index0, a.l_scale, a.out_dt, a.ldo, a.score_stride = 28, 16, 22, 0.03, nv.DT_F32, 64, 144
    a.q_stride, a.row0 = 64 * 48, 0
    for k, v in over.items():
        setattr(a, k, v)
    return a


MULTI_REFUSALS = {
    "Q = 33": (dict(Q=33), EUNSUP, "1 <= Q <= 32"),
    "Q = 0": (dict(Q=0), EUNSUP, "1 <= Q <= 32"),
    "E = 768": (dict(E=768), EUNSUP, "only 1152"),
    "17 heads": (dict(nh=17), EUNSUP, "<= 16 folded rows"),
    "hidden = 100": (dict(hidden=100), EUNSUP, "multiple of 64"),
    "Tc % kt": (dict(Tc=6), EUNSUP, "exact window partition"),
    "window of 72 tokens": (dict(Tc=8, kt=8), EUNSUP, "<= 64"),
    "output dtype": (dict(out_dt=nv.DT_F16), EUNSUP, "output dtype"),
    "more chunks than tiles": (dict(nparts=10), EINVAL, "token chunks"),
    "NULL ff": (dict(ff=None), EINVAL, "NULL pointer"),
    "NULL guide": (dict(guide=None), EINVAL, "NULL pointer"),
    "NULL set": (dict(set_acc=None), EINVAL, "NULL pointer"),
    "NULL state": (dict(state_acc=None), EINVAL, "NULL pointer"),
    "NULL weight": (dict(lw2_f16=None), EINVAL, "NULL weight"),
    "pe without pos_a": (dict(pos_a=None), EINVAL, "come together"),
    "t0 inside a window group": (dict(t0=2), EINVAL, "whole window groups"),
    "frames past the tables": (dict(t0=16), EINVAL, "outside the positional tables"),
    "last frame past the tables": (dict(t0=12, Tc=8), EINVAL, "outside the positional tables"),
    "x rows past the tables": (dict(P=27), EINVAL, "outside the positional tables"),
    "unaligned ff": (dict(ff=ADDR + 8), EINVAL, "aligned"),
    "(M, L) blocks overlap: the same block": (dict(state_ml_out=ADDR), EINVAL, "overlap"),
    "(M, L) blocks overlap: 27 rows need 216 bytes": (dict(state_ml_out=ADDR + 208), EINVAL, "overlap"),
    "marginal form without pos-emb": (dict(marg=1, pe=None, pos_a=None), EUNSUP, "no in-kernel marginals"),
    "short score stride": (dict(score_stride=128), EINVAL, "score_stride"),
    "ldo < hidden": (dict(ldo=63), EINVAL, "output layout"),
    "guides closer than their rows": (dict(row0=46), EINVAL, "output layout"),
    "newline rows without a pointer": (dict(nl_group=2, nl_count=2, nl_first=2, nl_step=3, newline=None), EINVAL, "newline rows"),
    "newline rows off the packing": (dict(nl_group=2, nl_count=2, nl_first=1, nl_step=3, newline=ADDR), EINVAL, "newline rows"),
}


# ---- hicom_compressor_stream_push_multi_adapt ----------------------------------------------------------------------------------------------
def adaptor(**over):
    d = nv.SegAdaptor()
    for f, _ in nv.SegAdaptor._fields_:
        setattr(d, f, ADDR)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def adapt_block(base=None, **over):
    """The chunk of multi_push_block (4 frames of 6 x 6, Q = 3, hidden 64) with both adaptors: 144 tokens, planes and
    hidden planes of 144 x 1152 x 2 = 331776 bytes each."""
    x = nv.StreamPushMultiAdaptArgs()
    x.base = multi_push_block(**(base or {}))
    x.ak, x.av = adaptor(), adaptor()
    x.ky, x.vy, x.adapt_ws, x.adapt_ws_bytes, x.alpha_dt, x.eps = ADDR, ADDR, ADDR, 2 * 331776, nv.DT_BF16, 1e-6
    for k, v in over.items():
        setattr(x, k, v)
    return x


ADAPT_REFUSALS = {
    "both planes NULL": (dict(ky=None, vy=None, ak=adaptor(w0=None), av=adaptor(w0=None)), EINVAL, "neither stream has a prepared plane"),
    "a plane without its adaptor": (dict(av=adaptor(w0=None)), EINVAL, "come together"),
    "an adaptor without its plane": (dict(ky=None), EINVAL, "come together"),
    "workspace one byte short": (dict(adapt_ws_bytes=2 * 331776 - 1), EINVAL, "workspace of 663552 bytes"),
    "NULL workspace": (dict(adapt_ws=None), EINVAL, "workspace of"),
    "workspace off its 256 bytes": (dict(adapt_ws=ADDR + 128), EINVAL, "256-byte aligned"),
    "misaligned key plane": (dict(ky=ADDR + 8), EINVAL, "16-byte aligned planes"),
    "misaligned value plane": (dict(vy=ADDR + 2), EINVAL, "16-byte aligned planes"),
    "alpha dtype": (dict(alpha_dt=nv.DT_F16), EINVAL, "alpha dtype"),
    "NULL LayerNorm weight": (dict(ak=adaptor(gamma=None)), EINVAL, "adaptor weights"),
    "NULL alpha": (dict(av=adaptor(alpha=None)), EINVAL, "adaptor weights"),
    "NULL second layer": (dict(av=adaptor(w2_f16=None)), EINVAL, "adaptor weights"),
}


# ---- hicom_compressor_stream_group_push ----------------------------------------------------------------------------------------------------
def group_push_block(over=None):
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


GROUP_REFUSALS = {
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


# ---- hicom_compressor_stream_group_multi_push ----------------------------------------------------------------------------------------------
def group_multi_push_block(over=None):
    """Three items (4, 8, 4 frames) of a 6 x 6 grid for the slots (2, 0, 1) of a group of 3 with the guide counts (1, 2, 4): M = 7 pairs, slot
    s's first pair (0, 1, 3)[s]; `over`: fields, or (array, index) -> value."""
    a = nv.StreamGroupMultiPushArgs()
    a.B, a.M, a.items, a.H, a.W, a.E, a.kt, a.ks, a.nh, a.hidden, a.chunks = 3, 7, 3, 6, 6, 1152, 4, 3, 9, 64, 2
    for f in ("ff", "fe", "guide", "q_hi", "q_lo", "pos_a", "pe", "ws", "state_ml", "state_acc", "lw0_f16", "lb0", "lw2_f16", "lb2", "out"):
        setattr(a, f, ADDR)
    a.P, a.y_index0, a.x_index0, a.l_scale, a.out_dt, a.ldo, a.pair_rows, a.pair_stride = 28, 16, 22, 0.03, nv.DT_F32, 64, 48, 64 * 48
    for i, (tc, q, slot, t0, row0, pair0) in enumerate(((4, 4, 2, 0, 0, 3), (8, 1, 0, 4, 4, 0), (4, 2, 1, 8, 8, 1))):
        a.tc[i], a.q[i], a.slot[i], a.t0[i], a.row0[i], a.pair0[i] = tc, q, slot, t0, row0, pair0
    a.ws_bytes = 1 << 30
    for k, v in (over or {}).items():
        if isinstance(k, tuple):
            getattr(a, k[0])[k[1]] = v
        else:
            setattr(a, k, v)
    return a


GROUP_MULTI_REFUSALS = {
    "B = 0": ({"B": 0}, EUNSUP, "1 <= B <= 32"),
    "B = 33": ({"B": 33}, EUNSUP, "1 <= B <= 32"),
    "fewer pairs than slots": ({"M": 2}, EINVAL, "M=2 (slot, guide) pairs for 3 slots"),
    "more items than slots": ({"items": 4}, EINVAL, "a slot appears at most once"),
    "E = 768": ({"E": 768}, EUNSUP, "only 1152"),
    "17 heads": ({"nh": 17}, EUNSUP, "<= 16 folded rows"),
    "hidden = 100": ({"hidden": 100}, EUNSUP, "multiple of 64"),
    "Q = 0": ({("q", 1): 0}, EUNSUP, "item 1: Q=0 guides (1 <= Q <= 32 per slot)"),
    "Q = 33": ({("q", 0): 33}, EUNSUP, "item 0: Q=33 guides (1 <= Q <= 32 per slot)"),
    "Tc % kt": ({("tc", 1): 6}, EUNSUP, "item 1 needs an exact window partition"),
    "H % ks": ({"H": 7}, EUNSUP, "exact window partition"),
    "window of 72 tokens": ({"kt": 8, ("tc", 0): 8, ("tc", 2): 8}, EUNSUP, "<= 64"),
    "output dtype": ({"out_dt": nv.DT_F16}, EUNSUP, "output dtype"),
    "a chunk past the merge's LDS": ({"H": 30, "W": 30, ("tc", 1): 1024, "y_index0": 2048, "x_index0": 2078, "P": 2108}, EUNSUP, "marginal sums in LDS"),
    "workspace too small": ({"ws_bytes": 4096}, EINVAL, "workspace of"),
    "unaligned workspace": ({"ws": ADDR + 16}, EINVAL, "256-byte aligned"),
    "NULL ff": ({"ff": None}, EINVAL, "NULL pointer"),
    "NULL state": ({"state_acc": None}, EINVAL, "NULL pointer"),
    "NULL weight": ({"lw2_f16": None}, EINVAL, "NULL weight"),
    "pe without pos_a": ({"pos_a": None}, EINVAL, "come together"),
    "unaligned ff": ({"ff": ADDR + 8}, EINVAL, "16-byte aligned"),
    "unaligned (M, L)": ({"state_ml": ADDR + 4}, EINVAL, "8-byte aligned"),
    "duplicate slot": ({("slot", 2): 0}, EINVAL, "slot 0 appears twice"),
    "slot out of range": ({("slot", 0): 3}, EINVAL, "0 <= slot < B = 3"),
    "negative slot": ({("slot", 0): -1}, EINVAL, "0 <= slot < B = 3"),
    "pairs past M": ({("pair0", 0): 4}, EINVAL, "item 0: pairs 4 .. 8 outside the group's 7 pairs"),
    "negative pair": ({("pair0", 1): -1}, EINVAL, "outside the group's 7 pairs"),
    "two items on one pair": ({("pair0", 2): 2}, EINVAL, "items 0 and 2 share a pair"),
    "t0 inside a window group": ({("t0", 1): 2}, EINVAL, "whole window groups"),
    "frames past the tables": ({("t0", 1): 12}, EINVAL, "item 1: frames 12 .. 20, grid 6x6 outside the positional tables"),
    "rows past the pair's buffer": ({("row0", 1): 41}, EINVAL, "item 1: rows 41 .. 49 outside the pair's buffer of 48 rows"),
    "negative row": ({("row0", 0): -1}, EINVAL, "outside the pair's buffer"),
    "pairs closer than their rows": ({"pair_stride": 64 * 47}, EINVAL, "output layout"),
    "ldo < hidden": ({"ldo": 63}, EINVAL, "output layout"),
    "newline rows without a pointer": ({"nl_group": 2}, EINVAL, "no newline token"),
}


single = SimpleNamespace(push_block=single_push_block, C_REFUSALS=SINGLE_REFUSALS)
multi = SimpleNamespace(push_block=multi_push_block, C_REFUSALS=MULTI_REFUSALS)
adapt = SimpleNamespace(adapt_block=adapt_block, ADAPT_REFUSALS=ADAPT_REFUSALS)
group = SimpleNamespace(push_block=group_push_block, C_REFUSALS=GROUP_REFUSALS)
group_multi = SimpleNamespace(push_block=group_multi_push_block, C_REFUSALS=GROUP_MULTI_REFUSALS)
