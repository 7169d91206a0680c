// Host side of the two clip stream group pushes, written once: the shape check, the workspace layout, the per-push
// values, the slot check, workspace_bytes, prepare's item walk and upload, every check of a push in front of the first launch, the
// six-launch sequence with its parameter fill (launch 1 behind a flavour hook), and the stand-alone merge + fold entry.
// clip_stream_group.hip (one guide per slot) and clip_stream_group_multi.hip (several) keep their kernels, their table structs and a
// flavour description F; the functions here are templates over F and read `a->field` directly (the two argument blocks name every common field alike).  F says what truly differs:
//   Args, Item, Unit, StreamParams, MergeParams, PlaceParams; the kernels local, stream, merge, place
//   kWho, kFoldWho: the message prefixes; kUnit: what owns one state and one part of the output ("slot" | "pair")
//   kRowGroups: a stream workgroup has 256 kRowGroups threads and 16 kRowGroups folded rows, one pass of an item's row space
//   kStride, kRows, kPlaceStride: the members of Args and PlaceParams with the output's stride and rows per kUnit
//   guides(a, i); unit0(a): the per-item array of first units (slot | first pair); write(item, units, walk): an item's table entries
//   check_group, check_item, check_totals, check_units, check_fold_shape, check_fold_units: the flavour's own requirements, each at its
//   place in the order of the checks; uniform_guides(p, Q): the guide count of the stand-alone entry's items
// A flavour is also an OBJECT (`f`, default-constructed for the two plain flavours), for what a push may put in FRONT of launch 2:
//   f.regions(a, l, take): further workspace regions behind `loc` (l.front[]), so that every plain offset and total stays what it is
//   f.check_shape(a, tokens), f.check_push(a, l): its requirements on the tuple (behind check_totals) and on a push (behind the plain
//   checks, in front of the first launch); f.front(a, l, key_x, push): the launches that leave the fp16 contexts in ws + l.ctx16
// GroupPlainFront<F> is the trivial form -- no region, no requirement, launch 1 = F::local -- which the two plain flavours inherit; the
// k / v adaptor flavour (clip_stream_group_multi.hip) is Multi with the four of its own.
#pragma once
#include <vector>

#include "segment_host.hpp"

namespace hicom {

constexpr int kGroupMax = 32;            // slots per group, items per push and guides per slot

// what changes from push to push, per item of the call: by value in the kernel arguments
struct GroupPush {
    union { int slot[kGroupMax]; int pair0[kGroupMax]; };      // the item's slot | the first pair of the item's slot
    int t0[kGroupMax];
    int row0[kGroupMax];
};

}  // namespace hicom

namespace hicom_host {

using namespace hicom;

struct GroupLayout {
    long items, units, win_item, row_item, table_bytes;     // the table region
    long scores, part_m, part_l, part_acc, ctx16, hid16, loc, total;
    long front[3];                                          // the regions of the flavour's front step, behind loc (0: absent)
    long windows, ctx_rows, rows, slots, nunits, work_sum, score16, tokens;
    int max_T, max_Q, wps;
};

// one item of the walk over the tuple: where its tokens, windows, partial-state slots, logits (in 16 floats), context rows and chunk rows begin
struct GroupWalk {
    int i, T, Q, chunks;
    long tok, N, ntiles, passes, win, wins, nl, slot, score, ctx_row, row;
};

template <class A>
inline long group_item_win(const A* a, int i, int wps) { return (long)(a->tc[i] / a->kt) * wps; }
template <class A>
inline long group_item_nl(const A* a, int i, int wps) { return a->nl_group > 0 ? group_item_win(a, i, wps) / a->nl_group : 0; }
template <class F>
inline long group_item_passes(const typename F::Args* a, int i) { return ((long)a->nh * F::guides(a, i) + 16 * F::kRowGroups - 1) / (16 * F::kRowGroups); }

// everything that the tuple of the items and the geometry decide: the checks of workspace_bytes, prepare and push
// The trivial form of a flavour's front (header comment): launch 1 is F::local over the stack's windows.
template <class F>
struct GroupPlainFront {
    template <class A, class Take>
    void regions(const A*, GroupLayout&, Take&&) const {}
    template <class A>
    int check_shape(const A*, long) const { return HICOM_OK; }
    template <class A>
    int check_push(const A*, const GroupLayout&) const { return HICOM_OK; }
    template <class A>
    int front(const A* a, const GroupLayout& l, const uint16_t* key_x, const GroupPush& push) const {
        const char* ws = (const char*)a->ws;
        const hicom_axis ay{a->H, a->ks, a->H / a->ks, a->H / a->ks}, ax{a->W, a->ks, a->W / a->ks, a->W / a->ks};
        HICOM_LAUNCH(F::local, dim3((unsigned)((l.windows + 3) / 4)), dim3(256), 0, (hipStream_t)a->stream, key_x, (const uint16_t*)a->ff,
                     (const uint16_t*)a->guide, (const typename F::Item*)(ws + l.items), (const int*)(ws + l.win_item), ay, ax, (int)a->kt, (int)l.windows,
                     a->l_scale, (_Float16*)(ws + l.ctx16), push);
        return seg_check_launch(F::kWho, "local stage");
    }
};

template <class F>
int group_check_shape(const typename F::Args* a, const F& f = F()) {
    constexpr const char* who = F::kWho;
    HICOM_REQUIRE(a, HICOM_EINVAL, "%s: NULL arguments", who);
    HICOM_REQUIRE(a->B >= 1 && a->B <= kGroupMax, HICOM_EUNSUP, "%s: B=%d slots (1 <= B <= %d per group)", who, a->B, kGroupMax);
    int st = F::check_group(a);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->items >= 1 && a->items <= a->B, HICOM_EINVAL, "%s: %d items in one push (1 .. B = %d: a slot appears at most once)", who, a->items, a->B);
    HICOM_REQUIRE(a->H > 0 && a->W > 0 && a->kt > 0 && a->ks > 0 && a->hidden > 0 && a->nh > 0 && a->chunks >= 0 && a->nl_group >= 0, HICOM_EINVAL, "%s: bad shape",
                  who);
    HICOM_REQUIRE(a->E == 1152, HICOM_EUNSUP, "%s: E=%d (only 1152)", who, a->E);
    HICOM_REQUIRE(a->nh <= 16 && a->E % a->nh == 0, HICOM_EUNSUP, "%s: %d heads (<= 16 folded rows per %s)", who, a->nh, F::kUnit);
    HICOM_REQUIRE(a->hidden % 64 == 0, HICOM_EUNSUP, "%s: hidden=%d (multiple of 64: fp16 readout planes)", who, a->hidden);
    HICOM_REQUIRE(a->out_dt == HICOM_DT_F32 || a->out_dt == HICOM_DT_BF16, HICOM_EUNSUP, "%s: output dtype %d (bf16 | f32)", who, a->out_dt);
    HICOM_REQUIRE(a->H % a->ks == 0 && a->W % a->ks == 0, HICOM_EUNSUP, "%s: needs an exact window partition (H=%d W=%d, windows %dx%dx%d)", who, a->H, a->W,
                  a->kt, a->ks, a->ks);
    HICOM_REQUIRE(a->kt * a->ks * a->ks <= 64, HICOM_EUNSUP, "%s: windows of %d tokens (<= 64)", who, a->kt * a->ks * a->ks);
    const int wps = (a->H / a->ks) * (a->W / a->ks);
    long tokens = 0;
    int max_T = 0;
    for (int i = 0; i < a->items; ++i) {
        st = F::check_item(a, i);
        if (st != HICOM_OK) return st;
        HICOM_REQUIRE(a->tc[i] > 0 && a->tc[i] % a->kt == 0, HICOM_EUNSUP, "%s: item %d needs an exact window partition (Tc=%d, temporal window %d)", who, i,
                      a->tc[i], a->kt);
        const long N = (long)a->tc[i] * a->H * a->W;
        HICOM_REQUIRE(N < (1L << 27), HICOM_EUNSUP, "%s: item %d: too many tokens", who, i);
        HICOM_REQUIRE(!a->nl_group || group_item_win(a, i, wps) % a->nl_group == 0, HICOM_EINVAL, "%s: item %d: output layout", who, i);
        tokens += N;
        if (a->tc[i] > max_T) max_T = a->tc[i];
    }
    // (item offsets are ints on the device)
    HICOM_REQUIRE(tokens + 16L * a->items < (1L << 27), HICOM_EUNSUP, "%s: too many tokens in one push", who);
    st = F::check_totals(a, wps);
    if (st != HICOM_OK) return st;
    st = f.check_shape(a, tokens);
    if (st != HICOM_OK) return st;
    return seg_check_merge_lds(who, a, max_T);
}

// The partial-state slots of an item are ordered [pass][row group][chunk]; its logits are [16 kRowGroups passes][ceil16(N)].
template <class F>
GroupLayout group_layout(const typename F::Args* a, const F& f = F()) {
    GroupLayout l{};
    const long HW = (long)a->H * a->W, E = a->E;
    l.wps = (a->H / a->ks) * (a->W / a->ks);
    for (int i = 0; i < a->items; ++i) {
        const long N = a->tc[i] * HW, w = group_item_win(a, i, l.wps), ntiles = (N + 15) / 16, Q = F::guides(a, i);
        l.windows += w;
        l.tokens += N;
        l.ctx_rows += Q * w;
        l.rows += Q * (w + group_item_nl(a, i, l.wps));
        l.score16 += group_item_passes<F>(a, i) * 16 * F::kRowGroups * ntiles;
        l.work_sum += ntiles * group_item_passes<F>(a, i);
        if (a->tc[i] > l.max_T) l.max_T = a->tc[i];
        if (Q > l.max_Q) l.max_Q = (int)Q;
    }
    const int ncu = a->chunks > 0 ? 0 : num_cus();
    for (int i = 0; i < a->items; ++i) l.nunits += seg_share_chunks((a->tc[i] * HW + 15) / 16, l.work_sum, a->chunks, ncu) * group_item_passes<F>(a, i);
    l.slots = F::kRowGroups * l.nunits;
    long off = 0;
    auto take = [&](long bytes) { const long at = off; off += (bytes + 255) / 256 * 256; return at; };
    const int odt = a->out_dt == HICOM_DT_F32 ? 4 : 2;
    l.items = take(a->items * (long)sizeof(typename F::Item));
    l.units = take(l.nunits * (long)sizeof(typename F::Unit));
    l.win_item = take(l.windows * 4);
    l.row_item = take(l.rows * 4);
    l.table_bytes = off;
    l.scores = take(l.score16 * 16 * 4);
    l.part_m = take(l.slots * 16 * 4);
    l.part_l = take(l.slots * 16 * 4);
    l.part_acc = take(l.slots * 16 * E * 4);
    l.ctx16 = take(l.ctx_rows * E * 2);
    l.hid16 = take(l.ctx_rows * (long)a->hidden * 2);
    l.loc = take(l.ctx_rows * (long)a->hidden * odt);
    f.regions(a, l, take);
    l.total = off;
    return l;
}

inline GroupPush group_push_values(const int32_t* unit0, const int32_t* t0, const int32_t* row0, int items) {
    GroupPush v{};
    for (int i = 0; i < items; ++i) {
        v.slot[i] = unit0[i];
        v.t0[i] = t0[i];
        v.row0[i] = row0 ? row0[i] : 0;
    }
    return v;
}

// slots distinct and < B: one workgroup owns a carried row, and only when no other item of the push folds into it
inline int group_check_slots(const char* who, const int32_t* slot, int items, int B) {
    uint32_t seen = 0;
    for (int i = 0; i < items; ++i) {
        HICOM_REQUIRE(slot[i] >= 0 && slot[i] < B, HICOM_EINVAL, "%s: item %d: slot %d (0 <= slot < B = %d)", who, i, slot[i], B);
        HICOM_REQUIRE(!(seen >> slot[i] & 1u), HICOM_EINVAL, "%s: item %d: slot %d appears twice in one push (its state is updated in place)", who, i, slot[i]);
        seen |= 1u << slot[i];
    }
    return HICOM_OK;
}

template <class F>
int64_t group_workspace_bytes(const typename F::Args* a, const F& f = F()) {
    const int st = group_check_shape<F>(a, f);
    if (st != HICOM_OK) return st;
    return group_layout<F>(a, f).total;
}

template <class F>
int group_prepare(const typename F::Args* a, const F& f = F()) {
    int st = group_check_shape<F>(a, f);
    if (st != HICOM_OK) return st;
    const GroupLayout l = group_layout<F>(a, f);
    st = seg_check_ws(F::kWho, a, l.total);
    if (st != HICOM_OK) return st;
    std::vector<int> tab((size_t)(l.table_bytes / 4), 0);
    typename F::Item* items = reinterpret_cast<typename F::Item*>(tab.data() + l.items / 4);
    typename F::Unit* units = reinterpret_cast<typename F::Unit*>(tab.data() + l.units / 4);
    int* win_item = tab.data() + l.win_item / 4;
    int* row_item = tab.data() + l.row_item / 4;
    const long HW = (long)a->H * a->W;
    const int ncu = a->chunks > 0 ? 0 : num_cus();
    GroupWalk w{};
    for (int i = 0; i < a->items; ++i) {
        w.i = i; w.T = a->tc[i]; w.Q = F::guides(a, i);
        w.N = w.T * HW; w.ntiles = (w.N + 15) / 16; w.passes = group_item_passes<F>(a, i);
        w.wins = group_item_win(a, i, l.wps); w.nl = group_item_nl(a, i, l.wps);
        w.chunks = seg_share_chunks(w.ntiles, l.work_sum, a->chunks, ncu);
        const long rows = w.Q * (w.wins + w.nl);
        F::write(items[i], units, w);
        for (long k = 0; k < w.wins; ++k) win_item[w.win + k] = i;
        for (long k = 0; k < rows; ++k) row_item[w.row + k] = i;
        units += w.passes * w.chunks;
        w.tok += w.N; w.win += w.wins; w.row += rows; w.score += w.passes * 16 * F::kRowGroups * w.ntiles;
        w.slot += F::kRowGroups * w.passes * w.chunks; w.ctx_row += w.Q * w.wins;
    }
    return seg_upload_tables(F::kWho, a, tab.data(), l.table_bytes);
}

// The merge + fold kernel's parameters but where the items live: p.items (the table of a push), or u_T, u_nparts and uniform_guides of
// the stand-alone entry, whose items are packed one behind the other.
template <class F>
typename F::MergeParams group_merge_params(const float* part_m, const float* part_l, const float* part_acc, const float* scores, const float* pe, int E, int H, int W,
                                           int y_index0, int x_index0, int rows, float* state_ml, float* state_acc, const GroupPush& push) {
    typename F::MergeParams p{};
    p.c.part_m = part_m; p.c.part_l = part_l; p.c.part_acc = part_acc;
    p.c.pe = pe; p.c.E = E; p.c.H = H; p.c.W = W;
    p.c.t0i = 0; p.c.y0i = y_index0; p.c.x0i = x_index0;
    p.scores = scores;
    p.rows = rows;
    p.state_ml = state_ml; p.state_acc = state_acc;
    p.push = push;
    return p;
}

// grid (rows x the most guides of an item, items); T: the longest item's frames
template <class F>
int group_merge_launch(const char* who, const typename F::MergeParams& p, int max_Q, int items, int T, hipStream_t s) {
    HICOM_LAUNCH(F::merge, dim3((unsigned)(p.rows * max_Q), (unsigned)items), dim3(256), (size_t)seg_merge_smem(T, p.c.H, p.c.W), s, p);
    return seg_check_launch(who, "merge and fold");
}

template <class F>
int group_push(const typename F::Args* a, const F& f = F()) {
    constexpr const char* who = F::kWho;
    int st = group_check_shape<F>(a, f);
    if (st != HICOM_OK) return st;
    const GroupLayout l = group_layout<F>(a, f);
    st = seg_check_ws(who, a, l.total);
    if (st != HICOM_OK) return st;
    const long unit_stride = a->*F::kStride, unit_rows = a->*F::kRows;
    HICOM_REQUIRE(a->ff && a->guide && a->q_hi && a->q_lo && a->state_ml && a->state_acc && a->out, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE(a->lw0_f16 && a->lb0 && a->lw2_f16 && a->lb2, HICOM_EINVAL, "%s: NULL weight", who);
    HICOM_REQUIRE((a->pos_a != nullptr) == (a->pe != nullptr) && (!a->pe || a->P > 0), HICOM_EINVAL, "%s: pos_a and pe come together", who);
    HICOM_REQUIRE((uintptr_t)a->ff % 16 == 0 && (uintptr_t)a->fe % 16 == 0 && (uintptr_t)a->guide % 16 == 0 && (uintptr_t)a->q_hi % 16 == 0 &&
                      (uintptr_t)a->q_lo % 16 == 0 && (uintptr_t)a->lw0_f16 % 16 == 0 && (uintptr_t)a->lw2_f16 % 16 == 0 && (uintptr_t)a->state_acc % 16 == 0 &&
                      (uintptr_t)a->state_ml % 8 == 0, HICOM_EINVAL, "%s: 16-byte aligned inputs, planes and accumulators, 8-byte aligned (M, L)", who);
    st = group_check_slots(who, a->slot, a->items, a->B);
    if (st != HICOM_OK) return st;
    st = F::check_units(a);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->ldo >= a->hidden && unit_rows > 0 && unit_stride >= unit_rows * a->ldo, HICOM_EINVAL,
                  "%s: output layout (%ld rows per %s, row length %ld, %ss %ld elements apart)", who, unit_rows, F::kUnit, (long)a->ldo, F::kUnit, unit_stride);
    HICOM_REQUIRE(a->nl_group == 0 || a->newline, HICOM_EINVAL, "%s: newline rows (one behind every %d token rows) and there is no newline token", who,
                  a->nl_group);
    for (int i = 0; i < a->items; ++i) {
        HICOM_REQUIRE(a->t0[i] >= 0 && a->t0[i] % a->kt == 0, HICOM_EINVAL, "%s: item %d: t0=%d (whole window groups of %d frames)", who, i, a->t0[i], a->kt);
        if (a->pe)
            HICOM_REQUIRE((long)a->t0[i] + a->tc[i] <= a->y_index0 && a->y_index0 + a->H <= a->x_index0 && a->x_index0 + a->W <= a->P, HICOM_EINVAL,
                          "%s: item %d: frames %d .. %d, grid %dx%d outside the positional tables (t < %d, y at %d, x at %d, %d rows)", who, i, a->t0[i],
                          a->t0[i] + a->tc[i], a->H, a->W, a->y_index0, a->y_index0, a->x_index0, a->P);
        const long rows = group_item_win(a, i, l.wps) + group_item_nl(a, i, l.wps);
        HICOM_REQUIRE(a->row0[i] >= 0 && (long)a->row0[i] + rows <= unit_rows, HICOM_EINVAL, "%s: item %d: rows %d .. %ld outside the %s's buffer of %ld rows", who,
                      i, a->row0[i], (long)a->row0[i] + rows, F::kUnit, unit_rows);
    }
    HICOM_REQUIRE(l.windows <= INT32_MAX && l.rows <= INT32_MAX && l.nunits <= INT32_MAX, HICOM_EUNSUP, "%s: too many windows in one push", who);
    st = f.check_push(a, l);
    if (st != HICOM_OK) return st;

    char* ws = (char*)a->ws;
    hipStream_t s = (hipStream_t)a->stream;
    const GroupPush push = group_push_values(F::unit0(a), a->t0, a->row0, a->items);
    const typename F::Item* items = (const typename F::Item*)(ws + l.items);
    const uint16_t* key_x = (const uint16_t*)(a->fe ? a->fe : a->ff);      // (no frames_embed: the keys are frames_feature)

    // 1: local stage (the flavour's front: F::local, or what a flavour runs in its place)
    st = f.front(a, l, key_x, push);
    if (st != HICOM_OK) return st;
    // 2: segmented global stream
    {
        constexpr int smem = hicom::seg_stream_smem(F::kRowGroups);
        typename F::StreamParams p;
        p.c.qhi = (const uint16_t*)a->q_hi; p.c.qlo = (const uint16_t*)a->q_lo;
        p.c.pos_a = a->pos_a; p.c.pos_stride = a->P; p.c.rows = a->nh;
        p.c.H = a->H; p.c.W = a->W; p.c.HW = a->H * a->W;
        p.c.t0i = 0; p.c.y0i = a->y_index0; p.c.x0i = a->x_index0;
        p.c.part_m = (float*)(ws + l.part_m); p.c.part_l = (float*)(ws + l.part_l); p.c.part_acc = (float*)(ws + l.part_acc);
        p.x = (const uint16_t*)a->ff;
        p.scores = (float*)(ws + l.scores);
        p.units = (const typename F::Unit*)(ws + l.units); p.items = items;
        p.push = push;
        // (once per process, as in the other many-item steps: one device per process; a repeated call from a second host thread is harmless)
        static bool attr_set = false;
        if (!attr_set) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(F::stream), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
            if (e != hipSuccess) {
                set_error("%s: global stream: %d bytes of LDS per workgroup: %s", who, smem, hipGetErrorString(e));
                return HICOM_ELAUNCH;
            }
            attr_set = true;
        }
        HICOM_LAUNCH(F::stream, dim3((unsigned)l.nunits), dim3(256 * F::kRowGroups), smem, s, p);
        st = seg_check_launch(who, "global stream");
        if (st != HICOM_OK) return st;
    }
    // 3: merge + fold into the states of every item
    {
        typename F::MergeParams p = group_merge_params<F>((const float*)(ws + l.part_m), (const float*)(ws + l.part_l), (const float*)(ws + l.part_acc),
                                                          (const float*)(ws + l.scores), a->pe, a->E, a->H, a->W, a->y_index0, a->x_index0, a->nh, a->state_ml,
                                                          a->state_acc, push);
        p.items = items;
        st = group_merge_launch<F>(who, p, l.max_Q, a->items, l.max_T, s);
        if (st != HICOM_OK) return st;
    }
    // 4-5: the local readout as one GEMM pair over all window contexts
    st = hicom_readout16_gemm_fwd(ws + l.ctx16, a->lw0_f16, a->lb0, HICOM_DT_BF16, (int32_t)l.ctx_rows, a->hidden, a->E, HICOM_ACT_GELU, ws + l.hid16, nullptr, 0, 0,
                                  0, 0, nullptr, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_readout16_gemm_fwd(ws + l.hid16, a->lw2_f16, a->lb2, HICOM_DT_BF16, (int32_t)l.ctx_rows, a->hidden, a->hidden, HICOM_ACT_NONE, nullptr, ws + l.loc,
                                  a->out_dt, a->hidden, 0, 0, nullptr, a->stream);
    if (st != HICOM_OK) return st;
    // 6: every item's chunk rows to its own part of the output
    typename F::PlaceParams p;
    p.c.loc = ws + l.loc; p.c.tok = nullptr; p.c.newline = (const uint16_t*)a->newline; p.c.out = a->out;
    p.c.out_f32 = a->out_dt == HICOM_DT_F32; p.c.hidden = a->hidden;
    p.items = items; p.row_item = (const int*)(ws + l.row_item); p.nl_group = a->nl_group;
    p.ldo = a->ldo; p.*F::kPlaceStride = unit_stride;
    p.push = push;
    HICOM_LAUNCH(F::place, dim3((unsigned)l.rows), dim3(128), 0, s, p);
    return seg_check_launch(who, "placement");
}

// The merge + fold kernel alone: `items` chunks of Tc frames with Q guides each, packed one behind the other as the kernel's header says;
// folded into the state rows unit0[i] rows + R, R < rows Q.  units: the slots (B) or pairs (M) of the group.
template <class F>
int group_merge_fold(const float* part_m, const float* part_l, const float* part_acc, const float* scores, int items, int nparts, int rows, int Q, int E, int Tc,
                     int H, int W, const float* pe, int P, int y_index0, int x_index0, const int32_t* unit0, const int32_t* t0, int units, float* state_ml,
                     float* state_acc, void* stream) {
    constexpr const char* who = F::kFoldWho;
    HICOM_REQUIRE(part_m && part_l && part_acc && unit0 && t0 && state_ml && state_acc, HICOM_EINVAL, "%s: NULL pointer", who);
    int st = F::check_fold_shape(who, items, units, nparts, rows, Q, E, Tc, H, W);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(!pe || scores, HICOM_EINVAL, "%s: the positional term needs the logits", who);
    HICOM_REQUIRE((uintptr_t)part_acc % 16 == 0 && (uintptr_t)state_acc % 16 == 0 && (uintptr_t)state_ml % 8 == 0, HICOM_EINVAL,
                  "%s: 16-byte aligned accumulators, 8-byte aligned (M, L)", who);
    HICOM_REQUIRE(seg_merge_smem(Tc, H, W) <= 48 * 1024, HICOM_EUNSUP, "%s: Tc=%d frames of %dx%d: the merge keeps Tc (H + W) marginal sums in LDS", who, Tc, H, W);
    st = F::check_fold_units(who, unit0, Q, items, units);
    if (st != HICOM_OK) return st;
    for (int i = 0; i < items; ++i) {
        HICOM_REQUIRE(t0[i] >= 0, HICOM_EINVAL, "%s: item %d: t0=%d", who, i, t0[i]);
        if (pe)
            HICOM_REQUIRE((long)t0[i] + Tc <= y_index0 && y_index0 + H <= x_index0 && x_index0 + W <= P, HICOM_EINVAL,
                          "%s: item %d: frames %d .. %d, grid %dx%d outside the positional tables (t < %d, y at %d, x at %d, %d rows)", who, i, t0[i], t0[i] + Tc, H,
                          W, y_index0, y_index0, x_index0, P);
    }
    typename F::MergeParams p = group_merge_params<F>(part_m, part_l, part_acc, scores, pe, E, H, W, y_index0, x_index0, rows, state_ml, state_acc,
                                                      group_push_values(unit0, t0, nullptr, items));
    p.u_T = Tc; p.u_nparts = nparts;
    F::uniform_guides(p, Q);
    return group_merge_launch<F>(who, p, Q, items, Tc, (hipStream_t)stream);
}

}  // namespace hicom_host
