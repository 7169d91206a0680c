// Clip stream group: B live videos, each with its own guide and its own carried softmax state, pushed in ONE host
// call from the vision tower's stacked [sum Tc_i, H, W, E] tensor.  One push is six launches whatever B and the mix of chunk lengths
// are: the local stage over the concatenated window list (local_window_ctx16), the segmented global stream (stream_segment<9, 1>), the
// merge of every item's partials into its chunk's UN-normalised set folded into the slot's carried state (the one kernel that is new
// here), the readout GEMM pair over all windows and the placement (place_row) into each slot's own part of the output storage.
//
// What is static per tuple of chunk lengths lives in a table region at the head of the plan's workspace, as in ragged.hip
// (hicom_compressor_stream_group_prepare uploads it once): first token, token count, first window, work units, window -> item,
// row -> item.  What changes from push to push -- per item its slot, its absolute frame offset t0 and its first output row -- travels by
// value in the kernel arguments (GroupPush: three arrays of 32 ints), so a push copies nothing to the device and never synchronises.
//
// The carried state of slot s is state_ml [s][nh][2], state_acc [s][nh][E]: each slot's slice is one set as hicom_global_combine_fwd
// reads it.  The merge + fold kernel updates (M, L) and ACC in place: ONE workgroup owns the whole (item, head) row, reads (M, L),
// passes a barrier and lane 0 writes the new pair, so a slot may appear only once per push (the host entry refuses otherwise).
#include <math.h>

#include <vector>

#include "merge_fold.hpp"
#include "segment_host.hpp"

namespace hicom {

constexpr int kGroupMax = 32;            // slots per group and items per push

// what changes from push to push, per item of the call: by value in the kernel arguments
struct GroupPush {
    int slot[kGroupMax];
    int t0[kGroupMax];
    int row0[kGroupMax];
};

struct GroupItem {       // 12 ints, static per plan
    int tok0, N;         // first token in the stack, tokens
    int T;               // frames of the chunk
    int win0;            // first window in the concatenated window list
    int slot0, chunks;   // partial-state slots = work units of this item
    int score_off;       // its logits: scores + 16 * score_off, [16][ceil16(N)]
    int lrow0;           // first row in the concatenated list of the call's chunk rows
    int rows;            // chunk rows: windows + chunk-local newline rows
    int nl_count;
    int pad0, pad1;
};
static_assert(sizeof(GroupItem) == 48, "item table entries are 12 ints");

// ---- 1: local stage, one wave per window of the concatenated window list; the guide row of the item's SLOT ----
template <int NV>
__global__ __launch_bounds__(256) void group_local_attn_kernel(const uint16_t* key, const uint16_t* value, const uint16_t* guide,
                                                               const GroupItem* items, const int* win_item, hicom_axis ay, hicom_axis ax, int kt,
                                                               int nwin, float scale, _Float16* ctx16, GroupPush push) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const int item = win_item[win];
    const GroupItem it = items[item];
    const int slot = push.slot[item];
    const hicom_axis at{it.T, kt, it.T / kt, it.T / kt};
    const WindowGeom g(at, ay, ax, win - it.win0);
    const long first = (long)it.tok0 * D;
    local_window_ctx16<NV>(key + first, value + first, guide + (long)slot * D, g, lane, scale, ctx16 + (long)win * D);
}

// ---- 2: segmented global stream, one workgroup per work unit: the item's frames count from its absolute offset, its queries are its slot's ----
struct GroupStreamParams {
    SegStreamParams c;
    const uint16_t* x;      // [sum N_i][E]
    float* scores;
    const int4* units;      // {item, first tile, last tile (exclusive), partial-state slot}
    const GroupItem* items;
    GroupPush push;
};

template <int NB>
__global__ __launch_bounds__(256, 2) void group_global_stream_kernel(GroupStreamParams p) {
    constexpr int E = NB * 128;
    const int4 u = p.units[blockIdx.x];
    const int N = p.items[u.x].N, tok0 = p.items[u.x].tok0, soff = p.items[u.x].score_off;
    SegStreamParams c = p.c;
    c.t0i += p.push.t0[u.x];
    stream_segment<NB, 1>(c, p.x + (long)tok0 * E, N, u.y, u.z, 0, c.rows, (long)p.push.slot[u.x] * c.rows, p.scores + (long)soff * 16,
                          (long)((N + 15) / 16 * 16), (long)u.w, 0);
}

// ---- 3: merge + fold, grid (rows, items), 256 threads: one workgroup owns one (item, head) row ----
// merge_fold_row (merge_fold.hpp) has the arithmetic: the chunk's un-normalised set relative to its maximum, folded into the carried row.
struct GroupMergeParams {
    SegMergeParams c;
    const float* scores;
    const GroupItem* items; // NULL: every item has u_T frames and u_nparts partials, packed one behind the other (the stand-alone entry)
    int u_T, u_nparts;
    int rows;
    float* state_ml;        // [B][rows][2]
    float* state_acc;       // [B][rows][E]
    GroupPush push;
};

__global__ __launch_bounds__(256) void group_merge_fold_kernel(GroupMergeParams p) {
    extern __shared__ float ms[];
    const int r = blockIdx.x, item = blockIdx.y;
    int T, N, nparts, slot0;
    long soff;
    if (p.items) {
        const GroupItem it = p.items[item];
        T = it.T; N = it.N; nparts = it.chunks; slot0 = it.slot0; soff = it.score_off;
    } else {
        T = p.u_T; N = T * p.c.H * p.c.W; nparts = p.u_nparts; slot0 = item * nparts; soff = (long)item * ((N + 15) / 16 * 16);
    }
    const long stride = (N + 15) / 16 * 16;
    const long row = (long)p.push.slot[item] * p.rows + r;
    merge_fold_row(p.c, ms, r, threadIdx.x, T, p.push.t0[item], nparts, (long)slot0, p.scores + soff * 16 + r * stride, p.state_ml + 2 * row,
                   p.state_acc + row * p.c.E);
}

// ---- 6: placement, one output row per workgroup over all items' chunk rows, into the slot's own buffer ----
struct GroupPlaceParams {
    SegPlaceParams c;
    const GroupItem* items;
    const int* row_item;
    int nl_group;
    long ldo, slot_stride;
    GroupPush push;
};

__global__ __launch_bounds__(128) void group_place_kernel(GroupPlaceParams p) {
    const long row = blockIdx.x;
    const int item = p.row_item[row];
    const GroupItem it = p.items[item];
    const long r = row - it.lrow0;
    place_row(p.c, r, (long)p.push.slot[item] * p.slot_stride + ((long)p.push.row0[item] + r) * p.ldo, item, it.win0, p.nl_group, it.nl_count, it.rows,
              p.nl_group, p.nl_group + 1);
}

}  // namespace hicom

using namespace hicom;
using namespace hicom_host;

namespace {

constexpr const char* kWho = "compressor_stream_group";

struct GroupLayout {
    long items, units, win_item, row_item, table_bytes;     // the table region
    long scores, part_m, part_l, part_acc, ctx16, hid16, loc, total;
    long windows, rows, slots, ntiles_sum;
    int max_T, wps;
};

long item_win(const hicom_stream_group_push_args* a, int i, int wps) { return (long)(a->tc[i] / a->kt) * wps; }
long item_nl(const hicom_stream_group_push_args* a, int i, int wps) { return a->nl_group > 0 ? item_win(a, i, wps) / a->nl_group : 0; }

// everything that the tuple of chunk lengths and the geometry decide: the checks of workspace_bytes, prepare and push
int group_check_shape(const hicom_stream_group_push_args* a) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "%s: NULL arguments", kWho);
    HICOM_REQUIRE(a->B >= 1 && a->B <= kGroupMax, HICOM_EUNSUP, "%s: B=%d slots (1 <= B <= %d per group)", kWho, a->B, kGroupMax);
    HICOM_REQUIRE(a->items >= 1 && a->items <= a->B, HICOM_EINVAL, "%s: %d items in one push (1 .. B = %d: a slot appears at most once)", kWho, a->items, a->B);
    HICOM_REQUIRE(a->H > 0 && a->W > 0 && a->kt > 0 && a->ks > 0 && a->hidden > 0 && a->nh > 0 && a->chunks >= 0 && a->nl_group >= 0, HICOM_EINVAL, "%s: bad shape",
                  kWho);
    HICOM_REQUIRE(a->E == 1152, HICOM_EUNSUP, "%s: E=%d (only 1152)", kWho, a->E);
    HICOM_REQUIRE(a->nh <= 16 && a->E % a->nh == 0, HICOM_EUNSUP, "%s: %d heads (<= 16 folded rows per slot)", kWho, a->nh);
    HICOM_REQUIRE(a->hidden % 64 == 0, HICOM_EUNSUP, "%s: hidden=%d (multiple of 64: fp16 readout planes)", kWho, a->hidden);
    HICOM_REQUIRE(a->out_dt == HICOM_DT_F32 || a->out_dt == HICOM_DT_BF16, HICOM_EUNSUP, "%s: output dtype %d (bf16 | f32)", kWho, a->out_dt);
    HICOM_REQUIRE(a->H % a->ks == 0 && a->W % a->ks == 0, HICOM_EUNSUP, "%s: needs an exact window partition (H=%d W=%d, windows %dx%dx%d)", kWho, a->H, a->W,
                  a->kt, a->ks, a->ks);
    HICOM_REQUIRE(a->kt * a->ks * a->ks <= 64, HICOM_EUNSUP, "%s: windows of %d tokens (<= 64)", kWho, a->kt * a->ks * a->ks);
    const int wps = (a->H / a->ks) * (a->W / a->ks);
    long tokens = 0;
    int max_T = 0;
    for (int i = 0; i < a->items; ++i) {
        HICOM_REQUIRE(a->tc[i] > 0 && a->tc[i] % a->kt == 0, HICOM_EUNSUP, "%s: item %d needs an exact window partition (Tc=%d, temporal window %d)", kWho, i,
                      a->tc[i], a->kt);
        const long N = (long)a->tc[i] * a->H * a->W;
        HICOM_REQUIRE(N < (1L << 27), HICOM_EUNSUP, "%s: item %d: too many tokens", kWho, i);
        HICOM_REQUIRE(!a->nl_group || item_win(a, i, wps) % a->nl_group == 0, HICOM_EINVAL, "%s: item %d: output layout", kWho, i);
        tokens += N;
        if (a->tc[i] > max_T) max_T = a->tc[i];
    }
    HICOM_REQUIRE(tokens + 16L * a->items < (1L << 27), HICOM_EUNSUP, "%s: too many tokens in one push", kWho);
    return seg_check_merge_lds(kWho, a, max_T);
}

GroupLayout group_layout(const hicom_stream_group_push_args* a) {
    GroupLayout l{};
    const long HW = (long)a->H * a->W, E = a->E;
    l.wps = (a->H / a->ks) * (a->W / a->ks);
    long score_floats = 0;
    for (int i = 0; i < a->items; ++i) {
        const long N = a->tc[i] * HW, w = item_win(a, i, l.wps);
        l.windows += w;
        l.rows += w + item_nl(a, i, l.wps);
        score_floats += 16 * ((N + 15) / 16 * 16);
        l.ntiles_sum += (N + 15) / 16;
        if (a->tc[i] > l.max_T) l.max_T = a->tc[i];
    }
    const int ncu = a->chunks > 0 ? 0 : num_cus();
    for (int i = 0; i < a->items; ++i) l.slots += seg_share_chunks((a->tc[i] * HW + 15) / 16, l.ntiles_sum, a->chunks, ncu);
    long off = 0;
    auto take = [&](long bytes) { const long at = off; off += (bytes + 255) / 256 * 256; return at; };
    const int odt = a->out_dt == HICOM_DT_F32 ? 4 : 2;
    l.items = take(a->items * (long)sizeof(GroupItem));
    l.units = take(l.slots * 16);
    l.win_item = take(l.windows * 4);
    l.row_item = take(l.rows * 4);
    l.table_bytes = off;
    l.scores = take(score_floats * 4);
    l.part_m = take(l.slots * 16 * 4);
    l.part_l = take(l.slots * 16 * 4);
    l.part_acc = take(l.slots * 16 * E * 4);
    l.ctx16 = take(l.windows * E * 2);
    l.hid16 = take(l.windows * (long)a->hidden * 2);
    l.loc = take(l.windows * (long)a->hidden * odt);
    l.total = off;
    return l;
}

GroupPush group_push_values(const int32_t* slot, const int32_t* t0, const int32_t* row0, int items) {
    GroupPush v{};
    for (int i = 0; i < items; ++i) {
        v.slot[i] = slot[i];
        v.t0[i] = t0[i];
        v.row0[i] = row0 ? row0[i] : 0;
    }
    return v;
}

// slots distinct and < B: one workgroup owns a carried row, and only when no other item of the push folds into it
int group_check_slots(const char* who, const int32_t* slot, int items, int B) {
    uint32_t seen = 0;
    for (int i = 0; i < items; ++i) {
        HICOM_REQUIRE(slot[i] >= 0 && slot[i] < B, HICOM_EINVAL, "%s: item %d: slot %d (0 <= slot < B = %d)", who, i, slot[i], B);
        HICOM_REQUIRE(!(seen >> slot[i] & 1u), HICOM_EINVAL, "%s: item %d: slot %d appears twice in one push (its state is updated in place)", who, i, slot[i]);
        seen |= 1u << slot[i];
    }
    return HICOM_OK;
}

}  // namespace

extern "C" int64_t hicom_compressor_stream_group_workspace_bytes(const hicom_stream_group_push_args* a) {
    const int st = group_check_shape(a);
    if (st != HICOM_OK) return st;
    return group_layout(a).total;
}

extern "C" int hicom_compressor_stream_group_prepare(const hicom_stream_group_push_args* a) {
    int st = group_check_shape(a);
    if (st != HICOM_OK) return st;
    const GroupLayout l = group_layout(a);
    st = seg_check_ws(kWho, a, l.total);
    if (st != HICOM_OK) return st;
    std::vector<int> tab((size_t)(l.table_bytes / 4), 0);
    GroupItem* items = reinterpret_cast<GroupItem*>(tab.data() + l.items / 4);
    int* units = tab.data() + l.units / 4;
    int* win_item = tab.data() + l.win_item / 4;
    int* row_item = tab.data() + l.row_item / 4;
    const long HW = (long)a->H * a->W;
    const int ncu = a->chunks > 0 ? 0 : num_cus();
    long tok = 0, win = 0, row = 0, score = 0, slot = 0;
    for (int i = 0; i < a->items; ++i) {
        const long N = a->tc[i] * HW, w = item_win(a, i, l.wps), nl = item_nl(a, i, l.wps), ntiles = (N + 15) / 16;
        const int chunks = seg_share_chunks(ntiles, l.ntiles_sum, a->chunks, ncu);
        GroupItem& d = items[i];
        d.tok0 = (int)tok; d.N = (int)N; d.T = a->tc[i]; d.win0 = (int)win; d.slot0 = (int)slot; d.chunks = chunks;
        d.score_off = (int)score; d.lrow0 = (int)row; d.rows = (int)(w + nl); d.nl_count = (int)nl;
        for (int c = 0; c < chunks; ++c) {
            int* u = units + 4 * (slot + c);
            u[0] = i; u[1] = seg_tile_at(ntiles, c, chunks); u[2] = seg_tile_at(ntiles, c + 1, chunks); u[3] = (int)(slot + c);
        }
        for (long k = 0; k < w; ++k) win_item[win + k] = i;
        for (long k = 0; k < w + nl; ++k) row_item[row + k] = i;
        tok += N; win += w; row += w + nl; score += ntiles * 16; slot += chunks;
    }
    return seg_upload_tables(kWho, a, tab.data(), l.table_bytes);
}

extern "C" int hicom_compressor_stream_group_push(const hicom_stream_group_push_args* a) {
    int st = group_check_shape(a);
    if (st != HICOM_OK) return st;
    const GroupLayout l = group_layout(a);
    st = seg_check_ws(kWho, a, l.total);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->ff && a->guide && a->q_hi && a->q_lo && a->state_ml && a->state_acc && a->out, HICOM_EINVAL, "%s: NULL pointer", kWho);
    HICOM_REQUIRE(a->lw0_f16 && a->lb0 && a->lw2_f16 && a->lb2, HICOM_EINVAL, "%s: NULL weight", kWho);
    HICOM_REQUIRE((a->pos_a != nullptr) == (a->pe != nullptr) && (!a->pe || a->P > 0), HICOM_EINVAL, "%s: pos_a and pe come together", kWho);
    HICOM_REQUIRE((uintptr_t)a->ff % 16 == 0 && (uintptr_t)a->fe % 16 == 0 && (uintptr_t)a->guide % 16 == 0 && (uintptr_t)a->q_hi % 16 == 0 &&
                      (uintptr_t)a->q_lo % 16 == 0 && (uintptr_t)a->lw0_f16 % 16 == 0 && (uintptr_t)a->lw2_f16 % 16 == 0 && (uintptr_t)a->state_acc % 16 == 0 &&
                      (uintptr_t)a->state_ml % 8 == 0, HICOM_EINVAL, "%s: 16-byte aligned inputs, planes and accumulators, 8-byte aligned (M, L)", kWho);
    st = group_check_slots(kWho, a->slot, a->items, a->B);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->ldo >= a->hidden && a->slot_rows > 0 && a->slot_stride >= a->slot_rows * a->ldo, HICOM_EINVAL,
                  "%s: output layout (%ld rows per slot, row length %ld, slots %ld elements apart)", kWho, (long)a->slot_rows, (long)a->ldo, (long)a->slot_stride);
    HICOM_REQUIRE(a->nl_group == 0 || a->newline, HICOM_EINVAL, "%s: newline rows (one behind every %d token rows) and there is no newline token", kWho,
                  a->nl_group);
    for (int i = 0; i < a->items; ++i) {
        HICOM_REQUIRE(a->t0[i] >= 0 && a->t0[i] % a->kt == 0, HICOM_EINVAL, "%s: item %d: t0=%d (whole window groups of %d frames)", kWho, i, a->t0[i], a->kt);
        if (a->pe)
            HICOM_REQUIRE((long)a->t0[i] + a->tc[i] <= a->y_index0 && a->y_index0 + a->H <= a->x_index0 && a->x_index0 + a->W <= a->P, HICOM_EINVAL,
                          "%s: item %d: frames %d .. %d, grid %dx%d outside the positional tables (t < %d, y at %d, x at %d, %d rows)", kWho, i, a->t0[i],
                          a->t0[i] + a->tc[i], a->H, a->W, a->y_index0, a->y_index0, a->x_index0, a->P);
        const long rows = item_win(a, i, l.wps) + item_nl(a, i, l.wps);
        HICOM_REQUIRE(a->row0[i] >= 0 && (long)a->row0[i] + rows <= a->slot_rows, HICOM_EINVAL, "%s: item %d: rows %d .. %ld outside the slot's buffer of %ld rows",
                      kWho, i, a->row0[i], (long)a->row0[i] + rows, (long)a->slot_rows);
    }
    HICOM_REQUIRE(l.windows <= INT32_MAX && l.rows <= INT32_MAX, HICOM_EUNSUP, "%s: too many windows in one push", kWho);

    char* ws = (char*)a->ws;
    hipStream_t s = (hipStream_t)a->stream;
    const GroupPush push = group_push_values(a->slot, a->t0, a->row0, a->items);
    const GroupItem* items = (const GroupItem*)(ws + l.items);
    const uint16_t* key_x = (const uint16_t*)(a->fe ? a->fe : a->ff);      // (no frames_embed: the keys are frames_feature)

    // 1: local stage
    {
        const hicom_axis ay{a->H, a->ks, a->H / a->ks, a->H / a->ks}, ax{a->W, a->ks, a->W / a->ks, a->W / a->ks};
        HICOM_LAUNCH(group_local_attn_kernel<3>, dim3((unsigned)((l.windows + 3) / 4)), dim3(256), 0, s, key_x, (const uint16_t*)a->ff, (const uint16_t*)a->guide,
                     items, (const int*)(ws + l.win_item), ay, ax, (int)a->kt, (int)l.windows, a->l_scale, (_Float16*)(ws + l.ctx16), push);
        st = seg_check_launch(kWho, "local stage");
        if (st != HICOM_OK) return st;
    }
    // 2: segmented global stream
    {
        GroupStreamParams p;
        p.c.qhi = (const uint16_t*)a->q_hi; p.c.qlo = (const uint16_t*)a->q_lo;
        p.c.pos_a = a->pos_a; p.c.pos_stride = a->P; p.c.rows = a->nh;
        p.c.H = a->H; p.c.W = a->W; p.c.HW = a->H * a->W;
        p.c.t0i = 0; p.c.y0i = a->y_index0; p.c.x0i = a->x_index0;
        p.c.part_m = (float*)(ws + l.part_m); p.c.part_l = (float*)(ws + l.part_l); p.c.part_acc = (float*)(ws + l.part_acc);
        p.x = (const uint16_t*)a->ff;
        p.scores = (float*)(ws + l.scores);
        p.units = (const int4*)(ws + l.units); p.items = items;
        p.push = push;
        static bool attr_set = false;
        if (!attr_set) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(group_global_stream_kernel<9>), hipFuncAttributeMaxDynamicSharedMemorySize, seg_stream_smem(1));
            attr_set = true;
        }
        HICOM_LAUNCH(group_global_stream_kernel<9>, dim3((unsigned)l.slots), dim3(256), seg_stream_smem(1), s, p);
        st = seg_check_launch(kWho, "global stream");
        if (st != HICOM_OK) return st;
    }
    // 3: merge + fold into every item's slot
    {
        GroupMergeParams p;
        p.c.part_m = (const float*)(ws + l.part_m); p.c.part_l = (const float*)(ws + l.part_l); p.c.part_acc = (const float*)(ws + l.part_acc);
        p.c.pe = a->pe; p.c.E = a->E; p.c.H = a->H; p.c.W = a->W;
        p.c.t0i = 0; p.c.y0i = a->y_index0; p.c.x0i = a->x_index0;
        p.scores = (const float*)(ws + l.scores);
        p.items = items; p.u_T = 0; p.u_nparts = 0; p.rows = a->nh;
        p.state_ml = a->state_ml; p.state_acc = a->state_acc;
        p.push = push;
        HICOM_LAUNCH(group_merge_fold_kernel, dim3((unsigned)a->nh, (unsigned)a->items), dim3(256), (size_t)seg_merge_smem(l.max_T, a->H, a->W), s, p);
        st = seg_check_launch(kWho, "merge and fold");
        if (st != HICOM_OK) return st;
    }
    // 4-5: the local readout as one GEMM pair over all items' windows
    st = hicom_readout16_gemm_fwd(ws + l.ctx16, a->lw0_f16, a->lb0, HICOM_DT_BF16, (int32_t)l.windows, a->hidden, a->E, HICOM_ACT_GELU, ws + l.hid16, nullptr, 0, 0,
                                  0, 0, nullptr, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_readout16_gemm_fwd(ws + l.hid16, a->lw2_f16, a->lb2, HICOM_DT_BF16, (int32_t)l.windows, a->hidden, a->hidden, HICOM_ACT_NONE, nullptr, ws + l.loc,
                                  a->out_dt, a->hidden, 0, 0, nullptr, a->stream);
    if (st != HICOM_OK) return st;
    // 6: every item's chunk rows to its slot's buffer
    GroupPlaceParams p;
    p.c.loc = ws + l.loc; p.c.tok = nullptr; p.c.newline = (const uint16_t*)a->newline; p.c.out = a->out;
    p.c.out_f32 = a->out_dt == HICOM_DT_F32; p.c.hidden = a->hidden;
    p.items = items; p.row_item = (const int*)(ws + l.row_item); p.nl_group = a->nl_group;
    p.ldo = a->ldo; p.slot_stride = a->slot_stride;
    p.push = push;
    HICOM_LAUNCH(group_place_kernel, dim3((unsigned)l.rows), dim3(128), 0, s, p);
    return seg_check_launch(kWho, "placement");
}

// The merge + fold kernel alone: `items` chunks of Tc frames each, item i's nparts partials in the slots [i nparts, (i + 1) nparts) of part_*
// ([slots][16] and [slots][16][E]), its logits at scores + i 16 ceil16(Tc H W), folded into state rows slot[i] rows + r.
extern "C" int hicom_stream_group_merge_fold_fwd(const float* part_m, const float* part_l, const float* part_acc, const float* scores, int32_t items,
                                                 int32_t nparts, int32_t rows, int32_t E, int32_t Tc, int32_t H, int32_t W, const float* pe, int32_t P,
                                                 int32_t y_index0, int32_t x_index0, const int32_t* slot, const int32_t* t0, int32_t B, float* state_ml,
                                                 float* state_acc, void* stream) {
    constexpr const char* who = "stream_group_merge_fold";
    HICOM_REQUIRE(part_m && part_l && part_acc && slot && t0 && state_ml && state_acc, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE(B >= 1 && B <= kGroupMax, HICOM_EUNSUP, "%s: B=%d slots (1 <= B <= %d per group)", who, B, kGroupMax);
    HICOM_REQUIRE(items >= 1 && items <= B && nparts >= 1 && nparts <= kSegMaxChunks && rows >= 1 && rows <= 16 && E > 0 && E % 4 == 0 && Tc > 0 && H > 0 && W > 0 &&
                      (long)Tc * H * W < (1L << 27) / kGroupMax, HICOM_EINVAL, "%s: bad shape (items=%d nparts=%d rows=%d E=%d Tc=%d H=%d W=%d)", who, items, nparts,
                  rows, E, Tc, H, W);
    HICOM_REQUIRE(!pe || scores, HICOM_EINVAL, "%s: the positional term needs the logits", who);
    HICOM_REQUIRE((uintptr_t)part_acc % 16 == 0 && (uintptr_t)state_acc % 16 == 0 && (uintptr_t)state_ml % 8 == 0, HICOM_EINVAL,
                  "%s: 16-byte aligned accumulators, 8-byte aligned (M, L)", who);
    HICOM_REQUIRE(seg_merge_smem(Tc, H, W) <= 48 * 1024, HICOM_EUNSUP, "%s: Tc=%d frames of %dx%d: the merge keeps Tc (H + W) marginal sums in LDS", who, Tc, H, W);
    int st = group_check_slots(who, slot, items, B);
    if (st != HICOM_OK) return st;
    for (int i = 0; i < items; ++i) {
        HICOM_REQUIRE(t0[i] >= 0, HICOM_EINVAL, "%s: item %d: t0=%d", who, i, t0[i]);
        if (pe)
            HICOM_REQUIRE((long)t0[i] + Tc <= y_index0 && y_index0 + H <= x_index0 && x_index0 + W <= P, HICOM_EINVAL,
                          "%s: item %d: frames %d .. %d, grid %dx%d outside the positional tables (t < %d, y at %d, x at %d, %d rows)", who, i, t0[i], t0[i] + Tc, H,
                          W, y_index0, y_index0, x_index0, P);
    }
    GroupMergeParams p;
    p.c.part_m = part_m; p.c.part_l = part_l; p.c.part_acc = part_acc;
    p.c.pe = pe; p.c.E = E; p.c.H = H; p.c.W = W;
    p.c.t0i = 0; p.c.y0i = y_index0; p.c.x0i = x_index0;
    p.scores = scores;
    p.items = nullptr; p.u_T = Tc; p.u_nparts = nparts; p.rows = rows;
    p.state_ml = state_ml; p.state_acc = state_acc;
    p.push = group_push_values(slot, t0, nullptr, items);
    HICOM_LAUNCH(group_merge_fold_kernel, dim3((unsigned)rows, (unsigned)items), dim3(256), (size_t)seg_merge_smem(Tc, H, W), (hipStream_t)stream, p);
    return seg_check_launch(who, "merge and fold");
}
