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
//
// This file has the four kernels, their table entry and the description of the flavour (Single); the host side of the entry points is
// stream_group_host.hpp, shared with clip_stream_group_multi.hip.
#include <math.h>

#include "merge_fold.hpp"
#include "stream_group_host.hpp"

namespace hicom {

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

// one guide per slot: an item is one folded-row group of its slot, one pass, one work unit per token chunk
struct Single : GroupPlainFront<Single> {
    typedef hicom_stream_group_push_args Args;
    typedef GroupItem Item;
    typedef int4 Unit;
    typedef GroupStreamParams StreamParams;
    typedef GroupMergeParams MergeParams;
    typedef GroupPlaceParams PlaceParams;
    static constexpr const char *kWho = "compressor_stream_group", *kFoldWho = "stream_group_merge_fold", *kUnit = "slot";
    static constexpr int kRowGroups = 1;
    static constexpr auto kStride = &Args::slot_stride, kRows = &Args::slot_rows;
    static constexpr auto kPlaceStride = &PlaceParams::slot_stride;
    static constexpr auto local = group_local_attn_kernel<3>;
    static constexpr auto stream = group_global_stream_kernel<9>;
    static constexpr auto merge = group_merge_fold_kernel;
    static constexpr auto place = group_place_kernel;

    static int guides(const Args*, int) { return 1; }
    static const int32_t* unit0(const Args* a) { return a->slot; }
    static int check_group(const Args*) { return HICOM_OK; }
    static int check_item(const Args*, int) { return HICOM_OK; }
    static int check_totals(const Args*, int) { return HICOM_OK; }
    static int check_units(const Args*) { return HICOM_OK; }

    static void write(GroupItem& d, int4* units, const GroupWalk& w) {
        d.tok0 = (int)w.tok; d.N = (int)w.N; d.T = w.T; d.win0 = (int)w.win; d.slot0 = (int)w.slot; d.chunks = w.chunks;
        d.score_off = (int)w.score; d.lrow0 = (int)w.row; d.rows = (int)(w.wins + w.nl); d.nl_count = (int)w.nl;
        for (int c = 0; c < w.chunks; ++c)
            units[c] = make_int4(w.i, seg_tile_at(w.ntiles, c, w.chunks), seg_tile_at(w.ntiles, c + 1, w.chunks), (int)(w.slot + c));
    }

    static void uniform_guides(GroupMergeParams&, int) {}
    static int check_fold_shape(const char* who, int items, int B, int nparts, int rows, int, int E, int Tc, int H, int W) {
        HICOM_REQUIRE(B >= 1 && B <= kGroupMax, HICOM_EUNSUP, "%s: B=%d slots (1 <= B <= %d per group)", who, B, kGroupMax);
        HICOM_REQUIRE(items >= 1 && items <= B && nparts >= 1 && nparts <= kSegMaxChunks && rows >= 1 && rows <= 16 && E > 0 && E % 4 == 0 && Tc > 0 && H > 0 && W > 0 &&
                          (long)Tc * H * W < (1L << 27) / kGroupMax, HICOM_EINVAL, "%s: bad shape (items=%d nparts=%d rows=%d E=%d Tc=%d H=%d W=%d)", who, items, nparts,
                      rows, E, Tc, H, W);
        return HICOM_OK;
    }
    static int check_fold_units(const char* who, const int32_t* slot, int, int items, int B) { return group_check_slots(who, slot, items, B); }
};

}  // namespace

extern "C" int64_t hicom_compressor_stream_group_workspace_bytes(const hicom_stream_group_push_args* a) { return group_workspace_bytes<Single>(a); }
extern "C" int hicom_compressor_stream_group_prepare(const hicom_stream_group_push_args* a) { return group_prepare<Single>(a); }
extern "C" int hicom_compressor_stream_group_push(const hicom_stream_group_push_args* a) { return group_push<Single>(a); }

// The merge + fold kernel alone: `items` chunks of Tc frames each, item i's nparts partials in the slots [i nparts, (i + 1) nparts) of part_*
// ([slots][16] and [slots][16][E]), its logits at scores + i 16 ceil16(Tc H W), folded into state rows slot[i] rows + r.
extern "C" int hicom_stream_group_merge_fold_fwd(const float* part_m, const float* part_l, const float* part_acc, const float* scores, int32_t items,
                                                 int32_t nparts, int32_t rows, int32_t E, int32_t Tc, int32_t H, int32_t W, const float* pe, int32_t P,
                                                 int32_t y_index0, int32_t x_index0, const int32_t* slot, const int32_t* t0, int32_t B, float* state_ml,
                                                 float* state_acc, void* stream) {
    return group_merge_fold<Single>(part_m, part_l, part_acc, scores, items, nparts, rows, 1, E, Tc, H, W, pe, P, y_index0, x_index0, slot, t0, B, state_ml, state_acc,
                                    stream);
}
