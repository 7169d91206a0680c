// Clip stream group with several guides per slot: B live videos, slot s with its own Q_s guides and one carried softmax
// state per (slot, guide) PAIR, pushed in ONE host call from the vision tower's stacked [sum Tc_i, H, W, E] tensor.  Pairs are numbered
// slot-major, then guide-major: slot s owns the pairs [pair0_s, pair0_s + Q_s), pair0_s = sum_{j<s} Q_j, M = sum Q_s of them
// (forward_ragged_multi_guide's convention).  One push is six launches whatever B, the Q_s and the mix of chunk lengths are:
//    1  gm_local_kernel: one wave per window of the STACKED tensor, the wave walks the guides of the item's SLOT in groups of kGuideGroup
//       (multi_window.hpp: multi_window_guides_ctx16), fp16 contexts pair-major within the call as in rmg_local_kernel
//    2  gm_stream_kernel: stream_segment<9, 2> (segment_item.hpp), 32 densely packed folded rows of ONE item per workgroup, the frame rows of
//       the score-side table at the item's absolute offset, the query rows from pair0_slot nh
//    3  gm_merge_fold_kernel: merge_fold_row (merge_fold.hpp) per (item, folded row R < nh Q_item), IN PLACE into state row pair0_slot nh + R
//  4-5  the readout GEMM pair over all pairs' window contexts
//    6  gm_place_kernel: place_row to out[pair0_slot + q], row row0_item + r
//
// Row space of an item, passes, row groups and the order of the partial-state slots ([item][pass][row group][chunk]) are those of
// ragged_multi_guide.hip.  What the tuple of (Tc_i, Q_i) decides lives in a table region at the head of the plan's workspace
// (hicom_compressor_stream_group_multi_prepare uploads it once).  What changes from push to push -- per item its slot's first pair, its
// absolute frame offset and its first output row -- travels by value in the kernel arguments (GmPush: arrays of 32 ints read with a
// wave-uniform index), so a push copies nothing to the device and never synchronises.
//
// finish_many (hicom_amd/clip_stream_group_multi.py) is hicom_global_combine_fwd over the whole state, the four hicom_linear_fwd of
// GlobalCompressor.finish_guides with M rows and gm_place_global_kernel: for every pair of a NAMED slot the whole-clip newline rows and
// the 32 copies of its global row behind the slot's local rows; rows of other pairs are never read or written.
#include <vector>

#include "merge_fold.hpp"
#include "multi_window.hpp"
#include "segment_host.hpp"

namespace hicom {

constexpr int kGmMax = 32;               // slots per group, items per push and guides per slot

// what changes from push to push, per item of the call: by value in the kernel arguments
struct GmPush {
    int pair0[kGmMax];       // first pair of the item's slot
    int t0[kGmMax];
    int row0[kGmMax];
};

struct GmItem {          // 16 ints, static per plan
    int tok0, N;         // first token in the stack, tokens
    int T;               // frames of the chunk
    int win0, wins;      // first window in the stacked tensor's window list, windows = context rows of one pair
    int slot0, chunks;   // first partial-state slot; token chunks per pass (slots: passes x 2 x chunks)
    int score_off;       // its logits: scores + 16 * score_off, [32 passes][ceil16(N)]
    int Q;               // guides of the item's slot
    int ctx_row0;        // first context row of its first pair (pair q: + q wins)
    int lrow0;           // first row in the concatenated list of the call's chunk rows (pair q: + q rows)
    int rows;            // chunk rows of one pair: windows + chunk-local newline rows
    int nl_count;
    int pad0, pad1, pad2;
};
static_assert(sizeof(GmItem) == 64, "item table entries are 16 ints");

struct GmUnit {          // 8 ints
    int item, tb, te;    // tiles [tb, te) of the item, counted from its first token
    int pass;            // rows [32 pass, 32 pass + 32) of the item's row space
    int slot;            // partial-state slot of row group 0; row group 1: + the item's chunks
    int pad0, pad1, pad2;
};
static_assert(sizeof(GmUnit) == 32, "work units are 8 ints");

// ---- 1: local stage, one wave per window of the stacked tensor, the guides of the item's slot in groups of kGuideGroup ----
template <int NV>
__global__ __launch_bounds__(256) void gm_local_kernel(const uint16_t* key, const uint16_t* value, const uint16_t* guide, const GmItem* items,
                                                       const int* win_item, hicom_axis ay, hicom_axis ax, int kt, int nwin, float scale, _Float16* ctx16,
                                                       GmPush push) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const int item = win_item[win];
    const GmItem it = items[item];
    const hicom_axis at{it.T, kt, it.T / kt, it.T / kt};
    const WindowGeom g(at, ay, ax, win - it.win0);
    const long first = (long)it.tok0 * D;
    multi_window_guides_ctx16<NV>(key + first, value + first, guide, push.pair0[item], it.Q, g, lane, scale,
                                  ctx16 + ((long)it.ctx_row0 + (win - it.win0)) * D, (long)it.wins * D);
}

// ---- 2: segmented many-row stream: the item's frames count from its absolute offset, its query rows are its slot's pairs' ----
struct GmStreamParams {
    SegStreamParams c;
    const uint16_t* x;      // [sum N_i][E]
    float* scores;
    const GmUnit* units;
    const GmItem* items;
    GmPush push;
};

template <int NB>
__global__ __launch_bounds__(512, 1) void gm_stream_kernel(GmStreamParams p) {
    constexpr int E = NB * 128;
    const GmUnit u = p.units[blockIdx.x];
    const GmItem it = p.items[u.item];
    SegStreamParams c = p.c;
    c.t0i += p.push.t0[u.item];
    stream_segment<NB, 2>(c, p.x + (long)it.tok0 * E, it.N, u.tb, u.te, 32 * u.pass, c.rows * it.Q, (long)p.push.pair0[u.item] * c.rows,
                          p.scores + (long)it.score_off * 16, (long)((it.N + 15) / 16 * 16), (long)u.slot, it.chunks);
}

// ---- 3: merge + fold, grid (nh max Q, items), 256 threads: one workgroup owns one (item, folded row) ----
struct GmMergeParams {
    SegMergeParams c;
    const float* scores;
    const GmItem* items;    // NULL: every item has u_T frames, u_Q guides and u_nparts chunks, packed one behind the other (the stand-alone entry)
    int u_T, u_Q, u_nparts;
    int rows;               // heads
    float* state_ml;        // [M rows][2]
    float* state_acc;       // [M rows][E]
    GmPush push;
};

__global__ __launch_bounds__(256) void gm_merge_fold_kernel(GmMergeParams p) {
    extern __shared__ float ms[];
    const int R = blockIdx.x, item = blockIdx.y;
    int T, N, Q, nparts;
    long slot0, soff;
    if (p.items) {
        const GmItem it = p.items[item];
        T = it.T; N = it.N; Q = it.Q; nparts = it.chunks; slot0 = it.slot0; soff = it.score_off;
    } else {
        T = p.u_T; N = T * p.c.H * p.c.W; Q = p.u_Q; nparts = p.u_nparts;
        const long passes = (p.rows * Q + 31) / 32;
        slot0 = item * 2 * passes * nparts;
        soff = item * passes * 32 * ((N + 15) / 16);
    }
    if (R >= p.rows * Q) return;                                // (uniform over the workgroup, in front of every barrier)
    const long stride = (N + 15) / 16 * 16;
    const long row = (long)p.push.pair0[item] * p.rows + R;
    merge_fold_row(p.c, ms, R & 15, threadIdx.x, T, p.push.t0[item], nparts, slot0 + (long)(R >> 4) * nparts, p.scores + soff * 16 + R * stride,
                   p.state_ml + 2 * row, p.state_acc + row * p.c.E);
}

// ---- 6: placement, one output row per workgroup over all pairs' chunk rows, into the pair's own buffer ----
struct GmPlaceParams {
    SegPlaceParams c;
    const GmItem* items;
    const int* row_item;
    int nl_group;
    long ldo, pair_stride;
    GmPush push;
};

__global__ __launch_bounds__(128) void gm_place_kernel(GmPlaceParams p) {
    const long row = blockIdx.x;
    const int item = p.row_item[row];
    const GmItem it = p.items[item];
    const long local = row - it.lrow0;
    const long q = local / it.rows, r = local - q * it.rows;
    place_row(p.c, r, ((long)p.push.pair0[item] + q) * p.pair_stride + ((long)p.push.row0[item] + r) * p.ldo, 0, (long)it.ctx_row0 + q * it.wins, p.nl_group,
              it.nl_count, it.rows, p.nl_group, p.nl_group + 1);
}

// ---- finish_many: the rows behind the local rows of every pair of a named slot; grid (tail + global rows, max Q, B) ----
struct GmFinish {
    int pair0[kGmMax];
    int Q[kGmMax];
    int row0[kGmMax];       // the slot's first row behind its local rows
    unsigned named;         // bit s: slot s is placed
};

struct GmPlaceGlobalParams {
    SegPlaceParams c;       // loc NULL: every row is a newline row or a global row
    int tail;               // whole-clip newline rows in front of the global rows (0 | 1)
    long ldo, pair_stride;
    GmFinish f;
};

__global__ __launch_bounds__(128) void gm_place_global_kernel(GmPlaceGlobalParams p) {
    const int r = blockIdx.x, q = blockIdx.y, slot = blockIdx.z;
    if (!(p.f.named >> slot & 1u) || q >= p.f.Q[slot]) return;
    const long pair = (long)p.f.pair0[slot] + q;
    place_row(p.c, r, pair * p.pair_stride + ((long)p.f.row0[slot] + r) * p.ldo, pair, 0, 0, p.tail, p.tail, 0, 1);
}

}  // namespace hicom

using namespace hicom;
using namespace hicom_host;

namespace {

constexpr const char* kWho = "compressor_stream_group_multi";
constexpr int kPassRows = 32;               // folded rows of one pass of the stream

typedef hicom_stream_group_multi_push_args Args;

struct GmLayout {
    long items, units, win_item, row_item, table_bytes;     // the table region
    long scores, part_m, part_l, part_acc, ctx16, hid16, loc, total;
    long windows, ctx_rows, rows, slots, nunits, work_sum, score16;
    int max_T, max_Q, wps;
};

long item_win(const Args* a, int i, int wps) { return (long)(a->tc[i] / a->kt) * wps; }
long item_nl(const Args* a, int i, int wps) { return a->nl_group > 0 ? item_win(a, i, wps) / a->nl_group : 0; }
long item_passes(const Args* a, int i) { return ((long)a->nh * a->q[i] + kPassRows - 1) / kPassRows; }

// everything that the tuple of (chunk length, guide count) and the geometry decide: the checks of workspace_bytes, prepare and push
int gm_check_shape(const Args* a) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "%s: NULL arguments", kWho);
    HICOM_REQUIRE(a->B >= 1 && a->B <= kGmMax, HICOM_EUNSUP, "%s: B=%d slots (1 <= B <= %d per group)", kWho, a->B, kGmMax);
    HICOM_REQUIRE(a->M >= a->B && a->M <= kGmMax * kGmMax, HICOM_EINVAL, "%s: M=%d (slot, guide) pairs for %d slots (B <= M <= %d)", kWho, a->M, a->B,
                  kGmMax * kGmMax);
    HICOM_REQUIRE(a->items >= 1 && a->items <= a->B, HICOM_EINVAL, "%s: %d items in one push (1 .. B = %d: a slot appears at most once)", kWho, a->items, a->B);
    HICOM_REQUIRE(a->H > 0 && a->W > 0 && a->kt > 0 && a->ks > 0 && a->hidden > 0 && a->nh > 0 && a->chunks >= 0 && a->nl_group >= 0, HICOM_EINVAL, "%s: bad shape",
                  kWho);
    HICOM_REQUIRE(a->E == 1152, HICOM_EUNSUP, "%s: E=%d (only 1152)", kWho, a->E);
    HICOM_REQUIRE(a->nh <= 16 && a->E % a->nh == 0, HICOM_EUNSUP, "%s: %d heads (<= 16 folded rows per pair)", kWho, a->nh);
    HICOM_REQUIRE(a->hidden % 64 == 0, HICOM_EUNSUP, "%s: hidden=%d (multiple of 64: fp16 readout planes)", kWho, a->hidden);
    HICOM_REQUIRE(a->out_dt == HICOM_DT_F32 || a->out_dt == HICOM_DT_BF16, HICOM_EUNSUP, "%s: output dtype %d (bf16 | f32)", kWho, a->out_dt);
    HICOM_REQUIRE(a->H % a->ks == 0 && a->W % a->ks == 0, HICOM_EUNSUP, "%s: needs an exact window partition (H=%d W=%d, windows %dx%dx%d)", kWho, a->H, a->W,
                  a->kt, a->ks, a->ks);
    HICOM_REQUIRE(a->kt * a->ks * a->ks <= 64, HICOM_EUNSUP, "%s: windows of %d tokens (<= 64)", kWho, a->kt * a->ks * a->ks);
    const int wps = (a->H / a->ks) * (a->W / a->ks);
    long tokens = 0, products = 0, ctx_rows = 0;
    int max_T = 0;
    for (int i = 0; i < a->items; ++i) {
        HICOM_REQUIRE(a->q[i] >= 1 && a->q[i] <= kGmMax, HICOM_EUNSUP, "%s: item %d: Q=%d guides (1 <= Q <= %d per slot)", kWho, i, a->q[i], kGmMax);
        HICOM_REQUIRE(a->tc[i] > 0 && a->tc[i] % a->kt == 0, HICOM_EUNSUP, "%s: item %d needs an exact window partition (Tc=%d, temporal window %d)", kWho, i,
                      a->tc[i], a->kt);
        const long N = (long)a->tc[i] * a->H * a->W;
        HICOM_REQUIRE(N < (1L << 27), HICOM_EUNSUP, "%s: item %d: too many tokens", kWho, i);
        HICOM_REQUIRE(!a->nl_group || item_win(a, i, wps) % a->nl_group == 0, HICOM_EINVAL, "%s: item %d: output layout", kWho, i);
        tokens += N;
        products += item_passes(a, i) * kPassRows * ((N + 15) / 16);
        ctx_rows += a->q[i] * item_win(a, i, wps);
        if (a->tc[i] > max_T) max_T = a->tc[i];
    }
    // (item offsets, the logits' offsets -- counted in 16 floats, 32 rows per pass and tile -- and the context rows are ints on the device)
    HICOM_REQUIRE(tokens + 16L * a->items < (1L << 27), HICOM_EUNSUP, "%s: too many tokens in one push", kWho);
    HICOM_REQUIRE(products < (1L << 27), HICOM_EUNSUP, "%s: too many token x guide products in one push", kWho);
    HICOM_REQUIRE(ctx_rows < (1L << 20), HICOM_EUNSUP, "%s: %ld window contexts over all pairs of one push (< 2^20)", kWho, ctx_rows);
    return seg_check_merge_lds(kWho, a, max_T);
}

GmLayout gm_layout(const Args* a) {
    GmLayout l{};
    const long HW = (long)a->H * a->W, E = a->E;
    l.wps = (a->H / a->ks) * (a->W / a->ks);
    for (int i = 0; i < a->items; ++i) {
        const long N = a->tc[i] * HW, w = item_win(a, i, l.wps), ntiles = (N + 15) / 16;
        l.windows += w;
        l.ctx_rows += a->q[i] * w;
        l.rows += a->q[i] * (w + item_nl(a, i, l.wps));
        l.score16 += item_passes(a, i) * kPassRows * ntiles;
        l.work_sum += ntiles * item_passes(a, i);
        if (a->tc[i] > l.max_T) l.max_T = a->tc[i];
        if (a->q[i] > l.max_Q) l.max_Q = a->q[i];
    }
    const int ncu = a->chunks > 0 ? 0 : num_cus();
    for (int i = 0; i < a->items; ++i) l.nunits += seg_share_chunks((a->tc[i] * HW + 15) / 16, l.work_sum, a->chunks, ncu) * item_passes(a, i);
    l.slots = 2 * l.nunits;
    long off = 0;
    auto take = [&](long bytes) { const long at = off; off += (bytes + 255) / 256 * 256; return at; };
    const int odt = a->out_dt == HICOM_DT_F32 ? 4 : 2;
    l.items = take(a->items * (long)sizeof(GmItem));
    l.units = take(l.nunits * (long)sizeof(GmUnit));
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
    l.total = off;
    return l;
}

GmPush gm_push_values(const int32_t* pair0, const int32_t* t0, const int32_t* row0, int items) {
    GmPush v{};
    for (int i = 0; i < items; ++i) {
        v.pair0[i] = pair0[i];
        v.t0[i] = t0[i];
        v.row0[i] = row0 ? row0[i] : 0;
    }
    return v;
}

// the items' pair ranges lie inside the M pairs and do not meet: one workgroup owns a carried row, and only when no other item of the push
// folds into it
int gm_check_pairs(const char* who, const int32_t* pair0, const int32_t* q, int uniform_q, int items, int M) {
    for (int i = 0; i < items; ++i) {
        const int Qi = q ? q[i] : uniform_q;
        HICOM_REQUIRE(pair0[i] >= 0 && (long)pair0[i] + Qi <= M, HICOM_EINVAL, "%s: item %d: pairs %d .. %d outside the group's %d pairs", who, i, pair0[i],
                      pair0[i] + Qi, M);
        for (int j = 0; j < i; ++j) {
            const int Qj = q ? q[j] : uniform_q;
            HICOM_REQUIRE(pair0[i] + Qi <= pair0[j] || pair0[j] + Qj <= pair0[i], HICOM_EINVAL,
                          "%s: items %d and %d share a pair (%d .. %d and %d .. %d: a state is updated in place)", who, j, i, pair0[j], pair0[j] + Qj, pair0[i],
                          pair0[i] + Qi);
        }
    }
    return HICOM_OK;
}

// slots distinct and < B
int gm_check_slots(const char* who, const int32_t* slot, int items, int B) {
    uint32_t seen = 0;
    for (int i = 0; i < items; ++i) {
        HICOM_REQUIRE(slot[i] >= 0 && slot[i] < B, HICOM_EINVAL, "%s: item %d: slot %d (0 <= slot < B = %d)", who, i, slot[i], B);
        HICOM_REQUIRE(!(seen >> slot[i] & 1u), HICOM_EINVAL, "%s: item %d: slot %d appears twice in one push (its state is updated in place)", who, i, slot[i]);
        seen |= 1u << slot[i];
    }
    return HICOM_OK;
}

}  // namespace

extern "C" int64_t hicom_compressor_stream_group_multi_workspace_bytes(const hicom_stream_group_multi_push_args* a) {
    const int st = gm_check_shape(a);
    if (st != HICOM_OK) return st;
    return gm_layout(a).total;
}

extern "C" int hicom_compressor_stream_group_multi_prepare(const hicom_stream_group_multi_push_args* a) {
    int st = gm_check_shape(a);
    if (st != HICOM_OK) return st;
    const GmLayout l = gm_layout(a);
    st = seg_check_ws(kWho, a, l.total);
    if (st != HICOM_OK) return st;
    std::vector<int> tab((size_t)(l.table_bytes / 4), 0);
    GmItem* items = reinterpret_cast<GmItem*>(tab.data() + l.items / 4);
    GmUnit* units = reinterpret_cast<GmUnit*>(tab.data() + l.units / 4);
    int* win_item = tab.data() + l.win_item / 4;
    int* row_item = tab.data() + l.row_item / 4;
    const long HW = (long)a->H * a->W;
    const int ncu = a->chunks > 0 ? 0 : num_cus();
    long tok = 0, win = 0, row = 0, score = 0, slot = 0, unit = 0, ctx_row = 0;
    for (int i = 0; i < a->items; ++i) {
        const long N = a->tc[i] * HW, w = item_win(a, i, l.wps), nl = item_nl(a, i, l.wps), ntiles = (N + 15) / 16, passes = item_passes(a, i);
        const int Q = a->q[i], chunks = seg_share_chunks(ntiles, l.work_sum, a->chunks, ncu);
        GmItem& d = items[i];
        d.tok0 = (int)tok; d.N = (int)N; d.T = a->tc[i]; d.win0 = (int)win; d.wins = (int)w; d.slot0 = (int)slot; d.chunks = chunks;
        d.score_off = (int)score; d.Q = Q; d.ctx_row0 = (int)ctx_row; d.lrow0 = (int)row; d.rows = (int)(w + nl); d.nl_count = (int)nl;
        for (long p = 0; p < passes; ++p)
            for (int c = 0; c < chunks; ++c) {
                GmUnit& u = units[unit++];
                u.item = i; u.tb = seg_tile_at(ntiles, c, chunks); u.te = seg_tile_at(ntiles, c + 1, chunks); u.pass = (int)p;
                u.slot = (int)(slot + 2 * p * chunks + c);
            }
        for (long k = 0; k < w; ++k) win_item[win + k] = i;
        for (long k = 0; k < Q * (w + nl); ++k) row_item[row + k] = i;
        tok += N; win += w; row += Q * (w + nl); score += passes * kPassRows * ntiles; slot += 2 * passes * chunks; ctx_row += Q * w;
    }
    return seg_upload_tables(kWho, a, tab.data(), l.table_bytes);
}

extern "C" int hicom_compressor_stream_group_multi_push(const hicom_stream_group_multi_push_args* a) {
    int st = gm_check_shape(a);
    if (st != HICOM_OK) return st;
    const GmLayout l = gm_layout(a);
    st = seg_check_ws(kWho, a, l.total);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->ff && a->guide && a->q_hi && a->q_lo && a->state_ml && a->state_acc && a->out, HICOM_EINVAL, "%s: NULL pointer", kWho);
    HICOM_REQUIRE(a->lw0_f16 && a->lb0 && a->lw2_f16 && a->lb2, HICOM_EINVAL, "%s: NULL weight", kWho);
    HICOM_REQUIRE((a->pos_a != nullptr) == (a->pe != nullptr) && (!a->pe || a->P > 0), HICOM_EINVAL, "%s: pos_a and pe come together", kWho);
    HICOM_REQUIRE((uintptr_t)a->ff % 16 == 0 && (uintptr_t)a->fe % 16 == 0 && (uintptr_t)a->guide % 16 == 0 && (uintptr_t)a->q_hi % 16 == 0 &&
                      (uintptr_t)a->q_lo % 16 == 0 && (uintptr_t)a->lw0_f16 % 16 == 0 && (uintptr_t)a->lw2_f16 % 16 == 0 && (uintptr_t)a->state_acc % 16 == 0 &&
                      (uintptr_t)a->state_ml % 8 == 0, HICOM_EINVAL, "%s: 16-byte aligned inputs, planes and accumulators, 8-byte aligned (M, L)", kWho);
    st = gm_check_slots(kWho, a->slot, a->items, a->B);
    if (st != HICOM_OK) return st;
    st = gm_check_pairs(kWho, a->pair0, a->q, 0, a->items, a->M);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->ldo >= a->hidden && a->pair_rows > 0 && a->pair_stride >= a->pair_rows * a->ldo, HICOM_EINVAL,
                  "%s: output layout (%ld rows per pair, row length %ld, pairs %ld elements apart)", kWho, (long)a->pair_rows, (long)a->ldo, (long)a->pair_stride);
    HICOM_REQUIRE(a->nl_group == 0 || a->newline, HICOM_EINVAL, "%s: newline rows (one behind every %d token rows) and there is no newline token", kWho,
                  a->nl_group);
    for (int i = 0; i < a->items; ++i) {
        HICOM_REQUIRE(a->t0[i] >= 0 && a->t0[i] % a->kt == 0, HICOM_EINVAL, "%s: item %d: t0=%d (whole window groups of %d frames)", kWho, i, a->t0[i], a->kt);
        if (a->pe)
            HICOM_REQUIRE((long)a->t0[i] + a->tc[i] <= a->y_index0 && a->y_index0 + a->H <= a->x_index0 && a->x_index0 + a->W <= a->P, HICOM_EINVAL,
                          "%s: item %d: frames %d .. %d, grid %dx%d outside the positional tables (t < %d, y at %d, x at %d, %d rows)", kWho, i, a->t0[i],
                          a->t0[i] + a->tc[i], a->H, a->W, a->y_index0, a->y_index0, a->x_index0, a->P);
        const long rows = item_win(a, i, l.wps) + item_nl(a, i, l.wps);
        HICOM_REQUIRE(a->row0[i] >= 0 && (long)a->row0[i] + rows <= a->pair_rows, HICOM_EINVAL, "%s: item %d: rows %d .. %ld outside the pair's buffer of %ld rows",
                      kWho, i, a->row0[i], (long)a->row0[i] + rows, (long)a->pair_rows);
    }
    HICOM_REQUIRE(l.windows <= INT32_MAX && l.rows <= INT32_MAX && l.nunits <= INT32_MAX, HICOM_EUNSUP, "%s: too many windows in one push", kWho);

    char* ws = (char*)a->ws;
    hipStream_t s = (hipStream_t)a->stream;
    const GmPush push = gm_push_values(a->pair0, a->t0, a->row0, a->items);
    const GmItem* items = (const GmItem*)(ws + l.items);
    const uint16_t* key_x = (const uint16_t*)(a->fe ? a->fe : a->ff);      // (no frames_embed: the keys are frames_feature)

    // 1: local stage
    {
        const hicom_axis ay{a->H, a->ks, a->H / a->ks, a->H / a->ks}, ax{a->W, a->ks, a->W / a->ks, a->W / a->ks};
        HICOM_LAUNCH(gm_local_kernel<3>, dim3((unsigned)((l.windows + 3) / 4)), dim3(256), 0, s, key_x, (const uint16_t*)a->ff, (const uint16_t*)a->guide, items,
                     (const int*)(ws + l.win_item), ay, ax, (int)a->kt, (int)l.windows, a->l_scale, (_Float16*)(ws + l.ctx16), push);
        st = seg_check_launch(kWho, "local stage");
        if (st != HICOM_OK) return st;
    }
    // 2: segmented global stream
    {
        GmStreamParams p;
        p.c.qhi = (const uint16_t*)a->q_hi; p.c.qlo = (const uint16_t*)a->q_lo;
        p.c.pos_a = a->pos_a; p.c.pos_stride = a->P; p.c.rows = a->nh;
        p.c.H = a->H; p.c.W = a->W; p.c.HW = a->H * a->W;
        p.c.t0i = 0; p.c.y0i = a->y_index0; p.c.x0i = a->x_index0;
        p.c.part_m = (float*)(ws + l.part_m); p.c.part_l = (float*)(ws + l.part_l); p.c.part_acc = (float*)(ws + l.part_acc);
        p.x = (const uint16_t*)a->ff;
        p.scores = (float*)(ws + l.scores);
        p.units = (const GmUnit*)(ws + l.units); p.items = items;
        p.push = push;
        // (once per process, as in the other many-item steps: one device per process; a repeated call from a second host thread is harmless)
        static bool attr_set = false;
        if (!attr_set) {
            const hipError_t e =
                hipFuncSetAttribute(reinterpret_cast<const void*>(gm_stream_kernel<9>), hipFuncAttributeMaxDynamicSharedMemorySize, seg_stream_smem(2));
            if (e != hipSuccess) {
                set_error("%s: global stream: %d bytes of LDS per workgroup: %s", kWho, seg_stream_smem(2), hipGetErrorString(e));
                return HICOM_ELAUNCH;
            }
            attr_set = true;
        }
        HICOM_LAUNCH(gm_stream_kernel<9>, dim3((unsigned)l.nunits), dim3(512), seg_stream_smem(2), s, p);
        st = seg_check_launch(kWho, "global stream");
        if (st != HICOM_OK) return st;
    }
    // 3: merge + fold into every item's pairs
    {
        GmMergeParams p;
        p.c.part_m = (const float*)(ws + l.part_m); p.c.part_l = (const float*)(ws + l.part_l); p.c.part_acc = (const float*)(ws + l.part_acc);
        p.c.pe = a->pe; p.c.E = a->E; p.c.H = a->H; p.c.W = a->W;
        p.c.t0i = 0; p.c.y0i = a->y_index0; p.c.x0i = a->x_index0;
        p.scores = (const float*)(ws + l.scores);
        p.items = items; p.u_T = 0; p.u_Q = 0; p.u_nparts = 0; p.rows = a->nh;
        p.state_ml = a->state_ml; p.state_acc = a->state_acc;
        p.push = push;
        HICOM_LAUNCH(gm_merge_fold_kernel, dim3((unsigned)(a->nh * l.max_Q), (unsigned)a->items), dim3(256), (size_t)seg_merge_smem(l.max_T, a->H, a->W), s, p);
        st = seg_check_launch(kWho, "merge and fold");
        if (st != HICOM_OK) return st;
    }
    // 4-5: the local readout as one GEMM pair over all pairs' window contexts
    st = hicom_readout16_gemm_fwd(ws + l.ctx16, a->lw0_f16, a->lb0, HICOM_DT_BF16, (int32_t)l.ctx_rows, a->hidden, a->E, HICOM_ACT_GELU, ws + l.hid16, nullptr, 0, 0,
                                  0, 0, nullptr, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_readout16_gemm_fwd(ws + l.hid16, a->lw2_f16, a->lb2, HICOM_DT_BF16, (int32_t)l.ctx_rows, a->hidden, a->hidden, HICOM_ACT_NONE, nullptr, ws + l.loc,
                                  a->out_dt, a->hidden, 0, 0, nullptr, a->stream);
    if (st != HICOM_OK) return st;
    // 6: every pair's chunk rows to its own buffer
    GmPlaceParams p;
    p.c.loc = ws + l.loc; p.c.tok = nullptr; p.c.newline = (const uint16_t*)a->newline; p.c.out = a->out;
    p.c.out_f32 = a->out_dt == HICOM_DT_F32; p.c.hidden = a->hidden;
    p.items = items; p.row_item = (const int*)(ws + l.row_item); p.nl_group = a->nl_group;
    p.ldo = a->ldo; p.pair_stride = a->pair_stride;
    p.push = push;
    HICOM_LAUNCH(gm_place_kernel, dim3((unsigned)l.rows), dim3(128), 0, s, p);
    return seg_check_launch(kWho, "placement");
}

// The merge + fold kernel alone: `items` chunks of Tc frames with Q guides each; item i's partials in the slots [i S, (i + 1) S), S = 2 passes
// nparts, ordered [pass][row group][chunk]; its logits [32 passes][ceil16(Tc H W)] at scores + i 32 passes ceil16(Tc H W); folded into the state
// rows pair0[i] rows + R, R < rows Q.
extern "C" int hicom_stream_group_multi_merge_fold_fwd(const float* part_m, const float* part_l, const float* part_acc, const float* scores, int32_t items,
                                                       int32_t nparts, int32_t rows, int32_t Q, int32_t E, int32_t Tc, int32_t H, int32_t W, const float* pe,
                                                       int32_t P, int32_t y_index0, int32_t x_index0, const int32_t* pair0, const int32_t* t0, int32_t M,
                                                       float* state_ml, float* state_acc, void* stream) {
    constexpr const char* who = "stream_group_multi_merge_fold";
    HICOM_REQUIRE(part_m && part_l && part_acc && pair0 && t0 && state_ml && state_acc, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE(Q >= 1 && Q <= kGmMax, HICOM_EUNSUP, "%s: Q=%d guides (1 <= Q <= %d per slot)", who, Q, kGmMax);
    HICOM_REQUIRE(items >= 1 && items <= kGmMax && M >= 1 && M <= kGmMax * kGmMax && nparts >= 1 && nparts <= kSegMaxChunks && rows >= 1 && rows <= 16 && E > 0 &&
                      E % 4 == 0 && Tc > 0 && H > 0 && W > 0 && (long)Tc * H * W < (1L << 27) / (kGmMax * kGmMax), HICOM_EINVAL,
                  "%s: bad shape (items=%d M=%d nparts=%d rows=%d E=%d Tc=%d H=%d W=%d)", who, items, M, nparts, rows, E, Tc, H, W);
    HICOM_REQUIRE(!pe || scores, HICOM_EINVAL, "%s: the positional term needs the logits", who);
    HICOM_REQUIRE((uintptr_t)part_acc % 16 == 0 && (uintptr_t)state_acc % 16 == 0 && (uintptr_t)state_ml % 8 == 0, HICOM_EINVAL,
                  "%s: 16-byte aligned accumulators, 8-byte aligned (M, L)", who);
    HICOM_REQUIRE(seg_merge_smem(Tc, H, W) <= 48 * 1024, HICOM_EUNSUP, "%s: Tc=%d frames of %dx%d: the merge keeps Tc (H + W) marginal sums in LDS", who, Tc, H, W);
    int st = gm_check_pairs(who, pair0, nullptr, Q, items, M);
    if (st != HICOM_OK) return st;
    for (int i = 0; i < items; ++i) {
        HICOM_REQUIRE(t0[i] >= 0, HICOM_EINVAL, "%s: item %d: t0=%d", who, i, t0[i]);
        if (pe)
            HICOM_REQUIRE((long)t0[i] + Tc <= y_index0 && y_index0 + H <= x_index0 && x_index0 + W <= P, HICOM_EINVAL,
                          "%s: item %d: frames %d .. %d, grid %dx%d outside the positional tables (t < %d, y at %d, x at %d, %d rows)", who, i, t0[i], t0[i] + Tc, H,
                          W, y_index0, y_index0, x_index0, P);
    }
    GmMergeParams p;
    p.c.part_m = part_m; p.c.part_l = part_l; p.c.part_acc = part_acc;
    p.c.pe = pe; p.c.E = E; p.c.H = H; p.c.W = W;
    p.c.t0i = 0; p.c.y0i = y_index0; p.c.x0i = x_index0;
    p.scores = scores;
    p.items = nullptr; p.u_T = Tc; p.u_Q = Q; p.u_nparts = nparts; p.rows = rows;
    p.state_ml = state_ml; p.state_acc = state_acc;
    p.push = gm_push_values(pair0, t0, nullptr, items);
    HICOM_LAUNCH(gm_merge_fold_kernel, dim3((unsigned)(rows * Q), (unsigned)items), dim3(256), (size_t)seg_merge_smem(Tc, H, W), (hipStream_t)stream, p);
    return seg_check_launch(who, "merge and fold");
}

// The placement of finish_many alone: for every slot s with bit s of `named` set and every q < guide_counts[s], behind row row0[s] of pair
// pair0_s + q: `tail` copies of newline, then n_rows copies of tok[pair0_s + q] (rounded once).  Nothing else is read or written.
extern "C" int hicom_stream_group_place_global_fwd(const float* tok, const void* newline, int32_t B, const int32_t* guide_counts, const int32_t* row0,
                                                   uint32_t named, int32_t tail, int32_t n_rows, int32_t hidden, void* out, int32_t out_dt, int64_t ldo,
                                                   int64_t pair_stride, int64_t pair_rows, void* stream) {
    constexpr const char* who = "stream_group_place_global";
    HICOM_REQUIRE(tok && out && guide_counts && row0, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE(B >= 1 && B <= kGmMax, HICOM_EUNSUP, "%s: B=%d slots (1 <= B <= %d per group)", who, B, kGmMax);
    HICOM_REQUIRE(out_dt == HICOM_DT_F32 || out_dt == HICOM_DT_BF16, HICOM_EUNSUP, "%s: output dtype %d (bf16 | f32)", who, out_dt);
    HICOM_REQUIRE(hidden > 0 && n_rows > 0 && (tail == 0 || tail == 1) && ldo >= hidden && pair_rows > 0 && pair_stride >= pair_rows * ldo, HICOM_EINVAL,
                  "%s: bad shape (hidden=%d, %d global rows behind %d newline rows, %ld rows per pair of %ld elements, pairs %ld elements apart)", who, hidden,
                  n_rows, tail, (long)pair_rows, (long)ldo, (long)pair_stride);
    HICOM_REQUIRE(tail == 0 || newline, HICOM_EINVAL, "%s: a newline row and there is no newline token", who);
    HICOM_REQUIRE(named != 0 && (B == 32 || !(named >> B)), HICOM_EINVAL, "%s: named slots %#x (a non-empty set of the %d slots)", who, named, B);
    GmPlaceGlobalParams p;
    int pair = 0, max_Q = 0;
    for (int s = 0; s < kGmMax; ++s) p.f.pair0[s] = p.f.Q[s] = p.f.row0[s] = 0;
    for (int s = 0; s < B; ++s) {
        const int Q = guide_counts[s];
        HICOM_REQUIRE(Q >= 1 && Q <= kGmMax, HICOM_EUNSUP, "%s: slot %d: Q=%d guides (1 <= Q <= %d per slot)", who, s, Q, kGmMax);
        p.f.pair0[s] = pair; p.f.Q[s] = Q; p.f.row0[s] = row0[s];
        pair += Q;
        if (!(named >> s & 1u)) continue;
        HICOM_REQUIRE(row0[s] >= 0 && (long)row0[s] + tail + n_rows <= pair_rows, HICOM_EINVAL, "%s: slot %d: rows %d .. %ld outside the pair's buffer of %ld rows",
                      who, s, row0[s], (long)row0[s] + tail + n_rows, (long)pair_rows);
        if (Q > max_Q) max_Q = Q;
    }
    p.f.named = named;
    p.c.loc = nullptr; p.c.tok = tok; p.c.newline = (const uint16_t*)newline; p.c.out = out;
    p.c.out_f32 = out_dt == HICOM_DT_F32; p.c.hidden = hidden;
    p.tail = tail; p.ldo = ldo; p.pair_stride = pair_stride;
    HICOM_LAUNCH(gm_place_global_kernel, dim3((unsigned)(tail + n_rows), (unsigned)max_Q, (unsigned)B), dim3(128), 0, (hipStream_t)stream, p);
    return seg_check_launch(who, "placement");
}
