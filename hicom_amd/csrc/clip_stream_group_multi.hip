// Clip stream group with several guides per slot: B live videos, slot s with its own Q_s guides and one carried softmax
// state per (slot, guide) PAIR, pushed in ONE host call from the vision tower's stacked [sum Tc_i, H, W, E] tensor.  Pairs are numbered
// slot-major, then guide-major: slot s owns the pairs [pair0_s, pair0_s + Q_s), pair0_s = sum_{j<s} Q_j, M = sum Q_s of them
// (forward_ragged_multi_guide's convention).  One push is six launches whatever B, the Q_s and the mix of chunk lengths are:
//    1  gm_local_kernel: one wave per window of the STACKED tensor, the wave walks the guides of the item's SLOT in groups of kGuideGroup
//       (multi_window.hpp: multi_window_guides_ctx16), fp16 contexts pair-major within the call as in rmg_local_kernel
//    2  gm_stream_kernel: stream_segment<9, 2> (stream_body.hpp), 32 densely packed folded rows of ONE item per workgroup, the frame rows of
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
//
// This file has the kernels, their table entries, the description of the flavour (Multi) and the finish placement's entry; the host side of
// the other entry points is stream_group_host.hpp, shared with clip_stream_group.hip.  At the foot: the same group on the k / v adaptor
// recipe -- the flavour Adapt, which is Multi with a front of its own (the adaptor MLPs over the stacked tokens and
// gm_local_adapt_kernel in the place of launch 1), its three entry points and the stand-alone entry of its local stage.
#include "merge_fold.hpp"
#include "multi_window.hpp"
#include "stream_group_host.hpp"

namespace hicom {

constexpr int kGmMax = kGroupMax;        // slots per group, items per push and guides per slot
typedef GroupPush GmPush;                // (pair0: the first pair of the item's slot)

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

// The logits form of launch 1: the same wave -> window -> item map and the same pair-major context placement with the local
// logits given (multi_window.hpp: multi_window_guides_logits_ctx16).  logits f32 [max Q over the push's items][q_stride]: guide q of item i
// at q q_stride + tok0_i + n, n counted from the item's first token -- the layout hicom_head_scores_ragged_fwd writes for the tick's stack;
// planes q >= Q_i of an item's columns are not read.  Guide q of an item is plane q, so the slot's first pair is not needed; no key row
// and no guide row is read.
template <int NV>
__global__ __launch_bounds__(256) void gm_local_logits_kernel(const uint16_t* value, const float* logits, long q_stride, const GmItem* items,
                                                              const int* win_item, hicom_axis ay, hicom_axis ax, int kt, int nwin, float scale,
                                                              _Float16* ctx16) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const GmItem it = items[win_item[win]];
    const hicom_axis at{it.T, kt, it.T / kt, it.T / kt};
    const WindowGeom g(at, ay, ax, win - it.win0);
    multi_window_guides_logits_ctx16<NV>(value + (long)it.tok0 * D, logits + it.tok0, q_stride, it.Q, g, lane, scale,
                                         ctx16 + ((long)it.ctx_row0 + (win - it.win0)) * D, (long)it.wins * D);
}

// The same wave -> window map for the k / v adaptor recipe: launch 3 of the adaptor flavour's push, behind the adaptor MLPs
// over the tick's STACKED tokens.  ad: gamma / beta / alpha / eps of the call and the fp16 planes y = MLP(x) of the whole stack (either may
// be NULL, not both), indexed like the tokens: the by-value copy has them advanced to the item's first token, as clips_local_adapt_kernel
// (ragged_multi_guide.hip) replaces them per item.  Contexts pair-major, exactly where gm_local_kernel puts them.  items NULL: the
// stand-alone entry's uniform form -- every item has u_T frames and u_Q guides, tokens, planes and context rows packed item after item.
// Every branch on `items` and every lookup is wave-uniform (win is); nothing is stored through what the lookups return.
template <int NV>
__global__ __launch_bounds__(256) void gm_local_adapt_kernel(const uint16_t* key, const uint16_t* value, const uint16_t* guide, SegAdaptParams ad,
                                                             const GmItem* items, const int* win_item, hicom_axis ay, hicom_axis ax, int kt, int nwin,
                                                             int u_T, int u_Q, float scale, _Float16* ctx16, GmPush push) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    int item, T, Q, win0, wins;
    long tok0, ctx_row0;
    if (items) {
        item = win_item[win];
        const GmItem it = items[item];
        T = it.T; Q = it.Q; win0 = it.win0; wins = it.wins; tok0 = it.tok0; ctx_row0 = it.ctx_row0;
    } else {
        T = u_T; Q = u_Q; wins = (u_T / kt) * ay.nwin * ax.nwin;
        item = win / wins;
        win0 = item * wins; tok0 = (long)item * u_T * ay.n * ax.n; ctx_row0 = (long)item * u_Q * wins;
    }
    const hicom_axis at{T, kt, T / kt, T / kt};
    const WindowGeom g(at, ay, ax, win - win0);
    const long first = tok0 * D;
    if (ad.ky) ad.ky += first;
    if (ad.vy) ad.vy += first;
    multi_window_guides_adapt_ctx16<NV, kAdaptGuideGroup>(key + first, value + first, ad, guide, push.pair0[item], Q, g, lane, scale,
                                                          ctx16 + (ctx_row0 + (win - win0)) * D, (long)wins * D);
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

// Q_i guides per item: nh Q_i folded rows in passes of 32 (two row groups per stream workgroup), one work unit per (pass, token chunk).
// Names: the message prefixes (the adaptor flavour at the foot of this file is the same description under its own)
struct MultiNames {
    static constexpr const char *kWho = "compressor_stream_group_multi", *kFoldWho = "stream_group_multi_merge_fold";
};

template <class Names>
struct MultiOf : GroupPlainFront<MultiOf<Names>> {
    typedef hicom_stream_group_multi_push_args Args;
    typedef GmItem Item;
    typedef GmUnit Unit;
    typedef GmStreamParams StreamParams;
    typedef GmMergeParams MergeParams;
    typedef GmPlaceParams PlaceParams;
    static constexpr const char *kWho = Names::kWho, *kFoldWho = Names::kFoldWho, *kUnit = "pair";
    static constexpr int kRowGroups = 2;
    static constexpr auto kStride = &Args::pair_stride, kRows = &Args::pair_rows;
    static constexpr auto kPlaceStride = &PlaceParams::pair_stride;
    static constexpr auto local = gm_local_kernel<3>;
    static constexpr auto stream = gm_stream_kernel<9>;
    static constexpr auto merge = gm_merge_fold_kernel;
    static constexpr auto place = gm_place_kernel;

    static int guides(const Args* a, int i) { return a->q[i]; }
    static const int32_t* unit0(const Args* a) { return a->pair0; }
    static int check_group(const Args* a) {
        HICOM_REQUIRE(a->M >= a->B && a->M <= kGmMax * kGmMax, HICOM_EINVAL, "%s: M=%d (slot, guide) pairs for %d slots (B <= M <= %d)", kWho, a->M, a->B,
                      kGmMax * kGmMax);
        return HICOM_OK;
    }
    static int check_item(const Args* a, int i) {
        HICOM_REQUIRE(a->q[i] >= 1 && a->q[i] <= kGmMax, HICOM_EUNSUP, "%s: item %d: Q=%d guides (1 <= Q <= %d per slot)", kWho, i, a->q[i], kGmMax);
        return HICOM_OK;
    }
    // (the logits' offsets -- counted in 16 floats, 32 rows per pass and tile -- and the context rows are ints on the device)
    static int check_totals(const Args* a, int wps) {
        long products = 0, ctx_rows = 0;
        for (int i = 0; i < a->items; ++i) {
            products += group_item_passes<MultiOf>(a, i) * 32 * (((long)a->tc[i] * a->H * a->W + 15) / 16);
            ctx_rows += a->q[i] * group_item_win(a, i, wps);
        }
        HICOM_REQUIRE(products < (1L << 27), HICOM_EUNSUP, "%s: too many token x guide products in one push", kWho);
        HICOM_REQUIRE(ctx_rows < (1L << 20), HICOM_EUNSUP, "%s: %ld window contexts over all pairs of one push (< 2^20)", kWho, ctx_rows);
        return HICOM_OK;
    }
    static int check_units(const Args* a) { return gm_check_pairs(kWho, a->pair0, a->q, 0, a->items, a->M); }

    static void write(GmItem& d, GmUnit* units, const GroupWalk& w) {
        d.tok0 = (int)w.tok; d.N = (int)w.N; d.T = w.T; d.win0 = (int)w.win; d.wins = (int)w.wins; d.slot0 = (int)w.slot; d.chunks = w.chunks;
        d.score_off = (int)w.score; d.Q = w.Q; d.ctx_row0 = (int)w.ctx_row; d.lrow0 = (int)w.row; d.rows = (int)(w.wins + w.nl); d.nl_count = (int)w.nl;
        for (long p = 0; p < w.passes; ++p)
            for (int c = 0; c < w.chunks; ++c) {
                GmUnit& u = *units++;
                u.item = w.i; u.tb = seg_tile_at(w.ntiles, c, w.chunks); u.te = seg_tile_at(w.ntiles, c + 1, w.chunks); u.pass = (int)p;
                u.slot = (int)(w.slot + 2 * p * w.chunks + c);
            }
    }

    static void uniform_guides(GmMergeParams& p, int Q) { p.u_Q = Q; }
    static int check_fold_shape(const char* who, int items, int M, int nparts, int rows, int Q, int E, int Tc, int H, int W) {
        HICOM_REQUIRE(Q >= 1 && Q <= kGmMax, HICOM_EUNSUP, "%s: Q=%d guides (1 <= Q <= %d per slot)", who, Q, kGmMax);
        HICOM_REQUIRE(items >= 1 && items <= kGmMax && M >= 1 && M <= kGmMax * kGmMax && nparts >= 1 && nparts <= kSegMaxChunks && rows >= 1 && rows <= 16 && E > 0 &&
                          E % 4 == 0 && Tc > 0 && H > 0 && W > 0 && (long)Tc * H * W < (1L << 27) / (kGmMax * kGmMax), HICOM_EINVAL,
                      "%s: bad shape (items=%d M=%d nparts=%d rows=%d E=%d Tc=%d H=%d W=%d)", who, items, M, nparts, rows, E, Tc, H, W);
        return HICOM_OK;
    }
    static int check_fold_units(const char* who, const int32_t* pair0, int Q, int items, int M) { return gm_check_pairs(who, pair0, nullptr, Q, items, M); }
};

typedef MultiOf<MultiNames> Multi;

// The logits form: Multi with its front replaced -- launch 1 is gm_local_logits_kernel on the caller's logits.  No region, no
// requirement on the tuple: the workspace, its size function, the prepare call and the tables are Multi's.  (MultiOf<LogitsNames> is a
// second instantiation for the sake of the entry's name in the messages: its `local` and kFoldWho are never used, and group_push's
// once-per-process hipFuncSetAttribute on the one stream kernel runs once more for it.)
struct LogitsNames {
    static constexpr const char *kWho = "compressor_stream_group_multi_push_logits", *kFoldWho = "stream_group_multi_merge_fold";
};

struct MultiLogits : MultiOf<LogitsNames> {
    const float* logits;     // f32 [max Q_i][q_stride], hicom_head_scores_ragged_fwd's layout over the tick's stack
    long q_stride;
    MultiLogits(const float* logits_, long q_stride_) : logits(logits_), q_stride(q_stride_) {}

    int check_push(const Args*, const GroupLayout& l) const {
        HICOM_REQUIRE(logits && (uintptr_t)logits % 4 == 0, HICOM_EINVAL, "%s: local_logits is f32 [max Q_i][sum Tc_i H W]", kWho);
        HICOM_REQUIRE(q_stride >= l.tokens, HICOM_EINVAL, "%s: q_stride=%ld floats between the guides' logit planes of %ld tokens", kWho, q_stride, l.tokens);
        return HICOM_OK;
    }
    int front(const Args* a, const GroupLayout& l, const uint16_t*, const GroupPush&) const {
        const char* ws = (const char*)a->ws;
        const hicom_axis ay{a->H, a->ks, a->H / a->ks, a->H / a->ks}, ax{a->W, a->ks, a->W / a->ks, a->W / a->ks};
        HICOM_LAUNCH(gm_local_logits_kernel<3>, dim3((unsigned)((l.windows + 3) / 4)), dim3(256), 0, (hipStream_t)a->stream, (const uint16_t*)a->ff, logits, q_stride,
                     (const GmItem*)(ws + l.items), (const int*)(ws + l.win_item), ay, ax, (int)a->kt, (int)l.windows, a->l_scale, (_Float16*)(ws + l.ctx16));
        return seg_check_launch(kWho, "local stage");
    }
};

}  // namespace

extern "C" int64_t hicom_compressor_stream_group_multi_workspace_bytes(const hicom_stream_group_multi_push_args* a) { return group_workspace_bytes<Multi>(a); }
extern "C" int hicom_compressor_stream_group_multi_prepare(const hicom_stream_group_multi_push_args* a) { return group_prepare<Multi>(a); }
extern "C" int hicom_compressor_stream_group_multi_push(const hicom_stream_group_multi_push_args* a) { return group_push<Multi>(a); }

// The logits form: a->fe is not read (an address left in the block by a keyed push is not looked at); a->guide stays the group's block.
extern "C" int hicom_compressor_stream_group_multi_push_logits(const hicom_stream_group_multi_push_args* a, const float* local_logits, int64_t q_stride) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "%s: NULL arguments", LogitsNames::kWho);
    hicom_stream_group_multi_push_args keyless = *a;
    keyless.fe = nullptr;
    return group_push<MultiLogits>(&keyless, MultiLogits(local_logits, (long)q_stride));
}

// The merge + fold kernel alone: `items` chunks of Tc frames with Q guides each; item i's partials in the slots [i S, (i + 1) S), S = 2 passes
// nparts, ordered [pass][row group][chunk]; its logits [32 passes][ceil16(Tc H W)] at scores + i 32 passes ceil16(Tc H W); folded into the state
// rows pair0[i] rows + R, R < rows Q.
extern "C" int hicom_stream_group_multi_merge_fold_fwd(const float* part_m, const float* part_l, const float* part_acc, const float* scores, int32_t items,
                                                       int32_t nparts, int32_t rows, int32_t Q, int32_t E, int32_t Tc, int32_t H, int32_t W, const float* pe,
                                                       int32_t P, int32_t y_index0, int32_t x_index0, const int32_t* pair0, const int32_t* t0, int32_t M,
                                                       float* state_ml, float* state_acc, void* stream) {
    return group_merge_fold<Multi>(part_m, part_l, part_acc, scores, items, nparts, rows, Q, E, Tc, H, W, pe, P, y_index0, x_index0, pair0, t0, M, state_ml, state_acc,
                                   stream);
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

// ---- the k / v adaptor recipe ----------------------------------------------------------------------------------------------
// The adaptors sit on the local stage only and the adaptor MLPs know neither the guide nor the slot, so a push differs in its front alone:
// hicom_clip_adapt_prepare_fwd over the tick's sum N_i STACKED tokens (layer 1 and layer 2, one GEMM pair per layer with both adaptors)
// into fp16 planes ky / vy [sum N_i, E] that live for that push, then gm_local_adapt_kernel; launches 2-6 of the plain push follow
// unchanged: eight launches.  The planes and the hidden planes of layer 1 are regions of the plan's ONE workspace, behind `loc`.
namespace {

struct AdaptNames {
    static constexpr const char *kWho = "compressor_stream_group_adapt", *kFoldWho = "stream_group_multi_merge_fold";
};

struct Adapt : MultiOf<AdaptNames> {
    const hicom_stream_group_adapt_push_args* x;
    explicit Adapt(const hicom_stream_group_adapt_push_args* x_) : x(x_) {}
    SegAdapt adaptors() const { return SegAdapt{&x->ak, &x->av, x->alpha_dt, x->eps}; }
    enum { kKy, kVy, kHid };                 // l.front[]: the two planes, the hidden planes of layer 1 (hicom_clip_adapt_prepare_workspace_bytes)

    int check_shape(const Args* a, long tokens) const {
        const SegAdapt ad = adaptors();
        return seg_adapt_check(kWho, &ad, tokens, a->E);
    }
    template <class Take>
    void regions(const Args* a, GroupLayout& l, Take&& take) const {
        const SegAdapt ad = adaptors();
        const long plane = l.tokens * a->E * 2;
        const int64_t hid = hicom_clip_adapt_prepare_workspace_bytes(l.tokens, a->E, &x->ak, &x->av);
        l.front[kKy] = ad.k() ? take(plane) : 0;
        l.front[kVy] = ad.v() ? take(plane) : 0;
        l.front[kHid] = take(hid > 0 ? hid : 0);
    }
    const void* key_x(const Args* a) const { return a->fe ? a->fe : a->ff; }      // (no frames_embed: the k adaptor reads frames_feature, as the keys do)
    int check_push(const Args* a, const GroupLayout& l) const {
        const SegAdapt ad = adaptors();
        const int st = seg_adapt_check_weights(kWho, &ad);
        if (st != HICOM_OK) return st;
        char* ws = (char*)a->ws;
        return clip_adapt_prepare_args_check(key_x(a), a->ff, l.tokens, a->E, &x->ak, &x->av, ad.k() ? ws + l.front[kKy] : nullptr,
                                             ad.v() ? ws + l.front[kVy] : nullptr, ws + l.front[kHid], l.total - l.front[kHid], nullptr);
    }
    int front(const Args* a, const GroupLayout& l, const uint16_t* kx, const GroupPush& push) const {
        const SegAdapt ad = adaptors();
        char* ws = (char*)a->ws;
        // 1-2: y = MLP(x) of the adapted streams over the whole stack
        const int st = hicom_clip_adapt_prepare_fwd(kx, a->ff, l.tokens, a->E, &x->ak, &x->av, ad.k() ? ws + l.front[kKy] : nullptr,
                                                    ad.v() ? ws + l.front[kVy] : nullptr, ws + l.front[kHid], l.total - l.front[kHid], a->stream);
        if (st != HICOM_OK) return st;
        // 3: local stage on the planes
        SegAdaptLayout planes;
        planes.ky = l.front[kKy]; planes.vy = l.front[kVy];
        const hicom_axis ay{a->H, a->ks, a->H / a->ks, a->H / a->ks}, ax{a->W, a->ks, a->W / a->ks, a->W / a->ks};
        HICOM_LAUNCH(gm_local_adapt_kernel<3>, dim3((unsigned)((l.windows + 3) / 4)), dim3(256), 0, (hipStream_t)a->stream, kx, (const uint16_t*)a->ff,
                     (const uint16_t*)a->guide, seg_adapt_params(ad, ws, planes), (const GmItem*)(ws + l.items), (const int*)(ws + l.win_item), ay, ax,
                     (int)a->kt, (int)l.windows, 0, 0, a->l_scale, (_Float16*)(ws + l.ctx16), push);
        return seg_check_launch(kWho, "local stage");
    }
};

}  // namespace

extern "C" int64_t hicom_compressor_stream_group_adapt_workspace_bytes(const hicom_stream_group_adapt_push_args* x) {
    HICOM_REQUIRE(x, HICOM_EINVAL, "%s: NULL arguments", Adapt::kWho);
    return group_workspace_bytes<Adapt>(&x->base, Adapt(x));
}
extern "C" int hicom_compressor_stream_group_adapt_prepare(const hicom_stream_group_adapt_push_args* x) {
    HICOM_REQUIRE(x, HICOM_EINVAL, "%s: NULL arguments", Adapt::kWho);
    return group_prepare<Adapt>(&x->base, Adapt(x));
}
extern "C" int hicom_compressor_stream_group_adapt_push(const hicom_stream_group_adapt_push_args* x) {
    HICOM_REQUIRE(x, HICOM_EINVAL, "%s: NULL arguments", Adapt::kWho);
    return group_push<Adapt>(&x->base, Adapt(x));
}

// Launch 3 of that push alone: `items` chunks of Tc frames with Q guides each, packed one behind the other -- item i's tokens (and plane
// rows) at i Tc H W, its contexts at ctx_f16 + i Q windows E, pair-major within the item -- with the guide rows pair0[i] .. pair0[i] + Q of
// guide [M][E].  ky / vy: the planes of the whole stack, one of them may be NULL.
extern "C" int hicom_stream_group_local_adapt_fwd(const void* key, const void* value, const void* guide, const void* ky, const void* vy,
                                                  const hicom_seg_adaptor* ak, const hicom_seg_adaptor* av, int32_t alpha_dt, float eps, int32_t items,
                                                  int32_t Q, int32_t Tc, int32_t H, int32_t W, int32_t E, int32_t kt, int32_t ks, float scale,
                                                  const int32_t* pair0, int32_t M, void* ctx_f16, void* stream) {
    constexpr const char* who = "stream_group_local_adapt";
    HICOM_REQUIRE(pair0, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE(items >= 1 && items <= kGmMax && M >= 1 && M <= kGmMax * kGmMax, HICOM_EINVAL, "%s: bad shape (items=%d M=%d)", who, items, M);
    // the checks of the one-clip launch on an item's shape: pointers, Q, the window partition, E, alignment, the planes and their adaptors
    int st = multi_guide_local_adapt_args_check(key, value, guide, ky, vy, ak, av, alpha_dt, Q, Tc, H, W, E, kt, ks, ctx_f16);
    if (st != HICOM_OK) return st;
    const long N = (long)Tc * H * W, wins = (long)(Tc / kt) * (H / ks) * (W / ks);
    // (item offsets are ints on the device, as in a push)
    HICOM_REQUIRE(N * items < (1L << 27) && wins * Q * items < (1L << 20), HICOM_EUNSUP, "%s: too many tokens in one call", who);
    st = gm_check_pairs(who, pair0, nullptr, Q, items, M);
    if (st != HICOM_OK) return st;
    SegAdaptParams p;
    p.ky = (const _Float16*)ky; p.kgamma = (const uint16_t*)ak->gamma; p.kbeta = (const uint16_t*)ak->beta; p.kalpha = ak->alpha;
    p.vy = (const _Float16*)vy; p.vgamma = (const uint16_t*)av->gamma; p.vbeta = (const uint16_t*)av->beta; p.valpha = av->alpha;
    p.alpha_f32 = alpha_dt == HICOM_DT_F32;
    p.eps = eps;
    const hicom_axis ay{H, ks, H / ks, H / ks}, ax{W, ks, W / ks, W / ks};
    const long nwin = wins * items;
    HICOM_LAUNCH(gm_local_adapt_kernel<3>, dim3((unsigned)((nwin + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)key, (const uint16_t*)value,
                 (const uint16_t*)guide, p, (const GmItem*)nullptr, (const int*)nullptr, ay, ax, (int)kt, (int)nwin, (int)Tc, (int)Q, scale, (_Float16*)ctx_f16,
                 group_push_values(pair0, pair0, nullptr, items));       // (this launch reads pair0 alone: the frame offsets are not its business)
    return seg_check_launch(who, "local stage");
}
