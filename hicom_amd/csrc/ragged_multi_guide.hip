// Ragged multi-guide compressor step: B items of unequal length and mixed modality, item i with its own Q_i instructions, in one call
// (DESIGN.md §3.9).  A PAIR is one (item, guide); pairs are numbered item-major, then guide-major, M = sum Q_i of them.
//
// Behind the two launches that read tokens a pair is just an item of the ragged step, so the launch sequence, the workspace regions and
// the common checks are segment_host.hpp's with M pairs as its items (twelve launches, whatever B, the Q_i and the mix are):
//    1-2  q_proj and the fold with M rows: the nh folded rows of pair p are rows nh p .. nh p + nh - 1
//    3    rmg_local_kernel: one wave per window of the STACKED tensor (window -> item lookup as in ragged.hip); the wave walks its item's
//         guides in groups of kGuideGroup (multi_window.hpp: multi_window_guides_ctx16), so every key row and every value row is loaded
//         once per group; fp16 contexts go out pair-major: pair p of item i owns rows [ctx_row0_p, + windows_i)
//    4    rmg_stream_kernel: stream_segment (stream_body.hpp: the one body of the four-wave stream machine) with two row groups, 32 densely packed
//         folded rows of ONE item per workgroup, one workgroup per work unit {item, first tile, last tile, row pass, partial-state slot}
//    5    merge_segments (segment_item.hpp) per (pair, head)
//    6-11 the global tail with M rows, the local readout as one GEMM pair over all pairs' window contexts
//   12    place_row with item = pair, the layout integers those of the pair's item
// Only launches 3 and 4 know that several pairs alias one item's tokens.  This file holds the kernels, the table region
// (hicom_compressor_ragged_multiguide_prepare derives it on the host, once per plan; hicom_amd/ragged_multi_guide.py: plan_tables restates
// it) and the step's own limits; the walk over the item descriptors (per-item requirements, chunk share by tiles x passes, tile ranges,
// table upload) is segment_host.hpp's, shared with ragged.hip.
//
// Row space of an item: guide q owns rows nh q .. nh q + nh - 1, rows_i = nh Q_i in all; pass p of the stream carries rows [32 p, 32 p + 32),
// its row group g (waves 4 g .. 4 g + 3) rows [32 p + 16 g, + 16).  Partial-state slots (16 rows each) are ordered
// [item][pass][row group][chunk]: every 16-row group has its chunks in consecutive slots, which is what merge_segments walks.
//
// Prepared clips (hicom_compressor_clips_multiguide_*): the same step over B clips that live at their own addresses, each
// with its own y planes for the k / v adaptor recipe.  Launches 3 and 4 are clips_local_kernel / clips_local_adapt_kernel and
// clips_stream_kernel, which take an item's base pointers from a [B][4] device table the caller fills per call; checks, layout, table
// region and every other launch are the functions of this file on the base block.
//
// Logits form: hicom_compressor_ragged_multiguide_logits_fwd is the plain sequence with launch 3 replaced by
// rmg_local_logits_kernel, which takes every pair's local logits precomputed (hicom_head_scores_ragged_fwd) and reads the value rows only.
// Same launch count, same workspace, same tables; frames_embed is not read.
// The table entries (RmgItem, RmgPair, RmgUnit), the limits, rmg_check and rmg_layout are ragged_multi_guide_host.hpp's, shared with the
// step's training surface (ragged_multi_guide_train.hip).
#include "ragged_multi_guide_host.hpp"

namespace hicom {

// ---- 3: local stage, one wave per window of the stacked tensor, the item's guides in groups of kGuideGroup ----
template <int NV>
__global__ __launch_bounds__(256) void rmg_local_kernel(const uint16_t* key, const uint16_t* value, const uint16_t* guide, const RmgItem* items,
                                                        const int* win_item, hicom_axis ay, hicom_axis ax, int nwin, float scale, _Float16* ctx16) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const RmgItem it = items[win_item[win]];
    const hicom_axis at{it.T, it.kt, it.T / it.kt, it.T / it.kt};
    const int wi = (it.T / it.kt) * ay.nwin * ax.nwin;          // windows of the item = context rows of one pair
    const WindowGeom g(at, ay, ax, win - it.win0);
    const long first = (long)it.tok0 * D;
    multi_window_guides_ctx16<NV>(key + first, value + first, guide, it.pair0, it.Q, g, lane, scale,
                                  ctx16 + ((long)it.ctx_row0 + (win - it.win0)) * D, (long)wi * D);
}

// The logits form of launch 3: the same wave -> window -> item map with the local logits given
// (multi_window.hpp: multi_window_guides_logits_ctx16).  logits f32 [Qmax][q_stride]: guide q of item i at q q_stride + tok0_i + n, the
// layout hicom_head_scores_ragged_fwd writes; planes q >= Q_i of an item's columns are not read.  No key row is read.
template <int NV>
__global__ __launch_bounds__(256) void rmg_local_logits_kernel(const uint16_t* value, const float* logits, long q_stride, const RmgItem* items,
                                                               const int* win_item, hicom_axis ay, hicom_axis ax, int nwin, float scale, _Float16* ctx16) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const RmgItem it = items[win_item[win]];
    const hicom_axis at{it.T, it.kt, it.T / it.kt, it.T / it.kt};
    const int wi = (it.T / it.kt) * ay.nwin * ax.nwin;
    const WindowGeom g(at, ay, ax, win - it.win0);
    multi_window_guides_logits_ctx16<NV>(value + (long)it.tok0 * D, logits + it.tok0, q_stride, it.Q, g, lane, scale,
                                         ctx16 + ((long)it.ctx_row0 + (win - it.win0)) * D, (long)wi * D);
}

// ---- 4: segmented many-row stream, stream_segment (stream_body.hpp) with two row groups: 32 densely packed rows of ONE item per
// workgroup, so the item's tokens come from HBM once per 32 folded rows ----
struct RmgStreamParams {
    SegStreamParams c;
    const uint16_t* x;      // [sum N_i][E]
    float* scores;
    const RmgUnit* units;
    const RmgItem* items;
};

template <int NB>
__global__ __launch_bounds__(512, 1) void rmg_stream_kernel(RmgStreamParams p) {
    constexpr int E = NB * 128;
    const RmgUnit u = p.units[blockIdx.x];
    const RmgItem it = p.items[u.item];
    stream_segment<NB, 2>(p.c, p.x + (long)it.tok0 * E, it.N, u.tb, u.te, 32 * u.pass, p.c.rows * it.Q, (long)it.pair0 * p.c.rows,
                          p.scores + (long)it.score_off * 16, (long)((it.N + 15) / 16 * 16), (long)u.slot, it.chunks);
}

// ---- 3 and 4 over PREPARED CLIPS: every item lives at its own addresses ----
// One row of the caller's device table per item (hicom_compressor_clips_multiguide_args.item_ptrs): where the item's key tokens, value
// tokens and y planes begin.  ky / vy are NULL for a stream without adaptor.  The kernels only read through these pointers.
struct ClipPtrs {
    const uint16_t* key_x;      // frames_embed, or frames_feature without it: [N_i][E]
    const uint16_t* value_x;    // frames_feature [N_i][E]: the values of the local stage, the tokens of the global stream
    const _Float16* ky;         // MLP_k(key_x) fp16 [N_i][E]
    const _Float16* vy;         // MLP_v(value_x) fp16 [N_i][E]
};
static_assert(sizeof(ClipPtrs) == 32, "a table row is four 64-bit addresses");

// rmg_local_kernel with the item's base pointers from the table instead of key + tok0 D: the window list, the wave -> window map, the
// device function and the pair-major context rows are the same, so a plain-recipe call has the bits of the ragged multi-guide step.
// The lookups are wave-uniform (win is); nothing is stored through what they return.
template <int NV>
__global__ __launch_bounds__(256) void clips_local_kernel(const ClipPtrs* clips, const uint16_t* guide, const RmgItem* items, const int* win_item,
                                                          hicom_axis ay, hicom_axis ax, int nwin, float scale, _Float16* ctx16) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const int item = win_item[win];
    const RmgItem it = items[item];
    const ClipPtrs c = clips[item];
    const hicom_axis at{it.T, it.kt, it.T / it.kt, it.T / it.kt};
    const int wi = (it.T / it.kt) * ay.nwin * ax.nwin;
    const WindowGeom g(at, ay, ax, win - it.win0);
    multi_window_guides_ctx16<NV>(c.key_x, c.value_x, guide, it.pair0, it.Q, g, lane, scale, ctx16 + ((long)it.ctx_row0 + (win - it.win0)) * D,
                                  (long)wi * D);
}

// The same for the k / v adaptor recipe: the window of multi_guide_local_adapt_kernel (multi_window.hpp: groups of kAdaptGuideGroup guides)
// on the item's own tokens and planes.  ad: gamma / beta / alpha / eps of the call; its ky / vy are replaced by the item's.
template <int NV>
__global__ __launch_bounds__(256) void clips_local_adapt_kernel(const ClipPtrs* clips, const uint16_t* guide, SegAdaptParams ad, const RmgItem* items,
                                                                const int* win_item, hicom_axis ay, hicom_axis ax, int nwin, float scale,
                                                                _Float16* ctx16) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const int item = win_item[win];
    const RmgItem it = items[item];
    const ClipPtrs c = clips[item];
    ad.ky = c.ky;
    ad.vy = c.vy;
    const hicom_axis at{it.T, it.kt, it.T / it.kt, it.T / it.kt};
    const int wi = (it.T / it.kt) * ay.nwin * ax.nwin;
    const WindowGeom g(at, ay, ax, win - it.win0);
    multi_window_guides_adapt_ctx16<NV, kAdaptGuideGroup>(c.key_x, c.value_x, ad, guide, it.pair0, it.Q, g, lane, scale,
                                                          ctx16 + ((long)it.ctx_row0 + (win - it.win0)) * D, (long)wi * D);
}

// rmg_stream_kernel with the unit's tokens at the item's value_x: work units, passes, slots and scores are the same
struct ClipsStreamParams {
    SegStreamParams c;
    const ClipPtrs* clips;
    float* scores;
    const RmgUnit* units;
    const RmgItem* items;
};

template <int NB>
__global__ __launch_bounds__(512, 1) void clips_stream_kernel(ClipsStreamParams p) {
    const RmgUnit u = p.units[blockIdx.x];
    const RmgItem it = p.items[u.item];
    stream_segment<NB, 2>(p.c, p.clips[u.item].value_x, it.N, u.tb, u.te, 32 * u.pass, p.c.rows * it.Q, (long)it.pair0 * p.c.rows,
                          p.scores + (long)it.score_off * 16, (long)((it.N + 15) / 16 * 16), (long)u.slot, it.chunks);
}

// ---- 5: merge per (pair, head), grid = (heads, M), LDS sized for the longest item ----
struct RmgMergeParams {
    SegMergeParams c;
    const float* scores;
    const RmgItem* items;
    const RmgPair* pairs;
    int rows;               // heads
    float* ctx;             // [M * rows][E]
};

__global__ __launch_bounds__(256) void rmg_merge_kernel(RmgMergeParams p) {
    extern __shared__ float ms[];
    const int h = blockIdx.x, pair = blockIdx.y;
    const RmgPair pr = p.pairs[pair];
    const RmgItem it = p.items[pr.item];
    const int R = pr.q * p.rows + h;                            // the head's row in the item's row space
    const long stride = (it.N + 15) / 16 * 16;
    merge_segments(p.c, ms, R & 15, threadIdx.x, it.T, it.chunks, (long)it.slot0 + (long)(R >> 4) * it.chunks,
                   p.scores + (long)it.score_off * 16 + R * stride, p.ctx + ((long)pair * p.rows + h) * p.c.E);
}

// ---- 12: placement, one output row per workgroup over all pairs' rows ----
struct RmgPlaceParams {
    SegPlaceParams c;
    const RmgItem* items;
    const RmgPair* pairs;
    const int* row_pair;
    long ldo;
};

__global__ __launch_bounds__(128) void rmg_place_kernel(RmgPlaceParams p) {
    const long row = blockIdx.x;
    const int pair = p.row_pair[row];
    const RmgPair pr = p.pairs[pair];
    const RmgItem it = p.items[pr.item];
    place_row(p.c, row - pr.row0, row * p.ldo, pair, pr.ctx_row0, it.nl_group, it.nl_count, it.global_row0, it.nl_first, it.nl_step);
}

}  // namespace hicom

using namespace hicom;
using namespace hicom_host;

namespace {

int rmg_prepare(const Args* a) {
    int st = rmg_check(a);
    if (st != HICOM_OK) return st;
    const RmgLayout l = rmg_layout(a);
    st = seg_check_ws(kWho, a, l.s.total);
    if (st != HICOM_OK) return st;
    std::vector<int> tab((size_t)(l.table_bytes / 4), 0);
    RmgItem* items = reinterpret_cast<RmgItem*>(tab.data() + l.items / 4);
    RmgUnit* units = reinterpret_cast<RmgUnit*>(tab.data() + l.units / 4);
    int* win_item = tab.data() + l.win_item / 4;
    RmgPair* pairs = reinterpret_cast<RmgPair*>(tab.data() + l.pairs / 4);
    int* row_pair = tab.data() + l.row_pair / 4;
    const long HW = (long)a->H * a->W;
    const int ncu = a->chunks > 0 ? 0 : num_cus();
    long tok = 0, win = 0, row = 0, score = 0, slot = 0, unit = 0, pair = 0, ctx_row = 0;
    for (int i = 0; i < a->B; ++i) {
        const hicom_ragged_item& h = a->items[i];
        const long N = h.T * HW, w = item_windows(h, l.wps), ntiles = (N + 15) / 16, passes = item_passes(a, i);
        const int Q = a->guide_counts[i], chunks = seg_share_chunks(ntiles, l.work_sum, a->chunks, ncu);
        RmgItem& d = items[i];
        d.tok0 = (int)tok; d.N = (int)N; d.T = h.T; d.kt = h.kt; d.win0 = (int)win; d.slot0 = (int)slot; d.chunks = chunks;
        d.score_off = (int)score; d.pair0 = (int)pair; d.Q = Q; d.ctx_row0 = (int)ctx_row; d.global_row0 = (int)(w + h.nl_count);
        d.nl_group = h.nl_group; d.nl_count = h.nl_count; d.nl_first = h.nl_first; d.nl_step = h.nl_step > 0 ? h.nl_step : 1;
        for (long p = 0; p < passes; ++p)
            for (int c = 0; c < chunks; ++c) {
                RmgUnit& u = units[unit++];
                u.item = i; u.tb = seg_tile_at(ntiles, c, chunks); u.te = seg_tile_at(ntiles, c + 1, chunks); u.pass = (int)p;
                u.slot = (int)(slot + 2 * p * chunks + c);
            }
        for (long k = 0; k < w; ++k) win_item[win + k] = i;
        const long rows = w + h.nl_count + h.n_global_rows;
        for (int q = 0; q < Q; ++q) {
            RmgPair& pr = pairs[pair + q];
            pr.item = i; pr.q = q; pr.ctx_row0 = (int)(ctx_row + q * w); pr.row0 = (int)(row + q * rows);
            for (long k = 0; k < rows; ++k) row_pair[row + q * rows + k] = (int)(pair + q);
        }
        tok += N; win += w; row += Q * rows; score += passes * kPassRows * ntiles; slot += 2 * passes * chunks; pair += Q; ctx_row += Q * w;
    }
    return seg_upload_tables(kWho, a, tab.data(), l.table_bytes);
}

// the clips step (hicom_compressor_clips_multiguide_fwd): the caller's device table and the local stage's adaptor parameters (their ky / vy
// come from the table per item)
struct ClipsCall {
    const ClipPtrs* ptrs;
    bool adapted;
    SegAdaptParams ad;
};

// the local logits of the logits step (hicom_compressor_ragged_multiguide_logits_fwd): f32 [max Q_i][q_stride], guide q of item i at
// q q_stride + tok0_i + n; p NULL: the keyed forms
struct LocalLogits {
    const float* p;
    long q_stride;
};

// the four launches that look their pair or item up in the table region (segment_host.hpp: seg_step)
struct PairItems {
    const Args* a;
    const RmgLayout& l;
    const ClipsCall* clips;     // the items are prepared clips at their own addresses; NULL: the stacked tensor a->ff / a->fe
    LocalLogits logits;         // the logits form on the stacked tensor: no key row is read
    char* ws() const { return (char*)a->ws; }
    hipStream_t s() const { return (hipStream_t)a->stream; }
    const RmgItem* items() const { return (const RmgItem*)(ws() + l.items); }
    const RmgPair* pairs() const { return (const RmgPair*)(ws() + l.pairs); }

    int local(const uint16_t* key_x, const SegAdaptParams*) const {
        const hicom_axis ay{a->H, a->ks, a->H / a->ks, a->H / a->ks}, ax{a->W, a->ks, a->W / a->ks, a->W / a->ks};
        const dim3 grid((unsigned)((l.item_windows + 3) / 4));
        const int* win_item = (const int*)(ws() + l.win_item);
        _Float16* ctx16 = (_Float16*)(ws() + l.s.ctx16);
        if (logits.p)
            HICOM_LAUNCH(rmg_local_logits_kernel<3>, grid, dim3(256), 0, s(), (const uint16_t*)a->ff, logits.p, logits.q_stride, items(), win_item, ay, ax,
                         (int)l.item_windows, a->l_scale, ctx16);
        else if (clips && clips->adapted)
            HICOM_LAUNCH(clips_local_adapt_kernel<3>, grid, dim3(256), 0, s(), clips->ptrs, (const uint16_t*)a->guide, clips->ad, items(), win_item, ay, ax,
                         (int)l.item_windows, a->l_scale, ctx16);
        else if (clips)
            HICOM_LAUNCH(clips_local_kernel<3>, grid, dim3(256), 0, s(), clips->ptrs, (const uint16_t*)a->guide, items(), win_item, ay, ax,
                         (int)l.item_windows, a->l_scale, ctx16);
        else
            HICOM_LAUNCH(rmg_local_kernel<3>, grid, dim3(256), 0, s(), key_x, (const uint16_t*)a->ff, (const uint16_t*)a->guide, items(), win_item, ay, ax,
                         (int)l.item_windows, a->l_scale, ctx16);
        return seg_check_launch(kWho, "local stage");
    }

    int stream_clips(const SegStreamParams& c) const {
        ClipsStreamParams p;
        p.c = c;
        p.clips = clips->ptrs;
        p.scores = (float*)(ws() + l.s.scores);
        p.units = (const RmgUnit*)(ws() + l.units); p.items = items();
        static bool attr_set = false;
        if (!attr_set) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(clips_stream_kernel<9>), hipFuncAttributeMaxDynamicSharedMemorySize, seg_stream_smem(2));
            attr_set = true;
        }
        HICOM_LAUNCH(clips_stream_kernel<9>, dim3((unsigned)l.nunits), dim3(512), seg_stream_smem(2), s(), p);
        return seg_check_launch(kWho, "global stream");
    }

    int stream(const SegStreamParams& c) const {
        if (clips) return stream_clips(c);
        RmgStreamParams p;
        p.c = c;
        p.x = (const uint16_t*)a->ff;
        p.scores = (float*)(ws() + l.s.scores);
        p.units = (const RmgUnit*)(ws() + l.units); p.items = items();
        static bool attr_set = false;
        if (!attr_set) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(rmg_stream_kernel<9>), hipFuncAttributeMaxDynamicSharedMemorySize, seg_stream_smem(2));
            attr_set = true;
        }
        HICOM_LAUNCH(rmg_stream_kernel<9>, dim3((unsigned)l.nunits), dim3(512), seg_stream_smem(2), s(), p);
        return seg_check_launch(kWho, "global stream");
    }

    int merge(const SegMergeParams& c) const {
        RmgMergeParams p;
        p.c = c;
        p.scores = (const float*)(ws() + l.s.scores);
        p.items = items(); p.pairs = pairs(); p.rows = a->nh;
        p.ctx = (float*)(ws() + l.s.ctxg);
        HICOM_LAUNCH(rmg_merge_kernel, dim3((unsigned)a->nh, (unsigned)l.M), dim3(256), (size_t)seg_merge_smem(l.max_T, a->H, a->W), s(), p);
        return seg_check_launch(kWho, "merge");
    }

    int place(const SegPlaceParams& c) const {
        RmgPlaceParams p;
        p.c = c;
        p.items = items(); p.pairs = pairs(); p.row_pair = (const int*)(ws() + l.row_pair); p.ldo = a->ldo;
        HICOM_LAUNCH(rmg_place_kernel, dim3((unsigned)l.rows), dim3(128), 0, s(), p);
        return seg_check_launch(kWho, "placement");
    }
};

// clips: the items are prepared clips at their own addresses (clips_fwd); every check runs as for the stacked tensor, only a->ff / a->fe
// are not looked at.  logits: the logits form (the stacked tensor only): launch 3 is rmg_local_logits_kernel, a->fe is not looked at either.
int rmg_fwd(const Args* a, const ClipsCall* clips = nullptr, LocalLogits logits = LocalLogits{nullptr, 0}) {
    int st = rmg_check(a);
    if (st != HICOM_OK) return st;
    Args keyless;
    if (logits.p) {
        HICOM_REQUIRE(!clips, HICOM_EINVAL, "%s: the logits form reads the stacked tensor", kWho);
        long tokens = 0;
        int q_max = 0;
        for (int i = 0; i < a->B; ++i) {
            tokens += (long)a->items[i].T * a->H * a->W;
            q_max = a->guide_counts[i] > q_max ? a->guide_counts[i] : q_max;
        }
        HICOM_REQUIRE(q_max == 1 || logits.q_stride >= tokens, HICOM_EINVAL, "%s: q_stride=%ld floats between the guides' logit planes of %ld tokens", kWho,
                      logits.q_stride, tokens);
        keyless = *a;
        keyless.fe = nullptr;
        a = &keyless;
    }
    const RmgLayout l = rmg_layout(a);
    st = seg_check_fwd(kWho, a, nullptr, l.s.total, clips != nullptr);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->ldo >= a->hidden, HICOM_EINVAL, "compressor_ragged_multiguide: output layout");
    for (int i = 0; i < a->B; ++i)
        HICOM_REQUIRE(a->items[i].nl_count == 0 || a->newline, HICOM_EINVAL,
                      "compressor_ragged_multiguide: item %d has newline rows and there is no newline token", i);
    Args pairs = *a;            // the shared host sees the pairs as its items: M guide rows, M global tokens, all pairs' window contexts
    pairs.B = l.M;
    return seg_step(&pairs, nullptr, l.s, PairItems{a, l, clips, logits});
}

// ---- prepared clips, Q_i guides each (hicom_compressor_clips_multiguide_*) -----------------------------------------------------------------
constexpr const char* kWhoClips = "compressor_clips_multiguide";
typedef hicom_compressor_clips_multiguide_args ClipsArgs;

// what the block adds to the checks of its base block (which run behind these, under the base step's name)
int clips_check(const ClipsArgs* a) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "%s: NULL arguments", kWhoClips);
    HICOM_REQUIRE(!a->base.ff && !a->base.fe, HICOM_EINVAL, "%s: the clips' tokens come through item_ptrs: base.ff and base.fe must be NULL", kWhoClips);
    if (a->ak.w0 || a->av.w0)
        HICOM_REQUIRE(a->alpha_dt == HICOM_DT_BF16 || a->alpha_dt == HICOM_DT_F32, HICOM_EINVAL, "%s: alpha dtype %d (bf16 | f32)", kWhoClips, a->alpha_dt);
    return rmg_check(&a->base);
}

int clips_fwd(const ClipsArgs* a) {
    int st = clips_check(a);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->item_ptrs && (uintptr_t)a->item_ptrs % 16 == 0, HICOM_EINVAL, "%s: item_ptrs is a 16-byte aligned DEVICE table [B][4]", kWhoClips);
    for (const hicom_seg_adaptor* s : {&a->ak, &a->av})
        if (s->w0) HICOM_REQUIRE(s->gamma && s->beta && s->alpha, HICOM_EINVAL, "%s: adaptor weights", kWhoClips);
    ClipsCall c;
    c.ptrs = (const ClipPtrs*)a->item_ptrs;
    c.adapted = a->ak.w0 || a->av.w0;
    c.ad.ky = nullptr; c.ad.kgamma = (const uint16_t*)a->ak.gamma; c.ad.kbeta = (const uint16_t*)a->ak.beta; c.ad.kalpha = a->ak.alpha;
    c.ad.vy = nullptr; c.ad.vgamma = (const uint16_t*)a->av.gamma; c.ad.vbeta = (const uint16_t*)a->av.beta; c.ad.valpha = a->av.alpha;
    c.ad.alpha_f32 = a->alpha_dt == HICOM_DT_F32;
    c.ad.eps = a->eps;
    return rmg_fwd(&a->base, &c);
}

}  // namespace

extern "C" int64_t hicom_compressor_ragged_multiguide_workspace_bytes(const hicom_compressor_ragged_multiguide_args* a) {
    const int st = rmg_check(a);
    if (st != HICOM_OK) return st;
    return rmg_layout(a).s.total;
}

extern "C" int hicom_compressor_ragged_multiguide_prepare(const hicom_compressor_ragged_multiguide_args* a) { return rmg_prepare(a); }

extern "C" int hicom_compressor_ragged_multiguide_fwd(const hicom_compressor_ragged_multiguide_args* a) { return rmg_fwd(a); }

// The logits form: a->fe is not read (the workspace, its size function and the prepare call are the keyed step's).
extern "C" int hicom_compressor_ragged_multiguide_logits_fwd(const hicom_compressor_ragged_multiguide_args* a, const float* local_logits, int64_t q_stride) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "%s: NULL arguments", kWho);
    HICOM_REQUIRE(local_logits && (uintptr_t)local_logits % 4 == 0, HICOM_EINVAL, "%s: local_logits is f32 [max Q_i][sum T_i H W]", kWho);
    return rmg_fwd(a, nullptr, LocalLogits{local_logits, (long)q_stride});
}

// The planes and the tokens are the caller's: the workspace and its table region are the ragged multi-guide step's for the base block.
extern "C" int64_t hicom_compressor_clips_multiguide_workspace_bytes(const hicom_compressor_clips_multiguide_args* a) {
    const int st = clips_check(a);
    if (st != HICOM_OK) return st;
    return rmg_layout(&a->base).s.total;
}

extern "C" int hicom_compressor_clips_multiguide_prepare(const hicom_compressor_clips_multiguide_args* a) {
    const int st = clips_check(a);
    if (st != HICOM_OK) return st;
    return rmg_prepare(&a->base);
}

extern "C" int hicom_compressor_clips_multiguide_fwd(const hicom_compressor_clips_multiguide_args* a) { return clips_fwd(a); }
