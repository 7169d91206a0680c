// Batched compressor step: B items of one shape (images or short clips) through a launch sequence whose length does not depend on B
// (twelve launches, fourteen with the k / v adaptors; the sequence, the workspace regions and the common checks: segment_host.hpp).
//
// What is this file's own is where a wave finds its item -- by a constant stride:
//   * local stage: kt | T, so no window crosses an item boundary: the [B T, H, W] stack is ONE window grid and window w reads the
//     guide row of item w / windows_per_item (batch_local_attn_kernel, batch_local_attn_adapt_kernel: one wave per window);
//   * global stage: batch_global_stream_kernel with blockIdx.y = item.  A workgroup walks a contiguous range of 16-token tiles of ONE
//     item (chunk blockIdx.x of `chunks`), so a partial state (m, l, ACC) never mixes tokens of two items; batch_merge_kernel merges the
//     chunks of each (item, head) row.  The stream itself is stream_segment (stream_body.hpp): the one body of the four-wave machine,
//     the same text hicom_global_stream_fwd's narrow kernel runs; this file holds only the wrapper that finds the item;
//   * placement: batch_place_kernel, output row / item_rows = item;
//   * the chunk policy (B x chunks fills the chip twice over) and the checks of the one item shape and its packed-row layout.
#include "segment_host.hpp"

namespace hicom {

// ---------------------------------------------------------------------------------------------------------------------------------
// Local stage: one wave per window of the stacked grid, the item's guide row as the query (segment_item.hpp: local_window_ctx16).
// ---------------------------------------------------------------------------------------------------------------------------------
template <int NV>
__global__ __launch_bounds__(256) void batch_local_attn_kernel(const uint16_t* key, const uint16_t* value, const uint16_t* guide,
                                                               hicom_axis at, hicom_axis ay, hicom_axis ax, int wpi, int nwin,
                                                               float scale, _Float16* ctx16) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (win >= nwin) return;
    const WindowGeom g(at, ay, ax, win);
    local_window_ctx16<NV>(key, value, guide + (long)(win / wpi) * D, g, lane, scale, ctx16 + (long)win * D);
}

// The same with the k / v adaptor blends fused into the row loads (segment_item.hpp: local_window_adapt_ctx16); ky / vy rows are indexed
// like the tokens of the stacked grid.
template <int NV>
__global__ __launch_bounds__(256) void batch_local_attn_adapt_kernel(const uint16_t* key, const uint16_t* value, const uint16_t* guide,
                                                                     SegAdaptParams ad, hicom_axis at, hicom_axis ay, hicom_axis ax, int wpi,
                                                                     int nwin, float scale, _Float16* ctx16) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const WindowGeom g(at, ay, ax, win);
    local_window_adapt_ctx16<NV>(key, ad.ky, value, ad.vy, ad, guide + (long)(win / wpi) * D, g, lane, scale, ctx16 + (long)win * D);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Segmented global stream: grid = (chunks, B), workgroup (part, item) walks chunk `part` of the item's tiles (stream_body.hpp:
// stream_segment, one row group, row0 = 0, every row of the item).
// ---------------------------------------------------------------------------------------------------------------------------------
struct BatchStreamParams {
    SegStreamParams c;
    const uint16_t* x;      // [B][N][E]
    int N;                  // tokens per item
    int ntiles;             // 16-token tiles per item
    float* scores;          // [B][16][score_stride]
    long score_stride;
};

template <int NB>
__global__ __launch_bounds__(256, 2) void batch_global_stream_kernel(BatchStreamParams p) {
    constexpr int E = NB * 128;
    const int part = blockIdx.x, item = blockIdx.y, nparts = gridDim.x;
    const int tb = (int)(((long)p.ntiles * part) / nparts);
    const int te = (int)(((long)p.ntiles * (part + 1)) / nparts);
    stream_segment<NB, 1>(p.c, p.x + (long)item * p.N * E, p.N, tb, te, 0, p.c.rows, (long)item * p.c.rows, p.scores + (long)item * 16 * p.score_stride,
                          p.score_stride, (long)item * nparts + part, 0);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Merge per (item, head) (segment_item.hpp: merge_segments).  grid = (rows, B).
// ---------------------------------------------------------------------------------------------------------------------------------
struct BatchMergeParams {
    SegMergeParams c;
    const float* scores;
    long score_stride;
    int nparts, rows, T;
    float* ctx;             // [B * rows][E]
};

__global__ __launch_bounds__(256) void batch_merge_kernel(BatchMergeParams p) {
    extern __shared__ float ms[];
    const int r = blockIdx.x, item = blockIdx.y;
    merge_segments(p.c, ms, r, threadIdx.x, p.T, p.nparts, (long)item * p.nparts, p.scores + ((long)item * 16 + r) * p.score_stride,
                   p.ctx + ((long)item * p.rows + r) * p.c.E);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Placement of every item's packed rows (segment_item.hpp: place_equal_row): grid = B * item_rows, one output row per workgroup.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void batch_place_kernel(EqualPlaceParams p) { place_equal_row(p); }

}  // namespace hicom

using namespace hicom;
using namespace hicom_host;

namespace {

constexpr const char* kWho = "compressor_batch";

// workgroups per item of the segmented stream: B x chunks fills the chip twice over (two resident workgroups per CU); one chunk
// per item once B alone does
int batch_chunks(const hicom_compressor_batch_args* a) {
    const long ntiles = ((long)a->T * a->H * a->W + 15) / 16;
    long c = a->chunks > 0 ? a->chunks : (2L * num_cus() + a->B - 1) / a->B;
    if (c > ntiles) c = ntiles;
    if (c > kSegMaxChunks) c = kSegMaxChunks;
    return (int)(c < 1 ? 1 : c);
}

struct BatchLayout {
    SegLayout s;
    long score_stride;
    int chunks, wpi;
};

// ad: the k / v adaptors of the local stage, NULL for the plain recipe (hicom_compressor_batch_*)
BatchLayout batch_layout(const hicom_compressor_batch_args* a, const SegAdapt* ad) {
    BatchLayout l;
    const long B = a->B, N = (long)a->T * a->H * a->W;
    l.chunks = batch_chunks(a);
    l.wpi = (a->T / a->kt) * (a->H / a->ks) * (a->W / a->ks);
    l.score_stride = (N + 15) / 16 * 16;
    l.s = seg_layout(a, ad, SegTotals{B * 16 * l.score_stride, B * l.chunks, B * l.wpi, B * N, B * a->nh, B * l.chunks * 16, 0}, 0);
    return l;
}

int batch_check(const hicom_compressor_batch_args* a, const SegAdapt* ad) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "compressor_batch: NULL arguments");
    HICOM_REQUIRE(a->B > 0 && a->T > 0 && a->H > 0 && a->W > 0 && a->hidden > 0 && a->kt > 0 && a->ks > 0, HICOM_EINVAL, "compressor_batch: bad shape");
    int st = seg_check_items_shape(kWho, a);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->T % a->kt == 0 && a->H % a->ks == 0 && a->W % a->ks == 0, HICOM_EUNSUP,
                  "compressor_batch: needs an exact window partition (T=%d H=%d W=%d, windows %dx%dx%d)", a->T, a->H, a->W, a->kt, a->ks, a->ks);
    HICOM_REQUIRE(a->kt * a->ks * a->ks <= 64, HICOM_EUNSUP, "compressor_batch: windows of %d tokens (<= 64)", a->kt * a->ks * a->ks);
    HICOM_REQUIRE((long)a->B * a->T * a->H * a->W < (1L << 31) / 16, HICOM_EUNSUP, "compressor_batch: too many tokens in one call");
    st = seg_check_merge_lds(kWho, a, a->T);
    if (st != HICOM_OK) return st;
    return seg_adapt_check(kWho, ad, (long)a->B * a->T * a->H * a->W, a->E);
}

int64_t batch_workspace_bytes(const hicom_compressor_batch_args* a, const SegAdapt* ad) {
    const int st = batch_check(a, ad);
    if (st != HICOM_OK) return st;
    return batch_layout(a, ad).s.total;
}

// the four launches that divide by the item stride (segment_host.hpp: seg_step)
struct BatchItem {
    const hicom_compressor_batch_args* a;
    const BatchLayout& l;
    char* ws() const { return (char*)a->ws; }
    hipStream_t s() const { return (hipStream_t)a->stream; }

    int local(const uint16_t* key_x, const SegAdaptParams* ad) const {
        const int B = a->B, nwin = (int)l.s.n.windows;
        const hicom_axis at{B * a->T, a->kt, B * a->T / a->kt, B * a->T / a->kt};
        const hicom_axis ay{a->H, a->ks, a->H / a->ks, a->H / a->ks}, ax{a->W, a->ks, a->W / a->ks, a->W / a->ks};
        if (ad)
            HICOM_LAUNCH(batch_local_attn_adapt_kernel<3>, dim3((unsigned)((nwin + 3) / 4)), dim3(256), 0, s(), key_x, (const uint16_t*)a->ff,
                         (const uint16_t*)a->guide, *ad, at, ay, ax, l.wpi, nwin, a->l_scale, (_Float16*)(ws() + l.s.ctx16));
        else
            HICOM_LAUNCH(batch_local_attn_kernel<3>, dim3((unsigned)((nwin + 3) / 4)), dim3(256), 0, s(), key_x, (const uint16_t*)a->ff,
                         (const uint16_t*)a->guide, at, ay, ax, l.wpi, nwin, a->l_scale, (_Float16*)(ws() + l.s.ctx16));
        return seg_check_launch(kWho, "local stage");
    }

    int stream(const SegStreamParams& c) const {
        BatchStreamParams p;
        const int N = a->T * a->H * a->W;
        p.c = c;
        p.x = (const uint16_t*)a->ff; p.N = N; p.ntiles = (N + 15) / 16;
        p.scores = (float*)(ws() + l.s.scores); p.score_stride = l.score_stride;
        static bool attr_set = false;
        if (!attr_set) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(batch_global_stream_kernel<9>), hipFuncAttributeMaxDynamicSharedMemorySize, seg_stream_smem(1));
            attr_set = true;
        }
        HICOM_LAUNCH(batch_global_stream_kernel<9>, dim3((unsigned)l.chunks, (unsigned)a->B), dim3(256), seg_stream_smem(1), s(), p);
        return seg_check_launch(kWho, "global stream");
    }

    int merge(const SegMergeParams& c) const {
        BatchMergeParams p;
        p.c = c;
        p.scores = (const float*)(ws() + l.s.scores); p.score_stride = l.score_stride;
        p.nparts = l.chunks; p.rows = a->nh; p.T = a->T;
        p.ctx = (float*)(ws() + l.s.ctxg);
        HICOM_LAUNCH(batch_merge_kernel, dim3((unsigned)a->nh, (unsigned)a->B), dim3(256), (size_t)seg_merge_smem(a->T, a->H, a->W), s(), p);
        return seg_check_launch(kWho, "merge");
    }

    int place(const SegPlaceParams& c) const { return seg_place_equal(kWho, batch_place_kernel, a, c, l.wpi); }
};

int batch_fwd(const hicom_compressor_batch_args* a, const SegAdapt* ad) {
    int st = batch_check(a, ad);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->ws, HICOM_EINVAL, "compressor_batch: NULL pointer");
    const BatchLayout l = batch_layout(a, ad);
    st = seg_check_fwd(kWho, a, ad, l.s.total);
    if (st != HICOM_OK) return st;
    st = seg_check_equal_rows(kWho, a, l.wpi);
    if (st != HICOM_OK) return st;
    return seg_step(a, ad, l.s, BatchItem{a, l});
}

}  // namespace

extern "C" int64_t hicom_compressor_batch_workspace_bytes(const hicom_compressor_batch_args* a) { return batch_workspace_bytes(a, nullptr); }

extern "C" int hicom_compressor_batch_fwd(const hicom_compressor_batch_args* a) { return batch_fwd(a, nullptr); }

// ---- the adaptor recipe: the same step with the k / v adaptors on the local stage -------------------------------------------------------
extern "C" int64_t hicom_compressor_batch_adapt_workspace_bytes(const hicom_compressor_batch_adapt_args* a) { return seg_with_adapt(kWho, a, batch_workspace_bytes); }

extern "C" int hicom_compressor_batch_adapt_fwd(const hicom_compressor_batch_adapt_args* a) { return seg_with_adapt(kWho, a, batch_fwd); }
