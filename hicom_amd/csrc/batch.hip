// Batched compressor step: B items of one shape (images or short clips) through a launch sequence whose length does not depend on B.
//
// The math per item is the release recipe's (direct guide, local + global compressor); new is the item dimension:
//   * queries: q_proj, the k_proj fold with hi / lo planes and the score-side positional table run with M = B rows through the
//     existing small linears (hicom_linear_fwd, hicom_fold_query_split_fwd);
//   * local stage: kt | T, so no window crosses an item boundary: the [B T, H, W] stack is ONE window grid and window w reads the
//     guide row of item w / windows_per_item (batch_local_attn_kernel: one wave per window, contexts as the fp16 plane that
//     hicom_readout16_gemm_fwd takes);
//   * global stage: batch_global_stream_kernel, the narrow streaming kernel of global_stream.hip with blockIdx.y = item.  A
//     workgroup walks a contiguous range of 16-token tiles of ONE item (chunk blockIdx.x of `chunks`), so a partial state (m, l, ACC)
//     never mixes tokens of two items; the token index is item-local (frame index restarts at 0 per item), the tail tile re-reads
//     the item's own last token and is masked.  batch_merge_kernel then merges the chunks of each (item, head) row and adds the
//     value-side positional term from the row's t / y / x marginals (taken from the logits the stream kernel left);
//   * tail: v_proj per head, out_proj + residual, the two global readout layers with M = B rows (hicom_linear_fwd), both local
//     readout layers as one GEMM pair over all B x windows_per_item contexts (hicom_readout16_gemm_fwd), and ONE placement launch
//     that writes every item's packed rows: local tokens around the newline gaps, newline rows, the 32 copies of the global row.
// Twelve launches for any B.  Everything on the caller's stream, nothing synchronises the host.
//
// The k / v adaptor recipe (`local43_adaptkv_global32`, hicom_compressor_batch_adapt_*) is the same step with two more launches in
// front of the local stage -- the two layers of the adaptor MLPs as dense GEMMs over all B N tokens (segment_item.hpp: seg_adapt_mlps)
// -- and batch_local_attn_adapt_kernel in the local stage's place: fourteen launches.  One host implementation serves both; the plain
// entry points are its "no adaptor" case and run exactly the kernels and the workspace layout they ran before.
#include "segment_item.hpp"

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
// Segmented global stream: grid = (chunks, B), workgroup (part, item) walks chunk `part` of the item's tiles (segment_item.hpp:
// stream_segment).
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
    stream_segment<NB>(p.c, p.x + (long)item * p.N * E, p.N, tb, te, item, p.scores + (long)item * 16 * p.score_stride, p.score_stride,
                       (long)item * nparts + part);
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
// Placement of every item's packed rows (segment_item.hpp: place_row): grid = B * item_rows, one output row per workgroup.
// ---------------------------------------------------------------------------------------------------------------------------------
struct BatchPlaceParams {
    SegPlaceParams c;
    int wpi, nl_group, nl_count;
    long item_rows, global_row0, nl_first, nl_step, ldo;
};

__global__ __launch_bounds__(128) void batch_place_kernel(BatchPlaceParams p) {
    const long row = blockIdx.x;
    const long item = row / p.item_rows, r = row - item * p.item_rows;
    place_row(p.c, r, row * p.ldo, item, item * p.wpi, p.nl_group, p.nl_count, p.global_row0, p.nl_first, p.nl_step);
}

}  // namespace hicom

using namespace hicom;

namespace {

constexpr int kBatchMax = hicom_host::kSegMaxItems;
constexpr int kBatchMaxChunks = hicom_host::kSegMaxChunks;

// workgroups per item of the segmented stream: B x chunks fills the chip twice over (two resident workgroups per CU); one chunk
// per item once B alone does
int batch_chunks(const hicom_compressor_batch_args* a) {
    const long ntiles = ((long)a->T * a->H * a->W + 15) / 16;
    long c = a->chunks > 0 ? a->chunks : (2L * hicom_host::num_cus() + a->B - 1) / a->B;
    if (c > ntiles) c = ntiles;
    if (c > kBatchMaxChunks) c = kBatchMaxChunks;
    return (int)(c < 1 ? 1 : c);
}

struct BatchLayout {
    long qp, qhi, qlo, pos_a, scores, part_m, part_l, part_acc, ctxg, o, pre, hid, tok, ctx16, hid16, loc, total;
    hicom_host::SegAdaptLayout ad;      // behind the plain layout, whose offsets and total do not depend on it
    long score_stride;
    int chunks, wpi, rows_all;
};

// ad: the k / v adaptors of the local stage, NULL for the plain recipe (hicom_compressor_batch_*)
BatchLayout batch_layout(const hicom_compressor_batch_args* a, const hicom_host::SegAdapt* ad) {
    BatchLayout l;
    long off = 0;
    auto take = [&](long bytes) { const long at = off; off += (bytes + 255) / 256 * 256; return at; };
    const long B = a->B, E = a->E, N = (long)a->T * a->H * a->W, R = B * a->nh;
    l.chunks = batch_chunks(a);
    l.wpi = (a->T / a->kt) * (a->H / a->ks) * (a->W / a->ks);
    l.rows_all = (int)(B * l.wpi);
    l.score_stride = (N + 15) / 16 * 16;
    const int odt = a->out_dt == HICOM_DT_F32 ? 4 : 2;
    l.qp = take(B * E * 4);
    l.qhi = take(R * E * 2);
    l.qlo = take(R * E * 2);
    l.pos_a = take(R * (long)(a->P > 0 ? a->P : 1) * 4);
    l.scores = take(B * 16 * l.score_stride * 4);
    l.part_m = take(B * l.chunks * 16 * 4);
    l.part_l = take(B * l.chunks * 16 * 4);
    l.part_acc = take(B * l.chunks * 16 * E * 4);
    l.ctxg = take(R * E * 4);
    l.o = take(B * E * 4);
    l.pre = take(B * E * 4);
    l.hid = take(B * (long)a->hidden * 4);
    l.tok = take(B * (long)a->hidden * 4);
    l.ctx16 = take((long)l.rows_all * E * 2);
    l.hid16 = take((long)l.rows_all * a->hidden * 2);
    l.loc = take((long)l.rows_all * a->hidden * odt);
    l.ad = hicom_host::seg_adapt_layout(ad, B * N, E, take);
    l.total = off;
    return l;
}

int batch_check(const hicom_compressor_batch_args* a, const hicom_host::SegAdapt* ad) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "compressor_batch: NULL arguments");
    HICOM_REQUIRE(a->B > 0 && a->T > 0 && a->H > 0 && a->W > 0 && a->hidden > 0 && a->kt > 0 && a->ks > 0, HICOM_EINVAL, "compressor_batch: bad shape");
    HICOM_REQUIRE(a->B <= kBatchMax, HICOM_EUNSUP, "compressor_batch: B=%d items (<= %d per call)", a->B, kBatchMax);
    HICOM_REQUIRE(a->E == 1152, HICOM_EUNSUP, "compressor_batch: E=%d (only 1152)", a->E);
    HICOM_REQUIRE(a->nh > 0 && a->nh <= 16 && a->E % a->nh == 0, HICOM_EUNSUP, "compressor_batch: %d heads (<= 16 folded rows per item)", a->nh);
    HICOM_REQUIRE(a->hidden % 64 == 0, HICOM_EUNSUP, "compressor_batch: hidden=%d (multiple of 64: fp16 readout planes)", a->hidden);
    HICOM_REQUIRE(a->T % a->kt == 0 && a->H % a->ks == 0 && a->W % a->ks == 0, HICOM_EUNSUP,
                  "compressor_batch: needs an exact window partition (T=%d H=%d W=%d, windows %dx%dx%d)", a->T, a->H, a->W, a->kt, a->ks, a->ks);
    HICOM_REQUIRE(a->kt * a->ks * a->ks <= 64, HICOM_EUNSUP, "compressor_batch: windows of %d tokens (<= 64)", a->kt * a->ks * a->ks);
    HICOM_REQUIRE((long)a->B * a->T * a->H * a->W < (1L << 31) / 16, HICOM_EUNSUP, "compressor_batch: too many tokens in one call");
    HICOM_REQUIRE(((long)a->T * a->H + (long)a->T * a->W + a->T + a->H + a->W) * 4 <= 48 * 1024, HICOM_EUNSUP,
                  "compressor_batch: T=%d frames of %dx%d: the merge keeps T (H + W) marginal sums in LDS", a->T, a->H, a->W);
    HICOM_REQUIRE(a->out_dt == HICOM_DT_BF16 || a->out_dt == HICOM_DT_F32, HICOM_EUNSUP, "compressor_batch: output dtype %d (bf16 | f32)", a->out_dt);
    HICOM_REQUIRE(!a->pe == !a->kpe && (!a->pe || a->P > 0), HICOM_EINVAL, "compressor_batch: pe and kpe come together");
    return hicom_host::seg_adapt_check("compressor_batch", ad, (long)a->B * a->T * a->H * a->W, a->E);
}

int64_t batch_workspace_bytes(const hicom_compressor_batch_args* a, const hicom_host::SegAdapt* ad) {
    const int st = batch_check(a, ad);
    if (st != HICOM_OK) return st;
    return batch_layout(a, ad).total;
}

int batch_fwd(const hicom_compressor_batch_args* a, const hicom_host::SegAdapt* ad) {
    int st = batch_check(a, ad);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->ff && a->guide && a->out && a->ws, HICOM_EINVAL, "compressor_batch: NULL pointer");
    HICOM_REQUIRE(a->lw0_f16 && a->lw2_f16 && a->wq && a->wk && a->wv && a->wo && a->gw0 && a->gw2, HICOM_EINVAL, "compressor_batch: NULL weight");
    st = hicom_host::seg_adapt_check_weights("compressor_batch", ad);
    if (st != HICOM_OK) return st;
    const BatchLayout l = batch_layout(a, ad);
    HICOM_REQUIRE(a->ws_bytes >= l.total && (uintptr_t)a->ws % 256 == 0, HICOM_EINVAL, "compressor_batch: workspace of %ld bytes, 256-byte aligned",
                  l.total);
    HICOM_REQUIRE((uintptr_t)a->ff % 16 == 0 && (!a->fe || (uintptr_t)a->fe % 16 == 0) && (uintptr_t)a->guide % 16 == 0, HICOM_EINVAL,
                  "compressor_batch: 16-byte aligned inputs");
    const long item_local = (long)l.wpi + (a->nl_group ? l.wpi / a->nl_group : 0);
    HICOM_REQUIRE(a->n_global_rows > 0 && a->global_row0 >= item_local && a->item_rows == a->global_row0 + a->n_global_rows && a->ldo >= a->hidden &&
                      a->nl_group >= 0 && (!a->nl_group || l.wpi % a->nl_group == 0),
                  HICOM_EINVAL, "compressor_batch: output layout");
    HICOM_REQUIRE(a->nl_count == 0 || (a->newline && a->nl_step > 0 && a->nl_first >= 0 &&
                                       a->nl_first + (long)(a->nl_count - 1) * a->nl_step < a->global_row0),
                  HICOM_EINVAL, "compressor_batch: newline rows");
    // every local row of an item is a token row or a newline row
    HICOM_REQUIRE(a->global_row0 == (long)l.wpi + a->nl_count, HICOM_EINVAL, "compressor_batch: %ld local rows for %d tokens + %d newline rows",
                  (long)a->global_row0, l.wpi, a->nl_count);
    char* ws = (char*)a->ws;
    hipStream_t s = (hipStream_t)a->stream;
    const int B = a->B, E = a->E, nh = a->nh, R = B * nh, hd = E / nh, hidden = a->hidden;
    const int N = a->T * a->H * a->W;
    float* qp = (float*)(ws + l.qp);
    float* pos_a = a->pe ? (float*)(ws + l.pos_a) : nullptr;
    float* ctxg = (float*)(ws + l.ctxg);
    float *o = (float*)(ws + l.o), *pre = (float*)(ws + l.pre), *hid = (float*)(ws + l.hid), *tok = (float*)(ws + l.tok);

    // 1-2: queries per item
    st = hicom_linear_fwd(a->guide, HICOM_DT_BF16, a->wq, HICOM_DT_BF16, a->bq, HICOM_DT_BF16, nullptr, 0, B, E, E, 0, 0, HICOM_ACT_NONE, qp, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_fold_query_split_fwd(qp, a->wk, a->kpe, B, nh, E, a->P, 1.0f / sqrtf((float)hd), ws + l.qhi, ws + l.qlo, pos_a, a->P, nullptr, 0, 0,
                                    a->stream);
    if (st != HICOM_OK) return st;

    // 3: local stage over the stacked window grid (adaptor recipe: the two layers of the adaptor MLPs over all tokens in front of it)
    {
        const hicom_axis at{B * a->T, a->kt, B * a->T / a->kt, B * a->T / a->kt};
        const hicom_axis ay{a->H, a->ks, a->H / a->ks, a->H / a->ks}, ax{a->W, a->ks, a->W / a->ks, a->W / a->ks};
        const uint16_t* key_x = (const uint16_t*)(a->fe ? a->fe : a->ff);
        if (ad) {
            st = hicom_host::seg_adapt_mlps(*ad, key_x, a->ff, (long)B * N, E, ws, l.ad, a->stream);
            if (st != HICOM_OK) return st;
            HICOM_LAUNCH(batch_local_attn_adapt_kernel<3>, dim3((unsigned)((l.rows_all + 3) / 4)), dim3(256), 0, s, key_x, (const uint16_t*)a->ff,
                         (const uint16_t*)a->guide, hicom_host::seg_adapt_params(*ad, ws, l.ad), at, ay, ax, l.wpi, l.rows_all, a->l_scale,
                         (_Float16*)(ws + l.ctx16));
        } else {
            HICOM_LAUNCH(batch_local_attn_kernel<3>, dim3((unsigned)((l.rows_all + 3) / 4)), dim3(256), 0, s, key_x, (const uint16_t*)a->ff,
                         (const uint16_t*)a->guide, at, ay, ax, l.wpi, l.rows_all, a->l_scale, (_Float16*)(ws + l.ctx16));
        }
        st = hicom_host::check_launch("compressor_batch: local stage");
        if (st != HICOM_OK) return st;
    }

    // 4: segmented global stream
    {
        BatchStreamParams p;
        p.x = (const uint16_t*)a->ff; p.N = N; p.ntiles = (N + 15) / 16;
        p.c.qhi = (const uint16_t*)(ws + l.qhi); p.c.qlo = (const uint16_t*)(ws + l.qlo);
        p.c.pos_a = pos_a; p.c.pos_stride = a->P; p.c.rows = nh;
        p.c.H = a->H; p.c.W = a->W; p.c.HW = a->H * a->W;
        p.c.t0i = a->t_index0; p.c.y0i = a->y_index0; p.c.x0i = a->x_index0;
        p.scores = (float*)(ws + l.scores); p.score_stride = l.score_stride;
        p.c.part_m = (float*)(ws + l.part_m); p.c.part_l = (float*)(ws + l.part_l); p.c.part_acc = (float*)(ws + l.part_acc);
        constexpr int smem = hicom_host::kSegStreamSmem;
        static bool attr_set = false;
        if (!attr_set) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(batch_global_stream_kernel<9>), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
            attr_set = true;
        }
        HICOM_LAUNCH(batch_global_stream_kernel<9>, dim3((unsigned)l.chunks, (unsigned)B), dim3(256), smem, s, p);
        st = hicom_host::check_launch("compressor_batch: global stream");
        if (st != HICOM_OK) return st;
    }

    // 5: merge per item
    {
        BatchMergeParams p;
        p.c.part_m = (const float*)(ws + l.part_m); p.c.part_l = (const float*)(ws + l.part_l); p.c.part_acc = (const float*)(ws + l.part_acc);
        p.scores = (const float*)(ws + l.scores); p.score_stride = l.score_stride;
        p.c.pe = a->pe; p.nparts = l.chunks; p.rows = nh; p.c.E = E; p.T = a->T; p.c.H = a->H; p.c.W = a->W;
        p.c.t0i = a->t_index0; p.c.y0i = a->y_index0; p.c.x0i = a->x_index0;
        p.ctx = ctxg;
        const size_t smem = ((size_t)a->T * a->H + (size_t)a->T * a->W + a->T + a->H + a->W) * 4;
        HICOM_LAUNCH(batch_merge_kernel, dim3((unsigned)nh, (unsigned)B), dim3(256), smem, s, p);
        st = hicom_host::check_launch("compressor_batch: merge");
        if (st != HICOM_OK) return st;
    }

    // 6-9: the global tail with M = B rows
    st = hicom_linear_fwd(ctxg, HICOM_DT_F32, a->wv, HICOM_DT_BF16, a->bv, HICOM_DT_BF16, nullptr, 0, B, E, E, nh, hd, HICOM_ACT_NONE, o, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_linear_fwd(o, HICOM_DT_F32, a->wo, HICOM_DT_BF16, a->bo, HICOM_DT_BF16, a->guide, 2, B, E, E, 0, 0, HICOM_ACT_NONE, pre, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_linear_fwd(pre, HICOM_DT_F32, a->gw0, HICOM_DT_BF16, a->gb0, HICOM_DT_BF16, nullptr, 0, B, hidden, E, 0, 0, HICOM_ACT_GELU, hid, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_linear_fwd(hid, HICOM_DT_F32, a->gw2, HICOM_DT_BF16, a->gb2, HICOM_DT_BF16, nullptr, 0, B, hidden, hidden, 0, 0, HICOM_ACT_NONE, tok, a->stream);
    if (st != HICOM_OK) return st;

    // 10-11: the local readout as one GEMM pair over all items' windows
    st = hicom_readout16_gemm_fwd(ws + l.ctx16, a->lw0_f16, a->lb0, HICOM_DT_BF16, l.rows_all, hidden, E, HICOM_ACT_GELU, ws + l.hid16, nullptr, 0, 0, 0, 0,
                                  nullptr, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_readout16_gemm_fwd(ws + l.hid16, a->lw2_f16, a->lb2, HICOM_DT_BF16, l.rows_all, hidden, hidden, HICOM_ACT_NONE, nullptr, ws + l.loc, a->out_dt,
                                  hidden, 0, 0, nullptr, a->stream);
    if (st != HICOM_OK) return st;

    // 12: every item's packed rows
    {
        BatchPlaceParams p;
        p.c.loc = ws + l.loc; p.c.tok = tok; p.c.newline = (const uint16_t*)a->newline; p.c.out = a->out;
        p.c.out_f32 = a->out_dt == HICOM_DT_F32; p.c.hidden = hidden; p.wpi = l.wpi; p.nl_group = a->nl_group; p.nl_count = a->nl_count;
        p.item_rows = a->item_rows; p.global_row0 = a->global_row0; p.nl_first = a->nl_first; p.nl_step = a->nl_step > 0 ? a->nl_step : 1; p.ldo = a->ldo;
        HICOM_LAUNCH(batch_place_kernel, dim3((unsigned)((long)B * a->item_rows)), dim3(128), 0, s, p);
        st = hicom_host::check_launch("compressor_batch: placement");
    }
    return st;
}

}  // namespace

extern "C" int64_t hicom_compressor_batch_workspace_bytes(const hicom_compressor_batch_args* a) { return batch_workspace_bytes(a, nullptr); }

extern "C" int hicom_compressor_batch_fwd(const hicom_compressor_batch_args* a) { return batch_fwd(a, nullptr); }

// ---- the adaptor recipe: the same step with the k / v adaptors on the local stage -------------------------------------------------------
extern "C" int64_t hicom_compressor_batch_adapt_workspace_bytes(const hicom_compressor_batch_adapt_args* a) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "compressor_batch: NULL arguments");
    const hicom_host::SegAdapt ad{&a->ak, &a->av, a->alpha_dt, a->eps};
    return batch_workspace_bytes(&a->base, &ad);
}

extern "C" int hicom_compressor_batch_adapt_fwd(const hicom_compressor_batch_adapt_args* a) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "compressor_batch: NULL arguments");
    const hicom_host::SegAdapt ad{&a->ak, &a->av, a->alpha_dt, a->eps};
    return batch_fwd(&a->base, &ad);
}
