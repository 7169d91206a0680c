// Multi-guide compressor step: ONE clip, Q instructions, the visual tokens read once.
//
// The guide enters the two stages only as a query: one more 1152-d query against the same keys and values of every window, nh more
// folded rows against the same token tiles.  So Q guides are one pass over the tokens plus Q times the window-sized work, in a launch
// sequence whose length does not depend on Q:
//    1-2  hicom_linear_fwd (q_proj), hicom_fold_query_split_fwd with M = Q: the nh folded rows of guide q are rows nh q .. nh q + nh - 1,
//         densely packed (rows_pad = the row count rounded up to the 32 rows of one pass of the many-row stream kernel)
//    3    multi_guide_local_kernel: one wave per window, every key row and every value row of the window loaded once per group of
//         kGuideGroup guides; fp16 contexts into the guide-major plane [Q][windows][E]
//    4    the many-row global stream (global_stream.hip, the kernel of the guide-off recipe) over the nh Q rows
//    5    its merge with the value-side positional term (merge.hip): two launches behind in-kernel marginals, three behind the logit tensor
//    6-9  v_proj per head, out_proj + residual, GELU(gw0 .), gw2 with M = Q
//  10-11  the local readout as one GEMM pair over M = Q x windows rows
//   12    placement (segment_item.hpp: place_row, item = guide)
// The packed-row layout integers are those of the batched step and hold for every guide.
#include <math.h>

#include "segment_host.hpp"

namespace hicom {

constexpr int kGuideGroup = 4;      // guides a wave carries through one walk over a window's rows (72 query / accumulator floats per lane)

// ---------------------------------------------------------------------------------------------------------------------------------
// Local stage: the window of local_window_ctx16 (segment_item.hpp) for NG guides at once.  Each key row meets NG queries, each value
// row NG accumulators; every guide keeps its own logit, softmax and accumulator chain, written as the single-guide loop writes them,
// so a guide's context does not depend on NG, on its place in the group or on its neighbours.  qrows: the group's first guide row;
// o: its context row, the next guide's `plane` elements further.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int NV, int NG>
__device__ __forceinline__ void multi_window_ctx16(const uint16_t* key, const uint16_t* value, const uint16_t* qrows, const WindowGeom& g,
                                                   int lane, float scale, _Float16* o, long plane) {
    constexpr int D = NV * 384;
    float sc[NG];
    {
        float q[NG][NV][6];
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            load_row<NV>(qrows + (long)u * D, lane, q[u]);
            sc[u] = -3.0e38f;
        }
        for (int i = 0; i < g.WIN; ++i) {
            float k[NV][6];
            load_row<NV>(key + g.token_of(i) * D, lane, k);
#pragma unroll
            for (int u = 0; u < NG; ++u) {
                const float d = wave_sum_fast(row_dot<NV>(q[u], k)) * scale;
                if (lane == i) sc[u] = d;
            }
        }
    }
    float pw[NG];
#pragma unroll
    for (int u = 0; u < NG; ++u) {
        const float mx = wave_max_fast(sc[u]);
        const float e = lane < g.WIN ? expf(sc[u] - mx) : 0.f;
        pw[u] = e / wave_sum_fast(e);
    }
    float acc[NG][NV][6];
#pragma unroll
    for (int u = 0; u < NG; ++u) row_zero<NV>(acc[u]);
    for (int i = 0; i < g.WIN; ++i) {
        float v[NV][6];
        load_row<NV>(value + g.token_of(i) * D, lane, v);
#pragma unroll
        for (int u = 0; u < NG; ++u) row_axpy<NV>(__shfl(pw[u], i, 64), v, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < NG; ++u)
#pragma unroll
        for (int s = 0; s < NV; ++s)
#pragma unroll
            for (int j = 0; j < 6; ++j)
                o[(long)u * plane + 384 * s + 6 * lane + j] = (_Float16)fminf(fmaxf(acc[u][s][j], -65504.f), 65504.f);
}

// One wave per window of the clip's grid; for Q > kGuideGroup the wave walks further groups over the same window (its rows are then
// expected to come from L2).  ctx16: [Q][nwin][D].
template <int NV>
__global__ __launch_bounds__(256) void multi_guide_local_kernel(const uint16_t* key, const uint16_t* value, const uint16_t* guide, hicom_axis at,
                                                                hicom_axis ay, hicom_axis ax, int Q, int nwin, float scale, _Float16* ctx16) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const WindowGeom g(at, ay, ax, win);
    const long plane = (long)nwin * D;
    for (int g0 = 0; g0 < Q; g0 += kGuideGroup) {
        const uint16_t* q = guide + (long)g0 * D;
        _Float16* o = ctx16 + (long)g0 * plane + (long)win * D;
        switch (Q - g0 < kGuideGroup ? Q - g0 : kGuideGroup) {      // (wave-uniform)
            case 1: multi_window_ctx16<NV, 1>(key, value, q, g, lane, scale, o, plane); break;
            case 2: multi_window_ctx16<NV, 2>(key, value, q, g, lane, scale, o, plane); break;
            case 3: multi_window_ctx16<NV, 3>(key, value, q, g, lane, scale, o, plane); break;
            default: multi_window_ctx16<NV, 4>(key, value, q, g, lane, scale, o, plane); break;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Placement of every guide's packed rows (segment_item.hpp: place_row, item = guide): grid = Q * item_rows, one output row per workgroup.
// ---------------------------------------------------------------------------------------------------------------------------------
struct MultiPlaceParams {
    SegPlaceParams c;
    int wpi, nl_group, nl_count;
    long item_rows, global_row0, nl_first, nl_step, ldo;
};

__global__ __launch_bounds__(128) void multi_guide_place_kernel(MultiPlaceParams p) {
    const long row = blockIdx.x;
    const long item = row / p.item_rows, r = row - item * p.item_rows;
    place_row(p.c, r, row * p.ldo, item, item * p.wpi, p.nl_group, p.nl_count, p.global_row0, p.nl_first, p.nl_step);
}

}  // namespace hicom

using namespace hicom;
using namespace hicom_host;

namespace {

constexpr const char* kWho = "compressor_multiguide";
constexpr int kMaxGuides = 32;          // nh = 9 heads x 32 guides = 288 rows: the row count the many-row stream kernel is proven at
constexpr int kMaxStreamChunks = 256;

typedef hicom_compressor_multiguide_args Args;

// token chunks of the global stream
int mg_chunks(const Args* a, long N, int rows_pad) {
    const long ntiles = (N + 15) / 16;
    long c = a->chunks > 0 ? a->chunks : hicom_global_stream_nparts(N, rows_pad);
    if (c > ntiles) c = ntiles;
    if (c > kMaxStreamChunks) c = kMaxStreamChunks;
    return (int)(c < 1 ? 1 : c);
}

// The workspace.  Per guide: qp, o, pre (E floats each), hid, tok (hidden floats each) and, per guide and window, the fp16 context
// row, the fp16 hidden row and the readout row of the output dtype.  Per folded row (rows_pad of them, whatever Q is inside a pass):
// the hi / lo query planes, the score-side positional table, the merged contexts and softmax states, the merge's scratch and, per row
// and token chunk, the partial states.  Token-sized: only `scores`, the [rows_pad][N] logits of the stream's logit-tensor form (the
// in-kernel-marginal form keeps its [chunks][rows_pad][marg width] marginals there instead; the region holds either).
struct MgLayout {
    long qp, qhi, qlo, pos_a, scores, part_m, part_l, part_acc, scratch, ml, ctxg, o, pre, hid, tok, ctx16, hid16, loc, total;
    long N, score_stride;
    int rows, rows_pad, nparts, wpi;
};

MgLayout mg_layout(const Args* a) {
    MgLayout l;
    long off = 0;
    auto take = [&](long bytes) { const long at = off; off += (bytes + 255) / 256 * 256; return at; };
    const long Q = a->Q, E = a->E, hidden = a->hidden;
    const int odt = a->out_dt == HICOM_DT_F32 ? 4 : 2;
    l.N = (long)a->T * a->H * a->W;
    l.rows = a->Q * a->nh;
    l.rows_pad = (l.rows + 31) / 32 * 32;
    l.nparts = mg_chunks(a, l.N, l.rows_pad);
    l.wpi = (a->T / a->kt) * (a->H / a->ks) * (a->W / a->ks);
    l.score_stride = (l.N + 15) / 16 * 16;
    const long R = l.rows_pad, W = (long)Q * l.wpi;
    const long logits = R * l.score_stride * 4, marg = (long)l.nparts * R * hicom_global_stream_marg_width(a->H, a->W) * 4;
    l.qp = take(Q * E * 4);
    l.qhi = take(R * E * 2);
    l.qlo = take(R * E * 2);
    l.pos_a = take(R * (long)(a->P > 0 ? a->P : 1) * 4);
    l.scores = take(logits > marg ? logits : marg);
    l.part_m = take((long)l.nparts * R * 4);
    l.part_l = take((long)l.nparts * R * 4);
    l.part_acc = take((long)l.nparts * R * E * 4);
    l.scratch = take(R * a->T * (a->H + a->W + 2) * 4);
    l.ml = take(R * 2 * 4);
    l.ctxg = take(R * E * 4);
    l.o = take(Q * E * 4);
    l.pre = take(Q * E * 4);
    l.hid = take(Q * hidden * 4);
    l.tok = take(Q * hidden * 4);
    l.ctx16 = take(W * E * 2);
    l.hid16 = take(W * hidden * 2);
    l.loc = take(W * hidden * odt);
    l.total = off;
    return l;
}

int mg_check(const Args* a) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "compressor_multiguide: NULL arguments");
    HICOM_REQUIRE(a->Q >= 1 && a->Q <= kMaxGuides, HICOM_EUNSUP, "compressor_multiguide: Q=%d guides (1 <= Q <= %d per call)", a->Q, kMaxGuides);
    HICOM_REQUIRE(a->T > 0 && a->H > 0 && a->W > 0 && a->hidden > 0 && a->kt > 0 && a->ks > 0, HICOM_EINVAL, "compressor_multiguide: bad shape");
    HICOM_REQUIRE(a->E == 1152, HICOM_EUNSUP, "compressor_multiguide: E=%d (only 1152)", a->E);
    HICOM_REQUIRE(a->nh > 0 && a->nh <= 16 && a->E % a->nh == 0, HICOM_EUNSUP, "compressor_multiguide: %d heads (<= 16 folded rows per guide)", a->nh);
    HICOM_REQUIRE(a->hidden % 64 == 0, HICOM_EUNSUP, "compressor_multiguide: hidden=%d (multiple of 64: fp16 readout planes)", a->hidden);
    HICOM_REQUIRE(a->out_dt == HICOM_DT_BF16 || a->out_dt == HICOM_DT_F32, HICOM_EUNSUP, "compressor_multiguide: output dtype %d (bf16 | f32)", a->out_dt);
    HICOM_REQUIRE(!a->pe == !a->kpe && (!a->pe || a->P > 0), HICOM_EINVAL, "compressor_multiguide: pe and kpe come together");
    HICOM_REQUIRE(a->T % a->kt == 0 && a->H % a->ks == 0 && a->W % a->ks == 0, HICOM_EUNSUP,
                  "compressor_multiguide: needs an exact window partition (T=%d H=%d W=%d, windows %dx%dx%d)", a->T, a->H, a->W, a->kt, a->ks, a->ks);
    HICOM_REQUIRE(a->kt * a->ks * a->ks <= 64, HICOM_EUNSUP, "compressor_multiguide: windows of %d tokens (<= 64)", a->kt * a->ks * a->ks);
    const long N = (long)a->T * a->H * a->W;
    HICOM_REQUIRE(N < (1L << 31) / 16 && N * a->Q < (1L << 31) / 16, HICOM_EUNSUP, "compressor_multiguide: too many tokens in one call");
    // what the merge (merge.hip) keeps in LDS: a frame of logits per workgroup on grids above 32 x 32, the row's weights and 64 staged
    // frames of marginals
    HICOM_REQUIRE(a->H + a->W <= 1024 && ((a->H <= 32 && a->W <= 32) || ((long)a->H * a->W + a->H + 4) * 4 <= 60000), HICOM_EUNSUP,
                  "compressor_multiguide: a %dx%d grid: the merge keeps a frame of logits in LDS", a->H, a->W);
    HICOM_REQUIRE(((long)kMaxStreamChunks + 2L * a->T + a->H + a->W + 64L * (a->H + a->W + 2) + 16 * 64 + 4) * 4 <= 60000, HICOM_EUNSUP,
                  "compressor_multiguide: T=%d frames of %dx%d: the merge keeps the row's T + H + W weights and 64 frames of marginals in LDS", a->T,
                  a->H, a->W);
    return HICOM_OK;
}

int mg_fwd(const Args* a) {
    int st = mg_check(a);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->ff && a->guide && a->out, HICOM_EINVAL, "compressor_multiguide: NULL pointer");
    HICOM_REQUIRE(a->lw0_f16 && a->lw2_f16 && a->wq && a->wk && a->wv && a->wo && a->gw0 && a->gw2, HICOM_EINVAL, "compressor_multiguide: NULL weight");
    const MgLayout l = mg_layout(a);
    st = seg_check_ws(kWho, a, l.total);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE((uintptr_t)a->ff % 16 == 0 && (!a->fe || (uintptr_t)a->fe % 16 == 0) && (uintptr_t)a->guide % 16 == 0, HICOM_EINVAL,
                  "compressor_multiguide: 16-byte aligned inputs");
    const long item_local = (long)l.wpi + (a->nl_group ? l.wpi / a->nl_group : 0);
    HICOM_REQUIRE(a->n_global_rows > 0 && a->global_row0 >= item_local && a->item_rows == a->global_row0 + a->n_global_rows && a->ldo >= a->hidden &&
                      a->nl_group >= 0 && (!a->nl_group || l.wpi % a->nl_group == 0),
                  HICOM_EINVAL, "compressor_multiguide: output layout");
    HICOM_REQUIRE(a->nl_count == 0 || (a->newline && a->nl_step > 0 && a->nl_first >= 0 &&
                                       a->nl_first + (long)(a->nl_count - 1) * a->nl_step < a->global_row0),
                  HICOM_EINVAL, "compressor_multiguide: newline rows");
    HICOM_REQUIRE(a->global_row0 == (long)l.wpi + a->nl_count, HICOM_EINVAL, "compressor_multiguide: %ld local rows for %d tokens + %d newline rows",
                  (long)a->global_row0, l.wpi, a->nl_count);

    char* ws = (char*)a->ws;
    hipStream_t s = (hipStream_t)a->stream;
    const int Q = a->Q, E = a->E, nh = a->nh, hd = E / nh, hidden = a->hidden, windows = Q * l.wpi;
    float* qp = (float*)(ws + l.qp);
    float* pos_a = a->pe ? (float*)(ws + l.pos_a) : nullptr;
    float *part_m = (float*)(ws + l.part_m), *part_l = (float*)(ws + l.part_l), *part_acc = (float*)(ws + l.part_acc);
    float *scores = (float*)(ws + l.scores), *scratch = (float*)(ws + l.scratch), *ml = (float*)(ws + l.ml), *ctxg = (float*)(ws + l.ctxg);
    float *o = (float*)(ws + l.o), *pre = (float*)(ws + l.pre), *hid = (float*)(ws + l.hid), *tok = (float*)(ws + l.tok);

    // 1-2: the queries of all guides; guide q's folded rows are rows nh q .. of the planes (rows >= nh Q are never stored by the stream)
    st = hicom_linear_fwd(a->guide, HICOM_DT_BF16, a->wq, HICOM_DT_BF16, a->bq, HICOM_DT_BF16, nullptr, 0, Q, E, E, 0, 0, HICOM_ACT_NONE, qp, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_fold_query_split_fwd(qp, a->wk, a->kpe, Q, nh, E, a->P, 1.0f / sqrtf((float)hd), ws + l.qhi, ws + l.qlo, pos_a, a->P, nullptr, 0, 0,
                                    a->stream);
    if (st != HICOM_OK) return st;

    // 3: local stage
    {
        const uint16_t* key_x = (const uint16_t*)(a->fe ? a->fe : a->ff);
        const hicom_axis at{a->T, a->kt, a->T / a->kt, a->T / a->kt};
        const hicom_axis ay{a->H, a->ks, a->H / a->ks, a->H / a->ks}, ax{a->W, a->ks, a->W / a->ks, a->W / a->ks};
        HICOM_LAUNCH(multi_guide_local_kernel<3>, dim3((unsigned)((l.wpi + 3) / 4)), dim3(256), 0, s, key_x, (const uint16_t*)a->ff,
                     (const uint16_t*)a->guide, at, ay, ax, Q, l.wpi, a->l_scale, (_Float16*)(ws + l.ctx16));
        st = seg_check_launch(kWho, "local stage");
        if (st != HICOM_OK) return st;
    }

    // 4-5: the many-row global stream over all guides' folded rows and its merge
    const bool marg = a->pe && hicom_global_stream_has_marg(l.N, E, l.rows_pad, a->H, a->W, l.nparts) == 1;
    if (marg) {
        st = hicom_global_stream_marg_fwd(a->ff, l.N, E, ws + l.qhi, ws + l.qlo, l.rows, l.rows_pad, pos_a, a->P, a->H, a->W, a->t_index0, a->y_index0,
                                          a->x_index0, nullptr, 0, part_m, part_l, part_acc, scores, l.nparts, a->stream);
        if (st != HICOM_OK) return st;
        st = hicom_global_merge_marg_fwd(part_m, part_l, part_acc, scores, l.nparts, l.rows, l.rows_pad, E, l.N, a->H, a->W, a->pe, a->t_index0,
                                         a->y_index0, a->x_index0, scratch, ml, ctxg, 1, a->stream);
    } else {
        st = hicom_global_stream_fwd(a->ff, l.N, E, ws + l.qhi, ws + l.qlo, l.rows, l.rows_pad, pos_a, a->P, a->H, a->W, a->t_index0, a->y_index0,
                                     a->x_index0, scores, l.score_stride, part_m, part_l, part_acc, l.nparts, a->stream);
        if (st != HICOM_OK) return st;
        st = hicom_global_merge_fwd(part_m, part_l, part_acc, l.nparts, l.rows, l.rows_pad, E, scores, l.score_stride, l.N, a->H, a->W, a->pe,
                                    a->t_index0, a->y_index0, a->x_index0, scratch, ml, ctxg, 1, a->stream);
    }
    if (st != HICOM_OK) return st;

    // 6-9: the global tail with M = Q rows
    st = hicom_linear_fwd(ctxg, HICOM_DT_F32, a->wv, HICOM_DT_BF16, a->bv, HICOM_DT_BF16, nullptr, 0, Q, E, E, nh, hd, HICOM_ACT_NONE, o, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_linear_fwd(o, HICOM_DT_F32, a->wo, HICOM_DT_BF16, a->bo, HICOM_DT_BF16, a->guide, 2, Q, E, E, 0, 0, HICOM_ACT_NONE, pre, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_linear_fwd(pre, HICOM_DT_F32, a->gw0, HICOM_DT_BF16, a->gb0, HICOM_DT_BF16, nullptr, 0, Q, hidden, E, 0, 0, HICOM_ACT_GELU, hid, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_linear_fwd(hid, HICOM_DT_F32, a->gw2, HICOM_DT_BF16, a->gb2, HICOM_DT_BF16, nullptr, 0, Q, hidden, hidden, 0, 0, HICOM_ACT_NONE, tok, a->stream);
    if (st != HICOM_OK) return st;

    // 10-11: the local readout as one GEMM pair over all guides' windows
    st = hicom_readout16_gemm_fwd(ws + l.ctx16, a->lw0_f16, a->lb0, HICOM_DT_BF16, windows, hidden, E, HICOM_ACT_GELU, ws + l.hid16, nullptr, 0, 0, 0, 0, nullptr,
                                  a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_readout16_gemm_fwd(ws + l.hid16, a->lw2_f16, a->lb2, HICOM_DT_BF16, windows, hidden, hidden, HICOM_ACT_NONE, nullptr, ws + l.loc, a->out_dt, hidden,
                                  0, 0, nullptr, a->stream);
    if (st != HICOM_OK) return st;

    // 12: every guide's packed rows
    {
        MultiPlaceParams p;
        p.c.loc = ws + l.loc; p.c.tok = tok; p.c.newline = (const uint16_t*)a->newline; p.c.out = a->out;
        p.c.out_f32 = a->out_dt == HICOM_DT_F32; p.c.hidden = hidden;
        p.wpi = l.wpi; p.nl_group = a->nl_group; p.nl_count = a->nl_count;
        p.item_rows = a->item_rows; p.global_row0 = a->global_row0; p.nl_first = a->nl_first; p.nl_step = a->nl_step > 0 ? a->nl_step : 1; p.ldo = a->ldo;
        HICOM_LAUNCH(multi_guide_place_kernel, dim3((unsigned)((long)Q * a->item_rows)), dim3(128), 0, s, p);
    }
    return seg_check_launch(kWho, "placement");
}

}  // namespace

extern "C" int64_t hicom_compressor_multiguide_workspace_bytes(const hicom_compressor_multiguide_args* a) {
    const int st = mg_check(a);
    if (st != HICOM_OK) return st;
    return mg_layout(a).total;
}

extern "C" int hicom_compressor_multiguide_fwd(const hicom_compressor_multiguide_args* a) { return mg_fwd(a); }
