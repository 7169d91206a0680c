// Ragged compressor step: B items of unequal length and mixed modality (single images, clips of any length, 1-frame "videos") read in
// place from the vision tower's stacked [sum T_i, H, W, E] tensor, through the twelve launches of the batched step (batch.hip).
//
// The math per item and the per-item device code are batch.hip's (segment_item.hpp); what differs is where a wave or workgroup
// learns its item.  batch.hip divides by a constant stride; here a table region at the head of the workspace says it
// (hicom_compressor_ragged_prepare derives it on the host, once per plan):
//   * item table, one RaggedItem per item: first token, token count, T, kt, first window, first output row, the layout integers of
//     its packed rows, where its logits and partial states live and how many work units stream it;
//   * work units {item, first tile, last tile, partial-state slot} of the segmented stream: a 1-D grid, one workgroup per unit.
//     Tiles are counted from the ITEM's first token (item offsets are 36, 180, 216 ... tokens: no multiple of a tile), a unit never
//     spans two items, and item i gets chunks_i ~ 2 #CUs ntiles_i / sum ntiles of them, in [1, min(ntiles_i, 64)];
//   * window -> item and output row -> item lookups (one int each) for the local stage and the placement.
// The stacked tensor is not one window grid (kt differs between neighbours), so the local stage builds each window's geometry from its
// item's own (T, kt) and offsets the token index by the item's first token.  The four lookups are wave-uniform loads through a
// kernel-argument pointer with a uniform index: they land in SGPRs.
// Launches 1-2 and 6-11 are the existing entry points with M = B or M = sum windows.  hicom_compressor_ragged_fwd only launches.
//
// The k / v adaptor recipe (hicom_compressor_ragged_adapt_*) adds what batch.hip adds: the adaptor MLPs as two dense GEMM launches over
// the whole stack in front of the local stage (token-wise: they need no item boundaries) and ragged_local_attn_adapt_kernel in the
// local stage's place -- fourteen launches.  The plain entry points are the "no adaptor" case of the one host implementation below.
#include <vector>

#include "segment_item.hpp"

namespace hicom {

struct RaggedItem {      // 16 ints; mirrored by hicom_amd/ragged.py: plan_tables
    int tok0, N;         // first token in the stack, tokens
    int T, kt;
    int win0;            // first window in the concatenated window list
    int slot0, chunks;   // partial-state slots = work units of this item
    int score_off;       // its logits: scores + 16 * score_off, [16][ceil16(N)]
    int row0;            // first output row
    int global_row0;     // rows of the item in front of its global rows
    int nl_group, nl_count, nl_first, nl_step;
    int pad0, pad1;
};
static_assert(sizeof(RaggedItem) == 64, "item table entries are 16 ints");

// ---- 3: local stage, one wave per window of the concatenated window list ----
template <int NV>
__global__ __launch_bounds__(256) void ragged_local_attn_kernel(const uint16_t* key, const uint16_t* value, const uint16_t* guide,
                                                                const RaggedItem* items, const int* win_item, hicom_axis ay, hicom_axis ax,
                                                                int nwin, float scale, _Float16* ctx16) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const int item = win_item[win];
    const RaggedItem it = items[item];
    const hicom_axis at{it.T, it.kt, it.T / it.kt, it.T / it.kt};
    const WindowGeom g(at, ay, ax, win - it.win0);
    const long first = (long)it.tok0 * D;
    local_window_ctx16<NV>(key + first, value + first, guide + (long)item * D, g, lane, scale, ctx16 + (long)win * D);
}

// ... with the k / v adaptor blends fused into the row loads (segment_item.hpp: local_window_adapt_ctx16); the y rows of an item start
// at its first token like its x rows
template <int NV>
__global__ __launch_bounds__(256) void ragged_local_attn_adapt_kernel(const uint16_t* key, const uint16_t* value, const uint16_t* guide,
                                                                      SegAdaptParams ad, const RaggedItem* items, const int* win_item,
                                                                      hicom_axis ay, hicom_axis ax, int nwin, float scale, _Float16* ctx16) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const int item = win_item[win];
    const RaggedItem it = items[item];
    const hicom_axis at{it.T, it.kt, it.T / it.kt, it.T / it.kt};
    const WindowGeom g(at, ay, ax, win - it.win0);
    const long first = (long)it.tok0 * D;
    local_window_adapt_ctx16<NV>(key + first, ad.ky ? ad.ky + first : nullptr, value + first, ad.vy ? ad.vy + first : nullptr, ad,
                                 guide + (long)item * D, g, lane, scale, ctx16 + (long)win * D);
}

// ---- 4: segmented global stream, one workgroup per work unit ----
struct RaggedStreamParams {
    SegStreamParams c;
    const uint16_t* x;      // [sum N_i][E]
    float* scores;
    const int4* units;      // {item, first tile, last tile (exclusive), slot}
    const RaggedItem* items;
};

template <int NB>
__global__ __launch_bounds__(256, 2) void ragged_global_stream_kernel(RaggedStreamParams p) {
    constexpr int E = NB * 128;
    const int4 u = p.units[blockIdx.x];
    const int N = p.items[u.x].N, tok0 = p.items[u.x].tok0, soff = p.items[u.x].score_off;
    stream_segment<NB>(p.c, p.x + (long)tok0 * E, N, u.y, u.z, u.x, p.scores + (long)soff * 16, (long)((N + 15) / 16 * 16), (long)u.w);
}

// ---- 5: merge per (item, head), grid = (rows, B), LDS sized for the longest item ----
struct RaggedMergeParams {
    SegMergeParams c;
    const float* scores;
    const RaggedItem* items;
    int rows;
    float* ctx;             // [B * rows][E]
};

__global__ __launch_bounds__(256) void ragged_merge_kernel(RaggedMergeParams p) {
    extern __shared__ float ms[];
    const int r = blockIdx.x, item = blockIdx.y;
    const RaggedItem it = p.items[item];
    const long stride = (it.N + 15) / 16 * 16;
    merge_segments(p.c, ms, r, threadIdx.x, it.T, it.chunks, (long)it.slot0, p.scores + (long)it.score_off * 16 + r * stride,
                   p.ctx + ((long)item * p.rows + r) * p.c.E);
}

// ---- 12: placement, one output row per workgroup over all items' rows ----
struct RaggedPlaceParams {
    SegPlaceParams c;
    const RaggedItem* items;
    const int* row_item;
    long ldo;
};

__global__ __launch_bounds__(128) void ragged_place_kernel(RaggedPlaceParams p) {
    const long row = blockIdx.x;
    const int item = p.row_item[row];
    const RaggedItem it = p.items[item];
    place_row(p.c, row - it.row0, row * p.ldo, item, it.win0, it.nl_group, it.nl_count, it.global_row0, it.nl_first, it.nl_step);
}

}  // namespace hicom

using namespace hicom;

namespace {

// work units of an item with `ntiles` tiles: its share of 2 #CUs by tile count, rounded to nearest (a function of ntiles, the call's
// tile total and #CUs only: permuting the items permutes the division); `chunks` > 0 overrides the share
int ragged_chunks(long ntiles, long ntiles_sum, int chunks, int ncu) {
    long c = chunks > 0 ? chunks : (2L * ncu * ntiles + ntiles_sum / 2) / ntiles_sum;
    if (c > ntiles) c = ntiles;
    if (c > hicom_host::kSegMaxChunks) c = hicom_host::kSegMaxChunks;
    return (int)(c < 1 ? 1 : c);
}

struct RaggedLayout {
    long items, units, win_item, row_item, table_bytes;     // the table region
    long qp, qhi, qlo, pos_a, scores, part_m, part_l, part_acc, ctxg, o, pre, hid, tok, ctx16, hid16, loc, total;
    hicom_host::SegAdaptLayout ad;                          // behind the plain layout, whose offsets and total do not depend on it
    long tokens, windows, rows, score16, ntiles_sum, units_n;
    int max_T, wps;
};

inline long item_windows(const hicom_compressor_ragged_args* a, const hicom_ragged_item& it, int wps) { return (long)(it.T / it.kt) * wps; }

// ad: the k / v adaptors of the local stage, NULL for the plain recipe (hicom_compressor_ragged_*)
RaggedLayout ragged_layout(const hicom_compressor_ragged_args* a, const hicom_host::SegAdapt* ad) {
    RaggedLayout l{};
    const long B = a->B, E = a->E, HW = (long)a->H * a->W, R = B * a->nh;
    l.wps = (a->H / a->ks) * (a->W / a->ks);
    for (int i = 0; i < a->B; ++i) {
        const hicom_ragged_item& it = a->items[i];
        const long N = it.T * HW, w = item_windows(a, it, l.wps);
        l.tokens += N;
        l.windows += w;
        l.rows += w + it.nl_count + it.n_global_rows;
        l.score16 += (N + 15) / 16 * 16;
        l.ntiles_sum += (N + 15) / 16;
        if (it.T > l.max_T) l.max_T = it.T;
    }
    const int ncu = a->chunks > 0 ? 0 : hicom_host::num_cus();
    for (int i = 0; i < a->B; ++i) l.units_n += ragged_chunks((a->items[i].T * HW + 15) / 16, l.ntiles_sum, a->chunks, ncu);
    long off = 0;
    auto take = [&](long bytes) { const long at = off; off += (bytes + 255) / 256 * 256; return at; };
    const int odt = a->out_dt == HICOM_DT_F32 ? 4 : 2;
    l.items = take(B * (long)sizeof(RaggedItem));
    l.units = take(l.units_n * 16);
    l.win_item = take(l.windows * 4);
    l.row_item = take(l.rows * 4);
    l.table_bytes = off;
    l.qp = take(B * E * 4);
    l.qhi = take(R * E * 2);
    l.qlo = take(R * E * 2);
    l.pos_a = take(R * (long)(a->P > 0 ? a->P : 1) * 4);
    l.scores = take(16 * l.score16 * 4);
    l.part_m = take(l.units_n * 16 * 4);
    l.part_l = take(l.units_n * 16 * 4);
    l.part_acc = take(l.units_n * 16 * E * 4);
    l.ctxg = take(R * E * 4);
    l.o = take(B * E * 4);
    l.pre = take(B * E * 4);
    l.hid = take(B * (long)a->hidden * 4);
    l.tok = take(B * (long)a->hidden * 4);
    l.ctx16 = take(l.windows * E * 2);
    l.hid16 = take(l.windows * a->hidden * 2);
    l.loc = take(l.windows * a->hidden * odt);
    l.ad = hicom_host::seg_adapt_layout(ad, l.tokens, E, take);
    l.total = off;
    return l;
}

int ragged_check(const hicom_compressor_ragged_args* a, const hicom_host::SegAdapt* ad) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "compressor_ragged: NULL arguments");
    HICOM_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0 && a->hidden > 0 && a->ks > 0 && a->items, HICOM_EINVAL, "compressor_ragged: bad shape");
    HICOM_REQUIRE(a->B <= hicom_host::kSegMaxItems, HICOM_EUNSUP, "compressor_ragged: B=%d items (<= %d per call)", a->B, hicom_host::kSegMaxItems);
    HICOM_REQUIRE(a->E == 1152, HICOM_EUNSUP, "compressor_ragged: E=%d (only 1152)", a->E);
    HICOM_REQUIRE(a->nh > 0 && a->nh <= 16 && a->E % a->nh == 0, HICOM_EUNSUP, "compressor_ragged: %d heads (<= 16 folded rows per item)", a->nh);
    HICOM_REQUIRE(a->hidden % 64 == 0, HICOM_EUNSUP, "compressor_ragged: hidden=%d (multiple of 64: fp16 readout planes)", a->hidden);
    HICOM_REQUIRE(a->H % a->ks == 0 && a->W % a->ks == 0, HICOM_EUNSUP, "compressor_ragged: needs an exact window partition (H=%d W=%d, windows %dx%d)",
                  a->H, a->W, a->ks, a->ks);
    HICOM_REQUIRE(a->out_dt == HICOM_DT_BF16 || a->out_dt == HICOM_DT_F32, HICOM_EUNSUP, "compressor_ragged: output dtype %d (bf16 | f32)", a->out_dt);
    HICOM_REQUIRE(!a->pe == !a->kpe && (!a->pe || a->P > 0), HICOM_EINVAL, "compressor_ragged: pe and kpe come together");
    const int wps = (a->H / a->ks) * (a->W / a->ks);
    long tokens = 0;
    int max_T = 0;
    for (int i = 0; i < a->B; ++i) {
        const hicom_ragged_item& it = a->items[i];
        HICOM_REQUIRE(it.T > 0 && it.kt > 0 && it.n_global_rows > 0 && it.nl_group >= 0 && it.nl_count >= 0, HICOM_EINVAL, "compressor_ragged: item %d: bad shape", i);
        HICOM_REQUIRE(it.T % it.kt == 0, HICOM_EUNSUP, "compressor_ragged: item %d needs an exact window partition (T=%d, temporal window %d)", i, it.T, it.kt);
        HICOM_REQUIRE(it.kt * a->ks * a->ks <= 64, HICOM_EUNSUP, "compressor_ragged: item %d: windows of %d tokens (<= 64)", i, it.kt * a->ks * a->ks);
        HICOM_REQUIRE((long)it.T * a->H * a->W < (1L << 27), HICOM_EUNSUP, "compressor_ragged: item %d: too many tokens", i);
        const long w = item_windows(a, it, wps);
        HICOM_REQUIRE(!it.nl_group || w % it.nl_group == 0, HICOM_EINVAL, "compressor_ragged: item %d: output layout", i);
        HICOM_REQUIRE(it.nl_count == 0 || (it.nl_step > 0 && it.nl_first >= 0 && it.nl_first + (long)(it.nl_count - 1) * it.nl_step < w + it.nl_count),
                      HICOM_EINVAL, "compressor_ragged: item %d: newline rows", i);
        tokens += (long)it.T * a->H * a->W;
        if (it.T > max_T) max_T = it.T;
    }
    // (item offsets and the logits' offsets, 16 floats per token and one padded tile per item, are ints on the device)
    HICOM_REQUIRE(tokens + 16L * a->B < (1L << 27), HICOM_EUNSUP, "compressor_ragged: too many tokens in one call");
    HICOM_REQUIRE(((long)max_T * a->H + (long)max_T * a->W + max_T + a->H + a->W) * 4 <= 48 * 1024, HICOM_EUNSUP,
                  "compressor_ragged: T=%d frames of %dx%d: the merge keeps T (H + W) marginal sums in LDS", max_T, a->H, a->W);
    return hicom_host::seg_adapt_check("compressor_ragged", ad, tokens, a->E);
}

int ragged_check_ws(const hicom_compressor_ragged_args* a, const RaggedLayout& l) {
    HICOM_REQUIRE(a->ws && a->ws_bytes >= l.total && (uintptr_t)a->ws % 256 == 0, HICOM_EINVAL, "compressor_ragged: workspace of %ld bytes, 256-byte aligned",
                  l.total);
    return HICOM_OK;
}

int64_t ragged_workspace_bytes(const hicom_compressor_ragged_args* a, const hicom_host::SegAdapt* ad) {
    const int st = ragged_check(a, ad);
    if (st != HICOM_OK) return st;
    return ragged_layout(a, ad).total;
}

int ragged_prepare(const hicom_compressor_ragged_args* a, const hicom_host::SegAdapt* ad) {
    int st = ragged_check(a, ad);
    if (st != HICOM_OK) return st;
    const RaggedLayout l = ragged_layout(a, ad);
    st = ragged_check_ws(a, l);
    if (st != HICOM_OK) return st;
    std::vector<int> tab((size_t)(l.table_bytes / 4), 0);
    RaggedItem* items = reinterpret_cast<RaggedItem*>(tab.data() + l.items / 4);
    int* units = tab.data() + l.units / 4;
    int* win_item = tab.data() + l.win_item / 4;
    int* row_item = tab.data() + l.row_item / 4;
    const long HW = (long)a->H * a->W;
    const int ncu = a->chunks > 0 ? 0 : hicom_host::num_cus();
    long tok = 0, win = 0, row = 0, score = 0, slot = 0;
    for (int i = 0; i < a->B; ++i) {
        const hicom_ragged_item& h = a->items[i];
        const long N = h.T * HW, w = item_windows(a, h, l.wps), ntiles = (N + 15) / 16;
        const int chunks = ragged_chunks(ntiles, l.ntiles_sum, a->chunks, ncu);
        RaggedItem& d = items[i];
        d.tok0 = (int)tok; d.N = (int)N; d.T = h.T; d.kt = h.kt; d.win0 = (int)win; d.slot0 = (int)slot; d.chunks = chunks;
        d.score_off = (int)score; d.row0 = (int)row; d.global_row0 = (int)(w + h.nl_count);
        d.nl_group = h.nl_group; d.nl_count = h.nl_count; d.nl_first = h.nl_first; d.nl_step = h.nl_step > 0 ? h.nl_step : 1;
        for (int c = 0; c < chunks; ++c) {
            int* u = units + 4 * (slot + c);
            u[0] = i; u[1] = (int)(ntiles * c / chunks); u[2] = (int)(ntiles * (c + 1) / chunks); u[3] = (int)(slot + c);
        }
        const long rows = w + h.nl_count + h.n_global_rows;
        for (long k = 0; k < w; ++k) win_item[win + k] = i;
        for (long k = 0; k < rows; ++k) row_item[row + k] = i;
        tok += N; win += w; row += rows; score += ntiles * 16; slot += chunks;
    }
    hipStream_t s = (hipStream_t)a->stream;
    if (hipMemcpyAsync(a->ws, tab.data(), (size_t)l.table_bytes, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        hicom_host::set_error("compressor_ragged: writing the table region: %s", hipGetErrorString(hipGetLastError()));
        return HICOM_ELAUNCH;
    }
    return HICOM_OK;
}

int ragged_fwd(const hicom_compressor_ragged_args* a, const hicom_host::SegAdapt* ad) {
    int st = ragged_check(a, ad);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->ff && a->guide && a->out, HICOM_EINVAL, "compressor_ragged: NULL pointer");
    HICOM_REQUIRE(a->lw0_f16 && a->lw2_f16 && a->wq && a->wk && a->wv && a->wo && a->gw0 && a->gw2, HICOM_EINVAL, "compressor_ragged: NULL weight");
    st = hicom_host::seg_adapt_check_weights("compressor_ragged", ad);
    if (st != HICOM_OK) return st;
    const RaggedLayout l = ragged_layout(a, ad);
    st = ragged_check_ws(a, l);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE((uintptr_t)a->ff % 16 == 0 && (!a->fe || (uintptr_t)a->fe % 16 == 0) && (uintptr_t)a->guide % 16 == 0, HICOM_EINVAL,
                  "compressor_ragged: 16-byte aligned inputs");
    HICOM_REQUIRE(a->ldo >= a->hidden, HICOM_EINVAL, "compressor_ragged: output layout");
    for (int i = 0; i < a->B; ++i)
        HICOM_REQUIRE(a->items[i].nl_count == 0 || a->newline, HICOM_EINVAL, "compressor_ragged: item %d has newline rows and there is no newline token", i);
    char* ws = (char*)a->ws;
    hipStream_t s = (hipStream_t)a->stream;
    const int B = a->B, E = a->E, nh = a->nh, hd = E / nh, hidden = a->hidden;
    const RaggedItem* items = (const RaggedItem*)(ws + l.items);
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

    // 3: local stage over the concatenated window list (adaptor recipe: the two layers of the adaptor MLPs over all tokens in front of it)
    {
        const hicom_axis ay{a->H, a->ks, a->H / a->ks, a->H / a->ks}, ax{a->W, a->ks, a->W / a->ks, a->W / a->ks};
        const uint16_t* key_x = (const uint16_t*)(a->fe ? a->fe : a->ff);
        if (ad) {
            st = hicom_host::seg_adapt_mlps(*ad, key_x, a->ff, l.tokens, E, ws, l.ad, a->stream);
            if (st != HICOM_OK) return st;
            HICOM_LAUNCH(ragged_local_attn_adapt_kernel<3>, dim3((unsigned)((l.windows + 3) / 4)), dim3(256), 0, s, key_x, (const uint16_t*)a->ff,
                         (const uint16_t*)a->guide, hicom_host::seg_adapt_params(*ad, ws, l.ad), items, (const int*)(ws + l.win_item), ay, ax,
                         (int)l.windows, a->l_scale, (_Float16*)(ws + l.ctx16));
        } else {
            HICOM_LAUNCH(ragged_local_attn_kernel<3>, dim3((unsigned)((l.windows + 3) / 4)), dim3(256), 0, s, key_x, (const uint16_t*)a->ff,
                         (const uint16_t*)a->guide, items, (const int*)(ws + l.win_item), ay, ax, (int)l.windows, a->l_scale,
                         (_Float16*)(ws + l.ctx16));
        }
        st = hicom_host::check_launch("compressor_ragged: local stage");
        if (st != HICOM_OK) return st;
    }

    // 4: segmented global stream over the work units
    {
        RaggedStreamParams p;
        p.x = (const uint16_t*)a->ff;
        p.c.qhi = (const uint16_t*)(ws + l.qhi); p.c.qlo = (const uint16_t*)(ws + l.qlo);
        p.c.pos_a = pos_a; p.c.pos_stride = a->P; p.c.rows = nh;
        p.c.H = a->H; p.c.W = a->W; p.c.HW = a->H * a->W;
        p.c.t0i = a->t_index0; p.c.y0i = a->y_index0; p.c.x0i = a->x_index0;
        p.scores = (float*)(ws + l.scores);
        p.c.part_m = (float*)(ws + l.part_m); p.c.part_l = (float*)(ws + l.part_l); p.c.part_acc = (float*)(ws + l.part_acc);
        p.units = (const int4*)(ws + l.units); p.items = items;
        constexpr int smem = hicom_host::kSegStreamSmem;
        static bool attr_set = false;
        if (!attr_set) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(ragged_global_stream_kernel<9>), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
            attr_set = true;
        }
        HICOM_LAUNCH(ragged_global_stream_kernel<9>, dim3((unsigned)l.units_n), dim3(256), smem, s, p);
        st = hicom_host::check_launch("compressor_ragged: global stream");
        if (st != HICOM_OK) return st;
    }

    // 5: merge per item
    {
        RaggedMergeParams p;
        p.c.part_m = (const float*)(ws + l.part_m); p.c.part_l = (const float*)(ws + l.part_l); p.c.part_acc = (const float*)(ws + l.part_acc);
        p.scores = (const float*)(ws + l.scores);
        p.c.pe = a->pe; p.rows = nh; p.c.E = E; p.c.H = a->H; p.c.W = a->W;
        p.c.t0i = a->t_index0; p.c.y0i = a->y_index0; p.c.x0i = a->x_index0;
        p.items = items;
        p.ctx = ctxg;
        const size_t smem = ((size_t)l.max_T * a->H + (size_t)l.max_T * a->W + l.max_T + a->H + a->W) * 4;
        HICOM_LAUNCH(ragged_merge_kernel, dim3((unsigned)nh, (unsigned)B), dim3(256), smem, s, p);
        st = hicom_host::check_launch("compressor_ragged: merge");
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
    st = hicom_readout16_gemm_fwd(ws + l.ctx16, a->lw0_f16, a->lb0, HICOM_DT_BF16, (int)l.windows, hidden, E, HICOM_ACT_GELU, ws + l.hid16, nullptr, 0, 0, 0, 0,
                                  nullptr, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_readout16_gemm_fwd(ws + l.hid16, a->lw2_f16, a->lb2, HICOM_DT_BF16, (int)l.windows, hidden, hidden, HICOM_ACT_NONE, nullptr, ws + l.loc, a->out_dt,
                                  hidden, 0, 0, nullptr, a->stream);
    if (st != HICOM_OK) return st;

    // 12: every item's packed rows
    {
        RaggedPlaceParams p;
        p.c.loc = ws + l.loc; p.c.tok = tok; p.c.newline = (const uint16_t*)a->newline; p.c.out = a->out;
        p.c.out_f32 = a->out_dt == HICOM_DT_F32; p.c.hidden = hidden;
        p.items = items; p.row_item = (const int*)(ws + l.row_item); p.ldo = a->ldo;
        HICOM_LAUNCH(ragged_place_kernel, dim3((unsigned)l.rows), dim3(128), 0, s, p);
        st = hicom_host::check_launch("compressor_ragged: placement");
    }
    return st;
}

}  // namespace

extern "C" int64_t hicom_compressor_ragged_workspace_bytes(const hicom_compressor_ragged_args* a) { return ragged_workspace_bytes(a, nullptr); }

extern "C" int hicom_compressor_ragged_prepare(const hicom_compressor_ragged_args* a) { return ragged_prepare(a, nullptr); }

extern "C" int hicom_compressor_ragged_fwd(const hicom_compressor_ragged_args* a) { return ragged_fwd(a, nullptr); }

// ---- the adaptor recipe: the same step with the k / v adaptors on the local stage; the table region is the plain one ----------------
extern "C" int64_t hicom_compressor_ragged_adapt_workspace_bytes(const hicom_compressor_ragged_adapt_args* a) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "compressor_ragged: NULL arguments");
    const hicom_host::SegAdapt ad{&a->ak, &a->av, a->alpha_dt, a->eps};
    return ragged_workspace_bytes(&a->base, &ad);
}

extern "C" int hicom_compressor_ragged_adapt_prepare(const hicom_compressor_ragged_adapt_args* a) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "compressor_ragged: NULL arguments");
    const hicom_host::SegAdapt ad{&a->ak, &a->av, a->alpha_dt, a->eps};
    return ragged_prepare(&a->base, &ad);
}

extern "C" int hicom_compressor_ragged_adapt_fwd(const hicom_compressor_ragged_adapt_args* a) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "compressor_ragged: NULL arguments");
    const hicom_host::SegAdapt ad{&a->ak, &a->av, a->alpha_dt, a->eps};
    return ragged_fwd(&a->base, &ad);
}
