// Ragged compressor step: B items of unequal length and mixed modality (single images, clips of any length, 1-frame "videos") read in
// place from the vision tower's stacked [sum T_i, H, W, E] tensor, through the launch sequence of the batched step (twelve launches,
// fourteen with the k / v adaptors; the sequence, the workspace regions behind the tables and the common checks: segment_host.hpp).
//
// What is this file's own is where a wave or workgroup learns its item.  batch.hip divides by a constant stride; here a table region
// at the head of the workspace says it (hicom_compressor_ragged_prepare derives it on the host, once per plan):
//   * item table, one RaggedItem per item: first token, token count, T, kt, first window, first output row, the layout integers of
//     its packed rows, where its logits and partial states live and how many work units stream it;
//   * work units {item, first tile, last tile, partial-state slot} of the segmented stream: a 1-D grid, one workgroup per unit.
//     Tiles are counted from the ITEM's first token (item offsets are 36, 180, 216 ... tokens: no multiple of a tile), a unit never
//     spans two items, and item i gets chunks_i ~ 2 #CUs ntiles_i / sum ntiles of them, in [1, min(ntiles_i, 64)];
//   * window -> item and output row -> item lookups (one int each) for the local stage and the placement.
// The stacked tensor is not one window grid (kt differs between neighbours), so the local stage builds each window's geometry from its
// item's own (T, kt) and offsets the token index by the item's first token.  The four lookups are wave-uniform loads through a
// kernel-argument pointer with a uniform index: they land in SGPRs.  hicom_compressor_ragged_fwd only launches.  The stream is
// stream_segment (stream_body.hpp: the one body of the four-wave stream machine, also behind hicom_global_stream_fwd's narrow kernel)
// with one row group; the per-item requirements, the chunk share, the tile ranges and the table upload
// are segment_host.hpp's, shared with ragged_multi_guide.hip.  The item record, the item walk of a window, the shape checks and the
// layout are ragged_host.hpp's, shared with the training surface of this step (ragged_train.hip).
#include <vector>

#include "multi_window.hpp"
#include "ragged_host.hpp"

namespace hicom {

// ---- 3: local stage, one wave per window of the concatenated window list ----
template <int NV>
__global__ __launch_bounds__(256) void ragged_local_attn_kernel(const uint16_t* key, const uint16_t* value, const uint16_t* guide,
                                                                const RaggedItem* items, const int* win_item, hicom_axis ay, hicom_axis ax,
                                                                int nwin, float scale, _Float16* ctx16) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const RaggedWindow w(items, win_item, ay, ax, win, D);
    local_window_ctx16<NV>(key + w.first, value + w.first, guide + (long)w.item * D, w.geom, lane, scale, ctx16 + (long)win * D);
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
    const RaggedWindow w(items, win_item, ay, ax, win, D);
    local_window_adapt_ctx16<NV>(key + w.first, ad.ky ? ad.ky + w.first : nullptr, value + w.first, ad.vy ? ad.vy + w.first : nullptr, ad,
                                 guide + (long)w.item * D, w.geom, lane, scale, ctx16 + (long)win * D);
}

// ... and the logits form: the same wave -> window -> item map with the raw scores key_n . guide_item given, f32 [sum N_i]
// over the stacked tokens (one guide per item: token n of item i at tok0_i + n).  Lane i fetches the score of the window's token i; no key
// row and no guide row is read (multi_window.hpp: multi_window_logits_ctx16 with one guide)
template <int NV>
__global__ __launch_bounds__(256) void ragged_local_logits_kernel(const uint16_t* value, const float* logits, const RaggedItem* items, const int* win_item,
                                                                  hicom_axis ay, hicom_axis ax, int nwin, float scale, _Float16* ctx16) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const RaggedWindow w(items, win_item, ay, ax, win, D);
    multi_window_logits_ctx16<NV, 1>(value + w.first, logits + w.it.tok0, 0, w.geom, lane, scale, ctx16 + (long)win * D, 0);
}

// ---- 4: segmented global stream, one workgroup per work unit (one row group: the item's nh rows) ----
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
    stream_segment<NB, 1>(p.c, p.x + (long)tok0 * E, N, u.y, u.z, 0, p.c.rows, (long)u.x * p.c.rows, p.scores + (long)soff * 16, (long)((N + 15) / 16 * 16),
                          (long)u.w, 0);
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
using namespace hicom_host;

namespace {

constexpr const char* kWho = "compressor_ragged";

int64_t ragged_workspace_bytes(const hicom_compressor_ragged_args* a, const SegAdapt* ad) {
    HICOM_TRY(ragged_check(a, ad));
    return ragged_layout(a, ad).s.total;
}

int ragged_prepare(const hicom_compressor_ragged_args* a, const SegAdapt* ad) {
    HICOM_TRY(ragged_check(a, ad));
    const RaggedLayout l = ragged_layout(a, ad);
    HICOM_TRY(seg_check_ws(kWho, a, l.s.total));
    std::vector<int> tab((size_t)(l.table_bytes / 4), 0);
    RaggedItem* items = reinterpret_cast<RaggedItem*>(tab.data() + l.items / 4);
    int* units = tab.data() + l.units / 4;
    int* win_item = tab.data() + l.win_item / 4;
    int* row_item = tab.data() + l.row_item / 4;
    const long HW = (long)a->H * a->W;
    const int ncu = a->chunks > 0 ? 0 : num_cus();
    long tok = 0, win = 0, row = 0, score = 0, slot = 0;
    for (int i = 0; i < a->B; ++i) {
        const hicom_ragged_item& h = a->items[i];
        const long N = h.T * HW, w = item_windows(h, l.wps), ntiles = (N + 15) / 16;
        const int chunks = seg_share_chunks(ntiles, l.ntiles_sum, a->chunks, ncu);
        RaggedItem& d = items[i];
        d.tok0 = (int)tok; d.N = (int)N; d.T = h.T; d.kt = h.kt; d.win0 = (int)win; d.slot0 = (int)slot; d.chunks = chunks;
        d.score_off = (int)score; d.row0 = (int)row; d.global_row0 = (int)(w + h.nl_count);
        d.nl_group = h.nl_group; d.nl_count = h.nl_count; d.nl_first = h.nl_first; d.nl_step = h.nl_step > 0 ? h.nl_step : 1;
        for (int c = 0; c < chunks; ++c) {
            int* u = units + 4 * (slot + c);
            u[0] = i; u[1] = seg_tile_at(ntiles, c, chunks); u[2] = seg_tile_at(ntiles, c + 1, chunks); u[3] = (int)(slot + c);
        }
        const long rows = w + h.nl_count + h.n_global_rows;
        for (long k = 0; k < w; ++k) win_item[win + k] = i;
        for (long k = 0; k < rows; ++k) row_item[row + k] = i;
        tok += N; win += w; row += rows; score += ntiles * 16; slot += chunks;
    }
    return seg_upload_tables(kWho, a, tab.data(), l.table_bytes);
}

// the four launches that look their item up in the table region (segment_host.hpp: seg_step)
struct RaggedItems {
    const hicom_compressor_ragged_args* a;
    const RaggedLayout& l;
    const float* logits;        // the logits form: f32 [sum N_i], no key row is read; NULL: the keyed forms
    char* ws() const { return (char*)a->ws; }
    hipStream_t s() const { return (hipStream_t)a->stream; }
    const RaggedItem* items() const { return (const RaggedItem*)(ws() + l.items); }

    int local(const uint16_t* key_x, const SegAdaptParams* ad) const {
        const long windows = l.s.n.windows;
        const RaggedAxes g = ragged_axes(a);
        if (logits)
            HICOM_LAUNCH(ragged_local_logits_kernel<3>, dim3((unsigned)((windows + 3) / 4)), dim3(256), 0, s(), (const uint16_t*)a->ff, logits, items(),
                         (const int*)(ws() + l.win_item), g.ay, g.ax, (int)windows, a->l_scale, (_Float16*)(ws() + l.s.ctx16));
        else if (ad)
            HICOM_LAUNCH(ragged_local_attn_adapt_kernel<3>, dim3((unsigned)((windows + 3) / 4)), dim3(256), 0, s(), key_x, (const uint16_t*)a->ff,
                         (const uint16_t*)a->guide, *ad, items(), (const int*)(ws() + l.win_item), g.ay, g.ax, (int)windows, a->l_scale,
                         (_Float16*)(ws() + l.s.ctx16));
        else
            HICOM_LAUNCH(ragged_local_attn_kernel<3>, dim3((unsigned)((windows + 3) / 4)), dim3(256), 0, s(), key_x, (const uint16_t*)a->ff,
                         (const uint16_t*)a->guide, items(), (const int*)(ws() + l.win_item), g.ay, g.ax, (int)windows, a->l_scale,
                         (_Float16*)(ws() + l.s.ctx16));
        return seg_check_launch(kWho, "local stage");
    }

    int stream(const SegStreamParams& c) const {
        RaggedStreamParams p;
        p.c = c;
        p.x = (const uint16_t*)a->ff;
        p.scores = (float*)(ws() + l.s.scores);
        p.units = (const int4*)(ws() + l.units); p.items = items();
        static bool attr_set = false;
        if (!attr_set) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(ragged_global_stream_kernel<9>), hipFuncAttributeMaxDynamicSharedMemorySize, seg_stream_smem(1));
            attr_set = true;
        }
        HICOM_LAUNCH(ragged_global_stream_kernel<9>, dim3((unsigned)l.s.n.slots), dim3(256), seg_stream_smem(1), s(), p);
        return seg_check_launch(kWho, "global stream");
    }

    int merge(const SegMergeParams& c) const {
        RaggedMergeParams p;
        p.c = c;
        p.scores = (const float*)(ws() + l.s.scores);
        p.items = items(); p.rows = a->nh;
        p.ctx = (float*)(ws() + l.s.ctxg);
        HICOM_LAUNCH(ragged_merge_kernel, dim3((unsigned)a->nh, (unsigned)a->B), dim3(256), (size_t)seg_merge_smem(l.max_T, a->H, a->W), s(), p);
        return seg_check_launch(kWho, "merge");
    }

    int place(const SegPlaceParams& c) const {
        RaggedPlaceParams p;
        p.c = c;
        p.items = items(); p.row_item = (const int*)(ws() + l.row_item); p.ldo = a->ldo;
        HICOM_LAUNCH(ragged_place_kernel, dim3((unsigned)l.rows), dim3(128), 0, s(), p);
        return seg_check_launch(kWho, "placement");
    }
};

// logits: the logits form (plain recipe only): launch 3 is ragged_local_logits_kernel, a->fe is not looked at
int ragged_fwd_form(const hicom_compressor_ragged_args* a, const SegAdapt* ad, const float* logits) {
    HICOM_TRY(ragged_check(a, ad));
    hicom_compressor_ragged_args keyless;
    if (logits) {
        keyless = *a;
        keyless.fe = nullptr;
        a = &keyless;
    }
    const RaggedLayout l = ragged_layout(a, ad);
    HICOM_TRY(seg_check_fwd(kWho, a, ad, l.s.total));
    HICOM_REQUIRE(a->ldo >= a->hidden, HICOM_EINVAL, "compressor_ragged: output layout");
    for (int i = 0; i < a->B; ++i)
        HICOM_REQUIRE(a->items[i].nl_count == 0 || a->newline, HICOM_EINVAL, "compressor_ragged: item %d has newline rows and there is no newline token", i);
    return seg_step(a, ad, l.s, RaggedItems{a, l, logits});
}

int ragged_fwd(const hicom_compressor_ragged_args* a, const SegAdapt* ad) { return ragged_fwd_form(a, ad, nullptr); }

}  // namespace

extern "C" int64_t hicom_compressor_ragged_workspace_bytes(const hicom_compressor_ragged_args* a) { return ragged_workspace_bytes(a, nullptr); }

extern "C" int hicom_compressor_ragged_prepare(const hicom_compressor_ragged_args* a) { return ragged_prepare(a, nullptr); }

extern "C" int hicom_compressor_ragged_fwd(const hicom_compressor_ragged_args* a) { return ragged_fwd(a, nullptr); }

// The logits form: a->fe is not read (the plan, the workspace, its size function and the prepare call are the keyed step's).
extern "C" int hicom_compressor_ragged_logits_fwd(const hicom_compressor_ragged_args* a, const float* local_logits) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "%s: NULL arguments", kWho);
    HICOM_REQUIRE(local_logits && (uintptr_t)local_logits % 4 == 0, HICOM_EINVAL, "%s: local_logits is f32 [sum T_i H W]", kWho);
    return ragged_fwd_form(a, nullptr, local_logits);
}

// ---- the adaptor recipe: the same step with the k / v adaptors on the local stage; the table region is the plain one ----------------
extern "C" int64_t hicom_compressor_ragged_adapt_workspace_bytes(const hicom_compressor_ragged_adapt_args* a) { return seg_with_adapt(kWho, a, ragged_workspace_bytes); }

extern "C" int hicom_compressor_ragged_adapt_prepare(const hicom_compressor_ragged_adapt_args* a) { return seg_with_adapt(kWho, a, ragged_prepare); }

extern "C" int hicom_compressor_ragged_adapt_fwd(const hicom_compressor_ragged_adapt_args* a) { return seg_with_adapt(kWho, a, ragged_fwd); }
