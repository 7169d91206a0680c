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
// are segment_host.hpp's, shared with ragged_multi_guide.hip.
// Training (plain recipe, hicom_amd/ragged_train.py): hicom_compressor_ragged_train_state hands the forward's state out of the workspace,
// hicom_compressor_ragged_global_bwd runs the global stage's attention backward over all items on the forward's unit table -- the same
// stream_segment in StreamMode::Bwd, then dq_merge_segments per (item, head).
#include <vector>

#include "segment_host.hpp"

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

// ---- training: (M, L) per (item, head) from the partial states, merge_segments' own order.  grid = B, 64 threads ----
__global__ __launch_bounds__(64) void ragged_state_ml_kernel(const float* part_m, const float* part_l, const RaggedItem* items, int rows, float* ml) {
    const int item = blockIdx.x, r = threadIdx.x;
    if (r >= rows) return;
    const RaggedItem it = items[item];
    const long pbase = (long)it.slot0 * 16 + r;
    float M = -1.0e30f;
    for (int c = 0; c < it.chunks; ++c) M = fmaxf(M, part_m[pbase + c * 16]);
    float L = 0.f;
    for (int c = 0; c < it.chunks; ++c) L += part_l[pbase + c * 16] * expf(part_m[pbase + c * 16] - M);
    ml[2 * ((long)item * rows + r)] = M;
    ml[2 * ((long)item * rows + r) + 1] = L;
}

// ---- training: the segmented backward of the global stream, the forward's unit table and slots (stream_body.hpp: StreamMode::Bwd).
// c.qhi / c.qlo: the planes of dctx, c.pos_a: pos_b = dctx . pe^T, c.part_acc: partial sums of dS x; part_m / part_l are not written ----
struct RaggedStreamBwdParams {
    SegStreamParams c;
    const uint16_t* x;      // [sum N_i][E]
    const float* s_in;      // the forward's scores region
    const float* ml;        // [B * rows][2]
    const float* delta;     // [B * rows]
    float* ds;              // laid out as s_in
    const int4* units;
    const RaggedItem* items;
};

template <int NB>
__global__ __launch_bounds__(256, 2) void ragged_global_stream_bwd_kernel(RaggedStreamBwdParams p) {
    constexpr int E = NB * 128;
    const int4 u = p.units[blockIdx.x];
    const int N = p.items[u.x].N, tok0 = p.items[u.x].tok0, soff = p.items[u.x].score_off;
    StreamModeArgs ma{};
    ma.s_in = p.s_in + (long)soff * 16;
    ma.ml = p.ml + 2 * (long)u.x * p.c.rows;
    ma.delta = p.delta + (long)u.x * p.c.rows;
    stream_segment<NB, 1, StreamMode::Bwd>(p.c, p.x + (long)tok0 * E, N, u.y, u.z, 0, p.c.rows, (long)u.x * p.c.rows, p.ds + (long)soff * 16,
                                           (long)((N + 15) / 16 * 16), (long)u.w, 0, ma);
}

// ---- training: dq merge per (item, head), grid = (rows, B), the forward merge's LDS ----
struct RaggedDqMergeParams {
    SegDqMergeParams c;
    const float* ds;
    const RaggedItem* items;
    int rows;
    float* dqt;             // [B * rows][E]
};

__global__ __launch_bounds__(256) void ragged_dq_merge_kernel(RaggedDqMergeParams p) {
    extern __shared__ float ms[];
    const int r = blockIdx.x, item = blockIdx.y;
    const RaggedItem it = p.items[item];
    const long stride = (it.N + 15) / 16 * 16;
    dq_merge_segments(p.c, ms, r, threadIdx.x, it.T, it.chunks, (long)it.slot0, p.ds + (long)it.score_off * 16 + r * stride,
                      p.dqt + ((long)item * p.rows + r) * p.c.E);
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

struct RaggedLayout {
    long items, units, win_item, row_item, table_bytes;     // the table region, in front of the step's own regions
    SegLayout s;
    long rows, ntiles_sum;
    int max_T, wps;
};

// ad: the k / v adaptors of the local stage, NULL for the plain recipe (hicom_compressor_ragged_*)
RaggedLayout ragged_layout(const hicom_compressor_ragged_args* a, const SegAdapt* ad) {
    RaggedLayout l{};
    SegTotals n{};
    const long HW = (long)a->H * a->W;
    l.wps = (a->H / a->ks) * (a->W / a->ks);
    for (int i = 0; i < a->B; ++i) {
        const hicom_ragged_item& it = a->items[i];
        const long N = it.T * HW, w = item_windows(it, l.wps);
        n.tokens += N;
        n.windows += w;
        l.rows += w + it.nl_count + it.n_global_rows;
        n.score_floats += 16 * ((N + 15) / 16 * 16);
        l.ntiles_sum += (N + 15) / 16;
        if (it.T > l.max_T) l.max_T = it.T;
    }
    const int ncu = a->chunks > 0 ? 0 : num_cus();
    for (int i = 0; i < a->B; ++i) n.slots += seg_share_chunks((a->items[i].T * HW + 15) / 16, l.ntiles_sum, a->chunks, ncu);
    n.rows = (long)a->B * a->nh;
    n.part_rows = n.slots * 16;
    long off = 0;
    auto take = [&](long bytes) { const long at = off; off += (bytes + 255) / 256 * 256; return at; };
    l.items = take(a->B * (long)sizeof(RaggedItem));
    l.units = take(n.slots * 16);
    l.win_item = take(n.windows * 4);
    l.row_item = take(l.rows * 4);
    l.table_bytes = off;
    l.s = seg_layout(a, ad, n, off);
    return l;
}

int ragged_check(const hicom_compressor_ragged_args* a, const SegAdapt* ad) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "compressor_ragged: NULL arguments");
    HICOM_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0 && a->hidden > 0 && a->ks > 0 && a->items, HICOM_EINVAL, "compressor_ragged: bad shape");
    int st = seg_check_items_shape(kWho, a);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->H % a->ks == 0 && a->W % a->ks == 0, HICOM_EUNSUP, "compressor_ragged: needs an exact window partition (H=%d W=%d, windows %dx%d)",
                  a->H, a->W, a->ks, a->ks);
    long tokens;
    int max_T;
    st = seg_check_ragged_items(kWho, a, tokens, max_T, [](int) { return HICOM_OK; });
    if (st != HICOM_OK) return st;
    // (item offsets and the logits' offsets, 16 floats per token and one padded tile per item, are ints on the device)
    HICOM_REQUIRE(tokens + 16L * a->B < (1L << 27), HICOM_EUNSUP, "compressor_ragged: too many tokens in one call");
    st = seg_check_merge_lds(kWho, a, max_T);
    if (st != HICOM_OK) return st;
    return seg_adapt_check(kWho, ad, tokens, a->E);
}

int64_t ragged_workspace_bytes(const hicom_compressor_ragged_args* a, const SegAdapt* ad) {
    const int st = ragged_check(a, ad);
    if (st != HICOM_OK) return st;
    return ragged_layout(a, ad).s.total;
}

int ragged_prepare(const hicom_compressor_ragged_args* a, const SegAdapt* ad) {
    int st = ragged_check(a, ad);
    if (st != HICOM_OK) return st;
    const RaggedLayout l = ragged_layout(a, ad);
    st = seg_check_ws(kWho, a, l.s.total);
    if (st != HICOM_OK) return st;
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
    char* ws() const { return (char*)a->ws; }
    hipStream_t s() const { return (hipStream_t)a->stream; }
    const RaggedItem* items() const { return (const RaggedItem*)(ws() + l.items); }

    int local(const uint16_t* key_x, const SegAdaptParams* ad) const {
        const long windows = l.s.n.windows;
        const hicom_axis ay{a->H, a->ks, a->H / a->ks, a->H / a->ks}, ax{a->W, a->ks, a->W / a->ks, a->W / a->ks};
        if (ad)
            HICOM_LAUNCH(ragged_local_attn_adapt_kernel<3>, dim3((unsigned)((windows + 3) / 4)), dim3(256), 0, s(), key_x, (const uint16_t*)a->ff,
                         (const uint16_t*)a->guide, *ad, items(), (const int*)(ws() + l.win_item), ay, ax, (int)windows, a->l_scale,
                         (_Float16*)(ws() + l.s.ctx16));
        else
            HICOM_LAUNCH(ragged_local_attn_kernel<3>, dim3((unsigned)((windows + 3) / 4)), dim3(256), 0, s(), key_x, (const uint16_t*)a->ff,
                         (const uint16_t*)a->guide, items(), (const int*)(ws() + l.win_item), ay, ax, (int)windows, a->l_scale,
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

int ragged_fwd(const hicom_compressor_ragged_args* a, const SegAdapt* ad) {
    int st = ragged_check(a, ad);
    if (st != HICOM_OK) return st;
    const RaggedLayout l = ragged_layout(a, ad);
    st = seg_check_fwd(kWho, a, ad, l.s.total);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->ldo >= a->hidden, HICOM_EINVAL, "compressor_ragged: output layout");
    for (int i = 0; i < a->B; ++i)
        HICOM_REQUIRE(a->items[i].nl_count == 0 || a->newline, HICOM_EINVAL, "compressor_ragged: item %d has newline rows and there is no newline token", i);
    return seg_step(a, ad, l.s, RaggedItems{a, l});
}

// ---- training (plain recipe): the state a backward reads, and the global stage's attention backward ---------------------------------
constexpr const char* kWhoBwd = "compressor_ragged_global_bwd";

struct RaggedBwdLayout { long dhi, dlo, pos_b, part_acc, total; };

RaggedBwdLayout ragged_bwd_layout(const hicom_compressor_ragged_args* a, const RaggedLayout& l) {
    RaggedBwdLayout b{};
    long off = 0;
    auto take = [&](long bytes) { const long at = off; off += (bytes + 255) / 256 * 256; return at; };
    const long R = l.s.n.rows, E = a->E;
    b.dhi = take(R * E * 2);
    b.dlo = take(R * E * 2);
    b.pos_b = take(a->pe ? R * (long)a->P * 4 : 0);
    b.part_acc = take(l.s.n.part_rows * E * 4);
    b.total = off;
    return b;
}

int ragged_train_state(const hicom_compressor_ragged_args* a, void* ctx16_out, float* scores_out, float* ml_out, float* ctxg_out) {
    constexpr const char* who = "compressor_ragged_train_state";
    int st = ragged_check(a, nullptr);
    if (st != HICOM_OK) return st;
    const RaggedLayout l = ragged_layout(a, nullptr);
    st = seg_check_ws(who, a, l.s.total);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(ctx16_out && scores_out && ml_out && ctxg_out, HICOM_EINVAL, "%s: NULL pointer", who);
    const char* ws = (const char*)a->ws;
    hipStream_t s = (hipStream_t)a->stream;
    const long E = a->E;
    if (hipMemcpyAsync(ctx16_out, ws + l.s.ctx16, (size_t)(l.s.n.windows * E * 2), hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(scores_out, ws + l.s.scores, (size_t)(l.s.n.score_floats * 4), hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(ctxg_out, ws + l.s.ctxg, (size_t)(l.s.n.rows * E * 4), hipMemcpyDeviceToDevice, s) != hipSuccess) {
        set_error("%s: copying the state: %s", who, hipGetErrorString(hipGetLastError()));
        return HICOM_ELAUNCH;
    }
    HICOM_LAUNCH(ragged_state_ml_kernel, dim3((unsigned)a->B), dim3(64), 0, s, (const float*)(ws + l.s.part_m), (const float*)(ws + l.s.part_l),
                 (const RaggedItem*)(ws + l.items), a->nh, ml_out);
    return seg_check_launch(who, "softmax state");
}

int64_t ragged_global_bwd_workspace_bytes(const hicom_compressor_ragged_args* a) {
    const int st = ragged_check(a, nullptr);
    if (st != HICOM_OK) return st;
    return ragged_bwd_layout(a, ragged_layout(a, nullptr)).total;
}

int ragged_global_bwd(const hicom_compressor_ragged_args* a, const void* x, const float* dctx, const float* delta, const float* scores, const float* ml,
                      float* ds_out, float* dqt_out, void* bws, int64_t bws_bytes) {
    int st = ragged_check(a, nullptr);
    if (st != HICOM_OK) return st;
    const RaggedLayout l = ragged_layout(a, nullptr);
    st = seg_check_ws(kWhoBwd, a, l.s.total);                 // (the table region at its head is what is read)
    if (st != HICOM_OK) return st;
    const RaggedBwdLayout b = ragged_bwd_layout(a, l);
    HICOM_REQUIRE(x && dctx && delta && scores && ml && ds_out && dqt_out, HICOM_EINVAL, "%s: NULL pointer", kWhoBwd);
    HICOM_REQUIRE(bws && bws_bytes >= b.total && (uintptr_t)bws % 256 == 0, HICOM_EINVAL, "%s: workspace of %ld bytes, 256-byte aligned", kWhoBwd, b.total);
    HICOM_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)scores % 16 == 0 && (uintptr_t)ds_out % 16 == 0 && (uintptr_t)dctx % 16 == 0, HICOM_EINVAL,
                  "%s: 16-byte aligned inputs", kWhoBwd);
    HICOM_REQUIRE(ds_out != scores, HICOM_EINVAL, "%s: dS cannot overwrite the logits", kWhoBwd);
    char* w = (char*)bws;
    const char* tab = (const char*)a->ws;
    const int R = (int)l.s.n.rows, E = a->E;
    hipStream_t s = (hipStream_t)a->stream;

    // 1: dctx -> bf16 hi / lo planes
    st = hicom_split_bf16_fwd(dctx, R, R, E, w + b.dhi, w + b.dlo, a->stream);
    if (st != HICOM_OK) return st;
    // 2: the score-side positional table of dP
    float* pos_b = a->pe ? (float*)(w + b.pos_b) : nullptr;
    if (a->pe) {
        st = hicom_linear_fwd(dctx, HICOM_DT_F32, a->pe, HICOM_DT_F32, nullptr, 0, nullptr, 0, R, a->P, E, 0, 0, HICOM_ACT_NONE, pos_b, a->stream);
        if (st != HICOM_OK) return st;
    }
    // 3: the segmented backward stream
    {
        RaggedStreamBwdParams p;
        p.c.qhi = (const uint16_t*)(w + b.dhi); p.c.qlo = (const uint16_t*)(w + b.dlo);
        p.c.pos_a = pos_b; p.c.pos_stride = a->P; p.c.rows = a->nh;
        p.c.H = a->H; p.c.W = a->W; p.c.HW = a->H * a->W;
        p.c.t0i = a->t_index0; p.c.y0i = a->y_index0; p.c.x0i = a->x_index0;
        p.c.part_m = nullptr; p.c.part_l = nullptr; p.c.part_acc = (float*)(w + b.part_acc);
        p.x = (const uint16_t*)x; p.s_in = scores; p.ml = ml; p.delta = delta; p.ds = ds_out;
        p.units = (const int4*)(tab + l.units); p.items = (const RaggedItem*)(tab + l.items);
        static bool attr_set = false;
        if (!attr_set) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(ragged_global_stream_bwd_kernel<9>), hipFuncAttributeMaxDynamicSharedMemorySize, seg_stream_smem(1));
            attr_set = true;
        }
        HICOM_LAUNCH(ragged_global_stream_bwd_kernel<9>, dim3((unsigned)l.s.n.slots), dim3(256), seg_stream_smem(1), s, p);
        st = seg_check_launch(kWhoBwd, "backward stream");
        if (st != HICOM_OK) return st;
    }
    // 4: dq merge per (item, head)
    RaggedDqMergeParams p;
    p.c.part_acc = (const float*)(w + b.part_acc); p.c.pe = a->pe; p.c.E = E; p.c.H = a->H; p.c.W = a->W;
    p.c.t0i = a->t_index0; p.c.y0i = a->y_index0; p.c.x0i = a->x_index0;
    p.ds = ds_out; p.items = (const RaggedItem*)(tab + l.items); p.rows = a->nh; p.dqt = dqt_out;
    HICOM_LAUNCH(ragged_dq_merge_kernel, dim3((unsigned)a->nh, (unsigned)a->B), dim3(256), (size_t)seg_merge_smem(l.max_T, a->H, a->W), s, p);
    return seg_check_launch(kWhoBwd, "dq merge");
}

}  // namespace

extern "C" int hicom_compressor_ragged_train_state(const hicom_compressor_ragged_args* a, void* ctx16_out, float* scores_out, float* ml_out, float* ctxg_out) {
    return ragged_train_state(a, ctx16_out, scores_out, ml_out, ctxg_out);
}

extern "C" int64_t hicom_compressor_ragged_global_bwd_workspace_bytes(const hicom_compressor_ragged_args* a) { return ragged_global_bwd_workspace_bytes(a); }

extern "C" int hicom_compressor_ragged_global_bwd(const hicom_compressor_ragged_args* a, const void* x, const float* dctx, const float* delta, const float* scores,
                                                  const float* ml, float* ds_out, float* dqt_out, void* ws, int64_t ws_bytes) {
    return ragged_global_bwd(a, x, dctx, delta, scores, ml, ds_out, dqt_out, ws, ws_bytes);
}

extern "C" int64_t hicom_compressor_ragged_workspace_bytes(const hicom_compressor_ragged_args* a) { return ragged_workspace_bytes(a, nullptr); }

extern "C" int hicom_compressor_ragged_prepare(const hicom_compressor_ragged_args* a) { return ragged_prepare(a, nullptr); }

extern "C" int hicom_compressor_ragged_fwd(const hicom_compressor_ragged_args* a) { return ragged_fwd(a, nullptr); }

// ---- the adaptor recipe: the same step with the k / v adaptors on the local stage; the table region is the plain one ----------------
extern "C" int64_t hicom_compressor_ragged_adapt_workspace_bytes(const hicom_compressor_ragged_adapt_args* a) { return seg_with_adapt(kWho, a, ragged_workspace_bytes); }

extern "C" int hicom_compressor_ragged_adapt_prepare(const hicom_compressor_ragged_adapt_args* a) { return seg_with_adapt(kWho, a, ragged_prepare); }

extern "C" int hicom_compressor_ragged_adapt_fwd(const hicom_compressor_ragged_adapt_args* a) { return seg_with_adapt(kWho, a, ragged_fwd); }
