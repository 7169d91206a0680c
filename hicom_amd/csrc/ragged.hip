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
// Input gradients (stage 3): hicom_compressor_ragged_local_bwd is the window backward over the concatenated window list (window_rows.hpp:
// local_window_bwd, the body of local_attn_bwd_kernel) with dq summed per item in a fixed order, hicom_compressor_ragged_global_dx the global
// stage's d x with an item per workgroup (global_dx.hpp: global_dx_tile, the body of global_dx_kernel).
// The adaptor recipe's training step: hicom_compressor_ragged_local_adapt_bwd (window_rows.hpp: local_window_adapt_bwd, the body of
// local_attn_adapt_bwd_kernel), hicom_compressor_ragged_adapt_dy (adapt_dy_token, the body of adapt_dy_kernel; the token's item by a search
// of the item table), hicom_compressor_ragged_dq_item and hicom_compressor_ragged_adapt_train_state (the y planes out of the workspace).
#include <vector>

#include "global_dx.hpp"
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

// ---- training, input gradients: the window backward over the concatenated window list, one 4-wave workgroup per window (the mapping and
// the body of local_attn_bwd_kernel: window_rows.hpp, local_window_bwd).  The workgroup learns its item from win_item, builds the window
// from the item's own (T, kt), offsets the tokens by tok0 and takes the item's guide row as the query.  dq f32 [sum windows][D]; dkey /
// dvalue bf16 [sum N_i][D] or NULL, plain stores: the windows of an item partition it, every token is written once ----
struct RaggedLocalBwdParams {
    const uint16_t* key;
    const uint16_t* value;
    const uint16_t* guide;  // [B][D]
    const RaggedItem* items;
    const int* win_item;
    hicom_axis ay, ax;
    float scale;
    const float* dctx;      // [sum windows][D]
    float* dq;              // [sum windows][D]
    uint16_t* dkey;
    uint16_t* dvalue;
    int value_is_key;
};

template <int NV>
__global__ __launch_bounds__(256) void ragged_local_attn_bwd_kernel(RaggedLocalBwdParams p) {
    constexpr int D = NV * 384;
    extern __shared__ __attribute__((aligned(16))) float lsm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int win = blockIdx.x;
    const int item = p.win_item[win];
    const RaggedItem it = p.items[item];
    const hicom_axis at{it.T, it.kt, it.T / it.kt, it.T / it.kt};
    const WindowGeom w(at, p.ay, p.ax, win - it.win0);
    const long first = (long)it.tok0 * D;
    float q[NV][6];
    load_row<NV>(p.guide + (long)item * D, lane, q);
    const WindowBwdArgs a{p.key + first, p.value + first, p.scale, 0.f, p.dctx + (long)win * D, p.dq + (long)win * D,
                          p.dkey ? p.dkey + first : nullptr, 0, nullptr, p.dvalue ? p.dvalue + first : nullptr, p.value_is_key, 0};
    local_window_bwd<NV>(a, w, q, lsm, tid);
}

// ... and the local share of d guide: dq_item[i] = sum of the dq rows of item i's windows, in a fixed order and without atomics.
// grid = (E / 64, B), 256 threads = 16 stripes x 16 lanes of 4 channels: stripe s sums windows s, s + 16, ... in order, the sixteen partial
// rows are added pairwise through LDS.
__global__ __launch_bounds__(256) void ragged_dq_item_kernel(const float* dq, const RaggedItem* items, int wps, int E, float* dq_item) {
    __shared__ float4 red[16][16];
    const int item = blockIdx.y, lane = threadIdx.x & 15, stripe = threadIdx.x >> 4;
    const int c = blockIdx.x * 64 + 4 * lane;
    const RaggedItem it = items[item];
    const int nwin = (it.T / it.kt) * wps;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < E)
        for (int w = stripe; w < nwin; w += 16) {
            const float4 v = *reinterpret_cast<const float4*>(dq + (long)(it.win0 + w) * E + c);
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
    red[stripe][lane] = a;
    __syncthreads();
    for (int half = 8; half > 0; half >>= 1) {
        if (stripe < half) {
            const float4 u = red[stripe][lane], v = red[stripe + half][lane];
            red[stripe][lane] = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
        }
        __syncthreads();
    }
    if (stripe == 0 && c < E) *reinterpret_cast<float4*>(dq_item + (long)item * E + c) = red[0][lane];
}

// ---- training, the adaptor recipe: the window backward through the LayerNorm blends over the concatenated window list, one 4-wave
// workgroup per window (the body of local_attn_adapt_bwd_kernel: window_rows.hpp, local_window_adapt_bwd).  Item, window geometry, token
// offset and query as in ragged_local_attn_bwd_kernel; the y rows of an item start at its first token like its x rows.  ds / pw f32
// [sum N_i], the four sums f32 [sum windows][D] or NULL; plain stores ----
struct RaggedLocalAdaptBwdParams {
    const uint16_t* kx; const _Float16* ky; const uint16_t* kgamma; const uint16_t* kbeta; const void* kalpha;
    const uint16_t* vx; const _Float16* vy; const uint16_t* vgamma; const uint16_t* vbeta; const void* valpha;
    int alpha_f32;
    float eps;
    const uint16_t* guide;  // [B][D]
    const RaggedItem* items;
    const int* win_item;
    hicom_axis ay, ax;
    float scale;
    const float* dctx;      // [sum windows][D]
    float* ds;              // [sum N_i]
    float* pw;              // [sum N_i]
    float* sxk; float* syk; float* sxv; float* syv;
};

template <int NV>
__global__ __launch_bounds__(256) void ragged_local_attn_adapt_bwd_kernel(RaggedLocalAdaptBwdParams p) {
    constexpr int D = NV * 384;
    extern __shared__ __attribute__((aligned(16))) float lsm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int win = blockIdx.x;
    const int item = p.win_item[win];
    const RaggedItem it = p.items[item];
    const hicom_axis at{it.T, it.kt, it.T / it.kt, it.T / it.kt};
    const WindowGeom w(at, p.ay, p.ax, win - it.win0);
    const long first = (long)it.tok0 * D, row = (long)win * D;
    const float ak = p.ky ? read_alpha(p.kalpha, p.alpha_f32) : 0.f, av = p.vy ? read_alpha(p.valpha, p.alpha_f32) : 0.f;
    float q[NV][6];
    load_row<NV>(p.guide + (long)item * D, lane, q);
    const WindowAdaptBwdArgs a{p.kx + first, p.ky ? p.ky + first : nullptr, p.kgamma, p.kbeta, ak, p.vx + first, p.vy ? p.vy + first : nullptr,
                               p.vgamma, p.vbeta, av, p.eps, p.scale, 0.f, p.dctx + row, p.ds + it.tok0, p.pw + it.tok0,
                               p.sxk ? p.sxk + row : nullptr, p.syk ? p.syk + row : nullptr, p.sxv ? p.sxv + row : nullptr,
                               p.syv ? p.syv + row : nullptr};
    local_window_adapt_bwd<NV>(a, w, q, lsm, tid);
}

// ... and d y of an adaptor stream over the stacked tokens, adapt_dy_kernel with the item looked up (the token's body: window_rows.hpp,
// adapt_dy_token).  One wave per token in flight; the wave finds its item by a binary search of tok0 in the item table (B entries, no table
// of token size), the window from the item's own (T, kt) plus win0.  The rank-1 vector: one row per item (K stream: the guide) or per
// window (V stream: dctx).  col_parts as adapt_dy_kernel: this workgroup's column sums of dy ----
struct RaggedAdaptDyParams {
    const _Float16* y;      // [sum N_i][D]
    const uint16_t* gamma;
    const void* vec;        // f32 | bf16 [B | sum windows][D]
    int vec_f32, vec_per_item;
    const float* coef;      // [sum N_i]
    const void* alpha; int alpha_f32;
    float eps;
    const RaggedItem* items;
    int B;
    hicom_axis ay, ax;
    uint16_t* dy;           // bf16 [sum N_i][D]
    uint16_t* r1;           // bf16 [sum N_i][D] or NULL
    long N;                 // sum N_i
    float* col_parts;       // f32 [gridDim.x][D] or NULL
};

template <int NV>
__global__ __launch_bounds__(256) void ragged_adapt_dy_kernel(RaggedAdaptDyParams p) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float csum[NV][6];
    row_zero<NV>(csum);
    for (long tok = (long)blockIdx.x * 4 + wave; tok < p.N; tok += (long)gridDim.x * 4) {
        int lo = 0, hi = p.B;                      // the last item whose first token is <= tok (tok0 rises strictly, items[0].tok0 == 0)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (p.items[mid].tok0 <= tok) lo = mid;
            else hi = mid;
        }
        const RaggedItem it = p.items[lo];
        const hicom_axis at{it.T, it.kt, it.T / it.kt, it.T / it.kt};
        const long win = it.win0 + WindowGeom::window_of(at, p.ay, p.ax, tok - it.tok0);
        const long vrow = (p.vec_per_item ? (long)lo : win) * D;
        const void* vec = p.vec_f32 ? (const void*)(reinterpret_cast<const float*>(p.vec) + vrow)
                                    : (const void*)(reinterpret_cast<const uint16_t*>(p.vec) + vrow);
        adapt_dy_token<NV>(p.y + tok * D, p.gamma, vec, p.vec_f32, p.coef[tok], read_alpha(p.alpha, p.alpha_f32), p.eps, p.dy + tok * D,
                           p.r1 ? p.r1 + tok * D : nullptr, lane, csum);
    }
    if (p.col_parts) {
        __shared__ float red[4 * D];
        store_partial_row<NV>(red, wave, lane, csum);
        __syncthreads();
        sum_partial_rows<NV>(red, threadIdx.x, p.col_parts + (long)blockIdx.x * D);
    }
}

// ---- training, input gradients: d x of the global stage, global_dx_kernel<9> with an item per workgroup (global_dx.hpp: the one body).
// A workgroup takes 64 tokens of ONE item: tiles are counted from the item's first token (item offsets are 36, 144, 180 ... tokens), the
// last tile of an item is masked at the item's end.  tiles: {item, first token of the tile inside the item} per workgroup, derived on the
// host once per plan (hicom_amd/ragged.py: dx_tile_table) ----
struct RaggedGlobalDxParams {
    const float* S;         // the forward's scores region
    const float* dS;        // laid out as S
    const float* ml;        // [B * rows][2]
    const float* qt;        // [B * rows][E]
    const float* dctx;      // [B * rows][E]
    const int2* tiles;
    const RaggedItem* items;
    int B, rows, E;
    uint16_t* dx;           // [sum N_i][E]
    int accumulate;
};

template <int RMAX>
__global__ __launch_bounds__(320) void ragged_global_dx_kernel(RaggedGlobalDxParams p) {
    __shared__ float coef[64][2 * RMAX];
    const int2 tile = p.tiles[blockIdx.x];
    if (tile.x < 0 || tile.x >= p.B) return;            // (a table that is not this plan's: nothing is indexed through it)
    const RaggedItem it = p.items[tile.x];
    if (tile.y < 0 || tile.y >= it.N) return;
    const long row0 = (long)tile.x * p.rows, stride = (it.N + 15) / 16 * 16;
    global_dx_tile<RMAX>(p.S + (long)it.score_off * 16, p.dS + (long)it.score_off * 16, stride, p.ml + 2 * row0, p.qt + row0 * p.E, p.dctx + row0 * p.E,
                      p.rows, (long)tile.y, (long)it.N, p.E, p.dx + (long)it.tok0 * p.E, p.accumulate, coef);
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

// ---- training, input gradients (stage 3): the window backward over all items, and d x of the global stage -----------------------------------
// Both read the table region at the head of args->ws; the pointers and the per-item partition are checked in front of everything that
// needs a device (the layout asks for the CU count when chunks == 0).
int ragged_local_bwd(const hicom_compressor_ragged_args* a, const void* key, const void* value, const void* guide, const float* dctx, float* dq,
                     float* dq_item, void* dkey, void* dvalue, int value_is_key) {
    constexpr const char* who = "compressor_ragged_local_bwd";
    int st = ragged_check(a, nullptr);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(key && value && guide && dctx && dq, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE(!(value_is_key && dkey), HICOM_EINVAL, "%s: value_is_key writes the summed gradient to dvalue (dkey must be NULL)", who);
    HICOM_REQUIRE(!value_is_key || key == value, HICOM_EINVAL, "%s: value_is_key: the keys are the value rows", who);
    HICOM_REQUIRE((uintptr_t)key % 4 == 0 && (uintptr_t)value % 4 == 0 && (uintptr_t)guide % 4 == 0 && (uintptr_t)dctx % 16 == 0 && (uintptr_t)dq % 16 == 0 &&
                      (uintptr_t)dq_item % 16 == 0 && (uintptr_t)dkey % 4 == 0 && (uintptr_t)dvalue % 4 == 0, HICOM_EINVAL, "%s: aligned pointers", who);
    const RaggedLayout l = ragged_layout(a, nullptr);
    st = seg_check_ws(who, a, l.s.total);                     // (the table region at its head is what is read)
    if (st != HICOM_OK) return st;
    int max_kt = 1;
    for (int i = 0; i < a->B; ++i) max_kt = a->items[i].kt > max_kt ? a->items[i].kt : max_kt;
    const long WIN = (long)max_kt * a->ks * a->ks;             // (<= 64: seg_check_ragged_items)
    const size_t smem = 5 * (((size_t)WIN + 3) & ~(size_t)3) * 4 + 4 * (size_t)a->E * 4;
    const char* tab = (const char*)a->ws;
    hipStream_t s = (hipStream_t)a->stream;
    RaggedLocalBwdParams p;
    p.key = (const uint16_t*)key; p.value = (const uint16_t*)value; p.guide = (const uint16_t*)guide;
    p.items = (const RaggedItem*)(tab + l.items); p.win_item = (const int*)(tab + l.win_item);
    p.ay = hicom_axis{a->H, a->ks, a->H / a->ks, a->H / a->ks}; p.ax = hicom_axis{a->W, a->ks, a->W / a->ks, a->W / a->ks};
    p.scale = a->l_scale; p.dctx = dctx; p.dq = dq; p.dkey = (uint16_t*)dkey; p.dvalue = (uint16_t*)dvalue; p.value_is_key = value_is_key ? 1 : 0;
    HICOM_LAUNCH(ragged_local_attn_bwd_kernel<3>, dim3((unsigned)l.s.n.windows), dim3(256), smem, s, p);      // (E == 1152: ragged_check)
    st = seg_check_launch(who, "window backward");
    if (st != HICOM_OK || !dq_item) return st;
    HICOM_LAUNCH(ragged_dq_item_kernel, dim3((unsigned)((a->E + 63) / 64), (unsigned)a->B), dim3(256), 0, s, (const float*)dq, p.items, l.wps, a->E, dq_item);
    return seg_check_launch(who, "dq per item");
}

int ragged_global_dx(const hicom_compressor_ragged_args* a, const float* scores, const float* ds, const float* ml, const float* qt, const float* dctx,
                     const int32_t* tiles, int ntiles, void* dx, int accumulate) {
    constexpr const char* who = "compressor_ragged_global_dx";
    int st = ragged_check(a, nullptr);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(scores && ds && ml && qt && dctx && tiles && dx, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE((uintptr_t)dx % 8 == 0 && (uintptr_t)qt % 16 == 0 && (uintptr_t)dctx % 16 == 0 && (uintptr_t)tiles % 8 == 0, HICOM_EINVAL, "%s: aligned pointers", who);
    HICOM_REQUIRE(a->nh > 0 && a->nh <= 16 && a->E % 4 == 0 && a->E <= 1280, HICOM_EUNSUP, "%s: nh=%d (<= 16), E=%d (<= 1280, %% 4)", who, a->nh, a->E);
    long want = 0;
    for (int i = 0; i < a->B; ++i) want += ((long)a->items[i].T * a->H * a->W + 63) / 64;
    HICOM_REQUIRE(ntiles == want, HICOM_EINVAL, "%s: %d tiles, the items have %ld tiles of 64 tokens", who, ntiles, want);
    const RaggedLayout l = ragged_layout(a, nullptr);
    st = seg_check_ws(who, a, l.s.total);                     // (the table region at its head is what is read)
    if (st != HICOM_OK) return st;
    RaggedGlobalDxParams p;
    p.S = scores; p.dS = ds; p.ml = ml; p.qt = qt; p.dctx = dctx; p.tiles = (const int2*)tiles;
    p.items = (const RaggedItem*)((const char*)a->ws + l.items);
    p.B = a->B; p.rows = a->nh; p.E = a->E; p.dx = (uint16_t*)dx; p.accumulate = accumulate ? 1 : 0;
    hipStream_t s = (hipStream_t)a->stream;
    if (a->nh <= 9) HICOM_LAUNCH(ragged_global_dx_kernel<9>, dim3((unsigned)ntiles), dim3(320), 0, s, p);
    else HICOM_LAUNCH(ragged_global_dx_kernel<16>, dim3((unsigned)ntiles), dim3(320), 0, s, p);
    return seg_check_launch(who, "global dx");
}

// ---- training, the adaptor recipe (hicom_amd/ragged_train.py, adaptors=True) ------------------------------------------------------------------
// What the three calls check alike behind their own pointer checks, in front of everything that needs a device: the per-item partition
// (ragged_check) and tokens * E < 2^32 (the operands of the adaptor GEMMs that take these matrices).  Leaves the token total.
int ragged_adapt_bwd_check(const char* who, const hicom_compressor_ragged_args* a, long& tokens) {
    tokens = 0;
    for (int i = 0; i < a->B; ++i) tokens += (long)a->items[i].T * a->H * a->W;
    HICOM_REQUIRE(tokens * a->E < (1L << 32), HICOM_EUNSUP, "%s: %ld tokens: the adaptor GEMMs take operands below 2^32 elements", who, tokens);
    return HICOM_OK;
}

int ragged_local_adapt_bwd(const hicom_compressor_ragged_args* a, const void* key_x, const void* key_y, const void* k_gamma, const void* k_beta,
                           const void* k_alpha, const void* value_x, const void* value_y, const void* v_gamma, const void* v_beta, const void* v_alpha,
                           int alpha_dt, float eps, const void* guide, const float* dctx, float* ds, float* pw, float* sxk, float* syk, float* sxv,
                           float* syv) {
    constexpr const char* who = "compressor_ragged_local_adapt_bwd";
    int st = ragged_check(a, nullptr);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(key_x && value_x && guide && dctx && ds && pw && (key_y || value_y), HICOM_EINVAL, "%s: NULL pointer / no adapted stream", who);
    HICOM_REQUIRE((!key_y || (k_gamma && k_beta && k_alpha)) && (!value_y || (v_gamma && v_beta && v_alpha)), HICOM_EINVAL, "%s: adaptor parameters", who);
    HICOM_REQUIRE((key_y || !syk) && (value_y || !syv), HICOM_EINVAL, "%s: syk / syv are the sums of an ADAPTED stream (NULL without its y)", who);
    HICOM_REQUIRE(alpha_dt == HICOM_DT_BF16 || alpha_dt == HICOM_DT_F32, HICOM_EINVAL, "%s: alpha dtype %d (bf16 | f32)", who, alpha_dt);
    for (const void* q : {key_x, key_y, k_gamma, k_beta, value_x, value_y, v_gamma, v_beta, guide, (const void*)ds, (const void*)pw})
        HICOM_REQUIRE((uintptr_t)q % 4 == 0, HICOM_EINVAL, "%s: 4-byte aligned rows", who);
    for (const void* q : {(const void*)dctx, (const void*)sxk, (const void*)syk, (const void*)sxv, (const void*)syv})
        HICOM_REQUIRE((uintptr_t)q % 16 == 0, HICOM_EINVAL, "%s: 16-byte aligned f32 matrices", who);
    long tokens;
    st = ragged_adapt_bwd_check(who, a, tokens);
    if (st != HICOM_OK) return st;
    const RaggedLayout l = ragged_layout(a, nullptr);
    st = seg_check_ws(who, a, l.s.total);                     // (the table region at its head is what is read)
    if (st != HICOM_OK) return st;
    int max_kt = 1;
    for (int i = 0; i < a->B; ++i) max_kt = a->items[i].kt > max_kt ? a->items[i].kt : max_kt;
    const long WIN = (long)max_kt * a->ks * a->ks;             // (<= 64: seg_check_ragged_items)
    const size_t smem = 6 * (((size_t)WIN + 3) & ~(size_t)3) * 4 + 4 * (size_t)a->E * 4;
    const char* tab = (const char*)a->ws;
    RaggedLocalAdaptBwdParams p;
    p.kx = (const uint16_t*)key_x; p.ky = (const _Float16*)key_y; p.kgamma = (const uint16_t*)k_gamma; p.kbeta = (const uint16_t*)k_beta; p.kalpha = k_alpha;
    p.vx = (const uint16_t*)value_x; p.vy = (const _Float16*)value_y; p.vgamma = (const uint16_t*)v_gamma; p.vbeta = (const uint16_t*)v_beta; p.valpha = v_alpha;
    p.alpha_f32 = alpha_dt == HICOM_DT_F32; p.eps = eps; p.guide = (const uint16_t*)guide;
    p.items = (const RaggedItem*)(tab + l.items); p.win_item = (const int*)(tab + l.win_item);
    p.ay = hicom_axis{a->H, a->ks, a->H / a->ks, a->H / a->ks}; p.ax = hicom_axis{a->W, a->ks, a->W / a->ks, a->W / a->ks};
    p.scale = a->l_scale; p.dctx = dctx; p.ds = ds; p.pw = pw; p.sxk = sxk; p.syk = syk; p.sxv = sxv; p.syv = syv;
    HICOM_LAUNCH(ragged_local_attn_adapt_bwd_kernel<3>, dim3((unsigned)l.s.n.windows), dim3(256), smem, (hipStream_t)a->stream, p);      // (E == 1152: ragged_check)
    return seg_check_launch(who, "window backward");
}

int ragged_adapt_dy(const hicom_compressor_ragged_args* a, const void* y, const void* gamma, const void* vec, int vec_dt, int vec_per_item, const float* coef,
                    const void* alpha, int alpha_dt, float eps, void* dy, void* r1, float* col_parts, int nparts) {
    constexpr const char* who = "compressor_ragged_adapt_dy";
    int st = ragged_check(a, nullptr);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(y && gamma && vec && coef && alpha && dy && (!col_parts || nparts > 0), HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE((vec_dt == HICOM_DT_BF16 || vec_dt == HICOM_DT_F32) && (alpha_dt == HICOM_DT_BF16 || alpha_dt == HICOM_DT_F32), HICOM_EINVAL, "%s: dtypes", who);
    HICOM_REQUIRE((uintptr_t)y % 4 == 0 && (uintptr_t)gamma % 4 == 0 && (uintptr_t)vec % 4 == 0 && (uintptr_t)coef % 4 == 0 && (uintptr_t)dy % 4 == 0 &&
                      (uintptr_t)r1 % 4 == 0 && (uintptr_t)col_parts % 4 == 0, HICOM_EINVAL, "%s: 4-byte aligned rows", who);
    long tokens;
    st = ragged_adapt_bwd_check(who, a, tokens);
    if (st != HICOM_OK) return st;
    const RaggedLayout l = ragged_layout(a, nullptr);
    st = seg_check_ws(who, a, l.s.total);                     // (the table region at its head is what is read)
    if (st != HICOM_OK) return st;
    RaggedAdaptDyParams p;
    p.y = (const _Float16*)y; p.gamma = (const uint16_t*)gamma; p.vec = vec; p.vec_f32 = vec_dt == HICOM_DT_F32; p.vec_per_item = vec_per_item ? 1 : 0;
    p.coef = coef; p.alpha = alpha; p.alpha_f32 = alpha_dt == HICOM_DT_F32; p.eps = eps;
    p.items = (const RaggedItem*)((const char*)a->ws + l.items); p.B = a->B;
    p.ay = hicom_axis{a->H, a->ks, a->H / a->ks, a->H / a->ks}; p.ax = hicom_axis{a->W, a->ks, a->W / a->ks, a->W / a->ks};
    p.dy = (uint16_t*)dy; p.r1 = (uint16_t*)r1; p.N = tokens; p.col_parts = col_parts;
    // with column partials: `nparts` workgroups walk the tokens (each leaves one partial row); without: one token per wave
    const unsigned grid = col_parts ? (unsigned)nparts : (unsigned)((tokens + 3) / 4);
    HICOM_LAUNCH(ragged_adapt_dy_kernel<3>, dim3(grid), dim3(256), 0, (hipStream_t)a->stream, p);      // (E == 1152: ragged_check)
    return seg_check_launch(who, "adapt dy");
}

int ragged_dq_item(const hicom_compressor_ragged_args* a, const float* dq, float* dq_item) {
    constexpr const char* who = "compressor_ragged_dq_item";
    int st = ragged_check(a, nullptr);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(dq && dq_item, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE((uintptr_t)dq % 16 == 0 && (uintptr_t)dq_item % 16 == 0, HICOM_EINVAL, "%s: 16-byte aligned pointers", who);
    long tokens;
    st = ragged_adapt_bwd_check(who, a, tokens);
    if (st != HICOM_OK) return st;
    const RaggedLayout l = ragged_layout(a, nullptr);
    st = seg_check_ws(who, a, l.s.total);                     // (the table region at its head is what is read)
    if (st != HICOM_OK) return st;
    HICOM_LAUNCH(ragged_dq_item_kernel, dim3((unsigned)((a->E + 63) / 64), (unsigned)a->B), dim3(256), 0, (hipStream_t)a->stream, dq,
                 (const RaggedItem*)((const char*)a->ws + l.items), l.wps, a->E, dq_item);
    return seg_check_launch(who, "dq per item");
}

// the y planes of the adapted streams out of the adaptor regions of the workspace (hicom_compressor_ragged_adapt_fwd left them there)
int ragged_adapt_train_state(const hicom_compressor_ragged_args* a, const SegAdapt* ad, void* ky_out, void* vy_out) {
    constexpr const char* who = "compressor_ragged_adapt_train_state";
    int st = ragged_check(a, ad);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(ky_out || vy_out, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE((!ky_out || ad->k()) && (!vy_out || ad->v()), HICOM_EINVAL, "%s: a y plane of a stream without adaptor", who);
    const RaggedLayout l = ragged_layout(a, ad);
    st = seg_check_ws(who, a, l.s.total);
    if (st != HICOM_OK) return st;
    const char* ws = (const char*)a->ws;
    hipStream_t s = (hipStream_t)a->stream;
    const size_t bytes = (size_t)(l.s.n.tokens * a->E * 2);
    if ((ky_out && hipMemcpyAsync(ky_out, ws + l.s.ad.ky, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) ||
        (vy_out && hipMemcpyAsync(vy_out, ws + l.s.ad.vy, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess)) {
        set_error("%s: copying the state: %s", who, hipGetErrorString(hipGetLastError()));
        return HICOM_ELAUNCH;
    }
    return HICOM_OK;
}

}  // namespace

extern "C" int hicom_compressor_ragged_local_adapt_bwd(const hicom_compressor_ragged_args* a, const void* key_x, const void* key_y, const void* k_gamma,
                                                       const void* k_beta, const void* k_alpha, const void* value_x, const void* value_y, const void* v_gamma,
                                                       const void* v_beta, const void* v_alpha, int32_t alpha_dt, float eps, const void* guide, const float* dctx,
                                                       float* ds, float* pw, float* sxk, float* syk, float* sxv, float* syv) {
    return ragged_local_adapt_bwd(a, key_x, key_y, k_gamma, k_beta, k_alpha, value_x, value_y, v_gamma, v_beta, v_alpha, alpha_dt, eps, guide, dctx, ds, pw, sxk,
                                  syk, sxv, syv);
}

extern "C" int hicom_compressor_ragged_adapt_dy(const hicom_compressor_ragged_args* a, const void* y, const void* gamma, const void* vec, int32_t vec_dt,
                                                int32_t vec_per_item, const float* coef, const void* alpha, int32_t alpha_dt, float eps, void* dy, void* r1,
                                                float* col_parts, int32_t nparts) {
    return ragged_adapt_dy(a, y, gamma, vec, vec_dt, vec_per_item, coef, alpha, alpha_dt, eps, dy, r1, col_parts, nparts);
}

extern "C" int hicom_compressor_ragged_dq_item(const hicom_compressor_ragged_args* a, const float* dq, float* dq_item) { return ragged_dq_item(a, dq, dq_item); }

extern "C" int hicom_compressor_ragged_adapt_train_state(const hicom_compressor_ragged_adapt_args* a, void* ky_out, void* vy_out) {
    return seg_with_adapt("compressor_ragged_adapt_train_state", a,
                          [&](const hicom_compressor_ragged_args* b, const SegAdapt* ad) { return ragged_adapt_train_state(b, ad, ky_out, vy_out); });
}

extern "C" int hicom_compressor_ragged_local_bwd(const hicom_compressor_ragged_args* a, const void* key, const void* value, const void* guide, const float* dctx,
                                                 float* dq, float* dq_item, void* dkey, void* dvalue, int32_t value_is_key) {
    return ragged_local_bwd(a, key, value, guide, dctx, dq, dq_item, dkey, dvalue, value_is_key);
}

extern "C" int hicom_compressor_ragged_global_dx(const hicom_compressor_ragged_args* a, const float* scores, const float* ds, const float* ml, const float* qt,
                                                 const float* dctx, const int32_t* tiles, int32_t ntiles, void* dx, int32_t accumulate) {
    return ragged_global_dx(a, scores, ds, ml, qt, dctx, tiles, ntiles, dx, accumulate);
}

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
