// Training surface of the ragged compressor step (hicom_amd/ragged_train.py): what a backward over all items of a mixed batch launches.
// The forward is ragged.hip's; every call here reads the table region hicom_compressor_ragged_prepare left at the head of the workspace
// (item table, work units, window -> item: ragged_host.hpp) and finds its item the way the forward does.
// Plain recipe: hicom_compressor_ragged_train_state hands the forward's state out of the workspace, hicom_compressor_ragged_global_bwd runs
// the global stage's attention backward over all items on the forward's unit table -- the same stream_segment in StreamMode::Bwd, then
// dq_merge_segments per (item, head).
// Input gradients (stage 3): hicom_compressor_ragged_local_bwd is the window backward over the concatenated window list (window_rows.hpp:
// local_window_bwd, the body of local_attn_bwd_kernel) with dq summed per item in a fixed order, hicom_compressor_ragged_global_dx the global
// stage's d x with an item per workgroup (global_dx.hpp: global_dx_tile, the body of global_dx_kernel).
// The logits form (the forward took the local scores precomputed: ragged.hip, hicom_compressor_ragged_logits_fwd):
// hicom_compressor_ragged_local_logits_bwd, one wave per window on the row helpers of window_rows.hpp: d local_logits and the value-side
// share of d frames_feature, no dq.
// The adaptor recipe's training step: hicom_compressor_ragged_local_adapt_bwd (window_rows.hpp: local_window_adapt_bwd, the body of
// local_attn_adapt_bwd_kernel), hicom_compressor_ragged_adapt_dy (adapt_dy_token, the body of adapt_dy_kernel; the token's item by a search
// of the item table), hicom_compressor_ragged_dq_item and hicom_compressor_ragged_adapt_train_state (the y planes out of the workspace).
// Every entry point opens alike: ragged_check (no device), the call's own checks, then ragged_tables (layout, workspace check, typed
// pointers into the table region).
#include "global_dx.hpp"
#include "ragged_host.hpp"

namespace hicom {

// ---- (M, L) per (item, head) from the partial states, merge_segments' own order.  grid = B, 64 threads ----
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

// ---- the segmented backward of the global stream, the forward's unit table and slots (stream_body.hpp: StreamMode::Bwd).
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

// ---- dq merge per (item, head), grid = (rows, B), the forward merge's LDS ----
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

// ---- input gradients: the window backward over the concatenated window list, one 4-wave workgroup per window (the mapping and the body
// of local_attn_bwd_kernel: window_rows.hpp, local_window_bwd).  The workgroup learns its item from win_item, builds the window from the
// item's own (T, kt), offsets the tokens by tok0 and takes the item's guide row as the query (ragged_host.hpp: RaggedWindow).  dq f32
// [sum windows][D]; dkey / dvalue bf16 [sum N_i][D] or NULL, plain stores: the windows of an item partition it, every token is written once ----
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
    const RaggedWindow w(p.items, p.win_item, p.ay, p.ax, win, D);
    const long first = w.first;
    float q[NV][6];
    load_row<NV>(p.guide + (long)w.item * D, lane, q);
    const WindowBwdArgs a{p.key + first, p.value + first, p.scale, 0.f, p.dctx + (long)win * D, p.dq + (long)win * D,
                          p.dkey ? p.dkey + first : nullptr, 0, nullptr, p.dvalue ? p.dvalue + first : nullptr, p.value_is_key, 0};
    local_window_bwd<NV>(a, w.geom, q, lsm, tid);
}

// ... and the local share of d guide: dq_item[i] = sum of the dq rows of item i's windows, in a fixed order and without atomics
// (window_rows.hpp: sum_rows_striped has the order).  grid = (E / 64, B), 256 threads.
__global__ __launch_bounds__(256) void ragged_dq_item_kernel(const float* dq, const RaggedItem* items, int wps, int E, float* dq_item) {
    __shared__ float4 red[16][16];
    const RaggedItem it = items[blockIdx.y];
    sum_rows_striped(dq, (long)it.win0, (it.T / it.kt) * wps, E, dq_item + (long)blockIdx.y * E, red);
}

// ---- the logits form: the window backward where the forward took its scores precomputed, l_n = key_n . guide_item as f32
// [sum N_i].  One wave per window, four windows per workgroup -- the forward's wave -> window -> item map (ragged_local_logits_kernel).
// Lane i holds token i of the window: p = softmax(scale l) as the forward forms it, then ONE walk over the window's value rows:
//     dp_i = dctx . v_i (a wave sum, kept by lane i),   dvalue_i = p_i dctx (bf16 row, or not written with dvalue NULL)
// and behind it  dl_i = scale p_i (dp_i - sum_j p_j dp_j).  No key row, no guide row, no dq: the guide does not enter the local stage.
// Every sum is a fixed-order wave reduction or one lane's chain; every token lies in one window, so dl and dvalue are plain stores ----
struct RaggedLocalLogitsBwdParams {
    const uint16_t* value;  // [sum N_i][D]
    const float* logits;    // [sum N_i]
    const RaggedItem* items;
    const int* win_item;
    hicom_axis ay, ax;
    int nwin;
    float scale;
    const float* dctx;      // [sum windows][D]
    float* dlogits;         // [sum N_i]
    uint16_t* dvalue;       // bf16 [sum N_i][D] or NULL
};

template <int NV>
__global__ __launch_bounds__(256) void ragged_local_logits_bwd_kernel(RaggedLocalLogitsBwdParams p) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= p.nwin) return;
    const RaggedWindow w(p.items, p.win_item, p.ay, p.ax, win, D);
    const WindowGeom& g = w.geom;
    const bool live = lane < g.WIN;
    const long mine = w.it.tok0 + g.token_of(live ? lane : 0);
    const float sc = live ? p.logits[mine] * p.scale : -3.0e38f;
    const float mx = wave_max_fast(sc);
    const float e = live ? expf(sc - mx) : 0.f;
    const float pw = e / wave_sum_fast(e);
    float dc[NV][6];
    load_row_f32<NV>(p.dctx + (long)win * D, lane, dc);
    const uint16_t* value = p.value + w.first;
    uint16_t* dvalue = p.dvalue ? p.dvalue + w.first : nullptr;
    float dp = 0.f;
    for (int i0 = 0; i0 < g.WIN; i0 += 2) {          // two value rows in flight
        float v[2][NV][6];
#pragma unroll
        for (int u = 0; u < 2; ++u)
            if (i0 + u < g.WIN) load_row<NV>(value + g.token_of(i0 + u) * D, lane, v[u]);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = i0 + u;
            if (i < g.WIN) {
                const float d = wave_sum_fast(row_dot<NV>(dc, v[u]));
                if (lane == i) dp = d;
                if (dvalue) {
                    const float pi_ = __shfl(pw, i, 64);
                    store_row_bf16<NV>(dvalue + g.token_of(i) * D, lane, false, [&](int s, int j) { return pi_ * dc[s][j]; });
                }
            }
        }
    }
    const float delta = wave_sum_fast(pw * dp);      // (lanes >= WIN: pw = 0, dp = 0)
    if (live) p.dlogits[mine] = p.scale * pw * (dp - delta);
}

// ---- the adaptor recipe: the window backward through the LayerNorm blends over the concatenated window list, one 4-wave workgroup per
// window (the body of local_attn_adapt_bwd_kernel: window_rows.hpp, local_window_adapt_bwd).  Item, window geometry, token offset and query
// as in ragged_local_attn_bwd_kernel; the y rows of an item start at its first token like its x rows.  ds / pw f32 [sum N_i], the four
// sums f32 [sum windows][D] or NULL; plain stores ----
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
    const RaggedWindow w(p.items, p.win_item, p.ay, p.ax, win, D);
    const long first = w.first, row = (long)win * D;
    const float ak = p.ky ? read_alpha(p.kalpha, p.alpha_f32) : 0.f, av = p.vy ? read_alpha(p.valpha, p.alpha_f32) : 0.f;
    float q[NV][6];
    load_row<NV>(p.guide + (long)w.item * D, lane, q);
    const WindowAdaptBwdArgs a{p.kx + first, p.ky ? p.ky + first : nullptr, p.kgamma, p.kbeta, ak, p.vx + first, p.vy ? p.vy + first : nullptr,
                               p.vgamma, p.vbeta, av, p.eps, p.scale, 0.f, p.dctx + row, p.ds + w.it.tok0, p.pw + w.it.tok0,
                               p.sxk ? p.sxk + row : nullptr, p.syk ? p.syk + row : nullptr, p.sxv ? p.sxv + row : nullptr,
                               p.syv ? p.syv + row : nullptr};
    local_window_adapt_bwd<NV>(a, w.geom, q, lsm, tid);
}

// ... and d y of an adaptor stream over the stacked tokens, adapt_dy_kernel with the item looked up (the token's body: window_rows.hpp,
// adapt_dy_token).  One wave per token in flight; the wave finds its item and window through the item table (ragged_host.hpp: RaggedToken;
// no table of token size).  The rank-1 vector: one row per item (K stream: the guide) or per window (V stream: dctx).  col_parts as
// adapt_dy_kernel: this workgroup's column sums of dy ----
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
        const RaggedToken t(p.items, p.B, p.ay, p.ax, tok);
        const long vrow = (p.vec_per_item ? (long)t.item : t.win) * D;
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

// ---- input gradients: d x of the global stage, global_dx_kernel<9> with an item per workgroup (global_dx.hpp: the one body).
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

}  // namespace hicom

using namespace hicom;
using namespace hicom_host;

namespace {

// ---- the one call prologue, in two halves around the call's own checks.  ragged_check (NULL block, shape, per-item partition) asks for no
// device; ragged_tables does: the layout wants the CU count when chunks == 0, so the pointer checks of a call stay in front of it ----
struct RaggedTables {
    RaggedLayout l;
    const char* ws;
    const RaggedItem* items;
    const int4* units;
    const int* win_item;
};

int ragged_tables(const char* who, const hicom_compressor_ragged_args* a, const SegAdapt* ad, RaggedTables& t) {
    t.l = ragged_layout(a, ad);
    HICOM_TRY(seg_check_ws(who, a, t.l.s.total));             // (the table region at its head is what the training calls read)
    t.ws = (const char*)a->ws;
    t.items = (const RaggedItem*)(t.ws + t.l.items);
    t.units = (const int4*)(t.ws + t.l.units);
    t.win_item = (const int*)(t.ws + t.l.win_item);
    return HICOM_OK;
}

// ... with, in front of it, what the three calls of the adaptor recipe check alike behind their own pointer checks: tokens * E < 2^32 (the
// operands of the adaptor GEMMs that take these matrices).  The token total is t.l.s.n.tokens.
int ragged_adapt_tables(const char* who, const hicom_compressor_ragged_args* a, RaggedTables& t) {
    long tokens = 0;
    for (int i = 0; i < a->B; ++i) tokens += (long)a->items[i].T * a->H * a->W;
    HICOM_REQUIRE(tokens * a->E < (1L << 32), HICOM_EUNSUP, "%s: %ld tokens: the adaptor GEMMs take operands below 2^32 elements", who, tokens);
    return ragged_tables(who, a, nullptr, t);
}

// LDS of a window backward: `per_token` floats for every token of the call's largest window (rounded up to 4) and four rows of E floats
size_t ragged_window_bwd_smem(const hicom_compressor_ragged_args* a, int per_token) {
    int max_kt = 1;
    for (int i = 0; i < a->B; ++i) max_kt = a->items[i].kt > max_kt ? a->items[i].kt : max_kt;
    const long WIN = (long)max_kt * a->ks * a->ks;             // (<= 64: seg_check_ragged_items)
    return per_token * (((size_t)WIN + 3) & ~(size_t)3) * 4 + 4 * (size_t)a->E * 4;
}

int ragged_launch_dq_item(const char* who, const hicom_compressor_ragged_args* a, const RaggedTables& t, const float* dq, float* dq_item) {
    HICOM_LAUNCH(ragged_dq_item_kernel, dim3((unsigned)((a->E + 63) / 64), (unsigned)a->B), dim3(256), 0, (hipStream_t)a->stream, dq, t.items, t.l.wps, a->E,
                 dq_item);
    return seg_check_launch(who, "dq per item");
}

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

}  // namespace

// ---- plain recipe: the state a backward reads, and the global stage's attention backward -------------------------------------------------
extern "C" int hicom_compressor_ragged_train_state(const hicom_compressor_ragged_args* a, void* ctx16_out, float* scores_out, float* ml_out, float* ctxg_out) {
    constexpr const char* who = "compressor_ragged_train_state";
    HICOM_TRY(ragged_check(a, nullptr));
    RaggedTables t;
    HICOM_TRY(ragged_tables(who, a, nullptr, t));
    HICOM_REQUIRE(ctx16_out && scores_out && ml_out && ctxg_out, HICOM_EINVAL, "%s: NULL pointer", who);
    const SegLayout& l = t.l.s;
    hipStream_t s = (hipStream_t)a->stream;
    const long E = a->E;
    if (hipMemcpyAsync(ctx16_out, t.ws + l.ctx16, (size_t)(l.n.windows * E * 2), hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(scores_out, t.ws + l.scores, (size_t)(l.n.score_floats * 4), hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(ctxg_out, t.ws + l.ctxg, (size_t)(l.n.rows * E * 4), hipMemcpyDeviceToDevice, s) != hipSuccess) {
        set_error("%s: copying the state: %s", who, hipGetErrorString(hipGetLastError()));
        return HICOM_ELAUNCH;
    }
    HICOM_LAUNCH(ragged_state_ml_kernel, dim3((unsigned)a->B), dim3(64), 0, s, (const float*)(t.ws + l.part_m), (const float*)(t.ws + l.part_l), t.items, a->nh,
                 ml_out);
    return seg_check_launch(who, "softmax state");
}

extern "C" int64_t hicom_compressor_ragged_global_bwd_workspace_bytes(const hicom_compressor_ragged_args* a) {
    HICOM_TRY(ragged_check(a, nullptr));
    return ragged_bwd_layout(a, ragged_layout(a, nullptr)).total;
}

extern "C" int hicom_compressor_ragged_global_bwd(const hicom_compressor_ragged_args* a, const void* x, const float* dctx, const float* delta, const float* scores,
                                                  const float* ml, float* ds_out, float* dqt_out, void* bws, int64_t bws_bytes) {
    constexpr const char* who = "compressor_ragged_global_bwd";
    HICOM_TRY(ragged_check(a, nullptr));
    RaggedTables t;
    HICOM_TRY(ragged_tables(who, a, nullptr, t));
    const RaggedBwdLayout b = ragged_bwd_layout(a, t.l);
    HICOM_REQUIRE(x && dctx && delta && scores && ml && ds_out && dqt_out, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE(bws && bws_bytes >= b.total && (uintptr_t)bws % 256 == 0, HICOM_EINVAL, "%s: workspace of %ld bytes, 256-byte aligned", who, b.total);
    HICOM_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)scores % 16 == 0 && (uintptr_t)ds_out % 16 == 0 && (uintptr_t)dctx % 16 == 0, HICOM_EINVAL,
                  "%s: 16-byte aligned inputs", who);
    HICOM_REQUIRE(ds_out != scores, HICOM_EINVAL, "%s: dS cannot overwrite the logits", who);
    char* w = (char*)bws;
    const int R = (int)t.l.s.n.rows, E = a->E;
    hipStream_t s = (hipStream_t)a->stream;

    // 1: dctx -> bf16 hi / lo planes
    HICOM_TRY(hicom_split_bf16_fwd(dctx, R, R, E, w + b.dhi, w + b.dlo, a->stream));
    // 2: the score-side positional table of dP
    float* pos_b = a->pe ? (float*)(w + b.pos_b) : nullptr;
    if (a->pe) HICOM_TRY(hicom_linear_fwd(dctx, HICOM_DT_F32, a->pe, HICOM_DT_F32, nullptr, 0, nullptr, 0, R, a->P, E, 0, 0, HICOM_ACT_NONE, pos_b, a->stream));
    // 3: the segmented backward stream
    {
        RaggedStreamBwdParams p;
        p.c.qhi = (const uint16_t*)(w + b.dhi); p.c.qlo = (const uint16_t*)(w + b.dlo);
        p.c.pos_a = pos_b; p.c.pos_stride = a->P; p.c.rows = a->nh;
        p.c.H = a->H; p.c.W = a->W; p.c.HW = a->H * a->W;
        p.c.t0i = a->t_index0; p.c.y0i = a->y_index0; p.c.x0i = a->x_index0;
        p.c.part_m = nullptr; p.c.part_l = nullptr; p.c.part_acc = (float*)(w + b.part_acc);
        p.x = (const uint16_t*)x; p.s_in = scores; p.ml = ml; p.delta = delta; p.ds = ds_out;
        p.units = t.units; p.items = t.items;
        static bool attr_set = false;
        if (!attr_set) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(ragged_global_stream_bwd_kernel<9>), hipFuncAttributeMaxDynamicSharedMemorySize, seg_stream_smem(1));
            attr_set = true;
        }
        HICOM_LAUNCH(ragged_global_stream_bwd_kernel<9>, dim3((unsigned)t.l.s.n.slots), dim3(256), seg_stream_smem(1), s, p);
        HICOM_TRY(seg_check_launch(who, "backward stream"));
    }
    // 4: dq merge per (item, head)
    RaggedDqMergeParams p;
    p.c.part_acc = (const float*)(w + b.part_acc); p.c.pe = a->pe; p.c.E = E; p.c.H = a->H; p.c.W = a->W;
    p.c.t0i = a->t_index0; p.c.y0i = a->y_index0; p.c.x0i = a->x_index0;
    p.ds = ds_out; p.items = t.items; p.rows = a->nh; p.dqt = dqt_out;
    HICOM_LAUNCH(ragged_dq_merge_kernel, dim3((unsigned)a->nh, (unsigned)a->B), dim3(256), (size_t)seg_merge_smem(t.l.max_T, a->H, a->W), s, p);
    return seg_check_launch(who, "dq merge");
}

// ---- input gradients (stage 3): the window backward over all items, and d x of the global stage ---------------------------------------------
extern "C" int hicom_compressor_ragged_local_bwd(const hicom_compressor_ragged_args* a, const void* key, const void* value, const void* guide, const float* dctx,
                                                 float* dq, float* dq_item, void* dkey, void* dvalue, int32_t value_is_key) {
    constexpr const char* who = "compressor_ragged_local_bwd";
    HICOM_TRY(ragged_check(a, nullptr));
    HICOM_REQUIRE(key && value && guide && dctx && dq, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE(!(value_is_key && dkey), HICOM_EINVAL, "%s: value_is_key writes the summed gradient to dvalue (dkey must be NULL)", who);
    HICOM_REQUIRE(!value_is_key || key == value, HICOM_EINVAL, "%s: value_is_key: the keys are the value rows", who);
    HICOM_REQUIRE((uintptr_t)key % 4 == 0 && (uintptr_t)value % 4 == 0 && (uintptr_t)guide % 4 == 0 && (uintptr_t)dctx % 16 == 0 && (uintptr_t)dq % 16 == 0 &&
                      (uintptr_t)dq_item % 16 == 0 && (uintptr_t)dkey % 4 == 0 && (uintptr_t)dvalue % 4 == 0, HICOM_EINVAL, "%s: aligned pointers", who);
    RaggedTables t;
    HICOM_TRY(ragged_tables(who, a, nullptr, t));
    const RaggedAxes ax = ragged_axes(a);
    RaggedLocalBwdParams p;
    p.key = (const uint16_t*)key; p.value = (const uint16_t*)value; p.guide = (const uint16_t*)guide;
    p.items = t.items; p.win_item = t.win_item; p.ay = ax.ay; p.ax = ax.ax;
    p.scale = a->l_scale; p.dctx = dctx; p.dq = dq; p.dkey = (uint16_t*)dkey; p.dvalue = (uint16_t*)dvalue; p.value_is_key = value_is_key ? 1 : 0;
    HICOM_LAUNCH(ragged_local_attn_bwd_kernel<3>, dim3((unsigned)t.l.s.n.windows), dim3(256), ragged_window_bwd_smem(a, 5), (hipStream_t)a->stream,
                 p);                                           // (E == 1152: ragged_check)
    HICOM_TRY(seg_check_launch(who, "window backward"));
    return dq_item ? ragged_launch_dq_item(who, a, t, dq, dq_item) : HICOM_OK;
}

extern "C" int hicom_compressor_ragged_global_dx(const hicom_compressor_ragged_args* a, const float* scores, const float* ds, const float* ml, const float* qt,
                                                 const float* dctx, const int32_t* tiles, int32_t ntiles, void* dx, int32_t accumulate) {
    constexpr const char* who = "compressor_ragged_global_dx";
    HICOM_TRY(ragged_check(a, nullptr));
    HICOM_REQUIRE(scores && ds && ml && qt && dctx && tiles && dx, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE((uintptr_t)dx % 8 == 0 && (uintptr_t)qt % 16 == 0 && (uintptr_t)dctx % 16 == 0 && (uintptr_t)tiles % 8 == 0, HICOM_EINVAL, "%s: aligned pointers", who);
    HICOM_REQUIRE(a->nh > 0 && a->nh <= 16 && a->E % 4 == 0 && a->E <= 1280, HICOM_EUNSUP, "%s: nh=%d (<= 16), E=%d (<= 1280, %% 4)", who, a->nh, a->E);
    long want = 0;
    for (int i = 0; i < a->B; ++i) want += ((long)a->items[i].T * a->H * a->W + 63) / 64;
    HICOM_REQUIRE(ntiles == want, HICOM_EINVAL, "%s: %d tiles, the items have %ld tiles of 64 tokens", who, ntiles, want);
    RaggedTables t;
    HICOM_TRY(ragged_tables(who, a, nullptr, t));
    RaggedGlobalDxParams p;
    p.S = scores; p.dS = ds; p.ml = ml; p.qt = qt; p.dctx = dctx; p.tiles = (const int2*)tiles;
    p.items = t.items;
    p.B = a->B; p.rows = a->nh; p.E = a->E; p.dx = (uint16_t*)dx; p.accumulate = accumulate ? 1 : 0;
    hipStream_t s = (hipStream_t)a->stream;
    if (a->nh <= 9) HICOM_LAUNCH(ragged_global_dx_kernel<9>, dim3((unsigned)ntiles), dim3(320), 0, s, p);
    else HICOM_LAUNCH(ragged_global_dx_kernel<16>, dim3((unsigned)ntiles), dim3(320), 0, s, p);
    return seg_check_launch(who, "global dx");
}

// ---- the logits form (forward_ragged_train(local_logits=), input_grads=True): d local_logits and the value-side share of d frames_feature ----
extern "C" int hicom_compressor_ragged_local_logits_bwd(const hicom_compressor_ragged_args* a, const void* value, const float* local_logits, const float* dctx,
                                                        float* dlogits, void* dvalue) {
    constexpr const char* who = "compressor_ragged_local_logits_bwd";
    HICOM_TRY(ragged_check(a, nullptr));
    HICOM_REQUIRE(value && local_logits && dctx && dlogits, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE((uintptr_t)value % 4 == 0 && (uintptr_t)local_logits % 4 == 0 && (uintptr_t)dctx % 16 == 0 && (uintptr_t)dlogits % 4 == 0 &&
                      (uintptr_t)dvalue % 4 == 0, HICOM_EINVAL, "%s: aligned pointers", who);
    HICOM_REQUIRE(dlogits != local_logits, HICOM_EINVAL, "%s: d local_logits cannot overwrite the scores", who);
    RaggedTables t;
    HICOM_TRY(ragged_tables(who, a, nullptr, t));
    const RaggedAxes ax = ragged_axes(a);
    const long windows = t.l.s.n.windows;
    RaggedLocalLogitsBwdParams p;
    p.value = (const uint16_t*)value; p.logits = local_logits;
    p.items = t.items; p.win_item = t.win_item; p.ay = ax.ay; p.ax = ax.ax; p.nwin = (int)windows;
    p.scale = a->l_scale; p.dctx = dctx; p.dlogits = dlogits; p.dvalue = (uint16_t*)dvalue;
    HICOM_LAUNCH(ragged_local_logits_bwd_kernel<3>, dim3((unsigned)((windows + 3) / 4)), dim3(256), 0, (hipStream_t)a->stream, p);   // (E == 1152: ragged_check)
    return seg_check_launch(who, "window backward");
}

// ---- the adaptor recipe (hicom_amd/ragged_train.py, adaptors=True) ---------------------------------------------------------------------------
extern "C" int hicom_compressor_ragged_local_adapt_bwd(const hicom_compressor_ragged_args* a, const void* key_x, const void* key_y, const void* k_gamma,
                                                       const void* k_beta, const void* k_alpha, const void* value_x, const void* value_y, const void* v_gamma,
                                                       const void* v_beta, const void* v_alpha, int32_t alpha_dt, float eps, const void* guide, const float* dctx,
                                                       float* ds, float* pw, float* sxk, float* syk, float* sxv, float* syv) {
    constexpr const char* who = "compressor_ragged_local_adapt_bwd";
    HICOM_TRY(ragged_check(a, nullptr));
    HICOM_REQUIRE(key_x && value_x && guide && dctx && ds && pw && (key_y || value_y), HICOM_EINVAL, "%s: NULL pointer / no adapted stream", who);
    HICOM_REQUIRE((!key_y || (k_gamma && k_beta && k_alpha)) && (!value_y || (v_gamma && v_beta && v_alpha)), HICOM_EINVAL, "%s: adaptor parameters", who);
    HICOM_REQUIRE((key_y || !syk) && (value_y || !syv), HICOM_EINVAL, "%s: syk / syv are the sums of an ADAPTED stream (NULL without its y)", who);
    HICOM_REQUIRE(alpha_dt == HICOM_DT_BF16 || alpha_dt == HICOM_DT_F32, HICOM_EINVAL, "%s: alpha dtype %d (bf16 | f32)", who, alpha_dt);
    for (const void* q : {key_x, key_y, k_gamma, k_beta, value_x, value_y, v_gamma, v_beta, guide, (const void*)ds, (const void*)pw})
        HICOM_REQUIRE((uintptr_t)q % 4 == 0, HICOM_EINVAL, "%s: 4-byte aligned rows", who);
    for (const void* q : {(const void*)dctx, (const void*)sxk, (const void*)syk, (const void*)sxv, (const void*)syv})
        HICOM_REQUIRE((uintptr_t)q % 16 == 0, HICOM_EINVAL, "%s: 16-byte aligned f32 matrices", who);
    RaggedTables t;
    HICOM_TRY(ragged_adapt_tables(who, a, t));
    const RaggedAxes ax = ragged_axes(a);
    RaggedLocalAdaptBwdParams p;
    p.kx = (const uint16_t*)key_x; p.ky = (const _Float16*)key_y; p.kgamma = (const uint16_t*)k_gamma; p.kbeta = (const uint16_t*)k_beta; p.kalpha = k_alpha;
    p.vx = (const uint16_t*)value_x; p.vy = (const _Float16*)value_y; p.vgamma = (const uint16_t*)v_gamma; p.vbeta = (const uint16_t*)v_beta; p.valpha = v_alpha;
    p.alpha_f32 = alpha_dt == HICOM_DT_F32; p.eps = eps; p.guide = (const uint16_t*)guide;
    p.items = t.items; p.win_item = t.win_item; p.ay = ax.ay; p.ax = ax.ax;
    p.scale = a->l_scale; p.dctx = dctx; p.ds = ds; p.pw = pw; p.sxk = sxk; p.syk = syk; p.sxv = sxv; p.syv = syv;
    HICOM_LAUNCH(ragged_local_attn_adapt_bwd_kernel<3>, dim3((unsigned)t.l.s.n.windows), dim3(256), ragged_window_bwd_smem(a, 6), (hipStream_t)a->stream,
                 p);                                           // (E == 1152: ragged_check)
    return seg_check_launch(who, "window backward");
}

extern "C" int hicom_compressor_ragged_adapt_dy(const hicom_compressor_ragged_args* a, const void* y, const void* gamma, const void* vec, int32_t vec_dt,
                                                int32_t vec_per_item, const float* coef, const void* alpha, int32_t alpha_dt, float eps, void* dy, void* r1,
                                                float* col_parts, int32_t nparts) {
    constexpr const char* who = "compressor_ragged_adapt_dy";
    HICOM_TRY(ragged_check(a, nullptr));
    HICOM_REQUIRE(y && gamma && vec && coef && alpha && dy && (!col_parts || nparts > 0), HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE((vec_dt == HICOM_DT_BF16 || vec_dt == HICOM_DT_F32) && (alpha_dt == HICOM_DT_BF16 || alpha_dt == HICOM_DT_F32), HICOM_EINVAL, "%s: dtypes", who);
    HICOM_REQUIRE((uintptr_t)y % 4 == 0 && (uintptr_t)gamma % 4 == 0 && (uintptr_t)vec % 4 == 0 && (uintptr_t)coef % 4 == 0 && (uintptr_t)dy % 4 == 0 &&
                      (uintptr_t)r1 % 4 == 0 && (uintptr_t)col_parts % 4 == 0, HICOM_EINVAL, "%s: 4-byte aligned rows", who);
    RaggedTables t;
    HICOM_TRY(ragged_adapt_tables(who, a, t));
    const RaggedAxes ax = ragged_axes(a);
    const long tokens = t.l.s.n.tokens;
    RaggedAdaptDyParams p;
    p.y = (const _Float16*)y; p.gamma = (const uint16_t*)gamma; p.vec = vec; p.vec_f32 = vec_dt == HICOM_DT_F32; p.vec_per_item = vec_per_item ? 1 : 0;
    p.coef = coef; p.alpha = alpha; p.alpha_f32 = alpha_dt == HICOM_DT_F32; p.eps = eps;
    p.items = t.items; p.B = a->B; p.ay = ax.ay; p.ax = ax.ax;
    p.dy = (uint16_t*)dy; p.r1 = (uint16_t*)r1; p.N = tokens; p.col_parts = col_parts;
    // with column partials: `nparts` workgroups walk the tokens (each leaves one partial row); without: one token per wave
    const unsigned grid = col_parts ? (unsigned)nparts : (unsigned)((tokens + 3) / 4);
    HICOM_LAUNCH(ragged_adapt_dy_kernel<3>, dim3(grid), dim3(256), 0, (hipStream_t)a->stream, p);      // (E == 1152: ragged_check)
    return seg_check_launch(who, "adapt dy");
}

extern "C" int hicom_compressor_ragged_dq_item(const hicom_compressor_ragged_args* a, const float* dq, float* dq_item) {
    constexpr const char* who = "compressor_ragged_dq_item";
    HICOM_TRY(ragged_check(a, nullptr));
    HICOM_REQUIRE(dq && dq_item, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE((uintptr_t)dq % 16 == 0 && (uintptr_t)dq_item % 16 == 0, HICOM_EINVAL, "%s: 16-byte aligned pointers", who);
    RaggedTables t;
    HICOM_TRY(ragged_adapt_tables(who, a, t));
    return ragged_launch_dq_item(who, a, t, dq, dq_item);
}

// the y planes of the adapted streams out of the adaptor regions of the workspace (hicom_compressor_ragged_adapt_fwd left them there)
extern "C" int hicom_compressor_ragged_adapt_train_state(const hicom_compressor_ragged_adapt_args* args, void* ky_out, void* vy_out) {
    constexpr const char* who = "compressor_ragged_adapt_train_state";
    return seg_with_adapt(who, args, [&](const hicom_compressor_ragged_args* a, const SegAdapt* ad) -> int {
        HICOM_TRY(ragged_check(a, ad));
        HICOM_REQUIRE(ky_out || vy_out, HICOM_EINVAL, "%s: NULL pointer", who);
        HICOM_REQUIRE((!ky_out || ad->k()) && (!vy_out || ad->v()), HICOM_EINVAL, "%s: a y plane of a stream without adaptor", who);
        RaggedTables t;
        HICOM_TRY(ragged_tables(who, a, ad, t));
        hipStream_t s = (hipStream_t)a->stream;
        const size_t bytes = (size_t)(t.l.s.n.tokens * a->E * 2);
        if ((ky_out && hipMemcpyAsync(ky_out, t.ws + t.l.s.ad.ky, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) ||
            (vy_out && hipMemcpyAsync(vy_out, t.ws + t.l.s.ad.vy, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess)) {
            set_error("%s: copying the state: %s", who, hipGetErrorString(hipGetLastError()));
            return HICOM_ELAUNCH;
        }
        return HICOM_OK;
    });
}
