// Training surface of the ragged multi-guide compressor step (hicom_amd/ragged_multi_guide_train.py): what a backward over all M = sum Q_i
// (item, guide) pairs of a mixed batch launches.  The forward is ragged_multi_guide.hip's; every call here reads the table region
// hicom_compressor_ragged_multiguide_prepare left at the head of the workspace (item table, work units, pair table:
// ragged_multi_guide_host.hpp) and finds its item and its slots the way the forward does.
//   hicom_compressor_ragged_multiguide_train_state  hands the forward's state out of the workspace: the fp16 window contexts of all pairs,
//       the scores region, the merged contexts, and (M, L) per (pair, head) from the partial states in merge_segments' own order.
//   hicom_compressor_ragged_multiguide_global_bwd   the global stage's attention backward over all pairs on the forward's unit table: the
//       same stream_segment with two row groups in StreamMode::Bwd -- an item's tokens are read once per 32 folded rows, as in the forward
//       -- then dq_merge_segments per (pair, head).
// Input gradients (stage 3): a token's gradient is a sum over its item's Q_i guides, formed in fp32 and written once.
//   hicom_compressor_ragged_multiguide_local_bwd    the window backward over the sum windows_i windows of the stacked tensor (multi_window.hpp:
//       multi_window_bwd): dq f32 per (pair, window) in ctx16's pair-major order, d frames_embed and the local share of d frames_feature
//       as bf16 rows, plain stores -- the windows of an item partition it
//   hicom_compressor_ragged_multiguide_dq_pair      dq summed per pair in a fixed order (window_rows.hpp: sum_rows_striped)
//   hicom_compressor_ragged_multiguide_global_dx    the global stage's d x with 64 tokens of one item per workgroup over all nh Q_i rows of
//       the item (global_dx.hpp: global_dx_rows_tile), added into the rows the window backward left
// Row space of an item, passes and slot order [item][pass][row group][chunk]: ragged_multi_guide.hip.  Row R = nh q + h of item i lives in
// the slots slot0_i + (R >> 4) chunks_i .. + chunks_i - 1, row R & 15 of each.
// Every entry point opens alike: rmg_check (no device), the call's own pointer checks, then rmg_tables (layout, workspace check, typed
// pointers into the table region).
#include "global_dx.hpp"
#include "ragged_multi_guide_host.hpp"

namespace hicom {

// ---- (M, L) per (pair, head) from the partial states, merge_segments' own order.  grid = M, 64 threads ----
__global__ __launch_bounds__(64) void rmg_state_ml_kernel(const float* part_m, const float* part_l, const RmgItem* items, const RmgPair* pairs, int rows,
                                                          float* ml) {
    const int pair = blockIdx.x, r = threadIdx.x;
    if (r >= rows) return;
    const RmgPair pr = pairs[pair];
    const RmgItem it = items[pr.item];
    const int R = pr.q * rows + r;                              // the head's row in the item's row space
    const long pbase = ((long)it.slot0 + (long)(R >> 4) * it.chunks) * 16 + (R & 15);
    float M = -1.0e30f;
    for (int c = 0; c < it.chunks; ++c) M = fmaxf(M, part_m[pbase + c * 16]);
    float L = 0.f;
    for (int c = 0; c < it.chunks; ++c) L += part_l[pbase + c * 16] * expf(part_m[pbase + c * 16] - M);
    ml[2 * ((long)pair * rows + r)] = M;
    ml[2 * ((long)pair * rows + r) + 1] = L;
}

// ---- the segmented backward of the many-row stream, the forward's unit table and slots (stream_body.hpp: StreamMode::Bwd, two row groups).
// c.qhi / c.qlo: the planes of dctx, c.pos_a: pos_b = dctx . pe^T, c.part_acc: partial sums of dS x; part_m / part_l are not written.
// ml / delta are pair-major like the query planes: the rows of item i begin at row nh pair0_i, in the item's row space from there ----
struct RmgStreamBwdParams {
    SegStreamParams c;
    const uint16_t* x;      // [sum N_i][E]
    const float* s_in;      // the forward's scores region
    const float* ml;        // [M * rows][2]
    const float* delta;     // [M * rows]
    float* ds;              // laid out as s_in
    const RmgUnit* units;
    const RmgItem* items;
};

template <int NB>
__global__ __launch_bounds__(512, 1) void rmg_stream_bwd_kernel(RmgStreamBwdParams p) {
    constexpr int E = NB * 128;
    const RmgUnit u = p.units[blockIdx.x];
    const RmgItem it = p.items[u.item];
    const long qrow0 = (long)it.pair0 * p.c.rows;
    StreamModeArgs ma{};
    ma.s_in = p.s_in + (long)it.score_off * 16;
    ma.ml = p.ml + 2 * qrow0;
    ma.delta = p.delta + qrow0;
    stream_segment<NB, 2, StreamMode::Bwd>(p.c, p.x + (long)it.tok0 * E, it.N, u.tb, u.te, 32 * u.pass, p.c.rows * it.Q, qrow0,
                                           p.ds + (long)it.score_off * 16, (long)((it.N + 15) / 16 * 16), (long)u.slot, it.chunks, ma);
}

// ---- dq merge per (pair, head), grid = (heads, M), the forward merge's LDS ----
struct RmgDqMergeParams {
    SegDqMergeParams c;
    const float* ds;
    const RmgItem* items;
    const RmgPair* pairs;
    int rows;               // heads
    float* dqt;             // [M * rows][E]
};

__global__ __launch_bounds__(256) void rmg_dq_merge_kernel(RmgDqMergeParams p) {
    extern __shared__ float ms[];
    const int h = blockIdx.x, pair = blockIdx.y;
    const RmgPair pr = p.pairs[pair];
    const RmgItem it = p.items[pr.item];
    const int R = pr.q * p.rows + h;                            // the head's row in the item's row space
    const long stride = (it.N + 15) / 16 * 16;
    dq_merge_segments(p.c, ms, R & 15, threadIdx.x, it.T, it.chunks, (long)it.slot0 + (long)(R >> 4) * it.chunks,
                      p.ds + (long)it.score_off * 16 + R * stride, p.dqt + ((long)pair * p.rows + h) * p.c.E);
}

// ---- input gradients: the window backward, one 4-wave workgroup per window of the STACKED tensor (sum windows_i of them, not one per
// (pair, window)): the window's key and value rows serve all Q_i guides of its item (multi_window.hpp: multi_window_bwd).  Item lookup,
// window geometry and the pair-major context rows as in rmg_local_kernel ----
struct RmgLocalBwdParams {
    const uint16_t* key;
    const uint16_t* value;
    const uint16_t* guide;  // [M][D]
    const RmgItem* items;
    const int* win_item;
    hicom_axis ay, ax;
    float scale;
    const float* dctx;      // [sum Q_i windows_i][D], pair-major as ctx16
    float* dq;              // likewise
    uint16_t* dkey;         // bf16 [sum N_i][D] or NULL
    uint16_t* dvalue;       // bf16 [sum N_i][D] or NULL
    int value_is_key;
};

template <int NV>
__global__ __launch_bounds__(256) void rmg_local_bwd_kernel(RmgLocalBwdParams p) {
    constexpr int D = NV * 384;
    extern __shared__ __attribute__((aligned(16))) float lsm[];
    const int win = blockIdx.x;
    const RmgItem it = p.items[p.win_item[win]];
    const hicom_axis at{it.T, it.kt, it.T / it.kt, it.T / it.kt};
    const int wi = (it.T / it.kt) * p.ay.nwin * p.ax.nwin;      // windows of the item = context rows of one pair
    const WindowGeom g(at, p.ay, p.ax, win - it.win0);
    const long first = (long)it.tok0 * D, row = ((long)it.ctx_row0 + (win - it.win0)) * D;
    const MultiWindowBwdArgs a{p.key + first, p.value + first, p.guide + (long)it.pair0 * D, it.Q, p.scale, p.dctx + row, p.dq + row, (long)wi * D,
                               p.dkey ? p.dkey + first : nullptr, p.dvalue ? p.dvalue + first : nullptr, p.value_is_key};
    multi_window_bwd<NV>(a, g, lsm, threadIdx.x);
}

// ... and the local share of d guide: dq_pair[p] = the sum of pair p's window rows of dq.  grid = (E / 64, M), 256 threads
__global__ __launch_bounds__(256) void rmg_dq_pair_kernel(const float* dq, const RmgItem* items, const RmgPair* pairs, int wps, int E, float* dq_pair) {
    __shared__ float4 red[16][16];
    const RmgPair pr = pairs[blockIdx.y];
    const RmgItem it = items[pr.item];
    sum_rows_striped(dq, (long)pr.ctx_row0, (it.T / it.kt) * wps, E, dq_pair + (long)blockIdx.y * E, red);
}

// ---- input gradients: d x of the global stage for Q_i guides.  A workgroup takes 64 tokens of ONE item (tiles: {item, first token of the
// tile inside the item}, hicom_amd/ragged.py: dx_tile_table on the step's tables) and all nh Q_i rows of the item's row space: row R of
// the logits and of dS at R * stride behind the item's score_off (row0 = 32 pass of the stream's passes: the passes are dense), its
// (M, L), qt and dctx rows at nh pair0_i + R ----
struct RmgGlobalDxParams {
    const float* S;         // the forward's scores region
    const float* dS;        // laid out as S
    const float* ml;        // [M * rows][2]
    const float* qt;        // [M * rows][E]
    const float* dctx;      // [M * rows][E]
    const int2* tiles;
    const RmgItem* items;
    int B, rows, E;         // rows: heads
    uint16_t* dx;           // [sum N_i][E]
    int accumulate;
};

__global__ __launch_bounds__(320) void rmg_global_dx_kernel(RmgGlobalDxParams p) {
    __shared__ __attribute__((aligned(16))) float coef[kDxSubTile][kDxCoefStride];
    const int2 tile = p.tiles[blockIdx.x];
    if (tile.x < 0 || tile.x >= p.B) return;            // (a table that is not this plan's: nothing is indexed through it)
    const RmgItem it = p.items[tile.x];
    if (tile.y < 0 || tile.y >= it.N) return;
    const long row0 = (long)it.pair0 * p.rows, stride = (it.N + 15) / 16 * 16;
    global_dx_rows_tile(p.S + (long)it.score_off * 16, p.dS + (long)it.score_off * 16, stride, p.ml + 2 * row0, p.qt + row0 * p.E, p.dctx + row0 * p.E,
                        p.rows * it.Q, (long)tile.y, (long)it.N, p.E, p.dx + (long)it.tok0 * p.E, p.accumulate, coef);
}

}  // namespace hicom

using namespace hicom;
using namespace hicom_host;

namespace {

struct RmgTables {
    RmgLayout l;
    const char* ws;
    const RmgItem* items;
    const RmgUnit* units;
    const RmgPair* pairs;
};

int rmg_tables(const char* who, const Args* a, RmgTables& t) {
    t.l = rmg_layout(a);
    HICOM_TRY(seg_check_ws(who, a, t.l.s.total));               // (the table region at its head is what the training calls read)
    t.ws = (const char*)a->ws;
    t.items = (const RmgItem*)(t.ws + t.l.items);
    t.units = (const RmgUnit*)(t.ws + t.l.units);
    t.pairs = (const RmgPair*)(t.ws + t.l.pairs);
    return HICOM_OK;
}

struct RmgBwdLayout { long dhi, dlo, pos_b, part_acc, total; };

RmgBwdLayout rmg_bwd_layout(const Args* a, const RmgLayout& l) {
    RmgBwdLayout b{};
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

extern "C" int hicom_compressor_ragged_multiguide_train_state(const hicom_compressor_ragged_multiguide_args* a, void* ctx16_out, float* scores_out,
                                                              float* ml_out, float* ctxg_out) {
    constexpr const char* who = "compressor_ragged_multiguide_train_state";
    HICOM_TRY(rmg_check(a));
    HICOM_REQUIRE(ctx16_out && scores_out && ml_out && ctxg_out, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE((uintptr_t)ctx16_out % 2 == 0 && (uintptr_t)scores_out % 4 == 0 && (uintptr_t)ml_out % 4 == 0 && (uintptr_t)ctxg_out % 4 == 0, HICOM_EINVAL,
                  "%s: aligned pointers", who);
    RmgTables t;
    HICOM_TRY(rmg_tables(who, a, t));
    const SegLayout& l = t.l.s;
    hipStream_t s = (hipStream_t)a->stream;
    const long E = a->E;
    if (hipMemcpyAsync(ctx16_out, t.ws + l.ctx16, (size_t)(l.n.windows * E * 2), hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(scores_out, t.ws + l.scores, (size_t)(l.n.score_floats * 4), hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(ctxg_out, t.ws + l.ctxg, (size_t)(l.n.rows * E * 4), hipMemcpyDeviceToDevice, s) != hipSuccess) {
        set_error("%s: copying the state: %s", who, hipGetErrorString(hipGetLastError()));
        return HICOM_ELAUNCH;
    }
    HICOM_LAUNCH(rmg_state_ml_kernel, dim3((unsigned)t.l.M), dim3(64), 0, s, (const float*)(t.ws + l.part_m), (const float*)(t.ws + l.part_l), t.items, t.pairs,
                 a->nh, ml_out);
    return seg_check_launch(who, "softmax state");
}

extern "C" int64_t hicom_compressor_ragged_multiguide_global_bwd_workspace_bytes(const hicom_compressor_ragged_multiguide_args* a) {
    HICOM_TRY(rmg_check(a));
    return rmg_bwd_layout(a, rmg_layout(a)).total;
}

extern "C" int hicom_compressor_ragged_multiguide_global_bwd(const hicom_compressor_ragged_multiguide_args* a, const void* x, const float* dctx,
                                                             const float* delta, const float* scores, const float* ml, float* ds_out, float* dqt_out,
                                                             void* bws, int64_t bws_bytes) {
    constexpr const char* who = "compressor_ragged_multiguide_global_bwd";
    HICOM_TRY(rmg_check(a));
    HICOM_REQUIRE(x && dctx && delta && scores && ml && ds_out && dqt_out, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)scores % 16 == 0 && (uintptr_t)ds_out % 16 == 0 && (uintptr_t)dctx % 16 == 0 &&
                      (uintptr_t)dqt_out % 16 == 0 && (uintptr_t)ml % 8 == 0 && (uintptr_t)delta % 4 == 0, HICOM_EINVAL, "%s: 16-byte aligned inputs", who);
    HICOM_REQUIRE(ds_out != scores, HICOM_EINVAL, "%s: dS cannot overwrite the logits", who);
    RmgTables t;
    HICOM_TRY(rmg_tables(who, a, t));
    const RmgBwdLayout b = rmg_bwd_layout(a, t.l);
    HICOM_REQUIRE(bws && bws_bytes >= b.total && (uintptr_t)bws % 256 == 0, HICOM_EINVAL, "%s: backward workspace of %ld bytes, 256-byte aligned", who, b.total);
    char* w = (char*)bws;
    const int R = (int)t.l.s.n.rows, E = a->E;
    hipStream_t s = (hipStream_t)a->stream;

    // 1: dctx -> bf16 hi / lo planes
    HICOM_TRY(hicom_split_bf16_fwd(dctx, R, R, E, w + b.dhi, w + b.dlo, a->stream));
    // 2: the score-side positional table of dP
    float* pos_b = a->pe ? (float*)(w + b.pos_b) : nullptr;
    if (a->pe) HICOM_TRY(hicom_linear_fwd(dctx, HICOM_DT_F32, a->pe, HICOM_DT_F32, nullptr, 0, nullptr, 0, R, a->P, E, 0, 0, HICOM_ACT_NONE, pos_b, a->stream));
    // 3: the segmented backward stream, one 512-thread workgroup per work unit of the forward
    {
        RmgStreamBwdParams p;
        p.c.qhi = (const uint16_t*)(w + b.dhi); p.c.qlo = (const uint16_t*)(w + b.dlo);
        p.c.pos_a = pos_b; p.c.pos_stride = a->P; p.c.rows = a->nh;
        p.c.H = a->H; p.c.W = a->W; p.c.HW = a->H * a->W;
        p.c.t0i = a->t_index0; p.c.y0i = a->y_index0; p.c.x0i = a->x_index0;
        p.c.part_m = nullptr; p.c.part_l = nullptr; p.c.part_acc = (float*)(w + b.part_acc);
        p.x = (const uint16_t*)x; p.s_in = scores; p.ml = ml; p.delta = delta; p.ds = ds_out;
        p.units = t.units; p.items = t.items;
        static bool attr_set = false;
        if (!attr_set) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(rmg_stream_bwd_kernel<9>), hipFuncAttributeMaxDynamicSharedMemorySize, seg_stream_smem(2));
            attr_set = true;
        }
        HICOM_LAUNCH(rmg_stream_bwd_kernel<9>, dim3((unsigned)t.l.nunits), dim3(512), seg_stream_smem(2), s, p);
        HICOM_TRY(seg_check_launch(who, "backward stream"));
    }
    // 4: dq merge per (pair, head)
    RmgDqMergeParams p;
    p.c.part_acc = (const float*)(w + b.part_acc); p.c.pe = a->pe; p.c.E = E; p.c.H = a->H; p.c.W = a->W;
    p.c.t0i = a->t_index0; p.c.y0i = a->y_index0; p.c.x0i = a->x_index0;
    p.ds = ds_out; p.items = t.items; p.pairs = t.pairs; p.rows = a->nh; p.dqt = dqt_out;
    HICOM_LAUNCH(rmg_dq_merge_kernel, dim3((unsigned)a->nh, (unsigned)t.l.M), dim3(256), (size_t)seg_merge_smem(t.l.max_T, a->H, a->W), s, p);
    return seg_check_launch(who, "dq merge");
}

// ---- input gradients (stage 3): the window backward over all windows, dq per pair, and d x of the global stage ----------------------------
extern "C" int hicom_compressor_ragged_multiguide_local_bwd(const hicom_compressor_ragged_multiguide_args* a, const void* key, const void* value,
                                                            const void* guide, const float* dctx, float* dq, void* dkey, void* dvalue, int32_t value_is_key) {
    constexpr const char* who = "compressor_ragged_multiguide_local_bwd";
    HICOM_TRY(rmg_check(a));
    HICOM_REQUIRE(key && value && guide && dctx && dq, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE(!(value_is_key && dkey), HICOM_EINVAL, "%s: value_is_key writes the summed gradient to dvalue (dkey must be NULL)", who);
    HICOM_REQUIRE(!value_is_key || key == value, HICOM_EINVAL, "%s: value_is_key: the keys are the value rows", who);
    HICOM_REQUIRE((uintptr_t)key % 4 == 0 && (uintptr_t)value % 4 == 0 && (uintptr_t)guide % 4 == 0 && (uintptr_t)dctx % 16 == 0 && (uintptr_t)dq % 16 == 0 &&
                      (uintptr_t)dkey % 4 == 0 && (uintptr_t)dvalue % 4 == 0, HICOM_EINVAL, "%s: aligned pointers", who);
    HICOM_REQUIRE(dkey != key && dkey != value && dvalue != key && dvalue != value && (!dkey || dkey != dvalue), HICOM_EINVAL,
                  "%s: a gradient cannot overwrite the tokens or the other gradient", who);
    RmgTables t;
    HICOM_TRY(rmg_tables(who, a, t));
    int max_kt = 1, max_q = 1;
    for (int i = 0; i < a->B; ++i) {
        max_kt = a->items[i].kt > max_kt ? a->items[i].kt : max_kt;
        max_q = a->guide_counts[i] > max_q ? a->guide_counts[i] : max_q;
    }
    RmgLocalBwdParams p;
    p.key = (const uint16_t*)key; p.value = (const uint16_t*)value; p.guide = (const uint16_t*)guide;
    p.items = t.items; p.win_item = (const int*)(t.ws + t.l.win_item);
    p.ay = hicom_axis{a->H, a->ks, a->H / a->ks, a->H / a->ks}; p.ax = hicom_axis{a->W, a->ks, a->W / a->ks, a->W / a->ks};
    p.scale = a->l_scale; p.dctx = dctx; p.dq = dq; p.dkey = (uint16_t*)dkey; p.dvalue = (uint16_t*)dvalue; p.value_is_key = value_is_key ? 1 : 0;
    // (E == 1152 and WIN <= 64: rmg_check; Q <= 32: 16 KiB of coefficients + the 18 KiB slab at the most)
    HICOM_LAUNCH(rmg_local_bwd_kernel<3>, dim3((unsigned)t.l.item_windows), dim3(256), multi_window_bwd_smem(max_q, max_kt * a->ks * a->ks, a->E),
                 (hipStream_t)a->stream, p);
    return seg_check_launch(who, "window backward");
}

extern "C" int hicom_compressor_ragged_multiguide_dq_pair(const hicom_compressor_ragged_multiguide_args* a, const float* dq, float* dq_pair) {
    constexpr const char* who = "compressor_ragged_multiguide_dq_pair";
    HICOM_TRY(rmg_check(a));
    HICOM_REQUIRE(dq && dq_pair, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE((uintptr_t)dq % 16 == 0 && (uintptr_t)dq_pair % 16 == 0 && a->E % 4 == 0, HICOM_EINVAL, "%s: 16-byte aligned rows", who);
    RmgTables t;
    HICOM_TRY(rmg_tables(who, a, t));
    HICOM_LAUNCH(rmg_dq_pair_kernel, dim3((unsigned)((a->E + 63) / 64), (unsigned)t.l.M), dim3(256), 0, (hipStream_t)a->stream, dq, t.items, t.pairs, t.l.wps,
                 a->E, dq_pair);
    return seg_check_launch(who, "dq per pair");
}

extern "C" int hicom_compressor_ragged_multiguide_global_dx(const hicom_compressor_ragged_multiguide_args* a, const float* scores, const float* ds,
                                                            const float* ml, const float* qt, const float* dctx, const int32_t* tiles, int32_t ntiles, void* dx,
                                                            int32_t accumulate) {
    constexpr const char* who = "compressor_ragged_multiguide_global_dx";
    HICOM_TRY(rmg_check(a));
    HICOM_REQUIRE(scores && ds && ml && qt && dctx && tiles && dx, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE((uintptr_t)dx % 8 == 0 && (uintptr_t)qt % 16 == 0 && (uintptr_t)dctx % 16 == 0 && (uintptr_t)tiles % 8 == 0 && (uintptr_t)scores % 4 == 0 &&
                      (uintptr_t)ds % 4 == 0 && (uintptr_t)ml % 4 == 0, HICOM_EINVAL, "%s: aligned pointers", who);
    HICOM_REQUIRE(a->nh > 0 && a->E % 4 == 0 && a->E <= 1280, HICOM_EUNSUP, "%s: nh=%d, E=%d (<= 1280, %% 4)", who, a->nh, a->E);
    long want = 0;
    for (int i = 0; i < a->B; ++i) want += ((long)a->items[i].T * a->H * a->W + 63) / 64;
    HICOM_REQUIRE(ntiles == want, HICOM_EINVAL, "%s: %d tiles, the items have %ld tiles of 64 tokens", who, ntiles, want);
    RmgTables t;
    HICOM_TRY(rmg_tables(who, a, t));
    RmgGlobalDxParams p;
    p.S = scores; p.dS = ds; p.ml = ml; p.qt = qt; p.dctx = dctx; p.tiles = (const int2*)tiles;
    p.items = t.items;
    p.B = a->B; p.rows = a->nh; p.E = a->E; p.dx = (uint16_t*)dx; p.accumulate = accumulate ? 1 : 0;
    HICOM_LAUNCH(rmg_global_dx_kernel, dim3((unsigned)ntiles), dim3(320), 0, (hipStream_t)a->stream, p);
    return seg_check_launch(who, "global dx");
}
