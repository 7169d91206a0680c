// Local compressor: windowed single-head cross-attention as ONE streaming pass.
//
// Replaces LocalCompressor.forward's divide_feature x3 + bmm + softmax + bmm + un-window
// (reference projector.py:544-558).  The window regroup is pure address arithmetic here
// (zero bytes moved); every key row and every value row is read from HBM exactly once.
//
// Mapping: one 256-thread workgroup (4 waves) per window.  A token row of D bf16 channels is
// spread over the 64 lanes of a wave as NV segments of 64 x 12 B (global_load_dwordx3, fully
// coalesced 768-B runs; the 3 tokens of a window row are contiguous in HBM).  Wave w scores
// tokens w, w+4, ... with a 64-lane shuffle reduction, the softmax over the <= few-hundred
// window scores is done in LDS, then the same wave->token assignment accumulates p * value in
// fp32 registers and the four partial rows are summed through LDS.
//
// Roofline: HBM-bound streaming (4*D flop per 4*D bytes); no MFMA on purpose -- one query row
// per window with private keys is a block-diagonal M=1 product (SURVEY.md §7 "Where MFMA applies").
//
// Five kernels: the forward, the forward with the adaptor blends fused into the row loads, their two backwards, and adapt_dy (the
// LayerNorm-blend backward per token).  Each window kernel reads "geometry, query, phase 1 (scores), softmax statistics, phase 2
// (weighted sums), reduce over the four waves"; the parts they share -- WindowGeom, the row loads and row primitives, ln_stats,
// affine_prep / blend_dot, softmax_stats, the partial rows through LDS -- are in window_rows.hpp.  The kernels stay separate on
// purpose: tokens in flight per wave (3 / 2 / 2 / 1) and register budgets were sized one by one.
#include "window_rows.hpp"

namespace hicom {

struct LocalParams {
    const void* key;
    const void* value;
    int key_f32, value_f32;      // stream dtype code: 0 = bf16 (raw tokens), 1 = fp32, 2 = fp16 (alpha-blended adaptor outputs)
    const void* query;
    int query_f32;
    long query_stride;
    hicom_axis at, ay, ax;
    float scale, bias;
    int l2norm;
    float* ctx;
    _Float16* ctx16;             // fp16 [Nw, D] (saturating) instead of / beside ctx: the operand of hicom_readout16_gemm_fwd, or NULL
};

template <int NV>
__global__ __launch_bounds__(256) void local_attn_kernel(LocalParams p) {
    constexpr int D = NV * 384;
    extern __shared__ __attribute__((aligned(16))) float lsm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int win = blockIdx.x;
    const WindowGeom w(p.at, p.ay, p.ax, win);
    const int WIN = w.WIN;
    float* sc = lsm;                              // [WIN] scores
    float* part = lsm + ((WIN + 3) & ~3);         // [4][D] partial contexts

    float q[NV][6];
    load_query<NV>(p.query, p.query_f32, p.query_stride, win, lane, q);
    if (p.l2norm & 2) {   // clip-scale variant: guide / ||guide||  (projector.py:529)
        float qq = 0.f;
#pragma unroll
        for (int s = 0; s < NV; ++s)
#pragma unroll
            for (int j = 0; j < 6; ++j) qq += q[s][j] * q[s][j];
        const float inv = 1.0f / sqrtf(wave_sum_fast(qq));
#pragma unroll
        for (int s = 0; s < NV; ++s)
#pragma unroll
            for (int j = 0; j < 6; ++j) q[s][j] *= inv;
    }

    // ---- phase 1: scores ---------------------------------------------------------------
    for (int i0 = wave; i0 < WIN; i0 += 12) {     // up to 3 tokens in flight per wave
        float k[3][NV][6];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int i = i0 + 4 * u;
            if (i < WIN) load_stream_row<NV>(p.key, p.key_f32, w.token_of(i), lane, k[u]);
        }
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int i = i0 + 4 * u;
            if (i < WIN) {
                float dot = wave_sum_fast(row_dot<NV>(q, k[u]));
                const float kk = row_dot<NV>(k[u], k[u]);
                if (p.l2norm & 1) dot /= sqrtf(wave_sum_fast(kk));   // frames_embed / ||.||  (:528)
                if (lane == 0) sc[i] = dot * p.scale + p.bias;
            }
        }
    }
    __syncthreads();
    float mx, inv_sum;
    softmax_stats(sc, WIN, lane, mx, inv_sum);

    // ---- phase 2: context = sum_i p_i * value_i ---------------------------------------------
    float acc[NV][6];
    row_zero<NV>(acc);
    for (int i0 = wave; i0 < WIN; i0 += 12) {
        float v[3][NV][6];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int i = i0 + 4 * u;
            if (i < WIN) load_stream_row<NV>(p.value, p.value_f32, w.token_of(i), lane, v[u]);
        }
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int i = i0 + 4 * u;
            if (i < WIN) row_axpy<NV>(expf(sc[i] - mx) * inv_sum, v[u], acc);
        }
    }
    store_partial_row<NV>(part, wave, lane, acc);
    __syncthreads();
    sum_partial_rows<NV>(part, tid, [&](int c, float v) {
        if (p.ctx) p.ctx[(long)win * D + c] = v;
        if (p.ctx16) p.ctx16[(long)win * D + c] = (_Float16)fminf(fmaxf(v, -65504.f), 65504.f);
    });
}

// ---- windowed attention with the adaptor blend fused into the row loads ("fused into the K/V tile load") -------
// adapt_k / adapt_v (reference projector.py:533-534):  key_n = (1 - a_k) x_n + a_k (LN(y_n) gamma_k + beta_k)  with y = k_proj(x) from the
// two dense GEMMs, likewise for the values.  The blended streams never exist: a wave that holds a token's x row and y row computes
//   logit_n = (1 - a) q.x_n + a (rstd_n ((q gamma).y_n - mu_n sum(q gamma)) + q.beta)                      (four wave reductions)
//   ctx     = (1 - a) sum_n p_n v_n + a (gamma (sum_n p_n rstd_n y_n - sum_n p_n rstd_n mu_n) + beta)       (two accumulators)
// with mu_n, rstd_n the LayerNorm statistics of y_n over D (fp32, from the row in registers).  Saves, per adapted stream, the
// LayerNorm-blend pass (107 MB fp16 + 107 MB bf16 read, 107 MB written) and costs one more 107-MB row read here.
struct LocalAdaptParams {
    const uint16_t* kx;        // key source tokens bf16 [N, D]
    const _Float16* ky;        // k_proj(kx) fp16 [N, D] or NULL (no key adaptor: key = kx)
    const uint16_t* kgamma; const uint16_t* kbeta; const void* kalpha;
    const uint16_t* vx;        // value source tokens bf16 [N, D]
    const _Float16* vy;        // v_proj(vx) fp16 [N, D] or NULL
    const uint16_t* vgamma; const uint16_t* vbeta; const void* valpha;
    int alpha_f32;
    float eps;
    const void* query;
    int query_f32;
    long query_stride;
    hicom_axis at, ay, ax;
    float scale, bias;
    float* ctx;
};

template <int NV>
__global__ __launch_bounds__(256) void local_attn_adapt_kernel(LocalAdaptParams p) {
    constexpr int D = NV * 384;
    extern __shared__ __attribute__((aligned(16))) float lsm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int win = blockIdx.x;
    const WindowGeom w(p.at, p.ay, p.ax, win);
    const int WIN = w.WIN;
    float* sc = lsm;                              // [WIN] scores
    float* part = lsm + ((WIN + 3) & ~3);         // [4][D] partial contexts (x part, then y part)
    const float ak = p.ky ? read_alpha(p.kalpha, p.alpha_f32) : 0.f, av = p.vy ? read_alpha(p.valpha, p.alpha_f32) : 0.f;

    float q[NV][6];
    load_query<NV>(p.query, p.query_f32, p.query_stride, win, lane, q);
    // q gamma_k (the query seen by the normalised y row), sum(q gamma_k), q . beta_k
    float qg[NV][6];
    float cg = 0.f, cb = 0.f;
    if (p.ky) affine_prep<NV>(q, p.kgamma, p.kbeta, lane, qg, cg, cb);

    // ---- phase 1: scores ---------------------------------------------------------------
    for (int i0 = wave; i0 < WIN; i0 += 8) {      // 2 tokens (x row + y row each) in flight per wave
        float kx[2][NV][6], ky[2][NV][6];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = i0 + 4 * u;
            if (i < WIN) {
                const long tok = w.token_of(i);
                load_row<NV>(p.kx + tok * D, lane, kx[u]);
                if (p.ky) load_row_f16<NV>(p.ky + tok * D, lane, ky[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = i0 + 4 * u;
            if (i < WIN) {
                float mu, rstd;
                const float logit = blend_dot<NV>(kx[u], ky[u], p.ky != nullptr, q, qg, cg, cb, ak, p.eps, mu, rstd);
                if (lane == 0) sc[i] = logit * p.scale + p.bias;
            }
        }
    }
    __syncthreads();
    float mx, inv_sum;
    softmax_stats(sc, WIN, lane, mx, inv_sum);

    // ---- phase 2: context ----------------------------------------------------------------
    float accx[NV][6], accy[NV][6];
    float smu = 0.f;                                // sum_n p_n rstd_n mu_n (identical in every lane)
    row_zero<NV>(accx);
    row_zero<NV>(accy);
    for (int i0 = wave; i0 < WIN; i0 += 8) {
        float vx[2][NV][6], vy[2][NV][6];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = i0 + 4 * u;
            if (i < WIN) {
                const long tok = w.token_of(i);
                load_row<NV>(p.vx + tok * D, lane, vx[u]);
                if (p.vy) load_row_f16<NV>(p.vy + tok * D, lane, vy[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = i0 + 4 * u;
            if (i < WIN) {
                const float pi = expf(sc[i] - mx) * inv_sum;
                float wy = 0.f;
                if (p.vy) {
                    float mu, rstd;
                    ln_stats<NV>(vy[u], p.eps, mu, rstd);
                    wy = pi * rstd;
                    smu = fmaf(wy, mu, smu);
                }
                row_axpy<NV>(pi, vx[u], accx);
                if (p.vy) row_axpy<NV>(wy, vy[u], accy);
            }
        }
    }
    // per-wave blend (linear in the accumulators, so the four waves' results simply add: the beta term once, by wave 0)
    if (p.vy) {
        float g[NV][6], b[NV][6];
        load_row<NV>(p.vgamma, lane, g);
        load_row<NV>(p.vbeta, lane, b);
#pragma unroll
        for (int s = 0; s < NV; ++s)
#pragma unroll
            for (int j = 0; j < 6; ++j)
                accx[s][j] = (1.0f - av) * accx[s][j] + av * (g[s][j] * (accy[s][j] - smu) + (wave == 0 ? b[s][j] : 0.f));
    }
    store_partial_row<NV>(part, wave, lane, accx);
    __syncthreads();
    sum_partial_rows<NV>(part, tid, p.ctx + (long)win * D);
}

// ---- backward of the windowed attention (training path; stage 3 of the reference's script trains the
// SigLIP head and the guide encoder too: train.py:717-726, so the gradients w.r.t. the KEY stream frames_embed and the query
// are needed; frames_feature comes from the frozen tower body).  Per window, autograd through projector.py:550-553:
//     s_i = scale q.k_i + bias,  p = softmax(s),  ctx = sum_i p_i v_i
//     dP_i = dctx . v_i,  dS_i = p_i (dP_i - sum_j p_j dP_j),  dq = scale sum_i dS_i k_i,  dk_i = scale dS_i q
// Same mapping as the forward kernel: one 4-wave workgroup per window, a token row over the 64 lanes; the key rows are read
// twice (scores, then dq), the value rows once.  dkey is written by plain stores: the caller guarantees an exact partition
// (every token in exactly one window).
struct LocalBwdParams {
    const uint16_t* key;
    const uint16_t* value;
    const void* query;
    int query_f32;
    long query_stride;
    hicom_axis at, ay, ax;
    float scale, bias;
    const float* dctx;     // [Nw, D]
    float* dq;             // [Nw, D]
    uint16_t* dkey;        // bf16 [N, D] or NULL
    // clip-scale (reference projector.py:527-529, :549; round 6): the key rows are L2-normalised, khat_i = k_i / ||k_i||, and
    // s_i = e^ls (q . khat_i) + lb  (scale = e^ls, bias = lb).  Then  dq = scale sum_i dS_i khat_i,
    // dk_i = scale dS_i (q - khat_i (q . khat_i)) / ||k_i||  (through the normalisation), and -- since ds_i / d ls = s_i - lb --
    // dls[w] = sum_i dS_i (s_i - lb) per window (d lb = sum_i dS_i = 0 exactly: the softmax cancels a shift).
    int l2norm_key;
    float* dls;            // [Nw] or NULL
    // d VALUE stream (round 6: d frames_feature, reference train.py:712-715 `pure_vision_model` trains the tower body): dv_i = p_i dctx_w,
    // bf16 [N, D], plain stores (exact partition) -- or NULL.  value_is_key (frames_embed is None: the keys ARE the value rows,
    // projector.py:532): the key-side gradient of the same row is added in, d x_i = p_i dctx_w + dk_i.
    uint16_t* dvalue;
    int value_is_key;
    // Overlapping windows (an axis the kernel does not divide: reference projector.py:501-522 shifts the trailing windows by k - 1, so a window
    // shares ONE plane of tokens with its predecessor): the per-token outputs are then ACCUMULATED (read-modify-write of the bf16 rows, cleared by
    // the host), one launch per parity class of the window index along every such axis -- windows of one class never share a token, so the
    // sums are ordered by the launches: deterministic, no atomics.  par_mask: bit a set = axis a (t, y, x) is filtered; par_val: the class.
    int accumulate, par_mask, par_val;
};

// the body is window_rows.hpp's local_window_bwd, shared with the ragged training step (ragged_train.hip: ragged_local_attn_bwd_kernel)
template <int NV>
__global__ __launch_bounds__(256) void local_attn_bwd_kernel(LocalBwdParams p) {
    constexpr int D = NV * 384;
    extern __shared__ __attribute__((aligned(16))) float lsm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int win = blockIdx.x;
    const WindowGeom w(p.at, p.ay, p.ax, win);
    if ((((w.t1 & 1) | ((w.h1 & 1) << 1) | ((w.w1 & 1) << 2)) & p.par_mask) != p.par_val) return;      // (another launch's parity class)

    float q[NV][6];
    load_query<NV>(p.query, p.query_f32, p.query_stride, win, lane, q);
    const WindowBwdArgs a{p.key, p.value, p.scale, p.bias, p.dctx + (long)win * D, p.dq + (long)win * D, p.dkey, p.l2norm_key,
                          p.dls ? p.dls + win : nullptr, p.dvalue, p.value_is_key, p.accumulate};
    local_window_bwd<NV>(a, w, q, lsm, tid);
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward of the windowed attention WITH the k / v adaptor blends (training path of the second released recipe
// `local43_adaptkv_global32`; autograd through reference projector.py:533-534 + :550-553).  Round 3 ran this half as fp32 torch
// algebra over window-regrouped [1296, 36, 1152] tensors; here it is two streaming passes over the four token streams
// (x_k, y_k = k_proj(x_k), x_v, y_v), same mapping as the forward kernel (one 4-wave workgroup per window, a token row over a wave):
//     K_n = (1 - a_k) x_n + a_k (gamma_k yhat_n + beta_k),   yhat_n = (y_n - mu_n) rstd_n          (likewise V_n)
//     s_n = scale q.K_n + bias,  p = softmax(s),  dP_n = dctx . V_n,  dS_n = p_n (dP_n - sum_m p_m dP_m)
// Outputs -- everything the rest of the backward needs, none of it of token-stream size except two scalars per token:
//     ds[tok] = scale dS_n,  pw[tok] = p_n                     (d K_n = ds q,  d V_n = pw dctx: rank-1 per token, never materialised)
//     sxk[w] = sum_n ds_n x_k,n    syk[w] = sum_n ds_n yhat_k,n    sxv[w] = sum_n p_n x_v,n    syv[w] = sum_n p_n yhat_v,n      ([Nw, D] f32)
// from which dq = (1 - a_k) sxk + a_k gamma_k syk, d alpha, d gamma, d beta of both adaptors follow as reductions over the windows
// (tiny), and the adaptor-MLP backward starts from (ds, q) / (pw, dctx) through hicom_adapt_dy_fwd.
struct LocalAdaptBwdParams {
    const uint16_t* kx; const _Float16* ky; const uint16_t* kgamma; const uint16_t* kbeta; const void* kalpha;
    const uint16_t* vx; const _Float16* vy; const uint16_t* vgamma; const uint16_t* vbeta; const void* valpha;
    int alpha_f32;
    float eps;
    const void* query;
    int query_f32;
    long query_stride;
    hicom_axis at, ay, ax;
    float scale, bias;
    const float* dctx;      // [Nw, D]
    float* ds;              // [N] token-indexed
    float* pw;              // [N]
    float* sxk; float* syk; float* sxv; float* syv;     // [Nw, D] (syk / syv NULL when that stream has no adaptor)
};

// the body is window_rows.hpp's local_window_adapt_bwd, shared with the ragged training step (ragged_train.hip: ragged_local_attn_adapt_bwd_kernel)
template <int NV>
__global__ __launch_bounds__(256) void local_attn_adapt_bwd_kernel(LocalAdaptBwdParams p) {
    constexpr int D = NV * 384;
    extern __shared__ __attribute__((aligned(16))) float lsm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int win = blockIdx.x;
    const WindowGeom w(p.at, p.ay, p.ax, win);
    const float ak = p.ky ? read_alpha(p.kalpha, p.alpha_f32) : 0.f, av = p.vy ? read_alpha(p.valpha, p.alpha_f32) : 0.f;
    float q[NV][6];
    load_query<NV>(p.query, p.query_f32, p.query_stride, win, lane, q);
    const WindowAdaptBwdArgs a{p.kx, p.ky, p.kgamma, p.kbeta, ak, p.vx, p.vy, p.vgamma, p.vbeta, av, p.eps, p.scale, p.bias, p.dctx + (long)win * D,
                               p.ds, p.pw, p.sxk + (long)win * D, p.syk ? p.syk + (long)win * D : nullptr, p.sxv + (long)win * D,
                               p.syv ? p.syv + (long)win * D : nullptr};
    local_window_adapt_bwd<NV>(a, w, q, lsm, tid);
}

// ---- d y of one adaptor stream: backward of the LayerNorm blend for a rank-1 upstream gradient ---------------------------------------
// The gradient w.r.t. the blended row is coef[tok] * vec[w(tok)] (K stream: ds * q, V stream: pw * dctx), so with n = gamma yhat + beta,
// g = d yhat = alpha coef (vec gamma):  dy = rstd (g - mean(g) - yhat mean(g yhat)).  One wave per token: reads the fp16 y row, writes dy as
// bf16 (the operand dtype of the GEMMs behind it); optionally also r1[tok] = coef2 coef[tok] vec[w] (the (1 - alpha) x-branch of d
// frames_embed, stage 3).  Exact window partition (every token in one window).
struct AdaptDyParams {
    const _Float16* y;      // [N, D]
    const uint16_t* gamma;
    const void* vec;        // f32 | bf16 [Nw | 1, D]
    int vec_f32;
    long vec_stride;
    const float* coef;      // [N]
    const void* alpha; int alpha_f32;
    float eps;
    hicom_axis at, ay, ax;
    uint16_t* dy;           // bf16 [N, D]
    uint16_t* r1;           // bf16 [N, D] or NULL
    long N;
    float* col_parts;       // f32 [gridDim.x][D] or NULL: this workgroup's column sums of dy (as stored: bf16-rounded) -- the bias gradient
};

template <int NV>
__global__ __launch_bounds__(256) void adapt_dy_kernel(AdaptDyParams p) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float csum[NV][6];
    row_zero<NV>(csum);
    for (long tok = (long)blockIdx.x * 4 + wave; tok < p.N; tok += (long)gridDim.x * 4) {      // (the token's body: window_rows.hpp, adapt_dy_token)
        const long win = WindowGeom::window_of(p.at, p.ay, p.ax, tok);
        const void* vec = p.vec_f32 ? (const void*)(reinterpret_cast<const float*>(p.vec) + win * p.vec_stride)
                                    : (const void*)(reinterpret_cast<const uint16_t*>(p.vec) + win * p.vec_stride);
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

}  // namespace hicom

using namespace hicom;

// ---- host side -----------------------------------------------------------------------------------------------------------------
// D and the three axes of a window call; leaves the tokens per window and the window count.  exact: every token lies in exactly one
// window (the per-token outputs are written once); otherwise trailing windows may overlap, but none may run off its axis.
static int check_window_call(const char* who, int D, hicom_axis at, hicom_axis ay, hicom_axis ax, bool exact, long& win, long& nwin) {
    HICOM_REQUIRE(D == 1152 || D == 768, HICOM_EUNSUP, "%s: D=%d (only 1152 / 768)", who, D);
    for (const hicom_axis* a : {&at, &ay, &ax}) {
        HICOM_REQUIRE(a->n > 0 && a->k > 0 && a->nwin > 0 && a->nfull >= 0 && a->nfull <= a->nwin && a->k <= a->n,
                      HICOM_EINVAL, "%s: bad axis n=%d k=%d nwin=%d nfull=%d", who, a->n, a->k, a->nwin, a->nfull);
        if (exact) {
            HICOM_REQUIRE((long)a->nwin * a->k == a->n, HICOM_EUNSUP, "%s: needs an exact window partition (n=%d k=%d)", who, a->n, a->k);
        } else {
            const int last = axis_start(*a, a->nwin - 1);
            HICOM_REQUIRE(last >= 0 && last + a->k <= a->n, HICOM_EINVAL, "%s: window runs off the axis", who);
        }
    }
    win = (long)at.k * ay.k * ax.k;
    nwin = (long)at.nwin * ay.nwin * ax.nwin;
    return HICOM_OK;
}

// LDS of a window kernel: n_arrays per-token float arrays of the window, then the [4][D] slab of partial rows
static size_t window_smem(long win, int D, int n_arrays) { return n_arrays * (((size_t)win + 3) & ~(size_t)3) * 4 + 4 * (size_t)D * 4; }

// the forward's and the plain backward's limits on a window and on the grid.  smem: the caller's window_smem -- the kernels take it as
// dynamic LDS and nothing here raises the 64-KB default, so it stays under the bound merge.hip uses for its dynamic LDS.
static int check_window_limits(const char* who, long win, long nwin, size_t smem) {
    HICOM_REQUIRE(win <= 4096, HICOM_EUNSUP, "%s: window of %ld tokens is too large", who, win);
    HICOM_REQUIRE(smem <= 60000, HICOM_EUNSUP, "%s: window of %ld tokens needs %zu bytes of LDS (at most 60000)", who, win, smem);
    HICOM_REQUIRE(nwin < (1L << 31), HICOM_EINVAL, "%s: too many windows", who);
    return HICOM_OK;
}

// kernel<NV> for D = NV * 384 (D was checked: 1152 or 768)
#define LAUNCH_BY_WIDTH(kernel, D, grid, smem, stream, ...)                                                \
    do {                                                                                                   \
        if ((D) == 1152) hipLaunchKernelGGL(kernel<3>, grid, dim3(256), smem, stream, __VA_ARGS__);        \
        else hipLaunchKernelGGL(kernel<2>, grid, dim3(256), smem, stream, __VA_ARGS__);                    \
    } while (0)

extern "C" int hicom_local_attn_fwd(const void* key, int32_t key_dt, const void* value, int32_t value_dt, int32_t D,
                                    hicom_axis at, hicom_axis ay, hicom_axis ax,
                                    const void* query, int32_t query_dt, int64_t query_stride,
                                    float scale, float bias, int32_t l2norm,
                                    float* ctx, void* ctx_f16, void* stream) {
    HICOM_REQUIRE(key && value && query && (ctx || ctx_f16), HICOM_EINVAL, "local_attn: NULL pointer");
    HICOM_REQUIRE(query_dt == HICOM_DT_BF16 || query_dt == HICOM_DT_F32, HICOM_EINVAL, "local_attn: query dtype");
    HICOM_REQUIRE(key_dt >= 0 && key_dt <= 2 && value_dt >= 0 && value_dt <= 2, HICOM_EINVAL, "local_attn: stream dtype");
    long win, nwin;
    if (int rc = check_window_call("local_attn", D, at, ay, ax, false, win, nwin)) return rc;
    if (int rc = check_window_limits("local_attn", win, nwin, window_smem(win, D, 1))) return rc;
    LocalParams p{key, value, key_dt, value_dt, query, query_dt == HICOM_DT_F32,
                  (long)query_stride, at, ay, ax, scale, bias, l2norm, ctx, (_Float16*)ctx_f16};
    LAUNCH_BY_WIDTH(local_attn_kernel, D, dim3((unsigned)nwin), window_smem(win, D, 1), (hipStream_t)stream, p);
    return hicom_host::check_launch("local_attn");
}

extern "C" int hicom_local_attn_adapt_fwd(const void* key_x, const void* key_y, const void* k_gamma, const void* k_beta, const void* k_alpha,
                                          const void* value_x, const void* value_y, const void* v_gamma, const void* v_beta, const void* v_alpha,
                                          int32_t alpha_dt, float eps, int32_t D, hicom_axis at, hicom_axis ay, hicom_axis ax,
                                          const void* query, int32_t query_dt, int64_t query_stride, float scale, float bias,
                                          float* ctx, void* stream) {
    HICOM_REQUIRE(key_x && value_x && query && ctx && (key_y || value_y), HICOM_EINVAL, "local_attn_adapt: NULL pointer / no adapted stream");
    HICOM_REQUIRE(!key_y || (k_gamma && k_beta && k_alpha), HICOM_EINVAL, "local_attn_adapt: key adaptor parameters");
    HICOM_REQUIRE(!value_y || (v_gamma && v_beta && v_alpha), HICOM_EINVAL, "local_attn_adapt: value adaptor parameters");
    HICOM_REQUIRE(query_dt == HICOM_DT_BF16 || query_dt == HICOM_DT_F32, HICOM_EINVAL, "local_attn_adapt: query dtype");
    HICOM_REQUIRE(alpha_dt == HICOM_DT_BF16 || alpha_dt == HICOM_DT_F32, HICOM_EINVAL, "local_attn_adapt: alpha dtype");
    long win, nwin;
    if (int rc = check_window_call("local_attn_adapt", D, at, ay, ax, false, win, nwin)) return rc;
    if (int rc = check_window_limits("local_attn_adapt", win, nwin, window_smem(win, D, 1))) return rc;
    LocalAdaptParams p{(const uint16_t*)key_x, (const _Float16*)key_y, (const uint16_t*)k_gamma, (const uint16_t*)k_beta, k_alpha,
                       (const uint16_t*)value_x, (const _Float16*)value_y, (const uint16_t*)v_gamma, (const uint16_t*)v_beta, v_alpha,
                       alpha_dt == HICOM_DT_F32, eps, query, query_dt == HICOM_DT_F32, (long)query_stride, at, ay, ax, scale, bias, ctx};
    LAUNCH_BY_WIDTH(local_attn_adapt_kernel, D, dim3((unsigned)nwin), window_smem(win, D, 1), (hipStream_t)stream, p);
    return hicom_host::check_launch("local_attn_adapt");
}

extern "C" int hicom_local_attn_bwd(const void* key, const void* value, int32_t D,
                                    hicom_axis at, hicom_axis ay, hicom_axis ax,
                                    const void* query, int32_t query_dt, int64_t query_stride,
                                    float scale, float bias, const float* dctx, float* dq, void* dkey,
                                    int32_t l2norm_key, float* dls, void* dvalue, int32_t value_is_key, void* stream) {
    HICOM_REQUIRE(key && value && query && dctx && dq, HICOM_EINVAL, "local_attn_bwd: NULL pointer");
    HICOM_REQUIRE(query_dt == HICOM_DT_BF16 || query_dt == HICOM_DT_F32, HICOM_EINVAL, "local_attn_bwd: query dtype");
    long win, nwin;
    if (int rc = check_window_call("local_attn_bwd", D, at, ay, ax, false, win, nwin)) return rc;
    if (int rc = check_window_limits("local_attn_bwd", win, nwin, window_smem(win, D, 5))) return rc;
    LocalBwdParams p{(const uint16_t*)key, (const uint16_t*)value, query, query_dt == HICOM_DT_F32, (long)query_stride, at, ay, ax,
                     scale, bias, dctx, dq, (uint16_t*)dkey, l2norm_key ? 1 : 0, dls, (uint16_t*)dvalue, value_is_key ? 1 : 0, 0, 0, 0};
    HICOM_REQUIRE(!(value_is_key && dkey), HICOM_EINVAL, "local_attn_bwd: value_is_key writes the summed gradient to dvalue (dkey must be NULL)");
    hipStream_t s = (hipStream_t)stream;
    // per-token outputs over OVERLAPPING windows: cleared, then one accumulating launch per parity class of the axes that overlap
    int mask = 0;
    if (dkey || dvalue) {
        const hicom_axis* axs[3] = {&at, &ay, &ax};
        for (int a = 0; a < 3; ++a)
            if ((long)axs[a]->nwin * axs[a]->k != axs[a]->n) mask |= 1 << a;
    }
    if (mask) {
        const size_t bytes = (size_t)at.n * ay.n * ax.n * D * 2;
        if (dkey) HICOM_REQUIRE(hipMemsetAsync(dkey, 0, bytes, s) == hipSuccess, HICOM_ELAUNCH, "local_attn_bwd: memset");
        if (dvalue) HICOM_REQUIRE(hipMemsetAsync(dvalue, 0, bytes, s) == hipSuccess, HICOM_ELAUNCH, "local_attn_bwd: memset");
        p.accumulate = 1;
        p.par_mask = mask;
    }
    for (int val = 0; val < 8; ++val) {
        if (val & ~mask) continue;
        p.par_val = val;
        LAUNCH_BY_WIDTH(local_attn_bwd_kernel, D, dim3((unsigned)nwin), window_smem(win, D, 5), s, p);
    }
    return hicom_host::check_launch("local_attn_bwd");
}

extern "C" int hicom_local_attn_adapt_bwd(const void* key_x, const void* key_y, const void* k_gamma, const void* k_beta, const void* k_alpha,
                                          const void* value_x, const void* value_y, const void* v_gamma, const void* v_beta, const void* v_alpha,
                                          int32_t alpha_dt, float eps, int32_t D, hicom_axis at, hicom_axis ay, hicom_axis ax,
                                          const void* query, int32_t query_dt, int64_t query_stride, float scale, float bias,
                                          const float* dctx, float* ds, float* pw, float* sxk, float* syk, float* sxv, float* syv, void* stream) {
    HICOM_REQUIRE(key_x && value_x && query && dctx && ds && pw && sxk && sxv && (key_y || value_y), HICOM_EINVAL, "local_attn_adapt_bwd: NULL pointer");
    HICOM_REQUIRE((!key_y || (k_gamma && k_beta && k_alpha && syk)) && (!value_y || (v_gamma && v_beta && v_alpha && syv)), HICOM_EINVAL,
                  "local_attn_adapt_bwd: adaptor parameters / outputs");
    HICOM_REQUIRE((query_dt == HICOM_DT_BF16 || query_dt == HICOM_DT_F32) && (alpha_dt == HICOM_DT_BF16 || alpha_dt == HICOM_DT_F32), HICOM_EINVAL,
                  "local_attn_adapt_bwd: query / alpha dtype");
    long win, nwin;
    if (int rc = check_window_call("local_attn_adapt_bwd", D, at, ay, ax, true, win, nwin)) return rc;      // (ds / pw are written once per token)
    HICOM_REQUIRE(win <= 1024 && nwin < (1L << 31), HICOM_EUNSUP, "local_attn_adapt_bwd: window of %ld tokens is too large", win);
    LocalAdaptBwdParams p{(const uint16_t*)key_x, (const _Float16*)key_y, (const uint16_t*)k_gamma, (const uint16_t*)k_beta, k_alpha,
                          (const uint16_t*)value_x, (const _Float16*)value_y, (const uint16_t*)v_gamma, (const uint16_t*)v_beta, v_alpha,
                          alpha_dt == HICOM_DT_F32, eps, query, query_dt == HICOM_DT_F32, (long)query_stride, at, ay, ax, scale, bias,
                          dctx, ds, pw, sxk, syk, sxv, syv};
    LAUNCH_BY_WIDTH(local_attn_adapt_bwd_kernel, D, dim3((unsigned)nwin), window_smem(win, D, 6), (hipStream_t)stream, p);
    return hicom_host::check_launch("local_attn_adapt_bwd");
}

extern "C" int hicom_adapt_dy_fwd(const void* y, const void* gamma, const void* vec, int32_t vec_dt, int64_t vec_stride, const float* coef,
                                  const void* alpha, int32_t alpha_dt, float eps, int32_t D, hicom_axis at, hicom_axis ay, hicom_axis ax,
                                  void* dy, void* r1, float* col_parts, int32_t nparts, void* stream) {
    HICOM_REQUIRE(y && gamma && vec && coef && alpha && dy && (!col_parts || nparts > 0), HICOM_EINVAL, "adapt_dy: NULL pointer");
    HICOM_REQUIRE((vec_dt == HICOM_DT_BF16 || vec_dt == HICOM_DT_F32) && (alpha_dt == HICOM_DT_BF16 || alpha_dt == HICOM_DT_F32), HICOM_EINVAL, "adapt_dy: dtypes");
    long win, nwin;
    if (int rc = check_window_call("adapt_dy", D, at, ay, ax, true, win, nwin)) return rc;
    const long N = (long)at.n * ay.n * ax.n;
    AdaptDyParams p{(const _Float16*)y, (const uint16_t*)gamma, vec, vec_dt == HICOM_DT_F32, (long)vec_stride, coef, alpha, alpha_dt == HICOM_DT_F32, eps,
                    at, ay, ax, (uint16_t*)dy, (uint16_t*)r1, N, col_parts};
    // with column partials: `nparts` workgroups walk the tokens (each leaves one partial row); without: one token per wave
    const unsigned grid = col_parts ? (unsigned)nparts : (unsigned)((N + 3) / 4);
    LAUNCH_BY_WIDTH(adapt_dy_kernel, D, dim3(grid), 0, (hipStream_t)stream, p);
    return hicom_host::check_launch("adapt_dy");
}
