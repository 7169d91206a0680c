// Row and window scaffold shared by the windowed-attention kernels (local_attn.hip) and the row-wise kernels (rowwise_ops.hip).
//
// A token row of D = NV * 384 channels is spread over the 64 lanes of a wave as NV segments of 64 x 6 channels: lane l holds
// channels 384 s + 6 l .. + 5 of segment s in a float [NV][6] (12 B of bf16 / fp16 per lane and segment: global_load_dwordx3,
// fully coalesced 768-B runs).  Everything here keeps the element order (s outer, j inner) and one accumulator chain per sum, so a
// kernel written with these helpers rounds exactly as the loops they replace.
#pragma once
#include "common.hpp"

namespace hicom {

struct __attribute__((packed, aligned(4))) Seg12 { uint32_t a, b, c; };

// ---- row loads -----------------------------------------------------------------------------------------------------------------
template <int NV>
__device__ __forceinline__ void load_row(const uint16_t* row, int lane, float (&v)[NV][6]) {
#pragma unroll
    for (int s = 0; s < NV; ++s) {
        const Seg12 g = *reinterpret_cast<const Seg12*>(row + 384 * s + 6 * lane);
        v[s][0] = bf16lo_to_f32(g.a); v[s][1] = bf16hi_to_f32(g.a);
        v[s][2] = bf16lo_to_f32(g.b); v[s][3] = bf16hi_to_f32(g.b);
        v[s][4] = bf16lo_to_f32(g.c); v[s][5] = bf16hi_to_f32(g.c);
    }
}

template <int NV>
__device__ __forceinline__ void load_row_f32(const float* row, int lane, float (&v)[NV][6]) {
#pragma unroll
    for (int s = 0; s < NV; ++s) {
        const Seg12 a = *reinterpret_cast<const Seg12*>(row + 384 * s + 6 * lane);
        const Seg12 b = *reinterpret_cast<const Seg12*>(row + 384 * s + 6 * lane + 3);
        v[s][0] = __uint_as_float(a.a); v[s][1] = __uint_as_float(a.b); v[s][2] = __uint_as_float(a.c);
        v[s][3] = __uint_as_float(b.a); v[s][4] = __uint_as_float(b.b); v[s][5] = __uint_as_float(b.c);
    }
}

template <int NV>
__device__ __forceinline__ void load_row_f16(const _Float16* row, int lane, float (&v)[NV][6]) {
    typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int s = 0; s < NV; ++s) {
        const Seg12 g = *reinterpret_cast<const Seg12*>(row + 384 * s + 6 * lane);
        const half2_t a = __builtin_bit_cast(half2_t, g.a), b = __builtin_bit_cast(half2_t, g.b), c = __builtin_bit_cast(half2_t, g.c);
        v[s][0] = (float)a[0]; v[s][1] = (float)a[1]; v[s][2] = (float)b[0]; v[s][3] = (float)b[1]; v[s][4] = (float)c[0]; v[s][5] = (float)c[1];
    }
}

// stream dtype code: 0 = bf16 (raw tokens), 1 = fp32, 2 = fp16 (alpha-blended adaptor outputs)
template <int NV>
__device__ __forceinline__ void load_stream_row(const void* base, int dt, long token, int lane, float (&v)[NV][6]) {
    constexpr int D = NV * 384;
    if (dt == 1) load_row_f32<NV>(reinterpret_cast<const float*>(base) + token * D, lane, v);
    else if (dt == 2) load_row_f16<NV>(reinterpret_cast<const _Float16*>(base) + token * D, lane, v);
    else load_row<NV>(reinterpret_cast<const uint16_t*>(base) + token * D, lane, v);
}

// query fragment of this lane (fp32): row `win` of a bf16 or f32 [Nw | 1, D] matrix (stride 0: one shared query)
template <int NV>
__device__ __forceinline__ void load_query(const void* query, int query_f32, long query_stride, int win, int lane, float (&q)[NV][6]) {
    if (query_f32) {
        const float* qp = reinterpret_cast<const float*>(query) + (long)win * query_stride;
#pragma unroll
        for (int s = 0; s < NV; ++s)
#pragma unroll
            for (int j = 0; j < 6; ++j) q[s][j] = qp[384 * s + 6 * lane + j];
    } else {
        load_row<NV>(reinterpret_cast<const uint16_t*>(query) + (long)win * query_stride, lane, q);
    }
}

__device__ __forceinline__ float read_alpha(const void* a, int is_f32) {
    return is_f32 ? *reinterpret_cast<const float*>(a) : bf16_to_f32(*reinterpret_cast<const uint16_t*>(a));
}

// ---- bf16 row segments: six floats of a lane <-> the 12 bytes it stores --------------------------------------------------------------
__device__ __forceinline__ void seg12_accum(float (&e)[6], const Seg12 w) {
    e[0] += bf16lo_to_f32(w.a); e[1] += bf16hi_to_f32(w.a); e[2] += bf16lo_to_f32(w.b); e[3] += bf16hi_to_f32(w.b);
    e[4] += bf16lo_to_f32(w.c); e[5] += bf16hi_to_f32(w.c);
}
__device__ __forceinline__ void seg12_add(float (&e)[6], const uint16_t* o) { seg12_accum(e, *reinterpret_cast<const Seg12*>(o)); }

// rounds and stores one segment; returns the words as stored (a caller that sums what it wrote sums the ROUNDED values)
__device__ __forceinline__ Seg12 store_seg12(uint16_t* o, const float (&e)[6]) {
    Seg12 w;
    w.a = f32_to_bf16(e[0]) | ((uint32_t)f32_to_bf16(e[1]) << 16);
    w.b = f32_to_bf16(e[2]) | ((uint32_t)f32_to_bf16(e[3]) << 16);
    w.c = f32_to_bf16(e[4]) | ((uint32_t)f32_to_bf16(e[5]) << 16);
    *reinterpret_cast<Seg12*>(o) = w;
    return w;
}

// this lane's part of a bf16 row from elem(s, j); accumulate: added to what the row holds (read-modify-write)
template <int NV, class F>
__device__ __forceinline__ void store_row_bf16(uint16_t* row, int lane, bool accumulate, F&& elem) {
#pragma unroll
    for (int s = 0; s < NV; ++s) {
        float e[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) e[j] = elem(s, j);
        if (accumulate) seg12_add(e, row + 384 * s + 6 * lane);
        store_seg12(row + 384 * s + 6 * lane, e);
    }
}

// ---- row primitives over a lane's float [NV][6] (per-lane partials: the caller reduces over the wave) -----------------------------------
template <int NV>
__device__ __forceinline__ void row_zero(float (&a)[NV][6]) {
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int j = 0; j < 6; ++j) a[s][j] = 0.f;
}

template <int NV>
__device__ __forceinline__ float row_dot(const float (&a)[NV][6], const float (&b)[NV][6]) {
    float d = 0.f;
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int j = 0; j < 6; ++j) d = fmaf(a[s][j], b[s][j], d);
    return d;
}

template <int NV>
__device__ __forceinline__ float row_sum(const float (&a)[NV][6]) {
    float t = 0.f;
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int j = 0; j < 6; ++j) t += a[s][j];
    return t;
}

// acc = fmaf(w, x, acc)
template <int NV>
__device__ __forceinline__ void row_axpy(float w, const float (&x)[NV][6], float (&acc)[NV][6]) {
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int j = 0; j < 6; ++j) acc[s][j] = fmaf(w, x[s][j], acc[s][j]);
}

template <int NV>
__device__ __forceinline__ void row_mul(const float (&a)[NV][6], const float (&b)[NV][6], float (&out)[NV][6]) {
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int j = 0; j < 6; ++j) out[s][j] = a[s][j] * b[s][j];
}

// LayerNorm statistics of a row in registers (two passes, fp32); every lane gets both
template <int NV>
__device__ __forceinline__ void ln_stats(const float (&y)[NV][6], float eps, float& mu, float& rstd) {
    constexpr int D = NV * 384;
    mu = wave_sum_fast(row_sum<NV>(y)) * (1.0f / D);
    float s2 = 0.f;
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int j = 0; j < 6; ++j) { const float d = y[s][j] - mu; s2 = fmaf(d, d, s2); }
    rstd = 1.0f / sqrtf(wave_sum_fast(s2) * (1.0f / D) + eps);
}

// what a vector v needs to meet a LayerNorm-affine row without forming it:  vg = v gamma,  cg = sum(v gamma),  cb = v . beta
template <int NV>
__device__ __forceinline__ void affine_prep(const float (&v)[NV][6], const uint16_t* gamma, const uint16_t* beta, int lane, float (&vg)[NV][6],
                                            float& cg, float& cb) {
    float g[NV][6], b[NV][6];
    load_row<NV>(gamma, lane, g);
    load_row<NV>(beta, lane, b);
    row_mul<NV>(v, g, vg);
    cg = wave_sum_fast(row_sum<NV>(vg));
    cb = wave_sum_fast(row_dot<NV>(v, b));
}

// v . ((1 - a) x + a (gamma yhat + beta)) for one token of an adaptor-blended stream, yhat = LN(y), from the x row, the y row and
// affine_prep(v):  (1 - a) v.x + a (rstd (vg.y - mu cg) + cb).  Leaves the LayerNorm statistics of y.  has_y false: the plain v.x.
template <int NV>
__device__ __forceinline__ float blend_dot(const float (&x)[NV][6], const float (&y)[NV][6], bool has_y, const float (&v)[NV][6],
                                          const float (&vg)[NV][6], float cg, float cb, float a, float eps, float& mu, float& rstd) {
    const float dx = wave_sum_fast(row_dot<NV>(v, x));
    if (!has_y) return dx;
    const float dy = wave_sum_fast(row_dot<NV>(vg, y));
    ln_stats<NV>(y, eps, mu, rstd);
    return (1.0f - a) * dx + a * (rstd * (dy - mu * cg) + cb);
}

// ---- one window of the [T, H, W] token grid --------------------------------------------------------------------------------------
// Window `win` (t-major over at.nwin x ay.nwin x ax.nwin) starts at (t0, y0, x0) and holds WIN = kt * ks2 tokens, t-major too.
struct WindowGeom {
    int t1, h1, w1, t0, y0, x0, kx, ks2, WIN, H, W;
    __device__ __forceinline__ WindowGeom(const hicom_axis& at, const hicom_axis& ay, const hicom_axis& ax, int win) {
        w1 = win % ax.nwin;
        h1 = (win / ax.nwin) % ay.nwin;
        t1 = win / (ax.nwin * ay.nwin);
        t0 = axis_start(at, t1); y0 = axis_start(ay, h1); x0 = axis_start(ax, w1);
        kx = ax.k;
        ks2 = ay.k * ax.k;
        WIN = at.k * ks2;
        H = ay.n; W = ax.n;
    }
    // i-th token of the window -> token index
    __device__ __forceinline__ long token_of(int i) const {
        const int t2 = i / ks2, r = i - t2 * ks2;
        const int h2 = r / kx, w2 = r - h2 * kx;
        return ((long)(t0 + t2) * H + (y0 + h2)) * W + (x0 + w2);
    }
    // the inverse, for an EXACT partition (every token in one window): token index -> window
    __device__ __forceinline__ static long window_of(const hicom_axis& at, const hicom_axis& ay, const hicom_axis& ax, long tok) {
        const int H = ay.n, W = ax.n;
        const int t = (int)(tok / ((long)H * W)), rem = (int)(tok - (long)t * H * W), yy = rem / W, xx = rem - yy * W;
        return ((long)(t / at.k) * ay.nwin + yy / ay.k) * ax.nwin + xx / ax.k;
    }
};

// softmax statistics over the window's scores in LDS (every wave redundantly; WIN is tiny).  With dp (the backward):
// also delta = sum_i p_i dp_i.
__device__ __forceinline__ void softmax_stats(const float* sc, int WIN, int lane, float& mx, float& inv_sum, const float* dp = nullptr,
                                              float* delta = nullptr) {
    mx = -3.0e38f;
    for (int i = lane; i < WIN; i += 64) mx = fmaxf(mx, sc[i]);
    mx = wave_max_fast(mx);
    float sum = 0.f, pd = 0.f;
    for (int i = lane; i < WIN; i += 64) {
        const float e = expf(sc[i] - mx);
        sum += e;
        if (dp) pd = fmaf(e, dp[i], pd);
    }
    inv_sum = 1.0f / wave_sum_fast(sum);
    if (dp) *delta = wave_sum_fast(pd) * inv_sum;
}

// ---- the four waves' partial rows through a [4][D] slab of LDS -------------------------------------------------------------------------
template <int NV>
__device__ __forceinline__ void store_partial_row(float* part, int wave, int lane, const float (&a)[NV][6]) {
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int j = 0; j < 6; ++j) part[wave * (NV * 384) + 384 * s + 6 * lane + j] = a[s][j];
}

// after a barrier: emit(c, sum of the four rows at column c), the columns strided over the workgroup
template <int NV, class F>
__device__ __forceinline__ void sum_partial_rows(const float* part, int tid, F&& emit) {
    constexpr int D = NV * 384;
    for (int c = tid; c < D; c += 256) emit(c, (part[c] + part[D + c]) + (part[2 * D + c] + part[3 * D + c]));
}
template <int NV>
__device__ __forceinline__ void sum_partial_rows(const float* part, int tid, float* out) {
    sum_partial_rows<NV>(part, tid, [&](int c, float v) { out[c] = v; });
}

// ---- backward of one window of the plain windowed attention: the one body of local_attn_bwd_kernel (local_attn.hip: the window comes from
// blockIdx and the call's one grid) and ragged_local_attn_bwd_kernel (ragged_train.hip: the window's item comes from a device table, the grid is
// the item's own).  Per window, autograd through projector.py:550-553 (local_attn.hip has the algebra and the clip-scale terms):
//     s_i = scale q.k_i + bias,  p = softmax(s),  dP_i = dctx . v_i,  dS_i = p_i (dP_i - sum_j p_j dP_j),
//     dq = scale sum_i dS_i k_i,  dk_i = scale dS_i q,  dv_i = p_i dctx (+ dk_i with value_is_key)
// key / value / dkey / dvalue point at the first token of the grid `w` indexes; dctx / dq at the window's own row; dls at the window's own
// element or NULL.  One 4-wave workgroup, lsm: 5 per-token arrays of the window + the [4][D] slab (window_smem(WIN, D, 5)).
struct WindowBwdArgs {
    const uint16_t* key;
    const uint16_t* value;
    float scale, bias;
    const float* dctx;     // [D]
    float* dq;             // [D]
    uint16_t* dkey;        // bf16 [N, D] or NULL
    int l2norm_key;
    float* dls;            // one float or NULL
    uint16_t* dvalue;      // bf16 [N, D] or NULL
    int value_is_key;
    int accumulate;
};

template <int NV>
__device__ __forceinline__ void local_window_bwd(const WindowBwdArgs& p, const WindowGeom& w, const float (&q)[NV][6], float* lsm, int tid) {
    constexpr int D = NV * 384;
    const int lane = tid & 63, wave = tid >> 6;
    const int WIN = w.WIN, WP = (WIN + 3) & ~3;
    float* sc = lsm;                              // [WIN] scores, then dS
    float* dp = lsm + WP;                         // [WIN] dP
    float* rin = lsm + 2 * WP;                    // [WIN] 1 / ||k_i|| (1 without l2norm_key)
    float* sraw = lsm + 3 * WP;                   // [WIN] q . khat_i
    float* pwt = lsm + 4 * WP;                    // [WIN] softmax weights p_i
    float* part = lsm + 5 * WP;                   // [4][D] partial dq

    float g[NV][6];
    load_row_f32<NV>(p.dctx, lane, g);

    // ---- phase 1: scores and dP ------------------------------------------------------------------
    for (int i0 = wave; i0 < WIN; i0 += 8) {      // 2 tokens (key + value rows) in flight per wave
        float k[2][NV][6], v[2][NV][6];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = i0 + 4 * u;
            if (i < WIN) {
                const long tok = w.token_of(i);
                load_row<NV>(p.key + tok * D, lane, k[u]);
                load_row<NV>(p.value + tok * D, lane, v[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = i0 + 4 * u;
            if (i < WIN) {
                float dot = wave_sum_fast(row_dot<NV>(q, k[u]));
                const float dd = wave_sum_fast(row_dot<NV>(g, v[u]));
                float ri = 1.0f;
                if (p.l2norm_key) {
                    ri = 1.0f / sqrtf(wave_sum_fast(row_dot<NV>(k[u], k[u])));
                    dot *= ri;
                }
                if (lane == 0) { sc[i] = dot * p.scale + p.bias; dp[i] = dd; rin[i] = ri; sraw[i] = dot; }
            }
        }
    }
    __syncthreads();
    float mx, inv_sum, delta;
    softmax_stats(sc, WIN, lane, mx, inv_sum, dp, &delta);
    __syncthreads();                               // every wave has read sc / dp as scores
    if (wave == 0) {
        float dl = 0.f;
        for (int i = lane; i < WIN; i += 64) {
            const float s_i = sc[i], pi_ = expf(s_i - mx) * inv_sum, dS = pi_ * (dp[i] - delta);
            dl = fmaf(dS, s_i - p.bias, dl);
            sc[i] = dS;
            pwt[i] = pi_;
        }
        if (p.dls) {
            dl = wave_sum_fast(dl);
            if (lane == 0) *p.dls = dl;
        }
    }
    __syncthreads();

    // ---- phase 2: dq = scale sum_i dS_i k_i ;  dkey_i = scale dS_i q -----------------------------------------
    float acc[NV][6];
    row_zero<NV>(acc);
    for (int i0 = wave; i0 < WIN; i0 += 12) {
        float k[3][NV][6];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int i = i0 + 4 * u;
            if (i < WIN) load_row<NV>(p.key + w.token_of(i) * D, lane, k[u]);
        }
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int i = i0 + 4 * u;
            if (i < WIN) {
                // (plain: dsk = ds, kc = 0.  clip-scale: d k_i = ds / ||k|| (q - khat (q . khat)) = dsk q - kc k with dsk = ds / ||k||,
                // kc = dsk (q . khat) / ||k||; the dq sum runs over khat = k / ||k||)
                const float ds = sc[i] * p.scale, dsk = ds * rin[i], kc = p.l2norm_key ? dsk * sraw[i] * rin[i] : 0.f;
                row_axpy<NV>(dsk, k[u], acc);
                auto dk = [&](int s, int j) { return fmaf(dsk, q[s][j], -kc * k[u][s][j]); };
                if (p.dkey) store_row_bf16<NV>(p.dkey + w.token_of(i) * D, lane, p.accumulate, dk);
                if (p.dvalue) {
                    const float pi_ = pwt[i];
                    store_row_bf16<NV>(p.dvalue + w.token_of(i) * D, lane, p.accumulate, [&](int s, int j) {
                        float e = pi_ * g[s][j];
                        if (p.value_is_key) e += dk(s, j);
                        return e;
                    });
                }
            }
        }
    }
    store_partial_row<NV>(part, wave, lane, acc);
    __syncthreads();
    sum_partial_rows<NV>(part, tid, p.dq);
}

// ---- backward of one window of the windowed attention WITH the k / v adaptor blends: the one body of local_attn_adapt_bwd_kernel
// (local_attn.hip has the algebra: the window comes from blockIdx and the call's one grid) and ragged_local_attn_adapt_bwd_kernel
// (ragged_train.hip: the window's item comes from a device table, the grid is the item's own).  kx / ky / vx / vy / ds / pw point at the first
// token of the grid `w` indexes; dctx and the four sums at the window's own row.  A sum whose pointer is NULL is not written (syk / syv
// of a stream without adaptor: its y pointer is NULL too).  One 4-wave workgroup, lsm: 6 per-token arrays of the window + the [4][D] slab.
struct WindowAdaptBwdArgs {
    const uint16_t* kx; const _Float16* ky; const uint16_t* kgamma; const uint16_t* kbeta; float ak;
    const uint16_t* vx; const _Float16* vy; const uint16_t* vgamma; const uint16_t* vbeta; float av;
    float eps, scale, bias;
    const float* dctx;      // [D]
    float* ds;              // [N] token-indexed
    float* pw;              // [N]
    float* sxk; float* syk; float* sxv; float* syv;     // [D] or NULL
};

template <int NV>
__device__ __forceinline__ void local_window_adapt_bwd(const WindowAdaptBwdArgs& p, const WindowGeom& w, const float (&q)[NV][6], float* lsm, int tid) {
    constexpr int D = NV * 384;
    const int lane = tid & 63, wave = tid >> 6;
    const int WIN = w.WIN, WP = (WIN + 3) & ~3;
    float* sc = lsm;                               // [WIN] scores, then ds
    float* dp = lsm + WP;                          // [WIN] dP, then p
    float* stk = lsm + 2 * WP;                     // [2][WIN] mu, rstd of y_k
    float* stv = lsm + 4 * WP;                     // [2][WIN] mu, rstd of y_v
    float* part = lsm + 6 * WP;                    // [4][D]
    const float ak = p.ak, av = p.av;

    float g[NV][6];
    load_row_f32<NV>(p.dctx, lane, g);
    // q gamma_k, sum(q gamma_k), q . beta_k  and  g gamma_v, sum(g gamma_v), g . beta_v
    float qg[NV][6], gg[NV][6];
    float cgk = 0.f, cbk = 0.f, cgv = 0.f, cbv = 0.f;
    if (p.ky) affine_prep<NV>(q, p.kgamma, p.kbeta, lane, qg, cgk, cbk);
    if (p.vy) affine_prep<NV>(g, p.vgamma, p.vbeta, lane, gg, cgv, cbv);

    // ---- phase 1: scores, dP, LayerNorm statistics (one token per wave in flight: four rows) -----------------------------------
    for (int i = wave; i < WIN; i += 4) {
        const long tok = w.token_of(i);
        float kx[NV][6], ky[NV][6], vx[NV][6], vy[NV][6];
        load_row<NV>(p.kx + tok * D, lane, kx);
        if (p.ky) load_row_f16<NV>(p.ky + tok * D, lane, ky);
        load_row<NV>(p.vx + tok * D, lane, vx);
        if (p.vy) load_row_f16<NV>(p.vy + tok * D, lane, vy);
        float muk = 0.f, rsk = 0.f, muv = 0.f, rsv = 0.f;
        const float logit = blend_dot<NV>(kx, ky, p.ky != nullptr, q, qg, cgk, cbk, ak, p.eps, muk, rsk);
        const float dpi = blend_dot<NV>(vx, vy, p.vy != nullptr, g, gg, cgv, cbv, av, p.eps, muv, rsv);
        if (lane == 0) {
            sc[i] = logit * p.scale + p.bias;
            dp[i] = dpi;
            stk[i] = muk; stk[WP + i] = rsk;
            stv[i] = muv; stv[WP + i] = rsv;
        }
    }
    __syncthreads();
    float mx, inv_sum, delta;
    softmax_stats(sc, WIN, lane, mx, inv_sum, dp, &delta);
    __syncthreads();                               // every wave has read sc / dp as scores / dP
    if (wave == 0)
        for (int i = lane; i < WIN; i += 64) {
            const float pi = expf(sc[i] - mx) * inv_sum;
            const float dsi = pi * (dp[i] - delta) * p.scale;
            sc[i] = dsi;
            dp[i] = pi;
            const long tok = w.token_of(i);
            p.ds[tok] = dsi;
            p.pw[tok] = pi;
        }
    __syncthreads();
    // ---- phase 2: the four weighted sums over the window ------------------------------------------------------------------------
    float axk[NV][6], ayk[NV][6], axv[NV][6], ayv[NV][6];
    row_zero<NV>(axk);
    row_zero<NV>(ayk);
    row_zero<NV>(axv);
    row_zero<NV>(ayv);
    for (int i = wave; i < WIN; i += 4) {
        const long tok = w.token_of(i);
        float kx[NV][6], ky[NV][6], vx[NV][6], vy[NV][6];
        load_row<NV>(p.kx + tok * D, lane, kx);
        if (p.ky) load_row_f16<NV>(p.ky + tok * D, lane, ky);
        load_row<NV>(p.vx + tok * D, lane, vx);
        if (p.vy) load_row_f16<NV>(p.vy + tok * D, lane, vy);
        const float dsi = sc[i], pi = dp[i];
        const float muk = stk[i], wk = dsi * stk[WP + i], muv = stv[i], wv = pi * stv[WP + i];
        row_axpy<NV>(dsi, kx, axk);
        row_axpy<NV>(pi, vx, axv);
#pragma unroll
        for (int s = 0; s < NV; ++s)
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                if (p.ky) ayk[s][j] = fmaf(wk, ky[s][j] - muk, ayk[s][j]);
                if (p.vy) ayv[s][j] = fmaf(wv, vy[s][j] - muv, ayv[s][j]);
            }
    }
    auto reduce_out = [&](const float (&a)[NV][6], float* dst) {
        __syncthreads();
        store_partial_row<NV>(part, wave, lane, a);
        __syncthreads();
        sum_partial_rows<NV>(part, tid, dst);
    };
    if (p.sxk) reduce_out(axk, p.sxk);             // (the pointers are the same for the whole workgroup: the barriers inside are uniform)
    if (p.sxv) reduce_out(axv, p.sxv);
    if (p.ky && p.syk) reduce_out(ayk, p.syk);
    if (p.vy && p.syv) reduce_out(ayv, p.syv);
}

// ---- d y of one token of an adaptor stream (local_attn.hip: adapt_dy_kernel has the algebra), the one body of adapt_dy_kernel and
// ragged_adapt_dy_kernel (ragged_train.hip): the caller finds the token's rows and the row of the rank-1 vector.  One wave; csum: this lane's
// column sums of dy as stored (bf16-rounded).
template <int NV>
__device__ __forceinline__ void adapt_dy_token(const _Float16* y_row, const uint16_t* gamma, const void* vec_row, int vec_f32, float c, float alpha, float eps,
                                               uint16_t* dy_row, uint16_t* r1_row, int lane, float (&csum)[NV][6]) {
    constexpr int D = NV * 384;
    float y[NV][6], v[NV][6], vg[NV][6];
    load_row_f16<NV>(y_row, lane, y);
    if (vec_f32) load_row_f32<NV>(reinterpret_cast<const float*>(vec_row), lane, v);
    else load_row<NV>(reinterpret_cast<const uint16_t*>(vec_row), lane, v);
    load_row<NV>(gamma, lane, vg);
    float mu, rstd;
    ln_stats<NV>(y, eps, mu, rstd);
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int j = 0; j < 6; ++j) y[s][j] = (y[s][j] - mu) * rstd;      // yhat
    row_mul<NV>(v, vg, vg);                                               // (vec gamma)
    const float m1 = wave_sum_fast(row_sum<NV>(vg)) * (1.0f / D);
    const float m2 = wave_sum_fast(row_dot<NV>(vg, y)) * (1.0f / D);
    const float k = alpha * c * rstd;
#pragma unroll
    for (int s = 0; s < NV; ++s) {
        float r[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) r[j] = k * (vg[s][j] - m1 - y[s][j] * m2);
        seg12_accum(csum[s], store_seg12(dy_row + 384 * s + 6 * lane, r));
    }
    if (r1_row) {
        const float k1 = (1.0f - alpha) * c;
        store_row_bf16<NV>(r1_row, lane, false, [&](int s, int j) { return k1 * v[s][j]; });
    }
}

// ---- rows [first, first + count) of an f32 [*, E] matrix summed into out[E], in a fixed order and without atomics: the one body of
// ragged_dq_item_kernel (ragged_train.hip: the dq rows of an item's windows) and rmg_dq_pair_kernel (ragged_multi_guide_train.hip: of a
// pair's).  Workgroup x of E / 64, 256 threads = 16 stripes x 16 lanes of 4 channels: stripe s sums rows s, s + 16, ... in order, the sixteen
// partial rows are added pairwise through LDS.
__device__ __forceinline__ void sum_rows_striped(const float* m, long first, int count, int E, float* out, float4 (*red)[16]) {
    const int lane = threadIdx.x & 15, stripe = threadIdx.x >> 4;
    const int c = blockIdx.x * 64 + 4 * lane;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < E)
        for (int w = stripe; w < count; w += 16) {
            const float4 v = *reinterpret_cast<const float4*>(m + (first + w) * E + c);
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
    if (stripe == 0 && c < E) *reinterpret_cast<float4*>(out + c) = red[0][lane];
}

}  // namespace hicom
