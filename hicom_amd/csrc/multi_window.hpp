// The window of the local stage for several guides at once, shared by the multi-guide step (multi_guide.hip: the guides of one clip) and
// the ragged multi-guide step (ragged_multi_guide.hip: the guides of the window's own item).
#pragma once
#include "segment_item.hpp"

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

// All Q guides of one window, in groups of kGuideGroup (the window's rows are expected to come from L2 from the second group on).
// guide: the guide rows, the window's first guide is row q0; o: the first guide's context row, guide q's `plane` elements times q
// further.  Q and q0 must be wave-uniform.
template <int NV>
__device__ __forceinline__ void multi_window_guides_ctx16(const uint16_t* key, const uint16_t* value, const uint16_t* guide, int q0, int Q,
                                                          const WindowGeom& g, int lane, float scale, _Float16* o, long plane) {
    constexpr int D = NV * 384;
    for (int g0 = 0; g0 < Q; g0 += kGuideGroup) {
        const uint16_t* q = guide + (long)(q0 + g0) * D;
        _Float16* og = o + (long)g0 * plane;
        switch (Q - g0 < kGuideGroup ? Q - g0 : kGuideGroup) {
            case 1: multi_window_ctx16<NV, 1>(key, value, q, g, lane, scale, og, plane); break;
            case 2: multi_window_ctx16<NV, 2>(key, value, q, g, lane, scale, og, plane); break;
            case 3: multi_window_ctx16<NV, 3>(key, value, q, g, lane, scale, og, plane); break;
            default: multi_window_ctx16<NV, 4>(key, value, q, g, lane, scale, og, plane); break;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Backward of one window for all Q guides of its item (ragged_multi_guide_train.hip: rmg_local_bwd_kernel), one 4-wave workgroup.
// Per guide q the algebra and the arithmetic of local_window_bwd (window_rows.hpp) without clip-scale:
//     s_qi = scale guide_q . k_i,  p_q = softmax(s_q),  dP_qi = dctx_q . v_i,  dS_qi = p_qi (dP_qi - sum_j p_qj dP_qj),
//     dq_q = scale sum_i dS_qi k_i                                  (f32, one row per (guide, window), written once)
// and per token, summed over the guides in fp32 in the order q = 0 .. Q - 1, rounded to bf16 once and stored plainly:
//     dkey_i = scale sum_q dS_qi guide_q,   dvalue_i = (dkey_i with value_is_key +) sum_q p_qi dctx_q
// Every dot product, softmax and dq sum is its own chain, written as the single-guide body writes it (token i of the window goes to wave
// i & 3 in both), so a guide's dS, p and dq do not depend on Q or on its place in a group, and with Q = 1 dq, dkey and dvalue have the
// single-guide kernel's values.  The guides go through the key / value walk in groups of kGuideGroup as in the forward: a row is loaded
// once per group.  key / value / dkey / dvalue point at the first token of the grid `w` indexes; guide at the item's first guide row;
// dctx / dq at guide 0's row of this window, guide q's `plane` elements times q further.  dkey / dvalue may be NULL.
// lsm: dS [Q][WP], p [Q][WP] (WP = WIN rounded up to 4) and the [4][D] slab: multi_window_bwd_smem.
// ---------------------------------------------------------------------------------------------------------------------------------
struct MultiWindowBwdArgs {
    const uint16_t* key;
    const uint16_t* value;
    const uint16_t* guide;  // [Q][D]
    int Q;
    float scale;
    const float* dctx;      // [Q] rows of D, `plane` apart
    float* dq;              // likewise
    long plane;
    uint16_t* dkey;         // bf16 [N, D] or NULL
    uint16_t* dvalue;       // bf16 [N, D] or NULL
    int value_is_key;
};

__host__ __device__ inline size_t multi_window_bwd_smem(int Q, int WIN, int D) { return ((size_t)2 * Q * ((WIN + 3) & ~3) + 4 * (size_t)D) * 4; }

// scores and dP of the guides g0 .. g0 + NG - 1: sc / dp rows g0 .. of [Q][WP]
template <int NV, int NG>
__device__ __forceinline__ void multi_window_bwd_scores(const MultiWindowBwdArgs& p, const WindowGeom& w, int g0, float* sc, float* dp, int WP, int lane,
                                                        int wave) {
    constexpr int D = NV * 384;
    float q[NG][NV][6], g[NG][NV][6];
#pragma unroll
    for (int u = 0; u < NG; ++u) {
        load_row<NV>(p.guide + (long)(g0 + u) * D, lane, q[u]);
        load_row_f32<NV>(p.dctx + (long)(g0 + u) * p.plane, lane, g[u]);
    }
    for (int i = wave; i < w.WIN; i += 4) {
        float k[NV][6], v[NV][6];
        const long tok = w.token_of(i);
        load_row<NV>(p.key + tok * D, lane, k);
        load_row<NV>(p.value + tok * D, lane, v);
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const float dot = wave_sum_fast(row_dot<NV>(q[u], k));
            const float dd = wave_sum_fast(row_dot<NV>(g[u], v));
            if (lane == 0) { sc[(g0 + u) * WP + i] = dot * p.scale; dp[(g0 + u) * WP + i] = dd; }
        }
    }
}

// dq of the guides g0 .. g0 + NG - 1 from dS (in sc): per wave one chain per guide over its tokens, the four waves' rows through the slab
template <int NV, int NG>
__device__ __forceinline__ void multi_window_bwd_dq(const MultiWindowBwdArgs& p, const WindowGeom& w, int g0, const float* sc, int WP, float* part, int tid) {
    constexpr int D = NV * 384;
    const int lane = tid & 63, wave = tid >> 6;
    float acc[NG][NV][6];
#pragma unroll
    for (int u = 0; u < NG; ++u) row_zero<NV>(acc[u]);
    for (int i = wave; i < w.WIN; i += 4) {
        float k[NV][6];
        load_row<NV>(p.key + w.token_of(i) * D, lane, k);
#pragma unroll
        for (int u = 0; u < NG; ++u) row_axpy<NV>(sc[(g0 + u) * WP + i] * p.scale, k, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < NG; ++u) {
        __syncthreads();                           // (the slab's readers of the guide before)
        store_partial_row<NV>(part, wave, lane, acc[u]);
        __syncthreads();
        sum_partial_rows<NV>(part, tid, p.dq + (long)(g0 + u) * p.plane);
    }
}

template <int NV>
__device__ __forceinline__ void multi_window_bwd(const MultiWindowBwdArgs& p, const WindowGeom& w, float* lsm, int tid) {
    constexpr int D = NV * 384;
    const int lane = tid & 63, wave = tid >> 6;
    const int WIN = w.WIN, WP = (WIN + 3) & ~3, Q = p.Q;
    float* sc = lsm;                               // [Q][WP] scores, then dS
    float* dp = lsm + Q * WP;                      // [Q][WP] dP, then p
    float* part = lsm + 2 * Q * WP;                // [4][D]

    // ---- phase 1: scores and dP, every key / value row once per group of guides ----
    for (int g0 = 0; g0 < Q; g0 += kGuideGroup)
        switch (Q - g0 < kGuideGroup ? Q - g0 : kGuideGroup) {
            case 1: multi_window_bwd_scores<NV, 1>(p, w, g0, sc, dp, WP, lane, wave); break;
            case 2: multi_window_bwd_scores<NV, 2>(p, w, g0, sc, dp, WP, lane, wave); break;
            case 3: multi_window_bwd_scores<NV, 3>(p, w, g0, sc, dp, WP, lane, wave); break;
            default: multi_window_bwd_scores<NV, 4>(p, w, g0, sc, dp, WP, lane, wave); break;
        }
    __syncthreads();
    // ---- softmax, delta, dS and p per guide: wave `wave` takes the guides q = wave, wave + 4, ...; a lane rewrites what it alone read ----
    for (int q = wave; q < Q; q += 4) {
        float* s = sc + q * WP;
        float* d = dp + q * WP;
        float mx, inv_sum, delta;
        softmax_stats(s, WIN, lane, mx, inv_sum, d, &delta);
        for (int i = lane; i < WIN; i += 64) {
            const float pi_ = expf(s[i] - mx) * inv_sum;
            s[i] = pi_ * (d[i] - delta);
            d[i] = pi_;
        }
    }
    __syncthreads();
    // ---- phase 2: dq per guide ----
    for (int g0 = 0; g0 < Q; g0 += kGuideGroup)
        switch (Q - g0 < kGuideGroup ? Q - g0 : kGuideGroup) {
            case 1: multi_window_bwd_dq<NV, 1>(p, w, g0, sc, WP, part, tid); break;
            case 2: multi_window_bwd_dq<NV, 2>(p, w, g0, sc, WP, part, tid); break;
            case 3: multi_window_bwd_dq<NV, 3>(p, w, g0, sc, WP, part, tid); break;
            default: multi_window_bwd_dq<NV, 4>(p, w, g0, sc, WP, part, tid); break;
        }
    // ---- phase 3: the token side, one fp32 chain per token and channel over the guides in order, one rounding, one plain store ----
    if (!p.dkey && !p.dvalue) return;
    const bool key_side = p.dkey || p.value_is_key;
    for (int i = wave; i < WIN; i += 4) {
        const long tok = w.token_of(i);
        float dk[NV][6];
        row_zero<NV>(dk);
        if (key_side)
            for (int q = 0; q < Q; ++q) {
                float gq[NV][6];
                load_row<NV>(p.guide + (long)q * D, lane, gq);
                row_axpy<NV>(sc[q * WP + i] * p.scale, gq, dk);
            }
        if (p.dkey) store_row_bf16<NV>(p.dkey + tok * D, lane, false, [&](int s, int j) { return dk[s][j]; });
        if (p.dvalue) {
            if (!p.value_is_key) row_zero<NV>(dk);
            for (int q = 0; q < Q; ++q) {
                float gc[NV][6];
                load_row_f32<NV>(p.dctx + (long)q * p.plane, lane, gc);
                row_axpy<NV>(dp[q * WP + i], gc, dk);
            }
            store_row_bf16<NV>(p.dvalue + tok * D, lane, false, [&](int s, int j) { return dk[s][j]; });
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The logits form: the raw dot products key_n . guide_q come precomputed, logits f32 [Q][tokens] with guide q's
// plane q_stride floats behind guide 0's (hicom_head_scores_multi_fwd writes them).  No key row is read and there is no dot product
// over the channels: lane i of the wave fetches the logit of the window's token i, `scale` and the softmax follow as in
// multi_window_ctx16, and every value row of the window is loaded once per group of NG guides into NG accumulators.  lrows: the
// group's first logit plane.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int NV, int NG>
__device__ __forceinline__ void multi_window_logits_ctx16(const uint16_t* value, const float* lrows, long q_stride, const WindowGeom& g, int lane,
                                                          float scale, _Float16* o, long plane) {
    constexpr int D = NV * 384;
    const long mine = g.token_of(lane < g.WIN ? lane : 0);
    float pw[NG];
#pragma unroll
    for (int u = 0; u < NG; ++u) {
        const float sc = lane < g.WIN ? lrows[(long)u * q_stride + mine] * scale : -3.0e38f;
        const float mx = wave_max_fast(sc);
        const float e = lane < g.WIN ? expf(sc - mx) : 0.f;
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

// All Q guides of one window in groups of kGuideGroup, as multi_window_guides_ctx16 walks them; logits: guide q0's plane.
template <int NV>
__device__ __forceinline__ void multi_window_guides_logits_ctx16(const uint16_t* value, const float* logits, long q_stride, int Q, const WindowGeom& g,
                                                                 int lane, float scale, _Float16* o, long plane) {
    for (int g0 = 0; g0 < Q; g0 += kGuideGroup) {
        const float* l = logits + (long)g0 * q_stride;
        _Float16* og = o + (long)g0 * plane;
        switch (Q - g0 < kGuideGroup ? Q - g0 : kGuideGroup) {
            case 1: multi_window_logits_ctx16<NV, 1>(value, l, q_stride, g, lane, scale, og, plane); break;
            case 2: multi_window_logits_ctx16<NV, 2>(value, l, q_stride, g, lane, scale, og, plane); break;
            case 3: multi_window_logits_ctx16<NV, 3>(value, l, q_stride, g, lane, scale, og, plane); break;
            default: multi_window_logits_ctx16<NV, 4>(value, l, q_stride, g, lane, scale, og, plane); break;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The same for the k / v adaptor recipe on PREPARED planes (multi_guide.hip: multi_guide_local_adapt_kernel): the window of
// local_window_adapt_ctx16 (segment_item.hpp) for NG guides in one walk.  ky / vy are the y = MLP(x) planes a clip keeps
// (hicom_clip_adapt_prepare_fwd); either may be NULL (that stream is not adapted and takes blend_dot's plain path), not both.
//
// What does not depend on the guide is done once per row: the x row and the y row are loaded once per group, and ln_stats of the y row
// -- a function of the row alone -- is computed once.  What depends on it is written as the single-guide loop writes it: every guide
// has its own affine_prep, blend_dot's two dot products and its blend expression, its own logit, softmax, accx / accy / smu chains and
// the unchanged epilogue.  So a guide's context does not depend on NG, on its place in the group or on its neighbours, and with one
// guide it has the bits of the batched adaptor step.  (gamma is NOT folded into the y row once per row: that would round differently.)
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kAdaptGuideGroup = 4;    // guides per walk of the adaptor window: 36 (q, qg) resp. 36 (accx, accy) floats per guide and lane
                                       // beside the x row and the y row in flight (DESIGN.md §3.10 has the resource table behind the choice)

// blend_dot (window_rows.hpp) with the LayerNorm statistics of the y row given: the same two dot products, the same expression
template <int NV>
__device__ __forceinline__ float blend_dot_stats(const float (&x)[NV][6], const float (&y)[NV][6], bool has_y, const float (&v)[NV][6],
                                                const float (&vg)[NV][6], float cg, float cb, float a, float mu, float rstd) {
    const float dx = wave_sum_fast(row_dot<NV>(v, x));
    if (!has_y) return dx;
    const float dy = wave_sum_fast(row_dot<NV>(vg, y));
    return (1.0f - a) * dx + a * (rstd * (dy - mu * cg) + cb);
}

template <int NV, int NG>
__device__ __forceinline__ void multi_window_adapt_ctx16(const uint16_t* kx, const _Float16* ky, const uint16_t* vx, const _Float16* vy,
                                                         const SegAdaptParams& ad, const uint16_t* qrows, const WindowGeom& g, int lane,
                                                         float scale, _Float16* o, long plane) {
    constexpr int D = NV * 384;
    const float ak = ky ? read_alpha(ad.kalpha, ad.alpha_f32) : 0.f, av = vy ? read_alpha(ad.valpha, ad.alpha_f32) : 0.f;
    float sc[NG];
    {
        float q[NG][NV][6], qg[NG][NV][6];
        float cg[NG], cb[NG];
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            load_row<NV>(qrows + (long)u * D, lane, q[u]);
            cg[u] = 0.f;
            cb[u] = 0.f;
            if (ky) affine_prep<NV>(q[u], ad.kgamma, ad.kbeta, lane, qg[u], cg[u], cb[u]);
            sc[u] = -3.0e38f;
        }
        for (int i = 0; i < g.WIN; ++i) {
            const long tok = g.token_of(i);
            float x[NV][6], y[NV][6];
            load_row<NV>(kx + tok * D, lane, x);
            float mu = 0.f, rstd = 0.f;
            if (ky) {
                load_row_f16<NV>(ky + tok * D, lane, y);
                ln_stats<NV>(y, ad.eps, mu, rstd);
            }
#pragma unroll
            for (int u = 0; u < NG; ++u) {
                const float d = blend_dot_stats<NV>(x, y, ky != nullptr, q[u], qg[u], cg[u], cb[u], ak, mu, rstd) * scale;
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
    float accx[NG][NV][6], accy[NG][NV][6];
    float smu[NG];                                  // sum_n p_n rstd_n mu_n per guide (identical in every lane)
#pragma unroll
    for (int u = 0; u < NG; ++u) {
        row_zero<NV>(accx[u]);
        row_zero<NV>(accy[u]);
        smu[u] = 0.f;
    }
    for (int i = 0; i < g.WIN; ++i) {
        const long tok = g.token_of(i);
        float x[NV][6], y[NV][6];
        load_row<NV>(vx + tok * D, lane, x);
        float mu = 0.f, rstd = 0.f;
        if (vy) {
            load_row_f16<NV>(vy + tok * D, lane, y);
            ln_stats<NV>(y, ad.eps, mu, rstd);
        }
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const float pi = __shfl(pw[u], i, 64);
            row_axpy<NV>(pi, x, accx[u]);
            if (vy) {
                const float wy = pi * rstd;
                smu[u] = fmaf(wy, mu, smu[u]);
                row_axpy<NV>(wy, y, accy[u]);
            }
        }
    }
    if (vy) {
        float gm[NV][6], bt[NV][6];
        load_row<NV>(ad.vgamma, lane, gm);
        load_row<NV>(ad.vbeta, lane, bt);
#pragma unroll
        for (int u = 0; u < NG; ++u)
#pragma unroll
            for (int s = 0; s < NV; ++s)
#pragma unroll
                for (int j = 0; j < 6; ++j)
                    accx[u][s][j] = (1.0f - av) * accx[u][s][j] + av * (gm[s][j] * (accy[u][s][j] - smu[u]) + bt[s][j]);
    }
#pragma unroll
    for (int u = 0; u < NG; ++u)
#pragma unroll
        for (int s = 0; s < NV; ++s)
#pragma unroll
            for (int j = 0; j < 6; ++j)
                o[(long)u * plane + 384 * s + 6 * lane + j] = (_Float16)fminf(fmaxf(accx[u][s][j], -65504.f), 65504.f);
}

// All Q guides of one window in groups of GROUP, the remainder group through its own NG instantiation (no padded work); from the second
// group on the wave walks the window's x and y rows again (that those re-reads come from L2 is expected, not measured).  Arguments as
// multi_window_guides_ctx16; Q and q0 must be wave-uniform.
template <int NV, int GROUP>
__device__ __forceinline__ void multi_window_guides_adapt_ctx16(const uint16_t* kx, const uint16_t* vx, const SegAdaptParams& ad,
                                                                const uint16_t* guide, int q0, int Q, const WindowGeom& g, int lane,
                                                                float scale, _Float16* o, long plane) {
    static_assert(GROUP >= 1 && GROUP <= 4, "the switch below knows remainders up to 3");
    constexpr int D = NV * 384;
    for (int g0 = 0; g0 < Q; g0 += GROUP) {
        const uint16_t* q = guide + (long)(q0 + g0) * D;
        _Float16* og = o + (long)g0 * plane;
        const int ng = Q - g0 < GROUP ? Q - g0 : GROUP;
        // (wave-uniform; the comparisons with GROUP fold away: a group of 2 keeps the first and the last branch only)
        if (ng == GROUP) multi_window_adapt_ctx16<NV, GROUP>(kx, ad.ky, vx, ad.vy, ad, q, g, lane, scale, og, plane);
        else if (GROUP > 3 && ng == 3) multi_window_adapt_ctx16<NV, 3>(kx, ad.ky, vx, ad.vy, ad, q, g, lane, scale, og, plane);
        else if (GROUP > 2 && ng == 2) multi_window_adapt_ctx16<NV, 2>(kx, ad.ky, vx, ad.vy, ad, q, g, lane, scale, og, plane);
        else multi_window_adapt_ctx16<NV, 1>(kx, ad.ky, vx, ad.vy, ad, q, g, lane, scale, og, plane);
    }
}

}  // namespace hicom
