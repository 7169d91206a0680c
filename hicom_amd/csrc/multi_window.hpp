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
