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

}  // namespace hicom
