// The merge + fold of ONE folded row of a clip stream group: the row's partials of one chunk merged into the
// chunk's UN-normalised set and folded into the row's carried state in place.  Shared by the two group files (clip_stream_group.hip: one
// guide per slot; clip_stream_group_multi.hip: several), so both round identically: a row's result depends on its partials, its logits,
// its frame offset and its carried state only.
#pragma once
#include <math.h>

#include "segment_item.hpp"

namespace hicom {

// e^(m - M') as the weight of a term whose running max is m; an empty term (m = -inf) weighs 0 whatever M' is (clip_stream.hip: fold_weight)
__device__ __forceinline__ float group_fold_weight(float m, float m_new) { return m == -INFINITY ? 0.f : expf(m - m_new); }

// The chunk's un-normalised set relative to the chunk maximum M_c (the item's partials in the slots [slot0, slot0 + nparts), its logits s):
//   L_c = sum_p e^(m_p - M_c) l_p,   ACC_c = sum_p e^(m_p - M_c) acc_p + sum_s marg_s pe[s],   marg = sum e^(logit - M_c) over the other two axes,
// the t rows of pe taken at p.t0i + t0 + t.  Then the fold into the carried row (ml = its (M, L), acc = its E floats), in place:
//   M' = max(M, M_c),  L' = e^(M - M') L + e^(M_c - M') L_c,  ACC' = e^(M - M') ACC + e^(M_c - M') ACC_c;  an empty term weighs 0.
// Fixed summation orders, no atomics.  ms: LDS, seg_merge_smem(T, H, W) bytes.
__device__ __forceinline__ void merge_fold_row(const SegMergeParams& p, float* ms, int r, int tid, int T, int t0, int nparts, long slot0, const float* s,
                                               float* ml, float* acc) {
    const int H = p.H, W = p.W;
    float* rowsum = ms;                 // [T][H]: weights summed over x
    float* colsum = ms + T * H;         // [T][W]: weights summed over y
    float* marg = colsum + T * W;       // [T + H + W]
    const long pbase = slot0 * 16 + r;
    float Mc = -1.0e30f;
    for (int c = 0; c < nparts; ++c) Mc = fmaxf(Mc, p.part_m[pbase + c * 16]);
    float Lc = 0.f;
    for (int c = 0; c < nparts; ++c) Lc += p.part_l[pbase + c * 16] * expf(p.part_m[pbase + c * 16] - Mc);
    if (p.pe) {
        for (int i = tid; i < T * H; i += 256) {
            float a = 0.f;
            for (int x = 0; x < W; ++x) a += expf(s[(long)i * W + x] - Mc);
            rowsum[i] = a;
        }
        for (int i = tid; i < T * W; i += 256) {
            const int t = i / W, x = i - t * W;
            float a = 0.f;
            for (int y = 0; y < H; ++y) a += expf(s[((long)t * H + y) * W + x] - Mc);
            colsum[i] = a;
        }
        __syncthreads();
        for (int i = tid; i < T + H + W; i += 256) {
            float a = 0.f;
            if (i < T) {
                for (int y = 0; y < H; ++y) a += rowsum[i * H + y];
            } else if (i < T + H) {
                for (int t = 0; t < T; ++t) a += rowsum[t * H + (i - T)];
            } else {
                for (int t = 0; t < T; ++t) a += colsum[t * W + (i - T - H)];
            }
            marg[i] = a;
        }
    }
    // every thread reads the old pair in front of the barrier; lane 0 writes the new one behind it
    const float m_old = ml[0], l_old = ml[1];
    __syncthreads();
    const float m_new = fmaxf(m_old, Mc);
    const float w_old = group_fold_weight(m_old, m_new), w_c = group_fold_weight(Mc, m_new);
    if (tid == 0) *reinterpret_cast<float2*>(ml) = make_float2(m_new, fmaf(w_c, Lc, w_old * l_old));
    const long tf = (long)p.t0i + t0;
    for (int e = tid; e < p.E; e += 256) {
        float v = 0.f;
        for (int c = 0; c < nparts; ++c)
            v += expf(p.part_m[pbase + c * 16] - Mc) * p.part_acc[(slot0 + c) * 16 * p.E + (long)r * p.E + e];
        if (p.pe) {
            float pos = 0.f;
            for (int t = 0; t < T; ++t) pos = fmaf(marg[t], p.pe[(tf + t) * p.E + e], pos);
            for (int y = 0; y < H; ++y) pos = fmaf(marg[T + y], p.pe[(long)(p.y0i + y) * p.E + e], pos);
            for (int x = 0; x < W; ++x) pos = fmaf(marg[T + H + x], p.pe[(long)(p.x0i + x) * p.E + e], pos);
            v += pos;
        }
        float a = m_old != -INFINITY ? acc[e] * w_old : 0.f;
        if (w_c != 0.f) a += v * w_c;
        acc[e] = a;
    }
}

}  // namespace hicom
