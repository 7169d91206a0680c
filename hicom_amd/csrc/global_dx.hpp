// d frames_feature of the global stage for 64 tokens of ONE token run: the one body of global_dx_kernel (small_ops.hip: the run is the
// whole call, the tile comes from blockIdx) and ragged_global_dx_kernel (ragged_train.hip: the run is an item, the tile comes from a device table).
//     dx[n] (+)= sum_r dS[r, n] qt[r] + exp(S[r, n] - M_r) / L_r dctx[r]          (direct recipe: <= 16 folded rows)
// Thread t owns channels 4t .. 4t+3 with the 2 * rows coefficient rows (qt | dctx) of those channels in registers and walks the tokens:
// per token 2 * rows broadcast LDS reads of the coefficients (dS, p), 8 * rows FMAs, one 8-byte store.  Every pointer is the run's own:
// S / dS [rows][stride] from its first token, ml / qt / dctx its rows, dx its first token's row; n0 the tile's first token inside the run
// and N the run's length.  coef: [64][2 * RMAX] floats of LDS.
#pragma once
#include "common.hpp"

namespace hicom {

template <int RMAX>
__device__ __forceinline__ void global_dx_tile(const float* S, const float* dS, long stride, const float* ml, const float* qt, const float* dctx,
                                               int rows, long n0, long N, int E, uint16_t* dx, int accumulate, float (*coef)[2 * RMAX]) {
    const int tid = threadIdx.x;
    // every coefficient the unrolled loop below reads is written here: rows >= `rows` and tokens past the run's end as zeros (stale LDS
    // holding Inf / NaN would otherwise meet the zeroed wq / wd and give NaN)
    for (int idx = tid; idx < 64 * RMAX; idx += blockDim.x) {
        const int r = idx / 64, t = idx - r * 64;
        const long n = n0 + t;
        float a = 0.f, b = 0.f;
        if (r < rows && n < N) {
            a = dS[(long)r * stride + n];
            b = expf(S[(long)r * stride + n] - ml[2 * r]) / ml[2 * r + 1];
        }
        coef[t][r] = a;
        coef[t][RMAX + r] = b;
    }
    const int c4 = 4 * tid;
    float4 wq[RMAX], wd[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        wq[r] = make_float4(0.f, 0.f, 0.f, 0.f);
        wd[r] = wq[r];
        if (r < rows && c4 < E) {
            wq[r] = *reinterpret_cast<const float4*>(qt + (long)r * E + c4);
            wd[r] = *reinterpret_cast<const float4*>(dctx + (long)r * E + c4);
        }
    }
    __syncthreads();
    if (c4 >= E) return;
    for (int t = 0; t < 64 && n0 + t < N; ++t) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        uint16_t* o = dx + (n0 + t) * (long)E + c4;
        if (accumulate) {
            const uint2 old = *reinterpret_cast<const uint2*>(o);
            a = make_float4(bf16lo_to_f32(old.x), bf16hi_to_f32(old.x), bf16lo_to_f32(old.y), bf16hi_to_f32(old.y));
        }
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            const float ca = coef[t][r], cb = coef[t][RMAX + r];
            a.x = fmaf(ca, wq[r].x, a.x); a.y = fmaf(ca, wq[r].y, a.y); a.z = fmaf(ca, wq[r].z, a.z); a.w = fmaf(ca, wq[r].w, a.w);
            a.x = fmaf(cb, wd[r].x, a.x); a.y = fmaf(cb, wd[r].y, a.y); a.z = fmaf(cb, wd[r].z, a.z); a.w = fmaf(cb, wd[r].w, a.w);
        }
        *reinterpret_cast<uint2*>(o) = make_uint2((unsigned)f32_to_bf16(a.x) | ((unsigned)f32_to_bf16(a.y) << 16),
                                                  (unsigned)f32_to_bf16(a.z) | ((unsigned)f32_to_bf16(a.w) << 16));
    }
}

}  // namespace hicom
