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

// The same for a run whose tokens meet MANY rows -- the nh Q_i folded rows of an item with Q_i guides, up to 288
// (ragged_multi_guide_train.hip: rmg_global_dx_kernel).  The coefficient rows no longer fit in registers, so the roles are turned round:
// thread t keeps the accumulators of its 4 channels for kDxSubTile tokens in registers and walks the rows, kDxRowBlock of them at a time
// through LDS (coefficients) and four at a time through registers (qt | dctx, from L2).  Per token and channel this is ONE fp32 chain in
// row order -- fma(dS, qt), fma(p, dctx) per row, as above -- that starts from the bf16 row the window backward left (accumulate) and ends
// in one bf16 store, whatever the number of rows; rows past `rows` and tokens past the run's end enter as zero coefficients (an exact
// no-op of the chain), so with rows <= 16 the result has global_dx_tile's values.  coef: [kDxSubTile][kDxCoefStride] floats of LDS.
constexpr int kDxRowBlock = 32, kDxSubTile = 32, kDxCoefStride = 2 * kDxRowBlock + 4;

__device__ __forceinline__ void global_dx_rows_tile(const float* S, const float* dS, long stride, const float* ml, const float* qt, const float* dctx,
                                                    int rows, long n0, long N, int E, uint16_t* dx, int accumulate, float (*coef)[kDxCoefStride]) {
    const int tid = threadIdx.x, c4 = 4 * tid;
    const bool live = c4 < E;                      // (threads past the last channel fill coefficients and meet the barriers only)
    for (int sub = 0; sub < 64 && n0 + sub < N; sub += kDxSubTile) {
        const long nb = n0 + sub;
        float4 acc[kDxSubTile];
#pragma unroll
        for (int t = 0; t < kDxSubTile; ++t) {
            acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (accumulate && live && nb + t < N) {
                const uint2 old = *reinterpret_cast<const uint2*>(dx + (nb + t) * (long)E + c4);
                acc[t] = make_float4(bf16lo_to_f32(old.x), bf16hi_to_f32(old.x), bf16lo_to_f32(old.y), bf16hi_to_f32(old.y));
            }
        }
        for (int rb = 0; rb < rows; rb += kDxRowBlock) {
            __syncthreads();                       // (the block before has been read)
            for (int idx = tid; idx < kDxRowBlock * kDxSubTile; idx += blockDim.x) {
                const int r = idx / kDxSubTile, t = idx - r * kDxSubTile, R = rb + r;
                const long n = nb + t;
                float a = 0.f, b = 0.f;
                if (R < rows && n < N) {
                    a = dS[(long)R * stride + n];
                    b = expf(S[(long)R * stride + n] - ml[2 * R]) / ml[2 * R + 1];
                }
                coef[t][r] = a;
                coef[t][kDxRowBlock + r] = b;
            }
            __syncthreads();
            if (!live) continue;
            for (int r0 = 0; r0 < kDxRowBlock && rb + r0 < rows; r0 += 4) {
                float4 wq[4], wd[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int R = rb + r0 + r;
                    wq[r] = make_float4(0.f, 0.f, 0.f, 0.f);
                    wd[r] = wq[r];
                    if (R < rows) {
                        wq[r] = *reinterpret_cast<const float4*>(qt + (long)R * E + c4);
                        wd[r] = *reinterpret_cast<const float4*>(dctx + (long)R * E + c4);
                    }
                }
#pragma unroll
                for (int t = 0; t < kDxSubTile; ++t) {
                    const float4 ca4 = *reinterpret_cast<const float4*>(&coef[t][r0]), cb4 = *reinterpret_cast<const float4*>(&coef[t][kDxRowBlock + r0]);
                    const float ca[4] = {ca4.x, ca4.y, ca4.z, ca4.w}, cb[4] = {cb4.x, cb4.y, cb4.z, cb4.w};
                    float4 a = acc[t];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        a.x = fmaf(ca[r], wq[r].x, a.x); a.y = fmaf(ca[r], wq[r].y, a.y); a.z = fmaf(ca[r], wq[r].z, a.z); a.w = fmaf(ca[r], wq[r].w, a.w);
                        a.x = fmaf(cb[r], wd[r].x, a.x); a.y = fmaf(cb[r], wd[r].y, a.y); a.z = fmaf(cb[r], wd[r].z, a.z); a.w = fmaf(cb[r], wd[r].w, a.w);
                    }
                    acc[t] = a;
                }
            }
        }
        if (live) {
#pragma unroll
            for (int t = 0; t < kDxSubTile; ++t)
                if (nb + t < N)
                    *reinterpret_cast<uint2*>(dx + (nb + t) * (long)E + c4) =
                        make_uint2((unsigned)f32_to_bf16(acc[t].x) | ((unsigned)f32_to_bf16(acc[t].y) << 16),
                                   (unsigned)f32_to_bf16(acc[t].z) | ((unsigned)f32_to_bf16(acc[t].w) << 16));
        }
    }
}

}  // namespace hicom
