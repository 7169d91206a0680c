// Row-wise kernels around the attention stages: the GELU forms and derivatives of the adaptor-MLP / head-projection backward
// (elementwise, 16-byte accesses; a wave per row where the column sums come out of the same pass), column sums of a token matrix
// (bias gradients) and the trilinear pooling of the per-window queries.  All HBM-bound streaming passes.  The row forms use the
// 12-bytes-per-lane row layout of the window kernels (window_rows.hpp).
#include "window_rows.hpp"

namespace hicom {

// ---- elementwise helpers of the adaptor-MLP backward (token-stream sized, 16-byte accesses) ------------------------------------------------
// erf-GELU derivative Phi(x) + x phi(x), same erf approximation as gelu_erf (A&S 7.1.26)
__device__ __forceinline__ float gelu_erf_grad(float x) {
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    float poly = fmaf(1.061405429f, t, -1.453152027f);
    poly = fmaf(poly, t, 1.421413741f);
    poly = fmaf(poly, t, -0.284496736f);
    poly = fmaf(poly, t, 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(-z * z * 1.44269504088896340736f);           // exp(-x^2 / 2)
    const float tail = poly * t * e;                                                    // 1 - erf(z)
    const float cdf = x >= 0.f ? 1.0f - 0.5f * tail : 0.5f * tail;
    return fmaf(x * 0.3989422804014327f, e, cdf);
}

// tanh form (HF gelu_pytorch_tanh, the SigLIP head's activation) and its derivative:  g(x) = x s(2u),  u = c0 (x + c1 x^3),
// s = logistic;  g'(x) = s + x s (1 - s) 2 c0 (1 + 3 c1 x^2)
__device__ __forceinline__ float gelu_tanh_val(float x) {
    const float t = x * x;
    const float arg = x * fmaf(t, -0.10294324f, -2.3022082f);                             // -2u log2(e)
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(arg));
}
__device__ __forceinline__ float gelu_tanh_grad(float x) {
    const float t = x * x;
    const float arg = x * fmaf(t, -0.10294324f, -2.3022082f);
    const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(arg));
    const float du2 = 1.5957691216f * fmaf(0.134145f, t, 1.0f);                            // d(2u)/dx = 2 c0 (1 + 3 c1 x^2)
    return fmaf(x * sg * (1.0f - sg), du2, sg);
}

// Pitched forms for the head projection's hidden layer ([M, 4304] inside rows of 4544 fp16 elements):
//   act_rows:      a_bf16[r, c] = act(h[r, c])                  (operand of dW2 = dY^T a; dense [rows, cols])
//   act_bwd_rows:  da[r, c]    *= act'(h[r, c])  in place       (dense [rows, cols] bf16)
// cols % 8 == 0; one 16-byte vector per thread.  TANH: gelu_pytorch_tanh, else erf.
template <bool TANH>
__global__ __launch_bounds__(256) void act_rows_kernel(const _Float16* h, long ldh, long rows, int c8, uint16_t* abf) {
    typedef _Float16 half8 __attribute__((ext_vector_type(8)));
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * c8) return;
    const long r = i / c8;
    const int c = (int)(i - r * c8);
    const half8 hv = *reinterpret_cast<const half8*>(h + r * ldh + 8 * c);
    u32x4 bv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float lo = TANH ? gelu_tanh_val((float)hv[2 * e]) : gelu_erf((float)hv[2 * e]);
        const float hi = TANH ? gelu_tanh_val((float)hv[2 * e + 1]) : gelu_erf((float)hv[2 * e + 1]);
        bv[e] = f32_to_bf16(lo) | ((uint32_t)f32_to_bf16(hi) << 16);
    }
    reinterpret_cast<u32x4*>(abf)[i] = bv;
}
template <bool TANH>
__global__ __launch_bounds__(256) void act_bwd_rows_kernel(uint16_t* da, const _Float16* h, long ldh, long rows, int c8) {
    typedef _Float16 half8 __attribute__((ext_vector_type(8)));
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * c8) return;
    const long r = i / c8;
    const int c = (int)(i - r * c8);
    const half8 hv = *reinterpret_cast<const half8*>(h + r * ldh + 8 * c);
    u32x4 d = reinterpret_cast<const u32x4*>(da)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float g0 = TANH ? gelu_tanh_grad((float)hv[2 * e]) : gelu_erf_grad((float)hv[2 * e]);
        const float g1 = TANH ? gelu_tanh_grad((float)hv[2 * e + 1]) : gelu_erf_grad((float)hv[2 * e + 1]);
        d[e] = f32_to_bf16(bf16lo_to_f32(d[e]) * g0) | ((uint32_t)f32_to_bf16(bf16hi_to_f32(d[e]) * g1) << 16);
    }
    reinterpret_cast<u32x4*>(da)[i] = d;
}

// a16 = GELU(h) as fp16 (operand of the recomputed second GEMM) and abf = GELU(h) as bf16 (operand of dW2 = dy^T a): n elements, n % 8 == 0
__global__ __launch_bounds__(256) void gelu_split_kernel(const _Float16* h, _Float16* a16, uint16_t* abf, long n8) {
    typedef _Float16 half8 __attribute__((ext_vector_type(8)));
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const half8 hv = reinterpret_cast<const half8*>(h)[i];
    half8 av;
    u32x4 bv;
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { f[e] = gelu_erf((float)hv[e]); av[e] = (_Float16)fminf(fmaxf(f[e], -65504.f), 65504.f); }
#pragma unroll
    for (int e = 0; e < 4; ++e) bv[e] = f32_to_bf16(f[2 * e]) | ((uint32_t)f32_to_bf16(f[2 * e + 1]) << 16);
    if (a16) reinterpret_cast<half8*>(a16)[i] = av;
    reinterpret_cast<u32x4*>(abf)[i] = bv;
}

// da (bf16, in place) *= GELU'(h)  (h fp16 pre-activation): the gradient through the adaptor's hidden activation
__global__ __launch_bounds__(256) void gelu_bwd_kernel(uint16_t* da, const _Float16* h, long n8) {
    typedef _Float16 half8 __attribute__((ext_vector_type(8)));
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const half8 hv = reinterpret_cast<const half8*>(h)[i];
    u32x4 d = reinterpret_cast<const u32x4*>(da)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float lo = bf16lo_to_f32(d[e]) * gelu_erf_grad((float)hv[2 * e]);
        const float hi = bf16hi_to_f32(d[e]) * gelu_erf_grad((float)hv[2 * e + 1]);
        d[e] = f32_to_bf16(lo) | ((uint32_t)f32_to_bf16(hi) << 16);
    }
    reinterpret_cast<u32x4*>(da)[i] = d;
}

// the same step with a wave per row and the rows strided over the grid, plus this workgroup's column sums of the result (as stored):
// the bias gradient db1 = sum over the tokens of d h1 without another pass over the 107-MB matrix
template <int NV>
__global__ __launch_bounds__(256) void gelu_bwd_rows_kernel(uint16_t* da, const _Float16* h, long N, float* col_parts) {
    constexpr int D = NV * 384;
    __shared__ float red[4][D];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float csum[NV][6];
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int j = 0; j < 6; ++j) csum[s][j] = 0.f;
    for (long r = (long)blockIdx.x * 4 + wave; r < N; r += (long)gridDim.x * 4) {
        float d[NV][6], hv[NV][6];
        load_row<NV>(da + r * D, lane, d);
        load_row_f16<NV>(h + r * D, lane, hv);
#pragma unroll
        for (int s = 0; s < NV; ++s) {
            float v[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) v[j] = d[s][j] * gelu_erf_grad(hv[s][j]);
            Seg12 w;
            w.a = f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
            w.b = f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
            w.c = f32_to_bf16(v[4]) | ((uint32_t)f32_to_bf16(v[5]) << 16);
            *reinterpret_cast<Seg12*>(da + r * D + 384 * s + 6 * lane) = w;
            csum[s][0] += bf16lo_to_f32(w.a); csum[s][1] += bf16hi_to_f32(w.a); csum[s][2] += bf16lo_to_f32(w.b);
            csum[s][3] += bf16hi_to_f32(w.b); csum[s][4] += bf16lo_to_f32(w.c); csum[s][5] += bf16hi_to_f32(w.c);
        }
    }
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int j = 0; j < 6; ++j) red[wave][384 * s + 6 * lane + j] = csum[s][j];
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += 256) col_parts[(long)blockIdx.x * D + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

// column sums of a bf16 [N, D] matrix (bias gradients: db = sum over the tokens): partial [gridDim.x][D] f32, a wave per row, rows
// strided over the grid; summed by hicom_partials_sum_fwd (block order: deterministic)
template <int NV>
__global__ __launch_bounds__(256) void colsum_kernel(const uint16_t* x, long N, float* parts) {
    constexpr int D = NV * 384;
    __shared__ float red[4][D];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float acc[NV][6];
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int j = 0; j < 6; ++j) acc[s][j] = 0.f;
    for (long r = (long)blockIdx.x * 4 + wave; r < N; r += (long)gridDim.x * 4) {
        float v[NV][6];
        load_row<NV>(x + r * D, lane, v);
#pragma unroll
        for (int s = 0; s < NV; ++s)
#pragma unroll
            for (int j = 0; j < 6; ++j) acc[s][j] += v[s][j];
    }
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int j = 0; j < 6; ++j) red[wave][384 * s + 6 * lane + j] = acc[s][j];
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += 256) parts[(long)blockIdx.x * D + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

// ---- pooled per-window query (trilinear, align_corners=False; projector.py:539-540) ----------
struct PoolParams {
    const uint16_t* x;
    int T, H, W, D, To, Ho, Wo;
    float* out;
};

__device__ __forceinline__ void lerp_tap(int i, int n_in, int n_out, int& i0, int& i1, float& lam) {
    // src = (i + 0.5) * n_in / n_out - 0.5 clamped at 0 (PyTorch area_pixel_compute_source_index)
    const float scale = (float)n_in / (float)n_out;
    float src = ((float)i + 0.5f) * scale - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = (int)floorf(src);
    if (i0 > n_in - 1) i0 = n_in - 1;
    i1 = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
    lam = src - (float)i0;
}

__global__ __launch_bounds__(256) void trilinear_pool_kernel(PoolParams p) {
    const int o = blockIdx.x;
    const int wo = o % p.Wo, ho = (o / p.Wo) % p.Ho, to = o / (p.Wo * p.Ho);
    int t0, t1, y0, y1, x0, x1;
    float lt, ly, lx;
    lerp_tap(to, p.T, p.To, t0, t1, lt);
    lerp_tap(ho, p.H, p.Ho, y0, y1, ly);
    lerp_tap(wo, p.W, p.Wo, x0, x1, lx);
    auto at = [&](int t, int y, int x, int c) -> float {
        return bf16_to_f32(p.x[(((long)t * p.H + y) * p.W + x) * p.D + c]);
    };
    for (int c = threadIdx.x; c < p.D; c += blockDim.x) {
        // same nesting as the separable restatement in the oracle: t, then h, then w
        const float a00 = at(t0, y0, x0, c) * (1.f - lt) + at(t1, y0, x0, c) * lt;
        const float a01 = at(t0, y0, x1, c) * (1.f - lt) + at(t1, y0, x1, c) * lt;
        const float a10 = at(t0, y1, x0, c) * (1.f - lt) + at(t1, y1, x0, c) * lt;
        const float a11 = at(t0, y1, x1, c) * (1.f - lt) + at(t1, y1, x1, c) * lt;
        const float b0 = a00 * (1.f - ly) + a10 * ly;
        const float b1 = a01 * (1.f - ly) + a11 * ly;
        p.out[(long)o * p.D + c] = b0 * (1.f - lx) + b1 * lx;
    }
}

}  // namespace hicom

using namespace hicom;

extern "C" int hicom_gelu_split_fwd(const void* h_f16, void* a_f16, void* a_bf16, int64_t n, void* stream) {
    HICOM_REQUIRE(h_f16 && a_bf16 && n > 0 && n % 8 == 0 && ((uintptr_t)h_f16 % 16 == 0) && ((uintptr_t)a_f16 % 16 == 0) && ((uintptr_t)a_bf16 % 16 == 0),
                  HICOM_EINVAL, "gelu_split: bad arguments (n %% 8, 16-byte alignment)");
    hipLaunchKernelGGL(gelu_split_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const _Float16*)h_f16, (_Float16*)a_f16,
                       (uint16_t*)a_bf16, (long)(n / 8));
    return hicom_host::check_launch("gelu_split");
}

extern "C" int hicom_gelu_bwd_fwd(void* da_bf16, const void* h_f16, int64_t n, int32_t D, float* col_parts, int32_t nparts, void* stream) {
    HICOM_REQUIRE(da_bf16 && h_f16 && n > 0 && n % 8 == 0 && ((uintptr_t)da_bf16 % 16 == 0) && ((uintptr_t)h_f16 % 16 == 0), HICOM_EINVAL,
                  "gelu_bwd: bad arguments (n %% 8, 16-byte alignment)");
    if (col_parts) {
        HICOM_REQUIRE((D == 1152 || D == 768) && n % D == 0 && nparts > 0, HICOM_EINVAL, "gelu_bwd: column partials need rows of D = 1152 / 768 and nparts > 0");
        if (D == 1152) hipLaunchKernelGGL(gelu_bwd_rows_kernel<3>, dim3((unsigned)nparts), dim3(256), 0, (hipStream_t)stream, (uint16_t*)da_bf16, (const _Float16*)h_f16, (long)(n / D), col_parts);
        else hipLaunchKernelGGL(gelu_bwd_rows_kernel<2>, dim3((unsigned)nparts), dim3(256), 0, (hipStream_t)stream, (uint16_t*)da_bf16, (const _Float16*)h_f16, (long)(n / D), col_parts);
        return hicom_host::check_launch("gelu_bwd");
    }
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint16_t*)da_bf16, (const _Float16*)h_f16,
                       (long)(n / 8));
    return hicom_host::check_launch("gelu_bwd");
}

extern "C" int hicom_act_rows_fwd(const void* h_f16, int64_t ldh, int64_t rows, int32_t cols, int32_t act, void* a_bf16, void* stream) {
    HICOM_REQUIRE(h_f16 && a_bf16 && rows > 0 && cols > 0 && cols % 8 == 0 && ldh >= cols && ldh % 8 == 0 && ((uintptr_t)h_f16 % 16 == 0) &&
                      ((uintptr_t)a_bf16 % 16 == 0) && (act == HICOM_ACT_GELU || act == 2), HICOM_EINVAL,
                  "act_rows: bad arguments (cols, ldh %% 8; 16-byte alignment; act GELU | GELU_TANH)");
    const long n = rows * (cols / 8);
    if (act == 2) hipLaunchKernelGGL(act_rows_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const _Float16*)h_f16, (long)ldh, (long)rows, cols / 8, (uint16_t*)a_bf16);
    else hipLaunchKernelGGL(act_rows_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const _Float16*)h_f16, (long)ldh, (long)rows, cols / 8, (uint16_t*)a_bf16);
    return hicom_host::check_launch("act_rows");
}

extern "C" int hicom_act_bwd_rows_fwd(void* da_bf16, const void* h_f16, int64_t ldh, int64_t rows, int32_t cols, int32_t act, void* stream) {
    HICOM_REQUIRE(h_f16 && da_bf16 && rows > 0 && cols > 0 && cols % 8 == 0 && ldh >= cols && ldh % 8 == 0 && ((uintptr_t)h_f16 % 16 == 0) &&
                      ((uintptr_t)da_bf16 % 16 == 0) && (act == HICOM_ACT_GELU || act == 2), HICOM_EINVAL,
                  "act_bwd_rows: bad arguments (cols, ldh %% 8; 16-byte alignment; act GELU | GELU_TANH)");
    const long n = rows * (cols / 8);
    if (act == 2) hipLaunchKernelGGL(act_bwd_rows_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint16_t*)da_bf16, (const _Float16*)h_f16, (long)ldh, (long)rows, cols / 8);
    else hipLaunchKernelGGL(act_bwd_rows_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint16_t*)da_bf16, (const _Float16*)h_f16, (long)ldh, (long)rows, cols / 8);
    return hicom_host::check_launch("act_bwd_rows");
}

extern "C" int hicom_colsum_fwd(const void* x_bf16, int64_t N, int32_t D, float* parts, int32_t nparts, void* stream) {
    HICOM_REQUIRE(x_bf16 && parts && N > 0 && nparts > 0 && (D == 1152 || D == 768), HICOM_EINVAL, "colsum: bad arguments (D 1152 / 768)");
    if (D == 1152) hipLaunchKernelGGL(colsum_kernel<3>, dim3((unsigned)nparts), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x_bf16, (long)N, parts);
    else hipLaunchKernelGGL(colsum_kernel<2>, dim3((unsigned)nparts), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x_bf16, (long)N, parts);
    return hicom_host::check_launch("colsum");
}

extern "C" int hicom_trilinear_pool_fwd(const void* x, int32_t T, int32_t H, int32_t W, int32_t D,
                                        int32_t To, int32_t Ho, int32_t Wo, float* out, void* stream) {
    HICOM_REQUIRE(x && out, HICOM_EINVAL, "trilinear_pool: NULL pointer");
    HICOM_REQUIRE(T > 0 && H > 0 && W > 0 && D > 0 && To > 0 && Ho > 0 && Wo > 0, HICOM_EINVAL, "trilinear_pool: bad shape");
    PoolParams p{(const uint16_t*)x, T, H, W, D, To, Ho, Wo, out};
    hipLaunchKernelGGL(trilinear_pool_kernel, dim3((unsigned)((long)To * Ho * Wo)), dim3(256), 0, (hipStream_t)stream, p);
    return hicom_host::check_launch("trilinear_pool");
}
