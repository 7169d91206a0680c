// Dev probe: the group size of the adaptor window for several guides (csrc/multi_window.hpp: multi_window_guides_adapt_ctx16, DESIGN.md
// §3.10).  Times the window walk alone at Q guides on a T x 27 x 27 clip with windows 4 x 3 x 3 for
//   group 2, __launch_bounds__(256, 4)   128 registers: four waves per SIMD
//   group 2, __launch_bounds__(256, 3)   168 registers: three waves per SIMD
//   group 4, __launch_bounds__(256)      up to 512 registers: one wave per SIMD
//   group 3, __launch_bounds__(256, 2)   256 registers: two waves per SIMD
// and the plain window of the multi-guide step (group 4) beside them.  Random tokens and planes; median of 30 launches after 5.
// resource table:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -Rpass-analysis=kernel-resource-usage -c tools/scratch/adapt_group_ab.hip -o /dev/null
// build + run:     hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/scratch/adapt_group_ab.hip -o adapt_group_ab && ./adapt_group_ab [T] [Q]
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../hicom_amd/csrc/multi_window.hpp"

using namespace hicom;

template <int GROUP, int WAVES>
__global__ __launch_bounds__(256, WAVES) void adapt_probe(const uint16_t* key, const uint16_t* value, const uint16_t* guide, SegAdaptParams ad, hicom_axis at,
                                                          hicom_axis ay, hicom_axis ax, int Q, int nwin, float scale, _Float16* ctx16) {
    constexpr int D = 1152;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const WindowGeom g(at, ay, ax, win);
    multi_window_guides_adapt_ctx16<3, GROUP>(key, value, ad, guide, 0, Q, g, lane, scale, ctx16 + (long)win * D, (long)nwin * D);
}

__global__ __launch_bounds__(256) void plain_probe(const uint16_t* key, const uint16_t* value, const uint16_t* guide, hicom_axis at, hicom_axis ay,
                                                   hicom_axis ax, int Q, int nwin, float scale, _Float16* ctx16) {
    constexpr int D = 1152;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const WindowGeom g(at, ay, ax, win);
    multi_window_guides_ctx16<3>(key, value, guide, 0, Q, g, lane, scale, ctx16 + (long)win * D, (long)nwin * D);
}

#define CHECK(x)                                                                  \
    do {                                                                          \
        hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                   \
            printf("%s: %s\n", #x, hipGetErrorString(e_));                        \
            return 1;                                                             \
        }                                                                         \
    } while (0)

static uint16_t bf16_of(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (uint16_t)((u + 0x7FFF + ((u >> 16) & 1)) >> 16);
}

int main(int argc, char** argv) {
    const int T = argc > 1 ? atoi(argv[1]) : 64, Q = argc > 2 ? atoi(argv[2]) : 4, H = 27, W = 27, D = 1152, kt = 4, ks = 3;
    if (T < kt || T % kt || Q < 1 || Q > 32) {
        printf("usage: adapt_group_ab [T: multiple of 4] [Q: 1..32]\n");
        return 1;
    }
    const long N = (long)T * H * W;
    const int nwin = (T / kt) * (H / ks) * (W / ks);
    srand(1);
    auto rnd = [] { return (float)rand() / RAND_MAX * 2.f - 1.f; };
    std::vector<uint16_t> tok((size_t)N * D), small((size_t)(Q + 4) * D);
    std::vector<_Float16> y((size_t)N * D);
    for (auto& v : tok) v = bf16_of(rnd());
    for (auto& v : y) v = (_Float16)rnd();
    for (auto& v : small) v = bf16_of(rnd() * 0.5f);
    uint16_t *fe, *ff, *sm;
    _Float16 *ky, *vy, *ctx;
    CHECK(hipMalloc(&fe, N * D * 2));
    CHECK(hipMalloc(&ff, N * D * 2));
    CHECK(hipMalloc(&ky, N * D * 2));
    CHECK(hipMalloc(&vy, N * D * 2));
    CHECK(hipMalloc(&sm, small.size() * 2));
    CHECK(hipMalloc(&ctx, (size_t)Q * nwin * D * 2));
    CHECK(hipMemcpy(fe, tok.data(), N * D * 2, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(ff, tok.data(), N * D * 2, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(ky, y.data(), N * D * 2, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(vy, y.data(), N * D * 2, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(sm, small.data(), small.size() * 2, hipMemcpyHostToDevice));
    // guide rows 0 .. Q - 1, then gamma, beta (shared by both streams) and a bf16 alpha
    SegAdaptParams ad;
    ad.ky = ky; ad.vy = vy;
    ad.kgamma = ad.vgamma = sm + (long)Q * D;
    ad.kbeta = ad.vbeta = sm + (long)(Q + 1) * D;
    ad.kalpha = ad.valpha = sm + (long)(Q + 2) * D;
    ad.alpha_f32 = 0;
    ad.eps = 1e-5f;
    const hicom_axis at{T, kt, T / kt, T / kt}, ay{H, ks, H / ks, H / ks}, ax{W, ks, W / ks, W / ks};
    const dim3 grid((unsigned)((nwin + 3) / 4)), block(256);
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    auto time = [&](const char* name, auto&& launch) -> int {
        std::vector<float> ms;
        for (int i = 0; i < 35; ++i) {
            CHECK(hipEventRecord(e0));
            launch();
            CHECK(hipEventRecord(e1));
            CHECK(hipEventSynchronize(e1));
            CHECK(hipGetLastError());
            float t;
            CHECK(hipEventElapsedTime(&t, e0, e1));
            if (i >= 5) ms.push_back(t);
        }
        std::sort(ms.begin(), ms.end());
        printf("T=%d Q=%d %-28s median %.1f us  (min %.1f, max %.1f)\n", T, Q, name, ms[ms.size() / 2] * 1e3, ms.front() * 1e3, ms.back() * 1e3);
        return 0;
    };
    const float scale = 0.0294628f;
    if (time("adapt group 2, 4 waves/SIMD", [&] { hipLaunchKernelGGL((adapt_probe<2, 4>), grid, block, 0, 0, fe, ff, sm, ad, at, ay, ax, Q, nwin, scale, ctx); })) return 1;
    if (time("adapt group 2, 3 waves/SIMD", [&] { hipLaunchKernelGGL((adapt_probe<2, 3>), grid, block, 0, 0, fe, ff, sm, ad, at, ay, ax, Q, nwin, scale, ctx); })) return 1;
    if (time("adapt group 3, 2 waves/SIMD", [&] { hipLaunchKernelGGL((adapt_probe<3, 2>), grid, block, 0, 0, fe, ff, sm, ad, at, ay, ax, Q, nwin, scale, ctx); })) return 1;
    if (time("adapt group 4, 1 wave/SIMD", [&] { hipLaunchKernelGGL((adapt_probe<4, 1>), grid, block, 0, 0, fe, ff, sm, ad, at, ay, ax, Q, nwin, scale, ctx); })) return 1;
    if (time("plain group 4", [&] { hipLaunchKernelGGL(plain_probe, grid, block, 0, 0, fe, ff, sm, at, ay, ax, Q, nwin, scale, ctx); })) return 1;
    return 0;
}
