// Local logits of Q guides straight from the SigLIP head's hidden layer.
//
// The local stage of the release recipe reads frames_embed = x + fc2(hid) + b2, hid = act(fc1(LN x)), only through the dot products
// g_q . frames_embed[n].  Those are linear in frames_embed:
//     g_q . frames_embed[n] = g_q . x[n]  +  U[q] . hid[n]  +  c[q],        U[q] = W2^T g_q  (inter values),   c[q] = g_q . b2
// so for Q guides the second head GEMM (M x inter x D) becomes one skinny product of [M, D] and [M, inter] against Q vectors each, and
// frames_embed is never formed.
//
//   hicom_head_guide_fold_fwd     U and c of every guide (two small launches): U in fp32 from the bf16 weight, then split into an fp16 hi + lo
//                                 pair at a power of two per row, 2^s with max_k |U[q, k]| 2^s in [2^14, 2^15) -- the rule fused_ring.hip states at
//                                 split_f16: a plain split of small values puts lo among the fp16 subnormals.  |U 2^s - hi - lo| <= 2^-22 max|U 2^s|.
//   hicom_head_scores_multi_fwd   logits[q][n] for all guides from ONE pass over x and hid: 2 (D + kpad) bytes per token whatever Q is.
// For a batch (B items stacked, item i with its own Q_i guides):
//   hicom_head_guide_fold_many_fwd   the fold for M = sum Q_i guide rows in the same two launches, every row bit for bit the single form's
//   hicom_head_scores_ragged_fwd     the scores kernel's tile body, one workgroup per tile of ONE item: item i's tokens meet item i's guides only
//
// The scores kernel.  A workgroup owns kHsTok = 32 tokens and the whole contraction; its four waves split the contraction into blocks of
// 128 channels (256-byte row segments, first those of x, then those of hid), block b going to wave b mod 4.  A wave stages its block by
// LDS-DMA (global_load_lds_dwordx4: 1 KiB = four row segments per instruction) into its OWN double buffer with the chunk ^ rot(row) swizzle
// of global_stream.hip, so the K loop has no workgroup barrier: the wave drains its own vmcnt, issues the next block's operand loads and
// DMA, and multiplies the block that has landed.  Rows of the MFMA are guides (16 per row group, one or two groups), columns are tokens:
//     x blocks    v_mfma_f32_16x16x32_bf16, A = the guides (exact bf16)
//     hid blocks  v_mfma_f32_16x16x32_f16,  A = U hi, then U lo, into an accumulator of their own that is scaled by 2^-s at the end
// A fragments come from global memory (L2: the guide planes are < 1 MiB), fetched one block ahead of their use.  The four waves' partial
// tiles are summed through LDS (the staging buffers, all DMA drained) and stored token-contiguous into logits[q][.]; rows >= Q and
// tokens >= M are never stored.  Tail tokens re-read row M - 1; a last block of hid that is only half inside kpad re-reads the 64 channels
// in front of it against zero columns of U.  The pitch gap of hid (ld > kpad) is never read.
#include "common.hpp"
#include "segment_host.hpp"

namespace hicom {

typedef _Float16 hs_f16x8 __attribute__((ext_vector_type(8)));

constexpr int kHsTok = 32;                  // tokens of one workgroup
constexpr int kHsBuf = kHsTok * 256;        // one staged block: 32 row segments of 256 bytes
constexpr int kFoldSlices = 16;             // slices of D in the fold's first launch
constexpr int kFoldDper = 128;              // channels per slice at most (D <= 2048)

// the 16-byte-chunk swizzle of global_stream.hip (bit rotation of the row index, bijective on 0..15)
__device__ __forceinline__ int hs_swz(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }

struct HeadScoresParams {
    const uint16_t* x;          // bf16 [M][D]
    const uint16_t* hid;        // fp16 [M][ld], columns [0, kpad) read
    long ld, M;
    int D, kpad, nbx, nbh;      // blocks of 128 channels of x and of hid
    const uint16_t* g;          // bf16 [Q][D]
    const uint16_t* uhi;        // fp16 [16 NRG][ldu]: U 2^s, zero from column inter on and in rows >= Q
    const uint16_t* ulo;
    long ldu;
    const float* usc;           // [16 NRG] 2^-s
    const float* c;             // [16 NRG]
    int Q;
    float* logits;              // [Q][q_stride]
    long q_stride;
};

// One tile of kHsTok tokens, the body of both kernels.  tok0: the tile's first token; tok_end: the end of the token range the tile belongs
// to (tokens >= tok_end re-read row tok_end - 1 and are never stored); row0: the tile's first row of the guide matrix, of the U planes and of
// u_scale / c; nrows: its live guide rows (rows >= nrows are never stored; their x fragments are zero, their U fragments whatever the planes
// hold behind them: a row of A only reaches its own row of C); logits: guide row r of the tile goes to logits[r q_stride + token].
template <int NRG>
__device__ __forceinline__ void head_scores_tile(const HeadScoresParams& p, char* smem, const long tok0, const long tok_end, const int row0, const int nrows,
                                                 float* logits) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kg = lane >> 4;
    char* mybuf = smem + wave * 2 * kHsBuf;
    const int nblk = p.nbx + p.nbh;

    f32x4 accx[NRG][2], acch[NRG][2];
#pragma unroll
    for (int rg = 0; rg < NRG; ++rg)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            accx[rg][s] = f32x4{0.f, 0.f, 0.f, 0.f};
            acch[rg][s] = f32x4{0.f, 0.f, 0.f, 0.f};
        }

    // ---- LDS-DMA of block b: 8 pieces of four 256-byte row segments ----------------------------------------------------------------------
    auto stage = [&](int b, int buf) {
        const bool is_h = b >= p.nbx;
        const int bb = is_h ? b - p.nbx : b;
        const char* base = reinterpret_cast<const char*>(is_h ? p.hid : p.x);
        const long pitch = (is_h ? p.ld : (long)p.D) * 2;
        const int width = is_h ? p.kpad : p.D;
        const int r = lane >> 4, cpos = lane & 15;
#pragma unroll
        for (int pi = 0; pi < kHsTok / 4; ++pi) {
            const int row = 4 * pi + r;
            long tok = tok0 + row;
            tok = tok < tok_end ? tok : tok_end - 1;                        // tail tokens: a valid row again (never stored)
            int col = bb * 128 + 8 * (cpos ^ hs_swz(row & 15));
            col = col < width ? col : col - 64;                             // half a block behind kpad: U is zero there
            const char* src = base + tok * pitch + (long)col * 2;
            char* dst = mybuf + buf * kHsBuf + pi * 1024;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src), (__attribute__((address_space(3))) void*)(dst), 16, 0,
                                             0);
        }
    };

    // ---- A fragments of block b: guide rows 16 rg + r16, channels 32 ks + 8 kg .. + 7 of the block ----------------------------------------------
    // (an x block has no lo part: its fragments are zero and never multiplied)
    bf16x8 nhi[NRG][4], nlo[NRG][4];
    auto load_a = [&](int b) {
        const bool is_h = b >= p.nbx;
#pragma unroll
        for (int rg = 0; rg < NRG; ++rg) {
            const int row = 16 * rg + r16;
            const bool on = is_h || row < nrows;
            const uint16_t* hi = is_h ? p.uhi + (long)(row0 + row) * p.ldu + (b - p.nbx) * 128 + 8 * kg
                                      : p.g + (long)(row0 + (on ? row : 0)) * p.D + b * 128 + 8 * kg;
            const uint16_t* lo = is_h ? p.ulo + (long)(row0 + row) * p.ldu + (b - p.nbx) * 128 + 8 * kg : hi;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 vh = *reinterpret_cast<const bf16x8*>(hi + 32 * ks);
                const bf16x8 vl = *reinterpret_cast<const bf16x8*>(lo + 32 * ks);
                const bf16x8 zero = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                nhi[rg][ks] = on ? vh : zero;
                nlo[rg][ks] = is_h ? vl : zero;
            }
        }
    };

    int b = wave;
    if (b < nblk) {
        load_a(b);
        stage(b, 0);
    }
    for (int it = 0; b < nblk; b += 4, ++it) {
        // this wave's DMA of block b and its A fragments have landed (the buffers are the wave's own: no barrier)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bf16x8 ahi[NRG][4], alo[NRG][4];
#pragma unroll
        for (int rg = 0; rg < NRG; ++rg)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                ahi[rg][ks] = nhi[rg][ks];
                alo[rg][ks] = nlo[rg][ks];
            }
        if (b + 4 < nblk) {
            load_a(b + 4);
            stage(b + 4, (it + 1) & 1);
        }
        const char* img = mybuf + (it & 1) * kHsBuf;
        const bool is_h = b >= p.nbx;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 t = *reinterpret_cast<const bf16x8*>(img + (16 * s + r16) * 256 + 16 * ((4 * ks + kg) ^ hs_swz(r16)));
#pragma unroll
                for (int rg = 0; rg < NRG; ++rg) {
                    if (!is_h) {
                        accx[rg][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi[rg][ks], t, accx[rg][s], 0, 0, 0);
                    } else {
                        const hs_f16x8 th = __builtin_bit_cast(hs_f16x8, t);
                        acch[rg][s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(hs_f16x8, ahi[rg][ks]), th, acch[rg][s], 0, 0, 0);
                        acch[rg][s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(hs_f16x8, alo[rg][ks]), th, acch[rg][s], 0, 0, 0);
                    }
                }
            }
    }

    // ---- the four waves' partial tiles: C layout = guide rows 4 kg + j of token column r16 --------------------------------------------------
    // (every wave's DMA is drained: its last pass waited for vmcnt(0) and staged nothing; a wave's own LDS reads and writes stay in order)
    float* red = reinterpret_cast<float*>(mybuf);                           // [16 NRG guides][32 tokens]
#pragma unroll
    for (int rg = 0; rg < NRG; ++rg)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = 16 * rg + 4 * kg + j;
            const float sc = p.usc[row0 + row];
#pragma unroll
            for (int s = 0; s < 2; ++s) red[row * kHsTok + 16 * s + r16] = accx[rg][s][j] + acch[rg][s][j] * sc;
        }
    __syncthreads();
    for (int e = tid; e < NRG * 16 * kHsTok; e += 256) {
        const int row = e / kHsTok, t = e % kHsTok;
        float v = p.c[row0 + row];
#pragma unroll
        for (int w = 0; w < 4; ++w) v += reinterpret_cast<const float*>(smem + w * 2 * kHsBuf)[e];
        if (row < nrows && tok0 + t < tok_end) logits[(long)row * p.q_stride + tok0 + t] = v;
    }
}

template <int NRG>
__global__ __launch_bounds__(256, 2) void head_scores_multi_kernel(HeadScoresParams p) {
    __shared__ __attribute__((aligned(16))) char smem[4 * 2 * kHsBuf];      // [wave][2][32 rows][256 B] = 64 KiB
    head_scores_tile<NRG>(p, smem, (long)blockIdx.x * kHsTok, p.M, 0, p.Q, p.logits);
}

// ---- the segmented form: B items stacked, item i's tokens against item i's guides only ---------------------------------------
// A workgroup is one tile of ONE item: tiles are counted per item (ceil(N_i / 32) each, tile_item[blockIdx.x] names the item as win_item
// does for rmg_local_kernel), so a tile never crosses into the next item and with B = 1 the tiling is head_scores_multi_kernel's.  The
// item's guides are rows [pair0, pair0 + Q) of the guide matrix and of the planes; rows behind them in the tile belong to the next items (or
// to the planes' zero pad) and are never stored.  Guide q of the item goes to logits[q q_stride + tok0 + n].  The lookups are
// workgroup-uniform.
struct HsItem {          // 8 ints; mirrored by hicom_amd/encoder.py: ragged_score_tables
    int tok0, N;         // first token in the stack, tokens
    int pair0, Q;        // first guide row, guides
    int tile0;           // first tile
    int pad0, pad1, pad2;
};
static_assert(sizeof(HsItem) == 32, "item rows are 8 ints");

template <int NRG>
__global__ __launch_bounds__(256, 2) void head_scores_ragged_kernel(HeadScoresParams p, const HsItem* items, const int* tile_item) {
    __shared__ __attribute__((aligned(16))) char smem[4 * 2 * kHsBuf];
    const HsItem it = items[tile_item[blockIdx.x]];
    const long tok0 = (long)it.tok0 + (long)((int)blockIdx.x - it.tile0) * kHsTok;
    head_scores_tile<NRG>(p, smem, tok0, (long)it.tok0 + it.N, it.pair0, it.Q, p.logits);
}

// ---- U = W2^T g and c = g . b2 ---------------------------------------------------------------------------------------------------------------
// First launch: grid (inter / 256, kFoldSlices); thread k of slice s sums w2[d][k] g[q][d] over the slice's channels for all guides
// (the slice of every guide in LDS as fp32, zero rows behind Q: 32 FMAs per weight whatever Q is).  part f32 [slices][Q][ldu].
// More than 32 guide rows (hicom_head_guide_fold_many_fwd): grid z walks blocks of 32 rows, block z the rows [32 z, 32 z + 32) of g and of
// part; a row's arithmetic does not depend on the block it is in.
__global__ __launch_bounds__(256) void head_fold_partial_kernel(const uint16_t* w2, int D, int inter, const uint16_t* g, int Q, long ldu, float* part) {
    __shared__ float gs[32][kFoldDper];
    const int tid = threadIdx.x, slice = blockIdx.y;
    const int q0 = 32 * blockIdx.z;
    const int dper = (D + kFoldSlices - 1) / kFoldSlices;
    const int d0 = slice * dper, d1 = min(D, d0 + dper);
    for (int i = tid; i < 32 * dper; i += 256) {
        const int q = i / dper, dd = i - q * dper;
        gs[q][dd] = (q0 + q < Q && d0 + dd < d1) ? bf16_to_f32(g[(long)(q0 + q) * D + d0 + dd]) : 0.f;
    }
    __syncthreads();
    const int k = blockIdx.x * 256 + tid;
    if (k >= inter) return;
    float acc[32];
#pragma unroll
    for (int q = 0; q < 32; ++q) acc[q] = 0.f;
    for (int d = d0; d < d1; ++d) {
        const float w = bf16_to_f32(w2[(long)d * inter + k]);
#pragma unroll
        for (int q = 0; q < 32; ++q) acc[q] = fmaf(w, gs[q][d - d0], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < 32; ++q)
        if (q0 + q < Q) part[((long)slice * Q + q0 + q) * ldu + k] = acc[q];
}

// Second launch: one workgroup per padded guide row.  Slices are added in slice order; the row's power of two; hi / lo planes with zeros
// from column inter on; rows >= Q all zero with scale 1 and c = 0.
__global__ __launch_bounds__(256) void head_fold_finish_kernel(const float* part, int D, int inter, const uint16_t* g, const uint16_t* b2, int Q, long ldu,
                                                               _Float16* uhi, _Float16* ulo, float* usc, float* c) {
    __shared__ float wred[4];
    const int tid = threadIdx.x, q = blockIdx.x;
    _Float16* hi = uhi + (long)q * ldu;
    _Float16* lo = ulo + (long)q * ldu;
    if (q >= Q) {
        for (long k = tid; k < ldu; k += 256) {
            hi[k] = (_Float16)0.f;
            lo[k] = (_Float16)0.f;
        }
        if (tid == 0) {
            usc[q] = 1.f;
            c[q] = 0.f;
        }
        return;
    }
    auto u_of = [&](int k) {
        float v = 0.f;
        for (int s = 0; s < kFoldSlices; ++s) v += part[((long)s * Q + q) * ldu + k];
        return v;
    };
    float mx = 0.f, dot = 0.f;
    for (int k = tid; k < inter; k += 256) mx = fmaxf(mx, fabsf(u_of(k)));
    if (b2)
        for (int d = tid; d < D; d += 256) dot = fmaf(bf16_to_f32(g[(long)q * D + d]), bf16_to_f32(b2[d]), dot);
    mx = wave_max(mx);
    if ((tid & 63) == 0) wred[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
    __syncthreads();
    dot = wave_sum(dot);
    if ((tid & 63) == 0) wred[tid >> 6] = dot;
    __syncthreads();
    int ex = 0;
    (void)frexpf(mx, &ex);                                                  // mx = m 2^ex, m in [0.5, 1)
    ex = min(max(ex, -100), 100);
    const float up = (mx > 0.f && mx < 3.0e38f) ? ldexpf(1.f, 15 - ex) : 1.f;
    for (long k = tid; k < ldu; k += 256) {
        const float v = k < inter ? fminf(fmaxf(u_of((int)k) * up, -65504.f), 65504.f) : 0.f;
        const _Float16 h = (_Float16)v;
        hi[k] = h;
        lo[k] = (_Float16)(v - (float)h);
    }
    if (tid == 0) {
        usc[q] = 1.f / up;
        c[q] = (wred[0] + wred[1]) + (wred[2] + wred[3]);
    }
}

}  // namespace hicom

using namespace hicom;

namespace {

// the two launches of the fold over Q guide rows: the partial kernel over blocks of 32 rows, the finish kernel over `rows` plane rows
// (rows >= Q: zero, scale 1, c = 0).  The checks of both entry points but the bound on Q.
int fold_launch(const char* who, const void* w2, const void* b2, int D, int inter, const void* guides, int Q, int rows, void* u_hi, void* u_lo, int64_t ldu,
                float* u_scale, float* c, void* ws, int64_t ws_bytes, void* stream) {
    HICOM_REQUIRE(D > 0 && D <= kFoldSlices * kFoldDper && inter > 0, HICOM_EUNSUP, "%s: D=%d (<= %d), inter=%d", who, D, kFoldSlices * kFoldDper, inter);
    HICOM_REQUIRE(ldu >= inter && ldu % 8 == 0, HICOM_EINVAL, "%s: ldu=%ld (>= inter = %d, a multiple of 8)", who, (long)ldu, inter);
    HICOM_REQUIRE(ws_bytes >= (int64_t)kFoldSlices * Q * ldu * 4 && (uintptr_t)ws % 4 == 0, HICOM_EINVAL, "%s: workspace of %ld bytes", who,
                  (long)kFoldSlices * Q * ldu * 4);
    HICOM_REQUIRE((uintptr_t)u_hi % 16 == 0 && (uintptr_t)u_lo % 16 == 0, HICOM_EINVAL, "%s: 16-byte aligned planes", who);
    HICOM_LAUNCH(head_fold_partial_kernel, dim3((unsigned)((inter + 255) / 256), kFoldSlices, (unsigned)((Q + 31) / 32)), dim3(256), 0, (hipStream_t)stream,
                 (const uint16_t*)w2, D, inter, (const uint16_t*)guides, Q, (long)ldu, (float*)ws);
    int st = hicom_host::check_launch("head_guide_fold (partials)");
    if (st != HICOM_OK) return st;
    HICOM_LAUNCH(head_fold_finish_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, (const float*)ws, D, inter, (const uint16_t*)guides,
                 (const uint16_t*)b2, Q, (long)ldu, (_Float16*)u_hi, (_Float16*)u_lo, u_scale, c);
    return hicom_host::check_launch("head_guide_fold");
}

// the operand rules both scores entry points share; nbh: blocks of 128 hidden channels
int scores_check(const char* who, const void* x, const void* hid, int64_t ld, int D, int kpad, const void* guides, const void* u_hi, const void* u_lo,
                 int64_t ldu, const float* logits, int& nbh) {
    HICOM_REQUIRE(D > 0 && D % 128 == 0, HICOM_EUNSUP, "%s: D=%d (a multiple of 128)", who, D);
    HICOM_REQUIRE(kpad >= 64 && kpad % 64 == 0 && ld >= kpad && ld % 8 == 0, HICOM_EINVAL, "%s: kpad=%d (a multiple of 64), ld=%ld (>= kpad, a multiple of 8)",
                  who, kpad, (long)ld);
    nbh = (kpad + 127) / 128;
    HICOM_REQUIRE(ldu >= (int64_t)nbh * 128 && ldu % 8 == 0, HICOM_EINVAL, "%s: ldu=%ld (>= kpad rounded up to 128, a multiple of 8)", who, (long)ldu);
    HICOM_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)hid % 16 == 0 && (uintptr_t)guides % 16 == 0 && (uintptr_t)u_hi % 16 == 0 && (uintptr_t)u_lo % 16 == 0 &&
                      (uintptr_t)logits % 4 == 0,
                  HICOM_EINVAL, "%s: 16-byte aligned operands", who);
    return HICOM_OK;
}

}  // namespace

extern "C" int hicom_head_guide_fold_fwd(const void* w2, const void* b2, int32_t D, int32_t inter, const void* guides, int32_t Q, void* u_hi, void* u_lo,
                                         int64_t ldu, float* u_scale, float* c, void* ws, int64_t ws_bytes, void* stream) {
    const char* who = "head_guide_fold";
    HICOM_REQUIRE(w2 && guides && u_hi && u_lo && u_scale && c && ws, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE(Q >= 1 && Q <= 32, HICOM_EUNSUP, "%s: Q=%d guides (1 <= Q <= 32 per call)", who, Q);
    return fold_launch(who, w2, b2, D, inter, guides, Q, (Q + 15) / 16 * 16, u_hi, u_lo, ldu, u_scale, c, ws, ws_bytes, stream);
}

// M = sum Q_i guide rows of a batch in the same two launches; the planes hold ceil16(M) + 32 rows, so a tile of
// head_scores_ragged_kernel that starts at the last item's first row stays inside them.
extern "C" int hicom_head_guide_fold_many_fwd(const void* w2, const void* b2, int32_t D, int32_t inter, const void* guides, int32_t M, void* u_hi, void* u_lo,
                                              int64_t ldu, float* u_scale, float* c, void* ws, int64_t ws_bytes, void* stream) {
    const char* who = "head_guide_fold_many";
    HICOM_REQUIRE(w2 && guides && u_hi && u_lo && u_scale && c && ws, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE(M >= 1 && M <= hicom_host::kSegMaxItems, HICOM_EUNSUP, "%s: M=%d guide rows (1 <= M <= %d per call)", who, M, hicom_host::kSegMaxItems);
    return fold_launch(who, w2, b2, D, inter, guides, M, (M + 15) / 16 * 16 + 32, u_hi, u_lo, ldu, u_scale, c, ws, ws_bytes, stream);
}

extern "C" int hicom_head_scores_multi_fwd(const void* x, const void* hid, int64_t ld, int64_t M, int32_t D, int32_t kpad, const void* guides,
                                           const void* u_hi, const void* u_lo, int64_t ldu, const float* u_scale, const float* c, int32_t Q, float* logits,
                                           int64_t q_stride, void* stream) {
    const char* who = "head_scores_multi";
    HICOM_REQUIRE(x && hid && guides && u_hi && u_lo && u_scale && c && logits, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE(Q >= 1 && Q <= 32, HICOM_EUNSUP, "%s: Q=%d guides (1 <= Q <= 32 per call)", who, Q);
    HICOM_REQUIRE(M > 0 && M < (1L << 31) - kHsTok, HICOM_EUNSUP, "%s: M=%ld tokens", who, (long)M);
    int nbh = 0;
    const int st = scores_check(who, x, hid, ld, D, kpad, guides, u_hi, u_lo, ldu, logits, nbh);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(Q == 1 || q_stride >= M, HICOM_EINVAL, "%s: q_stride=%ld floats between the guides' rows of %ld tokens", who, (long)q_stride, (long)M);
    HeadScoresParams p;
    p.x = (const uint16_t*)x; p.hid = (const uint16_t*)hid; p.ld = ld; p.M = M; p.D = D; p.kpad = kpad; p.nbx = D / 128; p.nbh = nbh;
    p.g = (const uint16_t*)guides; p.uhi = (const uint16_t*)u_hi; p.ulo = (const uint16_t*)u_lo; p.ldu = ldu; p.usc = u_scale; p.c = c; p.Q = Q;
    p.logits = logits; p.q_stride = q_stride;
    const dim3 grid((unsigned)((M + kHsTok - 1) / kHsTok));
    if (Q <= 16) HICOM_LAUNCH(head_scores_multi_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p);
    else HICOM_LAUNCH(head_scores_multi_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, p);
    return hicom_host::check_launch("head_scores_multi");
}

// items: DEVICE rows {tok0, N, pair0, Q, tile0, 0, 0, 0}; tile_item: DEVICE, the item of each of the ntiles = sum ceil(N_i / 32) tiles.
// The tables are the caller's (they depend on the token and guide counts only); what can be checked without reading them is checked here.
extern "C" int hicom_head_scores_ragged_fwd(const void* x, const void* hid, int64_t ld, int32_t D, int32_t kpad, const void* guides, const void* u_hi,
                                            const void* u_lo, int64_t ldu, const float* u_scale, const float* c, const int32_t* items,
                                            const int32_t* tile_item, int32_t B, int32_t ntiles, int32_t q_max, float* logits, int64_t q_stride, void* stream) {
    const char* who = "head_scores_ragged";
    HICOM_REQUIRE(x && hid && guides && u_hi && u_lo && u_scale && c && logits && items && tile_item, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE(B > 0 && B <= hicom_host::kSegMaxItems, HICOM_EUNSUP, "%s: B=%d items (1 <= B <= %d per call)", who, B, hicom_host::kSegMaxItems);
    HICOM_REQUIRE(q_max >= 1 && q_max <= 32, HICOM_EUNSUP, "%s: q_max=%d guides (1 <= Q_i <= 32 per item)", who, q_max);
    HICOM_REQUIRE(ntiles >= B && ntiles < (1 << 26), HICOM_EUNSUP, "%s: ntiles=%d tiles of 32 tokens for %d items (one per item at least, < 2^26)", who, ntiles,
                  B);
    int nbh = 0;
    const int st = scores_check(who, x, hid, ld, D, kpad, guides, u_hi, u_lo, ldu, logits, nbh);
    if (st != HICOM_OK) return st;
    // every item fills all its tiles but the last: sum N_i > 32 (ntiles - B)
    HICOM_REQUIRE(q_max == 1 || q_stride > (int64_t)kHsTok * (ntiles - B), HICOM_EINVAL,
                  "%s: q_stride=%ld floats between the guides' rows (>= sum N_i, which is above %ld for %d tiles of %d items)", who, (long)q_stride,
                  (long)kHsTok * (ntiles - B), ntiles, B);
    HICOM_REQUIRE((uintptr_t)items % 16 == 0 && (uintptr_t)tile_item % 4 == 0, HICOM_EINVAL, "%s: items is a 16-byte aligned device table [B][8]", who);
    HeadScoresParams p;
    p.x = (const uint16_t*)x; p.hid = (const uint16_t*)hid; p.ld = ld; p.M = 0; p.D = D; p.kpad = kpad; p.nbx = D / 128; p.nbh = nbh;
    p.g = (const uint16_t*)guides; p.uhi = (const uint16_t*)u_hi; p.ulo = (const uint16_t*)u_lo; p.ldu = ldu; p.usc = u_scale; p.c = c; p.Q = q_max;
    p.logits = logits; p.q_stride = q_stride;
    const dim3 grid((unsigned)ntiles);
    if (q_max <= 16) HICOM_LAUNCH(head_scores_ragged_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p, (const HsItem*)items, tile_item);
    else HICOM_LAUNCH(head_scores_ragged_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, p, (const HsItem*)items, tile_item);
    return hicom_host::check_launch("head_scores_ragged");
}
