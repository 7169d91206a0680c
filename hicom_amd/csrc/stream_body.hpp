// The four-wave global token stream: the ONE device text of the machine behind every narrow and segmented stream kernel.
//     S[r, n]   = qt[r, :] . x[n, :]  (+ separable positional terms a_t + a_y + a_x)
//     ACC[r, :] = sum_n exp(S[r, n] - m_r) x[n, :]          (online softmax, fp32)
// over the RAW bf16 tokens (K = V = x; k_proj / v_proj are folded into the queries in front), never materialising K, V or x + pos.
// Who calls it: global_stream_kernel (global_stream.hip: hicom_global_stream_fwd / _clip_fwd / _bwd when the wide form does not
// apply; tile range and row group from blockIdx) and the segmented kernels of the many-item steps (batch.hip, ragged.hip,
// clip_stream_group.hip: one row group; ragged_multi_guide.hip, clip_stream_group_multi.hip: two), which hand it one item's tokens,
// tile range and rows.  A row's result does not depend on which of them streamed it: there is no second copy to keep equal.
// (global_stream_wide_kernel, global_stream.hip, is a different machine -- three-tile ring, de-duplicated softmax -- and shares only
// the swizzle pair below.)
//
// CDNA4 mapping
//   * row group = 4 waves, 2 workgroups per CU (80 KiB LDS, <=256 VGPR each); a workgroup walks
//     a contiguous range of 16-token tiles with running (m, l, ACC) in registers.
//   * tile staging: global_load_lds_dwordx4 (LDS-DMA, 1 KiB per wave instruction, whole 256-B
//     row segments) into a double-buffered [E/128][16 rows][256 B] image with the
//     chunk ^ rot(row) swizzle, so that BOTH the row read (ds_read_b128: B operand of the
//     score MFMA) and the transposed read (ds_read_b64_tr_b16: B operand of the P.x MFMA)
//     of the same image are bank-conflict free / 2-way.
//   * scores: v_mfma_f32_16x16x32_bf16, A = folded queries as bf16 hi + lo pairs (two MFMAs
//     into one accumulator -> fp32-grade logits), each wave contracts its own E/4 channel
//     slice and the four partial 16x16 tiles are summed through LDS.
//   * softmax fused at wavefront level: lane (row, token-quad) owns 4 logits, row max / row sum
//     are two cross-lane shuffles; P is split hi/lo and is already in A-fragment order.
//   * P.x: v_mfma_f32_16x16x16_bf16, each wave owns E/4 output channels (72 accumulator VGPRs).
#pragma once
#include "common.hpp"

namespace hicom {

struct SegStreamParams {
    const uint16_t* qhi;    // [items * rows][E] folded queries, item-major
    const uint16_t* qlo;
    const float* pos_a;     // [items * rows][pos_stride]
    int pos_stride;
    int rows;               // folded rows per item and guide (heads), <= 16
    int H, W, HW;
    int t0i, y0i, x0i;
    float* part_m;          // [slots][16]
    float* part_l;
    float* part_acc;        // [slots][16][E]
};

// What the body does with a tile's logits.  Everything that tells the modes apart is `if constexpr`: StreamMode::Fwd is the text
// without any of it.
//   FwdClip (projector.py:184-191): logit = (qt . x + pos + row_const[r]) * inv_norm[n].
//   Bwd: attention backward over the same stream (reference autograd through projector.py:197-215): the "queries" are the upstream
//     gradients dctx_r of the per-head contexts, so the MFMA score tile is dP[r, n] = dctx_r . (x_n + pos_n); with the forward's
//     logits S and softmax state (M, L) the lane forms
//         dS[r, n] = exp(S[r, n] - M_r) / L_r * (dP[r, n] - delta_r),      delta_r = dctx_r . ctx_r
//     writes it to `scores` (the positional marginals are taken from it afterwards) and accumulates
//         ACC[r, :] += dS[r, n] x[n, :]        ( = the x part of d q~_r )
//     through the same hi/lo P.x MFMAs.  No running max: the state is known; part_m / part_l are not written.
enum class StreamMode { Fwd, FwdClip, Bwd };

// Mode inputs, indexed like `scores`: by the row in the item's row space.  Fwd reads none of them.
struct StreamModeArgs {
    const float* inv_norm;  // FwdClip: [N] per-token key norms
    const float* row_const; // FwdClip: [nrows]
    const float* s_in;      // Bwd: [nrows][score_stride] raw logits S the forward pass wrote
    const float* ml;        // Bwd: [nrows][2] (M, L) of the forward softmax
    const float* delta;     // Bwd: [nrows] dctx_r . ctx_r
};

// bit rotation of the row index used as the 16-byte-chunk swizzle (bijective on 0..15)
__device__ __forceinline__ int swz(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }
// token-quad permutation: MFMA k-group g <-> tile rows 4*sig(g)..4*sig(g)+3, so that the two
// 4-row blocks a 32-lane half reads with ds_read_b64_tr_b16 sit 8 rows apart (conflict-free)
__device__ __forceinline__ int sig(int g) { return ((g & 1) << 1) | (g >> 1); }

// One body for one or two ROW GROUPS of 16 folded rows: a workgroup of 64 * 4 * GROUPS threads in which waves 4 g .. 4 g + 3 are the
// four-wave machine of group g, all groups on ONE double-buffered LDS tile (staged once per workgroup, its 1 KB pieces dealt round-robin
// to all waves), so an item's tokens come from HBM once per 16 * GROUPS rows.  Each group has its own exchange area, online softmax and
// accumulators, in the same operations and the same order per row: a row's result does not depend on GROUPS, on its group, on the
// other rows of the workgroup or on how many of them are live.  A group without a live row (rows >= nrows) stages and keeps the
// barriers only.  GROUPS == 1 (row0 a multiple of 16 chosen by the caller, gslots = 0): the group index and everything derived
// from it are compile-time zero and the guards fold away.
// xi: the item's N tokens [N][E]; [tb, te): the 16-token tiles to walk, counted from xi; row0: the workgroup's first row in the item's
// row space, nrows: the item's rows (rows >= nrows are masked: zero queries, nothing stored); qrow0: the item's first row in the query
// planes; scores: the item's [nrows][score_stride] logits (Bwd: dS); slot: where group 0's partial state (m, l, ACC) goes, group g
// `g * gslots` slots further.  Token indices are int: a caller must not pass N > 2^31 - 1 (the last tile's index 16 tile + 15 is then
// still an int).  Everything but the lane-dependent parts must be wave-uniform.
template <int NB, int GROUPS, StreamMode MODE = StreamMode::Fwd>
__device__ __forceinline__ void stream_segment(const SegStreamParams& p, const uint16_t* xi, int N, int tb, int te, int row0, int nrows, long qrow0,
                                               float* scores, long score_stride, long slot, int gslots, const StreamModeArgs& ma = StreamModeArgs{}) {
    constexpr int E = NB * 128;
    constexpr int SLICE = E / 4;          // channels owned by one wave
    constexpr int KSTEPS = SLICE / 32;    // score MFMAs (K = 32 channels) per wave per pass
    constexpr int CBLK = SLICE / 16;      // 16-channel output blocks per wave
    constexpr int TILE_BYTES = NB * 4096;
    constexpr int PIECES = NB * 4;        // 1 KiB LDS-DMA pieces per tile
    constexpr int WAVES = 4 * GROUPS;
    constexpr bool BWD = MODE == StreamMode::Bwd, CLIP = MODE == StreamMode::FwdClip;
    static_assert(GROUPS == 1 || GROUPS == 2, "one or two row groups");
    static_assert(GROUPS != 1 || PIECES % 4 == 0, "pieces are dealt round-robin to the 4 waves");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* tilebuf = smem;                                           // [2][TILE_BYTES]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave_wg = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = GROUPS == 1 ? 0 : wave_wg >> 2;                 // row group
    const int wave = GROUPS == 1 ? wave_wg : wave_wg & 3;           // the wave inside its four-wave machine
    float* red = reinterpret_cast<float*>(smem + 2 * TILE_BYTES) + grp * 1024;   // per group: [4 waves][16 rows][16 tokens]
    const int r16 = lane & 15, kg = lane >> 4;
    const int grow0 = row0 + 16 * grp;                              // the group's first row in the item's row space
    const bool grp_on = GROUPS == 1 || grow0 < nrows;               // (wave-uniform)
    const bool row_ok = grow0 + r16 < nrows;
    const long qrow = qrow0 + grow0 + r16;

    // ---- A operand: the group's folded queries (rows >= nrows: zero), this wave's channel slice, hi and lo parts ----
    bf16x8 ahi[KSTEPS], alo[KSTEPS];
    {
        const long off = qrow * E + SLICE * wave + 8 * kg;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            ahi[s] = row_ok ? *reinterpret_cast<const bf16x8*>(p.qhi + off + 32 * s) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            alo[s] = row_ok ? *reinterpret_cast<const bf16x8*>(p.qlo + off + 32 * s) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
    }

    f32x4 acc[CBLK];
#pragma unroll
    for (int cb = 0; cb < CBLK; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -1.0e30f, l_run = 0.f;   // online-softmax state of row r16 (replicated over kg, waves)

    // ---- LDS-DMA staging of one 16-token tile ----
    auto stage = [&](int tile, int buf) {
        const int r = lane >> 4, cpos = lane & 15;
#pragma unroll
        for (int i = 0; i < (PIECES + WAVES - 1) / WAVES; ++i) {
            const int pi = wave_wg + WAVES * i;
            if (PIECES % WAVES == 0 || pi < PIECES) {               // (wave-uniform; two groups: 36 pieces, waves 0-3 issue five, waves 4-7 four)
                const int blk = pi >> 2, row = 4 * (pi & 3) + r;
                int tok = tile * 16 + row;
                tok = tok < N ? tok : N - 1;   // tail tile: the item's own last token again (masked below), never a neighbour's
                const char* src = reinterpret_cast<const char*>(xi) + (long)tok * (E * 2) + blk * 256 + 16 * (cpos ^ swz(row));
                char* dst = tilebuf + buf * TILE_BYTES + pi * 1024;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src),
                                                 (__attribute__((address_space(3))) void*)(dst), 16, 0, 0);
            }
        }
    };

    // per-lane LDS byte offsets inside a tile image
    const int q4 = (lane >> 2) & 3, pp = lane & 3;
    const int trow = 4 * sig(kg) + q4;                // row this lane addresses in transposed reads
    const int rd_row_off = r16 * 256, rd_swz = swz(r16);
    const int tr_row_off = trow * 256 + 8 * (pp & 1), tr_swz = swz(trow);
    const float* pa = (p.pos_a && row_ok) ? p.pos_a + qrow * p.pos_stride : nullptr;

    // positional logit terms are fetched ONE TILE AHEAD: vmcnt retires in order, so consuming an ordinary load issued after the
    // LDS-DMA of the next tile would drain that prefetch.  The token index is item-local: t restarts at 0 per item
    float pt[4] = {0.f, 0.f, 0.f, 0.f}, py[4] = {0.f, 0.f, 0.f, 0.f}, px[4] = {0.f, 0.f, 0.f, 0.f};
    auto fetch_pos = [&](int tile) {
        if (pa) {
            const int nb = tile * 16 + 4 * sig(kg);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int n = nb + j;
                n = n < N ? n : N - 1;
                const unsigned un = (unsigned)n;
                const unsigned t = un / (unsigned)p.HW, rem = un - t * (unsigned)p.HW;
                const unsigned y = rem / (unsigned)p.W, xx = rem - y * (unsigned)p.W;
                pt[j] = pa[p.t0i + t];
                py[j] = pa[p.y0i + y];
                px[j] = pa[p.x0i + xx];
            }
        }
    };

    // FwdClip: the key norms, Bwd: the forward's logits, of (row r16, tokens 4*sig(kg)..+3), one tile ahead like the positional terms
    // (tail tile: clamped, masked later)
    f32x4 s_next = f32x4{0.f, 0.f, 0.f, 0.f};
    float crow = 0.f, bw_m = 0.f, bw_linv = 0.f, bw_delta = 0.f;
    auto fetch_s = [&](int tile) {
        if constexpr (BWD) {
            if (row_ok) s_next = *reinterpret_cast<const f32x4*>(ma.s_in + (long)(grow0 + r16) * score_stride + tile * 16 + 4 * sig(kg));
        } else if constexpr (CLIP) {
            const int nb = tile * 16 + 4 * sig(kg);
#pragma unroll
            for (int j = 0; j < 4; ++j) s_next[j] = ma.inv_norm[nb + j < N ? nb + j : N - 1];
        }
    };
    if constexpr (CLIP) {
        if (row_ok) crow = ma.row_const[grow0 + r16];
    }
    if constexpr (BWD) {
        if (row_ok) {
            bw_m = ma.ml[2 * (grow0 + r16)];
            bw_linv = 1.0f / ma.ml[2 * (grow0 + r16) + 1];
            bw_delta = ma.delta[grow0 + r16];
        }
    }

    if (tb < te) {
        fetch_pos(tb);
        fetch_s(tb);
        stage(tb, 0);
    }

    for (int tile = tb; tile < te; ++tile) {
        const int cur = (tile - tb) & 1;
        // [A] every wave's LDS-DMA pieces of tile `tile` have landed (explicit drain: hipcc does not order LDS-DMA against the barrier
        //     by itself), and every wave is done reading the other buffer and the reduction scratch
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        float padd[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) padd[j] = pt[j] + py[j] + px[j];
        const f32x4 s_cur = s_next;
        if (tile + 1 < te) {
            fetch_pos(tile + 1);
            fetch_s(tile + 1);
            stage(tile + 1, cur ^ 1);
        }
        const char* img = tilebuf + cur * TILE_BYTES;

        // ---- partial scores over this wave's channel slice: S = qt_hi.x^T + qt_lo.x^T ----
        if (grp_on) {
            f32x4 s4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s) {
                const int ch0 = SLICE * wave + 32 * s;
                const int blk = ch0 >> 7, cbase = (ch0 & 127) >> 3;
                const bf16x8 b = *reinterpret_cast<const bf16x8*>(img + blk * 4096 + rd_row_off + 16 * ((cbase + kg) ^ rd_swz));
                s4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi[s], b, s4, 0, 0, 0);
                s4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo[s], b, s4, 0, 0, 0);
            }
            // C layout: lane holds rows 4*kg + j (j = 0..3) of token column r16
            float* rw = red + wave * 256;
#pragma unroll
            for (int j = 0; j < 4; ++j) rw[(4 * kg + j) * 16 + r16] = s4[j];
        }
        lds_barrier();   // [B] LDS only: the next tile's LDS-DMA stays in flight
        if (!grp_on) continue;                                      // (wave-uniform; both barriers of the tile are behind this wave)

        // ---- full logits of (row r16, tokens 4*sig(kg) .. +3) ----
        const float* rb = red + r16 * 16 + 4 * sig(kg);
        f32x4 lg = *reinterpret_cast<const f32x4*>(rb);
        lg += *reinterpret_cast<const f32x4*>(rb + 256);
        lg += *reinterpret_cast<const f32x4*>(rb + 512);
        lg += *reinterpret_cast<const f32x4*>(rb + 768);
        const int n0 = tile * 16 + 4 * sig(kg);
#pragma unroll
        for (int j = 0; j < 4; ++j) lg[j] += padd[j];
        if constexpr (CLIP) {
#pragma unroll
            for (int j = 0; j < 4; ++j) lg[j] = (lg[j] + crow) * s_cur[j];
        }
        float pr[4];
        if constexpr (BWD) {
            // dS = softmax weight x (dP - delta); masked rows and tail tokens contribute nothing
#pragma unroll
            for (int j = 0; j < 4; ++j) pr[j] = (n0 + j < N && row_ok) ? expf(s_cur[j] - bw_m) * bw_linv * (lg[j] - bw_delta) : 0.f;
            if (wave == 0 && row_ok) *reinterpret_cast<f32x4*>(scores + (long)(grow0 + r16) * score_stride + n0) = f32x4{pr[0], pr[1], pr[2], pr[3]};
        } else {
            if (wave == 0 && row_ok) *reinterpret_cast<f32x4*>(scores + (long)(grow0 + r16) * score_stride + n0) = lg;

            // ---- online softmax for row r16 (lanes r16, r16+16, r16+32, r16+48 share the row) ----
            float tmax = -1.0e30f;
#pragma unroll
            for (int j = 0; j < 4; ++j) tmax = (n0 + j < N) ? fmaxf(tmax, lg[j]) : tmax;
            tmax = xrow4_max(tmax);                          // (the row's four lanes r16 + 16 kg: gfx950 row swaps, no LDS round trip)
            const float m_new = fmaxf(m_run, tmax);
            const float alpha = expf(m_run - m_new);
            float lsum = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pr[j] = (n0 + j < N) ? expf(lg[j] - m_new) : 0.f;
                lsum += pr[j];
            }
            lsum = xrow4_sum(lsum);
            l_run = l_run * alpha + lsum;
            m_run = m_new;
            // rescale the running context when any row's max moved (wave-uniform branch)
            if (__any(alpha != 1.0f)) {
                const float a0 = __shfl(alpha, 4 * kg + 0, 64), a1 = __shfl(alpha, 4 * kg + 1, 64);
                const float a2 = __shfl(alpha, 4 * kg + 2, 64), a3 = __shfl(alpha, 4 * kg + 3, 64);
#pragma unroll
                for (int cb = 0; cb < CBLK; ++cb) {
                    acc[cb][0] *= a0; acc[cb][1] *= a1; acc[cb][2] *= a2; acc[cb][3] *= a3;
                }
            }
        }
        bf16x4 phi, plo;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint16_t h, l;
            split_bf16(pr[j], h, l);
            phi[j] = (short)h;
            plo[j] = (short)l;
        }

        // ---- ACC += P . x over this wave's output channels ----
#pragma unroll
        for (int cb = 0; cb < CBLK; ++cb) {
            const int ch0 = SLICE * wave + 16 * cb;
            const int blk = ch0 >> 7, c2 = (ch0 & 127) >> 3;
            const char* a = img + blk * 4096 + tr_row_off + 16 * ((c2 + (pp >> 1)) ^ tr_swz);
            const bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4*)(a));
            acc[cb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(phi, b, acc[cb], 0, 0, 0);
            acc[cb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(plo, b, acc[cb], 0, 0, 0);
        }
    }

    // ---- the group's partial state of this segment (rows >= nrows are not stored) ----
    if (!grp_on) return;
    const long prow = (slot + (long)grp * gslots) * 16;
    if (!BWD && wave == 0 && kg == 0 && row_ok) {
        p.part_m[prow + r16] = m_run;
        p.part_l[prow + r16] = l_run;
    }
#pragma unroll
    for (int cb = 0; cb < CBLK; ++cb) {
        float* o = p.part_acc + (prow + 4 * kg) * E + SLICE * wave + 16 * cb + r16;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (grow0 + 4 * kg + j < nrows) o[(long)j * E] = acc[cb][j];
    }
}

// LDS of a stream_segment<nb, groups> workgroup: the double-buffered tile, one exchange area per row group
constexpr int stream_smem(int nb, int groups) { return 2 * nb * 4096 + groups * 4096; }
constexpr int seg_stream_smem(int groups) { return stream_smem(9, groups); }

}  // namespace hicom
