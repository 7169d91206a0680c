// What one wave / workgroup does for ONE item of a many-item compressor step, shared by the equal-shape step (batch.hip: the item
// comes from a constant stride) and the ragged step (ragged.hip: the item comes from a device table); the multi-guide step
// (multi_guide.hip: the item is a guide) takes the placement, the ragged multi-guide step (ragged_multi_guide.hip: the item is an
// (item, guide) pair) the segmented stream with two row groups, the merge and the placement.  Each function gets the item's own pointers, token count and layout
// integers from its caller and indexes nothing outside them, so the callers round identically: an item's result does not depend on
// which of the steps ran it.
#pragma once
#include "window_rows.hpp"

namespace hicom {

// ---------------------------------------------------------------------------------------------------------------------------------
// Local stage, one wave per window: `key` / `value` point at the item's first token, g is the window inside the item's own grid,
// qrow the item's guide row.  WIN <= 64: lane i keeps logit i.  The context goes out as the fp16 plane hicom_readout16_gemm_fwd takes.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int NV>
__device__ __forceinline__ void local_window_ctx16(const uint16_t* key, const uint16_t* value, const uint16_t* qrow, const WindowGeom& g,
                                                   int lane, float scale, _Float16* o) {
    constexpr int D = NV * 384;
    float q[NV][6];
    load_row<NV>(qrow, lane, q);
    float sc = -3.0e38f;
    for (int i = 0; i < g.WIN; ++i) {
        float k[NV][6];
        load_row<NV>(key + g.token_of(i) * D, lane, k);
        const float d = wave_sum_fast(row_dot<NV>(q, k)) * scale;
        if (lane == i) sc = d;
    }
    const float mx = wave_max_fast(sc);
    const float e = lane < g.WIN ? expf(sc - mx) : 0.f;
    const float pw = e / wave_sum_fast(e);
    float acc[NV][6];
    row_zero<NV>(acc);
    for (int i = 0; i < g.WIN; ++i) {
        float v[NV][6];
        load_row<NV>(value + g.token_of(i) * D, lane, v);
        row_axpy<NV>(__shfl(pw, i, 64), v, acc);
    }
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int j = 0; j < 6; ++j) o[384 * s + 6 * lane + j] = (_Float16)fminf(fmaxf(acc[s][j], -65504.f), 65504.f);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The same window with the k / v adaptor blends fused into its row loads (local_attn.hip: local_attn_adapt_kernel has the algebra):
//   key_n = (1 - a_k) x_n + a_k (LN(y_n) gamma_k + beta_k),  y = MLP_k(x) from the two dense GEMMs in front, likewise the values.
// The blended streams are never written: a logit is blend_dot's four wave reductions over the x row and the y row, the context comes
// from two accumulators (sum p_n v_n and sum p_n rstd_n y_n) and the scalar sum p_n rstd_n mu_n; the LayerNorm statistics are fp32,
// from the row in registers.  One wave per window as above (WIN <= 64, lane i keeps logit i; no LDS, no barrier: the four waves of a
// workgroup are four independent windows); one token (x row + y row) in flight.  kx / ky / vx / vy point at the ITEM's first token;
// ky or vy may be NULL (that stream is not adapted), not both.
// ---------------------------------------------------------------------------------------------------------------------------------
struct SegAdaptParams {
    const _Float16* ky;        // MLP_k(key tokens) fp16 [all tokens][D] or NULL
    const uint16_t* kgamma; const uint16_t* kbeta; const void* kalpha;
    const _Float16* vy;        // MLP_v(value tokens) fp16 [all tokens][D] or NULL
    const uint16_t* vgamma; const uint16_t* vbeta; const void* valpha;
    int alpha_f32;
    float eps;
};

template <int NV>
__device__ __forceinline__ void local_window_adapt_ctx16(const uint16_t* kx, const _Float16* ky, const uint16_t* vx, const _Float16* vy,
                                                         const SegAdaptParams& ad, const uint16_t* qrow, const WindowGeom& g, int lane,
                                                         float scale, _Float16* o) {
    constexpr int D = NV * 384;
    const float ak = ky ? read_alpha(ad.kalpha, ad.alpha_f32) : 0.f, av = vy ? read_alpha(ad.valpha, ad.alpha_f32) : 0.f;
    float sc = -3.0e38f;
    {
        float q[NV][6], qg[NV][6];
        float cg = 0.f, cb = 0.f;
        load_row<NV>(qrow, lane, q);
        if (ky) affine_prep<NV>(q, ad.kgamma, ad.kbeta, lane, qg, cg, cb);
        for (int i = 0; i < g.WIN; ++i) {
            const long tok = g.token_of(i);
            float x[NV][6], y[NV][6];
            load_row<NV>(kx + tok * D, lane, x);
            if (ky) load_row_f16<NV>(ky + tok * D, lane, y);
            float mu, rstd;
            const float d = blend_dot<NV>(x, y, ky != nullptr, q, qg, cg, cb, ak, ad.eps, mu, rstd) * scale;
            if (lane == i) sc = d;
        }
    }
    const float mx = wave_max_fast(sc);
    const float e = lane < g.WIN ? expf(sc - mx) : 0.f;
    const float pw = e / wave_sum_fast(e);
    float accx[NV][6], accy[NV][6];
    float smu = 0.f;                                // sum_n p_n rstd_n mu_n (identical in every lane)
    row_zero<NV>(accx);
    row_zero<NV>(accy);
    for (int i = 0; i < g.WIN; ++i) {
        const long tok = g.token_of(i);
        float x[NV][6], y[NV][6];
        load_row<NV>(vx + tok * D, lane, x);
        if (vy) load_row_f16<NV>(vy + tok * D, lane, y);
        const float pi = __shfl(pw, i, 64);
        row_axpy<NV>(pi, x, accx);
        if (vy) {
            float mu, rstd;
            ln_stats<NV>(y, ad.eps, mu, rstd);
            const float wy = pi * rstd;
            smu = fmaf(wy, mu, smu);
            row_axpy<NV>(wy, y, accy);
        }
    }
    if (vy) {
        float gm[NV][6], bt[NV][6];
        load_row<NV>(ad.vgamma, lane, gm);
        load_row<NV>(ad.vbeta, lane, bt);
#pragma unroll
        for (int s = 0; s < NV; ++s)
#pragma unroll
            for (int j = 0; j < 6; ++j) accx[s][j] = (1.0f - av) * accx[s][j] + av * (gm[s][j] * (accy[s][j] - smu) + bt[s][j]);
    }
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int j = 0; j < 6; ++j) o[384 * s + 6 * lane + j] = (_Float16)fminf(fmaxf(accx[s][j], -65504.f), 65504.f);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Segmented global stream.  Tile staging, swizzle, MFMA operand layouts and the per-tile order of operations are those of
// global_stream_kernel (global_stream.hip); see there for the CDNA4 mapping.  A workgroup walks the 16-token tiles [tb, te) of ONE
// item, counted from the item's first token, for one or two groups of 16 folded rows of that item.
// ---------------------------------------------------------------------------------------------------------------------------------
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

__device__ __forceinline__ int bswz(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }
__device__ __forceinline__ int bsig(int g) { return ((g & 1) << 1) | (g >> 1); }

// One body for one or two ROW GROUPS of 16 folded rows: a workgroup of 64 * 4 * GROUPS threads in which waves 4 g .. 4 g + 3 are the
// four-wave machine of group g, all groups on ONE double-buffered LDS tile (staged once per workgroup, its 1 KB pieces dealt round-robin
// to all waves), so an item's tokens come from HBM once per 16 * GROUPS rows.  Each group has its own exchange area, online softmax and
// accumulators, in the same operations and the same order per row: a row's result does not depend on GROUPS, on its group, on the
// other rows of the workgroup or on how many of them are live.  A group without a live row (rows >= nrows) stages and keeps the
// barriers only.  GROUPS == 1 (batch.hip, ragged.hip: row0 = 0, nrows = p.rows, gslots = 0): the group index and everything derived
// from it are compile-time zero and the guards fold away.
// xi: the item's N tokens [N][E]; row0: the workgroup's first row in the item's row space, nrows: the item's rows; qrow0: the item's
// first row in the query planes; scores: the item's [nrows][score_stride] logits; slot: where group 0's partial state (m, l, ACC) goes,
// group g `g * gslots` slots further.  Everything but the lane-dependent parts must be wave-uniform.
template <int NB, int GROUPS>
__device__ __forceinline__ void stream_segment(const SegStreamParams& p, const uint16_t* xi, int N, int tb, int te, int row0, int nrows, long qrow0,
                                               float* scores, long score_stride, long slot, int gslots) {
    constexpr int E = NB * 128;
    constexpr int SLICE = E / 4;
    constexpr int KSTEPS = SLICE / 32;
    constexpr int CBLK = SLICE / 16;
    constexpr int TILE_BYTES = NB * 4096;
    constexpr int PIECES = NB * 4;
    constexpr int WAVES = 4 * GROUPS;
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

    // ---- A operand: the group's folded queries (rows >= nrows: zero), this wave's channel slice ----
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
    float m_run = -1.0e30f, l_run = 0.f;

    auto stage = [&](int tile, int buf) {
        const int r = lane >> 4, cpos = lane & 15;
#pragma unroll
        for (int i = 0; i < (PIECES + WAVES - 1) / WAVES; ++i) {
            const int pi = wave_wg + WAVES * i;
            if (PIECES % WAVES == 0 || pi < PIECES) {               // (wave-uniform; two groups: 36 pieces, waves 0-3 issue five, waves 4-7 four)
                const int blk = pi >> 2, row = 4 * (pi & 3) + r;
                int tok = tile * 16 + row;
                tok = tok < N ? tok : N - 1;   // tail tile: the item's own last token again (masked below), never a neighbour's
                const char* src = reinterpret_cast<const char*>(xi) + (long)tok * (E * 2) + blk * 256 + 16 * (cpos ^ bswz(row));
                char* dst = tilebuf + buf * TILE_BYTES + pi * 1024;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src),
                                                 (__attribute__((address_space(3))) void*)(dst), 16, 0, 0);
            }
        }
    };

    const int q4 = (lane >> 2) & 3, pp = lane & 3;
    const int trow = 4 * bsig(kg) + q4;
    const int rd_row_off = r16 * 256, rd_swz = bswz(r16);
    const int tr_row_off = trow * 256 + 8 * (pp & 1), tr_swz = bswz(trow);
    const float* pa = (p.pos_a && row_ok) ? p.pos_a + qrow * p.pos_stride : nullptr;

    // positional logit terms, one tile ahead (see global_stream_kernel); the token index is item-local: t restarts at 0 per item
    float pt[4] = {0.f, 0.f, 0.f, 0.f}, py[4] = {0.f, 0.f, 0.f, 0.f}, px[4] = {0.f, 0.f, 0.f, 0.f};
    auto fetch_pos = [&](int tile) {
        if (pa) {
            const int nb = tile * 16 + 4 * bsig(kg);
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

    if (tb < te) {
        fetch_pos(tb);
        stage(tb, 0);
    }

    for (int tile = tb; tile < te; ++tile) {
        const int cur = (tile - tb) & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        float padd[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) padd[j] = pt[j] + py[j] + px[j];
        if (tile + 1 < te) {
            fetch_pos(tile + 1);
            stage(tile + 1, cur ^ 1);
        }
        const char* img = tilebuf + cur * TILE_BYTES;

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
            float* rw = red + wave * 256;
#pragma unroll
            for (int j = 0; j < 4; ++j) rw[(4 * kg + j) * 16 + r16] = s4[j];
        }
        lds_barrier();
        if (!grp_on) continue;                                      // (wave-uniform; both barriers of the tile are behind this wave)

        const float* rb = red + r16 * 16 + 4 * bsig(kg);
        f32x4 lg = *reinterpret_cast<const f32x4*>(rb);
        lg += *reinterpret_cast<const f32x4*>(rb + 256);
        lg += *reinterpret_cast<const f32x4*>(rb + 512);
        lg += *reinterpret_cast<const f32x4*>(rb + 768);
        const int n0 = tile * 16 + 4 * bsig(kg);
#pragma unroll
        for (int j = 0; j < 4; ++j) lg[j] += padd[j];
        if (wave == 0 && row_ok) *reinterpret_cast<f32x4*>(scores + (long)(grow0 + r16) * score_stride + n0) = lg;

        float tmax = -1.0e30f;
#pragma unroll
        for (int j = 0; j < 4; ++j) tmax = (n0 + j < N) ? fmaxf(tmax, lg[j]) : tmax;
        tmax = xrow4_max(tmax);
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = expf(m_run - m_new);
        float pr[4], lsum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pr[j] = (n0 + j < N) ? expf(lg[j] - m_new) : 0.f;
            lsum += pr[j];
        }
        lsum = xrow4_sum(lsum);
        l_run = l_run * alpha + lsum;
        m_run = m_new;
        if (__any(alpha != 1.0f)) {
            const float a0 = __shfl(alpha, 4 * kg + 0, 64), a1 = __shfl(alpha, 4 * kg + 1, 64);
            const float a2 = __shfl(alpha, 4 * kg + 2, 64), a3 = __shfl(alpha, 4 * kg + 3, 64);
#pragma unroll
            for (int cb = 0; cb < CBLK; ++cb) {
                acc[cb][0] *= a0; acc[cb][1] *= a1; acc[cb][2] *= a2; acc[cb][3] *= a3;
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
    if (wave == 0 && kg == 0 && row_ok) {
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

// LDS of a stream_segment<9, groups> workgroup: the double-buffered tile, one exchange area per row group
constexpr int seg_stream_smem(int groups) { return 2 * 9 * 4096 + groups * 4096; }

// ---------------------------------------------------------------------------------------------------------------------------------
// Merge of one (item, head) row: ctx = sum_p e^(m_p - M) ACC_p / L + sum_s marg[s] pe[s], marg = the row's softmax weights summed
// over the other two axes (slots [T | H | W]), from the logits `s` the stream left for this row.  The item's partial states are the
// slots [slot0, slot0 + nparts).  Fixed summation orders: the result depends on the item's tokens, guide and nparts only.
// ms: LDS, T (H + W) + T + H + W floats.
// ---------------------------------------------------------------------------------------------------------------------------------
struct SegMergeParams {
    const float* part_m;
    const float* part_l;
    const float* part_acc;
    const float* pe;        // [P][E]
    int E, H, W;
    int t0i, y0i, x0i;
};

__device__ __forceinline__ void merge_segments(const SegMergeParams& p, float* ms, int r, int tid, int T, int nparts, long slot0, const float* s,
                                               float* ctx) {
    const int H = p.H, W = p.W;
    float* rowsum = ms;                 // [T][H]: weights summed over x
    float* colsum = ms + T * H;         // [T][W]: weights summed over y
    float* marg = colsum + T * W;       // [T + H + W]
    const long pbase = slot0 * 16 + r;
    float M = -1.0e30f;
    for (int c = 0; c < nparts; ++c) M = fmaxf(M, p.part_m[pbase + c * 16]);
    float L = 0.f;
    for (int c = 0; c < nparts; ++c) L += p.part_l[pbase + c * 16] * expf(p.part_m[pbase + c * 16] - M);
    const float invL = 1.0f / L;
    if (p.pe) {
        for (int i = tid; i < T * H; i += 256) {
            float a = 0.f;
            for (int x = 0; x < W; ++x) a += expf(s[(long)i * W + x] - M);
            rowsum[i] = a;
        }
        for (int i = tid; i < T * W; i += 256) {
            const int t = i / W, x = i - t * W;
            float a = 0.f;
            for (int y = 0; y < H; ++y) a += expf(s[((long)t * H + y) * W + x] - M);
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
            marg[i] = a * invL;
        }
        __syncthreads();
    }
    for (int e = tid; e < p.E; e += 256) {
        float v = 0.f;
        for (int c = 0; c < nparts; ++c)
            v += expf(p.part_m[pbase + c * 16] - M) * p.part_acc[(slot0 + c) * 16 * p.E + (long)r * p.E + e];
        v *= invL;
        if (p.pe) {
            float pos = 0.f;
            for (int t = 0; t < T; ++t) pos = fmaf(marg[t], p.pe[(long)(p.t0i + t) * p.E + e], pos);
            for (int y = 0; y < H; ++y) pos = fmaf(marg[T + y], p.pe[(long)(p.y0i + y) * p.E + e], pos);
            for (int x = 0; x < W; ++x) pos = fmaf(marg[T + H + x], p.pe[(long)(p.x0i + x) * p.E + e], pos);
            v += pos;
        }
        ctx[e] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Placement of one packed output row (byte work), r = the row inside its item, o = the row's element offset in `out`:
//   rows >= global_row0: the item's global row `tok` (f32, rounded once: the copies are bit-identical);
//   newline rows nl_first + i nl_step, i < nl_count; every other row: local token m = r - r / (nl_group + 1), row loc_row0 + m of loc.
// ---------------------------------------------------------------------------------------------------------------------------------
struct SegPlaceParams {
    const void* loc;        // [all windows][hidden], out dtype
    const float* tok;       // [items][hidden]
    const uint16_t* newline;// bf16 [hidden] or NULL
    void* out;
    int out_f32, hidden;
};

__device__ __forceinline__ void place_row(const SegPlaceParams& p, long r, long o, long item, long loc_row0, int nl_group, int nl_count,
                                          long global_row0, long nl_first, long nl_step) {
    const bool is_nl = nl_count > 0 && r >= nl_first && r < global_row0 && (r - nl_first) % nl_step == 0 && (r - nl_first) / nl_step < nl_count;
    for (int c = threadIdx.x; c < p.hidden; c += 128) {
        if (r >= global_row0) {
            const float v = p.tok[item * p.hidden + c];
            if (p.out_f32) reinterpret_cast<float*>(p.out)[o + c] = v;
            else reinterpret_cast<uint16_t*>(p.out)[o + c] = f32_to_bf16(v);
        } else if (is_nl) {
            if (p.out_f32) reinterpret_cast<float*>(p.out)[o + c] = bf16_to_f32(p.newline[c]);
            else reinterpret_cast<uint16_t*>(p.out)[o + c] = p.newline[c];
        } else {
            const long m = nl_group ? r - r / (nl_group + 1) : r;
            const long src = (loc_row0 + m) * p.hidden + c;
            if (p.out_f32) reinterpret_cast<float*>(p.out)[o + c] = reinterpret_cast<const float*>(p.loc)[src];
            else reinterpret_cast<uint16_t*>(p.out)[o + c] = reinterpret_cast<const uint16_t*>(p.loc)[src];
        }
    }
}

// Placement for items of ONE packed-row layout (batch.hip: item = item of the batch; multi_guide.hip: item = guide): output row /
// item_rows = item.  grid = items * item_rows, one output row per workgroup.
struct EqualPlaceParams {
    SegPlaceParams c;
    int wpi, nl_group, nl_count;
    long item_rows, global_row0, nl_first, nl_step, ldo;
};

__device__ __forceinline__ void place_equal_row(const EqualPlaceParams& p) {
    const long row = blockIdx.x;
    const long item = row / p.item_rows, r = row - item * p.item_rows;
    place_row(p.c, r, row * p.ldo, item, item * p.wpi, p.nl_group, p.nl_count, p.global_row0, p.nl_first, p.nl_step);
}

}  // namespace hicom
