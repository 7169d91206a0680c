// What one wave / workgroup does for ONE item of a many-item compressor step, shared by the equal-shape step (batch.hip: the item
// comes from a constant stride) and the ragged step (ragged.hip: the item comes from a device table); the multi-guide step
// (multi_guide.hip: the item is a guide) takes the placement, the ragged multi-guide step (ragged_multi_guide.hip: the item is an
// (item, guide) pair) the merge and the placement.  Each function gets the item's own pointers, token count and layout
// integers from its caller and indexes nothing outside them, so the callers round identically: an item's result does not depend on
// which of the steps ran it.  The segmented global stream of these steps is not here: it is stream_segment (stream_body.hpp, included
// below), the one body of the four-wave stream machine, which the single-item global_stream_kernel wraps as well.
#pragma once
#include "stream_body.hpp"
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
// The backward twin of merge_segments, one (item, head) row: dqt = sum_p ACC_p + sum_s marg[s] pe[s], ACC_p the partial sums of
// dS x the backward stream left in the item's slots, marg the PLAIN sums of the row's dS over the other two axes (no exp, no rescale:
// dS is final).  Same LDS (T (H + W) + T + H + W floats) and the same fixed summation orders: the result depends on the item's tokens,
// its cotangent and nparts only.
// ---------------------------------------------------------------------------------------------------------------------------------
struct SegDqMergeParams {
    const float* part_acc;
    const float* pe;        // [P][E] or NULL
    int E, H, W;
    int t0i, y0i, x0i;
};

__device__ __forceinline__ void dq_merge_segments(const SegDqMergeParams& p, float* ms, int r, int tid, int T, int nparts, long slot0, const float* ds,
                                                  float* dqt) {
    const int H = p.H, W = p.W;
    float* rowsum = ms;                 // [T][H]: dS summed over x
    float* colsum = ms + T * H;         // [T][W]: dS summed over y
    float* marg = colsum + T * W;       // [T + H + W]
    if (p.pe) {
        for (int i = tid; i < T * H; i += 256) {
            float a = 0.f;
            for (int x = 0; x < W; ++x) a += ds[(long)i * W + x];
            rowsum[i] = a;
        }
        for (int i = tid; i < T * W; i += 256) {
            const int t = i / W, x = i - t * W;
            float a = 0.f;
            for (int y = 0; y < H; ++y) a += ds[((long)t * H + y) * W + x];
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
        __syncthreads();
    }
    for (int e = tid; e < p.E; e += 256) {
        float v = 0.f;
        for (int c = 0; c < nparts; ++c) v += p.part_acc[(slot0 + c) * 16 * p.E + (long)r * p.E + e];
        if (p.pe) {
            float pos = 0.f;
            for (int t = 0; t < T; ++t) pos = fmaf(marg[t], p.pe[(long)(p.t0i + t) * p.E + e], pos);
            for (int y = 0; y < H; ++y) pos = fmaf(marg[T + y], p.pe[(long)(p.y0i + y) * p.E + e], pos);
            for (int x = 0; x < W; ++x) pos = fmaf(marg[T + H + x], p.pe[(long)(p.x0i + x) * p.E + e], pos);
            v += pos;
        }
        dqt[e] = v;
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
