// Batched compressor step: B items of one shape (images or short clips) through a launch sequence whose length does not depend on B.
//
// The math per item is the release recipe's (direct guide, local + global compressor); new is the item dimension:
//   * queries: q_proj, the k_proj fold with hi / lo planes and the score-side positional table run with M = B rows through the
//     existing small linears (hicom_linear_fwd, hicom_fold_query_split_fwd);
//   * local stage: kt | T, so no window crosses an item boundary: the [B T, H, W] stack is ONE window grid and window w reads the
//     guide row of item w / windows_per_item (batch_local_attn_kernel: one wave per window, contexts as the fp16 plane that
//     hicom_readout16_gemm_fwd takes);
//   * global stage: batch_global_stream_kernel, the narrow streaming kernel of global_stream.hip with blockIdx.y = item.  A
//     workgroup walks a contiguous range of 16-token tiles of ONE item (chunk blockIdx.x of `chunks`), so a partial state (m, l, ACC)
//     never mixes tokens of two items; the token index is item-local (frame index restarts at 0 per item), the tail tile re-reads
//     the item's own last token and is masked.  batch_merge_kernel then merges the chunks of each (item, head) row and adds the
//     value-side positional term from the row's t / y / x marginals (taken from the logits the stream kernel left);
//   * tail: v_proj per head, out_proj + residual, the two global readout layers with M = B rows (hicom_linear_fwd), both local
//     readout layers as one GEMM pair over all B x windows_per_item contexts (hicom_readout16_gemm_fwd), and ONE placement launch
//     that writes every item's packed rows: local tokens around the newline gaps, newline rows, the 32 copies of the global row.
// Twelve launches for any B.  Everything on the caller's stream, nothing synchronises the host.
#include "window_rows.hpp"

namespace hicom {

// ---------------------------------------------------------------------------------------------------------------------------------
// Local stage: one wave per window of the stacked grid, the item's guide row as the query.  WIN <= 64: lane i keeps logit i.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int NV>
__global__ __launch_bounds__(256) void batch_local_attn_kernel(const uint16_t* key, const uint16_t* value, const uint16_t* guide,
                                                               hicom_axis at, hicom_axis ay, hicom_axis ax, int wpi, int nwin,
                                                               float scale, _Float16* ctx16) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (win >= nwin) return;
    const WindowGeom g(at, ay, ax, win);
    float q[NV][6];
    load_row<NV>(guide + (long)(win / wpi) * D, lane, q);
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
    _Float16* o = ctx16 + (long)win * D;
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int j = 0; j < 6; ++j) o[384 * s + 6 * lane + j] = (_Float16)fminf(fmaxf(acc[s][j], -65504.f), 65504.f);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Segmented global stream.  Tile staging, swizzle, MFMA operand layouts and the per-tile order of operations are those of
// global_stream_kernel (global_stream.hip); see there for the CDNA4 mapping.  grid = (chunks, B).
// ---------------------------------------------------------------------------------------------------------------------------------
struct BatchStreamParams {
    const uint16_t* x;      // [B][N][E]
    int N;                  // tokens per item
    int ntiles;             // 16-token tiles per item
    const uint16_t* qhi;    // [B * rows][E] folded queries, item-major
    const uint16_t* qlo;
    const float* pos_a;     // [B * rows][pos_stride]
    int pos_stride;
    int rows;               // folded rows per item (heads), <= 16
    int H, W, HW;
    int t0i, y0i, x0i;
    float* scores;          // [B][16][score_stride]
    long score_stride;
    float* part_m;          // [B][chunks][16]
    float* part_l;
    float* part_acc;        // [B][chunks][16][E]
};

__device__ __forceinline__ int bswz(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }
__device__ __forceinline__ int bsig(int g) { return ((g & 1) << 1) | (g >> 1); }

template <int NB>
__global__ __launch_bounds__(256, 2) void batch_global_stream_kernel(BatchStreamParams p) {
    constexpr int E = NB * 128;
    constexpr int SLICE = E / 4;
    constexpr int KSTEPS = SLICE / 32;
    constexpr int CBLK = SLICE / 16;
    constexpr int TILE_BYTES = NB * 4096;
    constexpr int PIECES = NB * 4;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* tilebuf = smem;                                           // [2][TILE_BYTES]
    float* red = reinterpret_cast<float*>(smem + 2 * TILE_BYTES);  // [4 waves][16 rows][16 tokens]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kg = lane >> 4;
    const int part = blockIdx.x, item = blockIdx.y, nparts = gridDim.x;
    const int tb = (int)(((long)p.ntiles * part) / nparts);
    const int te = (int)(((long)p.ntiles * (part + 1)) / nparts);
    const bool row_ok = r16 < p.rows;
    const long qrow = (long)item * p.rows + r16;
    const uint16_t* xi = p.x + (long)item * p.N * E;                // this item's tokens: nothing below indexes past them

    // ---- A operand: the item's folded queries (rows >= p.rows: zero), this wave's channel slice ----
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
        static_assert(PIECES % 4 == 0, "pieces are dealt round-robin to the 4 waves");
#pragma unroll
        for (int i = 0; i < PIECES / 4; ++i) {
            const int pi = wave + 4 * i;
            const int blk = pi >> 2, row = 4 * (pi & 3) + r;
            int tok = tile * 16 + row;
            tok = tok < p.N ? tok : p.N - 1;   // tail tile: the item's own last token again (masked below), never a neighbour's
            const char* src = reinterpret_cast<const char*>(xi) + (long)tok * (E * 2) + blk * 256 + 16 * (cpos ^ bswz(row));
            char* dst = tilebuf + buf * TILE_BYTES + pi * 1024;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src),
                                             (__attribute__((address_space(3))) void*)(dst), 16, 0, 0);
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
                n = n < p.N ? n : p.N - 1;
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
        lds_barrier();

        const float* rb = red + r16 * 16 + 4 * bsig(kg);
        f32x4 lg = *reinterpret_cast<const f32x4*>(rb);
        lg += *reinterpret_cast<const f32x4*>(rb + 256);
        lg += *reinterpret_cast<const f32x4*>(rb + 512);
        lg += *reinterpret_cast<const f32x4*>(rb + 768);
        const int n0 = tile * 16 + 4 * bsig(kg);
#pragma unroll
        for (int j = 0; j < 4; ++j) lg[j] += padd[j];
        if (wave == 0 && row_ok) *reinterpret_cast<f32x4*>(p.scores + ((long)item * 16 + r16) * p.score_stride + n0) = lg;

        float tmax = -1.0e30f;
#pragma unroll
        for (int j = 0; j < 4; ++j) tmax = (n0 + j < p.N) ? fmaxf(tmax, lg[j]) : tmax;
        tmax = xrow4_max(tmax);
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = expf(m_run - m_new);
        float pr[4], lsum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pr[j] = (n0 + j < p.N) ? expf(lg[j] - m_new) : 0.f;
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

    // ---- this (item, chunk)'s partial state ----
    const long prow = ((long)item * nparts + part) * 16;
    if (wave == 0 && kg == 0 && row_ok) {
        p.part_m[prow + r16] = m_run;
        p.part_l[prow + r16] = l_run;
    }
#pragma unroll
    for (int cb = 0; cb < CBLK; ++cb) {
        float* o = p.part_acc + (prow + 4 * kg) * E + SLICE * wave + 16 * cb + r16;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * kg + j < p.rows) o[(long)j * E] = acc[cb][j];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Merge per (item, head): ctx = sum_p e^(m_p - M) ACC_p / L + sum_s marg[s] pe[s], marg = the row's softmax weights summed over the
// other two axes (slots [T | H | W]), from the logits of the item.  Fixed summation orders: bit-reproducible.  grid = (rows, B).
// ---------------------------------------------------------------------------------------------------------------------------------
struct BatchMergeParams {
    const float* part_m;
    const float* part_l;
    const float* part_acc;
    const float* scores;
    long score_stride;
    const float* pe;        // [P][E]
    int nparts, rows, E, T, H, W;
    int t0i, y0i, x0i;
    float* ctx;             // [B * rows][E]
};

__global__ __launch_bounds__(256) void batch_merge_kernel(BatchMergeParams p) {
    extern __shared__ float ms[];
    const int r = blockIdx.x, item = blockIdx.y, tid = threadIdx.x;
    const int T = p.T, H = p.H, W = p.W;
    float* rowsum = ms;                 // [T][H]: weights summed over x
    float* colsum = ms + T * H;         // [T][W]: weights summed over y
    float* marg = colsum + T * W;       // [T + H + W]
    const long pbase = (long)item * p.nparts * 16 + r;
    float M = -1.0e30f;
    for (int c = 0; c < p.nparts; ++c) M = fmaxf(M, p.part_m[pbase + c * 16]);
    float L = 0.f;
    for (int c = 0; c < p.nparts; ++c) L += p.part_l[pbase + c * 16] * expf(p.part_m[pbase + c * 16] - M);
    const float invL = 1.0f / L;
    const float* s = p.scores + ((long)item * 16 + r) * p.score_stride;
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
        for (int c = 0; c < p.nparts; ++c)
            v += expf(p.part_m[pbase + c * 16] - M) * p.part_acc[((long)item * p.nparts + c) * 16 * p.E + (long)r * p.E + e];
        v *= invL;
        if (p.pe) {
            float pos = 0.f;
            for (int t = 0; t < T; ++t) pos = fmaf(marg[t], p.pe[(long)(p.t0i + t) * p.E + e], pos);
            for (int y = 0; y < H; ++y) pos = fmaf(marg[T + y], p.pe[(long)(p.y0i + y) * p.E + e], pos);
            for (int x = 0; x < W; ++x) pos = fmaf(marg[T + H + x], p.pe[(long)(p.x0i + x) * p.E + e], pos);
            v += pos;
        }
        p.ctx[((long)item * p.rows + r) * p.E + e] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Placement of every item's packed rows (byte work): grid = B * item_rows, one output row per workgroup.
//   rows >= global_row0: the item's global row (f32, rounded once: the n_global copies are bit-identical);
//   newline rows nl_first + i nl_step, i < nl_count; every other row: local token m = r - r / (nl_group + 1) of the item.
// ---------------------------------------------------------------------------------------------------------------------------------
struct BatchPlaceParams {
    const void* loc;        // [B * wpi][hidden], out dtype
    const float* tok;       // [B][hidden]
    const uint16_t* newline;// bf16 [hidden] or NULL
    void* out;
    int out_f32, hidden, wpi, nl_group, nl_count;
    long item_rows, global_row0, nl_first, nl_step, ldo;
};

__global__ __launch_bounds__(128) void batch_place_kernel(BatchPlaceParams p) {
    const long row = blockIdx.x;
    const long item = row / p.item_rows, r = row - item * p.item_rows;
    const long o = row * p.ldo;
    const bool is_nl = p.nl_count > 0 && r >= p.nl_first && r < p.global_row0 && (r - p.nl_first) % p.nl_step == 0 &&
                       (r - p.nl_first) / p.nl_step < p.nl_count;
    for (int c = threadIdx.x; c < p.hidden; c += 128) {
        if (r >= p.global_row0) {
            const float v = p.tok[item * p.hidden + c];
            if (p.out_f32) reinterpret_cast<float*>(p.out)[o + c] = v;
            else reinterpret_cast<uint16_t*>(p.out)[o + c] = f32_to_bf16(v);
        } else if (is_nl) {
            if (p.out_f32) reinterpret_cast<float*>(p.out)[o + c] = bf16_to_f32(p.newline[c]);
            else reinterpret_cast<uint16_t*>(p.out)[o + c] = p.newline[c];
        } else {
            const long m = p.nl_group ? r - r / (p.nl_group + 1) : r;
            const long src = (item * p.wpi + m) * p.hidden + c;
            if (p.out_f32) reinterpret_cast<float*>(p.out)[o + c] = reinterpret_cast<const float*>(p.loc)[src];
            else reinterpret_cast<uint16_t*>(p.out)[o + c] = reinterpret_cast<const uint16_t*>(p.loc)[src];
        }
    }
}

}  // namespace hicom

using namespace hicom;

namespace {

constexpr int kBatchMax = 4096;          // items per call (grid y of the segmented kernels, far below the limit)
constexpr int kBatchMaxChunks = 64;

int batch_num_cus() {
    static int n = 0;
    if (n == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) n = v;
        else n = 256;
    }
    return n;
}

// workgroups per item of the segmented stream: B x chunks fills the chip twice over (two resident workgroups per CU); one chunk
// per item once B alone does
int batch_chunks(const hicom_compressor_batch_args* a) {
    const long ntiles = ((long)a->T * a->H * a->W + 15) / 16;
    long c = a->chunks > 0 ? a->chunks : (2L * batch_num_cus() + a->B - 1) / a->B;
    if (c > ntiles) c = ntiles;
    if (c > kBatchMaxChunks) c = kBatchMaxChunks;
    return (int)(c < 1 ? 1 : c);
}

struct BatchLayout {
    long qp, qhi, qlo, pos_a, scores, part_m, part_l, part_acc, ctxg, o, pre, hid, tok, ctx16, hid16, loc, total;
    long score_stride;
    int chunks, wpi, rows_all;
};

BatchLayout batch_layout(const hicom_compressor_batch_args* a) {
    BatchLayout l;
    long off = 0;
    auto take = [&](long bytes) { const long at = off; off += (bytes + 255) / 256 * 256; return at; };
    const long B = a->B, E = a->E, N = (long)a->T * a->H * a->W, R = B * a->nh;
    l.chunks = batch_chunks(a);
    l.wpi = (a->T / a->kt) * (a->H / a->ks) * (a->W / a->ks);
    l.rows_all = (int)(B * l.wpi);
    l.score_stride = (N + 15) / 16 * 16;
    const int odt = a->out_dt == HICOM_DT_F32 ? 4 : 2;
    l.qp = take(B * E * 4);
    l.qhi = take(R * E * 2);
    l.qlo = take(R * E * 2);
    l.pos_a = take(R * (long)(a->P > 0 ? a->P : 1) * 4);
    l.scores = take(B * 16 * l.score_stride * 4);
    l.part_m = take(B * l.chunks * 16 * 4);
    l.part_l = take(B * l.chunks * 16 * 4);
    l.part_acc = take(B * l.chunks * 16 * E * 4);
    l.ctxg = take(R * E * 4);
    l.o = take(B * E * 4);
    l.pre = take(B * E * 4);
    l.hid = take(B * (long)a->hidden * 4);
    l.tok = take(B * (long)a->hidden * 4);
    l.ctx16 = take((long)l.rows_all * E * 2);
    l.hid16 = take((long)l.rows_all * a->hidden * 2);
    l.loc = take((long)l.rows_all * a->hidden * odt);
    l.total = off;
    return l;
}

int batch_check(const hicom_compressor_batch_args* a) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "compressor_batch: NULL arguments");
    HICOM_REQUIRE(a->B > 0 && a->T > 0 && a->H > 0 && a->W > 0 && a->hidden > 0 && a->kt > 0 && a->ks > 0, HICOM_EINVAL, "compressor_batch: bad shape");
    HICOM_REQUIRE(a->B <= kBatchMax, HICOM_EUNSUP, "compressor_batch: B=%d items (<= %d per call)", a->B, kBatchMax);
    HICOM_REQUIRE(a->E == 1152, HICOM_EUNSUP, "compressor_batch: E=%d (only 1152)", a->E);
    HICOM_REQUIRE(a->nh > 0 && a->nh <= 16 && a->E % a->nh == 0, HICOM_EUNSUP, "compressor_batch: %d heads (<= 16 folded rows per item)", a->nh);
    HICOM_REQUIRE(a->hidden % 64 == 0, HICOM_EUNSUP, "compressor_batch: hidden=%d (multiple of 64: fp16 readout planes)", a->hidden);
    HICOM_REQUIRE(a->T % a->kt == 0 && a->H % a->ks == 0 && a->W % a->ks == 0, HICOM_EUNSUP,
                  "compressor_batch: needs an exact window partition (T=%d H=%d W=%d, windows %dx%dx%d)", a->T, a->H, a->W, a->kt, a->ks, a->ks);
    HICOM_REQUIRE(a->kt * a->ks * a->ks <= 64, HICOM_EUNSUP, "compressor_batch: windows of %d tokens (<= 64)", a->kt * a->ks * a->ks);
    HICOM_REQUIRE((long)a->B * a->T * a->H * a->W < (1L << 31) / 16, HICOM_EUNSUP, "compressor_batch: too many tokens in one call");
    HICOM_REQUIRE(((long)a->T * a->H + (long)a->T * a->W + a->T + a->H + a->W) * 4 <= 48 * 1024, HICOM_EUNSUP,
                  "compressor_batch: T=%d frames of %dx%d: the merge keeps T (H + W) marginal sums in LDS", a->T, a->H, a->W);
    HICOM_REQUIRE(a->out_dt == HICOM_DT_BF16 || a->out_dt == HICOM_DT_F32, HICOM_EUNSUP, "compressor_batch: output dtype %d (bf16 | f32)", a->out_dt);
    HICOM_REQUIRE(!a->pe == !a->kpe && (!a->pe || a->P > 0), HICOM_EINVAL, "compressor_batch: pe and kpe come together");
    return HICOM_OK;
}

}  // namespace

extern "C" int64_t hicom_compressor_batch_workspace_bytes(const hicom_compressor_batch_args* a) {
    const int st = batch_check(a);
    if (st != HICOM_OK) return st;
    return batch_layout(a).total;
}

extern "C" int hicom_compressor_batch_fwd(const hicom_compressor_batch_args* a) {
    int st = batch_check(a);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->ff && a->guide && a->out && a->ws, HICOM_EINVAL, "compressor_batch: NULL pointer");
    HICOM_REQUIRE(a->lw0_f16 && a->lw2_f16 && a->wq && a->wk && a->wv && a->wo && a->gw0 && a->gw2, HICOM_EINVAL, "compressor_batch: NULL weight");
    const BatchLayout l = batch_layout(a);
    HICOM_REQUIRE(a->ws_bytes >= l.total && (uintptr_t)a->ws % 256 == 0, HICOM_EINVAL, "compressor_batch: workspace of %ld bytes, 256-byte aligned",
                  l.total);
    HICOM_REQUIRE((uintptr_t)a->ff % 16 == 0 && (!a->fe || (uintptr_t)a->fe % 16 == 0) && (uintptr_t)a->guide % 16 == 0, HICOM_EINVAL,
                  "compressor_batch: 16-byte aligned inputs");
    const long item_local = (long)l.wpi + (a->nl_group ? l.wpi / a->nl_group : 0);
    HICOM_REQUIRE(a->n_global_rows > 0 && a->global_row0 >= item_local && a->item_rows == a->global_row0 + a->n_global_rows && a->ldo >= a->hidden &&
                      a->nl_group >= 0 && (!a->nl_group || l.wpi % a->nl_group == 0),
                  HICOM_EINVAL, "compressor_batch: output layout");
    HICOM_REQUIRE(a->nl_count == 0 || (a->newline && a->nl_step > 0 && a->nl_first >= 0 &&
                                       a->nl_first + (long)(a->nl_count - 1) * a->nl_step < a->global_row0),
                  HICOM_EINVAL, "compressor_batch: newline rows");
    // every local row of an item is a token row or a newline row
    HICOM_REQUIRE(a->global_row0 == (long)l.wpi + a->nl_count, HICOM_EINVAL, "compressor_batch: %ld local rows for %d tokens + %d newline rows",
                  (long)a->global_row0, l.wpi, a->nl_count);
    char* ws = (char*)a->ws;
    hipStream_t s = (hipStream_t)a->stream;
    const int B = a->B, E = a->E, nh = a->nh, R = B * nh, hd = E / nh, hidden = a->hidden;
    const int N = a->T * a->H * a->W;
    float* qp = (float*)(ws + l.qp);
    float* pos_a = a->pe ? (float*)(ws + l.pos_a) : nullptr;
    float* ctxg = (float*)(ws + l.ctxg);
    float *o = (float*)(ws + l.o), *pre = (float*)(ws + l.pre), *hid = (float*)(ws + l.hid), *tok = (float*)(ws + l.tok);

    // 1-2: queries per item
    st = hicom_linear_fwd(a->guide, HICOM_DT_BF16, a->wq, HICOM_DT_BF16, a->bq, HICOM_DT_BF16, nullptr, 0, B, E, E, 0, 0, HICOM_ACT_NONE, qp, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_fold_query_split_fwd(qp, a->wk, a->kpe, B, nh, E, a->P, 1.0f / sqrtf((float)hd), ws + l.qhi, ws + l.qlo, pos_a, a->P, nullptr, 0, 0,
                                    a->stream);
    if (st != HICOM_OK) return st;

    // 3: local stage over the stacked window grid
    {
        const hicom_axis at{B * a->T, a->kt, B * a->T / a->kt, B * a->T / a->kt};
        const hicom_axis ay{a->H, a->ks, a->H / a->ks, a->H / a->ks}, ax{a->W, a->ks, a->W / a->ks, a->W / a->ks};
        HICOM_LAUNCH(batch_local_attn_kernel<3>, dim3((unsigned)((l.rows_all + 3) / 4)), dim3(256), 0, s,
                     (const uint16_t*)(a->fe ? a->fe : a->ff), (const uint16_t*)a->ff, (const uint16_t*)a->guide, at, ay, ax, l.wpi, l.rows_all,
                     a->l_scale, (_Float16*)(ws + l.ctx16));
        st = hicom_host::check_launch("compressor_batch: local stage");
        if (st != HICOM_OK) return st;
    }

    // 4: segmented global stream
    {
        BatchStreamParams p;
        p.x = (const uint16_t*)a->ff; p.N = N; p.ntiles = (N + 15) / 16;
        p.qhi = (const uint16_t*)(ws + l.qhi); p.qlo = (const uint16_t*)(ws + l.qlo);
        p.pos_a = pos_a; p.pos_stride = a->P; p.rows = nh;
        p.H = a->H; p.W = a->W; p.HW = a->H * a->W;
        p.t0i = a->t_index0; p.y0i = a->y_index0; p.x0i = a->x_index0;
        p.scores = (float*)(ws + l.scores); p.score_stride = l.score_stride;
        p.part_m = (float*)(ws + l.part_m); p.part_l = (float*)(ws + l.part_l); p.part_acc = (float*)(ws + l.part_acc);
        constexpr int smem = 2 * 9 * 4096 + 4096;
        static bool attr_set = false;
        if (!attr_set) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(batch_global_stream_kernel<9>), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
            attr_set = true;
        }
        HICOM_LAUNCH(batch_global_stream_kernel<9>, dim3((unsigned)l.chunks, (unsigned)B), dim3(256), smem, s, p);
        st = hicom_host::check_launch("compressor_batch: global stream");
        if (st != HICOM_OK) return st;
    }

    // 5: merge per item
    {
        BatchMergeParams p;
        p.part_m = (const float*)(ws + l.part_m); p.part_l = (const float*)(ws + l.part_l); p.part_acc = (const float*)(ws + l.part_acc);
        p.scores = (const float*)(ws + l.scores); p.score_stride = l.score_stride;
        p.pe = a->pe; p.nparts = l.chunks; p.rows = nh; p.E = E; p.T = a->T; p.H = a->H; p.W = a->W;
        p.t0i = a->t_index0; p.y0i = a->y_index0; p.x0i = a->x_index0;
        p.ctx = ctxg;
        const size_t smem = ((size_t)a->T * a->H + (size_t)a->T * a->W + a->T + a->H + a->W) * 4;
        HICOM_LAUNCH(batch_merge_kernel, dim3((unsigned)nh, (unsigned)B), dim3(256), smem, s, p);
        st = hicom_host::check_launch("compressor_batch: merge");
        if (st != HICOM_OK) return st;
    }

    // 6-9: the global tail with M = B rows
    st = hicom_linear_fwd(ctxg, HICOM_DT_F32, a->wv, HICOM_DT_BF16, a->bv, HICOM_DT_BF16, nullptr, 0, B, E, E, nh, hd, HICOM_ACT_NONE, o, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_linear_fwd(o, HICOM_DT_F32, a->wo, HICOM_DT_BF16, a->bo, HICOM_DT_BF16, a->guide, 2, B, E, E, 0, 0, HICOM_ACT_NONE, pre, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_linear_fwd(pre, HICOM_DT_F32, a->gw0, HICOM_DT_BF16, a->gb0, HICOM_DT_BF16, nullptr, 0, B, hidden, E, 0, 0, HICOM_ACT_GELU, hid, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_linear_fwd(hid, HICOM_DT_F32, a->gw2, HICOM_DT_BF16, a->gb2, HICOM_DT_BF16, nullptr, 0, B, hidden, hidden, 0, 0, HICOM_ACT_NONE, tok, a->stream);
    if (st != HICOM_OK) return st;

    // 10-11: the local readout as one GEMM pair over all items' windows
    st = hicom_readout16_gemm_fwd(ws + l.ctx16, a->lw0_f16, a->lb0, HICOM_DT_BF16, l.rows_all, hidden, E, HICOM_ACT_GELU, ws + l.hid16, nullptr, 0, 0, 0, 0,
                                  nullptr, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_readout16_gemm_fwd(ws + l.hid16, a->lw2_f16, a->lb2, HICOM_DT_BF16, l.rows_all, hidden, hidden, HICOM_ACT_NONE, nullptr, ws + l.loc, a->out_dt,
                                  hidden, 0, 0, nullptr, a->stream);
    if (st != HICOM_OK) return st;

    // 12: every item's packed rows
    {
        BatchPlaceParams p;
        p.loc = ws + l.loc; p.tok = tok; p.newline = (const uint16_t*)a->newline; p.out = a->out;
        p.out_f32 = a->out_dt == HICOM_DT_F32; p.hidden = hidden; p.wpi = l.wpi; p.nl_group = a->nl_group; p.nl_count = a->nl_count;
        p.item_rows = a->item_rows; p.global_row0 = a->global_row0; p.nl_first = a->nl_first; p.nl_step = a->nl_step > 0 ? a->nl_step : 1; p.ldo = a->ldo;
        HICOM_LAUNCH(batch_place_kernel, dim3((unsigned)((long)B * a->item_rows)), dim3(128), 0, s, p);
        st = hicom_host::check_launch("compressor_batch: placement");
    }
    return st;
}
