// Clip stream: a video that arrives in chunks of whole window groups.  The local rows of a chunk are final when the
// chunk has been read; the global stage carries ONE un-normalised online-softmax state (M, L, ACC[rows, E]) of everything pushed so far,
// in the layout hicom_global_combine_fwd reads as one set.  This file has the kernel that folds a chunk's partials (as
// hicom_fused_stream_fwd leaves them) into that state, the kernel that empties it, and hicom_compressor_stream_push: the ring kernel on the
// chunk with its absolute frame offset, the fold and the two readout GEMMs of the chunk's rows in one host call.
#include <math.h>

#include "common.hpp"

namespace hicom {

// e^(m - M') as the weight of a term whose running max is m; an empty term (m = -inf) weighs 0 whatever M' is (no -inf - -inf)
__device__ __forceinline__ float fold_weight(float m, float m_new) { return m == -INFINITY ? 0.f : expf(m - m_new); }

// grid (ceil(E / 256), rows), one wave per workgroup: lane l of slice s owns the four channels 4 (64 s + l) .. + 3 of row blockIdx.y.
// (M, L) goes from ml_in to ml_out (two blocks: every slice of the row reads the old pair), ACC in place.
__global__ __launch_bounds__(64) void stream_state_fold_kernel(const float* __restrict__ part_m, const float* __restrict__ part_l,
                                                               const float* __restrict__ part_acc, int nparts, int rows_pad, int E,
                                                               const float* __restrict__ ml_in, float* __restrict__ ml_out, float* acc) {
    const int r = blockIdx.y;
    const int c = ((int)blockIdx.x * kWave + (int)threadIdx.x) * 4;
    const float m_old = ml_in[2 * r], l_old = ml_in[2 * r + 1];
    float m_new = m_old;
    for (int p = 0; p < nparts; ++p) m_new = fmaxf(m_new, part_m[(long)p * rows_pad + r]);
    const float w_old = fold_weight(m_old, m_new);
    float l_new = w_old * l_old;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    float* dst = acc + (long)r * E + c;
    if (c < E && m_old != -INFINITY) a = *reinterpret_cast<const f32x4*>(dst) * w_old;
    for (int p = 0; p < nparts; ++p) {
        const long pr = (long)p * rows_pad + r;
        const float w = fold_weight(part_m[pr], m_new);
        l_new = fmaf(w, part_l[pr], l_new);
        if (c < E && w != 0.f) a += *reinterpret_cast<const f32x4*>(part_acc + pr * E + c) * w;
    }
    if (c < E) *reinterpret_cast<f32x4*>(dst) = a;
    if (blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<float2*>(ml_out + 2 * r) = make_float2(m_new, l_new);
}

// (M, L) = (-inf, 0) for ml_rows pairs, ACC = 0 for acc_floats floats (a multiple of 4)
__global__ __launch_bounds__(256) void stream_state_clear_kernel(float* ml, int ml_rows, float* acc, long acc_floats) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < ml_rows) *reinterpret_cast<float2*>(ml + 2 * i) = make_float2(-INFINITY, 0.f);
    if (i * 4 < acc_floats) *reinterpret_cast<f32x4*>(acc + i * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
}

}  // namespace hicom

using namespace hicom;

extern "C" int hicom_stream_state_clear_fwd(float* state_ml, int32_t ml_rows, float* state_acc, int64_t acc_floats, void* stream) {
    HICOM_REQUIRE(state_ml && state_acc, HICOM_EINVAL, "stream_state_clear: NULL pointer");
    HICOM_REQUIRE(ml_rows > 0 && acc_floats > 0 && acc_floats % 4 == 0 && (uintptr_t)state_ml % 8 == 0 && (uintptr_t)state_acc % 16 == 0,
                  HICOM_EINVAL, "stream_state_clear: bad shape or alignment (ACC a multiple of 4 floats, 16-byte aligned)");
    const long n = acc_floats / 4 > ml_rows ? acc_floats / 4 : ml_rows;
    hipLaunchKernelGGL(stream_state_clear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, state_ml, ml_rows,
                       state_acc, (long)acc_floats);
    return hicom_host::check_launch("stream_state_clear");
}

extern "C" int hicom_stream_state_fold_fwd(const float* part_m, const float* part_l, const float* part_acc, int32_t nparts, int32_t rows,
                                           int32_t rows_pad, int32_t E, const float* state_ml_in, float* state_ml_out, float* state_acc,
                                           void* stream) {
    HICOM_REQUIRE(part_m && part_l && part_acc && state_ml_in && state_ml_out && state_acc, HICOM_EINVAL, "stream_state_fold: NULL pointer");
    HICOM_REQUIRE(nparts > 0 && rows > 0 && rows <= rows_pad && E > 0 && E % 4 == 0, HICOM_EINVAL,
                  "stream_state_fold: bad shape (nparts=%d rows=%d rows_pad=%d E=%d; E %% 4)", nparts, rows, rows_pad, E);
    HICOM_REQUIRE((uintptr_t)part_acc % 16 == 0 && (uintptr_t)state_acc % 16 == 0 && (uintptr_t)state_ml_in % 8 == 0 &&
                      (uintptr_t)state_ml_out % 8 == 0, HICOM_EINVAL, "stream_state_fold: 16-byte aligned accumulators, 8-byte aligned (M, L)");
    // every slice of a row reads the old (M, L): writing it back into the block being read would race between the row's workgroups
    HICOM_REQUIRE(state_ml_in + 2 * (long)rows <= state_ml_out || state_ml_out + 2 * (long)rows <= state_ml_in, HICOM_EINVAL,
                  "stream_state_fold: state_ml_in and state_ml_out overlap");
    hipLaunchKernelGGL(stream_state_fold_kernel, dim3((unsigned)((E + 4 * kWave - 1) / (4 * kWave)), (unsigned)rows), dim3(kWave), 0,
                       (hipStream_t)stream, part_m, part_l, part_acc, nparts, rows_pad, E, state_ml_in, state_ml_out, state_acc);
    return hicom_host::check_launch("stream_state_fold");
}

extern "C" int hicom_compressor_stream_push(const hicom_stream_push_args* a) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "compressor_stream_push: NULL arguments");
    HICOM_REQUIRE(a->Tc > 0 && a->H > 0 && a->W > 0 && a->kt > 0 && a->ks > 0 && a->hidden > 0 && a->rows > 0 && a->nparts > 0, HICOM_EINVAL,
                  "compressor_stream_push: bad shape");
    HICOM_REQUIRE(a->E == 1152, HICOM_EUNSUP, "compressor_stream_push: E=%d (only 1152)", a->E);
    HICOM_REQUIRE(a->rows <= 12, HICOM_EUNSUP, "compressor_stream_push: %d folded rows (<= 12)", a->rows);
    HICOM_REQUIRE(a->hidden % 64 == 0, HICOM_EUNSUP, "compressor_stream_push: hidden=%d (multiple of 64: fp16 readout planes)", a->hidden);
    HICOM_REQUIRE(a->Tc % a->kt == 0 && a->H % a->ks == 0 && a->W % a->ks == 0, HICOM_EUNSUP,
                  "compressor_stream_push: needs an exact window partition (Tc=%d H=%d W=%d, windows %dx%dx%d)", a->Tc, a->H, a->W, a->kt, a->ks,
                  a->ks);
    const int win = a->kt * a->ks * a->ks;
    HICOM_REQUIRE(win >= 16 && win <= 64, HICOM_EUNSUP, "compressor_stream_push: windows of %d tokens (16 .. 64)", win);
    HICOM_REQUIRE(a->out_dt == HICOM_DT_F32 || a->out_dt == HICOM_DT_BF16, HICOM_EUNSUP, "compressor_stream_push: output dtype %d (bf16 | f32)",
                  a->out_dt);
    HICOM_REQUIRE(a->ff && a->q_hi && a->q_lo && a->part_m && a->part_l && a->part_acc && a->ctx_f16 && a->hid_f16 && a->state_ml_in &&
                      a->state_ml_out && a->state_acc && a->out, HICOM_EINVAL, "compressor_stream_push: NULL pointer");
    HICOM_REQUIRE(a->lw0_f16 && a->lb0 && a->lw2_f16 && a->lb2, HICOM_EINVAL, "compressor_stream_push: NULL weight");
    HICOM_REQUIRE((a->pos_a != nullptr) == (a->pe_hi != nullptr) && (a->pe_hi != nullptr) == (a->pe_lo != nullptr), HICOM_EINVAL,
                  "compressor_stream_push: pos_a, pe_hi and pe_lo come together");
    HICOM_REQUIRE(a->t0 >= 0 && a->t0 % a->kt == 0, HICOM_EINVAL, "compressor_stream_push: t0=%d (whole window groups of %d frames)", a->t0, a->kt);
    if (a->pos_a)
        HICOM_REQUIRE((long)a->t0 + a->Tc <= a->y_index0 && a->y_index0 + a->H <= a->x_index0 && a->x_index0 + a->W <= a->P, HICOM_EINVAL,
                      "compressor_stream_push: frames %d .. %d, grid %dx%d outside the positional tables (t < %d, y at %d, x at %d, %d rows)",
                      a->t0, a->t0 + a->Tc, a->H, a->W, a->y_index0, a->y_index0, a->x_index0, a->P);
    HICOM_REQUIRE((uintptr_t)a->ff % 16 == 0 && (uintptr_t)a->fe % 16 == 0, HICOM_EINVAL, "compressor_stream_push: 16-byte aligned inputs");
    const long nw = (long)(a->Tc / a->kt) * (a->H / a->ks) * (a->W / a->ks);
    HICOM_REQUIRE(nw <= INT32_MAX && a->ldo >= a->hidden && a->row0 >= 0 && a->nl_group >= 0 && (a->nl_group == 0 || nw % a->nl_group == 0),
                  HICOM_EINVAL, "compressor_stream_push: output layout");
    HICOM_REQUIRE(a->nl_count >= 0 && (a->nl_count == 0 || (a->newline && a->nl_first >= a->row0 && a->nl_step > 0)), HICOM_EINVAL,
                  "compressor_stream_push: newline rows");
    // (no frames_embed: the keys are frames_feature, reference projector.py:532 -- the ring kernel streams it as its key tensor too)
    int st = hicom_fused_stream_fwd(a->ff, a->fe ? a->fe : a->ff, nullptr, a->Tc, a->H, a->W, a->E, a->kt, a->ks, a->q_hi, a->q_lo, a->rows, a->l_scale, 0.f,
                                    a->pos_a, a->P, a->pe_hi, a->pe_lo, a->t0, a->y_index0, a->x_index0, a->part_m, a->part_l, a->part_acc,
                                    a->nparts, nullptr, nullptr, nullptr, a->ctx_f16, nullptr, 0, nullptr, nullptr, 0, HICOM_DT_BF16, nullptr,
                                    a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_stream_state_fold_fwd(a->part_m, a->part_l, a->part_acc, a->nparts, a->rows, 16, a->E, a->state_ml_in, a->state_ml_out,
                                     a->state_acc, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_readout16_gemm_fwd(a->ctx_f16, a->lw0_f16, a->lb0, HICOM_DT_BF16, (int32_t)nw, a->hidden, a->E, HICOM_ACT_GELU, a->hid_f16, nullptr, 0,
                                  0, 0, 0, nullptr, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_readout16_gemm_fwd(a->hid_f16, a->lw2_f16, a->lb2, HICOM_DT_BF16, (int32_t)nw, a->hidden, a->hidden, HICOM_ACT_NONE, nullptr, a->out,
                                  a->out_dt, a->ldo, a->row0, a->nl_group, nullptr, a->stream);
    if (st != HICOM_OK || a->nl_count == 0) return st;
    return hicom_scatter_rows_fwd(a->newline, HICOM_DT_BF16, 1, a->hidden, a->out, a->out_dt, a->ldo, a->nl_first, a->nl_step, 0, a->nl_count,
                                  a->stream);
}
