// Clip stream: a video that arrives in chunks of whole window groups.  The local rows of a chunk are final when the
// chunk has been read; the global stage carries ONE un-normalised online-softmax state (M, L, ACC[rows, E]) of everything pushed so far,
// in the layout hicom_global_combine_fwd reads as one set.  This file has the kernel that folds a chunk's partials (as
// hicom_fused_stream_fwd leaves them) into that state, the kernel that empties it, and hicom_compressor_stream_push: the ring kernel on the
// chunk with its absolute frame offset, the fold and the two readout GEMMs of the chunk's rows in one host call.
//
// Several guides per stream: the carried state is one set of nh Q rows; hicom_compressor_stream_push_multi joins the
// multi-guide local kernel, the many-row global stream with t_index0 and its merge with normalize = 0 over time, with two kernels of this
// file: the fold of ONE merged set into the state (the body of the fold above) and the placement of Q x rows packed rows (place_row of
// segment_item.hpp), which finish() uses again for every guide's global rows.
//
// The k / v adaptor recipe: hicom_compressor_stream_push_multi_adapt is the same push with another local stage -- the adaptor
// MLPs over the chunk's tokens (hicom_clip_adapt_prepare_fwd) and the adapt local kernel (hicom_multi_guide_local_adapt_fwd) -- on one body,
// push_multi, which holds the checks and launches 2 ... for both entry points.  The host checks that the three pushes share are chunk_check; the
// two fold entry points share fold_launch.
#include <math.h>

#include "segment_host.hpp"

namespace hicom {

// e^(m - M') as the weight of a term whose running max is m; an empty term (m = -inf) weighs 0 whatever M' is (no -inf - -inf)
__device__ __forceinline__ float fold_weight(float m, float m_new) { return m == -INFINITY ? 0.f : expf(m - m_new); }

// The fold of `nterms` un-normalised terms into row blockIdx.y of the carried state, shared by the two fold kernels: grid (ceil(E / 256),
// rows), one wave per workgroup, lane l of slice s owns the four channels 4 (64 s + l) .. + 3 of the row.  (M, L) goes from ml_in to ml_out
// (two blocks: every slice of the row reads the old pair), ACC in place.  `t` says where term p of row r lives: t.m(p, r), t.l(p, r), and
// t.acc(p, r), its E accumulator floats.
template <class Terms>
__device__ __forceinline__ void fold_row(const Terms& t, int nterms, int E, const float* __restrict__ ml_in, float* __restrict__ ml_out, float* acc) {
    const int r = blockIdx.y;
    const int c = ((int)blockIdx.x * kWave + (int)threadIdx.x) * 4;
    const float m_old = ml_in[2 * r], l_old = ml_in[2 * r + 1];
    float m_new = m_old;
    for (int p = 0; p < nterms; ++p) m_new = fmaxf(m_new, t.m(p, r));
    const float w_old = fold_weight(m_old, m_new);
    float l_new = w_old * l_old;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    float* dst = acc + (long)r * E + c;
    if (c < E && m_old != -INFINITY) a = *reinterpret_cast<const f32x4*>(dst) * w_old;
    for (int p = 0; p < nterms; ++p) {
        const float w = fold_weight(t.m(p, r), m_new);
        l_new = fmaf(w, t.l(p, r), l_new);
        if (c < E && w != 0.f) a += *reinterpret_cast<const f32x4*>(t.acc(p, r) + c) * w;
    }
    if (c < E) *reinterpret_cast<f32x4*>(dst) = a;
    if (blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<float2*>(ml_out + 2 * r) = make_float2(m_new, l_new);
}

// the partials of one chunk as the ring kernel leaves them: part_m / part_l [nparts][rows_pad], part_acc [nparts][rows_pad][E]
struct PartialTerms {
    const float* part_m;
    const float* part_l;
    const float* part_acc;
    int rows_pad, E;
    __device__ __forceinline__ float m(int p, int r) const { return part_m[(long)p * rows_pad + r]; }
    __device__ __forceinline__ float l(int p, int r) const { return part_l[(long)p * rows_pad + r]; }
    __device__ __forceinline__ const float* acc(int p, int r) const { return part_acc + ((long)p * rows_pad + r) * E; }
};

// ONE merged set as the merge kernels write it with normalize = 0: ml [rows][2] = interleaved (M, L), acc [rows][E]
struct SetTerm {
    const float* ml;
    const float* set_acc;
    int E;
    __device__ __forceinline__ float m(int, int r) const { return ml[2 * r]; }
    __device__ __forceinline__ float l(int, int r) const { return ml[2 * r + 1]; }
    __device__ __forceinline__ const float* acc(int, int r) const { return set_acc + (long)r * E; }
};

__global__ __launch_bounds__(64) void stream_state_fold_kernel(const float* __restrict__ part_m, const float* __restrict__ part_l,
                                                               const float* __restrict__ part_acc, int nparts, int rows_pad, int E,
                                                               const float* __restrict__ ml_in, float* __restrict__ ml_out, float* acc) {
    fold_row(PartialTerms{part_m, part_l, part_acc, rows_pad, E}, nparts, E, ml_in, ml_out, acc);
}

__global__ __launch_bounds__(64) void stream_state_fold_set_kernel(const float* __restrict__ set_ml, const float* __restrict__ set_acc, int E,
                                                                   const float* __restrict__ ml_in, float* __restrict__ ml_out, float* acc) {
    fold_row(SetTerm{set_ml, set_acc, E}, 1, E, ml_in, ml_out, acc);
}

// Placement of a multi-guide stream's rows (hicom_stream_place_rows_fwd): grid = Q * rows, one output row per workgroup; guide q's row r
// goes to out[q][row0 + r].  The body is place_row of the many-item steps.
struct StreamPlaceParams {
    SegPlaceParams c;
    int windows, nl_group, nl_count;
    long rows, global_row0, nl_first, nl_step, ldo, q_stride, row0;
};

__global__ __launch_bounds__(128) void stream_place_rows_kernel(StreamPlaceParams p) {
    const long row = blockIdx.x;
    const long q = row / p.rows, r = row - q * p.rows;
    place_row(p.c, r, q * p.q_stride + (p.row0 + r) * p.ldo, q, q * p.windows, p.nl_group, p.nl_count, p.global_row0, p.nl_first, p.nl_step);
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

namespace {

// What the two fold entry points share behind their own NULL and shape checks: the alignment of the terms (`term_acc` their accumulators, `term_ml`
// (M, L) pairs or NULL) and of the state, the (M, L) blocks apart, and the launch of `kernel(terms..., E, state_ml_in, state_ml_out, state_acc)`.
template <class Kernel, class... Terms>
int fold_launch(const char* who, Kernel kernel, const float* term_acc, const float* term_ml, int rows, int E, const float* state_ml_in, float* state_ml_out,
                float* state_acc, void* stream, Terms... terms) {
    HICOM_REQUIRE((uintptr_t)term_acc % 16 == 0 && (uintptr_t)state_acc % 16 == 0 && (uintptr_t)term_ml % 8 == 0 && (uintptr_t)state_ml_in % 8 == 0 &&
                      (uintptr_t)state_ml_out % 8 == 0, HICOM_EINVAL, "%s: 16-byte aligned accumulators, 8-byte aligned (M, L)", who);
    // every slice of a row reads the old (M, L): writing it back into the block being read would race between the row's workgroups
    HICOM_REQUIRE(state_ml_in + 2 * (long)rows <= state_ml_out || state_ml_out + 2 * (long)rows <= state_ml_in, HICOM_EINVAL,
                  "%s: state_ml_in and state_ml_out overlap", who);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((E + 4 * kWave - 1) / (4 * kWave)), (unsigned)rows), dim3(kWave), 0, (hipStream_t)stream, terms..., E,
                       state_ml_in, state_ml_out, state_acc);
    return hicom_host::check_launch(who);
}

// The checks of one chunk that all three pushes make, on the fields their argument blocks share by name (`heads`: the folded rows per guide;
// `has_pos`: the positional tables are in play).  The limits on heads and windows, the pointers and the merge stay with the entry points.
template <class Args>
int chunk_check(const char* who, const Args* a, int heads, bool has_pos) {
    HICOM_REQUIRE(a->Tc > 0 && a->H > 0 && a->W > 0 && a->kt > 0 && a->ks > 0 && a->hidden > 0 && heads > 0 && a->nparts > 0, HICOM_EINVAL, "%s: bad shape", who);
    HICOM_REQUIRE(a->E == 1152, HICOM_EUNSUP, "%s: E=%d (only 1152)", who, a->E);
    HICOM_REQUIRE(a->hidden % 64 == 0, HICOM_EUNSUP, "%s: hidden=%d (multiple of 64: fp16 readout planes)", who, a->hidden);
    HICOM_REQUIRE(a->Tc % a->kt == 0 && a->H % a->ks == 0 && a->W % a->ks == 0, HICOM_EUNSUP,
                  "%s: needs an exact window partition (Tc=%d H=%d W=%d, windows %dx%dx%d)", who, a->Tc, a->H, a->W, a->kt, a->ks, a->ks);
    HICOM_REQUIRE(a->out_dt == HICOM_DT_F32 || a->out_dt == HICOM_DT_BF16, HICOM_EUNSUP, "%s: output dtype %d (bf16 | f32)", who, a->out_dt);
    HICOM_REQUIRE(a->lw0_f16 && a->lb0 && a->lw2_f16 && a->lb2, HICOM_EINVAL, "%s: NULL weight", who);
    HICOM_REQUIRE(a->t0 >= 0 && a->t0 % a->kt == 0, HICOM_EINVAL, "%s: t0=%d (whole window groups of %d frames)", who, a->t0, a->kt);
    if (has_pos)
        HICOM_REQUIRE((long)a->t0 + a->Tc <= a->y_index0 && a->y_index0 + a->H <= a->x_index0 && a->x_index0 + a->W <= a->P, HICOM_EINVAL,
                      "%s: frames %d .. %d, grid %dx%d outside the positional tables (t < %d, y at %d, x at %d, %d rows)", who, a->t0, a->t0 + a->Tc, a->H,
                      a->W, a->y_index0, a->y_index0, a->x_index0, a->P);
    return HICOM_OK;
}

constexpr int kMaxStreamGuides = 32;        // 9 heads x 32 guides = 288 rows: the row count the many-row stream kernel is proven at
constexpr int kMaxStreamParts = 256;        // token chunks of the global stream (the merge keeps a weight per chunk in LDS)

// the layout of `rows` placed rows per guide: `windows` token rows with a newline row behind every nl_group of them (nl_group > 0), or
// the token rows with nl_count newline rows behind them (nl_group == 0), then rows - global_row0 copies of the guide's global row
int place_check(const char* who, const void* loc, const float* tok, const void* newline, int Q, int windows, int hidden, int nl_group, int nl_count,
                long nl_first, long nl_step, long rows, long global_row0, const void* out, int out_dt, long ldo, long q_stride, long row0) {
    HICOM_REQUIRE(out, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE(Q >= 1 && Q <= kMaxStreamGuides, HICOM_EUNSUP, "%s: Q=%d guides (1 <= Q <= %d)", who, Q, kMaxStreamGuides);
    HICOM_REQUIRE(out_dt == HICOM_DT_F32 || out_dt == HICOM_DT_BF16, HICOM_EUNSUP, "%s: output dtype %d (bf16 | f32)", who, out_dt);
    HICOM_REQUIRE(hidden > 0 && windows >= 0 && rows > 0 && rows * Q < (1L << 31) && global_row0 >= 0 && global_row0 <= rows && nl_group >= 0 &&
                      nl_count >= 0 && global_row0 == (long)windows + nl_count && row0 >= 0 && ldo >= hidden &&
                      (row0 + rows) <= q_stride / ldo, HICOM_EINVAL,
                  "%s: output layout (%ld rows per guide at row %ld, %d token rows + %d newline rows, row length %ld, guides %ld elements apart)", who,
                  rows, row0, windows, nl_count, ldo, q_stride);
    HICOM_REQUIRE((windows == 0 || loc) && (global_row0 == rows || tok), HICOM_EINVAL, "%s: NULL pointer", who);
    if (nl_group > 0)
        HICOM_REQUIRE(windows % nl_group == 0 && nl_count == windows / nl_group && newline && nl_first == nl_group && nl_step == nl_group + 1, HICOM_EINVAL,
                      "%s: newline rows (one behind every %d token rows)", who, nl_group);
    else
        HICOM_REQUIRE(nl_count == 0 || (newline && nl_first == windows && nl_step == 1), HICOM_EINVAL, "%s: newline rows (behind the token rows)", who);
    return HICOM_OK;
}

int place_launch(const char* who, const void* loc, const float* tok, const void* newline, int Q, int windows, int hidden, int nl_group, int nl_count,
                 long nl_first, long nl_step, long rows, long global_row0, void* out, int out_dt, long ldo, long q_stride, long row0, void* stream) {
    StreamPlaceParams p;
    p.c.loc = loc; p.c.tok = tok; p.c.newline = (const uint16_t*)newline; p.c.out = out;
    p.c.out_f32 = out_dt == HICOM_DT_F32; p.c.hidden = hidden;
    p.windows = windows; p.nl_group = nl_group; p.nl_count = nl_count;
    p.rows = rows; p.global_row0 = global_row0; p.nl_first = nl_first; p.nl_step = nl_step > 0 ? nl_step : 1;
    p.ldo = ldo; p.q_stride = q_stride; p.row0 = row0;
    hipLaunchKernelGGL(stream_place_rows_kernel, dim3((unsigned)(rows * Q)), dim3(128), 0, (hipStream_t)stream, p);
    return hicom_host::check_launch(who);
}

}  // namespace

extern "C" int hicom_stream_state_fold_fwd(const float* part_m, const float* part_l, const float* part_acc, int32_t nparts, int32_t rows, int32_t rows_pad,
                                           int32_t E, const float* state_ml_in, float* state_ml_out, float* state_acc, void* stream) {
    HICOM_REQUIRE(part_m && part_l && part_acc && state_ml_in && state_ml_out && state_acc, HICOM_EINVAL, "stream_state_fold: NULL pointer");
    HICOM_REQUIRE(nparts > 0 && rows > 0 && rows <= rows_pad && E > 0 && E % 4 == 0, HICOM_EINVAL,
                  "stream_state_fold: bad shape (nparts=%d rows=%d rows_pad=%d E=%d; E %% 4)", nparts, rows, rows_pad, E);
    return fold_launch("stream_state_fold", stream_state_fold_kernel, part_acc, nullptr, rows, E, state_ml_in, state_ml_out, state_acc, stream, part_m, part_l,
                       part_acc, (int)nparts, (int)rows_pad);
}

namespace {

// One push of a single-guide stream, the body of both entry points.  local_logits NULL: the keyed form (hicom_compressor_stream_push).  Given
// (hicom_compressor_stream_push_logits): f32 [Tc H W] in the chunk's own token order, launch 1 is the ring kernel's logits instantiation and
// a->fe is not looked at.  `logits` names the entry, the pointer is its argument: the logits entry must REFUSE a NULL pointer, so NULL cannot
// stand for "the keyed form".  Nothing is launched before every check has passed.
int push_single(const char* who, const hicom_stream_push_args* a, const float* local_logits, bool logits) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "%s: NULL arguments", who);
    if (logits) HICOM_REQUIRE(local_logits && (uintptr_t)local_logits % 4 == 0, HICOM_EINVAL, "%s: local_logits is f32 [Tc H W]", who);
    int st = chunk_check(who, a, a->rows, a->pos_a != nullptr);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->rows <= 12, HICOM_EUNSUP, "%s: %d folded rows (<= 12)", who, a->rows);
    const int win = a->kt * a->ks * a->ks;
    HICOM_REQUIRE(win >= 16 && win <= 64, HICOM_EUNSUP, "%s: windows of %d tokens (16 .. 64)", who, win);
    HICOM_REQUIRE(a->ff && a->q_hi && a->q_lo && a->part_m && a->part_l && a->part_acc && a->ctx_f16 && a->hid_f16 && a->state_ml_in &&
                      a->state_ml_out && a->state_acc && a->out, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE((a->pos_a != nullptr) == (a->pe_hi != nullptr) && (a->pe_hi != nullptr) == (a->pe_lo != nullptr), HICOM_EINVAL,
                  "%s: pos_a, pe_hi and pe_lo come together", who);
    HICOM_REQUIRE((uintptr_t)a->ff % 16 == 0 && (logits || (uintptr_t)a->fe % 16 == 0), HICOM_EINVAL, "%s: 16-byte aligned inputs", who);
    const long nw = (long)(a->Tc / a->kt) * (a->H / a->ks) * (a->W / a->ks);
    HICOM_REQUIRE(nw <= INT32_MAX && a->ldo >= a->hidden && a->row0 >= 0 && a->nl_group >= 0 && (a->nl_group == 0 || nw % a->nl_group == 0),
                  HICOM_EINVAL, "%s: output layout", who);
    HICOM_REQUIRE(a->nl_count >= 0 && (a->nl_count == 0 || (a->newline && a->nl_first >= a->row0 && a->nl_step > 0)), HICOM_EINVAL, "%s: newline rows", who);
    // (no frames_embed: the keys are frames_feature, reference projector.py:532 -- the ring kernel streams it as its key tensor too)
    st = hicom_fused_stream_fwd(a->ff, logits ? nullptr : a->fe ? a->fe : a->ff, local_logits, a->Tc, a->H, a->W, a->E, a->kt, a->ks, a->q_hi, a->q_lo, a->rows, a->l_scale, 0.f,
                                a->pos_a, a->P, a->pe_hi, a->pe_lo, a->t0, a->y_index0, a->x_index0, a->part_m, a->part_l, a->part_acc, a->nparts, nullptr, nullptr,
                                nullptr, a->ctx_f16, nullptr, 0, nullptr, nullptr, 0, HICOM_DT_BF16, nullptr, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_stream_state_fold_fwd(a->part_m, a->part_l, a->part_acc, a->nparts, a->rows, 16, a->E, a->state_ml_in, a->state_ml_out, a->state_acc, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_readout16_gemm_fwd(a->ctx_f16, a->lw0_f16, a->lb0, HICOM_DT_BF16, (int32_t)nw, a->hidden, a->E, HICOM_ACT_GELU, a->hid_f16, nullptr, 0,
                                  0, 0, 0, nullptr, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_readout16_gemm_fwd(a->hid_f16, a->lw2_f16, a->lb2, HICOM_DT_BF16, (int32_t)nw, a->hidden, a->hidden, HICOM_ACT_NONE, nullptr, a->out,
                                  a->out_dt, a->ldo, a->row0, a->nl_group, nullptr, a->stream);
    if (st != HICOM_OK || a->nl_count == 0) return st;
    return hicom_scatter_rows_fwd(a->newline, HICOM_DT_BF16, 1, a->hidden, a->out, a->out_dt, a->ldo, a->nl_first, a->nl_step, 0, a->nl_count, a->stream);
}

}  // namespace

extern "C" int hicom_compressor_stream_push(const hicom_stream_push_args* a) { return push_single("compressor_stream_push", a, nullptr, false); }

// The logits form: the chunk's scores come precomputed (hicom_head_scores_multi_fwd with the stream's one guide); a->fe is not read.
extern "C" int hicom_compressor_stream_push_logits(const hicom_stream_push_args* a, const float* local_logits) {
    return push_single("compressor_stream_push_logits", a, local_logits, true);
}

// ---- several guides per stream ---------------------------------------------------------------------------------------------
extern "C" int hicom_stream_state_fold_set_fwd(const float* set_ml, const float* set_acc, int32_t rows, int32_t E, const float* state_ml_in,
                                               float* state_ml_out, float* state_acc, void* stream) {
    HICOM_REQUIRE(set_ml && set_acc && state_ml_in && state_ml_out && state_acc, HICOM_EINVAL, "stream_state_fold_set: NULL pointer");
    HICOM_REQUIRE(rows > 0 && rows <= 65535 && E > 0 && E % 4 == 0, HICOM_EINVAL, "stream_state_fold_set: bad shape (rows=%d E=%d; E %% 4)", rows, E);
    return fold_launch("stream_state_fold_set", stream_state_fold_set_kernel, set_acc, set_ml, rows, E, state_ml_in, state_ml_out, state_acc, stream, set_ml,
                       set_acc);
}

extern "C" int hicom_stream_place_rows_fwd(const void* loc, const float* tok, const void* newline, int32_t Q, int32_t windows, int32_t hidden,
                                           int32_t nl_group, int32_t nl_count, int64_t nl_first, int64_t nl_step, int64_t rows, int64_t global_row0,
                                           void* out, int32_t out_dt, int64_t ldo, int64_t q_stride, int64_t row0, void* stream) {
    const int st = place_check("stream_place_rows", loc, tok, newline, Q, windows, hidden, nl_group, nl_count, nl_first, nl_step, rows, global_row0, out,
                               out_dt, ldo, q_stride, row0);
    if (st != HICOM_OK) return st;
    return place_launch("stream_place_rows", loc, tok, newline, Q, windows, hidden, nl_group, nl_count, nl_first, nl_step, rows, global_row0, out, out_dt,
                        ldo, q_stride, row0, stream);
}

namespace {

// One push of a multi-guide stream, the body of both entry points: every check of the block, the entry's own checks (`more_checks`), then
// `local` -- the launches that leave the chunk's fp16 contexts in ctx_f16 -- and launches 2 ... of the plain push.  Nothing is launched
// before every check has passed.
template <class Checks, class Local>
int push_multi(const char* who, const hicom_stream_push_multi_args* a, Checks&& more_checks, Local&& local) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "%s: NULL arguments", who);
    HICOM_REQUIRE(a->Q >= 1 && a->Q <= kMaxStreamGuides, HICOM_EUNSUP, "%s: Q=%d guides (1 <= Q <= %d per stream)", who, a->Q, kMaxStreamGuides);
    int st = chunk_check(who, a, a->nh, a->pe != nullptr);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->nh <= 16 && a->E % a->nh == 0, HICOM_EUNSUP, "%s: %d heads (<= 16 folded rows per guide)", who, a->nh);
    HICOM_REQUIRE(a->kt * a->ks * a->ks <= 64, HICOM_EUNSUP, "%s: windows of %d tokens (<= 64)", who, a->kt * a->ks * a->ks);
    const long N = (long)a->Tc * a->H * a->W, ntiles = (N + 15) / 16;
    const long nw = (long)(a->Tc / a->kt) * (a->H / a->ks) * (a->W / a->ks);
    const int rows = a->Q * a->nh, rows_pad = (rows + 31) / 32 * 32;
    HICOM_REQUIRE(N < (1L << 31) / 16 && N * a->Q < (1L << 31) / 16, HICOM_EUNSUP, "%s: too many tokens in one chunk", who);
    HICOM_REQUIRE(a->nparts <= ntiles && a->nparts <= kMaxStreamParts, HICOM_EINVAL, "%s: %d token chunks (<= %ld tiles of 16 tokens, <= %d)", who, a->nparts,
                  ntiles, kMaxStreamParts);
    HICOM_REQUIRE(a->ff && a->guide && a->q_hi && a->q_lo && a->part_m && a->part_l && a->part_acc && a->scores && a->set_ml && a->set_acc && a->ctx_f16 &&
                      a->hid_f16 && a->loc && a->state_ml_in && a->state_ml_out && a->state_acc && a->out, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE((a->pos_a != nullptr) == (a->pe != nullptr) && (!a->pe || a->scratch), HICOM_EINVAL, "%s: pos_a, pe and scratch come together", who);
    HICOM_REQUIRE((uintptr_t)a->ff % 16 == 0 && (uintptr_t)a->fe % 16 == 0 && (uintptr_t)a->guide % 16 == 0 && (uintptr_t)a->q_hi % 16 == 0 &&
                      (uintptr_t)a->q_lo % 16 == 0 && (uintptr_t)a->scores % 16 == 0 && (uintptr_t)a->ctx_f16 % 16 == 0 && (uintptr_t)a->hid_f16 % 16 == 0 &&
                      (uintptr_t)a->loc % 16 == 0 && (uintptr_t)a->lw0_f16 % 16 == 0 && (uintptr_t)a->lw2_f16 % 16 == 0 && (uintptr_t)a->set_acc % 16 == 0 &&
                      (uintptr_t)a->state_acc % 16 == 0 && (uintptr_t)a->part_acc % 16 == 0 && (uintptr_t)a->set_ml % 8 == 0 &&
                      (uintptr_t)a->state_ml_in % 8 == 0 && (uintptr_t)a->state_ml_out % 8 == 0, HICOM_EINVAL,
                  "%s: 16-byte aligned inputs, planes and accumulators, 8-byte aligned (M, L)", who);
    HICOM_REQUIRE(a->state_ml_in + 2 * (long)rows <= a->state_ml_out || a->state_ml_out + 2 * (long)rows <= a->state_ml_in, HICOM_EINVAL,
                  "%s: state_ml_in and state_ml_out overlap", who);
    // the form of the global stage, chosen by the plan; the limits of the two merges (merge.hip), applied to the chunk and the nh Q rows
    if (a->marg) {
        HICOM_REQUIRE(a->pe && hicom_global_stream_has_marg(N, a->E, rows_pad, a->H, a->W, a->nparts) == 1, HICOM_EUNSUP,
                      "%s: no in-kernel marginals for a chunk of %dx%dx%d, %d rows, %d token chunks (hicom_global_stream_has_marg)", who, a->Tc, a->H, a->W,
                      rows_pad, a->nparts);
    } else {
        HICOM_REQUIRE(a->score_stride >= ntiles * 16 && a->score_stride % 4 == 0, HICOM_EINVAL, "%s: score_stride=%ld (>= %ld, %% 4)", who,
                      (long)a->score_stride, ntiles * 16);
        HICOM_REQUIRE(!a->pe || (a->H + a->W <= 1024 && ((a->H <= 32 && a->W <= 32) || ((long)a->H * a->W + a->H + 4) * 4 <= 60000)), HICOM_EUNSUP,
                      "%s: a %dx%d grid: the merge keeps a frame of logits in LDS", who, a->H, a->W);
    }
    HICOM_REQUIRE(((long)a->nparts + (a->pe ? 2L * a->Tc + a->H + a->W + 64L * (a->H + a->W + 2) : 0) + 16 * 64 + 4) * 4 <= 60000, HICOM_EUNSUP,
                  "%s: Tc=%d frames of %dx%d: the merge keeps the row's Tc + H + W weights and 64 frames of marginals in LDS", who, a->Tc, a->H, a->W);
    // the chunk's rows in every guide's part of the output: the placement's own check, with the newline rows made chunk-local
    HICOM_REQUIRE(a->nl_count >= 0 && (a->nl_count == 0 || a->nl_first >= a->row0), HICOM_EINVAL, "%s: newline rows", who);
    const long chunk_rows = nw + a->nl_count;
    st = place_check(who, a->loc, nullptr, a->newline, a->Q, (int)nw, a->hidden, a->nl_group, a->nl_count, a->nl_count ? a->nl_first - a->row0 : 0,
                     a->nl_step, chunk_rows, chunk_rows, a->out, a->out_dt, a->ldo, a->q_stride, a->row0);
    if (st != HICOM_OK) return st;
    st = more_checks();
    if (st != HICOM_OK) return st;

    // 1: local stage
    st = local();
    if (st != HICOM_OK) return st;
    // 2-3: the many-row global stream at the chunk's absolute frame offset and its merge into ONE un-normalised set
    if (a->marg) {
        st = hicom_global_stream_marg_fwd(a->ff, N, a->E, a->q_hi, a->q_lo, rows, rows_pad, a->pos_a, a->P, a->H, a->W, a->t0, a->y_index0, a->x_index0, nullptr, 0,
                                          a->part_m, a->part_l, a->part_acc, a->scores, a->nparts, a->stream);
        if (st != HICOM_OK) return st;
        st = hicom_global_merge_marg_fwd(a->part_m, a->part_l, a->part_acc, a->scores, a->nparts, rows, rows_pad, a->E, N, a->H, a->W, a->pe, a->t0, a->y_index0,
                                         a->x_index0, a->scratch, a->set_ml, a->set_acc, 0, a->stream);
    } else {
        st = hicom_global_stream_fwd(a->ff, N, a->E, a->q_hi, a->q_lo, rows, rows_pad, a->pos_a, a->P, a->H, a->W, a->t0, a->y_index0, a->x_index0, a->scores,
                                     a->score_stride, a->part_m, a->part_l, a->part_acc, a->nparts, a->stream);
        if (st != HICOM_OK) return st;
        st = hicom_global_merge_fwd(a->part_m, a->part_l, a->part_acc, a->nparts, rows, rows_pad, a->E, a->scores, a->score_stride, N, a->H, a->W, a->pe, a->t0,
                                    a->y_index0, a->x_index0, a->scratch, a->set_ml, a->set_acc, 0, a->stream);
    }
    if (st != HICOM_OK) return st;
    // 4: the set into the carried state
    st = hicom_stream_state_fold_set_fwd(a->set_ml, a->set_acc, rows, a->E, a->state_ml_in, a->state_ml_out, a->state_acc, a->stream);
    if (st != HICOM_OK) return st;
    // 5-6: the local readout over all guides' windows
    const int M = (int)(nw * a->Q);
    st = hicom_readout16_gemm_fwd(a->ctx_f16, a->lw0_f16, a->lb0, HICOM_DT_BF16, M, a->hidden, a->E, HICOM_ACT_GELU, a->hid_f16, nullptr, 0, 0, 0, 0, nullptr,
                                  a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_readout16_gemm_fwd(a->hid_f16, a->lw2_f16, a->lb2, HICOM_DT_BF16, M, a->hidden, a->hidden, HICOM_ACT_NONE, nullptr, a->loc, a->out_dt, a->hidden, 0, 0,
                                  nullptr, a->stream);
    if (st != HICOM_OK) return st;
    // 7: guide q's packed rows and the chunk's newline rows to out[q][row0 ..]
    return place_launch(who, a->loc, nullptr, a->newline, a->Q, (int)nw, a->hidden, a->nl_group, a->nl_count, a->nl_count ? a->nl_first - a->row0 : 0, a->nl_step,
                        chunk_rows, chunk_rows, a->out, a->out_dt, a->ldo, a->q_stride, a->row0, a->stream);
}

}  // namespace

extern "C" int hicom_compressor_stream_push_multi(const hicom_stream_push_multi_args* a) {
    // (no frames_embed: the keys are frames_feature, reference projector.py:532)
    return push_multi("compressor_stream_push_multi", a, [] { return (int)HICOM_OK; }, [a] {
        return hicom_multi_guide_local_fwd(a->fe ? a->fe : a->ff, a->ff, a->guide, a->Q, a->Tc, a->H, a->W, a->E, a->kt, a->ks, a->l_scale, a->ctx_f16, a->stream);
    });
}

// The logits form: local_logits f32 [Q][q_stride], guide q's [Tc H W] plane (the chunk's own token order) q_stride floats
// behind guide 0's, as hicom_head_scores_multi_fwd writes it; launch 1 reads the value rows only and a->fe is not looked at.
extern "C" int hicom_compressor_stream_push_multi_logits(const hicom_stream_push_multi_args* a, const float* local_logits, int64_t q_stride) {
    constexpr const char* who = "compressor_stream_push_multi_logits";
    hicom_stream_push_multi_args keyless;
    if (a) {                                    // (the shared checks look at the alignment of fe: an address left from a keyed push is not this entry's business)
        keyless = *a;
        keyless.fe = nullptr;
        a = &keyless;
    }
    return push_multi(
        who, a,
        [&] {
            HICOM_REQUIRE(local_logits && (uintptr_t)local_logits % 4 == 0, HICOM_EINVAL, "%s: local_logits is f32 [Q][Tc H W]", who);
            HICOM_REQUIRE(q_stride >= (int64_t)a->Tc * a->H * a->W, HICOM_EINVAL, "%s: q_stride=%ld floats between the guides' logit planes of %ld tokens", who,
                          (long)q_stride, (long)a->Tc * a->H * a->W);
            return (int)HICOM_OK;
        },
        [&] {
            const hicom_axis at{a->Tc, a->kt, a->Tc / a->kt, a->Tc / a->kt}, ay{a->H, a->ks, a->H / a->ks, a->H / a->ks}, ax{a->W, a->ks, a->W / a->ks, a->W / a->ks};
            return hicom_multi_guide_local_logits_fwd(a->ff, local_logits, q_stride, at, ay, ax, a->Q, at.nwin * ay.nwin * ax.nwin, a->l_scale, a->ctx_f16, a->stream);
        });
}

// ---- the k / v adaptor recipe: the adaptor MLPs over the chunk's tokens, then the adapt local stage, in front of launches 2 ...
extern "C" int hicom_compressor_stream_push_multi_adapt(const hicom_stream_push_multi_adapt_args* x) {
    constexpr const char* who = "compressor_stream_push_multi_adapt";
    HICOM_REQUIRE(x, HICOM_EINVAL, "%s: NULL arguments", who);
    const hicom_stream_push_multi_args* a = &x->base;
    const void* key_x = a->fe ? a->fe : a->ff;             // (no frames_embed: the k adaptor reads frames_feature, as the keys do)
    const long N = (long)a->Tc * a->H * a->W;
    return push_multi(
        who, a,
        [&] {
            HICOM_REQUIRE((x->ky != nullptr) == (x->ak.w0 != nullptr) && (x->vy != nullptr) == (x->av.w0 != nullptr), HICOM_EINVAL,
                          "%s: a plane and its adaptor come together (ky with ak.w0, vy with av.w0)", who);
            const int st = hicom_host::multi_guide_local_adapt_args_check(key_x, a->ff, a->guide, x->ky, x->vy, &x->ak, &x->av, x->alpha_dt, a->Q, a->Tc, a->H,
                                                                          a->W, a->E, a->kt, a->ks, a->ctx_f16);
            if (st != HICOM_OK) return st;
            return hicom_host::clip_adapt_prepare_args_check(key_x, a->ff, N, a->E, &x->ak, &x->av, x->ky, x->vy, x->adapt_ws, x->adapt_ws_bytes, nullptr);
        },
        [&] {
            const int st = hicom_clip_adapt_prepare_fwd(key_x, a->ff, N, a->E, &x->ak, &x->av, x->ky, x->vy, x->adapt_ws, x->adapt_ws_bytes, a->stream);
            if (st != HICOM_OK) return st;
            return hicom_multi_guide_local_adapt_fwd(key_x, a->ff, a->guide, x->ky, x->vy, &x->ak, &x->av, x->alpha_dt, x->eps, a->Q, a->Tc, a->H, a->W, a->E,
                                                     a->kt, a->ks, a->l_scale, a->ctx_f16, a->stream);
        });
}
