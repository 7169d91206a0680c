// Dev tool (tools/executor_trace/run.py): everything hicom_amd/csrc/executor.hip leaves undefined, as stubs that LOG the call -- name,
// every argument, role / gemv / gemm structs field by field, the stop event a launch would carry -- plus a fixed matrix of
// hicom_compressor_args (fake, distinct pointer constants: nothing is dereferenced) fed through the executor's entry points.  Two
// executor.hip that print the same log enqueue the same launches with the same arguments on the same streams in the same order.
// Host only: no device code, no GPU.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/hicom_hip.h"

namespace {

char g_error[1024];
void* g_stop_event;
int g_launches, g_fail_at;      // STUB_FAIL_AT=n: the n-th launch of a case returns HICOM_ELAUNCH (error propagation)

void put(const void* p) { p ? printf("%#llx", (unsigned long long)(uintptr_t)p) : printf("0"); }
void put(int32_t v) { printf("%d", v); }
void put(uint32_t v) { printf("%uu", v); }
void put(int64_t v) { printf("%lldL", (long long)v); }
void put(size_t v) { printf("%lluUL", (unsigned long long)v); }
void put(float v) { printf("%.9gf", v); }
void put(hicom_axis x) { printf("axis{%d %d %d %d}", x.n, x.k, x.nwin, x.nfull); }
void put(const hicom_aux_gemv& g);      // (the struct printers: declared in front of the template that has to find them)
void put(const hicom_aux_gemv* g);
void put(const hicom_r16_role* r);
void put(const hicom_r16_gemm* g);
template <class... A>
void put_all(A... a) {
    int i = 0;
    ((printf(i++ ? ", " : ""), put(a)), ...);
}
void put(const hicom_aux_gemv& g) {
    printf("gemv{");
    put_all(g.xs, g.x_parts, g.x_stride, g.xb, g.w, g.b, g.res, g.N, g.K, g.act, g.y, g.w_dt, g.b_dt, g.rows_dst, g.rows_dt, g.rows_reps, g.rows_ld,
            g.rows_row0, g.x_fixed, g.x_fixed_clear);
    printf("}");
}
void put(const hicom_aux_gemv* g) { g ? put(*g) : put((const void*)nullptr); }
void put(const hicom_r16_role* r) {
    if (!r) return put((const void*)nullptr);
    printf("role{");
    put_all(r->kind, r->gemv, r->gemv2, r->chain_state, r->part_m, r->part_l, r->part_acc, r->part_dt, r->nparts, r->rows, r->rows_pad, r->E, r->w_v,
            r->o_fix, r->out_ml, r->out_ctx, r->ctx_unnorm, r->part_marg, r->vpe_f16, r->marg_slots);
    printf("}");
}
void put(const hicom_r16_gemm* g) {
    if (!g) return put((const void*)nullptr);
    printf("gemm{");
    put_all(g->a, g->w, g->b, g->b_dt, g->M, g->N, g->K, g->act, g->out_f16, g->y, g->y_dt, g->ldy, g->row0, g->nl_group);
    printf("}");
}

template <class... A>
void log_call(const char* name, A... a) {
    printf("    %s(", name);
    put_all(a...);
    printf(")");
}
// a kernel launch: consumes the pending stop event as HICOM_LAUNCH does
template <class... A>
int launch(const char* name, A... a) {
    log_call(name, a...);
    if (g_stop_event) printf(" stop_event=%#llx", (unsigned long long)(uintptr_t)g_stop_event);
    g_stop_event = nullptr;
    const int rc = (++g_launches == g_fail_at) ? HICOM_ELAUNCH : HICOM_OK;
    printf(rc ? " -> %d\n" : "\n", rc);
    return rc;
}
bool env_is(const char* name, char c) { return getenv(name) && getenv(name)[0] == c; }

}  // namespace

namespace hicom_host {
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
void set_stop_event(void* ev) {
    log_call("set_stop_event", (const void*)ev);
    printf("\n");
    g_stop_event = ev;
}
void* take_stop_event() {
    void* ev = g_stop_event;
    g_stop_event = nullptr;
    return ev;
}
}  // namespace hicom_host

hipError_t hipEventRecord(hipEvent_t ev, hipStream_t st) { return launch("hipEventRecord", (const void*)ev, (const void*)st) ? hipErrorUnknown : hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t ev, unsigned flags) {
    return launch("hipStreamWaitEvent", (const void*)st, (const void*)ev, flags) ? hipErrorUnknown : hipSuccess;
}
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus* s) {      // STUB_CAPTURING=1: the main stream is being captured
    *s = env_is("STUB_CAPTURING", '1') ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t st) { return launch("hipStreamSynchronize", (const void*)st) ? hipErrorUnknown : hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t st) {
    memset(dst, 0, n);
    return launch("hipMemcpyAsync", src, n, (const void*)st) ? hipErrorUnknown : hipSuccess;
}

extern "C" {

// run.py --coverage writes a call of this in front of every launch call site of the executor.hip it compiles: the lines that ran go to $STUB_HITS
int hicom_trace_hit(int line) {
    static FILE* f = getenv("STUB_HITS") ? fopen(getenv("STUB_HITS"), "a") : nullptr;
    if (f) fprintf(f, "%d\n", line);
    return 0;
}

// size queries: the formulas of fused_ring.hip / global_stream.hip / query_prep.hip / readout16.hip on a 256-CU device, without their dev switches
int hicom_fused_stream_nparts(int32_t n_windows) {
    if (n_windows <= 0) return HICOM_EINVAL;
    int wpw = (n_windows + 255) / 256;
    if (wpw > 32) wpw = 32;
    return (n_windows + wpw - 1) / wpw;
}
int hicom_global_stream_nparts(int64_t N, int32_t rows_pad) {
    if (N <= 0 || rows_pad <= 0) return HICOM_EINVAL;
    const long ntiles = (N + 15) / 16;
    const int groups = rows_pad / 16;
    long want = 2L * 256 / (groups > 0 ? groups : 1);
    if (rows_pad % 32 == 0 && rows_pad > 16) want = 256L / (groups / 2);
    if (want < 1) want = 1;
    const long cap = ntiles / 4 < 1 ? 1 : ntiles / 4;
    return (int)(want < cap ? want : cap);
}
int hicom_global_stream_marg_width(int32_t H, int32_t W) { return H <= 0 || W <= 0 ? HICOM_EINVAL : 16 * (1 + (H + 15) / 16 + (W + 15) / 16); }
int hicom_global_stream_has_marg(int64_t N, int32_t E, int32_t rows_pad, int32_t H, int32_t W, int32_t nparts) {
    if (N <= 0 || nparts <= 0 || rows_pad <= 0 || H <= 0 || W <= 0) return HICOM_EINVAL;
    if (N % ((long)H * W) != 0) return 0;
    const long T = N / ((long)H * W), ntiles = (N + 15) / 16, HW = (long)H * W;
    if (2 + (long)nparts + T + H + W > T * (H + W + 2)) return 0;
    const bool span_ok = (((ntiles + nparts - 1) / nparts + 1) * 16 + HW - 1) / HW + 1 <= 8;
    return E == 1152 && rows_pad > 16 && rows_pad % 32 == 0 && H <= 64 && W <= 64 && span_ok && 1 + (H + 15) / 16 + (W + 15) / 16 <= 8;
}
int64_t hicom_query_prep_state_bytes(int32_t E) { return (int64_t)E * 8 + 256; }
int64_t hicom_r16_chain_state_bytes(int32_t n_mid) { return n_mid > 0 ? (int64_t)n_mid * 8 + 256 : HICOM_EINVAL; }
int64_t hicom_readout_tail_state_bytes(void) { return (int64_t)(2 + 64) * 128 + 256 * 8; }

// STUB_TAIL_EUNSUP=1: the fused tail launch declines the shape (the executor then issues the two role launches)
int hicom_readout_tail_fwd(const hicom_r16_gemm* g1, const hicom_r16_gemm* g2, const hicom_r16_role* merge, const hicom_r16_role* chain, void* state,
                           void* stream) {
    if (env_is("STUB_TAIL_EUNSUP", '1')) {
        log_call("hicom_readout_tail_fwd", g1, g2, merge, chain, state, stream);
        printf(" -> %d\n", HICOM_EUNSUP);
        return HICOM_EUNSUP;
    }
    return launch("hicom_readout_tail_fwd", g1, g2, merge, chain, state, stream);
}

int hicom_dense16_gemm_fwd(const void* a, int64_t lda, const void* w, int64_t ldw, int32_t operand_dt, const void* b, int32_t b_dt, int32_t M, int32_t
    N, int32_t K, int32_t act, void* out_f16, int64_t ldo, int32_t n_store, void* pre_f16, int64_t ldpre, void* y, int32_t y_dt, int64_t ldy, const
    void* res, int64_t ldr, float* ssq, const float* row_tab, int64_t row_tab_ld, int32_t tab_H, int32_t tab_W, int32_t tab_t0, int32_t tab_y0,
    int32_t tab_x0, const void* dot_vec, int32_t dot_vec_dt, float* row_dot, void* stream) { return launch("hicom_dense16_gemm_fwd", a, lda, w, ldw,
    operand_dt, b, b_dt, M, N, K, act, out_f16, ldo, n_store, pre_f16, ldpre, y, y_dt, ldy, res, ldr, ssq, row_tab, row_tab_ld, tab_H, tab_W, tab_t0,
    tab_y0, tab_x0, dot_vec, dot_vec_dt, row_dot, stream); }
int hicom_dense16_gemm_pair_fwd(const void* a_k, const void* w_k, const void* b_k, void* out_k, void* pre_k, const void* a_v, const void* w_v, const
    void* b_v, void* out_v, void* pre_v, int64_t lda, int64_t ldw, int32_t operand_dt, int32_t b_dt, int32_t M, int32_t N, int32_t K, int32_t act,
    int64_t ldo, int32_t n_store, int64_t ldpre, void* stream) { return launch("hicom_dense16_gemm_pair_fwd", a_k, w_k, b_k, out_k, pre_k, a_v, w_v,
    b_v, out_v, pre_v, lda, ldw, operand_dt, b_dt, M, N, K, act, ldo, n_store, ldpre, stream); }
int hicom_fold_query_split_fwd(const float* qp, const void* w_k, const float* kpe, int32_t nq, int32_t nh, int32_t E, int32_t P, float scale, void*
    qt_hi, void* qt_lo, float* pos_a, int32_t pos_stride, const void* fill_row, int32_t fill_row0, int32_t fill_rows, void* stream) { return
    launch("hicom_fold_query_split_fwd", qp, w_k, kpe, nq, nh, E, P, scale, qt_hi, qt_lo, pos_a, pos_stride, fill_row, fill_row0, fill_rows, stream);
    }
int hicom_fused_stream_fwd(const void* ff, const void* fe, const float* local_logits, int32_t T, int32_t H, int32_t W, int32_t E, int32_t kt, int32_t
    ks, const void* q_hi, const void* q_lo, int32_t rows, float l_scale, float l_bias, const float* pos_a, int32_t pos_stride, const void* pe_hi,
    const void* pe_lo, int32_t t_index0, int32_t y_index0, int32_t x_index0, float* part_m, float* part_l, float* part_acc, int32_t nparts, float*
    ctx_local, void* ctx_hi, void* ctx_lo, void* ctx_f16, void* zero_ptr, int64_t zero_bytes, void* part_ctx_f16, void* part_marg_f16, int32_t
    marg_slots, int32_t tok_dt, const float* q_f32, void* stream) { return launch("hicom_fused_stream_fwd", ff, fe, local_logits, T, H, W, E, kt, ks,
    q_hi, q_lo, rows, l_scale, l_bias, pos_a, pos_stride, pe_hi, pe_lo, t_index0, y_index0, x_index0, part_m, part_l, part_acc, nparts, ctx_local,
    ctx_hi, ctx_lo, ctx_f16, zero_ptr, zero_bytes, part_ctx_f16, part_marg_f16, marg_slots, tok_dt, q_f32, stream); }
int hicom_gemv_chain_fwd(const hicom_r16_role* role, void* stream) { return launch("hicom_gemv_chain_fwd", role, stream); }
int hicom_global_combine_strided_fwd(const float* ml, const float* acc, int64_t set_stride, int32_t nsets, int32_t rows, int32_t E, float* ctx, void*
    stream) { return launch("hicom_global_combine_strided_fwd", ml, acc, set_stride, nsets, rows, E, ctx, stream); }
int hicom_global_merge_fwd(const float* part_m, const float* part_l, const float* part_acc, int32_t nparts, int32_t rows, int32_t rows_pad, int32_t E,
    const float* scores, int64_t score_stride, int64_t N, int32_t H, int32_t W, const float* pe, int32_t t_index0, int32_t y_index0, int32_t x_index0,
    float* scratch, float* out_ml, float* out_acc, int32_t normalize, void* stream) { return launch("hicom_global_merge_fwd", part_m, part_l,
    part_acc, nparts, rows, rows_pad, E, scores, score_stride, N, H, W, pe, t_index0, y_index0, x_index0, scratch, out_ml, out_acc, normalize,
    stream); }
int hicom_global_merge_marg_fwd(const float* part_m, const float* part_l, const float* part_acc, const float* part_marg, int32_t nparts, int32_t rows,
    int32_t rows_pad, int32_t E, int64_t N, int32_t H, int32_t W, const float* pe, int32_t t_index0, int32_t y_index0, int32_t x_index0, float*
    scratch, float* out_ml, float* out_acc, int32_t normalize, void* stream) { return launch("hicom_global_merge_marg_fwd", part_m, part_l, part_acc,
    part_marg, nparts, rows, rows_pad, E, N, H, W, pe, t_index0, y_index0, x_index0, scratch, out_ml, out_acc, normalize, stream); }
int hicom_global_stream_fwd(const void* x, int64_t N, int32_t E, const void* qt_hi, const void* qt_lo, int32_t rows, int32_t rows_pad, const float*
    pos_a, int32_t pos_stride, int32_t H, int32_t W, int32_t t_index0, int32_t y_index0, int32_t x_index0, float* scores, int64_t score_stride, float*
    part_m, float* part_l, float* part_acc, int32_t nparts, void* stream) { return launch("hicom_global_stream_fwd", x, N, E, qt_hi, qt_lo, rows,
    rows_pad, pos_a, pos_stride, H, W, t_index0, y_index0, x_index0, scores, score_stride, part_m, part_l, part_acc, nparts, stream); }
int hicom_global_stream_marg_fwd(const void* x, int64_t N, int32_t E, const void* qt_hi, const void* qt_lo, int32_t rows, int32_t rows_pad, const
    float* pos_a, int32_t pos_stride, int32_t H, int32_t W, int32_t t_index0, int32_t y_index0, int32_t x_index0, float* scores, int64_t score_stride,
    float* part_m, float* part_l, float* part_acc, float* part_marg, int32_t nparts, void* stream) { return launch("hicom_global_stream_marg_fwd", x,
    N, E, qt_hi, qt_lo, rows, rows_pad, pos_a, pos_stride, H, W, t_index0, y_index0, x_index0, scores, score_stride, part_m, part_l, part_acc,
    part_marg, nparts, stream); }
int hicom_linear_fwd(const void* x, int32_t x_dt, const void* w, int32_t w_dt, const void* b, int32_t b_dt, const void* res, int32_t res_flags,
    int32_t M, int32_t N, int32_t K, int32_t head_rows, int32_t head_dim, int32_t act, float* y, void* stream) { return launch("hicom_linear_fwd", x,
    x_dt, w, w_dt, b, b_dt, res, res_flags, M, N, K, head_rows, head_dim, act, y, stream); }
int hicom_linear_to_rows_fwd(const void* x, int32_t x_dt, const void* w, int32_t w_dt, const void* b, int32_t b_dt, int32_t M, int32_t N, int32_t K,
    int32_t act, void* dst, int32_t dst_dt, int64_t ldd, int64_t row0, int32_t n_rows, void* stream) { return launch("hicom_linear_to_rows_fwd", x,
    x_dt, w, w_dt, b, b_dt, M, N, K, act, dst, dst_dt, ldd, row0, n_rows, stream); }
int hicom_local_attn_adapt_fwd(const void* key_x, const void* key_y, const void* k_gamma, const void* k_beta, const void* k_alpha, const void*
    value_x, const void* value_y, const void* v_gamma, const void* v_beta, const void* v_alpha, int32_t alpha_dt, float eps, int32_t D, hicom_axis at,
    hicom_axis ay, hicom_axis ax, const void* query, int32_t query_dt, int64_t query_stride, float scale, float bias, float* ctx, void* stream) {
    return launch("hicom_local_attn_adapt_fwd", key_x, key_y, k_gamma, k_beta, k_alpha, value_x, value_y, v_gamma, v_beta, v_alpha, alpha_dt, eps, D,
    at, ay, ax, query, query_dt, query_stride, scale, bias, ctx, stream); }
int hicom_local_attn_fwd(const void* key, int32_t key_dt, const void* value, int32_t value_dt, int32_t D, hicom_axis at, hicom_axis ay, hicom_axis ax,
    const void* query, int32_t query_dt, int64_t query_stride, float scale, float bias, int32_t l2norm, float* ctx, void* ctx_f16, void* stream) {
    return launch("hicom_local_attn_fwd", key, key_dt, value, value_dt, D, at, ay, ax, query, query_dt, query_stride, scale, bias, l2norm, ctx,
    ctx_f16, stream); }
int hicom_merge_vproj_fixed_fwd(const float* part_m, const float* part_l, const void* part_acc, int32_t part_dt, int32_t nparts, int32_t rows, int32_t
    rows_pad, int32_t E, const void* w_v, int64_t* o_fix, float* out_ml, float* out_ctx, void* stream) { return launch("hicom_merge_vproj_fixed_fwd",
    part_m, part_l, part_acc, part_dt, nparts, rows, rows_pad, E, w_v, o_fix, out_ml, out_ctx, stream); }
int hicom_merge_vproj_sets_fwd(const float* sets, int64_t set_stride, int32_t nsets, int32_t rows, int32_t E, const void* w_v, int64_t* o_fix, float*
    out_ml, float* out_ctx, void* stream) { return launch("hicom_merge_vproj_sets_fwd", sets, set_stride, nsets, rows, E, w_v, o_fix, out_ml, out_ctx,
    stream); }
int hicom_place_blocks_fwd(const void* src, int32_t block_rows, int32_t nblocks, int64_t block_stride_bytes, int32_t row_bytes, void* dst, int64_t
    ldd_bytes, int64_t row0, int32_t nl_group, void* stream) { return launch("hicom_place_blocks_fwd", src, block_rows, nblocks, block_stride_bytes,
    row_bytes, dst, ldd_bytes, row0, nl_group, stream); }
int hicom_planes_gemm_fwd(const void* a_hi, const void* a_lo, const void* w, const void* b, int32_t b_dt, int32_t M, int32_t N, int32_t K, int32_t
    act, void* out_hi, void* out_lo, void* y, int32_t y_dt, int64_t ldy, int64_t row0, int32_t nl_group, void* stream) { return
    launch("hicom_planes_gemm_fwd", a_hi, a_lo, w, b, b_dt, M, N, K, act, out_hi, out_lo, y, y_dt, ldy, row0, nl_group, stream); }
int hicom_query_prep_fwd(const void* guide, const void* local_q, const void* w_q, const void* b_q, const void* w_k, const float* kpe, int32_t nh,
    int32_t E, int32_t P, float scale, void* qt_hi, void* qt_lo, float* pos_a, int32_t pos_stride, int32_t rows, const void* g_w0, const void* g_b0,
    const void* b_o, int32_t hidden, float* r0, void* state, int32_t g_dt, float* qt_f32, void* stream) { return launch("hicom_query_prep_fwd", guide,
    local_q, w_q, b_q, w_k, kpe, nh, E, P, scale, qt_hi, qt_lo, pos_a, pos_stride, rows, g_w0, g_b0, b_o, hidden, r0, state, g_dt, qt_f32, stream); }
int hicom_readout16_gemm_fwd(const void* a, const void* w, const void* b, int32_t b_dt, int32_t M, int32_t N, int32_t K, int32_t act, void* out_f16,
    void* y, int32_t y_dt, int64_t ldy, int64_t row0, int32_t nl_group, const hicom_aux_gemv* aux, void* stream) { return
    launch("hicom_readout16_gemm_fwd", a, w, b, b_dt, M, N, K, act, out_f16, y, y_dt, ldy, row0, nl_group, aux, stream); }
int hicom_readout16_gemm_role_fwd(const void* a, const void* w, const void* b, int32_t b_dt, int32_t M, int32_t N, int32_t K, int32_t act, void*
    out_f16, void* y, int32_t y_dt, int64_t ldy, int64_t row0, int32_t nl_group, const hicom_r16_role* role, void* stream) { return
    launch("hicom_readout16_gemm_role_fwd", a, w, b, b_dt, M, N, K, act, out_f16, y, y_dt, ldy, row0, nl_group, role, stream); }
int hicom_readout_gemm_fwd(const float* x, const void* w, const void* b, int32_t b_dt, int32_t M, int32_t N, int32_t K, int32_t act, void* y, int32_t
    y_dt, int64_t ldy, int64_t row0, int32_t nl_group, void* stream) { return launch("hicom_readout_gemm_fwd", x, w, b, b_dt, M, N, K, act, y, y_dt,
    ldy, row0, nl_group, stream); }
int hicom_row_ln_fwd(const void* x, int32_t x_dt, int64_t x_stride, const float* mul, int64_t mul_stride, const float* add, int64_t add_stride, const
    void* gamma, const void* beta, int32_t gb_dt, const void* src, int32_t src_dt, int64_t src_stride, const void* alpha, int32_t alpha_dt, float eps,
    void* out, int32_t out_dt, int64_t out_stride, int32_t M, int32_t E, void* stream) { return launch("hicom_row_ln_fwd", x, x_dt, x_stride, mul,
    mul_stride, add, add_stride, gamma, beta, gb_dt, src, src_dt, src_stride, alpha, alpha_dt, eps, out, out_dt, out_stride, M, E, stream); }
int hicom_scatter_rows_fwd(const void* src, int32_t src_dt, int32_t src_rows, int32_t ncols, void* dst, int32_t dst_dt, int64_t ldd, int64_t row0,
    int64_t row_step, int32_t nl_group, int32_t count, void* stream) { return launch("hicom_scatter_rows_fwd", src, src_dt, src_rows, ncols, dst,
    dst_dt, ldd, row0, row_step, nl_group, count, stream); }
int hicom_small_mha_fwd(const float* q, const float* k, const float* v, int32_t M, int32_t L, int32_t nh, int32_t hd, float* out, void* stream) {
    return launch("hicom_small_mha_fwd", q, k, v, M, L, nh, hd, out, stream); }
int hicom_to_f16_fwd(const void* src, int32_t src_dt, void* dst, int64_t n, void* stream) { return launch("hicom_to_f16_fwd", src, src_dt, dst, n,
    stream); }
int hicom_trilinear_pool_fwd(const void* x, int32_t T, int32_t H, int32_t W, int32_t D, int32_t To, int32_t Ho, int32_t Wo, float* out, void* stream)
    { return launch("hicom_trilinear_pool_fwd", x, T, H, W, D, To, Ho, Wo, out, stream); }
}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------------
// the matrix
namespace {

// fake device pointers: one 16-MiB slot per name, so every argument of the log can be told apart (nothing reads through them)
void* fake(int slot) { return (void*)((uintptr_t)0x100000000000ull + (uintptr_t)slot * 0x1000000ull); }
int g_slot;
template <class T>
void fill(T*& p) { p = (T*)fake(++g_slot); }
template <class... P>
void fill_all(P&... p) { (fill(p), ...); }

int fake_allgather(const void* send, void* recv, size_t n, int dt, void* comm, hipStream_t st) {
    return launch("ncclAllGather", send, recv, n, dt, (const void*)comm, (const void*)st);
}
int fake_group_start() { return launch("ncclGroupStart"); }
int fake_group_end() { return launch("ncclGroupEnd"); }

hicom_axis axis(int n, int k) { return hicom_axis{n, k, n / k, n / k}; }

// the release recipe (local43_global32, use_guide = direct): T x 27 x 27 tokens of 1152, windows of 4 x 3 x 3, one query row per head
hicom_compressor_args release(int T, int hidden) {
    hicom_compressor_args a;
    memset(&a, 0, sizeof(a));
    g_slot = 0;
    fill_all(a.ff, a.fe, a.lq, a.lw0, a.lb0, a.lw2, a.lb2, a.lw0_f16, a.lw2_f16, a.gq, a.wq, a.bq, a.wk, a.wv, a.bv, a.wo, a.bo, a.gw0, a.gb0, a.gw2, a.gb2,
             a.pe, a.kpe, a.pe_hi, a.pe_lo, a.out, a.ws, a.stream_main, a.stream_side, a.ev_fork, a.ev_join, a.gc0);
    a.T = T; a.H = a.W = 27; a.E = 1152;
    a.has_local = a.has_global = 1;
    a.phases = HICOM_PHASE_STREAM | HICOM_PHASE_FINISH;
    a.hidden = hidden;
    a.at = axis(T, 4); a.ay = a.ax = axis(27, 3);
    a.l_scale = 0.25f; a.l_bias = -0.5f;
    a.nq = 1; a.nh = 9; a.n_global_rows = 32; a.P = T + 54;
    a.t_index0 = 1; a.y_index0 = 2; a.x_index0 = 3;
    a.ldo = hidden; a.local_row0 = 32; a.global_row0 = 0;
    a.ws_bytes = (int64_t)1 << 40;
    return a;
}
// guide off (`nq` learnable query rows per head, pooled local queries): the two-kernel form
hicom_compressor_args generic(int T, int nq) {
    hicom_compressor_args a = release(T, 896);
    a.lq = nullptr;
    a.nq = nq; a.n_global_rows = 32;
    a.gc0 = nullptr;
    fill(a.ev_merge);
    return a;
}
void with_newlines(hicom_compressor_args& a) {
    fill(a.newline);
    a.nl_count = 9 * a.at.nwin; a.nl_group = 9; a.nl_first = 32 + 9; a.nl_step = 10;
}
void with_ring_marg(hicom_compressor_args& a) {
    fill(a.vpe_f16);
    a.marg_slots = 8 * (a.E / 64);
}
// STREAM block of a frame-sharded step
void shard_stream(hicom_compressor_args& a, bool next_is_main, bool r0_buf) {
    a.phases = HICOM_PHASE_STREAM | HICOM_PHASE_MERGE_ON_NEXT | (next_is_main ? HICOM_PHASE_NEXT_IS_MAIN : 0);
    fill_all(a.state_out, a.local_out, a.ev_done);
    if (!next_is_main) fill(a.stream_next);
    if (r0_buf) fill(a.r0_buf);
}
// FINISH block of a frame-sharded step
void shard_finish(hicom_compressor_args& a, bool r0_buf) {
    a.phases = HICOM_PHASE_FINISH;
    fill(a.state_sets);
    a.nsets = 4; a.state_set_stride = 2 * 9 + 9 * 1152;
    fill(a.ev_done);
    if (r0_buf) fill(a.r0_buf);
}
void with_allgather(hicom_compressor_args& a, bool two) {
    a.ag_fn = (void*)&fake_allgather;
    fill_all(a.ag_comm, a.ag_send, a.ag_recv);
    a.ag_bytes = 4096;
    if (two) {
        a.ag_group_start = (void*)&fake_group_start; a.ag_group_end = (void*)&fake_group_end;
        fill_all(a.ag_send2, a.ag_recv2);
        a.ag_bytes2 = 512;
    }
}
void with_place(hicom_compressor_args& a) {
    fill(a.place_src);
    a.place_block_rows = 324; a.place_nblocks = 4; a.place_block_stride = 324 * 896 * 2;
}
void with_adaptor(hicom_compressor_args::hicom_adaptor& ad, bool y) {
    fill_all(ad.w0, ad.b0, ad.w2_f16, ad.b2, ad.gamma, ad.beta, ad.alpha);
    if (y) fill(ad.y);
}
void with_injector(hicom_compressor_args::hicom_injector& j, int mode, bool global) {
    j.mode = mode;
    fill_all(j.guide, j.c_w0, j.c_b0, j.c_w2, j.c_b2, j.wq, j.bq, j.wk, j.bk, j.wv, j.bv, j.wo, j.bo, j.ln_w, j.ln_b);
    j.guide_rows = mode == 1 ? 1 : 20; j.c_hidden = 576; j.nheads = 9; j.eps = 1e-5f;
    if (global) fill(j.visual);
}

int g_case;
void run(const char* name, const hicom_compressor_args* a, const hicom_compressor_args* second = nullptr) {
    printf("case %d: %s\n", ++g_case, name);
    printf("    workspace_bytes %lld zero_prefix_bytes %lld is_fused %d takes_shard4 %d ctx16_offset %lld\n", (long long)hicom_compressor_workspace_bytes(a),
           (long long)hicom_compressor_zero_prefix_bytes(a), hicom_compressor_is_fused(a), hicom_compressor_takes_shard4(a),
           (long long)hicom_compressor_ctx16_offset(a));
    static const int fail_env = getenv("STUB_FAIL_AT") ? atoi(getenv("STUB_FAIL_AT")) : 0;
    g_error[0] = 0;
    g_launches = 0;
    g_fail_at = fail_env;
    g_stop_event = nullptr;
    const int rc = second ? hicom_compressor_fwd2(a, second) : hicom_compressor_fwd(a);
    printf("    -> %d \"%s\"%s\n", rc, rc ? g_error : "", g_stop_event ? " (stop event left pending)" : "");
}

}  // namespace

int main() {
    hicom_compressor_args a, b;
    // ---- release recipe, single-stream step
    for (int hidden : {896, 3584})
        for (int T : {32, 64}) {       // 648 / 1296 windows: below / above the chain role's wide-hidden threshold
            char name[64];
            snprintf(name, sizeof(name), "release bf16 hidden %d T %d", hidden, T);
            a = release(T, hidden); run(name, &a);
        }
    a = release(64, 896); a.tok_dt = a.lq_dt = a.gq_dt = HICOM_DT_F16; a.out_dt = HICOM_DT_F16; run("release fp16 tokens", &a);
    a = release(64, 3584); a.tok_dt = a.lq_dt = a.gq_dt = HICOM_DT_F16; run("release fp16 tokens hidden 3584", &a);
    a = release(32, 3584); a.tok_dt = a.lq_dt = a.gq_dt = HICOM_DT_F16; run("release fp16 tokens hidden 3584 T 32 (chain role not wide by default)", &a);
    a = release(64, 896); a.tok_dt = HICOM_DT_F16; run("fp16 tokens with a bf16 guide in bf16 slots: lq_dt mismatch", &a);
    a = release(64, 896); with_ring_marg(a); run("release with vpe_f16 (HICOM_RING_MARG=1 takes the marginals out)", &a);
    a = release(64, 896); with_ring_marg(a); a.tok_dt = a.lq_dt = a.gq_dt = HICOM_DT_F16; run("release fp16 tokens with vpe_f16", &a);
    a = release(64, 896); a.pe = nullptr; a.kpe = nullptr; a.P = 0; run("release without pos-emb", &a);
    a = release(64, 896); fill(a.ev_merge); a.defer_join = 1; run("release defer_join", &a);
    a = release(64, 896); fill(a.ev_merge); a.defer_join = 1; with_newlines(a); run("release defer_join + newline rows", &a);
    a = release(64, 896); fill(a.local_out); run("release local_out", &a);
    a = release(64, 896); fill(a.local_out); with_newlines(a); run("release local_out + newline rows (no scatter)", &a);
    a = release(64, 896); with_newlines(a); run("release newline rows", &a);
    a = release(64, 896); fill(a.local_logits); run("release local_logits", &a);
    a = release(64, 896); fill_all(a.ev_done, a.stream_next); run("release ev_done + stream_next", &a);
    a = release(64, 896); a.gc0 = nullptr; run("release without gc0 (out_proj / readout 0 as aux GEMVs, last layer a launch)", &a);
    a = release(64, 3584); a.gc0 = nullptr; run("release without gc0 hidden 3584", &a);
    a = release(64, 896); a.nh = 8; run("release 8 heads (head dim 144: generic query prep, two-stream)", &a);
    // ---- release recipe, two-stream step
    a = release(64, 896); a.lw0_f16 = a.lw2_f16 = nullptr; run("release fp32-input readout weights (planes_gemm)", &a);
    a = release(64, 896); a.lw0_f16 = a.lw2_f16 = nullptr; fill(a.ev_merge); a.defer_join = 1; with_newlines(a); run("planes_gemm defer_join newline rows", &a);
    a = release(64, 896); fill_all(a.state_out, a.ev_merge); run("release two-stream (state_out, joined phases)", &a);
    a = release(64, 896); fill_all(a.state_out, a.ev_merge, a.ev_done, a.stream_next); a.defer_join = 1; run("release two-stream defer_join ev_done", &a);
    a = release(64, 896); a.phases = HICOM_PHASE_STREAM; fill(a.state_out); run("release STREAM only on two streams", &a);
    // ---- frame-sharded step
    for (int r0 = 1; r0 >= 0; --r0)
        for (int nim = 0; nim <= 1; ++nim) {
            char name[96];
            snprintf(name, sizeof(name), "STREAM + MERGE_ON_NEXT%s%s", nim ? " + NEXT_IS_MAIN" : "", r0 ? " (r0_buf: shard4)" : " (no r0_buf)");
            a = release(16, 896); shard_stream(a, nim, r0); run(name, &a);
        }
    a = release(16, 896); shard_stream(a, false, true); with_newlines(a); run("shard4 + newline rows", &a);
    a = release(16, 896); shard_stream(a, false, false); with_newlines(a); a.local_out = nullptr; run("MERGE_ON_NEXT packed rows + newline rows", &a);
    a = release(16, 896); shard_stream(a, false, true); a.state_out = nullptr; run("MERGE_ON_NEXT without state_out (solo merge on next)", &a);
    a = release(16, 3584); shard_stream(a, false, true); run("MERGE_ON_NEXT hidden 3584 (not shard4)", &a);
    a = release(16, 896); shard_stream(a, false, true); a.ev_done = nullptr; run("MERGE_ON_NEXT without ev_done", &a);
    a = generic(16, 32); shard_stream(a, false, true); run("MERGE_ON_NEXT on a generic recipe", &a);
    for (int r0 = 1; r0 >= 0; --r0) {
        a = release(64, 896); shard_finish(a, r0); run(r0 ? "FINISH state_sets (finish4)" : "FINISH state_sets (generic)", &a);
        a = release(64, 896); shard_finish(a, r0); with_allgather(a, false); with_place(a); run(r0 ? "finish4 + all-gather + place" : "generic FINISH + all-gather + place", &a);
        a = release(64, 896); shard_finish(a, r0); with_allgather(a, true); run(r0 ? "finish4 + grouped all-gather" : "generic FINISH + grouped all-gather", &a);
    }
    a = release(64, 896); shard_finish(a, true); a.state_set_stride = 8; run("finish4 bad state set stride", &a);
    a = release(64, 896); shard_finish(a, false); a.state_set_stride = 8; run("generic FINISH bad state set stride", &a);
    a = release(64, 896); shard_finish(a, true); a.nsets = 300; run("FINISH 300 sets (generic)", &a);
    a = release(64, 896); shard_finish(a, true); with_allgather(a, false); a.ag_comm = nullptr; run("all-gather arguments missing", &a);
    a = release(64, 896); shard_finish(a, true); with_allgather(a, true); a.ag_recv2 = nullptr; run("grouped all-gather arguments missing", &a);
    a = release(64, 896); shard_finish(a, true); with_place(a); a.ev_done = nullptr; fill(a.stream_next); run("FINISH place without ev_done", &a);
    a = release(64, 896); a.phases = HICOM_PHASE_FINISH; run("FINISH only without state_sets", &a);
    a = release(16, 896); shard_stream(a, true, true); b = release(64, 896); shard_finish(b, true); with_allgather(b, true); b.r0_buf = a.r0_buf;
    run("fwd2: joined sharded step", &a, &b);
    // ---- generic two-kernel form
    for (int T : {64, 1}) {        // (a single image keeps the logit tensor: no room for the marginal record)
        a = generic(T, 32); if (T == 1) a.at = axis(1, 1);
        run(T == 1 ? "guide off 288 rows, one image" : "guide off 288 rows", &a);
    }
    a = generic(64, 32); a.ev_merge = nullptr; run("guide off 288 rows without ev_merge (not stream_first)", &a);
    a = generic(64, 32); a.pe = nullptr; a.kpe = nullptr; a.P = 0; run("guide off without pos-emb", &a);
    a = generic(64, 32); a.reuse_queries = 1; run("guide off reuse_queries", &a);
    a = generic(64, 32); a.lw0_f16 = a.lw2_f16 = nullptr; with_newlines(a); run("guide off fp32-input readout + newline rows", &a);
    a = generic(64, 32); with_newlines(a); fill(a.local_out); run("guide off local_out", &a);
    a = generic(64, 32); with_newlines(a); run("guide off newline rows", &a);
    a = generic(64, 1); run("guide off 9 rows (16 padded: not stream_first)", &a);
    a = generic(64, 1); fill(a.lq); a.lq_dt = HICOM_DT_F32; a.lq_stride = 1152; a.gq_dt = HICOM_DT_F32; fill(a.ev_queries); run("caller-injected f32 queries + ev_queries", &a);
    a = generic(64, 1); a.l2norm = 1; run("clip-scale", &a);
    a = generic(64, 32); a.has_global = 0; run("local only", &a);
    a = generic(64, 32); a.has_local = 0; run("global only", &a);
    a = generic(64, 32); a.has_local = 0; a.phases = HICOM_PHASE_STREAM; fill(a.state_out); run("global only STREAM, state_out", &a);
    a = generic(64, 32); a.phases = HICOM_PHASE_STREAM; run("generic STREAM only", &a);
    a = generic(64, 32); a.phases = HICOM_PHASE_FINISH; run("generic FINISH only", &a);
    a = release(64, 896); a.at = hicom_axis{64, 4, 21, 0}; run("overlapping windows with a shared query (generic)", &a);
    for (int mode : {1, 2})
        for (int stage = 0; stage < 3; ++stage) {
            static const char* st[] = {"local", "global", "local + global"};
            char name[64];
            snprintf(name, sizeof(name), "%s injection, %s", mode == 1 ? "coarse" : "fine", st[stage]);
            a = generic(64, 32);
            if (stage != 1) with_injector(a.inj_l, mode, false);
            if (stage != 0) with_injector(a.inj_g, mode, true);
            run(name, &a);
        }
    a = generic(64, 32); with_injector(a.inj_l, 2, false); a.ev_merge = nullptr; run("fine local injection, not stream_first", &a);
    a = generic(8, 1); with_injector(a.inj_l, 2, false); run("fine local injection over 162 windows (linear rows)", &a);
    a = generic(8, 1); with_injector(a.inj_l, 2, false); a.at = axis(8, 8); run("fine local injection over 81 windows", &a);
    a = generic(64, 32); with_injector(a.inj_g, 1, true); a.inj_g.guide_rows = 2; run("coarse injector arguments", &a);
    a = generic(64, 32); with_injector(a.inj_l, 2, false); a.inj_l.guide_rows = 65; run("fine injector arguments", &a);
    a = generic(64, 32); with_injector(a.inj_g, 1, true); a.inj_g.visual = nullptr; run("global injector without visual", &a);
    a = generic(64, 32); with_injector(a.inj_l, 1, false); fill(a.lq); run("local injector with lq", &a);
    a = generic(64, 32); with_injector(a.inj_l, 3, false); run("injector mode 3", &a);
    a = generic(64, 32); with_injector(a.inj_l, 1, false); a.phases = HICOM_PHASE_STREAM; run("injection in a split-phase call", &a);
    for (int which = 1; which <= 3; ++which)
        for (int y = 0; y <= 1; ++y) {
            char name[64];
            snprintf(name, sizeof(name), "adaptor%s%s%s", which & 1 ? " k" : "", which & 2 ? " v" : "", y ? ", caller-supplied y" : "");
            a = release(64, 896);
            if (which & 1) with_adaptor(a.ak, y);
            if (which & 2) with_adaptor(a.av, y);
            run(name, &a);
        }
    a = release(64, 896); with_adaptor(a.ak, false); with_adaptor(a.av, true); run("adaptors k v, y for v only", &a);
    a = release(64, 896); with_adaptor(a.ak, false); with_adaptor(a.av, false); a.av.b2 = nullptr; run("adaptors k v without a bias (not paired)", &a);
    a = generic(64, 32); with_adaptor(a.ak, false); run("adaptor k, guide off", &a);
    a = release(64, 896); with_adaptor(a.ak, false); a.ak.gamma = nullptr; run("adaptor weights missing", &a);
    a = release(64, 896); with_adaptor(a.ak, false); a.l2norm = 1; run("adaptor with clip-scale", &a);
    // ---- refusals
    run("NULL args", nullptr);
    a = release(64, 896); a.has_local = a.has_global = 0; run("nothing to do", &a);
    a = release(64, 896); a.out = nullptr; run("NULL pointer", &a);
    a = release(64, 896); a.E = 1024; run("bad input shape", &a);
    a = release(64, 900); run("hidden not a multiple of 64", &a);
    a = release(64, 896); a.lw2 = nullptr; run("local readout weights missing", &a);
    a = release(64, 896); a.wv = nullptr; run("global weights missing", &a);
    a = release(64, 896); a.n_global_rows = 0; run("global row count", &a);
    a = release(64, 896); a.gq_dt = HICOM_DT_F16; run("gq_dt fp16 with bf16 tokens", &a);
    a = release(64, 896); a.kpe = nullptr; run("pe without kpe", &a);
    a = release(64, 896); a.ev_join = nullptr; run("side stream and events required", &a);
    a = release(64, 896); a.tok_dt = 7; run("tok_dt", &a);
    a = release(64, 896); a.ws_bytes = 1 << 20; run("workspace too small", &a);
    a = generic(64, 32); a.tok_dt = HICOM_DT_F16; run("fp16 tokens on a non-release recipe", &a);
    a = release(64, 896); a.tok_dt = a.lq_dt = a.gq_dt = HICOM_DT_F16; a.gc0 = nullptr; run("fp16 tokens without gc0", &a);
    a = release(64, 896); a.tok_dt = a.lq_dt = a.gq_dt = HICOM_DT_F16; fill(a.local_logits); run("fp16 tokens with local_logits", &a);
    a = generic(64, 32); fill(a.local_logits); run("local_logits on a generic recipe", &a);
    a = release(16, 896); shard_stream(a, false, true); a.stream_next = nullptr; run("MERGE_ON_NEXT without stream_next", &a);
    printf("%d cases\n", g_case);
    return 0;
}
