/*
 * hicom_hip.h -- C ABI of libhicom_hip.so: MI355X (gfx950 / CDNA4) kernels for the HICom
 * hybrid-level video-token compressor.
 *
 * The reference (lntzm/HICom) is pure Python and has no FFI; each entry point below replaces
 * a chain of stock PyTorch ops on the path
 *     hicom/model/projector.py:676-708   HIComProjector.forward
 * and is cited to the reference lines it stands in for.  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into memory owned by the caller (torch on the Python
 *     side); the library allocates nothing and keeps no state between calls;
 *   - dense row-major layouts, no strides; "bf16" = uint16_t bit patterns; f32 = float;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is
 *     enqueued asynchronously on it and nothing synchronises the host (graph-capturable);
 *   - return 0 on success, a negative HICOM_E* code otherwise; never throws.
 *     hicom_last_error() returns a thread-local description of the last failure.
 */
#ifndef HICOM_HIP_H
#define HICOM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HICOM_ABI_VERSION 16

#define HICOM_OK         0
#define HICOM_EINVAL    -1   /* bad argument (shape, alignment, NULL)        */
#define HICOM_EUNSUP    -2   /* configuration not supported by the kernels   */
#define HICOM_ELAUNCH   -3   /* HIP launch / runtime error                   */

#define HICOM_DT_BF16 0
#define HICOM_DT_F32  1
#define HICOM_DT_F16  2      /* IEEE half: activations that feed matrix cores (11 significand bits), accepted where noted */

/* activation / epilogue flags for the linear + GEMM entry points */
#define HICOM_ACT_NONE 0
#define HICOM_ACT_GELU 1     /* exact erf GELU (nn.GELU() default, projector.py:310) */
#define HICOM_ACT_GELU_TANH 2 /* tanh GELU (HF "gelu_pytorch_tanh": the SigLIP MLP, encoder.py:285) */

int hicom_abi_version(void);
const char* hicom_last_error(void);

/* One axis of the window tiling of LocalCompressor.divide_feature /
 * balance_divide_feature (projector.py:473-522): `nwin` windows of length `k` over `n`
 * elements; the first `nfull` start at i*k, the rest at nfull*k + (i-nfull)*(k-1) - 1
 * (one-element overlap).  Divisible axes have nfull == nwin. */
typedef struct hicom_axis {
    int32_t n, k, nwin, nfull;
} hicom_axis;

/* ---- local compressor: windowed single-head cross-attention ------------------------------
 * Replaces projector.py:544-558 (divide_feature x3, bmm, softmax, bmm, un-window) and, with
 * l2norm != 0, the clip-scale normalisation at :527-529,549.
 *   key, value : [T,H,W,D] bf16 (frames_embed / frames_feature; key may alias value), or f32 / fp16 (the
 *                alpha-blended adaptor outputs of projector.py:533-534); dtype key_dt / value_dt
 *   query      : [D] shared by every window (query_stride == 0, GuideInjector "direct",
 *                projector.py:352-368) or [Nw, D] with row stride query_stride elements;
 *                dtype query_dt
 *   logits     : (q.k) * scale + bias        (scale = 1/sqrt(D) or exp(logit_scale))
 *   ctx        : f32 [Nw, D], window order (t1,h1,w1) row-major, Nw = at.nwin*ay.nwin*ax.nwin; and / or
 *   ctx_f16    : the same contexts as one fp16 plane (saturating): the operand of hicom_readout16_gemm_fwd (either may be NULL)
 *   l2norm     : bit 0 = L2-normalise every key row, bit 1 = L2-normalise the query
 *                (clip-scale variant, projector.py:527-529)
 * D must be 1152 or 768 (projector.py:407-414). */
int hicom_local_attn_fwd(const void* key, int32_t key_dt, const void* value, int32_t value_dt, int32_t D,
                         hicom_axis at, hicom_axis ay, hicom_axis ax,
                         const void* query, int32_t query_dt, int64_t query_stride,
                         float scale, float bias, int32_t l2norm,
                         float* ctx, void* ctx_f16, void* stream);

/* ---- windowed attention with the k / v adaptor blend fused into its row loads (projector.py:533-534 in front of :544-553) ----
 *   key_n = (1 - a_k) key_x_n + a_k (LayerNorm_eps(key_y_n) k_gamma + k_beta),  key_y = k_proj(key_x) (the two dense GEMMs of the
 *   adaptor MLP, fp16 [N, D]); likewise the values.  The blended streams are never materialised: logits and contexts are formed
 *   from the x and y rows with the LayerNorm statistics computed on the row in registers.  key_y or value_y may be NULL (that stream
 *   has no adaptor).  key_x / value_x bf16 [T,H,W,D]; gamma / beta bf16 [D]; alpha: device scalar (bf16 | f32).  No clip-scale. */
int hicom_local_attn_adapt_fwd(const void* key_x, const void* key_y, const void* k_gamma, const void* k_beta, const void* k_alpha,
                               const void* value_x, const void* value_y, const void* v_gamma, const void* v_beta, const void* v_alpha,
                               int32_t alpha_dt, float eps, int32_t D, hicom_axis at, hicom_axis ay, hicom_axis ax,
                               const void* query, int32_t query_dt, int64_t query_stride, float scale, float bias,
                               float* ctx, void* stream);

/* ---- backward of the windowed attention with the k / v adaptor blends (training path of `local43_adaptkv_global32`; autograd
 * through projector.py:533-534 + :550-553).  Arguments as hicom_local_attn_adapt_fwd plus dctx f32 [Nw, D].  Outputs (exact window
 * partition required):
 *   ds [N] f32 = scale dS_n,  pw [N] f32 = p_n       token-indexed: d key_n = ds_n q_w, d value_n = pw_n dctx_w (rank 1, never written)
 *   sxk, sxv [Nw, D] f32 = sum_n ds_n key_x_n, sum_n pw_n value_x_n;   syk, syv [Nw, D] = sum_n ds_n yhat_k,n, sum_n pw_n yhat_v,n with
 *   yhat = LayerNorm-normalised y (no affine); syk / syv may be NULL when that stream has no adaptor.
 * From these: dq_w = (1 - a_k) sxk_w + a_k gamma_k syk_w, and d alpha / d gamma / d beta of both adaptors as sums over the windows.
 * hicom_adapt_dy_fwd continues into the adaptor MLP: dy[tok] = d/dy of alpha LN(y) gamma for the upstream gradient coef[tok] * vec[w(tok)]
 * (K: coef = ds, vec = q; V: coef = pw, vec = dctx), written as bf16 [N, D]; r1 (may be NULL) = (1 - alpha) coef[tok] vec[w] as bf16, the
 * x-branch of d frames_embed.  hicom_gelu_split_fwd / hicom_gelu_bwd_fwd / hicom_colsum_fwd: the elementwise steps of the adaptor-MLP backward
 * (a = GELU(h) as fp16 and bf16; da *= GELU'(h) in place; partial column sums [nparts][D] for the bias gradients).
 * hicom_adapt_dy_fwd and hicom_gelu_bwd_fwd leave the column partials of what they write themselves when col_parts (f32 [nparts][D],
 * summed by hicom_partials_sum_fwd) is given: `nparts` workgroups then walk the rows -- no separate pass for the bias gradients. */
int hicom_local_attn_adapt_bwd(const void* key_x, const void* key_y, const void* k_gamma, const void* k_beta, const void* k_alpha,
                               const void* value_x, const void* value_y, const void* v_gamma, const void* v_beta, const void* v_alpha,
                               int32_t alpha_dt, float eps, int32_t D, hicom_axis at, hicom_axis ay, hicom_axis ax,
                               const void* query, int32_t query_dt, int64_t query_stride, float scale, float bias,
                               const float* dctx, float* ds, float* pw, float* sxk, float* syk, float* sxv, float* syv, void* stream);
int hicom_adapt_dy_fwd(const void* y, const void* gamma, const void* vec, int32_t vec_dt, int64_t vec_stride, const float* coef,
                       const void* alpha, int32_t alpha_dt, float eps, int32_t D, hicom_axis at, hicom_axis ay, hicom_axis ax,
                       void* dy, void* r1, float* col_parts, int32_t nparts, void* stream);
int hicom_gelu_split_fwd(const void* h_f16, void* a_f16 /* may be NULL */, void* a_bf16, int64_t n, void* stream);
/* The same two steps for a hidden layer that lies inside pitched rows (the SigLIP head's [M, 4304] inside rows of 4544 fp16 elements,
 * encoder.py:284-286) and for either activation (act = HICOM_ACT_GELU | 2 = gelu_pytorch_tanh): a_bf16 [rows, cols] = act(h[r, c]);
 * da_bf16 [rows, cols] *= act'(h[r, c]) in place.  cols, ldh multiples of 8. */
int hicom_act_rows_fwd(const void* h_f16, int64_t ldh, int64_t rows, int32_t cols, int32_t act, void* a_bf16, void* stream);
int hicom_act_bwd_rows_fwd(void* da_bf16, const void* h_f16, int64_t ldh, int64_t rows, int32_t cols, int32_t act, void* stream);
int hicom_gelu_bwd_fwd(void* da_bf16, const void* h_f16, int64_t n, int32_t D, float* col_parts, int32_t nparts, void* stream);
int hicom_colsum_fwd(const void* x_bf16, int64_t N, int32_t D, float* parts, int32_t nparts, void* stream);

/* ---- backward of the windowed attention (training path; autograd through projector.py:550-553) ----------
 * For the reference's stage 3 (train.py:717-726: the SigLIP head and the guide encoder train too) the gradients
 * w.r.t. the key stream frames_embed and the query are needed.
 *   key, value : bf16 [T,H,W,D];  query as in hicom_local_attn_fwd;  dctx : f32 [Nw, D] upstream gradient of ctx
 *   dq         : f32 [Nw, D]  scale * sum_i dS_i k_i per window (a shared query's gradient is the sum over windows)
 *   dkey       : bf16 [T,H,W,D] scale * dS_i * q, or NULL.  Where the kernel does not divide an axis the trailing windows overlap by one plane
 *                (projector.py:501-522): dkey / dvalue are then cleared and accumulated by one launch per parity class of the window index along
 *                every such axis (windows of one class share no token: ordered sums, no atomics)
 *   l2norm_key (ABI 15): clip-scale on the local stage (projector.py:527-529, :549; trainable under `attn_scale`, train.py:730-733):
 *                the key rows enter L2-normalised, s_i = scale (q . k_i / ||k_i||) + bias with scale = e^logit_scale, bias = logit_bias;
 *                dq and dkey then go through the normalisation.  The query is used as given (the caller normalises the guide).
 *   dls        : f32 [Nw] or NULL: sum_i dS_i (s_i - bias) per window = this window's share of d logit_scale (d logit_bias is 0: the
 *                softmax cancels a shift) */
int hicom_local_attn_bwd(const void* key, const void* value, int32_t D,
                         hicom_axis at, hicom_axis ay, hicom_axis ax,
                         const void* query, int32_t query_dt, int64_t query_stride,
                         float scale, float bias, const float* dctx, float* dq, void* dkey,
                         int32_t l2norm_key, float* dls, void* dvalue, int32_t value_is_key, void* stream);
/* (dvalue, ABI 15: bf16 [T,H,W,D] = p_i dctx_w, the gradient w.r.t. the VALUE stream frames_feature, or NULL; value_is_key: the keys are
 * the value rows -- frames_embed None, projector.py:532 -- and the key-side gradient is added into dvalue, dkey NULL.)
 *
 * d frames_feature of the GLOBAL stage, direct recipe (<= 16 folded rows), from the tensors the attention backward leaves:
 *   dx[n, :] (+)= sum_r dS[r, n] qt[r, :] + exp(S[r, n] - M_r) / L_r dctx[r, :]
 * S = the forward's logits, dS = hicom_global_stream_bwd's ds_out (both f32 [rows_pad, score_stride]), ml f32 [rows][2], qt / dctx f32
 * [rows, E] (folded queries incl. the attention scale; upstream gradients of the per-head contexts), dx bf16 [N, E]; accumulate != 0:
 * dx already holds the local stage's share (read, added in fp32, written back).  The positional terms do not depend on x. */
int hicom_global_dx_fwd(const float* S, const float* dS, int64_t score_stride, const float* ml, const float* qt, const float* dctx,
                        int32_t rows, int64_t N, int32_t E, void* dx, int32_t accumulate, void* stream);

/* ---- pooled per-window query: F.interpolate(..., 'trilinear', align_corners=False) --------
 * Replaces projector.py:539-540.  x bf16 [T,H,W,D] -> out f32 [t',h',w',D]. */
int hicom_trilinear_pool_fwd(const void* x, int32_t T, int32_t H, int32_t W, int32_t D,
                             int32_t To, int32_t Ho, int32_t Wo, float* out, void* stream);

/* ---- small-M linear: y[M,N] = act(x[M,K] . w[N,K]^T + b) + res ---------------------------
 * nn.Linear on a handful of rows (q_proj / out_proj / readout of the global tokens,
 * projector.py:180,226,646; also the score-side positional table q~.PE^T).
 *   head_dim > 0 selects "per-head rows": column n reads x row m*head_rows + n/head_dim
 *   (v_proj applied to the per-head context, projector.py:182,215 after folding).
 *   b, res may be NULL.  res is [M,N]; res_flags bit 0 = broadcast row 0, bit 1 = res is bf16
 *   (otherwise f32). */
int hicom_linear_fwd(const void* x, int32_t x_dt, const void* w, int32_t w_dt,
                     const void* b, int32_t b_dt, const void* res, int32_t res_flags,
                     int32_t M, int32_t N, int32_t K, int32_t head_rows, int32_t head_dim,
                     int32_t act, float* y, void* stream);

/* Same product, written straight into a packed output: row m of y goes to rows
 * row0 + m + k*M, k < n_rows / M, of dst [*, ldd] (dtype dst_dt) -- the last Linear of the global
 * readout filling the 32 global rows (projector.py:646,707; in "direct" mode M == 1 and the 32 rows
 * are 32 copies). */
int hicom_linear_to_rows_fwd(const void* x, int32_t x_dt, const void* w, int32_t w_dt,
                             const void* b, int32_t b_dt, int32_t M, int32_t N, int32_t K, int32_t act,
                             void* dst, int32_t dst_dt, int64_t ldd, int64_t row0, int32_t n_rows,
                             void* stream);

/* ---- fold k_proj into the queries ---------------------------------------------------------
 * qt[(q*nh + h), c] = scale * sum_j w_k[h*hd + j, c] * qp[q, h*hd + j]
 * so that score_h(n) = qt_h . x_n (+ a key-independent constant that softmax cancels):
 * replaces k_proj over all T*729 tokens (projector.py:181,193-197).  qp f32 [nq,E],
 * w_k bf16 [E,E] (nn.Linear layout [out,in]), qt f32 [nq*nh, E]. */
int hicom_fold_query_fwd(const float* qp, const void* w_k, int32_t nq, int32_t nh, int32_t E,
                         float scale, float* qt, void* stream);

/* Fused form used on the hot path: emits qt directly as the bf16 hi/lo pair of the stream kernel
 * and, when kpe != NULL, the score-side positional table
 *   pos_a[(q*nh + h), p] = scale * sum_j kpe[h*hd + j, p] * qp[q, h*hd + j]  ( = qt . PE[p] )
 * from kpe = w_k . PE^T (f32 [E, P]; depends on the weights only -- the caller caches it, the way
 * the reference caches its pos_embed buffer, projector.py:603-607).  Rows >= nq*nh of qt_hi /
 * qt_lo / pos_a are not written (callers keep them zero), except that fill_row (bf16 [E], may be
 * NULL) is broadcast into rows [fill_row0, fill_row0 + fill_rows) of qt_hi: the local query rows of
 * hicom_fused_stream_fwd's operand. */
int hicom_fold_query_split_fwd(const float* qp, const void* w_k, const float* kpe, int32_t nq, int32_t nh,
                               int32_t E, int32_t P, float scale, void* qt_hi, void* qt_lo,
                               float* pos_a, int32_t pos_stride, const void* fill_row, int32_t fill_row0,
                               int32_t fill_rows, void* stream);

/* Release recipe, use_guide = "direct" (ONE injected query row = the guide): q_proj, the fold, the score-side positional
 * table, the local query rows of hicom_fused_stream_fwd's operand and the guide-dependent part of the global readout in ONE
 * launch (the q_proj -> fold hand-off travels inside the grid as tagged 8-byte granules):
 *   qt_hi / qt_lo rows h < nh : bf16 hi / lo of  scale * w_k[h]^T (w_q guide + b_q)[h]       (projector.py:180-181,193-197)
 *   qt_hi rows nh .. 15       : local_q bf16 [E], the shared local query (= the guide, :352-368); qt_lo rows stay as
 *                               the caller zeroed them
 *   pos_a[h, p]               : scale * kpe[h]^T (w_q guide + b_q)[h]   (kpe f32 [E, P] = w_k . PE^T, or NULL)
 *   r0 f32 [hidden]           : g_w0 (b_o + guide) + g_b0  -- with C = g_w0 . w_o (cached by the caller) the tail
 *                               GELU(g_w0 (w_o o + b_o + guide) + g_b0) of :226,:646,:307-312 is GELU(C o + r0); g_w0 NULL = no r0
 * state: hicom_query_prep_state_bytes(E) bytes of caller-owned device memory, zeroed ONCE, private to one stream of
 * calls with ONE problem shape (words 0-1 arrival counter, word 2 failed hand-offs, word 3 grid size of the first launch,
 * then the granules; the kernel maintains it).  A hand-off that fails -- a bounded spin that gave up, or a launch whose grid
 * differs from the first one on this block -- writes NaN into qt_hi / qt_lo / pos_a (every output token then is NaN) and
 * counts in word 2: a missed hand-off never passes for a result.
 * ABI 16, fp16 tokens: g_dt = HICOM_DT_F16 takes an fp16 guide and local_q (local_q is copied into qt_hi bit for bit: the local query
 * rows then are exact fp16 operands), and qt_f32 (f32 [16, E], 16-byte aligned) receives the folded global query rows UNSPLIT: the
 * fp16 instantiation of the ring kernel splits them itself at a power-of-two scale per row (hicom_fused_stream_fwd's q_f32); qt_hi /
 * qt_lo rows < nh are then not written.  g_dt = HICOM_DT_BF16: as before, qt_f32 ignored (may be NULL). */
int64_t hicom_query_prep_state_bytes(int32_t E);
int hicom_query_prep_fwd(const void* guide, const void* local_q, const void* w_q, const void* b_q, const void* w_k, const float* kpe,
                         int32_t nh, int32_t E, int32_t P, float scale, void* qt_hi, void* qt_lo, float* pos_a,
                         int32_t pos_stride, int32_t rows, const void* g_w0, const void* g_b0, const void* b_o,
                         int32_t hidden, float* r0, void* state, int32_t g_dt, float* qt_f32, void* stream);

/* Split f32 rows into bf16 hi + lo parts (x ~= hi + lo to 2^-16), zero-padding the row count
 * to rows_pad: the MFMA operand format for fp32 intermediates (SURVEY.md §7 strategy B). */
int hicom_split_bf16_fwd(const float* x, int32_t rows, int32_t rows_pad, int32_t E,
                         void* hi, void* lo, void* stream);
/* ABI 16: the same split into hi + lo of a 16-bit type, dt = HICOM_DT_BF16 (= hicom_split_bf16_fwd) or HICOM_DT_F16 (fp16 planes, for the
 * fp16 instantiation of hicom_fused_stream_fwd: |x - hi - lo| <= 2^-23 |x| + 2^-25, i.e. 2^-20 of a row whose max |x| is >= 2^-3 --
 * the pe table's rows, sinusoids whose max is near 1; the fp16 planes saturate: |x| > 65504 gives hi = +-65504 and lo = the saturating
 * fp16 of x - hi, never Inf) */
int hicom_split16_fwd(const float* x, int32_t rows, int32_t rows_pad, int32_t E, int32_t dt, void* hi, void* lo, void* stream);

/* ---- global compressor: streaming multi-query attention over all tokens -------------------
 * One pass over x = frames_feature[n0 : n0+N) (bf16 [N,E], E = 1152 | 768) computing, for a
 * block of `rows_pad` folded queries (multiple of 16), the raw scores and the online-softmax
 * partial sums of attn . x.  Replaces projector.py:193-215 for K = V = x (pos-emb handled
 * separably: `pos_a` holds qt . PE for the t / y / x axes).
 *   qt_hi, qt_lo : bf16 [rows_pad, E]; rows >= `rows` are zero padding and produce no output
 *   pos_a        : f32 [rows_pad, pos_stride] or NULL; token (t,y,x) adds
 *                  pos_a[r, t_index0 + t] + pos_a[r, y_index0 + y] + pos_a[r, x_index0 + x]
 *   geometry     : token n -> t = n / (H*W), y = (n / W) % H, x = n % W  (n relative to n0 = 0
 *                  of THIS call's x pointer; t_index0 carries the shard's frame offset)
 *   scores       : f32 [rows_pad, score_stride]  (score_stride >= roundup(N,16))
 *   part_m/l     : f32 [nparts, rows_pad]; part_acc : f32 [nparts, rows_pad, E]
 *   nparts       : number of token chunks (= workgroups per row group); returned layout is
 *                  consumed by hicom_global_merge_fwd.
 *   N            : 0 < N < 2^31, else HICOM_EINVAL (all four entries below and hicom_global_stream_bwd).  The narrow (one-row-group)
 *                  kernel indexes tokens with a 32-bit int, as the many-item steps do: the last tile's 16 * tile + 15 <= 2^31 - 1
 *                  still is one.  No such N fits device memory at E >= 768.
 */
int hicom_global_stream_fwd(const void* x, int64_t N, int32_t E,
                            const void* qt_hi, const void* qt_lo, int32_t rows, int32_t rows_pad,
                            const float* pos_a, int32_t pos_stride,
                            int32_t H, int32_t W, int32_t t_index0, int32_t y_index0, int32_t x_index0,
                            float* scores, int64_t score_stride,
                            float* part_m, float* part_l, float* part_acc, int32_t nparts,
                            void* stream);
/* Same pass for the clip-scale variant (projector.py:184-191): logit[r, n] = (qt_r . x_n + pos terms + row_const[r]) *
 * inv_norm[n], inv_norm f32 [N] = 1 / ||k_proj(x_n + pos_n)|| (hicom_inv_norm_fwd), row_const f32 [rows_pad]
 * (hicom_clip_query_prep_fwd; padding rows 0).  One 16-row group per workgroup (any row count). */
int hicom_global_stream_clip_fwd(const void* x, int64_t N, int32_t E,
                                 const void* qt_hi, const void* qt_lo, int32_t rows, int32_t rows_pad,
                                 const float* pos_a, int32_t pos_stride,
                                 int32_t H, int32_t W, int32_t t_index0, int32_t y_index0, int32_t x_index0,
                                 const float* inv_norm, const float* row_const,
                                 float* scores, int64_t score_stride,
                                 float* part_m, float* part_l, float* part_acc, int32_t nparts, void* stream);

/* The same pass with the positional marginals of the softmax weights accumulated IN the kernel (projector.py:176-179: the
 * value-side pos-emb term sum_n p_n pos(n) collapses to the t / y / x marginals of p): `scores` may be NULL -- the
 * [rows_pad, N] logit tensor (54 MB at 32 queries x 9 heads x 64 frames) is then neither written nor read back, and
 * hicom_global_merge_marg_fwd needs no per-frame marginal pass.  Only the many-row form of the kernel has it (E = 1152, rows_pad
 * a multiple of 32, grids up to 64 x 48): hicom_global_stream_has_marg(N, E, rows_pad, H, W, nparts) == 1, else HICOM_EUNSUP.
 *   part_marg : f32 [nparts][rows_pad][hicom_global_stream_marg_width(H, W)], un-normalised, relative to the chunk's own max
 *               like part_acc: [8 frames counted from the chunk's first | pad to 16 | H | pad to 16 | W | pad to 16]
 *   pos_a     : required (without pos-emb there are no marginals: use hicom_global_stream_fwd) */
int hicom_global_stream_marg_fwd(const void* x, int64_t N, int32_t E,
                                 const void* qt_hi, const void* qt_lo, int32_t rows, int32_t rows_pad,
                                 const float* pos_a, int32_t pos_stride,
                                 int32_t H, int32_t W, int32_t t_index0, int32_t y_index0, int32_t x_index0,
                                 float* scores, int64_t score_stride,
                                 float* part_m, float* part_l, float* part_acc, float* part_marg, int32_t nparts,
                                 void* stream);
int hicom_global_stream_marg_width(int32_t H, int32_t W);
int hicom_global_stream_has_marg(int64_t N, int32_t E, int32_t rows_pad, int32_t H, int32_t W, int32_t nparts);

/* ---- backward of the global attention over the token stream (training) ------
 * Autograd through projector.py:197-215 in the folded form: with the forward's logits S (the `scores`
 * hicom_global_stream_fwd wrote), its softmax state ml [rows][2] = (M, L) and delta_r = dctx_r . ctx_r,
 *   dP[r,n] = dctx_r . (x_n + pos_n),   dS[r,n] = exp(S[r,n] - M_r) / L_r * (dP[r,n] - delta_r)
 *   part_acc[p, r, :] = sum over chunk p of dS[r,n] x_n          (sum over p = the x part of d qt_r)
 * dctx_hi / dctx_lo: bf16 [rows_pad, E] planes of the upstream context gradients (padding rows zero);
 * pos_b: f32 [rows_pad, pos_stride] = dctx . PE^T (or NULL); ds_out: f32 [rows_pad, score_stride] (its t / y / x
 * marginals times PE give the positional part of d qt).  One pass over x, same tiling as the forward.  part_marg (may be NULL; f32
 * [nparts][rows_pad][hicom_global_stream_marg_width(H, W)], shapes with hicom_global_stream_has_marg == 1): the t / y / x marginals of dS
 * per token chunk, laid out as in hicom_global_stream_marg_fwd (no rescaling: plain sums) -- ds_out may then be NULL and the
 * [rows, N] dS tensor is never written. */
int hicom_global_stream_bwd(const void* x, int64_t N, int32_t E, const void* dctx_hi, const void* dctx_lo,
                            int32_t rows, int32_t rows_pad, const float* pos_b, int32_t pos_stride,
                            int32_t H, int32_t W, int32_t t_index0, int32_t y_index0, int32_t x_index0,
                            const float* s_in, int64_t score_stride, const float* ml, const float* delta,
                            float* ds_out, float* part_acc, float* part_marg, int32_t nparts, void* stream);

/* Suggested nparts for N tokens (fills the chip: 2 workgroups per CU). */
int hicom_global_stream_nparts(int64_t N, int32_t rows_pad);

/* ---- fused local + global stream (release recipe) -------------------------------------------
 * ONE pass over frames_embed and frames_feature computing BOTH the local window contexts
 * (projector.py:544-558, guide as the shared query) and the global online-softmax partial state
 * (projector.py:193-215): each visual tensor is read from HBM exactly once.
 * Requirements: windows partition the grid exactly (T % kt == H % ks == W % ks == 0), 16 <= kt*ks*ks
 * <= 64, rows <= 12 global folded rows, E == 1152.
 *   fe          : frames_embed bf16 [T,H,W,E] -- enters only through the local logit fe_n . local query per token -- or
 *   local_logits: f32 [T*H*W] = fe_n . local query already computed by the producer of frames_embed
 *                 (hicom_dense16_gemm_fwd's row-dot epilogue on the SigLIP head projection, encoder.py:284-286): the
 *                 kernel then does not read frames_embed at all (half the HBM bytes); NULL = stream fe
 *   q_hi / q_lo : bf16 [16, E]; rows < `rows` = folded global queries (hi / lo), rows >= `rows` =
 *                 the local query in q_hi (exact bf16; row `rows` is the one the kernel reads) and zeros in q_lo
 *   pos_a       : f32 [16, pos_stride] score-side pos-emb  a[r, p] = qt_r . pe[p]  (hicom_fold_query_split_fwd),
 *                 or NULL (no pos-emb)
 *   pe_hi/pe_lo : bf16 [P, E] hi / lo planes of the per-axis sinusoid table pe (hicom_split_bf16_fwd of the f32
 *                 table, projector.py:57-101); NULL iff pos_a is NULL.  The value-side pos-emb term
 *                 sum_n p_n (pe[t_index0 + t_n] + pe[y_index0 + y_n] + pe[x_index0 + x_n])  (:176-179) is folded into
 *                 part_acc by the kernel itself (marginals of the weights x pe rows, as extra P.x steps), so the
 *                 partials merge with hicom_global_merge_fwd(pe = NULL).
 *   part_*      : as hicom_global_stream_fwd with rows_pad = 16; nparts from
 *                 hicom_fused_stream_nparts(number of windows).  Partial p covers the contiguous window-major range
 *                 [p * wpw, min((p + 1) * wpw, Nw)) with wpw = ceil(Nw / nparts); an nparts that leaves a range empty is refused
 *   ctx_local   : f32 [Nw, E], window order (t1,h1,w1), and/or ctx_hi + ctx_lo: the same contexts as
 *                 bf16 planes (hi + lo) for hicom_planes_gemm_fwd, and/or ctx_f16: one fp16 plane (saturating) for
 *                 hicom_readout16_gemm_fwd; unused outputs NULL
 *   part_ctx_f16: not NULL: instead of part_acc (which may then be NULL) the kernel writes the NORMALISED partial contexts
 *                 acc / l as one fp16 plane (saturating at +-65504, like ctx_f16) [nparts][16][E] (rows < rows), for hicom_merge_vproj_fixed_fwd(part_dt = HICOM_DT_F16):
 *                 half the bytes of the partial states; the rounding (2^-12 relative per partial) averages over the partials
 *   zero_ptr    : zero_bytes (multiple of 8, 8-byte aligned) of scratch that the kernel clears for the launches behind it on the
 *                 stream (the fixed-point accumulators of hicom_merge_vproj_fixed_fwd), or NULL
 *   part_marg_f16 (ABI 15): not NULL (with pe_hi = pe_lo = NULL, pos_a and part_ctx_f16 given): the value-side pos-emb term is NOT folded
 *                 into the partial contexts; the kernel writes the t / y / x MARGINALS of every partial's softmax weights instead,
 *                 normalised like part_ctx_f16 (marginal / l), fp16 [nparts][rows][marg_slots] in absolute slot order
 *                 [T frames | H grid rows | W grid columns | zeros], marg_slots >= T + H + W and a multiple of 8 -- for the merge role
 *                 of hicom_readout16_gemm_role_fwd (hicom_r16_role.part_marg), which multiplies the merged marginals by v_proj . pe^T
 *   tok_dt (ABI 16): HICOM_DT_BF16, or HICOM_DT_F16: ff / fe, pe_hi / pe_lo (fp16 planes: hicom_split16_fwd) and the local query rows of
 *                 q_hi are fp16, and the folded global queries come as f32 rows q_f32 [16, E] (hicom_query_prep_fwd's qt_f32; q_hi / q_lo rows
 *                 < rows are then ignored) which the kernel splits into its fp16 operand per row at a power-of-two scale.  fp16 tokens take
 *                 the two-tensor form only (local_logits NULL, part_marg_f16 NULL); HICOM_EUNSUP otherwise */
int hicom_fused_stream_fwd(const void* ff, const void* fe, const float* local_logits, int32_t T, int32_t H, int32_t W, int32_t E,
                           int32_t kt, int32_t ks, const void* q_hi, const void* q_lo, int32_t rows,
                           float l_scale, float l_bias, const float* pos_a, int32_t pos_stride,
                           const void* pe_hi, const void* pe_lo,
                           int32_t t_index0, int32_t y_index0, int32_t x_index0,
                           float* part_m, float* part_l, float* part_acc, int32_t nparts, float* ctx_local,
                           void* ctx_hi, void* ctx_lo, void* ctx_f16, void* zero_ptr, int64_t zero_bytes, void* part_ctx_f16,
                           void* part_marg_f16, int32_t marg_slots, int32_t tok_dt, const float* q_f32, void* stream);
int hicom_fused_stream_nparts(int32_t n_windows);

/* ---- merge the partials (+ the value-side positional term) --------------------------------
 * out_acc[r,:] = sum_p e^(m_p - M_r) acc_p[r,:] + sum_n e^(s_n - M_r) pos(n)   (un-normalised)
 * out_ml[r]   = (M_r, L_r).  pos(n) = pe[t_index0+t] + pe[y_index0+y] + pe[x_index0+x] with
 * pe f32 [*, E] the per-axis sinusoid tables (projector.py:57-101), or NULL for no pos-emb.
 * scratch: f32 [rows * T * (H+W+2)] work area.  T = N / (H*W).  normalize != 0 divides by L_r
 * (single-shard case: out_acc is then the final context and no combine is needed). */
int hicom_global_merge_fwd(const float* part_m, const float* part_l, const float* part_acc,
                           int32_t nparts, int32_t rows, int32_t rows_pad, int32_t E,
                           const float* scores, int64_t score_stride, int64_t N,
                           int32_t H, int32_t W, const float* pe,
                           int32_t t_index0, int32_t y_index0, int32_t x_index0,
                           float* scratch, float* out_ml, float* out_acc, int32_t normalize, void* stream);

/* Merge behind hicom_global_stream_marg_fwd (same outputs; pe required; scratch as above, only the head of each row's region is
 * used for the row's weight record). */
int hicom_global_merge_marg_fwd(const float* part_m, const float* part_l, const float* part_acc, const float* part_marg,
                                int32_t nparts, int32_t rows, int32_t rows_pad, int32_t E, int64_t N,
                                int32_t H, int32_t W, const float* pe,
                                int32_t t_index0, int32_t y_index0, int32_t x_index0,
                                float* scratch, float* out_ml, float* out_acc, int32_t normalize, void* stream);

/* Combine `nsets` (M,L,ACC) triples (one per GPU after the all-gather, or one) and normalise:
 * ctx[r,:] = sum_k e^(M_k - M) ACC_k[r,:] / sum_k e^(M_k - M) L_k.
 * ml f32 [nsets, rows, 2]; acc f32 [nsets, rows, E]; ctx f32 [rows, E]. */
int hicom_global_combine_fwd(const float* ml, const float* acc, int32_t nsets, int32_t rows,
                             int32_t E, float* ctx, void* stream);

/* ---- readout MLP GEMM on matrix cores -------------------------------------------------------
 * y[out_row(m), :] = act(x[m,:] . w^T + b),  x f32 [M,K] (split hi/lo on the fly), w bf16 [N,K],
 * b bf16|f32 [N].  out_row(m) = row0 + m + (nl_group ? m / nl_group : 0) implements the
 * newline-interleaved packing of post_process_visual_feature (mm_utils.py:100-135).
 * Replaces build_mlp's Linear/GELU/Linear (projector.py:307-312,559,646).
 * K % 64 == 0; y dtype y_dt, row length ldy elements. */
int hicom_readout_gemm_fwd(const float* x, const void* w, const void* b, int32_t b_dt,
                           int32_t M, int32_t N, int32_t K, int32_t act,
                           void* y, int32_t y_dt, int64_t ldy, int64_t row0, int32_t nl_group,
                           void* stream);

/* Same GEMM on bf16 PLANES (the hot path): the activation arrives already split as a_hi + a_lo
 * (bf16 [M,K] each, written by the producing kernel), so all three operands go HBM -> LDS by LDS-DMA.
 * a_lo may be NULL when the activation is exactly bf16 (raw visual tokens).
 * Outputs (either or both): out_hi/out_lo = bf16 planes [M,N] of the result (feeds the next GEMM);
 * y = packed rows as in hicom_readout_gemm_fwd. */
int hicom_planes_gemm_fwd(const void* a_hi, const void* a_lo, const void* w, const void* b, int32_t b_dt,
                          int32_t M, int32_t N, int32_t K, int32_t act, void* out_hi, void* out_lo,
                          void* y, int32_t y_dt, int64_t ldy, int64_t row0, int32_t nl_group, void* stream);

/* ---- hot-path readout GEMM: ONE fp16 plane, with an optional co-scheduled GEMV ---------------------------------
 * y[out_row(m), :] / out_f16[m, :] = act(a[m,:] . w^T + b): a fp16 [M,K] (window contexts / hidden activations written
 * by the producing kernel), w fp16 [N,K] (hicom_to_f16_fwd of the bf16 nn.Linear weight, cached per weight version by the
 * caller), b bf16|f32 [N].  fp16 keeps 11 significand bits of the activation (<= 2^-12 relative, against the 1e-3
 * budget) at half the operand bytes and MFMAs of the hi/lo bf16 planes.  K % 64 == 0.
 * aux (may be NULL): a single-row linear layer executed by extra workgroups of the SAME launch on the CUs the tile grid
 * leaves idle -- the global compressor's out_proj / readout layers ride under the two local readout GEMMs:
 *   y[n] = act(sum_k w[n,k] x[k] + b[n]) + res[n],  x[k] = sum_{s < x_parts} xs[s * x_stride + k] + xb[k]
 * (xb, res bf16; w, b bf16 or f32 (w_dt / b_dt); xs, y f32; K <= 1536, K % 8 == 0). */
typedef struct hicom_aux_gemv {
    const float* xs;
    int32_t x_parts;
    int64_t x_stride;
    const void* xb;
    const void* w;
    const void* b;
    const void* res;
    int32_t N, K, act;
    float* y;                  /* f32 [N]; may be NULL when rows_dst is given */
    int32_t w_dt, b_dt;        /* HICOM_DT_BF16 | HICOM_DT_F32 (f32: products of weight matrices cached by the caller) */
    /* optional: the result row replicated into rows rows_row0 .. rows_row0 + rows_reps - 1 of rows_dst [*, rows_ld]
     * (dtype rows_dt): the 32 identical global rows of "direct" mode (projector.py:646,707) */
    void* rows_dst;
    int32_t rows_dt, rows_reps;
    int64_t rows_ld, rows_row0;
    /* alternative source of x: x[k] = x_fixed[k] / HICOM_FIXED_SCALE + xb[k] (hicom_merge_vproj_fixed_fwd's accumulators); then xs
     * may be NULL and x_parts is ignored */
    const int64_t* x_fixed;
    /* GEMV_CHAIN only (ABI 15): once every role workgroup has read x (= when a workgroup has swept every granule of the first layer),
     * role workgroup 0 clears the x_fixed accumulators for the next step -- the FINISH phase of the frame-sharded step then needs no
     * memset launch in front of its merge.  The accumulators must be zero before the FIRST step. */
    int32_t x_fixed_clear;
} hicom_aux_gemv;
int hicom_readout16_gemm_fwd(const void* a, const void* w, const void* b, int32_t b_dt,
                             int32_t M, int32_t N, int32_t K, int32_t act, void* out_f16,
                             void* y, int32_t y_dt, int64_t ldy, int64_t row0, int32_t nl_group,
                             const hicom_aux_gemv* aux, void* stream);
/* The same launch with a ROLE for the workgroups behind the tile grid (round 5: four launches per step of the release recipe):
 *   HICOM_ROLE_GEMV         `gemv`, as hicom_readout16_gemm_fwd's aux;
 *   HICOM_ROLE_MERGE_VPROJ  the (head, 64-channel slab) items of hicom_merge_vproj_fixed_fwd (fp16 partial contexts only): the merge
 *                           of the ring kernel's partial states (projector.py:193-215 after folding) is independent of the local
 *                           readout (projector.py:559), so it rides under readout GEMM 1 and its launch disappears;
 *   HICOM_ROLE_GEMV_CHAIN   two dependent single-row layers in one launch: h = act(gemv.w . x + gemv.b) with x from gemv.x_fixed,
 *                           then gemv2 with x = h (gemv2.K == gemv.N <= 1536, gemv2.w bf16): GELU(C o + r0) and the last global
 *                           readout layer (projector.py:226, :646, :307-312) under readout GEMM 2.  h travels between the role's
 *                           workgroups as {epoch, value} granules in `chain_state` (hicom_r16_chain_state_bytes(gemv.N) bytes,
 *                           zeroed ONCE by the caller, owned by one plan: every launch on it must have the same tile grid); a
 *                           failed hand-off (bounded spin) writes NaN rows and counts in word 2 of the state block. */
#define HICOM_ROLE_NONE 0
#define HICOM_ROLE_GEMV 1
#define HICOM_ROLE_MERGE_VPROJ 2
#define HICOM_ROLE_GEMV_CHAIN 3
typedef struct hicom_r16_role {
    int32_t kind;
    hicom_aux_gemv gemv;
    hicom_aux_gemv gemv2;
    void* chain_state;
    /* MERGE_VPROJ: the arguments of hicom_merge_vproj_fixed_fwd */
    const float* part_m;
    const float* part_l;
    const void* part_acc;
    int32_t part_dt, nparts, rows, rows_pad, E;
    const void* w_v;           /* NULL (with o_fix NULL): merge only, no v_proj -- the shard state of the frame-sharded path */
    int64_t* o_fix;
    float* out_ml;
    float* out_ctx;
    int32_t ctx_unnorm;        /* out_ctx receives the un-normalised accumulator sum_i e^(m_i - M) ACC_i (with out_ml = (M, L): a shard STATE) */
    /* value-side pos-emb in the merge (ABI 15; replaces `ff += pos` of projector.py:636-640 on the VALUE side): part_marg = fp16
     * [nparts][rows][marg_slots], the NORMALISED t / y / x marginals of every partial's softmax weights in absolute slot order
     * [T | H | W | zero padding] (hicom_fused_stream_fwd's part_marg_f16); vpe_f16 = fp16 [E][marg_slots] = v_proj.weight . pe^T over the
     * same slots (weight-only).  o_fix then receives W_v (ctx + sum_s mg[s] pe[s]).  marg_slots = 8 * (E / 64).  NULL: the partial
     * contexts already carry the pos-emb (or there is none). */
    const void* part_marg;
    const void* vpe_f16;
    int32_t marg_slots;
} hicom_r16_role;
int hicom_readout16_gemm_role_fwd(const void* a, const void* w, const void* b, int32_t b_dt,
                                  int32_t M, int32_t N, int32_t K, int32_t act, void* out_f16,
                                  void* y, int32_t y_dt, int64_t ldy, int64_t row0, int32_t nl_group,
                                  const hicom_r16_role* role, void* stream);
int64_t hicom_r16_chain_state_bytes(int32_t n_mid);
/* The GEMV chain as a launch of its own (no tile grid): role.kind must be HICOM_ROLE_GEMV_CHAIN.  The FINISH phase of the frame-sharded
 * step: GELU(C o + r0) and the last global readout layer behind the merge of the gathered shard states. */
int hicom_gemv_chain_fwd(const hicom_r16_role* role, void* stream);
/* The readout tail as ONE launch (replaces nn.Linear / GELU / nn.Linear of the local readout, projector.py:307-312,559, with the merge of
 * the global partial states, v_proj, out_proj and the global readout, projector.py:226,640-646, riding beside them): GEMM 1's tiles
 * publish the fp16 hidden plane inside the launch, the role workgroups run `merge` then `chain`, GEMM 2's tiles consume the plane row
 * block by row block.  g2->a must be g1->out_f16.  `state`: hicom_readout_tail_state_bytes() bytes, 128-byte aligned, zeroed ONCE
 * (the counters are cumulative); one state block per stream of launches.  HICOM_EUNSUP for shapes outside the fused form (the
 * caller then issues the two hicom_readout16_gemm_role_fwd launches). */
typedef struct hicom_r16_gemm {
    const void* a;             /* fp16 [M, K] */
    const void* w;             /* fp16 [N, K] */
    const void* b;             /* bias [N] (b_dt) or NULL */
    int32_t b_dt, M, N, K, act;
    void* out_f16;             /* fp16 [M, N] plane, or NULL */
    void* y;                   /* packed rows (y_dt), or NULL */
    int32_t y_dt;
    int64_t ldy, row0;
    int32_t nl_group;
} hicom_r16_gemm;
int64_t hicom_readout_tail_state_bytes(void);
int hicom_readout_tail_fwd(const hicom_r16_gemm* g1, const hicom_r16_gemm* g2, const hicom_r16_role* merge, const hicom_r16_role* chain,
                           void* state, void* stream);
/* hicom_merge_vproj_fixed_fwd over shard STATES as hicom_compressor_fwd's STREAM phase leaves them: `nsets` sets, `set_stride` floats apart,
 * each [(M, L) x rows | ACC rows x E] with un-normalised f32 accumulators.  o_fix as above (zero on entry). */
int hicom_merge_vproj_sets_fwd(const float* sets, int64_t set_stride, int32_t nsets, int32_t rows, int32_t E, const void* w_v, int64_t* o_fix,
                               float* out_ml, float* out_ctx, void* stream);
/* dst fp16 [rows, ld_dst] = saturating cast of src (bf16 or f32) [rows, cols]; columns [cols, ld_dst) are zero-filled */
int hicom_to_f16_fwd(const void* src, int32_t src_dt, void* dst, int64_t n, void* stream);
/* ABI 15: contiguous 16-bit <-> 16-bit cast, fp16 -> bf16 (round to nearest even) or bf16 -> fp16 (saturating); 16-byte aligned tensors.
 * The boundary's fp16 width: the reference's inference default is fp16 (inference_video_mcqa_videomme.py:323, model/__init__.py:44,
 * projector.py:53 `load_mm_projector` casts to fp16).  The release recipe takes fp16 tokens natively (hicom_compressor_args.tok_dt,
 * ABI 16: no cast, fp16 output from the fp32 accumulators); every other path of an fp16 projector still runs on the bf16 kernels through
 * casts of its inputs and of its result (hicom_amd/projector.py: HIComProjector._forward_half). */
int hicom_cast16_fwd(const void* src, int32_t src_dt, void* dst, int32_t dst_dt, int64_t n, void* stream);
int hicom_to_f16_padded_fwd(const void* src, int32_t src_dt, int64_t rows, int64_t cols, void* dst, int64_t ld_dst, void* stream);

/* Release recipe, one query row per head: merge of the ring kernel's partial states fused with v_proj
 * (projector.py:182,215 after folding).  po f32 [E/64][E]: partial v_proj outputs per 64-channel slab of the context,
 * summed in slab order by the consumer (hicom_readout16_gemm_fwd's aux GEMV with x_parts = E/64).  out_ml [rows][2] and
 * out_ctx [rows][E] (normalised contexts) may be NULL. */
int hicom_merge_vproj_fwd(const float* part_m, const float* part_l, const float* part_acc, int32_t nparts,
                          int32_t rows, int32_t rows_pad, int32_t E, const void* w_v, float* po,
                          float* out_ml, float* out_ctx, void* stream);
/* The same with the slab sums taken inside the launch: o_fix int64 [E] receives sum_slabs po[slab][:] as FIXED-POINT values
 * (value * 2^36 = HICOM_FIXED_SCALE; integer atomic adds, i.e. bit-identical results whatever the arrival order).  o_fix must be
 * ZERO on entry (hicom_fused_stream_fwd's zero_ptr: the launch in front of this one clears it).  part_dt HICOM_DT_F32: part_acc
 * are the un-normalised fp32 accumulators; HICOM_DT_F16: the normalised fp16 contexts (part_ctx_f16).  The consumer reads o_fix through
 * hicom_aux_gemv.x_fixed: one 9-KB vector instead of E/64 partial vectors per workgroup. */
#define HICOM_FIXED_SCALE 68719476736.0f
int hicom_merge_vproj_fixed_fwd(const float* part_m, const float* part_l, const void* part_acc, int32_t part_dt, int32_t nparts,
                                int32_t rows, int32_t rows_pad, int32_t E, const void* w_v, int64_t* o_fix,
                                float* out_ml, float* out_ctx, void* stream);

/* ---- dense 16-bit MFMA GEMM over all tokens (M = T*729) ------------------------------------------------------------
 * C = epilogue(A[M,K] . W[N,K]^T + b): A, W both fp16 or both bf16 (operand_dt), leading dimensions lda / ldw elements,
 * K % 64 == 0 (pad with zero columns), fp32 accumulation; act NONE | GELU (erf) | GELU_TANH.  Outputs, any subset:
 *   out_f16 [M, ldo] fp16 (saturating): the activated value; columns [N, n_store) are written as zeros (the K padding
 *           of a following GEMM);
 *   pre_f16 [M, ldpre] fp16 (saturating; may be NULL): acc + b BEFORE the activation -- what the activation's backward needs, kept by
 *           the training forward of the adaptor MLPs (needs N % 8 == 0, ldpre % 8 == 0, 16-byte aligned rows);
 *   y [M, ldy] bf16 | f32: value + res[m, n] (res bf16 [M, ldr] or NULL);
 *   ssq f32 [ceil(N/64)][M]: partial row sums of squares of (acc + b) per 64-column slice, summed by the consumer (key norms of the
 *           clip-scale global stage, projector.py:184-186).
 *   row_dot f32 [ceil(N/64)][M]: partial dot products sum_n dot_vec[n] * (value + res)[m, n] per 64-column slice (dot_vec bf16 | f32
 *           [N], 16-byte aligned; needs N % 8 == 0 and 16-byte aligned rows).  With the guide embedding as dot_vec on the fc2
 *           launch of the SigLIP head projection (encoder.py:284-286) the sum over slices IS the local logit frames_embed_n . guide
 *           of projector.py:551 before scaling: y may then be NULL and frames_embed is never written.
 * row_tab (may be NULL): f32 [*, row_tab_ld] table whose rows tab_t0 + m / (H*W), tab_y0 + (m / W) % H, tab_x0 + m % W are
 *           added to row m before bias / ssq / activation: the projected positional embedding W . pos(m) of token m,
 *           separable per axis (projector.py:57-101 through k_proj), so that x + pos is never formed.
 * The matrix-core-bound neighbours of the compressor: the SigLIP pooling-head projection that produces frames_embed
 * (encoder.py:284-286), the k / v adaptor MLPs (projector.py:533-534). */
int hicom_dense16_gemm_fwd(const void* a, int64_t lda, const void* w, int64_t ldw, int32_t operand_dt,
                           const void* b, int32_t b_dt, int32_t M, int32_t N, int32_t K, int32_t act,
                           void* out_f16, int64_t ldo, int32_t n_store, void* pre_f16, int64_t ldpre,
                           void* y, int32_t y_dt, int64_t ldy, const void* res, int64_t ldr,
                           float* ssq, const float* row_tab, int64_t row_tab_ld, int32_t tab_H, int32_t tab_W,
                           int32_t tab_t0, int32_t tab_y0, int32_t tab_x0,
                           const void* dot_vec, int32_t dot_vec_dt, float* row_dot, void* stream);
/* The same for TWO problems of one shape in ONE launch (fp16 outputs only): the same layer of the k and of the v adaptor MLP
 * (projector.py:533-534).  The tiles of both problems share the last, partly filled round of workgroup slots. */
int hicom_dense16_gemm_pair_fwd(const void* a_k, const void* w_k, const void* b_k, void* out_k, void* pre_k,
                                const void* a_v, const void* w_v, const void* b_v, void* out_v, void* pre_v,
                                int64_t lda, int64_t ldw, int32_t operand_dt, int32_t b_dt, int32_t M, int32_t N, int32_t K, int32_t act,
                                int64_t ldo, int32_t n_store, int64_t ldpre, void* stream);
/* TN form: c_parts[s][m][n] = sum over the s-th slice of the Kt rows of a[k][m] * b[k][n] -- the weight gradients dW = dY^T X of the
 * token-stream layers (a = dY [Kt, lda], b = X [Kt, ldb], both token-major, both fp16 or both bf16; fp32 accumulation).  The
 * contraction axis is split into `splits` slices (hicom_dense16_tn_splits proposes a count), each writing its own f32 partial
 * [M][ldc]; hicom_partials_sum_fwd(c_parts, splits, M * ldc, out) adds them in slice order (deterministic).  M, N, lda, ldb
 * multiples of 8, ldc of 4; Kt arbitrary. */
int hicom_dense16_tn_splits(int32_t M, int32_t N, int64_t Kt);
int hicom_dense16_tn_fwd(const void* a, int64_t lda, const void* b, int64_t ldb, int32_t operand_dt, int64_t Kt,
                         int32_t M, int32_t N, float* c_parts, int64_t ldc, int32_t splits, void* stream);
/* out[m] = sum_{s < nparts} parts[s * M + m], in slice order (the row_dot partials of hicom_dense16_gemm_fwd -> the per-token
 * local logits hicom_fused_stream_fwd / hicom_compressor_args.local_logits take). */
int hicom_partials_sum_fwd(const float* parts, int32_t nparts, int64_t M, float* out, void* stream);

/* ---- clip-scale on the global stage (projector.py:184-191) ---------------------------------------------------------
 * hicom_clip_query_prep_fwd: qp f32 [nq, E] (q_proj output) is L2-normalised in place over E; c[q*nh + h] =
 *   scale * sum_j qhat[q, h*hd + j] * b_k[h*hd + j]  (the key-bias part of the logit, which no longer cancels once
 *   every key is divided by its own norm).  b_k bf16 [E] or NULL.
 * hicom_inv_norm_fwd: inv[m] = 1 / sqrt(sum_{s < parts} ssq[s * M + m])  (key norms from hicom_dense16_gemm_fwd's ssq). */
int hicom_clip_query_prep_fwd(float* qp, const void* b_k, int32_t nq, int32_t nh, int32_t E, float scale, float* c, void* stream);
int hicom_inv_norm_fwd(const float* ssq, int32_t parts, int64_t M, float* inv, void* stream);
/* out[m,:] = x[m,:] / ||x[m,:]||_2, bf16 [M, E] -> bf16 [M, E] (E % 8 == 0, E <= 1536): frames_embed of the clip-scale local stage
 * when the k adaptor follows it (projector.py:527-529 in front of :533; without adaptor the window kernel normalises in place). */
int hicom_l2norm_stream_fwd(const void* x, void* out, int64_t M, int32_t E, void* stream);
/* out[m,:] = (1 - alpha) src[m,:] + alpha (LayerNorm_eps(x[m,:]) gamma + beta) over all tokens with 16-byte accesses:
 * x fp16 | bf16 | f32 [M, ldx]; gamma, beta, src (may be NULL) bf16; alpha device scalar or NULL (= 1); out fp16 | bf16
 * [M, E]; E % 8 == 0, E <= 1536.  head.layernorm of encoder.py:284 and the adaptor blend of projector.py:533-534. */
int hicom_ln_stream_fwd(const void* x, int32_t x_dt, int64_t ldx, const void* gamma, const void* beta,
                        const void* src, const void* alpha, int32_t alpha_dt, float eps,
                        void* out, int32_t out_dt, int32_t M, int32_t E, void* stream);

/* Row copy / broadcast with dtype conversion into the packed output:
 *   dst[row0 + i*row_step + (nl_group ? i / nl_group : 0), :] = src[(i % src_rows), :],  i in [0,count)
 * (newline tokens, the 32 identical global rows of "direct" mode, and the standalone
 * post_process_visual_feature packing of mm_utils.py:92-140). */
int hicom_scatter_rows_fwd(const void* src, int32_t src_dt, int32_t src_rows, int32_t ncols,
                           void* dst, int32_t dst_dt, int64_t ldd, int64_t row0, int64_t row_step,
                           int32_t nl_group, int32_t count, void* stream);

/* Rows of `nblocks` equal blocks lying `block_stride_bytes` apart (the per-rank segments of an all-gathered
 * buffer) -> consecutive packed rows of dst starting at row0, skipping one row after every nl_group rows (the
 * newline slots of mm_utils.py:100-135); same dtype on both sides, rows and strides multiples of 16 bytes.
 * Used by the frame-sharded path to place every rank's local tokens with one launch. */
int hicom_place_blocks_fwd(const void* src, int32_t block_rows, int32_t nblocks, int64_t block_stride_bytes,
                           int32_t row_bytes, void* dst, int64_t ldd_bytes, int64_t row0, int32_t nl_group,
                           void* stream);

/* Same, with the per-set (M,L) pairs and ACC blocks `set_stride` floats apart (the layout of the
 * all-gathered per-rank buffers): ml_k = ml + k*set_stride, acc_k = acc + k*set_stride. */
int hicom_global_combine_strided_fwd(const float* ml, const float* acc, int64_t set_stride, int32_t nsets,
                                     int32_t rows, int32_t E, float* ctx, void* stream);

/* ---- instruction injector / adaptor row operators -------------------------------------------
 * out = (1 - alpha) * src + alpha * (LayerNorm_eps(x * (1 + mul) + add) * gamma + beta), row-wise over E.
 * Covers GuideInjector "coarse" (FiLM + LayerNorm, projector.py:369-372: mul/add = one broadcast
 * row, stride 0), "fine" (LayerNorm(q + attn), :392: add per row), and the alpha-blended adaptors
 * (adapt_guide :365, adapt_q :541, adapt_k / adapt_v :533-534).  mul / add / src / alpha may be NULL
 * (alpha == NULL means 1 and needs no src); alpha is a 1-element DEVICE tensor (the nn.Parameter). */
int hicom_row_ln_fwd(const void* x, int32_t x_dt, int64_t x_stride,
                     const float* mul, int64_t mul_stride, const float* add, int64_t add_stride,
                     const void* gamma, const void* beta, int32_t gb_dt,
                     const void* src, int32_t src_dt, int64_t src_stride,
                     const void* alpha, int32_t alpha_dt, float eps,
                     void* out, int32_t out_dt, int64_t out_stride, int32_t M, int32_t E, void* stream);

/* Multi-head attention of M query rows over L <= 64 keys (the text tokens of "fine" injection,
 * projector.py:391 -> :193-215): q [M,E], k, v [L,E] are the PROJECTED states (f32), heads of hd
 * channels, scale hd^-1/2, fp32 softmax; out [M,E] f32 (before out_proj). */
int hicom_small_mha_fwd(const float* q, const float* k, const float* v, int32_t M, int32_t L,
                        int32_t nh, int32_t hd, float* out, void* stream);
/* The same with the logit scale given: the clip-scale form of projector.py:184-191 on the short-key branch passes the
 * L2-normalised projected states (hicom_clip_query_prep_fwd normalises rows in place) and scale = exp(logit_scale); the
 * additive logit_bias is a per-row shift that the softmax cancels. */
int hicom_small_mha_scaled_fwd(const float* q, const float* k, const float* v, int32_t M, int32_t L,
                               int32_t nh, int32_t hd, float scale, float* out, void* stream);

/* ---- splice of the compressed tokens into the LLM input embeddings (hicom_arch.py:271-373) ----------------------------
 * hicom_splice_rows_fwd: dst [nrows, row_bytes] <- row r copied from the DEVICE address row_src[r] (uint64 table on the
 *   device; 0 = a zero row: right padding).  Sources are rows of embed_tokens.weight and of the compressed-token tensors;
 *   the host (hicom_amd/splice.py) plans the table from the token ids.  row_bytes % 16 == 0.
 * hicom_splice_labels_fwd: new_labels int64 [B, Lmax] = labels[b, map[b,p]] where map >= 0, else ignore_index (visual
 *   tokens and padding, :309-311,:344-348); new_mask [B, Lmax] = ones for the first new_len[b] - S positions, then the
 *   original mask row, then zeros (:350-366); mask elements 1 (torch.bool) or 8 (torch.long) bytes.  labels / new_labels or
 *   mask / new_mask may be NULL. */
int hicom_splice_rows_fwd(const void* row_src, int64_t nrows, int32_t row_bytes, void* dst, void* stream);
int hicom_splice_labels_fwd(const void* labels, const void* mask, int32_t mask_elem_bytes, const int32_t* map,
                            const int32_t* new_len, int32_t B, int32_t S, int32_t Lmax, int64_t ignore_index,
                            void* new_labels, void* new_mask, void* stream);

/* ---- whole-forward executor ------------------------------------------------------------------
 * hicom_compressor_fwd enqueues HIComProjector.forward (projector.py:676-708) for one dense
 * [T,H,W,E] input as a fixed plan of kernel launches over a caller-owned workspace.  Release recipe
 * (use_guide = "direct", exact window partition, solo call): everything in order on stream_main -- query prep, the
 * fused stream kernel, merge + v_proj, the two readout GEMMs with the global tail's GEMVs riding in their launches;
 * no side stream, no events.  Generic recipes and the deferred / frame-sharded forms: the local chain on stream_main,
 * the global chain on stream_side (fork/join through ev_fork / ev_join).
 *
 * phases: HICOM_PHASE_STREAM = everything that touches the frames (local tokens, and the
 *         global online-softmax state); HICOM_PHASE_FINISH = the 32 global rows from the state.
 *         A single GPU passes both.  The frame-sharded path runs STREAM with local_out /
 *         state_out pointing into its send buffer, all-gathers, then runs FINISH with state_sets.
 * workspace: hicom_compressor_workspace_bytes(args) bytes, 256-B aligned; its first
 *         hicom_compressor_zero_prefix_bytes(args) bytes must be zeroed ONCE by the caller
 *         (padding rows the kernels never write) and the buffer must not be shared between
 *         concurrently running forwards. */
#define HICOM_PHASE_STREAM 1
#define HICOM_PHASE_FINISH 2
/* With HICOM_PHASE_STREAM on the release recipe, for the frame-sharded step: no side stream at all -- the merge of the
 * partial states runs on stream_next after it has been made to wait for ev_done (both required), i.e. on the comm
 * stream right in front of the all-gather.  Saves the fork / join / ev_merge event traffic (~17 us of host time per
 * step); the caller gives every buffer set its own workspace, since the merge then reads the partials while the
 * main stream may already run the next step. */
#define HICOM_PHASE_MERGE_ON_NEXT 4
/* With HICOM_PHASE_MERGE_ON_NEXT (ABI 15): "next" is this call's own stream_main -- a JOINED frame-sharded step runs both phases on the
 * caller's stream (which may be the null stream, handle 0: stream_next is ignored) and the executor puts no event wait between them. */
#define HICOM_PHASE_NEXT_IS_MAIN 8

typedef struct hicom_compressor_args {
    /* inputs: frames_feature (values; keys/values of the global stage), frames_embed (local keys, may be NULL) */
    const void* ff;
    const void* fe;
    int32_t T, H, W, E;
    int32_t has_local, has_global, phases, hidden;
    /* local compressor */
    hicom_axis at, ay, ax;
    const void* lq;            /* shared [E] (stride 0) or per-window query; NULL = pooled (guide off) */
    int32_t lq_dt;
    int32_t l2norm;
    int64_t lq_stride;
    float l_scale, l_bias;
    const void *lw0, *lb0, *lw2, *lb2;          /* readout Linear(E,hidden), Linear(hidden,hidden): bf16 */
    const void *lw0_f16, *lw2_f16;              /* fp16 copies of lw0 / lw2 (hicom_to_f16_fwd, cached by the caller per weight
                                                   version): the release recipe then runs its readout on one fp16 plane
                                                   (hicom_readout16_gemm_fwd); NULL = bf16 hi/lo planes (hicom_planes_gemm_fwd) */
    /* global compressor */
    const void* gq;            /* bf16 [nq, E] injected queries (1 row in "direct" mode) */
    int32_t nq, nh, n_global_rows, P;
    const void *wq, *bq, *wk, *wv, *bv, *wo, *bo;
    const void *gw0, *gb0, *gw2, *gb2;
    const float* pe;           /* f32 [P, E] stacked per-axis sinusoid tables, or NULL (no pos-emb) */
    const float* kpe;          /* f32 [E, P] = w_k . pe^T (weight-only cache) */
    const void *pe_hi, *pe_lo; /* bf16 [P, E] hi / lo planes of pe (hicom_split_bf16_fwd; cached with pe) */
    int32_t t_index0, y_index0, x_index0, nsets;
    /* output [rows, ldo] of dtype out_dt */
    void* out;
    int32_t out_dt, nl_group;
    int64_t ldo, local_row0, global_row0;
    const void* newline;       /* newline token [hidden] or NULL */
    int32_t newline_dt, nl_count;
    int64_t nl_first, nl_step;
    /* frame-sharded operation (all NULL / 0 on a single GPU) */
    void* local_out;           /* dense [Nw, hidden] (out_dt) instead of packed rows of `out` */
    void* state_out;           /* f32 [2R + R*E]: un-normalised (M,L) pairs then ACC of this shard */
    const void* state_sets;    /* gathered states, nsets blocks state_set_stride floats apart */
    int64_t state_set_stride;
    /* execution resources */
    void* ws;
    int64_t ws_bytes;
    void *stream_main, *stream_side, *ev_fork, *ev_join;
    /* Deferred join (release recipe only): with defer_join != 0 the main stream does NOT wait for the side stream's
     * global chain at the end of the call -- the 32 global rows of `out` are complete when ev_join (recorded on the
     * side stream) has fired, so the chain of one video overlaps the streaming of the next.  ev_merge (may be NULL
     * when defer_join == 0) is recorded after the merge kernel and waited on before the next stream kernel, which
     * overwrites the partial states the merge reads.  Generic path with many query rows (guide off: 288): when given, the side
     * stream launches the stream kernel first and records ev_merge behind it, the main stream waits for it before the local
     * chain -- the stream kernel runs alone, the local chain beside the global tail. */
    void* ev_merge;
    int32_t defer_join, reserved_;
    /* Frame-sharded serving (hicom_amd/dist.py): what follows a phase on its own stream, so that one C call enqueues
     * it all (each separate host call costs 3-6 us, and the sharded step is host-bound).
     *   place_src != NULL (FINISH phase): the gathered per-rank token blocks -- place_nblocks blocks of
     *     place_block_rows rows of `hidden` elements, place_block_stride bytes apart -- are placed into the packed
     *     rows of `out` from row 0 (newline gaps as in nl_group), as hicom_place_blocks_fwd does;
     *   ev_done != NULL: recorded at the end of the call on the stream the phase ran on (after the join);
     *   stream_next != NULL (needs ev_done): that stream is made to wait for ev_done. */
    const void* place_src;
    int64_t place_block_stride;
    int32_t place_block_rows, place_nblocks;
    void *ev_done, *stream_next;
    /* gc0: f32 [hidden, E] = gw0 . wo, the first global readout layer folded over out_proj (weight-only, cached by the
     * caller per weight state like kpe), or NULL.  With it the release recipe's step is five launches:
     * hicom_query_prep_fwd | fused stream | merge + v_proj | readout GEMM 1 (+ GELU(gc0 o + r0)) | readout GEMM 2 (+ the
     * last global readout layer -> the 32 global rows). */
    const float* gc0;
    /* local_logits: f32 [T*H*W] = frames_embed_n . guide per token, or NULL (release recipe only; see hicom_fused_stream_fwd) */
    const float* local_logits;
    /* reuse_queries != 0 (generic recipes, guide off only): the folded queries / score-side positional table in the workspace are
     * those of an earlier call with the SAME weights -- the injected queries are the learnable `query` parameter (IdentityMap,
     * projector.py:586-587), so q_proj + fold are weight-only work like kpe -- and the two prep launches are skipped.  The caller
     * clears it after a weight update. */
    int32_t reuse_queries;
    /* k / v adaptors of the local stage (projector.py:431-457, :533-534: key = (1 - a) x + a LN(MLP(x)) over ALL tokens; likewise
     * the values), the second released recipe `local43_adaptkv_global32`.  ak.w0 / av.w0 NULL = that stream has no adaptor.  The
     * executor runs the two dense GEMMs per stream (hicom_dense16_gemm_fwd) and the window attention with the LayerNorm + alpha
     * blend fused into its row loads (hicom_local_attn_adapt_fwd); not with clip-scale (l2norm != 0) and not on the release
     * recipe's single-kernel path (the local stage then reads adapted streams, the global stage the raw tokens). */
    struct hicom_adaptor {
        const void *w0, *b0;       /* Linear(E, E): bf16 [E, E], bf16 [E] */
        const void *w2_f16, *b2;   /* Linear(E, E): fp16 copy of the weight (cached by the caller per weight state), bf16 bias */
        const void *gamma, *beta;  /* LayerNorm: bf16 [E] */
        const void* alpha;         /* device scalar, dtype adapt_alpha_dt */
        const void* y;             /* optional: fp16 [T*H*W, E] = MLP(x) of this stream, already computed by the caller (the training
                                    * forward keeps the MLP's intermediates for its backward): the adaptor's two GEMMs are skipped */
    } ak, av;
    int32_t adapt_alpha_dt;
    float adapt_eps;
    /* r0_buf (frame-sharded release recipe, may be NULL): f32 [hidden] in CALLER memory that carries r0 = G0 (b_o + g) + g_b0 from the
     * STREAM phase (query prep writes it there) to the FINISH phase (the chain launch reads it), whose workspaces are separate.  With it
     * (and gc0, one query row per head, hidden <= 1536) the sharded step takes the four-launch form: the shard's state (M, L, ACC)
     * comes out of the merge ROLE of readout GEMM 1's launch, and FINISH is [memset | merge of the gathered states + v_proj |
     * chain launch -> 32 rows | token placement]. */
    float* r0_buf;
    /* dtype of gq (HICOM_DT_BF16 = 0, the learnable queries / the guide, or HICOM_DT_F32: queries a guide injector produced on the
     * caller's side -- coarse / fine injection, projector.py:369-397 -- handed in as f32 rows; with lq f32 [windows, E] the same way).
     * The release-recipe paths (query_prep kernel, fused stream kernel) take bf16 queries, or -- ABI 16, tok_dt = HICOM_DT_F16 -- the
     * fp16 guide (HICOM_DT_F16, with lq_dt = HICOM_DT_F16). */
    int32_t gq_dt;
    /* optional hipEvent_t: the main stream waits for it in front of the local stage's first launch -- the caller produces lq (injected
     * per-window queries) on a stream of its own, beside the global stage's stream kernel, and records this event behind it */
    void* ev_queries;
    /* GuideInjector.forward inside the call (projector.py:369-397), plain injectors (no text2qk projection, no adapt_guide): the local
     * stage injects the guide into its pooled per-window queries (lq must be NULL), the global stage into `visual` = its learnable
     * queries (gq is ignored).  STREAM | FINISH in one call only (the injected rows live in this call's workspace). */
    struct hicom_injector {
        int32_t mode;              /* 0: none; 1: coarse = LN(v (1 + scale) + shift), (scale | shift) = MLP(guide) (:370-372);
                                    * 2: fine = LN(v + MHA(v, guide tokens)) (:391-392) */
        const void* guide;         /* bf16 [guide_rows, E]: one row (coarse) or <= 64 text tokens (fine) */
        int32_t guide_rows;
        const void *c_w0, *c_b0, *c_w2, *c_b2;       /* coarse_proj: Linear(E, c_hidden) GELU Linear(c_hidden, 2E), bf16 */
        int32_t c_hidden;
        const void *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo;   /* fine_proj (MultiheadAttention, :166-228), bf16 [E, E] / [E] */
        int32_t nheads;
        const void *ln_w, *ln_b;   /* coarse_norm / fine_norm, bf16 [E] */
        float eps;
        const void* visual;        /* global stage: bf16 [nq, E]; local stage: NULL */
    } inj_l, inj_g;
    /* ABI 15 (may be NULL / 0): fp16 [E][marg_slots] = v_proj.weight . pe^T over the slots [T frames | H rows | W columns | zero padding],
     * marg_slots = 8 * (E / 64) >= T + H + W: the release step then takes the value-side pos-emb out of the streaming kernel (its
     * marginals leave it, hicom_fused_stream_fwd's part_marg_f16) and applies it in the merge role of readout GEMM 1's launch
     * (hicom_r16_role.part_marg / vpe_f16).  Weight-only, cached by the caller per weight state like kpe. */
    const void* vpe_f16;
    int32_t marg_slots;
    /* ABI 15, FINISH phase of the frame-sharded step (all NULL / 0 otherwise): the all-gather of the per-rank exchange buffers enqueued
     * BY THIS CALL, on stream_main, in front of everything else -- `ag_fn` = address of ncclAllGather of the RCCL the process has loaded
     * (ncclResult_t (*)(const void* send, void* recv, size_t count, ncclDataType_t, ncclComm_t, hipStream_t)), `ag_comm` = the
     * ncclComm_t of the caller's process group (torch: ProcessGroupNCCL._comm_ptr()), ag_bytes per rank as ncclUint8.  The library does not
     * link RCCL: one host call per phase instead of a torch.distributed call between two (the sharded step is host-bound). */
    void* ag_fn;
    void* ag_comm;
    const void* ag_send;
    void* ag_recv;
    int64_t ag_bytes;
    /* ... or TWO all-gathers in one RCCL group (ag_group_start / ag_group_end = addresses of ncclGroupStart / ncclGroupEnd): the second
     * one (ag_send2 -> ag_recv2, ag_bytes2 per rank) carries the shard STATES into a [world][ag_bytes2] buffer (= state_sets), the first
     * the local token rows STRAIGHT into their rows of the output (ag_recv = out: without newline rows the ranks' blocks are consecutive
     * rows) -- no placement launch behind the collective (place_src NULL). */
    void* ag_group_start;
    void* ag_group_end;
    const void* ag_send2;
    void* ag_recv2;
    int64_t ag_bytes2;
    /* ABI 16: dtype of ff / fe, HICOM_DT_BF16 (0) or HICOM_DT_F16.  fp16 tokens run on the release recipe's single-stream form only
     * (hicom_compressor_is_fused reports it: fused stream kernel in its fp16 instantiation, an fp16 guide -- lq_dt = gq_dt = HICOM_DT_F16
     * -- or a bf16 one, output in out_dt = HICOM_DT_F16 / F32 / BF16 from the fp32 accumulators); every other path given fp16 tokens
     * returns HICOM_EUNSUP and never reads them as bf16. */
    int32_t tok_dt;
} hicom_compressor_args;

/* Byte offset, inside the workspace, of the fp16 plane [windows, E] of the local stage's window contexts (the A operand of readout
 * GEMM 1) that a hicom_compressor_fwd call with these arguments leaves behind -- what the training forward keeps for the backward
 * (the readout's weight gradients need the contexts; recomputing them is a pass over every token).  Negative: HICOM_EUNSUP when the
 * call does not read out through fp16 planes, HICOM_EINVAL without a local stage. */
int64_t hicom_compressor_ctx16_offset(const hicom_compressor_args* args);
/* Two calls of hicom_compressor_fwd in one (the STREAM and the FINISH block of a frame-sharded step; stops at the first error). */
int hicom_compressor_fwd2(const hicom_compressor_args* first, const hicom_compressor_args* second);
/* 1 when a STREAM-phase call with these arguments takes the four-launch sharded form that hands r0 to the FINISH phase through r0_buf,
 * 0 otherwise (the caller then clears r0_buf in BOTH blocks so that FINISH takes its generic form too: ADVICE r5). */
int hicom_compressor_takes_shard4(const hicom_compressor_args* args);
/* Failed in-launch hand-offs (bounded spins that expired: the affected rows were poisoned with NaN) counted so far in this workspace's
 * state blocks: out[0] = query prep, out[1] = the GEMV chain.  Synchronous (two 4-byte device reads on `stream` + a stream sync):
 * for tests, benches and debug checks, not for the hot loop. */
int hicom_compressor_handoff_failures(const hicom_compressor_args* args, int32_t* out, void* stream);
/* 1 when hicom_compressor_fwd takes the release-recipe (single streaming kernel) path for these arguments (fp16 tokens included). */
int hicom_compressor_is_fused(const hicom_compressor_args* args);

int64_t hicom_compressor_workspace_bytes(const hicom_compressor_args* args);
int64_t hicom_compressor_zero_prefix_bytes(const hicom_compressor_args* args);
int hicom_compressor_fwd(const hicom_compressor_args* args);

/* ---- batched compressor step: B items of ONE shape in one call --------------------------------------------------------
 * What hicom/model/hicom_arch.py:166-178 does with one projector call per item of a batch (all items of equal length), for the
 * release recipe only (local + global compressor, use_guide = "direct", no clip-scale, bf16; no adaptors here -- the k / v adaptors
 * of the local stage go through hicom_compressor_batch_adapt_* below, fourteen launches): twelve launches on `stream` whatever B
 * is.  Item b of the output equals hicom_compressor_fwd on item b alone (same math; the window contexts and the hidden
 * layer of the local readout pass through fp16 planes as there).
 *   ff, fe   : bf16 [B, T, H, W, E] (fe NULL: the local keys are ff); guide bf16 [B, E], one instruction per item
 *   kt, ks   : local window (kt = 1 for images); T % kt == H % ks == W % ks == 0, kt ks ks <= 64; E == 1152, nh <= 16 heads,
 *              hidden % 64 == 0; HICOM_EUNSUP otherwise
 *   pe, kpe  : the tables of hicom_compressor_args, both NULL = no pos-emb; the frame index of the positional terms restarts at
 *              t_index0 for every item
 *   chunks   : workgroups per item of the segmented global stream, 0 = chosen so that B x chunks fills the chip (one per item
 *              once B alone does).  A workgroup streams tokens of ONE item; the (m, l, ACC) states of an item's chunks are merged
 *              per item, a tail tile is masked
 *   out      : [B, item_rows, ldo] of out_dt (bf16 | f32), item_rows = global_row0 + n_global_rows.  Rows [0, global_row0) of an
 *              item: its local tokens, one newline gap after every nl_group of them (0: none), the newline token (bf16) in rows
 *              nl_first + i nl_step, i < nl_count; rows from global_row0: n_global_rows identical copies of its global token
 *   ws       : hicom_compressor_batch_workspace_bytes(args) bytes (depends on the shape, B and chunks), 256-byte aligned, nothing
 *              to zero; not shared between concurrently running calls */
typedef struct hicom_compressor_batch_args {
    const void* ff;
    const void* fe;
    const void* guide;
    int32_t B, T, H, W, E, hidden, kt, ks, nh, P;
    float l_scale;
    int32_t chunks;
    const void *lw0_f16, *lb0, *lw2_f16, *lb2;      /* local readout: fp16 copies of the weights, bf16 biases */
    const void *wq, *bq, *wk, *wv, *bv, *wo, *bo;   /* global attention, bf16 */
    const void *gw0, *gb0, *gw2, *gb2;              /* global readout, bf16 */
    const float* pe;
    const float* kpe;
    int32_t t_index0, y_index0, x_index0, out_dt;
    void* out;
    int64_t ldo, item_rows, global_row0;
    int32_t n_global_rows, nl_group, nl_count, reserved_;
    int64_t nl_first, nl_step;
    const void* newline;
    void* ws;
    int64_t ws_bytes;
    void* stream;
} hicom_compressor_batch_args;
int64_t hicom_compressor_batch_workspace_bytes(const hicom_compressor_batch_args* args);
int hicom_compressor_batch_fwd(const hicom_compressor_batch_args* args);

/* ---- ragged compressor step: B items of UNEQUAL length and mixed modality in one call ------------------------------
 * The batch of hicom/model/hicom_arch.py:146-180 as it comes: the vision tower's stacked [sum T_i, H, W, E] tensor (:159-164, before
 * .split) with single images, clips of any length and 1-frame "videos" side by side, read in place.  Same recipe, same math per item
 * and the same twelve launches as the batched step above; item i of the output equals hicom_compressor_fwd on item i alone.
 *   ff, fe   : bf16 [sum T_i, H, W, E] (fe NULL: the local keys are ff); guide bf16 [B, E]
 *   items    : HOST array of B descriptors.  T frames; kt the item's temporal window (1 for images and 1-frame items), T % kt == 0;
 *              the item's packed rows as in hicom_compressor_batch_args: a newline gap after every nl_group local tokens (0: none),
 *              the newline token in rows nl_first + i nl_step, i < nl_count, then n_global_rows copies of its global token.  An item
 *              has (T / kt)(H / ks)(W / ks) + nl_count + n_global_rows rows; the items' rows follow each other in `out`
 *   H, W, ks : common to the call, H % ks == W % ks == 0, kt ks ks <= 64; E == 1152, nh <= 16, hidden % 64 == 0
 *   pe, kpe  : as above; the frame index of the positional terms restarts at t_index0 for every item (the tables hold max T_i frames)
 *   chunks   : work units per item of the segmented global stream, each clamped to the item's 16-token tiles; 0 = the item's share
 *              of 2 x #CUs units by its tile count, in [1, 64].  A unit streams tokens of ONE item, tiles counted from the item's
 *              first token
 *   out      : [sum rows_i, ldo] of out_dt (bf16 | f32)
 *   ws       : hicom_compressor_ragged_workspace_bytes(args) bytes, 256-byte aligned.  Its head is a table region (item table, work
 *              units {item, first tile, last tile, partial-state slot}, window -> item and row -> item lookups) that
 *              hicom_compressor_ragged_prepare(args) derives on the host and writes ONCE per (items, shape, chunks, ws): it copies to
 *              the device and synchronises `stream`, so it runs outside the hot loop (and outside a graph capture).
 * hicom_compressor_ragged_fwd then only launches: no copy, no synchronisation, no allocation, O(B) integer work on the host.  It
 * trusts the table region: calling it on a workspace that prepare has not filled for the same items is undefined. */
typedef struct hicom_ragged_item {
    int32_t T, kt, nl_group, nl_count, nl_first, nl_step, n_global_rows;
} hicom_ragged_item;
typedef struct hicom_compressor_ragged_args {
    const void* ff;
    const void* fe;
    const void* guide;
    int32_t B, H, W, E, hidden, ks, nh, P;
    float l_scale;
    int32_t chunks;
    const hicom_ragged_item* items;                 /* HOST memory, B entries */
    const void *lw0_f16, *lb0, *lw2_f16, *lb2;      /* local readout: fp16 copies of the weights, bf16 biases */
    const void *wq, *bq, *wk, *wv, *bv, *wo, *bo;   /* global attention, bf16 */
    const void *gw0, *gb0, *gw2, *gb2;              /* global readout, bf16 */
    const float* pe;
    const float* kpe;
    int32_t t_index0, y_index0, x_index0, out_dt;
    void* out;
    int64_t ldo;
    const void* newline;
    void* ws;
    int64_t ws_bytes;
    void* stream;
} hicom_compressor_ragged_args;
int64_t hicom_compressor_ragged_workspace_bytes(const hicom_compressor_ragged_args* args);
int hicom_compressor_ragged_prepare(const hicom_compressor_ragged_args* args);
int hicom_compressor_ragged_fwd(const hicom_compressor_ragged_args* args);

/* ---- training step of the ragged call (plain recipe; HIComProjector.forward_ragged_train) -----------
 * Rows are item-major, R = B nh of them: row = item nh + head.  The scores region is the forward's own: item i's logits at
 * 16 score_off_i floats, [16][ceil16(N_i)], score_off_i = 16 sum_{j<i} ceil(N_j / 16).
 * hicom_compressor_ragged_train_state, after hicom_compressor_ragged_fwd on the same block: copies out of args->ws what a backward
 * reads -- ctx16 fp16 [windows, E], the scores region, ctxg f32 [R, E] -- and writes ml f32 [R][2] = (M, L) of every row from the
 * partial states, in the merge's summation order.  Device-to-device copies and one launch on args->stream; no synchronisation.
 * hicom_compressor_ragged_global_bwd: the attention backward of the global stage over all items, four launches whatever B and the
 * mix are (dctx -> bf16 hi / lo planes; pos_b = dctx . pe^T; the segmented backward stream, one workgroup per work unit of the
 * forward's unit table; the dq merge per (item, head)).  It reads only the table region of args->ws (hicom_compressor_ragged_prepare
 * wrote it) and args' shape, pe and stream; x are the tokens the forward read (args->ff may have been patched since).
 *   dctx f32 [R, E], delta f32 [R] = dctx_r . ctx_r, scores / ml as train_state left them
 *   ds_out   : f32, laid out as the scores region: dS; the padded tail columns of a row are zero
 *   dqt_out  : f32 [R, E] = sum_n dS[r, n] (x_n + pe_n): the x part from the stream, the positional part from dS's marginals
 *   ws       : hicom_compressor_ragged_global_bwd_workspace_bytes(args) bytes, 256-byte aligned
 * Neither call takes the sizes of the caller's buffers; with N_i = T_i H W tokens and w_i = (T_i / kt_i)(H / ks)(W / ks) windows per item:
 *   ctx16_out            2 E sum w_i bytes
 *   scores_out, ds_out   4 * 16 * sum 16 ceil(N_i / 16) bytes each (16 rows per item, the item's tokens padded to a tile)
 *   ml_out               8 B nh bytes;   ctxg_out, dqt_out, dctx   4 E B nh bytes each;   delta   4 B nh bytes
 * Only launches: no allocation, no host copy, no synchronisation. */
int hicom_compressor_ragged_train_state(const hicom_compressor_ragged_args* args, void* ctx16_out, float* scores_out, float* ml_out, float* ctxg_out);
int64_t hicom_compressor_ragged_global_bwd_workspace_bytes(const hicom_compressor_ragged_args* args);
int hicom_compressor_ragged_global_bwd(const hicom_compressor_ragged_args* args, const void* x, const float* dctx, const float* delta,
                                       const float* scores, const float* ml, float* ds_out, float* dqt_out, void* ws, int64_t ws_bytes);

/* ---- input gradients of the ragged training step (stage 3; forward_ragged_train(input_grads=True)) ----
 * Both calls read only the table region of args->ws and args' shape, l_scale and stream; both check their pointers and the per-item
 * partition in front of everything that needs a device.  Only launches: no allocation, no host copy, no synchronisation.
 * hicom_compressor_ragged_local_bwd: hicom_local_attn_bwd over the concatenated window list, one 4-wave workgroup per window with the
 * window's geometry from its item's own (T, kt), the tokens offset by the item's first token and the item's guide row as the query.
 *   key, value : bf16 [sum N_i, E] (frames_embed and frames_feature; the same pointer twice without frames_embed), guide bf16 [B, E]
 *   dctx       : f32 [sum w_i, E], the cotangent of the window contexts
 *   dq         : f32 [sum w_i, E] per window;  dq_item f32 [B, E] or NULL: the rows of an item's windows summed in a fixed order (a
 *                second launch, no atomics): the local share of d guide
 *   dkey, dvalue : bf16 [sum N_i, E] or NULL, plain stores (every token lies in one window: nothing is cleared); value_is_key: key ==
 *                value, dkey NULL, and the key-side gradient of a row is added into dvalue
 * hicom_compressor_ragged_global_dx: hicom_global_dx_fwd with an item per workgroup,
 *   dx[n] (+)= sum_r ds[i nh + r, n] qt[i nh + r] + softmax(scores)[i nh + r, n] dctx[i nh + r]   for the tokens n of item i.
 *   scores, ds, ml : as hicom_compressor_ragged_global_bwd read and left them;  qt, dctx f32 [B nh, E]
 *   tiles      : DEVICE array of ntiles pairs {item, first token of the tile inside the item}, tiles of 64 tokens counted from each item's
 *                first token, ntiles = sum ceil(N_i / 64); a pair that names no item or no token of it is skipped
 *   dx         : bf16 [sum N_i, E]; accumulate: read, added to and rewritten (the rows the window backward left) */
int hicom_compressor_ragged_local_bwd(const hicom_compressor_ragged_args* args, const void* key, const void* value, const void* guide, const float* dctx,
                                      float* dq, float* dq_item, void* dkey, void* dvalue, int32_t value_is_key);
int hicom_compressor_ragged_global_dx(const hicom_compressor_ragged_args* args, const float* scores, const float* ds, const float* ml, const float* qt,
                                      const float* dctx, const int32_t* tiles, int32_t ntiles, void* dx, int32_t accumulate);

/* ---- the batched and the ragged step for the k / v adaptor recipe (`local43_adaptkv_global32`) ----------------------
 * The adaptors sit on the local stage only (projector.py:431-457, :533-534: key = (1 - a_k) x + a_k LN(MLP_k(x)) over ALL tokens of
 * the key stream, likewise the values over ff); the global stage reads the raw tokens, so launches 1-2 and 4-12 are those of the
 * plain steps above.  In front of the local stage the two adaptor MLPs run over M = all tokens of the call as dense MFMA GEMMs
 * (layer 1: raw bf16 tokens x bf16 weights -> fp16 hidden with GELU; layer 2: fp16 hidden x the fp16 weight copy -> fp16 y): with
 * both adaptors each layer is ONE paired launch (hicom_dense16_gemm_pair_fwd), with one adaptor two single launches -- fourteen
 * launches either way, whatever B and the mix are.  The local stage then blends LayerNorm(y) into the rows it loads (one wave per
 * window, the blended streams are never written) and leaves the same saturating fp16 context plane as the plain step.
 *   ak, av   : the adaptor of the key / of the value stream; w0 == NULL: that stream is not adapted (at least one of the two is).
 *              The k adaptor reads fe (ff when fe is NULL), the v adaptor ff.  Widths are E (E % 64 == 0)
 *   alpha_dt : dtype of the two alpha scalars (HICOM_DT_BF16 | HICOM_DT_F32); eps: the LayerNorms' epsilon
 *   ws       : the *_adapt_workspace_bytes of these arguments.  The plain layout (the table region of the ragged step included) keeps
 *              its offsets; BEHIND it come one fp16 [tokens, E] hidden plane and one fp16 [tokens, E] y plane per adapted stream --
 *              token-sized, unlike everything in front of them (2 x 2304 bytes per token and adapted stream)
 * Limits, error codes and the no-synchronisation contract of the *_fwd calls are those of the plain entry points; in addition
 * tokens x E < 2^32 (the dense GEMM's operand limit), HICOM_EUNSUP otherwise.  hicom_compressor_ragged_adapt_prepare writes the same
 * table region as hicom_compressor_ragged_prepare. */
typedef struct hicom_seg_adaptor {
    const void *w0, *b0;       /* Linear(E, E): bf16 [E, E], bf16 [E] (or NULL) */
    const void *w2_f16, *b2;   /* Linear(E, E): fp16 copy of the weight (cached by the caller per weight state), bf16 bias (or NULL) */
    const void *gamma, *beta;  /* LayerNorm: bf16 [E] */
    const void* alpha;         /* device scalar of dtype alpha_dt */
} hicom_seg_adaptor;
typedef struct hicom_compressor_batch_adapt_args {
    hicom_compressor_batch_args base;
    hicom_seg_adaptor ak, av;
    int32_t alpha_dt;
    float eps;
} hicom_compressor_batch_adapt_args;
int64_t hicom_compressor_batch_adapt_workspace_bytes(const hicom_compressor_batch_adapt_args* args);
int hicom_compressor_batch_adapt_fwd(const hicom_compressor_batch_adapt_args* args);
typedef struct hicom_compressor_ragged_adapt_args {
    hicom_compressor_ragged_args base;
    hicom_seg_adaptor ak, av;
    int32_t alpha_dt;
    float eps;
} hicom_compressor_ragged_adapt_args;
int64_t hicom_compressor_ragged_adapt_workspace_bytes(const hicom_compressor_ragged_adapt_args* args);
int hicom_compressor_ragged_adapt_prepare(const hicom_compressor_ragged_adapt_args* args);
int hicom_compressor_ragged_adapt_fwd(const hicom_compressor_ragged_adapt_args* args);

/* ---- training step of the ragged call for the k / v adaptor recipe (forward_ragged_train(adaptors=True)) ----
 * hicom_compressor_ragged_adapt_train_state, after hicom_compressor_ragged_adapt_fwd on the same block: copies the fp16 y planes
 * (the adaptor MLPs' outputs over all sum N_i tokens, 2 E sum N_i bytes each) out of the adaptor regions of args->base.ws; ky_out / vy_out
 * may be NULL (not copied), one of them is not, and neither names a stream without adaptor.  The rest of the state is
 * hicom_compressor_ragged_train_state(&args->base, ...): the plain layout does not move with the adaptors.
 * The three calls below take the PLAIN block (&args->base of an adaptor plan): they read only the table region of args->ws and args'
 * shape, l_scale and stream, and check their pointers, the alignment, the per-item partition and tokens x E < 2^32 in front of
 * everything that needs a device.  Only launches: no allocation, no host copy, no synchronisation.
 * hicom_compressor_ragged_local_adapt_bwd: hicom_local_attn_adapt_bwd over the concatenated window list, one 4-wave workgroup per window
 * with the window's geometry from its item's own (T, kt), the x and y rows offset by the item's first token, the item's guide row (bf16
 * [B, E]) as the query and bias 0.  key_x / value_x bf16, key_y / value_y fp16 [sum N_i, E] (NULL: that stream has no adaptor; not both),
 * dctx f32 [sum w_i, E].  Outputs, plain stores:
 *   ds, pw               f32 [sum N_i]
 *   sxk, syk, sxv, syv   f32 [sum w_i, E] each or NULL (not written); syk / syv must be NULL for a stream without adaptor
 * Per item the outputs are those of hicom_local_attn_adapt_bwd on that item alone, bit for bit.
 * hicom_compressor_ragged_adapt_dy: hicom_adapt_dy_fwd over the stacked tokens, one wave per token.  The token's item is found by a
 * search of the plan's item table, its window from the item's own axes; vec (bf16 | f32, rows of E) has one row per item (vec_per_item != 0:
 * the K stream's guide rows) or one per window of the concatenated list (the V stream's dctx).  y fp16, coef f32 [sum N_i], dy / r1 bf16
 * [sum N_i, E] (r1 may be NULL), col_parts f32 [nparts, E] or NULL as hicom_adapt_dy_fwd.
 * hicom_compressor_ragged_dq_item: dq_item f32 [B, E] = the rows of dq f32 [sum w_i, E] summed per item in a fixed order, no atomics
 * (the second launch of hicom_compressor_ragged_local_bwd on a dq of the caller's). */
int hicom_compressor_ragged_adapt_train_state(const hicom_compressor_ragged_adapt_args* args, void* ky_out, void* vy_out);
int hicom_compressor_ragged_local_adapt_bwd(const hicom_compressor_ragged_args* args, const void* key_x, const void* key_y, const void* k_gamma,
                                            const void* k_beta, const void* k_alpha, const void* value_x, const void* value_y, const void* v_gamma,
                                            const void* v_beta, const void* v_alpha, int32_t alpha_dt, float eps, const void* guide, const float* dctx,
                                            float* ds, float* pw, float* sxk, float* syk, float* sxv, float* syv);
int hicom_compressor_ragged_adapt_dy(const hicom_compressor_ragged_args* args, const void* y, const void* gamma, const void* vec, int32_t vec_dt,
                                     int32_t vec_per_item, const float* coef, const void* alpha, int32_t alpha_dt, float eps, void* dy, void* r1,
                                     float* col_parts, int32_t nparts);
int hicom_compressor_ragged_dq_item(const hicom_compressor_ragged_args* args, const float* dq, float* dq_item);

/* ---- multi-guide compressor step: ONE clip, Q instructions, the tokens read once ------------------------------------
 * What hicom/eval/video/inference_video_mcqa_videomme.py:268-303 does with one projector call per question on the same video tensor.
 * The guide enters both stages only as a query, so Q guides cost one pass over the tokens plus Q times the window-sized work.  The
 * plain release recipe only (no adaptors), bf16; a launch sequence on `stream` whose length does not depend on Q.  Guide q of the
 * output equals hicom_compressor_fwd with guide row q alone to the kernels' rounding.
 *   ff, fe   : bf16 [T, H, W, E] (fe NULL: the local keys are ff); guide bf16 [Q, E], 1 <= Q <= 32
 *   kt, ks   : local window; T % kt == H % ks == W % ks == 0, kt ks ks <= 64; E == 1152, nh <= 16 heads, hidden % 64 == 0;
 *              HICOM_EUNSUP otherwise
 *   pe, kpe  : the tables of hicom_compressor_args, both NULL = no pos-emb
 *   chunks   : token chunks (workgroups per 32-row pass) of the global stream, 0 = hicom_global_stream_nparts; clamped to the
 *              16-token tiles of the clip and to 256
 *   out      : [Q, item_rows, ldo] of out_dt (bf16 | f32); the packed-row layout integers are those of hicom_compressor_batch_args
 *              and hold for every guide: local tokens with a newline gap after every nl_group of them, then n_global_rows identical
 *              copies of the guide's global token
 *   ws       : hicom_compressor_multiguide_workspace_bytes(args) bytes (depends on the shape, Q and chunks), 256-byte aligned, nothing
 *              to zero; not shared between concurrently running calls
 * hicom_compressor_multiguide_fwd only launches: no copy, no synchronisation, no allocation. */
typedef struct hicom_compressor_multiguide_args {
    const void* ff;
    const void* fe;
    const void* guide;
    int32_t Q, T, H, W, E, hidden, kt, ks, nh, P;
    float l_scale;
    int32_t chunks;
    const void *lw0_f16, *lb0, *lw2_f16, *lb2;      /* local readout: fp16 copies of the weights, bf16 biases */
    const void *wq, *bq, *wk, *wv, *bv, *wo, *bo;   /* global attention, bf16 */
    const void *gw0, *gb0, *gw2, *gb2;              /* global readout, bf16 */
    const float* pe;
    const float* kpe;
    int32_t t_index0, y_index0, x_index0, out_dt;
    void* out;
    int64_t ldo, item_rows, global_row0;
    int32_t n_global_rows, nl_group, nl_count, reserved_;
    int64_t nl_first, nl_step;
    const void* newline;
    void* ws;
    int64_t ws_bytes;
    void* stream;
} hicom_compressor_multiguide_args;
int64_t hicom_compressor_multiguide_workspace_bytes(const hicom_compressor_multiguide_args* args);
int hicom_compressor_multiguide_fwd(const hicom_compressor_multiguide_args* args);

/* ---- prepared clips: the k / v adaptor recipe with the adaptor MLPs run ONCE per clip, Q guides per call ----------
 * key = (1 - a_k) x + a_k LN(MLP_k(x)) depends on the tokens only; the guide enters as the query.  hicom_clip_adapt_prepare_fwd runs
 * both layers of each adaptor MLP over the clip's N tokens -- the launches of the adaptor steps above: one hicom_dense16_gemm_pair_fwd per
 * layer with both adaptors, hicom_dense16_gemm_fwd per layer with one -- and leaves y = MLP(x) as fp16 [N, E] planes the CALLER owns.
 *   key_x, ff : bf16 [N, E]: what the k adaptor resp. the v adaptor reads (key_x = fe, or ff without frames_embed)
 *   ak, av    : w0 == NULL: that stream is not adapted (at least one is); gamma / beta / alpha are not read here
 *   ky, vy    : fp16 [N, E] out, 16-byte aligned (not read for a stream without adaptor)
 *   ws        : hicom_clip_adapt_prepare_workspace_bytes(N, E, ak, av) bytes, 256-byte aligned: the fp16 hidden plane of layer 1 per
 *               adapted stream, a temporary
 * E % 64 == 0 and N E < 2^32 (the dense GEMM's operand limit), HICOM_EUNSUP otherwise.  Only launches.
 *
 * hicom_compressor_multiguide_adapt_fwd is hicom_compressor_multiguide_fwd with the local stage reading those planes: the same launch
 * sequence (no adaptor MLP runs), the same workspace (hicom_compressor_multiguide_adapt_workspace_bytes equals the plain function on
 * `base`), the planes are read only.
 *   base      : the plain block; ff / fe are the tokens the planes were made from
 *   ak, av    : gamma / beta / alpha of the adapted streams are read (w0 .. b2 are not)
 *   ky, vy    : the prepared planes; NULL: that stream is not adapted and is read as in the plain step.  Not both NULL (HICOM_EINVAL)
 *   alpha_dt  : dtype of the two alpha scalars (HICOM_DT_BF16 | HICOM_DT_F32); eps: the LayerNorms' epsilon
 * Guide q of the output equals hicom_compressor_batch_adapt_fwd on the clip with guide row q alone: bit for bit on the local rows. */
int64_t hicom_clip_adapt_prepare_workspace_bytes(int64_t N, int32_t E, const hicom_seg_adaptor* ak, const hicom_seg_adaptor* av);
int hicom_clip_adapt_prepare_fwd(const void* key_x, const void* ff, int64_t N, int32_t E, const hicom_seg_adaptor* ak, const hicom_seg_adaptor* av,
                                 void* ky, void* vy, void* ws, int64_t ws_bytes, void* stream);
typedef struct hicom_compressor_multiguide_adapt_args {
    hicom_compressor_multiguide_args base;
    hicom_seg_adaptor ak, av;
    const void* ky;
    const void* vy;
    int32_t alpha_dt;
    float eps;
} hicom_compressor_multiguide_adapt_args;
int64_t hicom_compressor_multiguide_adapt_workspace_bytes(const hicom_compressor_multiguide_adapt_args* args);
int hicom_compressor_multiguide_adapt_fwd(const hicom_compressor_multiguide_adapt_args* args);

/* ---- ragged multi-guide compressor step: B items of unequal length, item i with its own Q_i instructions -----------
 * The product of the ragged and the multi-guide step: a Video-MME evaluation batch (several videos x 3 questions), or a batch of
 * multi-question items through hicom/model/hicom_arch.py:146-180.  A PAIR is one (item, guide); pairs are numbered item-major, then
 * guide-major, M = sum Q_i of them.  Pair (i, q) of the output equals hicom_compressor_fwd on item i alone with its guide q to the
 * kernels' rounding.  The plain release recipe only (no adaptors), bf16.  Every item's tokens are read once by the local stage and once
 * per pass of 32 folded rows by the global stream (nh = 9: one pass for Q_i <= 3, two for Q_i <= 7, nine at Q_i = 32); the launch
 * sequence is the twelve launches of the ragged step whatever B, the Q_i and the mix are.
 *   ff, fe   : bf16 [sum T_i, H, W, E] (fe NULL: the local keys are ff), as in hicom_compressor_ragged_args
 *   guide    : bf16 [M, E]; the guides of item i are the rows [sum_{j<i} Q_j, + Q_i)
 *   items    : HOST array of B descriptors, as in hicom_compressor_ragged_args; the packed-row layout of an item holds for each of
 *              its pairs
 *   guide_counts, n_guide_counts : HOST array of the Q_i and its length, which must be B; 1 <= Q_i <= 32
 *   chunks   : token chunks per item and pass of the global stream, each clamped to the item's 16-token tiles and to 64; 0 = the
 *              item's share of 2 x #CUs work units by tiles x passes.  A work unit {item, first tile, last tile, row pass, partial-state
 *              slot} streams tokens of ONE item, tiles counted from the item's first token, for 32 densely packed folded rows (guide q
 *              of an item owns rows nh q .. nh q + nh - 1 of the item's row space)
 *   out      : [sum Q_i rows_i, ldo] of out_dt (bf16 | f32): the pairs' packed rows follow each other
 *   ws       : hicom_compressor_ragged_multiguide_workspace_bytes(args) bytes, 256-byte aligned.  Its head is a table region (item
 *              table, work units, window -> item lookup, pair table, row -> pair lookup) that
 *              hicom_compressor_ragged_multiguide_prepare(args) derives on the host and writes ONCE per (items, guide counts, shape,
 *              chunks, ws): it copies to the device and synchronises `stream`, so it runs outside the hot loop and outside a capture.
 * Limits (HICOM_EUNSUP beyond them; the device tables hold int32 offsets): B <= 4096 items, M <= 4096 pairs (grid y of the merge);
 * per item T H W < 2^27 tokens; over the call sum N_i + 16 B < 2^27 tokens, sum Q_i ceil16(N_i) < 2^27 token x guide products (the
 * logits are 32 rows per pass and token, their offsets counted in 16 floats) and sum Q_i windows_i < 2^20 context rows; the grid,
 * window and merge-LDS limits of hicom_compressor_ragged_args.
 * hicom_compressor_ragged_multiguide_fwd then only launches: no copy, no synchronisation, no allocation, O(B) integer work on the host.
 * It trusts the table region as hicom_compressor_ragged_fwd does. */
typedef struct hicom_compressor_ragged_multiguide_args {
    const void* ff;
    const void* fe;
    const void* guide;
    int32_t B, H, W, E, hidden, ks, nh, P;
    float l_scale;
    int32_t chunks;
    const hicom_ragged_item* items;                 /* HOST memory, B entries */
    const int32_t* guide_counts;                    /* HOST memory, n_guide_counts entries */
    int32_t n_guide_counts, reserved_;
    const void *lw0_f16, *lb0, *lw2_f16, *lb2;      /* local readout: fp16 copies of the weights, bf16 biases */
    const void *wq, *bq, *wk, *wv, *bv, *wo, *bo;   /* global attention, bf16 */
    const void *gw0, *gb0, *gw2, *gb2;              /* global readout, bf16 */
    const float* pe;
    const float* kpe;
    int32_t t_index0, y_index0, x_index0, out_dt;
    void* out;
    int64_t ldo;
    const void* newline;
    void* ws;
    int64_t ws_bytes;
    void* stream;
} hicom_compressor_ragged_multiguide_args;
int64_t hicom_compressor_ragged_multiguide_workspace_bytes(const hicom_compressor_ragged_multiguide_args* args);
int hicom_compressor_ragged_multiguide_prepare(const hicom_compressor_ragged_multiguide_args* args);
int hicom_compressor_ragged_multiguide_fwd(const hicom_compressor_ragged_multiguide_args* args);

/* ---- prepared clips, Q_i instructions each: the ragged multi-guide step over clips at their own addresses ---------
 * B prepared clips (hicom_clip_adapt_prepare_fwd; or plain token tensors for the plain recipe) that were made at different times live
 * at different addresses, each with its own y planes.  This is hicom_compressor_ragged_multiguide_fwd with launch 3 (local windows) and
 * launch 4 (segmented stream) taking an item's base pointers from a device table instead of ff + tok0 E: the same twelve launches, no
 * adaptor MLP, nothing token-sized in the workspace.  One entry point serves both release recipes.
 *   base      : the ragged multi-guide block.  ff and fe are not used and must be NULL (HICOM_EINVAL); items, guide_counts, guide,
 *               chunks, out, ws as there
 *   ak, av    : w0 == NULL: that stream is not adapted; both NULL: the plain recipe (the plain window runs).  Of an adapted stream
 *               gamma / beta / alpha are read (w0 .. b2 are not), as in hicom_compressor_multiguide_adapt_args
 *   alpha_dt  : dtype of the two alpha scalars (HICOM_DT_BF16 | HICOM_DT_F32); eps: the LayerNorms' epsilon
 *   item_ptrs : DEVICE table [B][4] of 64-bit addresses {key_x, value_x, ky, vy} per item, 16-byte aligned.  key_x: the clip's
 *               frames_embed, or its frames_feature when there is none; value_x: its frames_feature (bf16 [T_i H W, E] each, 16-byte
 *               aligned); ky / vy: its fp16 [T_i H W, E] planes, 0 for a stream without adaptor.  The kernels only read through them.
 *               The table is the CALLER's to fill, per call, on `stream` in front of the call: stream order protects it against the
 *               previous call's kernels.  The host cannot look at device-resident addresses: the caller checks them.
 * hicom_compressor_clips_multiguide_workspace_bytes equals hicom_compressor_ragged_multiguide_workspace_bytes on `base` (the tokens and
 * the planes are the caller's); hicom_compressor_clips_multiguide_prepare writes the same table region, once per plan (tok0 stays in the
 * item table and is not used for addressing); hicom_compressor_clips_multiguide_fwd then only launches: no copy, no synchronisation, no
 * allocation.  Limits and error codes are those of the base step; its checks report under its name. */
typedef struct hicom_compressor_clips_multiguide_args {
    hicom_compressor_ragged_multiguide_args base;
    hicom_seg_adaptor ak, av;
    int32_t alpha_dt;
    float eps;
    const uint64_t* item_ptrs;                      /* DEVICE memory, B x 4 entries */
} hicom_compressor_clips_multiguide_args;
int64_t hicom_compressor_clips_multiguide_workspace_bytes(const hicom_compressor_clips_multiguide_args* args);
int hicom_compressor_clips_multiguide_prepare(const hicom_compressor_clips_multiguide_args* args);
int hicom_compressor_clips_multiguide_fwd(const hicom_compressor_clips_multiguide_args* args);

/* ---- clip stream: a video that arrives in chunks of whole window groups, one carried softmax state ----------------
 * The carried state of the global stage is the un-normalised online-softmax triple of everything pushed so far, in the layout
 * hicom_global_combine_fwd reads as ONE set:  state_ml f32 [rows][2] = (M, L),  state_acc f32 [rows][E].  Empty: M = -inf, L = 0, ACC = 0
 * (hicom_stream_state_clear_fwd writes that into ml_rows (M, L) pairs and acc_floats floats: a launch on `stream`).
 *
 * hicom_stream_state_fold_fwd folds the `nparts` partials of one chunk, as hicom_fused_stream_fwd writes them with pe_hi / pe_lo given
 * (part_m, part_l f32 [nparts][rows_pad], part_acc f32 [nparts][rows_pad][E]: the value-side positional term is inside part_acc), into it:
 *     M' = max(M, max_p m_p)     L' = e^(M - M') L + sum_p e^(m_p - M') l_p     ACC' = e^(M - M') ACC + sum_p e^(m_p - M') acc_p
 * A term whose max is -inf has weight 0 (no -inf - -inf): from the empty state the result is the merge of the partials alone.  Rows >= rows
 * of the padded partials are not read.  ACC is updated in place (every element is read and written by one lane).  (M, L) is read by every
 * workgroup of a row, so it is NOT updated in place: state_ml_in and state_ml_out are two different [rows][2] blocks and the caller swaps
 * them from push to push.  E % 4 == 0; part_acc and state_acc 16-byte aligned, state_ml_* 8-byte aligned. */
int hicom_stream_state_clear_fwd(float* state_ml, int32_t ml_rows, float* state_acc, int64_t acc_floats, void* stream);
int hicom_stream_state_fold_fwd(const float* part_m, const float* part_l, const float* part_acc, int32_t nparts, int32_t rows,
                                int32_t rows_pad, int32_t E, const float* state_ml_in, float* state_ml_out, float* state_acc, void* stream);

/* One push of a clip stream in ONE host call: hicom_fused_stream_fwd on the chunk (t_index0 = t0, f32 partials, the fp16 context plane),
 * hicom_stream_state_fold_fwd, the two hicom_readout16_gemm_fwd launches of the local readout writing the chunk's rows at row0 (packed with
 * nl_group), and -- nl_count > 0 -- the chunk's newline rows (hicom_scatter_rows_fwd).  Nothing is allocated, copied or synchronised.
 * The block is built once per chunk shape; ff, fe, t0, row0, nl_first, state_ml_in / state_ml_out, out and stream change from push to push.
 *   ff, fe      : bf16 [Tc, H, W, E] (fe NULL: the keys are frames_feature); Tc % kt == H % ks == W % ks == 0, 16 <= kt ks ks <= 64, E == 1152
 *   t0          : absolute number of the chunk's first frame: the frame rows of pos_a / pe_hi / pe_lo are read at t0 + t, so the state of
 *                 disjoint frame ranges merges exactly; t0 + Tc <= y_index0 (the tables' frame capacity), x_index0 + W <= P
 *   q_hi .. pe_lo, rows, l_scale : hicom_fused_stream_fwd's operands of the same names (guide-only: made once per stream)
 *   part_*      : the chunk's partials, nparts = hicom_fused_stream_nparts(windows of the chunk); ctx_f16 fp16 [windows, E]; hid_f16 fp16
 *                 [windows, hidden]
 *   lw0_f16 .. lb2 : the local readout (fp16 weight copies, bf16 biases); hidden % 64 == 0
 *   out         : the stream's output buffer (out_dt HICOM_DT_F32 | HICOM_DT_BF16, row length ldo >= hidden)
 *   newline     : bf16 [hidden], rows nl_first + i nl_step, i < nl_count (absolute rows of `out`), or nl_count = 0 */
typedef struct hicom_stream_push_args {
    const void* ff;
    const void* fe;
    int32_t Tc, H, W, E, kt, ks;
    int32_t t0, rows;
    const void* q_hi;
    const void* q_lo;
    const float* pos_a;
    const void* pe_hi;
    const void* pe_lo;
    int32_t P, y_index0, x_index0;
    float l_scale;
    float* part_m;
    float* part_l;
    float* part_acc;
    void* ctx_f16;
    void* hid_f16;
    int32_t nparts, hidden;
    const float* state_ml_in;
    float* state_ml_out;
    float* state_acc;
    const void* lw0_f16;
    const void* lb0;
    const void* lw2_f16;
    const void* lb2;
    void* out;
    int32_t out_dt, nl_group;
    int64_t ldo, row0;
    const void* newline;
    int64_t nl_first, nl_step;
    int32_t nl_count, reserved_;
    void* stream;
} hicom_stream_push_args;
int hicom_compressor_stream_push(const hicom_stream_push_args* args);

/* ---- clip stream for several instructions: one chunked video, Q guides ---------------------------------------------
 * The carried state is ONE un-normalised set of R = nh Q rows (guide q's heads are rows nh q .. nh q + nh - 1, as the multi-guide step
 * packs them), state_ml f32 [R][2], state_acc f32 [R][E]: what hicom_global_combine_fwd reads as one set.
 *
 * hicom_stream_state_fold_set_fwd folds ONE un-normalised set as hicom_global_merge_fwd / hicom_global_merge_marg_fwd write it with
 * normalize = 0 (set_ml f32 [rows][2] = interleaved (M, L), set_acc f32 [rows][E]) into the carried state, with the arithmetic of
 * hicom_stream_state_fold_fwd (one kernel body): an empty term weighs 0 by test, expf, ACC in place, (M, L) from state_ml_in to
 * state_ml_out (two blocks that must not overlap).  From the empty state the result is the set.  Any row count (288 = 9 heads x 32 guides).
 * E % 4 == 0; set_acc and state_acc 16-byte aligned, set_ml and state_ml_* 8-byte aligned. */
int hicom_stream_state_fold_set_fwd(const float* set_ml, const float* set_acc, int32_t rows, int32_t E, const float* state_ml_in,
                                    float* state_ml_out, float* state_acc, void* stream);

/* The local stage of the multi-guide step alone (multi_guide.hip's kernel: one wave per window, every row of the window loaded once per
 * group of guides): key / value bf16 [T, H, W, E] (E == 1152), guide bf16 [Q, E], fp16 contexts ctx_f16 [Q][windows][E], window order
 * (t1, h1, w1).  Exact window partition, kt ks ks <= 64 tokens, 1 <= Q <= 32.  Windows do not depend on a frame offset. */
int hicom_multi_guide_local_fwd(const void* key, const void* value, const void* guide, int32_t Q, int32_t T, int32_t H, int32_t W, int32_t E,
                                int32_t kt, int32_t ks, float scale, void* ctx_f16, void* stream);

/* Placement of `rows` packed rows per guide into a [Q][.][ldo] output whose guides lie q_stride ELEMENTS apart (byte work; the row body is
 * that of every many-item step): out[q][row0 + r], r < rows, is
 *   r >= global_row0                      : tok[q] (f32 [Q][hidden], rounded once) -- the global rows of finish();
 *   r = nl_first + i nl_step, i < nl_count: newline (bf16 [hidden]); nl_first is relative to row0;
 *   otherwise                             : row q windows + m of loc ([Q][windows][hidden], the output dtype), m = r - r / (nl_group + 1)
 *                                           (nl_group = 0: m = r).
 * A push places a chunk (global_row0 = rows = windows + nl_count, tok NULL); finish() the rows behind the local rows (loc NULL, windows = 0,
 * global_row0 = nl_count = the whole-clip newline rows, 0 or 1).  Grid Q x rows. */
int hicom_stream_place_rows_fwd(const void* loc, const float* tok, const void* newline, int32_t Q, int32_t windows, int32_t hidden,
                                int32_t nl_group, int32_t nl_count, int64_t nl_first, int64_t nl_step, int64_t rows, int64_t global_row0,
                                void* out, int32_t out_dt, int64_t ldo, int64_t q_stride, int64_t row0, void* stream);

/* One push of a multi-guide clip stream in ONE host call, eight launches (nine in the logit-tensor form): hicom_multi_guide_local_fwd on the
 * chunk; the many-row global stream over the chunk's tokens with t_index0 = t0 (hicom_global_stream_marg_fwd when marg != 0, else
 * hicom_global_stream_fwd) and its merge (hicom_global_merge_marg_fwd / hicom_global_merge_fwd) with normalize = 0 and t_index0 = t0 into
 * (set_ml, set_acc); hicom_stream_state_fold_set_fwd; the two hicom_readout16_gemm_fwd launches over M = Q x windows rows into `loc`;
 * hicom_stream_place_rows_fwd.  Every shape, pointer, alignment and table bound is checked in front of the first launch.  Nothing is
 * allocated, copied or synchronised.  The block is built once per (Q, chunk shape); ff, fe, guide, t0, row0, nl_first, the stream's
 * operands (q_hi .. pe, P, y_index0, x_index0, state_*, out, q_stride, newline) and stream change from push to push.
 *   ff, fe     : bf16 [Tc, H, W, E] (fe NULL: the keys are frames_feature); Tc % kt == H % ks == W % ks == 0, kt ks ks <= 64, E == 1152
 *   guide      : bf16 [Q, E], 1 <= Q <= 32: the local queries;  nh heads: rows = nh Q folded rows, rows_pad = rows rounded up to 32
 *   q_hi, q_lo : bf16 [rows_pad, E] (hicom_fold_query_split_fwd over the Q guides; rows >= rows zero); pos_a f32 [rows_pad, P] or NULL
 *   pe         : f32 [P, E], the table the merge reads, NULL iff pos_a is NULL; frames at t0 + t: t0 + Tc <= y_index0, y_index0 + H <=
 *                x_index0, x_index0 + W <= P
 *   marg       : the form, chosen once per plan: 1 needs pe and hicom_global_stream_has_marg(Tc H W, E, rows_pad, H, W, nparts) == 1
 *   part_*     : the chunk's partials [nparts][rows_pad] / [nparts][rows_pad][E], 1 <= nparts <= min(tiles of 16 tokens, 256)
 *   scores     : marg: f32 [nparts][rows_pad][hicom_global_stream_marg_width(H, W)]; else the logits f32 [rows_pad][score_stride],
 *                score_stride >= Tc H W rounded up to 16 and % 4 == 0.  16-byte aligned
 *   scratch    : f32 [rows_pad Tc (H + W + 2)] (pe given); set_ml f32 [rows][2], set_acc f32 [rows][E]
 *   ctx_f16    : fp16 [Q windows, E]; hid_f16 fp16 [Q windows, hidden]; loc [Q windows, hidden] of the output dtype; hidden % 64 == 0
 *   out        : guide q's rows start q_stride elements apart, row length ldo >= hidden; the chunk's rows go to rows row0 .. of each guide;
 *                nl_first: ABSOLUTE row of the chunk's first newline row (>= row0), as in hicom_stream_push_args */
typedef struct hicom_stream_push_multi_args {
    const void* ff;
    const void* fe;
    const void* guide;
    int32_t Q, Tc, H, W, E, kt, ks, nh;
    int32_t t0, marg;
    const void* q_hi;
    const void* q_lo;
    const float* pos_a;
    const float* pe;
    int32_t P, y_index0, x_index0;
    float l_scale;
    float* part_m;
    float* part_l;
    float* part_acc;
    float* scores;
    float* scratch;
    float* set_ml;
    float* set_acc;
    void* ctx_f16;
    void* hid_f16;
    void* loc;
    int32_t nparts, hidden;
    int64_t score_stride;
    const float* state_ml_in;
    float* state_ml_out;
    float* state_acc;
    const void* lw0_f16;
    const void* lb0;
    const void* lw2_f16;
    const void* lb2;
    void* out;
    int32_t out_dt, nl_group;
    int64_t ldo, q_stride, row0;
    const void* newline;
    int64_t nl_first, nl_step;
    int32_t nl_count, reserved_;
    void* stream;
} hicom_stream_push_multi_args;
int hicom_compressor_stream_push_multi(const hicom_stream_push_multi_args* args);

/* ---- clip stream for several instructions on the k / v adaptor recipe ----------------------------------------------
 * The adaptors sit on the local stage only, so the carried state, its fold, finish() and the placement are those above; a push differs
 * in its local stage alone: the adaptor MLPs run over the chunk's tokens once for all Q guides, into planes that live for one push.
 *
 * hicom_multi_guide_local_adapt_fwd is the local stage of hicom_compressor_multiguide_adapt_fwd alone (its kernel, its launch): key / value
 * bf16 [T, H, W, E], the fp16 planes ky / vy [T H W, E] of hicom_clip_adapt_prepare_fwd (NULL: that stream is not adapted; not both NULL,
 * HICOM_EINVAL; 16-byte aligned), gamma / beta / alpha of the two adaptors (of an adapted stream; w0 .. b2 are not read), alpha_dt and
 * eps as in hicom_compressor_multiguide_adapt_args; fp16 contexts ctx_f16 [Q][windows][E].  Shapes, limits and checks of
 * hicom_multi_guide_local_fwd.  Windows do not depend on a frame offset. */
int hicom_multi_guide_local_adapt_fwd(const void* key, const void* value, const void* guide, const void* ky, const void* vy,
                                      const hicom_seg_adaptor* ak, const hicom_seg_adaptor* av, int32_t alpha_dt, float eps, int32_t Q, int32_t T,
                                      int32_t H, int32_t W, int32_t E, int32_t kt, int32_t ks, float scale, void* ctx_f16, void* stream);

/* One push of a multi-guide clip stream on the adaptor recipe in ONE host call, ten launches (eleven in the logit-tensor form) whatever Q
 * is: hicom_clip_adapt_prepare_fwd on the chunk's N = Tc H W tokens (layer 1 and layer 2 of the adaptor MLPs, a GEMM pair each with both
 * adaptors) into ky / vy; hicom_multi_guide_local_adapt_fwd on the chunk; then launches 2 ... of hicom_compressor_stream_push_multi
 * unchanged.  Every check of that entry point and of the two parts runs in front of the first launch.  Nothing is allocated, copied or
 * synchronised.
 *   base         : the plain block, every field as there.  The k adaptor reads fe (ff when fe is NULL), the v adaptor ff
 *   ak, av       : w0 == NULL: that stream is not adapted (at least one is); every field of an adapted stream is read
 *   ky, vy       : fp16 [N, E] planes of ONE chunk, 16-byte aligned, written and read by this call; NULL exactly for a stream without
 *                  adaptor (HICOM_EINVAL otherwise)
 *   adapt_ws     : hicom_clip_adapt_prepare_workspace_bytes(N, E, ak, av) bytes, 256-byte aligned (the hidden planes of layer 1)
 *   alpha_dt, eps: as in hicom_compressor_multiguide_adapt_args
 * E % 64 == 0 and N E < 2^32 per chunk (the dense GEMM's operand limit), HICOM_EUNSUP otherwise. */
typedef struct hicom_stream_push_multi_adapt_args {
    hicom_stream_push_multi_args base;
    hicom_seg_adaptor ak, av;
    void* ky;
    void* vy;
    void* adapt_ws;
    int64_t adapt_ws_bytes;
    int32_t alpha_dt;
    float eps;
} hicom_stream_push_multi_adapt_args;
int hicom_compressor_stream_push_multi_adapt(const hicom_stream_push_multi_adapt_args* args);

/* ---- clip stream group: B live videos, one guide and one carried state each, pushed in one call -------------------
 * The group's state is state_ml f32 [B][nh][2] = (M, L) and state_acc f32 [B][nh][E]: slot s's slice is ONE set as
 * hicom_global_combine_fwd reads it (empty: hicom_stream_state_clear_fwd).  The query operands are slot-major: q_hi / q_lo bf16
 * [B nh][E], pos_a f32 [B nh][P] (hicom_linear_fwd + hicom_fold_query_split_fwd over the B guides), guide bf16 [B][E].
 *
 * One push takes `items` chunks (1 <= items <= B <= 32) of the stacked tensor ff / fe bf16 [sum tc_i, H, W, E] (fe NULL: the keys are
 * ff), item i with tc[i] frames (a positive multiple of kt) for slot slot[i], at the absolute frame offset t0[i], its chunk rows --
 * windows, with a newline row behind every nl_group of them when nl_group > 0 -- going to rows row0[i] .. of that slot's part of `out`
 * (slot s starts slot_stride ELEMENTS behind slot 0 and has slot_rows rows of ldo elements).  Six launches whatever items and the mix of
 * tc are: the local stage over all windows (the guide row of the item's slot), the segmented global stream (frame rows of pos_a at
 * t0[i] + t, query rows slot[i] nh ..), the merge of the item's partials into its chunk's UN-normalised set folded into the slot's
 * state IN PLACE (one workgroup per (item, head) row -- so a slot appears at most once per push), the two hicom_readout16_gemm_fwd
 * launches over all windows and the placement.
 *
 * hicom_compressor_stream_group_workspace_bytes: the plan's workspace for the tuple (tc[0 .. items)), from B, items, tc, the geometry,
 * hidden, out_dt, nl_group and chunks alone (a negative status on a refusal).  hicom_compressor_stream_group_prepare writes the static
 * tables of that tuple (first token, token count, first window, work units, window -> item, row -> item) to the head of ws: one copy,
 * synchronises `stream`; once per plan.  hicom_compressor_stream_group_push checks every shape, pointer, alignment, table bound and slot
 * in front of the first launch -- t0[i] + tc[i] <= y_index0, row0[i] + chunk rows <= slot_rows, slots distinct and < B -- and only
 * launches: slot, t0 and row0 travel by value in the kernel arguments, nothing is allocated, copied or synchronised.
 *   chunks : work units per item of the segmented stream (0: every item its share of 2 x #CUs units by token count), as in
 *            hicom_compressor_ragged_args; E == 1152, nh <= 16, hidden % 64 == 0, H % ks == W % ks == 0, kt ks ks <= 64 */
typedef struct hicom_stream_group_push_args {
    const void* ff;
    const void* fe;
    const void* guide;
    int32_t B, items, H, W, E, kt, ks, nh;
    int32_t hidden, chunks;
    const void* q_hi;
    const void* q_lo;
    const float* pos_a;
    const float* pe;
    int32_t P, y_index0, x_index0;
    float l_scale;
    void* ws;
    int64_t ws_bytes;
    float* state_ml;
    float* state_acc;
    const void* lw0_f16;
    const void* lb0;
    const void* lw2_f16;
    const void* lb2;
    void* out;
    int32_t out_dt, nl_group;
    int64_t ldo, slot_stride, slot_rows;
    const void* newline;
    int32_t tc[32];
    int32_t slot[32];
    int32_t t0[32];
    int32_t row0[32];
    void* stream;
} hicom_stream_group_push_args;
int64_t hicom_compressor_stream_group_workspace_bytes(const hicom_stream_group_push_args* args);
int hicom_compressor_stream_group_prepare(const hicom_stream_group_push_args* args);
int hicom_compressor_stream_group_push(const hicom_stream_group_push_args* args);

/* The merge + fold kernel of the push alone: `items` chunks of Tc frames, item i's nparts partials in the slots [i nparts, (i + 1) nparts)
 * of part_m / part_l f32 [slots][16] and part_acc f32 [slots][16][E] (rows >= rows are not read), its logits f32 [16][ceil16(Tc H W)] at
 * scores + i 16 ceil16(Tc H W) (read when pe is given).  With M_c the maximum of the item's m_p:
 *     L_c = sum_p e^(m_p - M_c) l_p      ACC_c = sum_p e^(m_p - M_c) acc_p + sum_s marg_s pe[s]
 * marg = the t / y / x marginals of e^(logit - M_c), the t rows of pe (f32 [P][E]) at t0[i] + t, the y / x rows at y_index0 / x_index0.
 * The set is folded into rows slot[i] rows .. of state_ml [B][rows][2] / state_acc [B][rows][E] in place with the arithmetic of
 * hicom_stream_state_fold_set_fwd (an empty term weighs 0).  slot / t0: HOST arrays of `items` ints; slots distinct and < B <= 32. */
int hicom_stream_group_merge_fold_fwd(const float* part_m, const float* part_l, const float* part_acc, const float* scores, int32_t items,
                                      int32_t nparts, int32_t rows, int32_t E, int32_t Tc, int32_t H, int32_t W, const float* pe, int32_t P,
                                      int32_t y_index0, int32_t x_index0, const int32_t* slot, const int32_t* t0, int32_t B, float* state_ml,
                                      float* state_acc, void* stream);

/* ---- clip stream group with several guides per slot -----------------------------------------------------------------
 * Slot s has Q_s guides (1 <= Q_s <= 32); a PAIR is one (slot, guide), numbered slot-major then guide-major: slot s owns the pairs
 * [pair0_s, pair0_s + Q_s), pair0_s = sum_{j<s} Q_j, M = sum Q_s pairs in all (hicom_compressor_ragged_multiguide_args' convention).
 * Everything is pair-major: guide bf16 [M][E], q_hi / q_lo bf16 [>= M nh][E] and pos_a f32 [>= M nh][P] with row pair nh + h
 * (hicom_linear_fwd + hicom_fold_query_split_fwd over the M guides), state_ml f32 [M nh][2], state_acc f32 [M nh][E] -- slot s's rows are
 * contiguous -- and out: pair p starts pair_stride ELEMENTS behind pair 0 and has pair_rows rows of ldo elements.
 *
 * One push takes `items` chunks (1 <= items <= B <= 32) of the stacked tensor ff / fe bf16 [sum tc_i, H, W, E]; item i has tc[i] frames and
 * the q[i] guides of slot slot[i], whose first pair is pair0[i]; its frames start at the absolute offset t0[i], its chunk rows go to rows
 * row0[i] .. of each of its pairs.  Six launches whatever items, q and tc are: the local stage over the stack's windows (every guide of the
 * item's slot, tokens loaded once per 4 guides), the segmented stream with two row groups (32 folded rows of one item per workgroup, one
 * pass per 32 rows), the merge of every folded row's partials folded into the pair's state IN PLACE (one workgroup per (item, folded row):
 * a slot appears at most once per push and the items' pair ranges do not meet), the two hicom_readout16_gemm_fwd launches over all pairs'
 * window contexts and the placement.
 *
 * hicom_compressor_stream_group_multi_workspace_bytes: the plan's workspace for the tuple ((tc[i], q[i])), from B, M, items, tc, q, the
 * geometry, hidden, out_dt, nl_group and chunks alone (a negative status on a refusal).  ..._prepare writes the static tables of that
 * tuple to the head of ws: one copy, synchronises `stream`; once per plan.  ..._push checks every shape, pointer, alignment, table bound,
 * slot and pair range in front of the first launch -- t0[i] + tc[i] <= y_index0, row0[i] + chunk rows <= pair_rows, slots distinct and
 * < B, 1 <= q[i] <= 32, pair0[i] + q[i] <= M -- and only launches: pair0, t0 and row0 travel by value in the kernel arguments, nothing is
 * allocated, copied or synchronised.  chunks: token chunks per item and pass (0: the item's share of 2 x #CUs work units by tiles x passes). */
typedef struct hicom_stream_group_multi_push_args {
    const void* ff;
    const void* fe;
    const void* guide;
    int32_t B, M, items, H, W, E, kt, ks, nh, hidden, chunks, reserved_;
    const void* q_hi;
    const void* q_lo;
    const float* pos_a;
    const float* pe;
    int32_t P, y_index0, x_index0;
    float l_scale;
    void* ws;
    int64_t ws_bytes;
    float* state_ml;
    float* state_acc;
    const void* lw0_f16;
    const void* lb0;
    const void* lw2_f16;
    const void* lb2;
    void* out;
    int32_t out_dt, nl_group;
    int64_t ldo, pair_stride, pair_rows;
    const void* newline;
    int32_t tc[32];
    int32_t q[32];
    int32_t slot[32];
    int32_t t0[32];
    int32_t row0[32];
    int32_t pair0[32];
    void* stream;
} hicom_stream_group_multi_push_args;
int64_t hicom_compressor_stream_group_multi_workspace_bytes(const hicom_stream_group_multi_push_args* args);
int hicom_compressor_stream_group_multi_prepare(const hicom_stream_group_multi_push_args* args);
int hicom_compressor_stream_group_multi_push(const hicom_stream_group_multi_push_args* args);

/* The merge + fold kernel of that push alone: `items` chunks of Tc frames with Q guides each, rows = heads, R = rows Q folded rows per item in
 * passes = ceil(R / 32) passes.  Item i's partials lie in the slots [i S, (i + 1) S), S = 2 passes nparts, ordered [pass][row group][chunk]
 * (folded row R: row R % 16 of the slots i S + (R / 16) nparts + c, c < nparts) of part_m / part_l f32 [slots][16] and part_acc f32
 * [slots][16][E]; its logits f32 [32 passes][ceil16(Tc H W)] at scores + i 32 passes ceil16(Tc H W) (read when pe is given).  The arithmetic
 * is that of hicom_stream_group_merge_fold_fwd per folded row, into rows pair0[i] rows + R of state_ml [M rows][2] / state_acc [M rows][E] in
 * place.  pair0 / t0: HOST arrays of `items` ints; the ranges [pair0[i], pair0[i] + Q) lie inside the M pairs and do not meet. */
int hicom_stream_group_multi_merge_fold_fwd(const float* part_m, const float* part_l, const float* part_acc, const float* scores, int32_t items,
                                            int32_t nparts, int32_t rows, int32_t Q, int32_t E, int32_t Tc, int32_t H, int32_t W, const float* pe,
                                            int32_t P, int32_t y_index0, int32_t x_index0, const int32_t* pair0, const int32_t* t0, int32_t M,
                                            float* state_ml, float* state_acc, void* stream);

/* The placement of a batched finish alone: for every slot s < B with bit s of `named` set and every q < guide_counts[s], into pair
 * pair0_s + q of out ([M][pair_rows][ldo], pairs pair_stride elements apart) at row row0[s]: `tail` (0 | 1) copies of newline (bf16
 * [hidden]), then n_rows copies of tok[pair0_s + q] (f32 [M][hidden], rounded once: the copies are bit-identical).  Rows of tok that
 * belong to slots not named are never read, their pairs never written.  guide_counts / row0: HOST arrays of B ints (row0 of a slot not
 * named is not looked at). */
int hicom_stream_group_place_global_fwd(const float* tok, const void* newline, int32_t B, const int32_t* guide_counts, const int32_t* row0,
                                        uint32_t named, int32_t tail, int32_t n_rows, int32_t hidden, void* out, int32_t out_dt, int64_t ldo,
                                        int64_t pair_stride, int64_t pair_rows, void* stream);

/* ---- clip stream group on the k / v adaptor recipe -------------------------------------------------------------------
 * The group above for a module with adapt_k and / or adapt_v on the local stage.  The adaptor MLPs know neither the guide nor the slot,
 * so one tick's tokens of all items go through them ONCE: a push is eight launches whatever items, q and tc are --
 * hicom_clip_adapt_prepare_fwd over the sum N_i STACKED tokens (two launches: layer 1 and layer 2, a GEMM pair each with both adaptors)
 * into fp16 planes ky / vy [sum N_i, E], the adaptor local stage over the stack's windows (item i reads its tokens and its plane rows at
 * its first token, the guides of its slot in groups of 4), then launches 2-6 of hicom_compressor_stream_group_multi_push unchanged.  The
 * k adaptor reads fe (ff when fe is NULL), the v adaptor ff.
 *   base         : the plain block, every field as there; its ws also holds the two planes and the hidden planes of layer 1
 *                  (hicom_clip_adapt_prepare_workspace_bytes(sum N_i, E, ak, av)) BEHIND the plain regions, whose offsets do not move:
 *                  4 x 2 E bytes per token of a push with both adaptors
 *   ak, av       : w0 == NULL: that stream is not adapted (at least one is, HICOM_EINVAL); every field of an adapted stream is read
 *   alpha_dt, eps: as in hicom_compressor_multiguide_adapt_args
 * ..._workspace_bytes / ..._prepare / ..._push as for the plain group, with (sum N_i) E < 2^32 (the dense GEMM's operand limit over the
 * stack, HICOM_EUNSUP) and the checks of hicom_clip_adapt_prepare_fwd, all in front of the first launch. */
typedef struct hicom_stream_group_adapt_push_args {
    hicom_stream_group_multi_push_args base;
    hicom_seg_adaptor ak, av;
    int32_t alpha_dt;
    float eps;
} hicom_stream_group_adapt_push_args;
int64_t hicom_compressor_stream_group_adapt_workspace_bytes(const hicom_stream_group_adapt_push_args* args);
int hicom_compressor_stream_group_adapt_prepare(const hicom_stream_group_adapt_push_args* args);
int hicom_compressor_stream_group_adapt_push(const hicom_stream_group_adapt_push_args* args);

/* The adaptor local stage of that push alone: `items` chunks of Tc frames with Q guides each, packed one behind the other.  key / value bf16
 * [items Tc, H, W, E]; ky / vy fp16 [items Tc H W, E], the planes of the whole stack (one of them may be NULL: that stream is not adapted);
 * guide bf16 [M][E], item i takes the rows pair0[i] .. pair0[i] + Q (pair0: a HOST array; the ranges lie inside the M pairs and do not
 * meet); fp16 contexts ctx_f16 [items][Q][windows of a chunk][E].  Per item the arithmetic, shapes, limits and checks of
 * hicom_multi_guide_local_adapt_fwd on that chunk with its own rows of the planes. */
int hicom_stream_group_local_adapt_fwd(const void* key, const void* value, const void* guide, const void* ky, const void* vy,
                                       const hicom_seg_adaptor* ak, const hicom_seg_adaptor* av, int32_t alpha_dt, float eps, int32_t items,
                                       int32_t Q, int32_t Tc, int32_t H, int32_t W, int32_t E, int32_t kt, int32_t ks, float scale,
                                       const int32_t* pair0, int32_t M, void* ctx_f16, void* stream);

/* ---- multi-guide step without frames_embed: the local logits of Q guides from the SigLIP head's hidden layer -----------
 * frames_embed = x + fc2(hid) + b2 enters the plain release recipe only through g_q . frames_embed[n], which is linear in it:
 *     g_q . frames_embed[n] = g_q . x[n] + U[q] . hid[n] + c[q],     U[q] = W2^T g_q,  c[q] = g_q . b2.
 * The second head GEMM is not run and frames_embed is never written (csrc/head_scores.hip).
 *
 * hicom_head_guide_fold_fwd (two launches): w2 bf16 [D][inter] (fc2.weight), b2 bf16 [D] or NULL, guides bf16 [Q][D], 1 <= Q <= 32,
 * D <= 2048.  U in fp32, split into an fp16 pair at a power of two per row: u_hi + u_lo = U[q] 2^s with max |U[q]| 2^s in [2^14, 2^15),
 * fp16 [Qpad][ldu], Qpad = Q rounded up to 16, zero from column inter on and in the rows behind Q; u_scale [Qpad] = 2^-s, c [Qpad].
 * ldu >= inter, a multiple of 8 (hicom_head_scores_multi_fwd wants kpad rounded up to 128).  ws: 16 Q ldu floats, nothing to zero.
 *
 * hicom_head_scores_multi_fwd (one launch): x bf16 [M][D], hid fp16 [M][ld] of which columns [0, kpad) are read (the fp16 hidden plane
 * hicom_dense16_gemm_fwd stores with n_store = kpad: zero from column inter on; the pitch gap behind kpad is never read), the planes of
 * the fold.  logits[q q_stride + n] = g_q . x[n] + 2^-s (u_hi + u_lo)[q] . hid[n] + c[q] for q < Q, n < M, fp32 accumulation: the raw
 * dot products in front of the 1 / sqrt(D) scale.  D % 128 == 0, kpad % 64 == 0, ld % 8 == 0, any M. */
int hicom_head_guide_fold_fwd(const void* w2, const void* b2, int32_t D, int32_t inter, const void* guides, int32_t Q, void* u_hi, void* u_lo,
                              int64_t ldu, float* u_scale, float* c, void* ws, int64_t ws_bytes, void* stream);
int hicom_head_scores_multi_fwd(const void* x, const void* hid, int64_t ld, int64_t M, int32_t D, int32_t kpad, const void* guides,
                                const void* u_hi, const void* u_lo, int64_t ldu, const float* u_scale, const float* c, int32_t Q, float* logits,
                                int64_t q_stride, void* stream);

/* The local stage of the multi-guide step with the logits given: value bf16 [T, H, W, 1152], logits f32, guide q's [T H W] plane q_stride
 * floats behind guide 0's; at / ay / ax describe an exact window partition (n = nwin k, nfull = nwin) with square spatial windows of at most
 * 64 tokens, nwin = their product.  Per window and guide: softmax(scale logits) over the window's tokens, every value row loaded once per
 * group of guides; fp16 contexts ctx_f16 [Q][nwin][1152] as hicom_multi_guide_local_fwd writes them.  No key row is read.
 *
 * hicom_compressor_multiguide_logits_fwd is hicom_compressor_multiguide_fwd with that launch as its local stage: the same launch count,
 * the same workspace (hicom_compressor_multiguide_workspace_bytes); args->fe is not read and may be NULL.  local_logits f32 [Q][q_stride],
 * q_stride >= T H W. */
int hicom_multi_guide_local_logits_fwd(const void* value, const float* logits, int64_t q_stride, hicom_axis at, hicom_axis ay, hicom_axis ax,
                                       int32_t Q, int32_t nwin, float scale, void* ctx_f16, void* stream);
int hicom_compressor_multiguide_logits_fwd(const hicom_compressor_multiguide_args* args, const float* local_logits, int64_t q_stride);

/* ---- ragged multi-guide step without frames_embed: head scores per item -------------------------------------------------
 * B items stacked, item i with N_i tokens and its own Q_i guides (rows [pair0_i, pair0_i + Q_i) of guides [M][D], M = sum Q_i): item i's
 * tokens meet item i's guides only.
 *
 * hicom_head_guide_fold_many_fwd: hicom_head_guide_fold_fwd for 1 <= M <= 4096 guide rows in the same two launches, every row bit for bit
 * what the single form gives it.  The planes hold ceil16(M) + 32 rows (u_hi / u_lo fp16 [rows][ldu], u_scale / c f32 [rows]); rows >= M are
 * zero with scale 1 and c = 0.  ws: 16 M ldu floats.
 *
 * hicom_head_scores_ragged_fwd (one launch, one workgroup per tile of 32 tokens of ONE item): items is a DEVICE table [B][8] of
 * {tok0, N, pair0, Q, tile0, 0, 0, 0} (first token in the stack, tokens, first guide row, guides, first tile; tiles are counted per item,
 * ceil(N_i / 32) each), tile_item a DEVICE array [ntiles] with the item of every tile, q_max = max Q_i (1 .. 32).  x, hid, ld, D, kpad, ldu
 * as for hicom_head_scores_multi_fwd; the planes are those of hicom_head_guide_fold_many_fwd (the rows behind an item's guides inside a tile
 * of 16 or 32 guide rows are read, so the 32 pad rows must exist).  logits f32 [q_max][q_stride], q_stride >= sum N_i: guide q of item i at
 * logits[q q_stride + tok0_i + n]; cells with q >= Q_i are not written.  That is q_max sum N_i floats: one item with many guides widens
 * every item's column.  With B = 1 the result equals hicom_head_scores_multi_fwd's bit for bit.  The tables are not read on the host: what
 * they hold is the caller's responsibility.
 *
 * hicom_compressor_ragged_multiguide_logits_fwd is hicom_compressor_ragged_multiguide_fwd with the local stage taking its scores from
 * local_logits (that layout; planes q >= Q_i of an item are not read): the same launch count, the same workspace, size function and
 * prepare call; args->fe is not read and may be NULL. */
int hicom_head_guide_fold_many_fwd(const void* w2, const void* b2, int32_t D, int32_t inter, const void* guides, int32_t M, void* u_hi, void* u_lo,
                                   int64_t ldu, float* u_scale, float* c, void* ws, int64_t ws_bytes, void* stream);
int hicom_head_scores_ragged_fwd(const void* x, const void* hid, int64_t ld, int32_t D, int32_t kpad, const void* guides, const void* u_hi,
                                 const void* u_lo, int64_t ldu, const float* u_scale, const float* c, const int32_t* items, const int32_t* tile_item,
                                 int32_t B, int32_t ntiles, int32_t q_max, float* logits, int64_t q_stride, void* stream);
int hicom_compressor_ragged_multiguide_logits_fwd(const hicom_compressor_ragged_multiguide_args* args, const float* local_logits, int64_t q_stride);

/* ---- clip streams without frames_embed: head scores per chunk -------------------------------------------------------------
 * The three plain pushes with the local stage taking its scores precomputed: the raw dot products frames_embed[n] . guide in front of
 * l_scale, f32, indexed by the token's place in the CHUNK (the stack of a tick for the group), never by its place in the clip.  Each entry
 * takes the keyed entry's argument block unchanged: args->fe is not read and may be NULL or stale; t0 positions the chunk on the time axis
 * for the positional tables only.  Launch count, workspace, size function, prepare call, tables and every other launch are the keyed
 * push's.  Nothing is launched before every check has passed (NULL or unaligned logits -- 4 bytes --, a short q_stride: HICOM_EINVAL).
 *
 * hicom_compressor_stream_push_logits: local_logits f32 [Tc H W]; launch 1 is hicom_fused_stream_fwd(ff, NULL, local_logits, ...).
 *
 * hicom_compressor_stream_push_multi_logits: local_logits f32 [Q][q_stride], q_stride >= Tc H W, guide q's plane q_stride floats behind
 * guide 0's (what hicom_head_scores_multi_fwd writes); launch 1 is hicom_multi_guide_local_logits_fwd.
 *
 * hicom_compressor_stream_group_multi_push_logits: local_logits f32 [max Q_i over the push's items][q_stride], q_stride >= sum Tc_i H W:
 * guide q of item i at logits[q q_stride + tok0_i + n], tok0_i = the item's first token in the stack, n < Tc_i H W -- the layout
 * hicom_head_scores_ragged_fwd writes for the tick's items.  Guide q of an item is plane q, whichever pairs its slot owns; planes q >= Q_i
 * over an item's tokens and the gap behind sum Tc_i H W are never read.  Launch 1 reads neither key rows nor guide rows. */
int hicom_compressor_stream_push_logits(const hicom_stream_push_args* args, const float* local_logits);
int hicom_compressor_stream_push_multi_logits(const hicom_stream_push_multi_args* args, const float* local_logits, int64_t q_stride);
int hicom_compressor_stream_group_multi_push_logits(const hicom_stream_group_multi_push_args* args, const float* local_logits, int64_t q_stride);

/* ---- ragged step and its training step without frames_embed: local scores given ---------------------------------------------
 * One guide per item.  local_logits f32 [sum T_i H W]: the raw dot products frames_embed[n] . guide_item in front of l_scale, token n of item
 * i at tok0_i + n (plane 0 of what hicom_head_scores_ragged_fwd writes with one guide per item).  Plain recipe only.
 *
 * hicom_compressor_ragged_logits_fwd is hicom_compressor_ragged_fwd with the local stage taking its scores from local_logits: the same launch
 * count, the same workspace, size function and prepare call; args->fe is not read and may be NULL or stale; only value rows are read by the
 * local stage.  hicom_compressor_ragged_train_state works unchanged behind it.
 *
 * hicom_compressor_ragged_local_logits_bwd: the window backward of that local stage over the concatenated window list, one launch, one wave
 * per window.  Per window, p = softmax(l_scale l) over its tokens, dp_n = dctx_w . value_n:
 *   dlogits f32 [sum T_i H W]:  l_scale p_n (dp_n - sum_m p_m dp_m)
 *   dvalue  bf16 [sum T_i H W, E] or NULL:  p_n dctx_w, the value-side share of d frames_feature (hicom_compressor_ragged_global_dx adds the
 *           global share with accumulate = 1)
 * Every token lies in exactly one window: plain stores, fixed summation orders, no atomics.  There is no dq: the guide does not enter the
 * local stage.  value bf16 [sum T_i H W, E], dctx f32 [sum w_i, E] (16-byte aligned).  It reads only the table region of args->ws. */
int hicom_compressor_ragged_logits_fwd(const hicom_compressor_ragged_args* args, const float* local_logits);
int hicom_compressor_ragged_local_logits_bwd(const hicom_compressor_ragged_args* args, const void* value, const float* local_logits, const float* dctx,
                                             float* dlogits, void* dvalue);

/* ---- training step of the ragged multi-guide step: Q_i guides per item, one backward ---------------------------------------
 * Behind hicom_compressor_ragged_multiguide_fwd (or _logits_fwd) on the same block.  M = sum Q_i pairs, numbered item-major then guide-major;
 * rows are pair-major: row nh p + h is head h of pair p.  Each call reads the table region at the head of args->ws and checks its pointers,
 * their alignment and the workspace size in front of any launch or copy.  Plain recipe only.
 *
 * hicom_compressor_ragged_multiguide_train_state copies out of args->ws what a backward reads:
 *   ctx16_out  fp16 [sum Q_i windows_i, E]  the window contexts, pair-major (pair p owns windows_i rows)
 *   scores_out f32, the scores region: item i at 16 score_off_i, [32 passes_i][ceil16(N_i)], row nh q + h of the item's row space
 *   ml_out     f32 [M nh, 2]  (M, L) of the global softmax per (pair, head), from the partial states in the merge's own summation order
 *   ctxg_out   f32 [M nh, E]  the merged contexts
 *
 * hicom_compressor_ragged_multiguide_global_bwd: the attention backward of the global stage over all pairs, four launches whatever B, the Q_i
 * and the mix are: dctx -> bf16 hi / lo planes; pos_b = dctx pe^T; the two-row-group backward stream on the forward's work units (an
 * item's tokens are read once per 32 folded rows); the dq merge per (pair, head).
 *   x        bf16 [sum T_i H W, E] the tokens the forward read (16-byte aligned)
 *   dctx     f32 [M nh, E], delta f32 [M nh] = dctx_r . ctx_r, scores / ml as train_state left them
 *   ds_out   f32, laid out as scores (!= scores): dS; rows >= nh Q_i of an item's last pass are not written
 *   dqt_out  f32 [M nh, E]: d of the folded queries
 *   bws      hicom_compressor_ragged_multiguide_global_bwd_workspace_bytes(args) bytes, 256-byte aligned */
int hicom_compressor_ragged_multiguide_train_state(const hicom_compressor_ragged_multiguide_args* args, void* ctx16_out, float* scores_out, float* ml_out,
                                                   float* ctxg_out);
int64_t hicom_compressor_ragged_multiguide_global_bwd_workspace_bytes(const hicom_compressor_ragged_multiguide_args* args);
int hicom_compressor_ragged_multiguide_global_bwd(const hicom_compressor_ragged_multiguide_args* args, const void* x, const float* dctx, const float* delta,
                                                  const float* scores, const float* ml, float* ds_out, float* dqt_out, void* bws, int64_t bws_bytes);

/* ---- input gradients of that training step (stage 3) ---------------------------------------------------------------------
 * A token's gradient is a sum over its item's Q_i guides: it is formed in fp32 in the order q = 0 .. Q_i - 1 and written once.  The calls
 * check their pointers and the per-item partition in front of anything that needs a device, and read the tables from the head of args->ws.
 *
 * hicom_compressor_ragged_multiguide_local_bwd: the window backward, one workgroup per window of the stacked tensor (sum windows_i of them);
 * a window's key and value rows serve all guides of its item.
 *   key / value  bf16 [sum N_i, E]: frames_embed (or frames_feature without it) / frames_feature;  guide bf16 [M, E]
 *   dctx         f32 [sum Q_i windows_i, E], pair-major as the window contexts;  dq f32, the same shape: scale sum_i dS_qi k_i
 *   dkey         bf16 [sum N_i, E] or NULL: scale sum_q dS_qi guide_q
 *   dvalue       bf16 [sum N_i, E] or NULL: sum_q p_qi dctx_q (+ dkey_i with value_is_key: key == value, dkey NULL)
 * Plain stores: every token lies in one window.  With every Q_i = 1 dq, dkey and dvalue have hicom_compressor_ragged_local_bwd's values.
 *
 * hicom_compressor_ragged_multiguide_dq_pair: dq_pair f32 [M, E] = the sum of a pair's windows_i rows of dq, in
 * hicom_compressor_ragged_local_bwd's fixed order, without atomics.
 *
 * hicom_compressor_ragged_multiguide_global_dx: dx[n] (+)= sum over the nh Q_i rows R of the token's item of dS[R, n] qt[R] + softmax(S)[R, n]
 * dctx[R]; one fp32 chain per token and channel in row order from the bf16 row dx holds (accumulate), one bf16 store.
 *   scores / ds / ml as train_state / global_bwd left them;  qt, dctx f32 [M nh, E]
 *   tiles  DEVICE int32 [ntiles, 2]: (item, first token of the tile inside the item), 64 tokens per tile, ntiles = sum ceil(N_i / 64)
 *   dx     bf16 [sum N_i, E] */
int hicom_compressor_ragged_multiguide_local_bwd(const hicom_compressor_ragged_multiguide_args* args, const void* key, const void* value, const void* guide,
                                                 const float* dctx, float* dq, void* dkey, void* dvalue, int32_t value_is_key);
int hicom_compressor_ragged_multiguide_dq_pair(const hicom_compressor_ragged_multiguide_args* args, const float* dq, float* dq_pair);
int hicom_compressor_ragged_multiguide_global_dx(const hicom_compressor_ragged_multiguide_args* args, const float* scores, const float* ds, const float* ml,
                                                 const float* qt, const float* dctx, const int32_t* tiles, int32_t ntiles, void* dx, int32_t accumulate);

#ifdef __cplusplus
}
#endif
#endif /* HICOM_HIP_H */
