// Multi-guide compressor step: ONE clip, Q instructions, the visual tokens read once.
//
// The guide enters the two stages only as a query: one more 1152-d query against the same keys and values of every window, nh more
// folded rows against the same token tiles.  So Q guides are one pass over the tokens plus Q times the window-sized work, in a launch
// sequence whose length does not depend on Q:
//    1-2  hicom_linear_fwd (q_proj), hicom_fold_query_split_fwd with M = Q: the nh folded rows of guide q are rows nh q .. nh q + nh - 1,
//         densely packed (rows_pad = the row count rounded up to the 32 rows of one pass of the many-row stream kernel)
//    3    multi_guide_local_kernel: one wave per window, every key row and every value row of the window loaded once per group of
//         kGuideGroup guides; fp16 contexts into the guide-major plane [Q][windows][E]
//    4    the many-row global stream (global_stream.hip, the kernel of the guide-off recipe) over the nh Q rows
//    5    its merge with the value-side positional term (merge.hip): two launches behind in-kernel marginals, three behind the logit tensor
//    6-9  v_proj per head, out_proj + residual, GELU(gw0 .), gw2 with M = Q
//  10-11  the local readout as one GEMM pair over M = Q x windows rows
//   12    placement (segment_item.hpp: place_equal_row, item = guide)
// Launches 1-2 and 6-11, the workspace regions and the common checks are segment_host.hpp's, with M = Q; this file holds the local kernel,
// the four launches that know a guide, the chunk policy and the step's own limits.  The packed-row layout integers are those of the batched
// step and hold for every guide.
//
// Prepared clips: for the k / v adaptor recipe hicom_clip_adapt_prepare_fwd runs the adaptor MLPs over a clip's tokens
// once, into planes the caller keeps; hicom_compressor_multiguide_adapt_fwd is the sequence above with launch 3 replaced by
// multi_guide_local_adapt_kernel, which blends LayerNorm of those planes into the rows it loads.  Same launch count, same workspace.
// hicom_multi_guide_local_adapt_fwd is that launch alone, for a clip stream's chunk.
//
// Logits form: hicom_compressor_multiguide_logits_fwd is the plain sequence with launch 3 replaced by
// multi_guide_local_logits_kernel, which takes the local logits of every guide precomputed (hicom_head_scores_multi_fwd) and reads the
// value rows only.  Same launch count, same workspace; frames_embed is not read.  hicom_multi_guide_local_logits_fwd is that launch alone.
#include "multi_window.hpp"
#include "segment_host.hpp"

namespace hicom {

// One wave per window of the clip's grid; for Q > kGuideGroup the wave walks further groups over the same window (its rows are then
// expected to come from L2).  ctx16: [Q][nwin][D].
template <int NV>
__global__ __launch_bounds__(256) void multi_guide_local_kernel(const uint16_t* key, const uint16_t* value, const uint16_t* guide, hicom_axis at,
                                                                hicom_axis ay, hicom_axis ax, int Q, int nwin, float scale, _Float16* ctx16) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const WindowGeom g(at, ay, ax, win);
    multi_window_guides_ctx16<NV>(key, value, guide, 0, Q, g, lane, scale, ctx16 + (long)win * D, (long)nwin * D);
}

// The same grid and wave -> window map for the k / v adaptor recipe on a clip's PREPARED planes (multi_window.hpp:
// multi_window_guides_adapt_ctx16; ad.ky / ad.vy: y = MLP(x) fp16 [tokens][D], indexed like the tokens).  Nothing here writes the planes.
// kAdaptGuideGroup = 4 guides per walk under the 256-thread launch bound alone: 233 VGPRs, no scratch, two waves per SIMD (DESIGN.md §3.10
// has the table: a group of 2 held to the 128 registers of four waves per SIMD spills 22 registers to scratch, and every no-scratch
// form of a smaller group was slower at Q = 4, the time being the number of walks).
template <int NV>
__global__ __launch_bounds__(256) void multi_guide_local_adapt_kernel(const uint16_t* key, const uint16_t* value, const uint16_t* guide, SegAdaptParams ad,
                                                                      hicom_axis at, hicom_axis ay, hicom_axis ax, int Q, int nwin, float scale,
                                                                      _Float16* ctx16) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const WindowGeom g(at, ay, ax, win);
    multi_window_guides_adapt_ctx16<NV, kAdaptGuideGroup>(key, value, ad, guide, 0, Q, g, lane, scale, ctx16 + (long)win * D, (long)nwin * D);
}

// The same grid and wave -> window map with the local logits given (multi_window.hpp: multi_window_guides_logits_ctx16; logits f32
// [Q][tokens], guide q's plane q_stride floats behind guide 0's).  No key row is read.
template <int NV>
__global__ __launch_bounds__(256) void multi_guide_local_logits_kernel(const uint16_t* value, const float* logits, long q_stride, hicom_axis at, hicom_axis ay,
                                                                       hicom_axis ax, int Q, int nwin, float scale, _Float16* ctx16) {
    constexpr int D = NV * 384;
    const int lane = threadIdx.x & 63;
    const int win = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (win >= nwin) return;
    const WindowGeom g(at, ay, ax, win);
    multi_window_guides_logits_ctx16<NV>(value, logits, q_stride, Q, g, lane, scale, ctx16 + (long)win * D, (long)nwin * D);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Placement of every guide's packed rows (segment_item.hpp: place_equal_row, item = guide): grid = Q * item_rows, one output row per
// workgroup.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void multi_guide_place_kernel(EqualPlaceParams p) { place_equal_row(p); }

}  // namespace hicom

using namespace hicom;
using namespace hicom_host;

namespace {

constexpr const char* kWho = "compressor_multiguide";
constexpr int kMaxGuides = 32;          // nh = 9 heads x 32 guides = 288 rows: the row count the many-row stream kernel is proven at
constexpr int kMaxStreamChunks = 256;

typedef hicom_compressor_multiguide_args Args;

// the plain local stage: one wave per window, four windows per workgroup (the step's launch 3 and hicom_multi_guide_local_fwd)
void launch_local_plain(const uint16_t* key, const uint16_t* value, const uint16_t* guide, hicom_axis at, hicom_axis ay, hicom_axis ax, int Q, int nwin,
                        float scale, _Float16* ctx16, void* stream) {
    HICOM_LAUNCH(multi_guide_local_kernel<3>, dim3((unsigned)((nwin + 3) / 4)), dim3(256), 0, (hipStream_t)stream, key, value, guide, at, ay, ax, Q, nwin,
                 scale, ctx16);
}

// the same grid for the adaptor recipe on prepared planes (the step's launch 3 and hicom_multi_guide_local_adapt_fwd)
void launch_local_adapt(const uint16_t* key, const uint16_t* value, const uint16_t* guide, const SegAdaptParams& ad, hicom_axis at, hicom_axis ay, hicom_axis ax,
                        int Q, int nwin, float scale, _Float16* ctx16, void* stream) {
    HICOM_LAUNCH(multi_guide_local_adapt_kernel<3>, dim3((unsigned)((nwin + 3) / 4)), dim3(256), 0, (hipStream_t)stream, key, value, guide, ad, at, ay, ax, Q,
                 nwin, scale, ctx16);
}

// the same grid with the local logits given (the logits step's launch 3 and hicom_multi_guide_local_logits_fwd)
void launch_local_logits(const uint16_t* value, const float* logits, long q_stride, hicom_axis at, hicom_axis ay, hicom_axis ax, int Q, int nwin, float scale,
                         _Float16* ctx16, void* stream) {
    HICOM_LAUNCH(multi_guide_local_logits_kernel<3>, dim3((unsigned)((nwin + 3) / 4)), dim3(256), 0, (hipStream_t)stream, value, logits, q_stride, at, ay, ax,
                 Q, nwin, scale, ctx16);
}

// the local logits of the logits step: f32 [Q][T H W], guide q's plane q_stride floats behind guide 0's; p NULL: the keyed forms
struct LocalLogits {
    const float* p;
    long q_stride;
};

// token chunks of the global stream
int mg_chunks(const Args* a, long N, int rows_pad) {
    const long ntiles = (N + 15) / 16;
    long c = a->chunks > 0 ? a->chunks : hicom_global_stream_nparts(N, rows_pad);
    if (c > ntiles) c = ntiles;
    if (c > kMaxStreamChunks) c = kMaxStreamChunks;
    return (int)(c < 1 ? 1 : c);
}

// The workspace (segment_host.hpp: seg_layout).  Per guide: qp, o, pre (E floats each), hid, tok (hidden floats each) and, per guide and
// window, the fp16 context row, the fp16 hidden row and the readout row of the output dtype.  Per folded row (rows_pad of them, whatever Q
// is inside a pass): the hi / lo query planes, the score-side positional table, the merged contexts and softmax states, the merge's scratch
// and, per row and token chunk, the partial states.  Token-sized: only `scores`, the [rows_pad][N] logits of the stream's logit-tensor form
// (the in-kernel-marginal form keeps its [chunks][rows_pad][marg width] marginals there instead; the region holds either).
struct MgLayout {
    SegLayout s;
    long N, score_stride;
    int rows, rows_pad, nparts, wpi;
};

MgLayout mg_layout(const Args* a) {
    MgLayout l;
    l.N = (long)a->T * a->H * a->W;
    l.rows = a->Q * a->nh;
    l.rows_pad = (l.rows + 31) / 32 * 32;
    l.nparts = mg_chunks(a, l.N, l.rows_pad);
    l.wpi = (a->T / a->kt) * (a->H / a->ks) * (a->W / a->ks);
    l.score_stride = (l.N + 15) / 16 * 16;
    const long R = l.rows_pad, logits = R * l.score_stride, marg = (long)l.nparts * R * hicom_global_stream_marg_width(a->H, a->W);
    l.s = seg_layout(a, nullptr, SegTotals{logits > marg ? logits : marg, l.nparts, (long)a->Q * l.wpi, l.N, R, l.nparts * R, R * a->T * (a->H + a->W + 2)}, 0);
    return l;
}

int mg_check(const Args* a) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "compressor_multiguide: NULL arguments");
    HICOM_REQUIRE(a->Q >= 1 && a->Q <= kMaxGuides, HICOM_EUNSUP, "compressor_multiguide: Q=%d guides (1 <= Q <= %d per call)", a->Q, kMaxGuides);
    HICOM_REQUIRE(a->T > 0 && a->H > 0 && a->W > 0 && a->hidden > 0 && a->kt > 0 && a->ks > 0, HICOM_EINVAL, "compressor_multiguide: bad shape");
    const int st = seg_check_shape(kWho, "guide", a);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->T % a->kt == 0 && a->H % a->ks == 0 && a->W % a->ks == 0, HICOM_EUNSUP,
                  "compressor_multiguide: needs an exact window partition (T=%d H=%d W=%d, windows %dx%dx%d)", a->T, a->H, a->W, a->kt, a->ks, a->ks);
    HICOM_REQUIRE(a->kt * a->ks * a->ks <= 64, HICOM_EUNSUP, "compressor_multiguide: windows of %d tokens (<= 64)", a->kt * a->ks * a->ks);
    const long N = (long)a->T * a->H * a->W;
    HICOM_REQUIRE(N < (1L << 31) / 16 && N * a->Q < (1L << 31) / 16, HICOM_EUNSUP, "compressor_multiguide: too many tokens in one call");
    // what the merge (merge.hip) keeps in LDS: a frame of logits per workgroup on grids above 32 x 32, the row's weights and 64 staged
    // frames of marginals
    HICOM_REQUIRE(a->H + a->W <= 1024 && ((a->H <= 32 && a->W <= 32) || ((long)a->H * a->W + a->H + 4) * 4 <= 60000), HICOM_EUNSUP,
                  "compressor_multiguide: a %dx%d grid: the merge keeps a frame of logits in LDS", a->H, a->W);
    HICOM_REQUIRE(((long)kMaxStreamChunks + 2L * a->T + a->H + a->W + 64L * (a->H + a->W + 2) + 16 * 64 + 4) * 4 <= 60000, HICOM_EUNSUP,
                  "compressor_multiguide: T=%d frames of %dx%d: the merge keeps the row's T + H + W weights and 64 frames of marginals in LDS", a->T,
                  a->H, a->W);
    return HICOM_OK;
}

// the four launches whose item is a guide of the one clip (segment_host.hpp: seg_step).  The stream and its merge are the many-row entry
// points of the guide-off recipe over all guides' folded rows -- guide q's are rows nh q .. of the planes, rows >= nh Q are never stored by
// the stream -- which take their arguments one by one: the common parameter blocks are not used.
struct GuideItems {
    const Args* a;
    const MgLayout& l;
    bool marg;              // in-kernel positional marginals (clips), the logit tensor otherwise
    const SegAdaptParams* prepared;     // the adaptor recipe on a clip's prepared planes (hicom_compressor_multiguide_adapt_fwd), NULL: plain
    LocalLogits logits;                 // the logits form (hicom_compressor_multiguide_logits_fwd): no key row is read
    char* ws() const { return (char*)a->ws; }
    float* f32(long off) const { return (float*)(ws() + off); }
    float* pos_a() const { return a->pe ? f32(l.s.pos_a) : nullptr; }

    int local(const uint16_t* key_x, const SegAdaptParams*) const {
        const hicom_axis at{a->T, a->kt, a->T / a->kt, a->T / a->kt};
        const hicom_axis ay{a->H, a->ks, a->H / a->ks, a->H / a->ks}, ax{a->W, a->ks, a->W / a->ks, a->W / a->ks};
        if (logits.p)
            launch_local_logits((const uint16_t*)a->ff, logits.p, logits.q_stride, at, ay, ax, a->Q, l.wpi, a->l_scale, (_Float16*)(ws() + l.s.ctx16), a->stream);
        else if (prepared)
            launch_local_adapt(key_x, (const uint16_t*)a->ff, (const uint16_t*)a->guide, *prepared, at, ay, ax, a->Q, l.wpi, a->l_scale,
                               (_Float16*)(ws() + l.s.ctx16), a->stream);
        else
            launch_local_plain(key_x, (const uint16_t*)a->ff, (const uint16_t*)a->guide, at, ay, ax, a->Q, l.wpi, a->l_scale, (_Float16*)(ws() + l.s.ctx16),
                               a->stream);
        return seg_check_launch(kWho, "local stage");
    }

    int stream(const SegStreamParams&) const {
        const SegLayout& s = l.s;
        if (marg)
            return hicom_global_stream_marg_fwd(a->ff, l.N, a->E, ws() + s.qhi, ws() + s.qlo, l.rows, l.rows_pad, pos_a(), a->P, a->H, a->W, a->t_index0,
                                                a->y_index0, a->x_index0, nullptr, 0, f32(s.part_m), f32(s.part_l), f32(s.part_acc), f32(s.scores), l.nparts,
                                                a->stream);
        return hicom_global_stream_fwd(a->ff, l.N, a->E, ws() + s.qhi, ws() + s.qlo, l.rows, l.rows_pad, pos_a(), a->P, a->H, a->W, a->t_index0, a->y_index0,
                                       a->x_index0, f32(s.scores), l.score_stride, f32(s.part_m), f32(s.part_l), f32(s.part_acc), l.nparts, a->stream);
    }

    int merge(const SegMergeParams&) const {
        const SegLayout& s = l.s;
        if (marg)
            return hicom_global_merge_marg_fwd(f32(s.part_m), f32(s.part_l), f32(s.part_acc), f32(s.scores), l.nparts, l.rows, l.rows_pad, a->E, l.N, a->H, a->W,
                                               a->pe, a->t_index0, a->y_index0, a->x_index0, f32(s.scratch), f32(s.ml), f32(s.ctxg), 1, a->stream);
        return hicom_global_merge_fwd(f32(s.part_m), f32(s.part_l), f32(s.part_acc), l.nparts, l.rows, l.rows_pad, a->E, f32(s.scores), l.score_stride, l.N, a->H,
                                      a->W, a->pe, a->t_index0, a->y_index0, a->x_index0, f32(s.scratch), f32(s.ml), f32(s.ctxg), 1, a->stream);
    }

    int place(const SegPlaceParams& c) const { return seg_place_equal(kWho, multi_guide_place_kernel, a, c, l.wpi); }
};

// prepared: the local stage's adaptor parameters with the caller's planes, NULL for the plain recipe.  seg_step runs as for the plain recipe
// (no adaptor MLP, no adaptor region in the workspace): only the local hook differs.  logits: the logits form, likewise.
int mg_fwd(const Args* a, const SegAdaptParams* prepared = nullptr, LocalLogits logits = LocalLogits{nullptr, 0}) {
    int st = mg_check(a);
    if (st != HICOM_OK) return st;
    const MgLayout l = mg_layout(a);
    st = seg_check_fwd(kWho, a, nullptr, l.s.total);
    if (st != HICOM_OK) return st;
    st = seg_check_equal_rows(kWho, a, l.wpi);
    if (st != HICOM_OK) return st;
    const bool marg = a->pe && hicom_global_stream_has_marg(l.N, a->E, l.rows_pad, a->H, a->W, l.nparts) == 1;
    return seg_step(a, nullptr, l.s, GuideItems{a, l, marg, prepared, logits});
}

// ---- the k / v adaptor recipe on prepared planes ------------------------------------------------------------------------------------------
typedef hicom_compressor_multiguide_adapt_args AdaptArgs;

// what prepared planes add to the plain checks; a stream is adapted when its plane is given
int planes_check(const char* who, const void* ky, const void* vy, const hicom_seg_adaptor* ak, const hicom_seg_adaptor* av, int alpha_dt) {
    HICOM_REQUIRE(ky || vy, HICOM_EINVAL, "%s: neither stream has a prepared plane (the plain entry point runs that recipe)", who);
    HICOM_REQUIRE((uintptr_t)ky % 16 == 0 && (uintptr_t)vy % 16 == 0, HICOM_EINVAL, "%s: 16-byte aligned planes", who);
    HICOM_REQUIRE(alpha_dt == HICOM_DT_BF16 || alpha_dt == HICOM_DT_F32, HICOM_EINVAL, "%s: alpha dtype %d (bf16 | f32)", who, alpha_dt);
    HICOM_REQUIRE((!ky || (ak->gamma && ak->beta && ak->alpha)) && (!vy || (av->gamma && av->beta && av->alpha)), HICOM_EINVAL, "%s: adaptor weights", who);
    return HICOM_OK;
}

int mga_check(const AdaptArgs* a) { return planes_check(kWho, a->ky, a->vy, &a->ak, &a->av, a->alpha_dt); }

SegAdaptParams planes_params(const void* ky, const void* vy, const hicom_seg_adaptor* ak, const hicom_seg_adaptor* av, int alpha_dt, float eps) {
    SegAdaptParams p;
    p.ky = (const _Float16*)ky; p.kgamma = (const uint16_t*)ak->gamma; p.kbeta = (const uint16_t*)ak->beta; p.kalpha = ak->alpha;
    p.vy = (const _Float16*)vy; p.vgamma = (const uint16_t*)av->gamma; p.vbeta = (const uint16_t*)av->beta; p.valpha = av->alpha;
    p.alpha_f32 = alpha_dt == HICOM_DT_F32;
    p.eps = eps;
    return p;
}

// ---- y = MLP(x) planes of a clip (hicom_clip_adapt_prepare_*) ---------------------------------------------------------------------------------
constexpr const char* kWhoPrepare = "clip_adapt_prepare";

// The workspace holds the fp16 [N, E] hidden plane of layer 1 per adapted stream (k first), each rounded up to 256 bytes: the y planes
// are the caller's.  hid_v: where the value stream's begins.
int prepare_check(int64_t N, int32_t E, const hicom_seg_adaptor* ak, const hicom_seg_adaptor* av, SegAdapt* ad, long* hid_v, long* total) {
    HICOM_REQUIRE(ak && av, HICOM_EINVAL, "%s: NULL arguments", kWhoPrepare);
    HICOM_REQUIRE(N > 0 && E > 0, HICOM_EINVAL, "%s: bad shape", kWhoPrepare);
    *ad = SegAdapt{ak, av, HICOM_DT_BF16, 0.f};            // (the MLPs read neither alpha nor eps)
    const int st = seg_adapt_check(kWhoPrepare, ad, N, E);
    if (st != HICOM_OK) return st;
    const long plane = ((long)N * E * 2 + 255) / 256 * 256;
    *hid_v = ad->k() ? plane : 0;
    *total = *hid_v + (ad->v() ? plane : 0);
    return HICOM_OK;
}

}  // namespace

// ---- the local stage alone, for a caller that runs the other stages itself (clip_stream.hip: a chunk of a streamed clip; windows do not
// depend on the frame offset).  Everything is checked in front of the launch.
namespace {

int local_check(const char* who, const void* key, const void* value, const void* guide, int Q, int T, int H, int W, int E, int kt, int ks, const void* ctx_f16) {
    HICOM_REQUIRE(key && value && guide && ctx_f16, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE(Q >= 1 && Q <= kMaxGuides, HICOM_EUNSUP, "%s: Q=%d guides (1 <= Q <= %d per call)", who, Q, kMaxGuides);
    HICOM_REQUIRE(T > 0 && H > 0 && W > 0 && kt > 0 && ks > 0, HICOM_EINVAL, "%s: bad shape", who);
    HICOM_REQUIRE(E == 1152, HICOM_EUNSUP, "%s: E=%d (only 1152)", who, E);
    HICOM_REQUIRE(T % kt == 0 && H % ks == 0 && W % ks == 0 && kt * ks * ks <= 64, HICOM_EUNSUP,
                  "%s: needs an exact partition into windows of <= 64 tokens (T=%d H=%d W=%d, windows %dx%dx%d)", who, T, H, W, kt, ks, ks);
    const long nwin = (long)(T / kt) * (H / ks) * (W / ks);
    HICOM_REQUIRE((long)T * H * W < (1L << 31) / 16 && nwin * Q < (1L << 31) / 16, HICOM_EUNSUP, "%s: too many tokens in one call", who);
    HICOM_REQUIRE((uintptr_t)key % 16 == 0 && (uintptr_t)value % 16 == 0 && (uintptr_t)guide % 16 == 0 && (uintptr_t)ctx_f16 % 16 == 0, HICOM_EINVAL,
                  "%s: 16-byte aligned inputs", who);
    return HICOM_OK;
}

constexpr const char* kWhoLocalAdapt = "multi_guide_local_adapt";

}  // namespace

extern "C" int hicom_multi_guide_local_fwd(const void* key, const void* value, const void* guide, int32_t Q, int32_t T, int32_t H, int32_t W, int32_t E,
                                           int32_t kt, int32_t ks, float scale, void* ctx_f16, void* stream) {
    const int st = local_check("multi_guide_local", key, value, guide, Q, T, H, W, E, kt, ks, ctx_f16);
    if (st != HICOM_OK) return st;
    const long nwin = (long)(T / kt) * (H / ks) * (W / ks);
    const hicom_axis at{T, kt, T / kt, T / kt}, ay{H, ks, H / ks, H / ks}, ax{W, ks, W / ks, W / ks};
    launch_local_plain((const uint16_t*)key, (const uint16_t*)value, (const uint16_t*)guide, at, ay, ax, Q, (int)nwin, scale, (_Float16*)ctx_f16, stream);
    return seg_check_launch("multi_guide_local", "local stage");
}

extern "C" int hicom_multi_guide_local_logits_fwd(const void* value, const float* logits, int64_t q_stride, hicom_axis at, hicom_axis ay, hicom_axis ax,
                                                  int32_t Q, int32_t nwin, float scale, void* ctx_f16, void* stream) {
    const char* who = "multi_guide_local_logits";
    HICOM_REQUIRE(value && logits && ctx_f16, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE(Q >= 1 && Q <= kMaxGuides, HICOM_EUNSUP, "%s: Q=%d guides (1 <= Q <= %d per call)", who, Q, kMaxGuides);
    for (const hicom_axis* x : {&at, &ay, &ax})
        HICOM_REQUIRE(x->n > 0 && x->k > 0 && x->nwin > 0 && x->nwin * x->k == x->n && x->nfull == x->nwin, HICOM_EUNSUP,
                      "%s: needs an exact window partition (an axis of %d in %d windows of %d)", who, x->n, x->nwin, x->k);
    HICOM_REQUIRE(ay.k == ax.k && at.k * ay.k * ax.k <= 64, HICOM_EUNSUP, "%s: square spatial windows of <= 64 tokens (%dx%dx%d)", who, at.k, ay.k, ax.k);
    const long N = (long)at.n * ay.n * ax.n;
    HICOM_REQUIRE(nwin == (long)at.nwin * ay.nwin * ax.nwin, HICOM_EINVAL, "%s: nwin=%d for a grid of %dx%dx%d windows", who, nwin, at.nwin, ay.nwin, ax.nwin);
    HICOM_REQUIRE(N < (1L << 31) / 16 && (long)nwin * Q < (1L << 31) / 16, HICOM_EUNSUP, "%s: too many tokens in one call", who);
    HICOM_REQUIRE(Q == 1 || q_stride >= N, HICOM_EINVAL, "%s: q_stride=%ld floats between the guides' planes of %ld tokens", who, (long)q_stride, N);
    HICOM_REQUIRE((uintptr_t)value % 16 == 0 && (uintptr_t)logits % 4 == 0 && (uintptr_t)ctx_f16 % 16 == 0, HICOM_EINVAL, "%s: aligned inputs", who);
    launch_local_logits((const uint16_t*)value, logits, q_stride, at, ay, ax, Q, nwin, scale, (_Float16*)ctx_f16, stream);
    return seg_check_launch(who, "local stage");
}

// segment_host.hpp declares the two *_args_check functions: the checks of an entry point without its launches
int hicom_host::multi_guide_local_adapt_args_check(const void* key, const void* value, const void* guide, const void* ky, const void* vy,
                                                   const hicom_seg_adaptor* ak, const hicom_seg_adaptor* av, int alpha_dt, int Q, int T, int H, int W, int E,
                                                   int kt, int ks, const void* ctx_f16) {
    HICOM_REQUIRE(ak && av, HICOM_EINVAL, "%s: NULL arguments", kWhoLocalAdapt);
    const int st = local_check(kWhoLocalAdapt, key, value, guide, Q, T, H, W, E, kt, ks, ctx_f16);
    return st != HICOM_OK ? st : planes_check(kWhoLocalAdapt, ky, vy, ak, av, alpha_dt);
}

extern "C" int hicom_multi_guide_local_adapt_fwd(const void* key, const void* value, const void* guide, const void* ky, const void* vy,
                                                 const hicom_seg_adaptor* ak, const hicom_seg_adaptor* av, int32_t alpha_dt, float eps, int32_t Q, int32_t T,
                                                 int32_t H, int32_t W, int32_t E, int32_t kt, int32_t ks, float scale, void* ctx_f16, void* stream) {
    const int st = multi_guide_local_adapt_args_check(key, value, guide, ky, vy, ak, av, alpha_dt, Q, T, H, W, E, kt, ks, ctx_f16);
    if (st != HICOM_OK) return st;
    const long nwin = (long)(T / kt) * (H / ks) * (W / ks);
    const hicom_axis at{T, kt, T / kt, T / kt}, ay{H, ks, H / ks, H / ks}, ax{W, ks, W / ks, W / ks};
    launch_local_adapt((const uint16_t*)key, (const uint16_t*)value, (const uint16_t*)guide, planes_params(ky, vy, ak, av, alpha_dt, eps), at, ay, ax, Q,
                       (int)nwin, scale, (_Float16*)ctx_f16, stream);
    return seg_check_launch(kWhoLocalAdapt, "local stage");
}

extern "C" int64_t hicom_compressor_multiguide_workspace_bytes(const hicom_compressor_multiguide_args* a) {
    const int st = mg_check(a);
    if (st != HICOM_OK) return st;
    return mg_layout(a).s.total;
}

extern "C" int hicom_compressor_multiguide_fwd(const hicom_compressor_multiguide_args* a) { return mg_fwd(a); }

// The logits form: a->fe is not read (the workspace and its size function are the plain entry point's).
extern "C" int hicom_compressor_multiguide_logits_fwd(const hicom_compressor_multiguide_args* a, const float* local_logits, int64_t q_stride) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "%s: NULL arguments", kWho);
    HICOM_REQUIRE(local_logits && (uintptr_t)local_logits % 4 == 0, HICOM_EINVAL, "%s: local_logits is f32 [Q][T H W]", kWho);
    HICOM_REQUIRE(a->Q <= 1 || q_stride >= (int64_t)a->T * a->H * a->W, HICOM_EINVAL, "%s: q_stride=%ld floats between the guides' logit planes", kWho,
                  (long)q_stride);
    return mg_fwd(a, nullptr, LocalLogits{local_logits, (long)q_stride});
}

// The planes are the caller's: the workspace is the plain entry point's for the same arguments.
extern "C" int64_t hicom_compressor_multiguide_adapt_workspace_bytes(const hicom_compressor_multiguide_adapt_args* a) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "%s: NULL arguments", kWho);
    return hicom_compressor_multiguide_workspace_bytes(&a->base);
}

extern "C" int hicom_compressor_multiguide_adapt_fwd(const hicom_compressor_multiguide_adapt_args* a) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "%s: NULL arguments", kWho);
    int st = mg_check(&a->base);
    if (st != HICOM_OK) return st;
    st = mga_check(a);
    if (st != HICOM_OK) return st;
    const SegAdaptParams p = planes_params(a->ky, a->vy, &a->ak, &a->av, a->alpha_dt, a->eps);
    return mg_fwd(&a->base, &p);
}

extern "C" int64_t hicom_clip_adapt_prepare_workspace_bytes(int64_t N, int32_t E, const hicom_seg_adaptor* ak, const hicom_seg_adaptor* av) {
    SegAdapt ad;
    long hid_v = 0, total = 0;
    const int st = prepare_check(N, E, ak, av, &ad, &hid_v, &total);
    return st != HICOM_OK ? st : total;
}

int hicom_host::clip_adapt_prepare_args_check(const void* key_x, const void* ff, long N, int E, const hicom_seg_adaptor* ak, const hicom_seg_adaptor* av,
                                              const void* ky, const void* vy, const void* ws, long ws_bytes, long* hid_v_out) {
    SegAdapt ad;
    long hid_v = 0, total = 0;
    const int st = prepare_check(N, E, ak, av, &ad, &hid_v, &total);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(key_x && ff && (!ad.k() || ky) && (!ad.v() || vy), HICOM_EINVAL, "%s: NULL pointer", kWhoPrepare);
    for (const hicom_seg_adaptor* s : {ak, av})
        if (s->w0) HICOM_REQUIRE(s->w2_f16, HICOM_EINVAL, "%s: adaptor weights", kWhoPrepare);
    HICOM_REQUIRE(ws && ws_bytes >= total && (uintptr_t)ws % 256 == 0, HICOM_EINVAL, "%s: workspace of %ld bytes, 256-byte aligned", kWhoPrepare, total);
    HICOM_REQUIRE((uintptr_t)key_x % 16 == 0 && (uintptr_t)ff % 16 == 0 && (uintptr_t)ky % 16 == 0 && (uintptr_t)vy % 16 == 0, HICOM_EINVAL,
                  "%s: 16-byte aligned tokens and planes", kWhoPrepare);
    if (hid_v_out) *hid_v_out = hid_v;
    return HICOM_OK;
}

extern "C" int hicom_clip_adapt_prepare_fwd(const void* key_x, const void* ff, int64_t N, int32_t E, const hicom_seg_adaptor* ak, const hicom_seg_adaptor* av,
                                            void* ky, void* vy, void* ws, int64_t ws_bytes, void* stream) {
    long hid_v = 0;
    const int st = clip_adapt_prepare_args_check(key_x, ff, N, E, ak, av, ky, vy, ws, ws_bytes, &hid_v);
    if (st != HICOM_OK) return st;
    const SegAdapt ad{ak, av, HICOM_DT_BF16, 0.f};            // (the MLPs read neither alpha nor eps)
    return seg_adapt_mlps(ad, key_x, ff, N, E, ws, (char*)ws + hid_v, ky, vy, stream);
}
