// Host side of a many-item compressor step, shared by the equal-shape step (batch.hip), the ragged step (ragged.hip), the multi-guide
// step (multi_guide.hip, whose items are the guides of one clip) and the ragged multi-guide step (ragged_multi_guide.hip, whose items
// are (item, guide) pairs): the limits, the k / v adaptors of the local stage, the checks, the workspace layout and the launch sequence
// that do not depend on how a wave finds its item, and the walk over hicom_ragged_item descriptors of the two ragged steps (per-item
// requirements, chunk share, tile ranges, table upload).  The files keep their kernels, the code that launches them, their table
// structs and their own layout checks.  The shared functions are templates over the argument block
// (hicom_compressor_batch_args / _ragged_args / _multiguide_args name every common field alike; the item count is B or Q: seg_items) and
// read `a->field` directly; `who` is the message prefix ("compressor_batch" / "compressor_ragged" / "compressor_multiguide").
#pragma once
#include "segment_item.hpp"

namespace hicom_host {

// compute units of the current device (the work division of the segmented stream fills the chip twice over)
inline int num_cus() {
    static int n = 0;
    if (n == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) n = v;
        else n = 256;
    }
    return n;
}

constexpr int kSegMaxItems = 4096;       // items per call (grid y of the merge kernels, far below the limit)
constexpr int kSegMaxChunks = 64;        // workgroups per item of the segmented stream

// ---- k / v adaptors of the local stage, shared by the two many-item steps (NULL: the plain recipe) ------------------------------------
struct SegAdapt {
    const hicom_seg_adaptor* ak;
    const hicom_seg_adaptor* av;
    int alpha_dt;
    float eps;
    bool k() const { return ak->w0 != nullptr; }
    bool v() const { return av->w0 != nullptr; }
};

// workspace regions behind the plain layout: fp16 [tokens, E] each, absent (0) for a stream without adaptor
struct SegAdaptLayout { long hid_k = 0, hid_v = 0, ky = 0, vy = 0; };

template <class Take>
inline SegAdaptLayout seg_adapt_layout(const SegAdapt* ad, long tokens, long E, Take&& take) {
    SegAdaptLayout l;
    if (!ad) return l;
    if (ad->k()) l.hid_k = take(tokens * E * 2);
    if (ad->v()) l.hid_v = take(tokens * E * 2);
    if (ad->k()) l.ky = take(tokens * E * 2);
    if (ad->v()) l.vy = take(tokens * E * 2);
    return l;
}

inline int seg_adapt_check(const char* who, const SegAdapt* ad, long tokens, int E) {
    if (!ad) return HICOM_OK;
    HICOM_REQUIRE(ad->k() || ad->v(), HICOM_EINVAL, "%s: neither stream has an adaptor (the plain entry point runs that recipe)", who);
    HICOM_REQUIRE(E % 64 == 0, HICOM_EUNSUP, "%s: adaptor width %d (multiple of 64)", who, E);
    HICOM_REQUIRE(tokens * E < (1L << 32), HICOM_EUNSUP, "%s: %ld tokens: the adaptor GEMMs take operands below 2^32 elements", who, tokens);
    HICOM_REQUIRE(ad->alpha_dt == HICOM_DT_BF16 || ad->alpha_dt == HICOM_DT_F32, HICOM_EINVAL, "%s: alpha dtype %d (bf16 | f32)", who, ad->alpha_dt);
    return HICOM_OK;
}

inline int seg_adapt_check_weights(const char* who, const SegAdapt* ad) {
    if (!ad) return HICOM_OK;
    for (const hicom_seg_adaptor* s : {ad->ak, ad->av})
        if (s->w0) HICOM_REQUIRE(s->w2_f16 && s->gamma && s->beta && s->alpha, HICOM_EINVAL, "%s: adaptor weights", who);
    return HICOM_OK;
}

// y = MLP(x) of the adapted streams over all `tokens` of the call: two launches.  Both adaptors with matching biases: each layer of the
// two MLPs is one paired launch; otherwise (one adaptor: two launches as well) the single-problem entry point per layer.
// hid_k / hid_v: the fp16 hidden planes of layer 1 (temporaries), ky / vy: the fp16 y planes; those of a stream without adaptor are not read.
inline int seg_adapt_mlps(const SegAdapt& ad, const void* key_x, const void* ff, long tokens, int E, void* hid_k, void* hid_v, void* ky, void* vy, void* stream) {
    const hicom_seg_adaptor &k = *ad.ak, &v = *ad.av;
    const int M = (int)tokens;
    if (ad.k() && ad.v() && !k.b0 == !v.b0 && !k.b2 == !v.b2) {
        const int st = hicom_dense16_gemm_pair_fwd(key_x, k.w0, k.b0, hid_k, nullptr, ff, v.w0, v.b0, hid_v, nullptr, E, E, HICOM_DT_BF16,
                                                   HICOM_DT_BF16, M, E, E, HICOM_ACT_GELU, E, E, 0, stream);
        if (st != HICOM_OK) return st;
        return hicom_dense16_gemm_pair_fwd(hid_k, k.w2_f16, k.b2, ky, nullptr, hid_v, v.w2_f16, v.b2, vy, nullptr, E, E,
                                           HICOM_DT_F16, HICOM_DT_BF16, M, E, E, HICOM_ACT_NONE, E, E, 0, stream);
    }
    auto mlp = [&](const hicom_seg_adaptor& a, const void* x, void* hid, void* y) -> int {
        const int st = hicom_dense16_gemm_fwd(x, E, a.w0, E, HICOM_DT_BF16, a.b0, HICOM_DT_BF16, M, E, E, HICOM_ACT_GELU, hid, E, E, nullptr, 0, nullptr,
                                              0, 0, nullptr, 0, nullptr, nullptr, 0, 0, 0, 0, 0, 0, nullptr, 0, nullptr, stream);
        if (st != HICOM_OK) return st;
        return hicom_dense16_gemm_fwd(hid, E, a.w2_f16, E, HICOM_DT_F16, a.b2, HICOM_DT_BF16, M, E, E, HICOM_ACT_NONE, y, E, E, nullptr, 0, nullptr,
                                      0, 0, nullptr, 0, nullptr, nullptr, 0, 0, 0, 0, 0, 0, nullptr, 0, nullptr, stream);
    };
    if (ad.k()) { const int st = mlp(k, key_x, hid_k, ky); if (st != HICOM_OK) return st; }
    if (ad.v()) { const int st = mlp(v, ff, hid_v, vy); if (st != HICOM_OK) return st; }
    return HICOM_OK;
}

inline hicom::SegAdaptParams seg_adapt_params(const SegAdapt& ad, const char* ws, const SegAdaptLayout& l) {
    hicom::SegAdaptParams p;
    p.ky = ad.k() ? (const _Float16*)(ws + l.ky) : nullptr;
    p.kgamma = (const uint16_t*)ad.ak->gamma; p.kbeta = (const uint16_t*)ad.ak->beta; p.kalpha = ad.ak->alpha;
    p.vy = ad.v() ? (const _Float16*)(ws + l.vy) : nullptr;
    p.vgamma = (const uint16_t*)ad.av->gamma; p.vbeta = (const uint16_t*)ad.av->beta; p.valpha = ad.av->alpha;
    p.alpha_f32 = ad.alpha_dt == HICOM_DT_F32;
    p.eps = ad.eps;
    return p;
}

// the entry points of the adaptor recipe (hicom_compressor_{batch,ragged}_adapt_*): f(plain block, adaptors) of an adaptor-recipe block
template <class AdaptArgs, class F>
inline auto seg_with_adapt(const char* who, const AdaptArgs* a, F&& f) -> decltype(f(&a->base, (const SegAdapt*)nullptr)) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "%s: NULL arguments", who);
    const SegAdapt ad{&a->ak, &a->av, a->alpha_dt, a->eps};
    return f(&a->base, &ad);
}

// multi_guide.hip: every argument check of hicom_clip_adapt_prepare_fwd and of hicom_multi_guide_local_adapt_fwd without their launches, for a
// host call that runs several entry points and checks all of them in front of its first launch (clip_stream.hip).  hid_v_out (may be NULL):
// where the value stream's hidden plane begins in the workspace.
int clip_adapt_prepare_args_check(const void* key_x, const void* ff, long N, int E, const hicom_seg_adaptor* ak, const hicom_seg_adaptor* av, const void* ky,
                                  const void* vy, const void* ws, long ws_bytes, long* hid_v_out);
int multi_guide_local_adapt_args_check(const void* key, const void* value, const void* guide, const void* ky, const void* vy, const hicom_seg_adaptor* ak,
                                       const hicom_seg_adaptor* av, int alpha_dt, int Q, int T, int H, int W, int E, int kt, int ks, const void* ctx_f16);

// items of the call: B of a batch / ragged block, Q (guides) of a multi-guide block
template <class A>
inline auto seg_items(const A* a) -> decltype(a->B) { return a->B; }
template <class A>
inline auto seg_items(const A* a) -> decltype(a->Q) { return a->Q; }

// ---- checks the steps make ----------------------------------------------------------------------------------------------------------------
// LDS of the merge kernels: T (H + W) marginal sums and the T + H + W marginals of the longest item
inline long seg_merge_smem(long T, long H, long W) { return (T * H + T * W + T + H + W) * 4; }

// behind the caller's own "bad shape" check (items, H, W, hidden, ks > 0) and its limit on the item count; `item`: what the step calls one
template <class A>
inline int seg_check_shape(const char* who, const char* item, const A* a) {
    HICOM_REQUIRE(a->E == 1152, HICOM_EUNSUP, "%s: E=%d (only 1152)", who, a->E);
    HICOM_REQUIRE(a->nh > 0 && a->nh <= 16 && a->E % a->nh == 0, HICOM_EUNSUP, "%s: %d heads (<= 16 folded rows per %s)", who, a->nh, item);
    HICOM_REQUIRE(a->hidden % 64 == 0, HICOM_EUNSUP, "%s: hidden=%d (multiple of 64: fp16 readout planes)", who, a->hidden);
    HICOM_REQUIRE(a->out_dt == HICOM_DT_BF16 || a->out_dt == HICOM_DT_F32, HICOM_EUNSUP, "%s: output dtype %d (bf16 | f32)", who, a->out_dt);
    HICOM_REQUIRE(!a->pe == !a->kpe && (!a->pe || a->P > 0), HICOM_EINVAL, "%s: pe and kpe come together", who);
    return HICOM_OK;
}

// batch / ragged: the item count, then seg_check_shape
template <class A>
inline int seg_check_items_shape(const char* who, const A* a) {
    HICOM_REQUIRE(a->B <= kSegMaxItems, HICOM_EUNSUP, "%s: B=%d items (<= %d per call)", who, a->B, kSegMaxItems);
    return seg_check_shape(who, "item", a);
}

// T: the longest item's frames
template <class A>
inline int seg_check_merge_lds(const char* who, const A* a, int T) {
    HICOM_REQUIRE(seg_merge_smem(T, a->H, a->W) <= 48 * 1024, HICOM_EUNSUP, "%s: T=%d frames of %dx%d: the merge keeps T (H + W) marginal sums in LDS", who,
                  T, a->H, a->W);
    return HICOM_OK;
}

template <class A>
inline int seg_check_ws(const char* who, const A* a, long total) {
    HICOM_REQUIRE(a->ws && a->ws_bytes >= total && (uintptr_t)a->ws % 256 == 0, HICOM_EINVAL, "%s: workspace of %ld bytes, 256-byte aligned", who, total);
    return HICOM_OK;
}

// what a *_fwd call checks on top of its shape checks, in front of the first launch; tokens_elsewhere: the step finds its tokens through a
// table of its own (ragged_multi_guide.hip: the clips step), ff / fe are not looked at
template <class A>
inline int seg_check_fwd(const char* who, const A* a, const SegAdapt* ad, long ws_total, bool tokens_elsewhere = false) {
    HICOM_REQUIRE((a->ff || tokens_elsewhere) && a->guide && a->out, HICOM_EINVAL, "%s: NULL pointer", who);
    HICOM_REQUIRE(a->lw0_f16 && a->lw2_f16 && a->wq && a->wk && a->wv && a->wo && a->gw0 && a->gw2, HICOM_EINVAL, "%s: NULL weight", who);
    int st = seg_adapt_check_weights(who, ad);
    if (st != HICOM_OK) return st;
    st = seg_check_ws(who, a, ws_total);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE((tokens_elsewhere || ((uintptr_t)a->ff % 16 == 0 && (!a->fe || (uintptr_t)a->fe % 16 == 0))) && (uintptr_t)a->guide % 16 == 0, HICOM_EINVAL,
                  "%s: 16-byte aligned inputs", who);
    return HICOM_OK;
}

// the packed-row layout of a step whose items share one shape (batch, multi-guide), in front of the first launch; wpi: windows per item
template <class A>
inline int seg_check_equal_rows(const char* who, const A* a, int wpi) {
    const long item_local = (long)wpi + (a->nl_group ? wpi / a->nl_group : 0);
    HICOM_REQUIRE(a->n_global_rows > 0 && a->global_row0 >= item_local && a->item_rows == a->global_row0 + a->n_global_rows && a->ldo >= a->hidden &&
                      a->nl_group >= 0 && (!a->nl_group || wpi % a->nl_group == 0),
                  HICOM_EINVAL, "%s: output layout", who);
    HICOM_REQUIRE(a->nl_count == 0 || (a->newline && a->nl_step > 0 && a->nl_first >= 0 &&
                                       a->nl_first + (long)(a->nl_count - 1) * a->nl_step < a->global_row0),
                  HICOM_EINVAL, "%s: newline rows", who);
    // every local row of an item is a token row or a newline row
    HICOM_REQUIRE(a->global_row0 == (long)wpi + a->nl_count, HICOM_EINVAL, "%s: %ld local rows for %d tokens + %d newline rows", who, (long)a->global_row0,
                  wpi, a->nl_count);
    return HICOM_OK;
}

// ---- the ragged item walk, shared by the two steps whose items come as hicom_ragged_item (ragged.hip, ragged_multi_guide.hip) ----------------
inline long item_windows(const hicom_ragged_item& it, int wps) { return (long)(it.T / it.kt) * wps; }

// tile `c` of `chunks` equal shares of an item's `ntiles` tiles: chunk c walks [seg_tile_at(c), seg_tile_at(c + 1))
inline int seg_tile_at(long ntiles, int c, int chunks) { return (int)(ntiles * c / chunks); }

// token chunks of an item with `ntiles` tiles: its share of 2 #CUs work units by `work` (ragged: tiles, work_sum the call's tile total;
// multi-guide: tiles x passes), rounded to nearest -- a function of ntiles, work_sum and #CUs only: permuting the items permutes the
// division; `chunks` > 0 overrides the share
inline int seg_share_chunks(long ntiles, long work_sum, int chunks, int ncu) {
    long c = chunks > 0 ? chunks : (2L * ncu * ntiles + work_sum / 2) / work_sum;
    if (c > ntiles) c = ntiles;
    if (c > kSegMaxChunks) c = kSegMaxChunks;
    return (int)(c < 1 ? 1 : c);
}

// the per-item requirements, item by item; first(i) runs in front of item i's (the step's own requirement on the item: its status, not
// HICOM_OK, ends the walk).  Adds up the call's tokens and finds the longest item's frames.
template <class A, class First>
inline int seg_check_ragged_items(const char* who, const A* a, long& tokens, int& max_T, First&& first) {
    const int wps = (a->H / a->ks) * (a->W / a->ks);
    tokens = 0;
    max_T = 0;
    for (int i = 0; i < a->B; ++i) {
        const int st = first(i);
        if (st != HICOM_OK) return st;
        const hicom_ragged_item& it = a->items[i];
        HICOM_REQUIRE(it.T > 0 && it.kt > 0 && it.n_global_rows > 0 && it.nl_group >= 0 && it.nl_count >= 0, HICOM_EINVAL, "%s: item %d: bad shape", who, i);
        HICOM_REQUIRE(it.T % it.kt == 0, HICOM_EUNSUP, "%s: item %d needs an exact window partition (T=%d, temporal window %d)", who, i, it.T, it.kt);
        HICOM_REQUIRE(it.kt * a->ks * a->ks <= 64, HICOM_EUNSUP, "%s: item %d: windows of %d tokens (<= 64)", who, i, it.kt * a->ks * a->ks);
        const long N = (long)it.T * a->H * a->W;
        HICOM_REQUIRE(N < (1L << 27), HICOM_EUNSUP, "%s: item %d: too many tokens", who, i);
        const long w = item_windows(it, wps);
        HICOM_REQUIRE(!it.nl_group || w % it.nl_group == 0, HICOM_EINVAL, "%s: item %d: output layout", who, i);
        HICOM_REQUIRE(it.nl_count == 0 || (it.nl_step > 0 && it.nl_first >= 0 && it.nl_first + (long)(it.nl_count - 1) * it.nl_step < w + it.nl_count),
                      HICOM_EINVAL, "%s: item %d: newline rows", who, i);
        tokens += N;
        if (it.T > max_T) max_T = it.T;
    }
    return HICOM_OK;
}

// the table region, derived on the host, to the head of the workspace (synchronises the stream)
template <class A>
inline int seg_upload_tables(const char* who, const A* a, const void* tab, long bytes) {
    hipStream_t s = (hipStream_t)a->stream;
    if (hipMemcpyAsync(a->ws, tab, (size_t)bytes, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        set_error("%s: writing the table region: %s", who, hipGetErrorString(hipGetLastError()));
        return HICOM_ELAUNCH;
    }
    return HICOM_OK;
}

// ---- workspace: the regions of the step from the call's totals, the adaptor planes behind them ----------------------------------------------
struct SegTotals {
    long score_floats;      // what the stream leaves for the merge: 16 rows of logits per item, the item's tokens padded to a tile (multi-guide:
                            // the larger of its logits and its in-kernel marginals)
    long slots;             // workgroups of the segmented stream (multi-guide: token chunks of the many-row stream)
    long windows, tokens;   // over all items
    long rows;              // folded query rows: heads x items (multi-guide: rounded up to a pass of the many-row stream)
    long part_rows;         // rows of partial state (m, l, ACC): 16 per slot (multi-guide: `rows` per chunk)
    long scratch_floats;    // scratch of the many-row merge, with its (M, L) per row behind it; 0: the segmented merge needs neither
};

struct SegLayout {
    long qp, qhi, qlo, pos_a, scores, part_m, part_l, part_acc, scratch, ml, ctxg, o, pre, hid, tok, ctx16, hid16, loc, total;
    SegAdaptLayout ad;      // behind the plain layout, whose offsets and total do not depend on it
    SegTotals n;
};

// off: bytes in front of the first region (the ragged step's tables), a multiple of 256.  Every region is rounded up to 256 bytes on its own:
// an absent (zero-byte) region moves nothing.
template <class A>
inline SegLayout seg_layout(const A* a, const SegAdapt* ad, const SegTotals& n, long off) {
    SegLayout l;
    auto take = [&](long bytes) { const long at = off; off += (bytes + 255) / 256 * 256; return at; };
    const long B = seg_items(a), E = a->E, R = n.rows, hidden = a->hidden;
    const int odt = a->out_dt == HICOM_DT_F32 ? 4 : 2;
    l.n = n;
    l.qp = take(B * E * 4);
    l.qhi = take(R * E * 2);
    l.qlo = take(R * E * 2);
    l.pos_a = take(R * (long)(a->P > 0 ? a->P : 1) * 4);
    l.scores = take(n.score_floats * 4);
    l.part_m = take(n.part_rows * 4);
    l.part_l = take(n.part_rows * 4);
    l.part_acc = take(n.part_rows * E * 4);
    l.scratch = take(n.scratch_floats * 4);
    l.ml = take(n.scratch_floats ? R * 2 * 4 : 0);
    l.ctxg = take(R * E * 4);
    l.o = take(B * E * 4);
    l.pre = take(B * E * 4);
    l.hid = take(B * hidden * 4);
    l.tok = take(B * hidden * 4);
    l.ctx16 = take(n.windows * E * 2);
    l.hid16 = take(n.windows * hidden * 2);
    l.loc = take(n.windows * hidden * odt);
    l.ad = seg_adapt_layout(ad, n.tokens, E, take);
    l.total = off;
    return l;
}

inline int seg_check_launch(const char* who, const char* stage) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return HICOM_OK;
    set_error("%s: %s: %s", who, stage, hipGetErrorString(e));
    return HICOM_ELAUNCH;
}

// placement of a step whose items share one packed-row layout: `kernel` is the caller's one-line wrapper of place_equal_row
template <class A>
inline int seg_place_equal(const char* who, void (*kernel)(hicom::EqualPlaceParams), const A* a, const hicom::SegPlaceParams& c, int wpi) {
    hicom::EqualPlaceParams p;
    p.c = c;
    p.wpi = wpi; p.nl_group = a->nl_group; p.nl_count = a->nl_count;
    p.item_rows = a->item_rows; p.global_row0 = a->global_row0; p.nl_first = a->nl_first; p.nl_step = a->nl_step > 0 ? a->nl_step : 1; p.ldo = a->ldo;
    HICOM_LAUNCH(kernel, dim3((unsigned)((long)seg_items(a) * a->item_rows)), dim3(128), 0, (hipStream_t)a->stream, p);
    return seg_check_launch(who, "placement");
}

// ---- the step: twelve launches, fourteen with adaptors (multi-guide: thirteen or fourteen, its merge being two or three) ------------------
// `item` launches what knows where an item lives, each hook on the common part of its parameter block (which a hook may ignore), and
// returns the status of its launches (seg_check_launch, or that of the entry point it called):
//   item.local(key_x, adapt)   3: local stage into ws + l.ctx16; adapt: the fused blends' parameters, NULL for the plain recipe
//   item.stream(c)             4: global stream
//   item.merge(c)              5: merge per (item, head) into ws + l.ctxg
//   item.place(c)             12: every item's packed rows
// Everything else is the same call for the three steps, with M = items or M = all windows.  Only launches: nothing here allocates, copies
// or synchronises.
template <class A, class Item>
inline int seg_step(const A* a, const SegAdapt* ad, const SegLayout& l, const Item& item) {
    char* ws = (char*)a->ws;
    const int B = seg_items(a), E = a->E, nh = a->nh, hd = E / nh, hidden = a->hidden, windows = (int)l.n.windows;
    float* qp = (float*)(ws + l.qp);
    float* pos_a = a->pe ? (float*)(ws + l.pos_a) : nullptr;
    float* ctxg = (float*)(ws + l.ctxg);
    float *o = (float*)(ws + l.o), *pre = (float*)(ws + l.pre), *hid = (float*)(ws + l.hid), *tok = (float*)(ws + l.tok);

    // 1-2: queries per item
    int st = hicom_linear_fwd(a->guide, HICOM_DT_BF16, a->wq, HICOM_DT_BF16, a->bq, HICOM_DT_BF16, nullptr, 0, B, E, E, 0, 0, HICOM_ACT_NONE, qp, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_fold_query_split_fwd(qp, a->wk, a->kpe, B, nh, E, a->P, 1.0f / sqrtf((float)hd), ws + l.qhi, ws + l.qlo, pos_a, a->P, nullptr, 0, 0,
                                    a->stream);
    if (st != HICOM_OK) return st;

    // 3: local stage (adaptor recipe: the two layers of the adaptor MLPs over all tokens in front of it)
    {
        const uint16_t* key_x = (const uint16_t*)(a->fe ? a->fe : a->ff);
        if (ad) {
            st = seg_adapt_mlps(*ad, key_x, a->ff, l.n.tokens, E, ws + l.ad.hid_k, ws + l.ad.hid_v, ws + l.ad.ky, ws + l.ad.vy, a->stream);
            if (st != HICOM_OK) return st;
            const hicom::SegAdaptParams p = seg_adapt_params(*ad, ws, l.ad);
            st = item.local(key_x, &p);
        } else {
            st = item.local(key_x, nullptr);
        }
        if (st != HICOM_OK) return st;
    }

    // 4: global stream
    {
        hicom::SegStreamParams c;
        c.qhi = (const uint16_t*)(ws + l.qhi); c.qlo = (const uint16_t*)(ws + l.qlo);
        c.pos_a = pos_a; c.pos_stride = a->P; c.rows = nh;
        c.H = a->H; c.W = a->W; c.HW = a->H * a->W;
        c.t0i = a->t_index0; c.y0i = a->y_index0; c.x0i = a->x_index0;
        c.part_m = (float*)(ws + l.part_m); c.part_l = (float*)(ws + l.part_l); c.part_acc = (float*)(ws + l.part_acc);
        st = item.stream(c);
        if (st != HICOM_OK) return st;
    }

    // 5: merge per item
    {
        hicom::SegMergeParams c;
        c.part_m = (const float*)(ws + l.part_m); c.part_l = (const float*)(ws + l.part_l); c.part_acc = (const float*)(ws + l.part_acc);
        c.pe = a->pe; c.E = E; c.H = a->H; c.W = a->W;
        c.t0i = a->t_index0; c.y0i = a->y_index0; c.x0i = a->x_index0;
        st = item.merge(c);
        if (st != HICOM_OK) return st;
    }

    // 6-9: the global tail with M = items rows
    st = hicom_linear_fwd(ctxg, HICOM_DT_F32, a->wv, HICOM_DT_BF16, a->bv, HICOM_DT_BF16, nullptr, 0, B, E, E, nh, hd, HICOM_ACT_NONE, o, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_linear_fwd(o, HICOM_DT_F32, a->wo, HICOM_DT_BF16, a->bo, HICOM_DT_BF16, a->guide, 2, B, E, E, 0, 0, HICOM_ACT_NONE, pre, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_linear_fwd(pre, HICOM_DT_F32, a->gw0, HICOM_DT_BF16, a->gb0, HICOM_DT_BF16, nullptr, 0, B, hidden, E, 0, 0, HICOM_ACT_GELU, hid, a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_linear_fwd(hid, HICOM_DT_F32, a->gw2, HICOM_DT_BF16, a->gb2, HICOM_DT_BF16, nullptr, 0, B, hidden, hidden, 0, 0, HICOM_ACT_NONE, tok, a->stream);
    if (st != HICOM_OK) return st;

    // 10-11: the local readout as one GEMM pair over all items' windows
    st = hicom_readout16_gemm_fwd(ws + l.ctx16, a->lw0_f16, a->lb0, HICOM_DT_BF16, windows, hidden, E, HICOM_ACT_GELU, ws + l.hid16, nullptr, 0, 0, 0, 0, nullptr,
                                  a->stream);
    if (st != HICOM_OK) return st;
    st = hicom_readout16_gemm_fwd(ws + l.hid16, a->lw2_f16, a->lb2, HICOM_DT_BF16, windows, hidden, hidden, HICOM_ACT_NONE, nullptr, ws + l.loc, a->out_dt, hidden,
                                  0, 0, nullptr, a->stream);
    if (st != HICOM_OK) return st;

    // 12: every item's packed rows
    hicom::SegPlaceParams c;
    c.loc = ws + l.loc; c.tok = tok; c.newline = (const uint16_t*)a->newline; c.out = a->out;
    c.out_f32 = a->out_dt == HICOM_DT_F32; c.hidden = hidden;
    return item.place(c);
}

}  // namespace hicom_host
