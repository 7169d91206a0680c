// What the ragged multi-guide step's forward (ragged_multi_guide.hip) and its training surface (ragged_multi_guide_train.hip) share: the
// entries of the table region (item, pair, work unit), and on the host the step's limits, its shape checks and the workspace layout with
// the table region at its head.
#pragma once
#include <vector>

#include "multi_window.hpp"
#include "segment_host.hpp"

namespace hicom {

struct RmgItem {         // 16 ints; mirrored by hicom_amd/ragged_multi_guide.py: table_image
    int tok0, N;         // first token in the stack, tokens
    int T, kt;
    int win0;            // first window in the stacked tensor's window list
    int slot0, chunks;   // first partial-state slot; token chunks per pass (slots: passes x 2 x chunks)
    int score_off;       // its logits: scores + 16 * score_off, [32 passes_i][ceil16(N)]
    int pair0, Q;        // first pair, guides
    int ctx_row0;        // first context row of its first pair (pair q: + q windows_i)
    int global_row0;     // rows of a pair in front of its global rows
    int nl_group, nl_count, nl_first, nl_step;
};
static_assert(sizeof(RmgItem) == 64, "item table entries are 16 ints");

struct RmgPair {         // 4 ints
    int item, q;
    int ctx_row0;        // first row of its window contexts (and of its readout rows)
    int row0;            // first output row
};

struct RmgUnit {         // 8 ints
    int item, tb, te;    // tiles [tb, te) of the item, counted from its first token
    int pass;            // rows [32 pass, 32 pass + 32) of the item's row space
    int slot;            // partial-state slot of row group 0; row group 1: + the item's chunks
    int pad0, pad1, pad2;
};
static_assert(sizeof(RmgUnit) == 32, "work units are 8 ints");

}  // namespace hicom

namespace hicom_host {

using hicom::RmgItem;
using hicom::RmgPair;
using hicom::RmgUnit;

constexpr const char* kWho = "compressor_ragged_multiguide";
constexpr int kMaxGuides = 32;              // per item, as in the multi-guide step
constexpr int kPassRows = 32;               // folded rows of one pass of the stream

typedef hicom_compressor_ragged_multiguide_args Args;

inline long item_passes(const Args* a, int i) { return ((long)a->nh * a->guide_counts[i] + kPassRows - 1) / kPassRows; }

struct RmgLayout {
    long items, units, win_item, pairs, row_pair, table_bytes;      // the table region, in front of the step's own regions
    SegLayout s;
    long rows, item_windows, nunits, work_sum;
    int M, max_T, wps;
};

inline RmgLayout rmg_layout(const Args* a) {
    RmgLayout l{};
    SegTotals n{};
    const long HW = (long)a->H * a->W;
    l.wps = (a->H / a->ks) * (a->W / a->ks);
    for (int i = 0; i < a->B; ++i) {
        const hicom_ragged_item& it = a->items[i];
        const long N = it.T * HW, w = item_windows(it, l.wps), Q = a->guide_counts[i], ntiles = (N + 15) / 16;
        n.tokens += N;
        l.item_windows += w;
        n.windows += Q * w;
        l.rows += Q * (w + it.nl_count + it.n_global_rows);
        n.score_floats += item_passes(a, i) * kPassRows * ntiles * 16;
        l.work_sum += ntiles * item_passes(a, i);
        l.M += (int)Q;
        if (it.T > l.max_T) l.max_T = it.T;
    }
    const int ncu = a->chunks > 0 ? 0 : num_cus();
    for (int i = 0; i < a->B; ++i) {
        const long c = seg_share_chunks((a->items[i].T * HW + 15) / 16, l.work_sum, a->chunks, ncu);
        l.nunits += c * item_passes(a, i);
    }
    n.slots = 2 * l.nunits;
    n.rows = (long)l.M * a->nh;
    n.part_rows = n.slots * 16;
    long off = 0;
    auto take = [&](long bytes) { const long at = off; off += (bytes + 255) / 256 * 256; return at; };
    l.items = take(a->B * (long)sizeof(RmgItem));
    l.units = take(l.nunits * (long)sizeof(RmgUnit));
    l.win_item = take(l.item_windows * 4);
    l.pairs = take(l.M * (long)sizeof(RmgPair));
    l.row_pair = take(l.rows * 4);
    l.table_bytes = off;
    Args pairs = *a;            // the shared host sees the pairs as its items
    pairs.B = l.M;
    l.s = seg_layout(&pairs, nullptr, n, off);
    return l;
}

inline int rmg_check(const Args* a) {
    HICOM_REQUIRE(a, HICOM_EINVAL, "compressor_ragged_multiguide: NULL arguments");
    HICOM_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0 && a->hidden > 0 && a->ks > 0 && a->items && a->guide_counts, HICOM_EINVAL,
                  "compressor_ragged_multiguide: bad shape");
    HICOM_REQUIRE(a->n_guide_counts == a->B, HICOM_EINVAL, "compressor_ragged_multiguide: %d guide counts for %d items (one per item)", a->n_guide_counts, a->B);
    int st = seg_check_items_shape(kWho, a);
    if (st != HICOM_OK) return st;
    HICOM_REQUIRE(a->H % a->ks == 0 && a->W % a->ks == 0, HICOM_EUNSUP,
                  "compressor_ragged_multiguide: needs an exact window partition (H=%d W=%d, windows %dx%d)", a->H, a->W, a->ks, a->ks);
    long tokens;
    int max_T;
    st = seg_check_ragged_items(kWho, a, tokens, max_T, [a](int i) -> int {        // item i's guide count in front of its shape
        const int Q = a->guide_counts[i];
        HICOM_REQUIRE(Q >= 1 && Q <= kMaxGuides, HICOM_EUNSUP, "compressor_ragged_multiguide: item %d: Q=%d guides (1 <= Q <= %d per item)", i, Q, kMaxGuides);
        return HICOM_OK;
    });
    if (st != HICOM_OK) return st;
    const int wps = (a->H / a->ks) * (a->W / a->ks);
    long pairs = 0, products = 0, ctx_rows = 0;
    for (int i = 0; i < a->B; ++i) {
        const long Q = a->guide_counts[i], N = (long)a->items[i].T * a->H * a->W;
        pairs += Q;
        products += Q * ((N + 15) / 16 * 16);
        ctx_rows += Q * item_windows(a->items[i], wps);
    }
    HICOM_REQUIRE(pairs <= kSegMaxItems, HICOM_EUNSUP, "compressor_ragged_multiguide: %ld (item, guide) pairs (<= %d per call)", pairs, kSegMaxItems);
    // (item offsets, the logits' offsets -- counted in 16 floats, 32 rows per pass and token -- and the context rows are ints on the device)
    HICOM_REQUIRE(tokens + 16L * a->B < (1L << 27), HICOM_EUNSUP, "compressor_ragged_multiguide: too many tokens in one call");
    HICOM_REQUIRE(products < (1L << 27), HICOM_EUNSUP, "compressor_ragged_multiguide: too many token x guide products in one call (%ld, < 2^27)", products);
    HICOM_REQUIRE(ctx_rows < (1L << 20), HICOM_EUNSUP, "compressor_ragged_multiguide: %ld window contexts over all pairs (< 2^20)", ctx_rows);
    return seg_check_merge_lds(kWho, a, max_T);
}

}  // namespace hicom_host
