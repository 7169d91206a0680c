// What the ragged step's forward (ragged.hip) and its training surface (ragged_train.hip) share: the item table's entry, the walk from a
// window or a token to its item on the device, and on the host the shape checks and the workspace layout with the table region at its head.
#pragma once
#include "segment_host.hpp"

namespace hicom {

struct RaggedItem {      // 16 ints; mirrored by hicom_amd/ragged.py: plan_tables
    int tok0, N;         // first token in the stack, tokens
    int T, kt;
    int win0;            // first window in the concatenated window list
    int slot0, chunks;   // partial-state slots = work units of this item
    int score_off;       // its logits: scores + 16 * score_off, [16][ceil16(N)]
    int row0;            // first output row
    int global_row0;     // rows of the item in front of its global rows
    int nl_group, nl_count, nl_first, nl_step;
    int pad0, pad1;
};
static_assert(sizeof(RaggedItem) == 64, "item table entries are 16 ints");

__device__ __forceinline__ hicom_axis ragged_item_axis(const RaggedItem& it) { return hicom_axis{it.T, it.kt, it.T / it.kt, it.T / it.kt}; }

// The item walk of a window of the concatenated window list: its item (the guide row), the item's record, the window's geometry from the
// item's own (T, kt), and where the item's token rows begin in a [sum N_i][D] matrix.  All wave-uniform.
struct RaggedWindow {
    int item;
    RaggedItem it;
    WindowGeom geom;
    long first;
    __device__ __forceinline__ RaggedWindow(const RaggedItem* items, const int* win_item, const hicom_axis& ay, const hicom_axis& ax, int win, int D)
        : item(win_item[win]), it(items[item]), geom(ragged_item_axis(it), ay, ax, win - it.win0), first((long)it.tok0 * D) {}
};

// ... and of a token of the stack: the last item whose first token is <= tok, by a binary search of the item table (B entries; tok0 rises
// strictly, items[0].tok0 == 0), and the token's window in the concatenated list
struct RaggedToken {
    int item;
    long win;
    __device__ __forceinline__ RaggedToken(const RaggedItem* items, int B, const hicom_axis& ay, const hicom_axis& ax, long tok) {
        int lo = 0, hi = B;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (items[mid].tok0 <= tok) lo = mid;
            else hi = mid;
        }
        const RaggedItem it = items[lo];
        item = lo;
        win = it.win0 + WindowGeom::window_of(ragged_item_axis(it), ay, ax, tok - it.tok0);
    }
};

}  // namespace hicom

namespace hicom_host {

using hicom::RaggedItem;

// the spatial axes of every item's window grid (the temporal one is the item's own: ragged_item_axis)
struct RaggedAxes { hicom_axis ay, ax; };
inline RaggedAxes ragged_axes(const hicom_compressor_ragged_args* a) {
    return {hicom_axis{a->H, a->ks, a->H / a->ks, a->H / a->ks}, hicom_axis{a->W, a->ks, a->W / a->ks, a->W / a->ks}};
}

struct RaggedLayout {
    long items, units, win_item, row_item, table_bytes;     // the table region, in front of the step's own regions
    SegLayout s;
    long rows, ntiles_sum;
    int max_T, wps;
};

// ad: the k / v adaptors of the local stage, NULL for the plain recipe (hicom_compressor_ragged_*)
inline RaggedLayout ragged_layout(const hicom_compressor_ragged_args* a, const SegAdapt* ad) {
    RaggedLayout l{};
    SegTotals n{};
    const long HW = (long)a->H * a->W;
    l.wps = (a->H / a->ks) * (a->W / a->ks);
    for (int i = 0; i < a->B; ++i) {
        const hicom_ragged_item& it = a->items[i];
        const long N = it.T * HW, w = item_windows(it, l.wps);
        n.tokens += N;
        n.windows += w;
        l.rows += w + it.nl_count + it.n_global_rows;
        n.score_floats += 16 * ((N + 15) / 16 * 16);
        l.ntiles_sum += (N + 15) / 16;
        if (it.T > l.max_T) l.max_T = it.T;
    }
    const int ncu = a->chunks > 0 ? 0 : num_cus();
    for (int i = 0; i < a->B; ++i) n.slots += seg_share_chunks((a->items[i].T * HW + 15) / 16, l.ntiles_sum, a->chunks, ncu);
    n.rows = (long)a->B * a->nh;
    n.part_rows = n.slots * 16;
    long off = 0;
    auto take = [&](long bytes) { const long at = off; off += (bytes + 255) / 256 * 256; return at; };
    l.items = take(a->B * (long)sizeof(RaggedItem));
    l.units = take(n.slots * 16);
    l.win_item = take(n.windows * 4);
    l.row_item = take(l.rows * 4);
    l.table_bytes = off;
    l.s = seg_layout(a, ad, n, off);
    return l;
}

inline int ragged_check(const hicom_compressor_ragged_args* a, const SegAdapt* ad) {
    constexpr const char* kWho = "compressor_ragged";
    HICOM_REQUIRE(a, HICOM_EINVAL, "compressor_ragged: NULL arguments");
    HICOM_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0 && a->hidden > 0 && a->ks > 0 && a->items, HICOM_EINVAL, "compressor_ragged: bad shape");
    HICOM_TRY(seg_check_items_shape(kWho, a));
    HICOM_REQUIRE(a->H % a->ks == 0 && a->W % a->ks == 0, HICOM_EUNSUP, "compressor_ragged: needs an exact window partition (H=%d W=%d, windows %dx%d)",
                  a->H, a->W, a->ks, a->ks);
    long tokens;
    int max_T;
    HICOM_TRY(seg_check_ragged_items(kWho, a, tokens, max_T, [](int) { return HICOM_OK; }));
    // (item offsets and the logits' offsets, 16 floats per token and one padded tile per item, are ints on the device)
    HICOM_REQUIRE(tokens + 16L * a->B < (1L << 27), HICOM_EUNSUP, "compressor_ragged: too many tokens in one call");
    HICOM_TRY(seg_check_merge_lds(kWho, a, max_T));
    return seg_adapt_check(kWho, ad, tokens, a->E);
}

}  // namespace hicom_host
