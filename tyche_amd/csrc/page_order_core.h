// page_order_core.h -- the page order of the lane-per-page launches (DESIGN.md
// 3.1): which page a lane decodes in which generation.  Shared verbatim by the
// gfx950 ordering pass (page_order.hip), by the decoder that walks the order
// (lz4_decode_lc.hip) and by the host emulator tools/page_order_emul.cpp.
//
// A lane-per-page kernel of `grid` one-wave workgroups gives every lane one page
// per generation: G = grid * 64 pages in flight, generation k the k-th G pages it
// takes.  A wave runs until its slowest lane is done, and a page's cost follows
// its stream length, so the pages are handed out by length:
//
//   bin    min(length, in_cap) >> shift, the smallest shift that leaves fewer
//          than kBins values: 256 to 511 bins over [0, in_cap].  (A page the
//          decoder answers without decoding costs nothing wherever it lands.)
//   order  the pages of every window of `window` consecutive pages (0: the whole
//          batch is one window) sorted by descending bin, equal bins in page
//          order: order[] is a permutation of [0, count) whose entries
//          [w * window, (w + 1) * window) are window w's pages.
//   slot   lane position t = wave * 64 + lane takes order[k * G + t] in an even
//          generation k and order[k * G + (G - 1 - t)] in an odd one.  A wave's 64
//          lanes hold 64 neighbours of the order in every generation, so the pages
//          decoded side by side are alike; a position that gets the longer pages
//          of one generation (or, with windows, of its window) gets the shorter
//          ones of the next, which evens out the sums of lanes and of waves; the
//          order's tail -- under the whole-batch order the shortest pages -- is
//          the partial last generation.
//
// The ordering pass is a counting sort over tiles of kTile pages that never
// straddle a window: a histogram per tile, one scan per window (bins outside,
// tiles inside), a scatter with the tile's own ranks.
//
// The includer defines PO_HOST (1: plain C++, the emulator; 0: hipcc).
#pragma once
#include <stdint.h>

#if PO_HOST
#define PO_FN static inline
#else
#define PO_FN __host__ __device__ __forceinline__
#endif

namespace po {

constexpr uint32_t kBins = 512;
constexpr uint32_t kTile = 2048;   // pages per tile: one wave, kTile / 64 steps
constexpr uint32_t kLanes = 64;

PO_FN uint32_t bin_shift(uint32_t in_cap) {
    uint32_t s = 0;
    while ((in_cap >> s) >= kBins) s++;
    return s;
}
PO_FN uint32_t bin_of(uint32_t length, uint32_t in_cap, uint32_t shift) { return (length < in_cap ? length : in_cap) >> shift; }
// the counting sort's key: 0 for the highest bin
PO_FN uint32_t rank_key(uint32_t length, uint32_t in_cap, uint32_t shift) { return kBins - 1u - bin_of(length, in_cap, shift); }

// windows and tiles of a batch of count pages (0 < count < 2^32)
struct Geo {
    uint32_t count;
    uint32_t win;      // pages per window (the last may hold fewer)
    uint32_t nwin;
    uint32_t tpw;      // tiles per window
    uint32_t ntiles;   // nwin * tpw (tiles past a short last window's end are empty)
};
PO_FN Geo geometry(uint32_t count, uint32_t window) {
    Geo g;
    g.count = count;
    g.win = window == 0 || window > count ? count : window;
    g.nwin = (uint32_t)(((uint64_t)count + g.win - 1u) / g.win);
    g.tpw = (uint32_t)(((uint64_t)g.win + kTile - 1u) / kTile);
    g.ntiles = g.nwin * g.tpw;
    return g;
}
// whether the pass's tables stay small: tiles * kBins counters
PO_FN bool geometry_ok(uint32_t count, uint32_t window) {
    const uint32_t win = window == 0 || window > count ? count : window;
    const uint64_t nwin = ((uint64_t)count + win - 1u) / win, tpw = ((uint64_t)win + kTile - 1u) / kTile;
    return nwin * tpw <= (1u << 20);
}
PO_FN uint32_t window_first(const Geo &g, uint32_t w) { return (uint32_t)((uint64_t)w * g.win); }
// pages [*first, *end) of tile t
PO_FN void tile_bounds(const Geo &g, uint32_t t, uint32_t *first, uint32_t *end) {
    const uint32_t w = t / g.tpw, j = t % g.tpw;
    const uint64_t w0 = (uint64_t)w * g.win;
    uint64_t w1 = w0 + g.win;
    if (w1 > g.count) w1 = g.count;
    uint64_t a = w0 + (uint64_t)j * kTile, b = a + kTile;
    if (a > w1) a = w1;
    if (b > w1) b = w1;
    *first = (uint32_t)a;
    *end = (uint32_t)b;
}

// The slot of lane `lane` of wave `wave` (of `grid`) in generation k: an index into order[], or a
// value >= count when the lane has no page in that generation (only in a partial last generation:
// every later generation's slot is larger still).  A bijection from the (k, wave, lane) with a slot
// below count onto [0, count).
PO_FN uint64_t slot(uint64_t k, uint32_t wave, uint32_t lane, uint32_t grid, uint64_t count) {
    const uint64_t G = (uint64_t)grid * kLanes, t = (uint64_t)wave * kLanes + lane;
    const uint64_t s = k * G + ((k & 1u) ? G - 1u - t : t);
    return s < count ? s : count;
}
PO_FN uint64_t generations(uint32_t grid, uint64_t count) {
    const uint64_t G = (uint64_t)grid * kLanes;
    return (count + G - 1u) / G;
}

}  // namespace po
