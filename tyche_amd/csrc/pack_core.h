// pack_core.h -- the rule of the packed compressed-page store (tyche_pack_batch,
// include/tyche_codec.h) and the geometry of its copy.  Shared verbatim by the
// gfx950 kernels (pack.hip), by tyche_pack_plan (the same rule on host arrays)
// and by the host emulator tools/pack_emul.cpp; tests/pack_cases.py restates the
// rule in numpy.
//
// The rule:
//   len_i   = results[i] if 0 < results[i] and (max_length == 0 or results[i] <= max_length), else 0
//   o_0     = round_up(state[1], align),  o_{i+1} = round_up(o_i + len_i, align)
//   end     = o_{n-1} + len_{n-1}  (not rounded)
//   stored  = state[0] == state[1] on entry and end <= capacity
//   state   = {end, end} when stored, {state[0], end} when refused
// Every o_i is a multiple of align, so o_i = o_0 + the exclusive prefix sum of
// room_i = round_up(len_i, align): the plan is a 64-bit scan of the rooms.
//
// The copy tiles the destination.  With skew = the arena address's low 7 bits,
// tile k owns the arena offsets o with (o + skew) / kTile == k, cut to
// [o_0, end): tile boundaries are 128-byte-aligned addresses, so every 16-byte
// destination line belongs to one tile.  A tile finds the last page whose offset
// is not above its first byte (first_page: rounds of 64 probes over offsets[],
// which is non-decreasing), then walks forward over the pages that start before
// its end and copies the piece of each that lies inside it (copy_tile).  A piece
// is cut at the destination's 16-byte lines (split_piece): head bytes up to the
// first line boundary, whole lines, tail bytes.  Heads and tails are written byte
// by byte, never by read-modify-write of a line.
//
// The includer defines PK_HOST (1: plain C++, the emulator; 0: hipcc).
#pragma once
#include <stdint.h>

#if PK_HOST
#define PK_FN static inline
#else
#define PK_FN __host__ __device__ __forceinline__
#endif

#ifndef TYCHE_PACK_TILE
#define TYCHE_PACK_TILE 65536   // A/B builds pass another (profiles/pack_time.log has 4 KiB .. 256 KiB)
#endif

namespace pk {

constexpr uint32_t kTile = TYCHE_PACK_TILE;   // T: destination bytes per claimed tile
constexpr uint32_t kSkewMask = 127;           // tiles start at 128-byte-aligned addresses
constexpr uint32_t kLine = 16;                // destination line: one 16-byte store
constexpr uint32_t kProbes = 64;              // probes per search round: one per lane
constexpr uint32_t kScanThreads = 256;
constexpr uint32_t kPagesPerThread = 4;
constexpr uint32_t kScanPages = kScanThreads * kPagesPerThread;   // S: pages per scan workgroup
constexpr uint32_t kFanIn = kScanThreads;     // tile sums per round of the one-workgroup scan
static_assert(kTile % 128 == 0 && kTile >= 128, "tiles are whole 128-byte lines");

PK_FN uint32_t page_len(int32_t result, uint32_t max_length) {
    return result > 0 && (max_length == 0 || (uint32_t)result <= max_length) ? (uint32_t)result : 0u;
}
PK_FN uint64_t round_up(uint64_t x, uint32_t align) { return (x + (align - 1u)) & ~(uint64_t)(align - 1u); }
PK_FN uint64_t room(int32_t result, uint32_t max_length, uint32_t align) {
    return round_up(page_len(result, max_length), align);
}
PK_FN bool align_ok(uint32_t align, uint32_t max_align) { return align != 0 && (align & (align - 1u)) == 0 && align <= max_align; }

// what one append does, decided once (the scan kernel's last step; tyche_pack_plan)
struct Plan {
    uint64_t base;         // o_0
    uint64_t end;
    uint64_t state0;       // state[0] after the call
    uint64_t first_tile;   // the tile that holds o_0
    uint32_t ntiles;       // tiles the copy claims: 0 when refused or empty
    uint32_t stored;
};

// total_room: the sum of every page's room; last_len: len_{n-1}; skew: arena address & kSkewMask
PK_FN Plan decide(uint64_t state0, uint64_t state1, uint64_t total_room, uint32_t last_len, uint32_t align,
                  uint64_t capacity, uint32_t skew) {
    Plan p;
    p.base = round_up(state1, align);
    p.end = p.base + (total_room - round_up(last_len, align)) + last_len;
    p.stored = state0 == state1 && p.end <= capacity ? 1u : 0u;
    p.state0 = p.stored ? p.end : state0;
    p.first_tile = (p.base + skew) / kTile;
    p.ntiles = p.stored && p.end > p.base ? (uint32_t)((p.end - 1u + skew) / kTile - p.first_tile + 1u) : 0u;
    return p;
}

// arena offsets [lo, hi) of tile first_tile + k
PK_FN void tile_bounds(const Plan &p, uint32_t k, uint32_t skew, uint64_t *lo, uint64_t *hi) {
    const uint64_t t = p.first_tile + k;
    const uint64_t a = t * kTile > skew ? t * kTile - skew : 0u;
    const uint64_t b = (t + 1u) * kTile - skew;
    *lo = a > p.base ? a : p.base;
    *hi = b < p.end ? b : p.end;
}

// ---- the search: how many of offsets[0 .. n) are <= lo, in rounds of kProbes probes.
// Invariant: every index below a holds, none from b on does.  Probe l of a round
// looks at index a + (l + 1) * step - 1 when that is below b; the predicate is
// monotone, so the number c of probes that hold narrows [a, b) to under `step`.
PK_FN uint32_t probe_step(uint32_t a, uint32_t b) { return (b - a + kProbes - 1u) / kProbes; }
PK_FN uint32_t probe_at(uint32_t a, uint32_t step, uint32_t l) { return a + (l + 1u) * step - 1u; }
PK_FN void narrow(uint32_t *a, uint32_t *b, uint32_t step, uint32_t c) {
    *a += c * step;
    const uint64_t nb = (uint64_t)*a + step - 1u;   // the first probe that did not hold (or beyond b)
    if (nb < *b) *b = (uint32_t)nb;
}

// the part of a piece of n bytes, whose destination address has the low bits d16 = dst & 15, before
// the first line boundary; whole lines and the tail follow from it
struct Split {
    uint32_t head, lines, tail;
};
PK_FN Split split_piece(uint32_t d16, uint32_t n) {
    Split s;
    const uint32_t to_line = (kLine - d16) & (kLine - 1u);
    s.head = n < to_line ? n : to_line;
    s.lines = (n - s.head) / kLine;
    s.tail = (n - s.head) % kLine;
    return s;
}

// Ops: probes_true(a, b, step, lo) -> c of one search round; page(i, &o, &len) reads
// offsets[i] and lengths[i]; copy(i, skip, dst, n) copies bytes [skip, skip + n) of
// page i's stream to arena offset dst.
template <class Ops>
PK_FN uint32_t first_page(Ops &ops, uint32_t n, uint64_t lo) {
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t step = probe_step(a, b);
        narrow(&a, &b, step, ops.probes_true(a, b, step, lo));
    }
    return a ? a - 1u : 0u;   // lo >= o_0, so at least one offset is <= lo
}

template <class Ops>
PK_FN void copy_tile(Ops &ops, const Plan &p, uint32_t k, uint32_t skew, uint32_t n) {
    uint64_t lo, hi;
    tile_bounds(p, k, skew, &lo, &hi);
    if (lo >= hi) return;
    uint32_t i = first_page(ops, n, lo);
    uint64_t o;
    uint32_t len;
    ops.page(i, &o, &len);
    while (o < hi) {
        const uint32_t cur = i;
        const uint64_t co = o;
        const uint32_t clen = len;
        i++;
        if (i < n) ops.page(i, &o, &len);   // the next page's metadata is on its way during the copy
        else o = hi;
        const uint64_t s = co > lo ? co : lo;
        const uint64_t e = co + clen < hi ? co + clen : hi;
        if (e > s) ops.copy(cur, (uint32_t)(s - co), s, (uint32_t)(e - s));
    }
}

}  // namespace pk
