// lz4_train_core.h -- the per-page and per-segment steps of the shared-dictionary
// trainer (lz4_dict_train.hip; tyche_lz4_dict_train_batch).  Shared verbatim by
// the gfx950 kernels and by the host emulator tools/lz4_train_emul.cpp, where one
// "thread" (t = 0 of nt = 1) walks every strided loop, the barriers are nothing
// and the atomics are plain integer operations: every update is a commutative
// integer or / add / max, so the order in which threads arrive never shows.
//
// The algorithm (tests/lz4_train_cases.py restates it in numpy):
//   key     h(q) = (le64(page + q) * 0x9E3779B185EBCA87) >> (64 - 20), 0 <= q <= len - 8
//   count   df[h] = number of pages that hold key h somewhere (count_page: a bitmap per
//           page, indexed by h itself, dedups the page's own repeats -- 2^18 bits at a
//           time, one quarter of the key space per walk over the page, so that which
//           position "wins" a bit never matters: equal bits are equal keys)
//   weight  w[h] = df[h] >= 2 ? df[h] : 0 (taken at every read: the table keeps df)
//   score   g(q) = 0 if q > 0 and h(q) == h(q-1) (runs of one byte), else w[h(q)];
//           a candidate segment starts at s = 0, 8, 16, ... with s + 128 <= len and
//           scores the sum of g over its 121 key positions (score_page)
//   round   the best candidate of all pages (ties: lowest page, then lowest s) is
//           taken: its 128 bytes go to the dictionary, its keys' slots to 0
//           (apply_segment); a best score of 0 ends the training.
// Every loop is bounded by a page length or a constant.
//
// The includer defines LZT_HOST (1: host emulator; 0: device, lds_io.h included
// first for lds_ld32).
#pragma once
#include <stdint.h>

#if LZT_HOST
#include <string.h>
#define LZT_FN static inline
#define LZT_SYNC() do {} while (0)
LZT_FN uint32_t lzt_ld32(const uint8_t *p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
LZT_FN uint32_t lzt_or(uint32_t *p, uint32_t v) {
    const uint32_t old = *p;
    *p = old | v;
    return old;
}
LZT_FN void lzt_add(uint32_t *p, uint32_t v) { *p += v; }
LZT_FN void lzt_max64(unsigned long long *p, unsigned long long v) {
    if (v > *p) *p = v;
}
#else
#define LZT_FN __device__ __forceinline__
#define LZT_SYNC() __syncthreads()
LZT_FN uint32_t lzt_ld32(const uint8_t *p) { return tyche::lds_ld32(p); }   // the staged page, any byte address
LZT_FN uint32_t lzt_or(uint32_t *p, uint32_t v) { return atomicOr(p, v); }
LZT_FN void lzt_add(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
LZT_FN void lzt_max64(unsigned long long *p, unsigned long long v) { atomicMax(p, v); }
#endif

namespace lzt {

constexpr uint32_t kSeg = 128;                        // S: bytes per segment
constexpr uint32_t kKey = 8;                          // d: bytes per key
constexpr uint32_t kTableBits = 20;                   // F
constexpr uint32_t kStep = 8;                         // candidate step
constexpr uint32_t kTableSize = 1u << kTableBits;     // 4 MiB of uint32
constexpr uint32_t kBitmapBits = 18;                  // the per-page dedup bitmap: 32 KiB, one part of the key space
constexpr uint32_t kBitmapWords = (1u << kBitmapBits) / 32u;
constexpr uint32_t kCountParts = 1u << (kTableBits - kBitmapBits);
constexpr uint32_t kSegKeys = kSeg - kKey + 1u;       // 121 key positions per segment
constexpr uint32_t kBlocksPerSeg = (kSegKeys - 1u) / kStep;   // 15 whole blocks of 8 positions + 1 position
constexpr uint32_t kMaxPage = 65535;                  // longest sample page
constexpr uint32_t kPageShift = 13;                   // candidate index = page << 13 | s / 8 (s / 8 < 8192)
constexpr uint32_t kMaxPages = 1u << (32 - kPageShift);   // 524,288 pages per training
static_assert(kSegKeys == kBlocksPerSeg * kStep + 1u, "a segment's keys are whole blocks and one more");
static_assert(kMaxPage / kStep < (1u << kPageShift), "a candidate's block index fits the candidate index");

struct Blk {
    uint32_t sum;     // g over the block's 8 positions
    uint32_t first;   // g of its first position
};

LZT_FN uint32_t hash_key(uint64_t k) { return (uint32_t)((k * 0x9E3779B185EBCA87ull) >> (64 - kTableBits)); }
// the key at p: 8 bytes of the staged page (LDS on the device), q <= len - 8
LZT_FN uint32_t hash_at(const uint8_t *p) { return hash_key((uint64_t)lzt_ld32(p) | ((uint64_t)lzt_ld32(p + 4) << 32)); }
// the same from memory read by bytes (the taken segment, in global memory on the device)
LZT_FN uint32_t hash_bytes(const uint8_t *p) {
    uint64_t k = 0;
    for (uint32_t i = 0; i < kKey; i++) k |= (uint64_t)p[i] << (8u * i);
    return hash_key(k);
}
LZT_FN uint32_t weight(uint32_t df) { return df >= 2u ? df : 0u; }

LZT_FN uint32_t candidates(uint32_t len) { return len >= kSeg ? (len - kSeg) / kStep + 1u : 0u; }
LZT_FN uint32_t key_blocks(uint32_t len) { return len >= kKey ? (len - kKey + kStep) / kStep : 0u; }   // ceil((len - 7) / 8)

// A round's running best and a candidate, as one 64-bit value that atomic max orders: the higher
// score first, then the lower page, then the lower s.
LZT_FN unsigned long long pack_best(uint32_t score, uint32_t page, uint32_t blk) {
    return ((unsigned long long)score << 32) | (uint32_t)~((page << kPageShift) | blk);
}
LZT_FN uint32_t best_page(unsigned long long key) { return (~(uint32_t)key) >> kPageShift; }
LZT_FN uint32_t best_start(unsigned long long key) { return ((~(uint32_t)key) & ((1u << kPageShift) - 1u)) * kStep; }

// Weights only ever fall, so a page's best score of an earlier round (ub; 0xFFFFFFFF before its
// first) bounds every later one: a page that cannot beat what the round has found so far -- any
// value the round's best has held will do, it only rises -- is not scored again.  What a round
// picks does not depend on who was skipped.
LZT_FN bool cannot_win(uint32_t ub, uint32_t page, unsigned long long best_so_far) {
    return ub == 0u || pack_best(ub, page, 0) < best_so_far;
}

// Adds the page to the document frequencies.  bitmap: kBitmapWords words, zero on entry and on return.
LZT_FN void count_page(const uint8_t *pg, uint32_t len, uint32_t *bitmap, uint32_t *df, uint32_t t, uint32_t nt) {
    for (uint32_t part = 0; part < kCountParts; part++) {
        for (uint32_t q = t; q + kKey <= len; q += nt) {
            const uint32_t h = hash_at(pg + q), bit = 1u << (h & 31u);
            if ((h >> kBitmapBits) != part) continue;
            if (!(lzt_or(&bitmap[(h & ((1u << kBitmapBits) - 1u)) >> 5], bit) & bit)) lzt_add(&df[h], 1u);
        }
        LZT_SYNC();
        for (uint32_t i = t; i < kBitmapWords; i += nt) bitmap[i] = 0;
        LZT_SYNC();
    }
}

// Scores every candidate of the page and raises *best (the caller's own word, zero on entry) to
// pack_best of the page's best candidate with a score above 0.  blk: key_blocks(len) entries of
// workspace.  Uniform control flow: every thread of the workgroup calls it with the same arguments.
LZT_FN void score_page(const uint8_t *pg, uint32_t len, const uint32_t *table, Blk *blk, uint32_t page,
                       unsigned long long *best, uint32_t t, uint32_t nt) {
    const uint32_t nc = candidates(len);
    if (nc == 0) return;
    const uint32_t nkeys = len - kKey + 1u, nb = key_blocks(len);
    for (uint32_t j = t; j < nb; j += nt) {
        const uint32_t q0 = j * kStep;
        uint32_t prev = q0 ? hash_at(pg + q0 - 1u) : 0xFFFFFFFFu, sum = 0, first = 0;
        for (uint32_t i = 0; i < kStep && q0 + i < nkeys; i++) {
            const uint32_t h = hash_at(pg + q0 + i);
            const uint32_t g = h == prev ? 0u : weight(table[h]);
            if (i == 0) first = g;
            sum += g;
            prev = h;
        }
        blk[j] = Blk{sum, first};
    }
    LZT_SYNC();
    unsigned long long mine = 0;
    for (uint32_t j = t; j < nc; j += nt) {   // ascending s per thread: a tie keeps the lower one
        uint32_t score = blk[j + kBlocksPerSeg].first;
        for (uint32_t i = 0; i < kBlocksPerSeg; i++) score += blk[j + i].sum;
        const unsigned long long key = pack_best(score, page, j);
        if (score && key > mine) mine = key;
    }
    if (mine) lzt_max64(best, mine);
    LZT_SYNC();
}

// Takes a segment: its kSeg bytes go to out, its keys' slots to 0.
LZT_FN void apply_segment(const uint8_t *seg, uint32_t *table, uint8_t *out, uint32_t t, uint32_t nt) {
    for (uint32_t q = t; q < kSegKeys; q += nt) table[hash_bytes(seg + q)] = 0;
    for (uint32_t i = t; i < kSeg; i += nt) out[i] = seg[i];
}

}  // namespace lzt
