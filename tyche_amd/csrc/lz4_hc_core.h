// lz4_hc_core.h -- the per-wave algorithm of the high-compression LZ4 encoder
// (lz4_encode_hc.hip, LZ4_HC=1) for a page of 0..65535 bytes: the LZ4 block
// format of every other encoder here, from a better parse.  Shared verbatim by
// the gfx950 kernel and by the host emulator tools/lz4_hc_emul.cpp, where the 64
// lanes are an explicit loop, so that tests/test_lz4_hc_emul.py checks the
// algorithm on the CPU and the GPU tests compare the kernel's bytes with it.
//
// The parse, per block of kStride consecutive positions (lane k: base + k):
//   * candidates: 4 bytes hash into kBuckets buckets of kWays 16-bit positions,
//     each bucket a ring of the kWays latest positions of earlier blocks with
//     that hash (every position is inserted; cnt[] holds a ring's next way).
//     A lane also sees the nearest lower lane of its own block with its hash,
//     which the table does not hold yet (runs, short periods).
//   * every lane takes the longest verified candidate, counted up to kProbe
//     bytes; the earliest of equal ones wins.
//   * the two-step lazy rule: position p stays a literal when len(p+1) > len(p)
//     or len(p+2) > len(p) + 1 (every lane judges itself from its neighbours'
//     lengths); a wave-uniform walk emits the first standing match at or after
//     the last one's end, and so on.  Lanes kStride and kStride + 1 exist only
//     to be looked at by that rule: the next block starts at base + kStride and
//     parses them again.
//   * the match is caught up backwards and counted to its full length by the
//     whole wave, and its sequence written, by the exact encoder's writer
//     (lzx::put_match), so a length of kProbe is a floor, not a cap.
//   * positions a match skips beyond its block are inserted too (insert()
//     alone, no search): later pages of text match into them.
// The stream is written as far as dst_capacity reaches, never beyond, and the
// result is its size when all of it fitted, else 0.
// The dictionary encoder (lz4_encode_hc_dict.hip, LZ4_HC_DICT=1; host emulator
// tools/lz4_hc_dict_emul.cpp) runs the same parse from a start position: the
// dictionary's tail in front of the page is history that candidates may lie in,
// and the rings start from a seed instead of from zero (seed_window,
// encode_window).  The plain page is the window whose start is 0.
// Every loop carries a bound derived from the window or the block, so a logic error ends
// in a wrong answer, never in a wave that does not finish.
//
// The includer defines LZH_HOST (1: lanes are loops over arrays; 0: SIMT) and,
// for the device, includes lds_io.h first, exactly as for lz4_exact_core.h,
// whose lane macros (LZX_*) and sequence writer this file uses.
#pragma once
#define LZX_HOST LZH_HOST
#include "lz4_exact_core.h"

#ifndef LZH_WAYS_LOG
#define LZH_WAYS_LOG 3
#endif
#ifndef LZH_HASH_LOG
#define LZH_HASH_LOG 9
#endif
#ifndef LZH_PROBE
#define LZH_PROBE 36
#endif
#ifndef LZH_INSERT_SKIPPED
#define LZH_INSERT_SKIPPED 1
#endif

namespace lzh {

constexpr uint32_t kWaysLog = LZH_WAYS_LOG, kWays = 1u << kWaysLog;   // 8 ways: one 16-byte LDS read per bucket
constexpr uint32_t kHashLog = LZH_HASH_LOG, kBuckets = 1u << kHashLog;
constexpr uint32_t kTableEntries = kBuckets * kWays;                   // 16-bit positions
constexpr uint32_t kProbe = LZH_PROBE;                                 // bytes a lane counts of a candidate (4 + dwords)
constexpr uint32_t kStride = 62;                                       // positions a block parses; 2 more are lookahead
constexpr uint64_t kParsed = (1ull << kStride) - 1ull;

LZX_FN uint32_t hash4(uint32_t w) { return (w * 2654435761u) >> (32 - kHashLog); }
LZX_FN uint32_t popc64(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }

// same[k]: the lanes of V whose hash equals lane k's, one ballot per hash bit
#define LZH_SAME(same, h, V)                                        \
    LZX_V(uint64_t, same);                                          \
    LZX_EACH L_(same) = (V);                                        \
    for (uint32_t b_ = 0; b_ < kHashLog; b_++) {                    \
        LZX_V(bool, bit_);                                          \
        LZX_EACH L_(bit_) = ((L_(h) >> b_) & 1u) != 0u;             \
        const uint64_t bal_ = LZX_BALLOT(bit_);                     \
        LZX_EACH L_(same) &= L_(bit_) ? bal_ : ~bal_;               \
    }

// The lanes of I put their positions q into their buckets' rings in rising lane
// order.  sameI[k]: the lanes of I with lane k's hash.  Of more than kWays lanes
// of one hash the last kWays write, so no two lanes of the store write one slot.
#if LZH_HOST
#define LZH_STORE_RING(table, cnt, h, q, sameI, I)                                              \
    {                                                                                           \
        LZX_V(uint32_t, c_);                                                                    \
        LZX_EACH L_(c_) = cnt[L_(h)];                                                           \
        LZX_EACH {                                                                              \
            if (((I) >> k) & 1ull) {                                                            \
                const uint32_t rank = popc64(L_(sameI) & ((1ull << k) - 1ull));                 \
                const uint32_t above = popc64(L_(sameI) & ~((2ull << k) - 1ull));               \
                if (above < kWays) table[L_(h) * kWays + ((L_(c_) + rank) & (kWays - 1u))] = (uint16_t)L_(q); \
                if (above == 0u) cnt[L_(h)] = (uint8_t)((L_(c_) + rank + 1u) & (kWays - 1u));   \
            }                                                                                   \
        }                                                                                       \
    }
#else
#define LZH_STORE_RING(table, cnt, h, q, sameI, I)                                              \
    {                                                                                           \
        const uint32_t c_ = cnt[h];                                                             \
        LZX_SYNC();                                                                             \
        if (((I) >> lane) & 1ull) {                                                             \
            const uint32_t rank = popc64(sameI & ((1ull << lane) - 1ull));                      \
            const uint32_t above = popc64(sameI & ~((2ull << lane) - 1ull));                    \
            if (above < kWays) table[h * kWays + ((c_ + rank) & (kWays - 1u))] = (uint16_t)q;   \
            if (above == 0u) cnt[h] = (uint8_t)((c_ + rank + 1u) & (kWays - 1u));               \
        }                                                                                       \
        LZX_SYNC();                                                                             \
    }
#endif

// Inserts the positions [from, to) (a match skipped them), 64 per step.
LZX_FN void insert(const uint8_t *in, uint32_t mflimit, uint16_t *table, uint8_t *cnt, uint32_t from,
                   uint32_t to LZX_LANE_PARAM) {
    for (uint32_t base = from; base < to && base <= mflimit; base += 64u) {
        LZX_V(uint32_t, q);
        LZX_V(uint32_t, h);
        LZX_V(bool, valid);
        LZX_EACH {
            const uint32_t qq = base + k;
            L_(valid) = qq < to && qq <= mflimit;
            L_(q) = L_(valid) ? qq : 0u;
            L_(h) = hash4(lzx_in32(in, L_(q)));
        }
        const uint64_t I = LZX_BALLOT(valid);
        LZH_SAME(sameI, h, I)
        LZH_STORE_RING(table, cnt, h, q, sameI, I)
    }
}

// Bytes in[q ..] and in[c ..] share, 4 known equal, counted up to kProbe and
// never past matchlimit: two dwords of each per step (four independent LDS
// reads), the second pair only where it lies inside the page.
static_assert((kProbe - 4u) % 8u == 0u && kProbe >= 4u, "probe() counts 8 bytes per step after the first 4");
LZX_FN uint32_t probe(const uint8_t *in, uint32_t q, uint32_t c, uint32_t matchlimit) {
    uint32_t n = 4u;
    while (n < kProbe) {
        const uint32_t p = q + n;
        if (p >= matchlimit) break;
        const uint32_t p1 = p + 4u < matchlimit ? 4u : 0u;    // (0: the first pair again, never counted)
        const uint32_t x0 = lzx_in32(in, p) ^ lzx_in32(in, c + n);
        const uint32_t x1 = lzx_in32(in, p + p1) ^ lzx_in32(in, c + n + p1);
        uint32_t m = x0 ? (uint32_t)__builtin_ctz(x0) >> 3 : !p1 ? 4u : x1 ? 4u + ((uint32_t)__builtin_ctz(x1) >> 3) : 8u;
        if (m > matchlimit - p) m = matchlimit - p;
        n += m;
        if (m < 8u) break;
    }
    return n;
}

// The dictionary encoder's seed (lz4_encode_hc_dict.hip): what inserting the
// positions 0 .. start - 4 of a window, those whose 4 bytes lie wholly in front
// of start, leaves in a zeroed table and zeroed counters.  Reads in[0, start).
LZX_FN void seed_window(const uint8_t *in, uint32_t start, uint16_t *table, uint8_t *cnt LZX_LANE_PARAM) {
    if (start >= 4u) insert(in, start - 4u, table, cnt, 0u, start - 3u LZX_LANE_ARG);
}

// The page in[start, W) of the window in[0, W), W <= 65536, into dst[0, cap):
// the stream's size, or 0 when it does not fit cap.  in[0, start) is history
// (a dictionary): blocks, the anchor and so every backward catch-up begin at
// start, candidates may be any earlier window position, and the end-of-block
// rules hold on the page.  table: kTableEntries entries and cnt: kBuckets
// bytes, as seed_window left them (start == 0: zeroed; an unwritten slot is
// candidate 0, verified like any other); the three positions in front of start
// whose 4 bytes run into the page are inserted here, so that a run across the
// seam finds its source.  No byte past in[W - 1] is read.
LZX_FN int32_t encode_window(const uint8_t *in, uint32_t start, uint32_t W, uint16_t *table, uint8_t *cnt, uint8_t *dst,
                             uint32_t cap LZX_LANE_PARAM) {
    using lzx::ctz64;
    const uint32_t L = W;   // the writers' and the loops' bound
    const uint32_t mflimit = W - lzx::kMfLimitX, matchlimit = W - lzx::kLastLiteralsX;   // used when W - start >= 13
    uint32_t anchor = start, op = 0;
    if (W - start >= lzx::kMinLength) {
        if (start >= 3u) insert(in, mflimit, table, cnt, start - 3u, start LZX_LANE_ARG);
        uint32_t base = start;
        for (uint32_t it = 0; it <= (W - start) / kStride + 2u && base <= mflimit; it++) {
            LZX_V(uint32_t, q);
            LZX_V(uint32_t, w);
            LZX_V(uint32_t, h);
            LZX_V(bool, valid);
            LZX_EACH {
                const uint32_t qq = base + k;
                L_(valid) = qq <= mflimit;
                L_(q) = L_(valid) ? qq : 0u;
                L_(w) = lzx_in32(in, L_(q));
                L_(h) = hash4(L_(w));
            }
            const uint64_t V = LZX_BALLOT(valid);
            LZH_SAME(same, h, V)
            // ---- every lane's longest candidate: its bucket's ways, then the nearest lower lane of its hash
            LZX_V(uint32_t, ln);   // 0: no match
            LZX_V(uint32_t, cd);
            LZX_V(uint32_t, pl);
            LZX_EACH {
                const uint64_t bl = L_(same) & ((1ull << k) - 1ull);
                L_(pl) = bl ? 63u - (uint32_t)__builtin_clzll(bl) : 64u;
            }
            LZX_EACH {
                // all candidates' first words are read before any is counted: independent LDS reads
                const uint16_t *bk = (const uint16_t *)__builtin_assume_aligned(table + L_(h) * kWays, 2u * kWays);
                uint32_t cs[kWays + 1u];
#pragma unroll
                for (uint32_t y = 0; y < kWays; y++) cs[y] = bk[y];
                cs[kWays] = L_(pl) < 64u ? base + L_(pl) : L_(q);
                uint32_t hit = 0;
#pragma unroll
                for (uint32_t y = 0; y <= kWays; y++)
                    if (lzx_in32(in, cs[y]) == L_(w) && cs[y] < L_(q)) hit |= 1u << y;
                if (!L_(valid)) hit = 0;
                uint32_t best = 0, bc = 0;
#pragma unroll
                for (uint32_t y = 0; y <= kWays; y++) {
                    if ((hit >> y) & 1u) {
                        const uint32_t n = probe(in, L_(q), cs[y], matchlimit);
                        if (n > best) {
                            best = n;
                            bc = cs[y];
                        }
                    }
                }
                L_(ln) = best;
                L_(cd) = bc;
            }
            LZX_SYNC();
            // ---- the parsed lanes enter the table
            {
                const uint64_t I = V & kParsed;
                LZX_V(uint64_t, sameI);
                LZX_EACH L_(sameI) = L_(same) & kParsed;
                LZH_STORE_RING(table, cnt, h, q, sameI, I)
            }
            // ---- the walk
            // em: the lanes whose match the lazy rule lets stand
            LZX_V(bool, em);
            LZX_EACH {
                const uint32_t l0 = L_(ln), l1 = LZX_SHFL(ln, (k + 1u) & 63u), l2 = LZX_SHFL(ln, (k + 2u) & 63u);
                L_(em) = k < kStride && l0 >= 4u && !(l1 > l0 || l2 > l0 + 1u);
            }
            const uint64_t E = LZX_BALLOT(em);
            uint32_t s = anchor > base ? anchor - base : 0u;
            for (uint32_t n = 0; n < 64u && s < kStride; n++) {
                const uint64_t rest = E >> s;
                if (!rest) break;
                s += ctz64(rest);
                if (!lzx::put_match(in, L, dst, cap, false, matchlimit, anchor, op, base + s,
                                    LZX_UNI(LZX_AT(cd, s)) LZX_LANE_ARG))
                    return 0;
                if (op > cap) return 0;
                s = anchor - base;
            }
            uint32_t nb = base + kStride;
            if (anchor > nb) {
#if LZH_INSERT_SKIPPED
                insert(in, mflimit, table, cnt, nb, anchor LZX_LANE_ARG);
#endif
                nb = anchor;
            }
            base = nb;
        }
    }
    // ---- last literals in[anchor, L)
    const uint32_t run = L - anchor;
    const uint32_t llb = run >= 15u ? (run - 15u) / 255u + 1u : 0u;
    const uint32_t total = 1u + llb + run;
    if (op + total > cap) return 0;
    for (uint32_t j0 = 0; j0 < total; j0 += 64u) {
        LZX_EACH {
            const uint32_t j = j0 + k;
            if (j < total) {
                uint32_t v;
                if (j == 0u) v = (run < 15u ? run : 15u) << 4;
                else if (j <= llb) v = j == llb ? (run - 15u) % 255u : 255u;
                else v = in[anchor + j - 1u - llb];
                lzx::put(dst, cap, op + j, v);
            }
        }
    }
    return (int32_t)(op + total);
}

// The page in[0, L) into dst[0, cap) from a zeroed table and zeroed counters
// (LZ4_HC=1): a window without history.
LZX_FN int32_t encode_page(const uint8_t *in, uint32_t L, uint16_t *table, uint8_t *cnt, uint8_t *dst,
                           uint32_t cap LZX_LANE_PARAM) {
    return encode_window(in, 0u, L, table, cnt, dst, cap LZX_LANE_ARG);
}

}  // namespace lzh
