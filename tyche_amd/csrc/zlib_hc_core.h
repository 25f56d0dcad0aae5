// zlib_hc_core.h -- the per-wave parse of the high-compression zlib encoder
// (zlib_deflate_hc_kernel in zlib_deflate_hc.hip, ZLIB_HC=1) for a page of 0..65535
// bytes.  Shared verbatim by the gfx950 kernel and by the host emulator
// tools/zlib_hc_emul.cpp, where the 64 lanes are an explicit loop, so that
// tests/test_zlib_hc_emul.py checks the algorithm on the CPU and the GPU tests
// compare the symbols of the kernel's streams with it.
//
// It writes no bytes: it fills up to 64 records of the form encode_page's passes
// 2 and 3 read (x = literal start | literal length << 16, y = match length |
// distance << 16; the match follows its literals) and hands them to sink(rec, n)
// in stream order, and returns the anchor where the last literal run starts, or
// 0xFFFFFFFF when the sink aborts.  A match may be longer than 258 bytes: the
// coder cuts it (n_chunks / chunk_len, zlib_deflate_core.h).
//
// The parse is lz4_hc_core.h's (blocks of kStride positions, lane k: base + k,
// bucket rings of the kWays latest positions of earlier blocks, the nearest lower
// lane of the block with the lane's hash, positions a match skips inserted too)
// with these differences:
//   * deflate's minimum: 3 bytes key a bucket, a candidate verifies on 3 bytes
//     and a match is 3 bytes or more.
//   * deflate's window: a candidate farther than kMaxDist = 32,768 is no
//     candidate (the default encoder's sink turns such a match back into
//     literals; here it never competes).
//   * choice by cost, not length: gain = kLenW * length - xbits(distance), where
//     xbits is the number of extra bits deflate's distance code carries (0 for
//     distances 1..4, highbit(distance - 1) - 1 above: 0..13).  kLenW stands for
//     the bits a covered byte saves.  A match of 3 bytes farther than kFar3, or
//     of 4 bytes farther than kFar4, is no match: its length and distance codes
//     cost more than its literals (deflate.c drops length 3 beyond TOO_FAR =
//     4096).  Of equal gains the lower lane wins, then the ways in ring order.
//   * the lazy rule on gains: position p stays a literal when gain(p + 1) >
//     gain(p) + kLazy1 or gain(p + 2) > gain(p) + kLazy2; every lane judges
//     itself from its neighbours' gains, one ballot.  Lanes kStride and
//     kStride + 1 exist only to be looked at by that rule.
//   * the walk (wave-uniform) takes the first standing match at or after the
//     previous match's end, extends it backwards over the literals before it
//     (at most 64 bytes, never below the previous match's end or position 0 of
//     the candidate), and counts a match that reached kProbe to its full length,
//     256 bytes per step.
// End rules: a match starts at or before L - 3 (its 3 keyed bytes lie inside the
// page) and ends at or before L.  Reads: a position's and a candidate's dword at
// q <= L - 3 reaches in[L]; probe() and extend() read dwords at p < L only, so
// at most in[L + 2] -- inside the 64 zero bytes that stand behind the page.  The
// zero bytes are never counted: every count is cut at L.
// Every loop carries a bound derived from L or the block, so a logic error ends
// in a wrong answer, never in a wave that does not finish.
//
// The includer defines ZLH_HOST (1: lanes are loops over arrays; 0: SIMT) and,
// for the device, includes lds_io.h first.  The lane macros (LZX_*) are
// lz4_exact_core.h's, the ring macros (LZH_SAME, LZH_STORE_RING) lz4_hc_core.h's:
// they take kHashLog and kWays from the namespace they are expanded in.
#pragma once
#ifndef LZH_HOST
#define LZH_HOST ZLH_HOST
#endif
#include "lz4_hc_core.h"

#ifndef ZLH_WAYS_LOG
#define ZLH_WAYS_LOG 4
#endif
#ifndef ZLH_HASH_LOG
#define ZLH_HASH_LOG 9
#endif
#ifndef ZLH_PROBE
#define ZLH_PROBE 36
#endif
#ifndef ZLH_LEN_W
#define ZLH_LEN_W 3
#endif
#ifndef ZLH_FAR3
#define ZLH_FAR3 2048
#endif
#ifndef ZLH_FAR4
#define ZLH_FAR4 32768
#endif
#ifndef ZLH_LAZY1
#define ZLH_LAZY1 1
#endif
#ifndef ZLH_LAZY2
#define ZLH_LAZY2 4
#endif
// ablation switches of the A/B in profiles/README.md (all on)
#ifndef ZLH_INSERT_SKIPPED
#define ZLH_INSERT_SKIPPED 1
#endif
#ifndef ZLH_LOWER_LANE
#define ZLH_LOWER_LANE 1
#endif
#ifndef ZLH_TRACE
#define ZLH_TRACE(base, gn, ln, cd, E, cursor)
#endif

namespace zlh {

#if ZLH_HOST
struct Rec {
    uint32_t x, y;
};
#else
typedef uint2 Rec;
#endif

using lzh::popc64;
constexpr uint32_t kWaysLog = ZLH_WAYS_LOG, kWays = 1u << kWaysLog;   // 16 ways: two 16-byte LDS reads per bucket
constexpr uint32_t kHashLog = ZLH_HASH_LOG, kBuckets = 1u << kHashLog;
constexpr uint32_t kTableEntries = kBuckets * kWays;                   // 16-bit positions
constexpr uint32_t kMinMatch = 3;
constexpr uint32_t kMaxDist = 32768;
constexpr uint32_t kProbe = ZLH_PROBE;                                 // bytes a lane counts of a candidate
constexpr uint32_t kStride = 62;                                       // positions a block parses; 2 more are lookahead
constexpr uint64_t kParsed = (1ull << kStride) - 1ull;
constexpr uint32_t kCands = 1u + kWays;                                // the lower lane, the ways
constexpr uint32_t kLenW = ZLH_LEN_W;
constexpr uint32_t kFar3 = ZLH_FAR3, kFar4 = ZLH_FAR4;
constexpr uint32_t kLazy1 = ZLH_LAZY1, kLazy2 = ZLH_LAZY2;
constexpr uint32_t kGainBase = 16u;                                    // a match's gain is stored + kGainBase: 0 is "none"
constexpr uint32_t kBlockRecs = (kStride + kMinMatch - 1u) / kMinMatch;   // a block adds at most 21 records
constexpr uint32_t kFull = 64u - kBlockRecs;
constexpr uint32_t kBackMax = 64;                                      // bytes of backward extension, one per lane
static_assert(kWays == 8u || kWays == 16u, "a bucket is read as one or two 16-byte vectors of positions");
static_assert((kProbe - 4u) % 8u == 0u && kProbe >= 4u, "probe() counts 8 bytes per step after the first 4");
static_assert(kLenW * kMinMatch + kGainBase > 13u, "a gain is never 0 or below");

// the bucket of a position whose first 4 bytes are w: keyed by its first 3
LZX_FN uint32_t bucket(uint32_t w) { return ((w << 8) * 2654435761u) >> (32 - kHashLog); }
LZX_FN uint32_t highbit(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }   // v >= 1
// extra bits of deflate's distance code (RFC 1951 3.2.5)
LZX_FN uint32_t dist_xbits(uint32_t dist) { return dist <= 4u ? 0u : highbit(dist - 1u) - 1u; }
// gain + kGainBase of a match of n bytes at distance dist; 0: not worth a match
LZX_FN uint32_t gain(uint32_t n, uint32_t dist) {
    if ((n == 3u && dist > kFar3) || (n == 4u && dist > kFar4)) return 0u;
    return kLenW * n + kGainBase - dist_xbits(dist);
}

// Inserts the positions [from, to) (a match skipped them), 64 per step.
LZX_FN void insert(const uint8_t *in, uint32_t last, uint16_t *table, uint8_t *cnt, uint32_t from,
                   uint32_t to LZX_LANE_PARAM) {
    for (uint32_t base = from; base < to && base <= last; base += 64u) {
        LZX_V(uint32_t, q);
        LZX_V(uint32_t, h);
        LZX_V(bool, valid);
        LZX_EACH {
            const uint32_t qq = base + k;
            L_(valid) = qq < to && qq <= last;
            L_(q) = L_(valid) ? qq : 0u;
            L_(h) = bucket(lzx_in32(in, L_(q)));
        }
        const uint64_t I = LZX_BALLOT(valid);
        LZH_SAME(sameI, h, I)
        LZH_STORE_RING(table, cnt, h, q, sameI, I)
    }
}

// Bytes in[q ..] and in[c ..] share, 3 known equal (w and cw: their first
// dwords), counted up to kProbe and never past limit.
LZX_FN uint32_t probe(const uint8_t *in, uint32_t q, uint32_t c, uint32_t w, uint32_t cw, uint32_t limit) {
    uint32_t n = w == cw ? 4u : 3u;
    if (n > limit - q) n = limit - q;
    if (n < 4u) return n;
    while (n < kProbe) {
        const uint32_t p = q + n;
        if (p >= limit) break;
        const uint32_t p1 = p + 4u < limit ? 4u : 0u;    // (0: the first pair again, never counted)
        const uint32_t x0 = lzx_in32(in, p) ^ lzx_in32(in, c + n);
        const uint32_t x1 = lzx_in32(in, p + p1) ^ lzx_in32(in, c + n + p1);
        uint32_t m = x0 ? (uint32_t)__builtin_ctz(x0) >> 3 : !p1 ? 4u : x1 ? 4u + ((uint32_t)__builtin_ctz(x1) >> 3) : 8u;
        if (m > limit - p) m = limit - p;
        n += m;
        if (m < 8u) break;
    }
    return n;
}

// Equal bytes of in[a ..] and in[b ..] (b < a), a stopping before limit: 256
// bytes per step, a dword per lane.
LZX_FN uint32_t extend(const uint8_t *in, uint32_t L, uint32_t a, uint32_t b, uint32_t limit LZX_LANE_PARAM) {
    for (uint32_t step = 0; step <= L / 256u + 1u; step++) {
        LZX_V(uint32_t, nb);
        LZX_V(bool, stop);
        LZX_EACH {
            const uint32_t d = 256u * step + 4u * k, p = a + d;
            uint32_t n = 0;
            if (p < limit) {
                const uint32_t x = lzx_in32(in, p) ^ lzx_in32(in, b + d);
                n = x ? (uint32_t)__builtin_ctz(x) >> 3 : 4u;
                if (n > limit - p) n = limit - p;
            }
            L_(nb) = n;
            L_(stop) = n < 4u;
        }
        const uint64_t B = LZX_BALLOT(stop);
        if (B) {
            const uint32_t f = lzx::ctz64(B);
            return 256u * step + 4u * f + LZX_UNI(LZX_AT(nb, f));
        }
    }
    return 0;
}

// Equal bytes right before in[pos] and in[cand], at most maxb <= kBackMax: a byte per lane.
LZX_FN uint32_t back(const uint8_t *in, uint32_t pos, uint32_t cand, uint32_t maxb LZX_LANE_PARAM) {
    LZX_V(bool, ne);
    LZX_EACH L_(ne) = k >= maxb || in[pos - 1u - (k < maxb ? k : 0u)] != in[cand - 1u - (k < maxb ? k : 0u)];
    const uint64_t B = LZX_BALLOT(ne);
    return B ? lzx::ctz64(B) : 64u;
}

// The parse of in[0, L), 64 zero bytes behind it.  table: kTableEntries entries
// and cnt: kBuckets bytes, both zeroed (an unwritten slot is candidate 0, verified
// like any other).  rec: 64 records.
template <typename Sink>
LZX_FN uint32_t parse_page(const uint8_t *in, uint32_t L, uint16_t *table, uint8_t *cnt, Rec *rec,
                           Sink &sink LZX_LANE_PARAM) {
    using lzx::ctz64;
    if (L < kMinMatch + 1u) return 0;           // a match needs an earlier position and 3 bytes
    const uint32_t last = L - kMinMatch;        // the last position a match may start at
    uint32_t cursor = 0, nacc = 0;              // cursor: the end of the last match, where the next literal run starts
    uint32_t base = 0;
    for (uint32_t it = 0; it <= L / kStride + 2u && base <= last; it++) {
        LZX_V(uint32_t, q);
        LZX_V(uint32_t, w);
        LZX_V(uint32_t, h);
        LZX_V(bool, valid);
        LZX_EACH {
            const uint32_t qq = base + k;
            L_(valid) = qq <= last;
            L_(q) = L_(valid) ? qq : 0u;
            L_(w) = lzx_in32(in, L_(q));
            L_(h) = bucket(L_(w));
        }
        const uint64_t V = LZX_BALLOT(valid);
        LZH_SAME(same, h, V)
        // ---- every lane's candidate of the highest gain
        LZX_V(uint32_t, gn);   // gain + kGainBase, 0: no match
        LZX_V(uint32_t, ln);
        LZX_V(uint32_t, cd);
        LZX_V(uint32_t, pl);
        LZX_EACH {
            const uint64_t bl = ZLH_LOWER_LANE ? L_(same) & ((1ull << k) - 1ull) : 0ull;
            L_(pl) = bl ? 63u - (uint32_t)__builtin_clzll(bl) : 64u;
        }
        LZX_EACH {
            // all candidates' first words are read before any is counted: independent LDS reads
            const uint16_t *bk = (const uint16_t *)__builtin_assume_aligned(table + L_(h) * kWays, 16);
            // (the lambdas are inlined by force: a closure left as a call keeps what it captures in memory)
            uint32_t best = 0, bn = 0, bc = 0;
            auto consider = [&](uint32_t c, uint32_t cwv) __attribute__((always_inline)) {
                const uint32_t n = probe(in, L_(q), c, L_(w), cwv, L);
                const uint32_t g = gain(n, L_(q) - c);
                if (g > best) {
                    best = g;
                    bn = n;
                    bc = c;
                }
            };
            auto verified = [&](uint32_t c, uint32_t cwv) __attribute__((always_inline)) {
                return L_(valid) && ((cwv ^ L_(w)) & 0xFFFFFFu) == 0u && c < L_(q) && L_(q) - c <= kMaxDist;
            };
            {
                const uint32_t c = L_(pl) < 64u ? base + L_(pl) : L_(q);
                const uint32_t cwv = lzx_in32(in, c);
                if (verified(c, cwv)) consider(c, cwv);
            }
            // (8 ways at a time: arrays that stay in registers)
            for (uint32_t g8 = 0; g8 < kWays; g8 += 8u) {
                uint32_t cs[8], cw[8];
#pragma unroll
                for (uint32_t y = 0; y < 8u; y++) cs[y] = bk[g8 + y];
                uint32_t hit = 0;
#pragma unroll
                for (uint32_t y = 0; y < 8u; y++) {
                    cw[y] = lzx_in32(in, cs[y]);
                    if (verified(cs[y], cw[y])) hit |= 1u << y;
                }
#pragma unroll
                for (uint32_t y = 0; y < 8u; y++)
                    if ((hit >> y) & 1u) consider(cs[y], cw[y]);
            }
            L_(gn) = best;
            L_(ln) = bn;
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
            const uint32_t g0 = L_(gn), g1 = LZX_SHFL(gn, (k + 1u) & 63u), g2 = LZX_SHFL(gn, (k + 2u) & 63u);
            L_(em) = k < kStride && g0 != 0u && !(g1 > g0 + kLazy1 || g2 > g0 + kLazy2);
        }
        const uint64_t E = LZX_BALLOT(em);
        ZLH_TRACE(base, gn, ln, cd, E, cursor)
        uint32_t s = cursor > base ? cursor - base : 0u;
        for (uint32_t n = 0; n < kBlockRecs && s < kStride; n++) {
            const uint64_t rest = E >> s;
            if (!rest) break;
            s += ctz64(rest);
            const uint32_t pos = base + s;
            const uint32_t cand = LZX_UNI(LZX_AT(cd, s));
            uint32_t len = LZX_UNI(LZX_AT(ln, s));
            if (len == kProbe && pos + len < L) len += extend(in, L, pos + len, cand + len, L LZX_LANE_ARG);
            uint32_t maxb = pos - cursor;
            if (maxb > cand) maxb = cand;
            if (maxb > kBackMax) maxb = kBackMax;
            const uint32_t bk = maxb ? back(in, pos, cand, maxb LZX_LANE_ARG) : 0u;
            if (LZX_LANE0) {
                rec[nacc].x = cursor | ((pos - bk - cursor) << 16);
                rec[nacc].y = (len + bk) | ((pos - cand) << 16);
            }
            nacc++;
            cursor = pos + len;
            s = cursor - base;
        }
        if (nacc > kFull) {
            LZX_SYNC();
            if (!sink(rec, nacc)) return 0xFFFFFFFFu;
            LZX_SYNC();
            nacc = 0;
        }
        uint32_t nb = base + kStride;
        if (cursor > nb) {
#if ZLH_INSERT_SKIPPED
            insert(in, last, table, cnt, nb, cursor LZX_LANE_ARG);
#endif
            nb = cursor;
        }
        base = nb;
    }
    if (nacc) {
        LZX_SYNC();
        if (!sink(rec, nacc)) return 0xFFFFFFFFu;
        LZX_SYNC();
    }
    return cursor;
}

}  // namespace zlh
