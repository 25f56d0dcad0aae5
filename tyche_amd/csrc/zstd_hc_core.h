// zstd_hc_core.h -- the per-wave parse of the high-compression zstd encoder
// (zstd_parse_hc_kernel in zstd_encode.hip, ZSTD_HC=1) for a page of 0..65535
// bytes.  Shared verbatim by the gfx950 kernel and by the host emulator
// tools/zstd_hc_emul.cpp, where the 64 lanes are an explicit loop, so that
// tests/test_zstd_hc_emul.py checks the algorithm on the CPU and the GPU tests
// compare the sequences of the kernel's frames with it.
//
// It writes no bytes: it fills the 64 lz_parse.h records (x = pos | cand << 16,
// y = len; the backward extension is the sink's, lz_parse.h kSinkBack) and hands them
// to sink(rec, n, anchor) in stream order exactly as lzp::parse_page does, and
// returns the anchor of the last literal run, or 0xFFFFFFFF when the sink aborts.
//
// The parse is lz4_hc_core.h's (blocks of kStride positions, lane k: base + k,
// bucket rings of the kWays latest positions of earlier blocks, the nearest lower
// lane of the block with the lane's hash, positions a match skips inserted too)
// with these differences:
//   * candidates: the ring's kWays, the lower lane, and the three repeat-offset
//     candidates pos - R, pos - R2, pos - R3, (R, R2, R3) as they stand after the
//     matches chosen before this block (parse_page's kRepCand; the walk is
//     wave-uniform, so it knows them).
//   * choice: not the longest but the one of the highest gain, in the form of the
//     reference's lazy parse (ZSTD_compressBlock_lazy_generic): 4 * length -
//     highbit32(offset + 1); a repeat candidate has offset cost 0 and kRepBonus on
//     top (its offset code has no extra bits and the cheapest symbols).  At the
//     offsets of a page, 2^8..2^15, that lets a repeat candidate win when 3 to 5
//     bytes shorter -- lz_parse.h's kRepSlack of 3 at a near offset.
//     Of equal gains the repeat candidates win, then the lower lane, then the ways.
//   * the lazy rule on gains: position p stays a literal when gain(p + 1) >
//     gain(p) + 4 or gain(p + 2) > gain(p) + 7 (the reference's depth 1 and 2);
//     every lane judges itself from its neighbours' gains, one ballot.
//   * the walk knows the repeat offsets as they are now, the lanes only those of
//     the block's start.  So the walk itself tries the first repeat offset at a
//     standing match when an earlier match of this block has brought a new one
//     (whole-wave count, the lanes' gain rule), and, as the reference does right
//     after every match ("check immediate repcode"), the second repeat offset at
//     the match's end: a match without literals, after which the two offsets
//     change places.  Records whose offsets repeat are what the frame codes
//     cheapest; without these two the mode closes half as much of the gap to the
//     reference's level 6 on record-structured pages (profiles/README.md).
//   * lengths are unbounded: a chosen match whose probe reached kProbe bytes is
//     counted on by the whole wave, 256 bytes per step.
// The bucket key is kHashBytes = 4 bytes: with 5, as the default zstd parse has,
// a match of exactly 4 bytes is never found through the rings, and pages of
// 16-byte items that differ in one byte lose 10-17 % (profiles/README.md).
// End rules: LZ4's MFLIMIT / LASTLITERALS do not exist here.  A match starts at
// or before L - 4 (its 4 hashed bytes lie inside the page) and ends at or before
// L.  Reads: a position's and a candidate's dword at q <= L - 4 stay inside the
// page (a 5- or 6-byte key reads in[q + 4], in[q + 5]: at most in[L + 1]);
// probe() and extend() read dwords at p < L only, so at most in[L + 2] --
// inside the 64 zero bytes that stand behind the page, and by less than
// parse_page's windows go (in[L + 11]).  The zero bytes are never counted: every
// count is cut at L.
// Every loop carries a bound derived from L or the block, so a logic error ends
// in a wrong answer, never in a wave that does not finish.
//
// The includer defines ZHC_HOST (1: lanes are loops over arrays; 0: SIMT) and,
// for the device, includes lds_io.h first.  The lane macros (LZX_*) are
// lz4_exact_core.h's, the ring macros (LZH_SAME, LZH_STORE_RING) lz4_hc_core.h's:
// they take kHashLog and kWays from the namespace they are expanded in.
#pragma once
#ifndef LZH_HOST
#define LZH_HOST ZHC_HOST
#endif
#include "lz4_hc_core.h"

#ifndef ZHC_WAYS_LOG
#define ZHC_WAYS_LOG 3
#endif
#ifndef ZHC_HASH_LOG
#define ZHC_HASH_LOG 9
#endif
#ifndef ZHC_HASH_BYTES
#define ZHC_HASH_BYTES 4
#endif
#ifndef ZHC_PROBE
#define ZHC_PROBE 36
#endif
#ifndef ZHC_REP_BONUS
#define ZHC_REP_BONUS 6
#endif
// ablation switches of the A/B in profiles/README.md (all on)
#ifndef ZHC_INSERT_SKIPPED
#define ZHC_INSERT_SKIPPED 1
#endif
#ifndef ZHC_WALK_REP
#define ZHC_WALK_REP 1
#endif
#ifndef ZHC_REP3
#define ZHC_REP3 1
#endif
#ifndef ZHC_REP_AFTER
#define ZHC_REP_AFTER 1
#endif
#ifndef ZHC_LAZY1
#define ZHC_LAZY1 4
#endif
#ifndef ZHC_LAZY2
#define ZHC_LAZY2 7
#endif

namespace zhc {

#if ZHC_HOST
struct Rec {
    uint32_t x, y;
};
#else
typedef uint2 Rec;
#endif

using lzh::popc64;
constexpr uint32_t kWaysLog = ZHC_WAYS_LOG, kWays = 1u << kWaysLog;   // 8 ways: one 16-byte LDS read per bucket
constexpr uint32_t kHashLog = ZHC_HASH_LOG, kBuckets = 1u << kHashLog;
constexpr uint32_t kTableEntries = kBuckets * kWays;                   // 16-bit positions
constexpr uint32_t kHashBytes = ZHC_HASH_BYTES;                        // bytes that key a bucket (4, 5 or 6)
constexpr uint32_t kProbe = ZHC_PROBE;                                 // bytes a lane counts of a candidate
constexpr uint32_t kStride = 62;                                       // positions a block parses; 2 more are lookahead
constexpr uint64_t kParsed = (1ull << kStride) - 1ull;
constexpr uint32_t kReps = ZHC_REP3 ? 3u : 2u;                         // repeat-offset candidates
constexpr uint32_t kCands = kReps + 1u + kWays;                        // the repeat offsets, the lower lane, the ways
constexpr uint32_t kGainBase = 32u;                                    // a match's gain is stored + kGainBase: 0 is "none"
constexpr uint32_t kRepBonus = ZHC_REP_BONUS;
// a block adds at most 16 records (each covers >= 4 of its positions) and as many right after them
constexpr uint32_t kFull = 64u - (ZHC_REP_AFTER ? 32u : 16u);
static_assert(kWays == 8u, "a bucket is read as 8 positions");
static_assert((kProbe - 4u) % 8u == 0u && kProbe >= 4u, "probe() counts 8 bytes per step after the first 4");

// the bucket of position q, whose first 4 bytes are w: keyed by kHashBytes bytes
LZX_FN uint32_t bucket(const uint8_t *in, uint32_t q, uint32_t w) {
    if (kHashBytes == 4u) return (w * 2654435761u) >> (32 - kHashLog);
    uint64_t x = (uint64_t)in[q + 4u] << 32;
    if (kHashBytes == 6u) x |= (uint64_t)in[q + 5u] << 40;
    return (uint32_t)(((x | w) * 0xCF1BBCDCB7A56463ull) >> (64 - kHashLog));
}
LZX_FN uint32_t highbit(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }   // v >= 1

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
            L_(h) = bucket(in, L_(q), lzx_in32(in, L_(q)));
        }
        const uint64_t I = LZX_BALLOT(valid);
        LZH_SAME(sameI, h, I)
        LZH_STORE_RING(table, cnt, h, q, sameI, I)
    }
}

// Bytes in[q ..] and in[c ..] share, 4 known equal, counted up to kProbe and
// never past limit (lzh::probe with this file's kProbe).
LZX_FN uint32_t probe(const uint8_t *in, uint32_t q, uint32_t c, uint32_t limit) {
    uint32_t n = 4u;
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

// The parse of in[0, L), 64 zero bytes behind it.  table: kTableEntries entries
// and cnt: kBuckets bytes, both zeroed (an unwritten slot is candidate 0, verified
// like any other).  rec: 64 records.
template <typename Sink>
LZX_FN uint32_t parse_page(const uint8_t *in, uint32_t L, uint16_t *table, uint8_t *cnt, Rec *rec,
                           Sink &sink LZX_LANE_PARAM) {
    using lzx::ctz64;
    if (L < 5u) return 0;                       // a match needs an earlier position and 4 bytes
    const uint32_t last = L - 4u;               // the last position a match may start at
    uint32_t anchor = 0, cursor = 0, nacc = 0;  // anchor: where the records' first literal run starts
    uint32_t R = 1u, R2 = 4u, R3 = 8u;                 // zstd's initial repeat offsets
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
            L_(h) = bucket(in, L_(q), L_(w));
        }
        const uint64_t V = LZX_BALLOT(valid);
        LZH_SAME(same, h, V)
        // ---- every lane's candidate of the highest gain
        LZX_V(uint32_t, gn);   // gain + kGainBase, 0: no match
        LZX_V(uint32_t, ln);
        LZX_V(uint32_t, cd);
        LZX_V(uint32_t, pl);
        LZX_EACH {
            const uint64_t bl = L_(same) & ((1ull << k) - 1ull);
            L_(pl) = bl ? 63u - (uint32_t)__builtin_clzll(bl) : 64u;
        }
        LZX_EACH {
            // all candidates' first words are read before any is counted: independent LDS reads
            const uint16_t *bk = (const uint16_t *)__builtin_assume_aligned(table + L_(h) * kWays, 2u * kWays);
            uint32_t cs[kCands];
            cs[0] = L_(q) >= R ? L_(q) - R : L_(q);
            cs[1] = L_(q) >= R2 && R2 != R ? L_(q) - R2 : L_(q);
            if (kReps == 3u) cs[2] = L_(q) >= R3 && R3 != R && R3 != R2 ? L_(q) - R3 : L_(q);
            cs[kReps] = L_(pl) < 64u ? base + L_(pl) : L_(q);
#pragma unroll
            for (uint32_t y = 0; y < kWays; y++) cs[kReps + 1u + y] = bk[y];
            uint32_t hit = 0;
#pragma unroll
            for (uint32_t y = 0; y < kCands; y++)
                if (lzx_in32(in, cs[y]) == L_(w) && cs[y] < L_(q)) hit |= 1u << y;
            if (!L_(valid)) hit = 0;
            uint32_t best = 0, bn = 0, bc = 0;
#pragma unroll
            for (uint32_t y = 0; y < kCands; y++) {
                if ((hit >> y) & 1u) {
                    const uint32_t n = probe(in, L_(q), cs[y], L);
                    const uint32_t g = 4u * n + kGainBase + (y < kReps ? kRepBonus : 0u) - (y < kReps ? 0u : highbit(L_(q) - cs[y] + 1u));
                    if (g > best) {
                        best = g;
                        bn = n;
                        bc = cs[y];
                    }
                }
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
            L_(em) = k < kStride && g0 != 0u && !(g1 > g0 + ZHC_LAZY1 || g2 > g0 + ZHC_LAZY2);
        }
        const uint64_t E = LZX_BALLOT(em);
        const uint32_t Rb = R, R2b = R2, R3b = R3;
        uint32_t s = cursor > base ? cursor - base : 0u;
        for (uint32_t n = 0; n < 16u && s < kStride; n++) {
            const uint64_t rest = E >> s;
            if (!rest) break;
            s += ctz64(rest);
            const uint32_t pos = base + s;
            uint32_t cand = LZX_UNI(LZX_AT(cd, s)), len = LZX_UNI(LZX_AT(ln, s));
            if (len == kProbe && pos + len < L) len += extend(in, L, pos + len, cand + len, L LZX_LANE_ARG);
#if ZHC_WALK_REP
            // the lanes saw the repeat offsets of the block's start; a match chosen earlier in this block
            // may have brought a new first one, which the walk tries here by the lanes' rule
            if (R != Rb && R != R2b && R != R3b && pos - cand != R && pos >= R) {
                const uint32_t rn = extend(in, L, pos, pos - R, L LZX_LANE_ARG);
                if (rn >= 4u && 4u * rn + kRepBonus + highbit(pos - cand + 1u) >= 4u * len) {
                    cand = pos - R;
                    len = rn;
                }
            }
#endif
            if (LZX_LANE0) {
                rec[nacc].x = pos | (cand << 16);
                rec[nacc].y = len;
            }
            nacc++;
            const uint32_t off = pos - cand;
            if (off != R) {
                if (off != R2) R3 = R2;
                R2 = R;
                R = off;
            }
            cursor = pos + len;
#if ZHC_REP_AFTER
            // the reference's check right after a match (zstd_compress.c, "check immediate repcode"):
            // where the bytes at its end repeat at the second repeat offset, a match without
            // literals, and the two offsets change places
            if (cursor <= last && cursor >= R2) {
                const uint32_t rn = extend(in, L, cursor, cursor - R2, L LZX_LANE_ARG);
                if (rn >= 4u) {
                    if (LZX_LANE0) {
                        rec[nacc].x = cursor | ((cursor - R2) << 16);
                        rec[nacc].y = rn;
                    }
                    nacc++;
                    const uint32_t t = R;
                    R = R2;
                    R2 = t;
                    cursor += rn;
                }
            }
#endif
            s = cursor - base;
        }
        if (nacc > kFull) {
            LZX_SYNC();
            if (!sink(rec, nacc, anchor)) return 0xFFFFFFFFu;
            LZX_SYNC();
            anchor = cursor;
            nacc = 0;
        }
        uint32_t nb = base + kStride;
        if (cursor > nb) {
#if ZHC_INSERT_SKIPPED
            insert(in, last, table, cnt, nb, cursor LZX_LANE_ARG);
#endif
            nb = cursor;
        }
        base = nb;
    }
    if (nacc) {
        LZX_SYNC();
        if (!sink(rec, nacc, anchor)) return 0xFFFFFFFFu;
        LZX_SYNC();
        anchor = cursor;
    }
    return anchor;
}

}  // namespace zhc
