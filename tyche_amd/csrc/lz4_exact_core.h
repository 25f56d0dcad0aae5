// lz4_exact_core.h -- the per-wave algorithm of the exact LZ4 encoder
// (lz4_encode_exact.hip, LZ4_EXACT=1): the stream LZ4_compress_default of LZ4
// 1.7.5 emits for a page of 0..65535 bytes (lz4.c:459-656 through :659-676,
// byU16 table), byte for byte and with its return value.  Shared verbatim by
// the gfx950 kernel and by the host emulator tools/lz4x_emul.cpp, where the 64
// lanes are an explicit loop, so that tests/test_lz4_exact_emul.py proves the
// algorithm against the oracle on the CPU.
//
// The reference walks the page serially; the wave is used where its result does
// not depend on order:
//   * search: the lanes of a batch hash 64 of the walk's positions at once (a
//     window of consecutive positions while a search's steps are 1, else 64
//     attempts at the schedule's closed-form positions, sched()).  A lane's
//     candidate is the position of the latest earlier walked lane of the batch
//     with the same hash (it would have overwritten the slot before it was
//     read), else the table's value.  The first walked lane whose candidate
//     matches is the walk's next match; only the lanes the walk reached store
//     their positions, the highest lane of every hash winning its slot (the
//     losers are masked: no two lanes of one store instruction write the same
//     slot).  encode_page() says how one window serves several sequences.
//   * catch-up and match length: 64 / 256 bytes per step by the whole wave.
//   * the sequence's bytes: 64 per store instruction.
// Every loop carries a bound derived from L, so a logic error ends in a wrong
// answer, never in a wave that does not finish.
//
// The includer defines LZX_HOST (1: lanes are loops over arrays; 0: SIMT, a
// `lane` variable in scope of every function below through LZX_LANE_ARG) and,
// for the device, includes lds_io.h first (rfl, rdlane, lds_ld32).
#pragma once
#include <stdint.h>

#if LZX_HOST
#define LZX_FN static inline
#define LZX_V(T, name) T name[64]                 // one value per lane
#define LZX_EACH for (uint32_t k = 0; k < 64u; k++)
#define L_(name) name[k]
#define LZX_AT(name, i) name[i]                   // lane i's value, i wave-uniform
#define LZX_SHFL(name, i) name[i]                 // lane i's value, i per lane
#define LZX_BALLOT(name) lzx_ballot_host(name)
#define LZX_UNI(x) (x)
#define LZX_SYNC() do {} while (0)
#define LZX_LANE_PARAM
#define LZX_LANE_ARG
#define LZX_LANE0 true
LZX_FN uint64_t lzx_ballot_host(const bool *p) {
    uint64_t m = 0;
    for (uint32_t k = 0; k < 64u; k++) m |= (uint64_t)p[k] << k;
    return m;
}
LZX_FN uint32_t lzx_in32(const uint8_t *in, uint32_t p) {
    return (uint32_t)in[p] | ((uint32_t)in[p + 1] << 8) | ((uint32_t)in[p + 2] << 16) | ((uint32_t)in[p + 3] << 24);
}
#else
#define LZX_FN __device__ __forceinline__
#define LZX_V(T, name) T name
#define LZX_EACH if (const uint32_t k = lane; true)
#define L_(name) name
#define LZX_AT(name, i) tyche::rdlane(name, i)
// (a lane that a divergent branch has switched off gives 0 to the lanes that read it: every
// LZX_SHFL stands where all 64 lanes execute it, never inside a per-lane condition)
#define LZX_SHFL(name, i) ((uint32_t)__shfl((int)(name), (int)(i)))
#define LZX_BALLOT(name) __ballot(name)
#define LZX_UNI(x) tyche::rfl(x)
#define LZX_SYNC() __builtin_amdgcn_wave_barrier()
#define LZX_LANE_PARAM , uint32_t lane
#define LZX_LANE_ARG , lane
#define LZX_LANE0 (lane == 0)
LZX_FN uint32_t lzx_in32(const uint8_t *in, uint32_t p) { return tyche::lds_ld32(in + p); }
#endif

namespace lzx {

constexpr uint32_t kHashLog = 13;                    // byU16: 8192 slots of 16-bit positions (lz4.c:402-408)
constexpr uint32_t kTableSize = 1u << kHashLog;
constexpr uint32_t kMfLimitX = 12, kLastLiteralsX = 5, kMinLength = 13;

LZX_FN uint32_t hash4(uint32_t w) { return (w * 2654435761u) >> (32 - kHashLog); }
LZX_FN uint32_t ctz64(uint64_t m) { return (uint32_t)__builtin_ctzll(m); }

// Attempt t of a search that starts at ip looks at ip + lzx_sched(t): steps
// s_0 = 1, s_t = (63 + t) >> 6 (lz4.c:519-546 with acceleration 1: 65 steps of
// 1, then 64 of 2, 64 of 3, ...).  For t > 65 the sum is 1 + F(62 + t) with
// F(M) = sum of floor(m / 64) over m = 0..M = 32 a (a - 1) + r a,
// a = (M + 1) / 64, r = (M + 1) % 64.
LZX_FN uint32_t sched(uint32_t t) {
    const uint32_t n = 63u + t, a = n >> 6, r = n & 63u;
    return t <= 65u ? t : 1u + 32u * a * (a - 1u) + r * a;
}

// dst[j] = v, never at or past the capacity (the reference's wild copies may
// overshoot what it then reports; exact mode keeps to the caller's buffer)
LZX_FN void put(uint8_t *dst, uint32_t cap, uint32_t j, uint32_t v) {
    if (j < cap) dst[j] = (uint8_t)v;
}

// Equal bytes of in[pos + 4 ..] and in[cnd + 4 ..], stopping at matchlimit
// (LZ4_count, lz4.c:567-599): 256 bytes per step from step0, a dword per lane.
LZX_FN uint32_t count_match(const uint8_t *in, uint32_t L, uint32_t pos, uint32_t cnd, uint32_t matchlimit,
                            uint32_t step0 LZX_LANE_PARAM) {
    for (uint32_t step = step0; step <= L / 256u + 1u; step++) {
        LZX_V(uint32_t, nb);
        LZX_V(bool, stop);
        LZX_EACH {
            const uint32_t d = 4u + 256u * step + 4u * k, p = pos + d;
            uint32_t n = 0;
            if (p < matchlimit) {
                const uint32_t x = lzx_in32(in, p) ^ lzx_in32(in, cnd + d);
                n = x ? (uint32_t)__builtin_ctz(x) >> 3 : 4u;
                if (n > matchlimit - p) n = matchlimit - p;
            }
            L_(nb) = n;
            L_(stop) = n < 4u;
        }
        const uint64_t B = LZX_BALLOT(stop);
        if (B) {
            const uint32_t f = ctz64(B);
            return 256u * step + 4u * f + LZX_UNI(LZX_AT(nb, f));
        }
    }
    return 0;
}

// One sequence at dst + op: token, literal-length bytes, the literals
// in[anchor, anchor + lit), the offset, match-length bytes (lz4.c:557-563,
// :597-605).  mc = match length - 4.  Returns its size.
LZX_FN uint32_t put_sequence(const uint8_t *in, uint8_t *dst, uint32_t cap, uint32_t op, uint32_t anchor, uint32_t lit,
                             uint32_t off, uint32_t mc LZX_LANE_PARAM) {
    const uint32_t llb = lit >= 15u ? (lit - 15u) / 255u + 1u : 0u;
    const uint32_t mlb = mc >= 15u ? (mc - 15u) / 255u + 1u : 0u;
    const uint32_t ob = 1u + llb + lit, total = ob + 2u + mlb;
    const uint32_t token = ((lit < 15u ? lit : 15u) << 4) | (mc < 15u ? mc : 15u);
    for (uint32_t j0 = 0; j0 < total; j0 += 64u) {
        LZX_EACH {
            const uint32_t j = j0 + k;
            if (j < total) {
                uint32_t v;
                if (j == 0u) v = token;
                else if (j <= llb) v = j == llb ? (lit - 15u) % 255u : 255u;
                else if (j < ob) v = in[anchor + j - 1u - llb];
                else if (j == ob) v = off & 0xFFu;
                else if (j == ob + 1u) v = off >> 8;
                else v = j == total - 1u ? (mc - 15u) % 255u : 255u;
                put(dst, cap, op + j, v);
            }
        }
    }
    return total;
}

// The sequence of the match in[pos ..] == in[cnd ..] (4 bytes known equal) after
// the literals from anchor: catch-up (lz4.c:549: backwards without bound, 64
// bytes per step) and the match length (LZ4_count from pos + 4, 256 bytes per
// step), their first steps read together; the limited-output checks; the bytes.
// anchor becomes the match's end.  false: the output does not fit (return 0).
LZX_FN bool put_match(const uint8_t *in, uint32_t L, uint8_t *dst, uint32_t cap, bool limited, uint32_t matchlimit,
                      uint32_t &anchor, uint32_t &op, uint32_t pos, uint32_t cnd LZX_LANE_PARAM) {
    uint32_t back = 0, extra = 0;
    LZX_V(uint32_t, litb);
    {
        const uint32_t lim = pos - anchor < cnd ? pos - anchor : cnd;
        LZX_V(bool, ne);
        LZX_V(uint32_t, nb);
        LZX_V(bool, stop);
        LZX_EACH {
            // byte k of a short sequence that is a literal (read with the rest: one LDS round trip less)
            const uint32_t li = anchor + (k ? k - 1u : 0u);
            L_(litb) = in[li < L ? li : L - 1u];
            L_(ne) = k >= lim || in[pos - 1u - k] != in[cnd - 1u - k];
            const uint32_t d = 4u + 4u * k, p = pos + d;
            uint32_t n = 0;
            if (p < matchlimit) {
                const uint32_t x = lzx_in32(in, p) ^ lzx_in32(in, cnd + d);
                n = x ? (uint32_t)__builtin_ctz(x) >> 3 : 4u;
                if (n > matchlimit - p) n = matchlimit - p;
            }
            L_(nb) = n;
            L_(stop) = n < 4u;
        }
        const uint64_t Bb = LZX_BALLOT(ne), Bf = LZX_BALLOT(stop);
        back = Bb ? ctz64(Bb) : 64u;
        if (Bf) {
            const uint32_t f = ctz64(Bf);
            extra = 4u * f + LZX_UNI(LZX_AT(nb, f));
        } else {
            extra = count_match(in, L, pos, cnd, matchlimit, 1u LZX_LANE_ARG);
        }
    }
    if (back == 64u) {
        for (uint32_t g = 0; g <= L / 64u + 1u; g++) {
            const uint32_t a = pos - back, c = cnd - back;
            const uint32_t lim = a - anchor < c ? a - anchor : c;
            if (!lim) break;
            LZX_V(bool, ne);
            LZX_EACH L_(ne) = k >= lim || in[a - 1u - k] != in[c - 1u - k];
            const uint64_t B = LZX_BALLOT(ne);
            const uint32_t n = B ? ctz64(B) : 64u;
            back += n;
            if (n < 64u) break;
        }
    }
    // the matched bytes before pos + 4 count in the sequence's length (lz4.c:551-605)
    const uint32_t end = pos + 4u + extra;
    pos -= back;
    cnd -= back;
    const uint32_t lit = pos - anchor, mc = back + extra;
    if (lit < 15u && mc < 15u) {
        // the common short sequence -- token, literals, offset: lit + 3 bytes in one store; both
        // checks below come to op + lit + 9 <= cap
        if (limited && op + lit + 9u > cap) return false;
        const uint32_t token = (lit << 4) | mc, off = pos - cnd;
        LZX_EACH {
            uint32_t v = L_(litb);
            v = k == 0u ? token : v;
            v = k == lit + 1u ? off & 0xFFu : v;
            v = k == lit + 2u ? off >> 8 : v;
            if (k < lit + 3u) put(dst, cap, op + k, v);
        }
        op += lit + 3u;
        anchor = end;
        return true;
    }
    const uint32_t llb = lit >= 15u ? (lit - 15u) / 255u + 1u : 0u;
    // lz4.c:554-556 (op after the token byte; a sequence without literals skips it there, and
    // the next check implies it), then lz4.c:594-596 (op after the offset)
    if (limited && op + 1u + lit + 8u + lit / 255u > cap) return false;
    if (limited && op + 1u + llb + lit + 2u + 6u + (mc >> 8) > cap) return false;
    op += put_sequence(in, dst, cap, op, anchor, lit, pos - cnd, mc LZX_LANE_ARG);
    anchor = end;
    return true;
}

// The page in[0, L) into dst[0, cap): the return of LZ4_compress_default(in, dst,
// L, cap).  table: kTableSize entries, zeroed.  No byte past in[L - 1] is read.
//
// Two kinds of batch:
//   * a window: lane k is position base + k.  While a search is in its first 64
//     attempts its steps are 1, so the walk -- attempts, the match, the insert
//     of end - 2, the test of end at once (lz4.c:615-631), the next search from
//     end + 1 -- visits lanes in rising order, and one window serves every
//     sequence that starts in it: W is the set of lanes walked so far, and a
//     lane's candidate is the highest walked lane below it with its hash, else
//     the table's value (read once per window; the walked lanes store their
//     positions when the window is left).  After a match a new window starts at
//     end - 2 unless end is still inside this one.
//   * a continuation: attempts 64 - s, ... of a search that found nothing in its
//     window, 64 per batch at the schedule's growing steps; the first hit ends
//     the batch.
LZX_FN int32_t encode_page(const uint8_t *in, uint32_t L, uint16_t *table, uint8_t *dst, uint32_t cap LZX_LANE_PARAM) {
    const bool limited = cap < L + L / 255u + 16u;          // LZ4_compressBound (lz4.c:672)
    const uint32_t mflimit = L - kMfLimitX, matchlimit = L - kLastLiteralsX;   // used when L >= 13
    uint32_t anchor = 0, op = 0;
    if (L >= kMinLength) {
        if (LZX_LANE0) table[hash4(lzx_in32(in, 0))] = 0;   // position 0 first (lz4.c:506)
        LZX_SYNC();
        // window state: lane s is tested next; imm: it is the position where a match ended
        // (tested even at mflimit, lz4.c:618); W0: lanes walked before the window's first test
        uint32_t base = 1, s = 0;
        bool imm = false;
        uint64_t W0 = 0;
        // continuation state: the search's first position and the attempt of lane 0
        bool cont = false;
        uint32_t start = 0, t0 = 0;
        // every batch ends a sequence (>= 4 bytes) or walks >= 62 positions no later search walks again
        for (uint32_t it = 0; it <= L / 2u + 8u; it++) {
            LZX_V(uint32_t, q);
            LZX_V(uint32_t, w);
            LZX_V(uint32_t, h);
            LZX_V(bool, valid);   // window: the word is readable; continuation: the attempt is not abandoned
            LZX_V(bool, vs);      // window: valid as a search attempt (the next one is not past mflimit, lz4.c:529)
            LZX_EACH {
                uint32_t qq;
                bool v;
                if (!cont) {
                    qq = base + k;
                    v = qq <= mflimit;
                    L_(vs) = qq + 1u <= mflimit;
                } else {
                    qq = start + sched(t0 + k);
                    v = start + sched(t0 + k + 1u) <= mflimit;
                    L_(vs) = v;
                }
                L_(valid) = v;
                L_(q) = v ? qq : 0u;
                L_(w) = lzx_in32(in, L_(q));
                L_(h) = hash4(L_(w));
            }
            const uint64_t V = LZX_BALLOT(valid), VS = LZX_BALLOT(vs);   // prefixes of the lanes
            // same[k]: the valid lanes whose hash equals lane k's, one ballot per hash bit
            LZX_V(uint64_t, same);
            LZX_EACH L_(same) = V;
            for (uint32_t b = 0; b < kHashLog; b++) {
                LZX_V(bool, bit);
                LZX_EACH L_(bit) = ((L_(h) >> b) & 1u) != 0u;
                const uint64_t bal = LZX_BALLOT(bit);
                LZX_EACH L_(same) &= L_(bit) ? bal : ~bal;
            }
            LZX_V(uint64_t, sb);   // ... and of those the lanes below lane k
            LZX_EACH L_(sb) = L_(same) & ((1ull << k) - 1ull);
            LZX_V(uint32_t, tv);   // the table's candidate and its word
            LZX_V(uint32_t, wt);
            LZX_EACH {
                L_(tv) = table[L_(h)];
                L_(wt) = lzx_in32(in, L_(tv));
            }
            LZX_SYNC();
            uint64_t W = 0;        // the lanes that store their positions
            bool finish = false;   // the parse goes to the last literals
            if (!cont) {
                W = W0;
                bool hit_left = false;   // a match ended past the window
                for (uint32_t n = 0;; n++) {
                    if (n > 16u) {   // (every match moves s up by >= 4)
                        finish = true;
                        break;
                    }
                    const uint64_t from = ~((1ull << s) - 1ull);
                    const uint64_t ok = imm && base + s == mflimit ? VS | (1ull << s) : VS;
                    const uint64_t inval = ~ok & from;
                    const uint32_t a = inval ? ctz64(inval) : 64u;   // the first abandoned attempt
                    LZX_V(uint32_t, cand);
                    LZX_V(bool, hit);
                    LZX_EACH {
                        const uint64_t bl = L_(sb) & (W | from);
                        const uint32_t pl = bl ? 63u - (uint32_t)__builtin_clzll(bl) : 0u;
                        const uint32_t wc = LZX_SHFL(w, pl);
                        L_(cand) = bl ? base + pl : L_(tv);
                        L_(hit) = k >= s && k < a && (bl ? wc : L_(wt)) == L_(w);
                    }
                    const uint64_t M = LZX_BALLOT(hit);
                    if (!M) {
                        if (a < 64u) {
                            W |= from & ((1ull << a) - 1ull);
                            finish = true;
                        } else {
                            W |= from;
                            const uint32_t ss = s + (imm ? 1u : 0u);   // the search's first lane
                            cont = true;
                            start = base + ss;
                            t0 = 64u - ss;
                        }
                        break;
                    }
                    const uint32_t m = ctz64(M);
                    W |= from & ((2ull << m) - 1ull);
                    if (!put_match(in, L, dst, cap, limited, matchlimit, anchor, op, base + m,
                                   LZX_UNI(LZX_AT(cand, m)) LZX_LANE_ARG))
                        return 0;
                    if (anchor > mflimit) {
                        finish = true;
                        break;
                    }
                    const uint32_t e = anchor - base;   // >= m + 4
                    if (e > 63u) {
                        hit_left = true;
                        break;
                    }
                    W |= 1ull << (e - 2u);   // lz4.c:615
                    s = e;
                    imm = true;
                }
                if (hit_left) {
                    base = anchor - 2u;
                    W0 = 1;
                    s = 2;
                    imm = true;
                }
            } else {
                LZX_V(uint32_t, cand);
                LZX_V(bool, hit);
                LZX_EACH {
                    const uint64_t bl = L_(sb);
                    const uint32_t pl = bl ? 63u - (uint32_t)__builtin_clzll(bl) : 0u;
                    const uint32_t qp = LZX_SHFL(q, pl), wc = LZX_SHFL(w, pl);
                    L_(cand) = bl ? qp : L_(tv);
                    L_(hit) = L_(valid) && (bl ? wc : L_(wt)) == L_(w);
                }
                const uint64_t M = LZX_BALLOT(hit);
                if (!M) {
                    W = V;
                    if (V != ~0ull) finish = true;   // an attempt was abandoned
                    else t0 += 64u;
                } else {
                    const uint32_t m = ctz64(M);
                    W = V & ((2ull << m) - 1ull);
                    if (!put_match(in, L, dst, cap, limited, matchlimit, anchor, op, LZX_UNI(LZX_AT(q, m)),
                                   LZX_UNI(LZX_AT(cand, m)) LZX_LANE_ARG))
                        return 0;
                    if (anchor > mflimit) finish = true;
                    cont = false;
                    base = anchor - 2u;
                    W0 = 1;
                    s = 2;
                    imm = true;
                }
            }
            // the walked lanes store their positions, the highest lane of every hash winning its slot
            LZX_EACH {
                const uint64_t above = ~((2ull << k) - 1ull);
                if (((W >> k) & 1ull) && !(L_(same) & W & above)) table[L_(h)] = (uint16_t)L_(q);
            }
            LZX_SYNC();
            if (finish) break;
        }
    }
    // ---- last literals in[anchor, L) (lz4.c:636-653)
    const uint32_t run = L - anchor;
    if (limited && op + run + 1u + (run + 255u - 15u) / 255u > cap) return 0;
    const uint32_t llb = run >= 15u ? (run - 15u) / 255u + 1u : 0u;
    const uint32_t total = 1u + llb + run;
    for (uint32_t j0 = 0; j0 < total; j0 += 64u) {
        LZX_EACH {
            const uint32_t j = j0 + k;
            if (j < total) {
                uint32_t v;
                if (j == 0u) v = (run < 15u ? run : 15u) << 4;
                else if (j <= llb) v = j == llb ? (run - 15u) % 255u : 255u;
                else v = in[anchor + j - 1u - llb];
                put(dst, cap, op + j, v);
            }
        }
    }
    return (int32_t)(op + total);
}

}  // namespace lzx
