// lz4_dict_core.h -- the per-wave algorithms of the shared-dictionary LZ4
// kernels (lz4_encode_dict.hip, lz4_decode_dict.hip) that do not depend on the
// wave-parallel parse: the decoder, and the encoder's emission of the parse's
// records.  Shared verbatim by the gfx950 kernels and by the host emulator
// tools/lz4_dict_emul.cpp, where the 64 lanes are an explicit loop, so that
// tests/test_lz4_dict_emul.py proves the logic against the reference on the CPU.
//
// A dictionary of D bytes followed by a page of L bytes is one LZ4 window
// (L + D <= 65536, so window positions fit 16 bits and no offset passes 65,535):
//
//   decode_page   LZ4_decompress_safe_usingDict (lz4.c:1382 -> :1089-1248) with
//                 its return value: the walk of decode_page_serial
//                 (lz4_decode.hip) over an output window that has the dictionary
//                 in front of it, `out` pointing at the page's first byte.  A
//                 match may start as far back as out - D (offset == position +
//                 D); one more is the reference's error at the same point.
//   emit_records  the LZ4 sequences of up to 64 parse records (lz_parse.h) whose
//                 positions are window positions: every sequence's lane writes
//                 its own bytes, long literal runs are copied by the whole wave.
//                 An offset is pos - cand whatever side of the seam cand is on.
//   write_last_literals  the block's closing literal run.
// Every loop carries a bound derived from the page or stream length, so a logic
// error ends in a wrong answer, never in a wave that does not finish.
//
// The includer defines LZD_HOST (1: lanes are loops over arrays; 0: SIMT, a
// `lane` variable in scope through LZD_LANE_ARG) and, for the device, includes
// lds_io.h first (rfl, rdlane, wave_incl_sum).
#pragma once
#include <stdint.h>

#if LZD_HOST
#define LZD_FN static inline
#define LZD_V(T, name) T name[64]                  // one value per lane
#define LZD_EACH for (uint32_t k = 0; k < 64u; k++)
#define D_(name) name[k]
#define LZD_AT(name, i) name[i]                    // lane i's value, i wave-uniform
#define LZD_BALLOT(name) lzd_ballot_host(name)
#define LZD_STRIDED(j, n) for (int32_t j = 0; j < (int32_t)(n); j++)   // j = lane, lane + 64, ... < n
#define LZD_UNI(x) (x)
#define LZD_SYNC() do {} while (0)
#define LZD_LANE_PARAM
#define LZD_LANE_ARG
LZD_FN uint64_t lzd_ballot_host(const bool *p) {
    uint64_t m = 0;
    for (uint32_t k = 0; k < 64u; k++) m |= (uint64_t)p[k] << k;
    return m;
}
// inclusive prefix sum over the lanes
LZD_FN void lzd_incl_sum(const uint32_t *v, uint32_t *out) {
    uint32_t s = 0;
    for (uint32_t k = 0; k < 64u; k++) out[k] = (s += v[k]);
}
// the stream byte at p, through a 64-byte window loaded at the sequence's token
struct lzd_win {
    const uint8_t *in;
};
LZD_FN lzd_win lzd_win_load(const uint8_t *in, uint32_t) { return lzd_win{in}; }
LZD_FN uint32_t lzd_win_byte(const lzd_win &w, const uint8_t *, uint32_t p) { return w.in[p]; }
#else
#define LZD_FN __device__ __forceinline__
#define LZD_V(T, name) T name
#define LZD_EACH if (const uint32_t k = lane; true)
#define D_(name) name
#define LZD_AT(name, i) tyche::rdlane((uint32_t)(name), i)
#define LZD_BALLOT(name) __ballot(name)
#define LZD_STRIDED(j, n) for (int32_t j = (int32_t)lane; j < (int32_t)(n); j += 64)
#define LZD_UNI(x) tyche::rfl(x)
#define LZD_SYNC() __builtin_amdgcn_wave_barrier()
#define LZD_LANE_PARAM , uint32_t lane
#define LZD_LANE_ARG , lane
LZD_FN void lzd_incl_sum(const uint32_t &v, uint32_t &out) { out = (uint32_t)tyche::wave_incl_sum((int32_t)v); }
// lane k holds stream byte base + k (the staged stream has 64 zero bytes after it): the token,
// the length bytes and the offset of most sequences come out of one LDS read
struct lzd_win {
    uint32_t base, v;
};
LZD_FN lzd_win lzd_win_load(const uint8_t *in, uint32_t p LZD_LANE_PARAM) { return lzd_win{p, in[p + lane]}; }
LZD_FN uint32_t lzd_win_byte(const lzd_win &w, const uint8_t *in, uint32_t p) {
    const uint32_t d = p - w.base;
    if (d < 64u) return tyche::rdlane(w.v, d);
    return tyche::rfl(in[p]);
}
#endif

namespace lzd {

constexpr int32_t kMinMatchD = 4, kLastLiteralsD = 5, kMfLimitD = 12, kRunMaskD = 15;
constexpr uint32_t kDictMax = 32768;                 // TYCHE_LZ4_DICT_MAX
constexpr uint32_t kWindowMax = 65536;               // dictionary + page
constexpr uint32_t kHashLogD = 12;                   // the encoder's table: 4096 16-bit window positions
constexpr uint32_t kTableSizeD = 1u << kHashLogD;
constexpr uint32_t kLitLaneD = 16;                   // literal bytes a sequence's own lane copies
constexpr uint32_t kCatchUpD = 8;                    // backward extension of a match, at most (lz4.c:549)

// the table's key: the 5 bytes at a position (lz_parse.h's hash5; the reference's LZ4_hash5)
LZD_FN uint32_t hash5(const uint8_t *p) {
    const uint64_t x = (uint64_t)p[0] | ((uint64_t)p[1] << 8) | ((uint64_t)p[2] << 16) | ((uint64_t)p[3] << 24) |
                       ((uint64_t)p[4] << 32);
    return (uint32_t)((x * 0xCF1BBCDCB7A56463ull) >> (64 - kHashLogD));
}

// The part of a dictionary the encoder matches against: its last D & ~63 bytes (the parse starts
// at a multiple of 64 window positions).  The decoder honours all D bytes.
LZD_FN uint32_t enc_dict_len(uint32_t D) { return D & ~63u; }

// in: the stream (L bytes, 64 zero bytes after them); out: the page's place in the output
// window, C bytes, with the dictionary's D bytes right before out[0].  Returns
// LZ4_decompress_safe_usingDict's value.  The dictionary bytes are only read.
LZD_FN int32_t decode_page(const uint8_t *in, int32_t L, uint8_t *out, int32_t C, int32_t D LZD_LANE_PARAM) {
    if (C == 0) return (L == 1 && LZD_UNI(in[0]) == 0) ? 0 : -1;   // lz4.c:1124
    if (L <= 0) return -1;
    int32_t ip = 0, op = 0;
    // every sequence but the last consumes at least 3 stream bytes
    for (int32_t guard = 0; guard <= L; guard++) {
        const lzd_win w = lzd_win_load(in, (uint32_t)ip LZD_LANE_ARG);
        const uint32_t token = lzd_win_byte(w, in, (uint32_t)ip);
        int32_t lit = (int32_t)(token >> 4);
        ip++;
        if (lit == kRunMaskD) {
            uint32_t s;
            do {
                s = lzd_win_byte(w, in, (uint32_t)ip);
                ip++;
                lit += (int32_t)s;
            } while (ip < L - kRunMaskD && s == 255);
        }
        // terminal literal run, or error (lz4.c:1147-1163)
        if (op + lit > C - kMfLimitD || ip + lit > L - 8) {
            if (ip + lit != L || op + lit > C) return -ip - 1;
            LZD_STRIDED(j, lit) out[op + j] = in[ip + j];
            return op + lit;
        }
        LZD_STRIDED(j, lit) out[op + j] = in[ip + j];
        ip += lit;
        op += lit;
        const int32_t off = (int32_t)(lzd_win_byte(w, in, (uint32_t)ip) | (lzd_win_byte(w, in, (uint32_t)ip + 1) << 8));
        ip += 2;
        if (off > op + D) return -ip - 1;                         // lz4.c:1168, lowLimit = dictionary start
        int32_t ml = (int32_t)(token & 15);
        if (ml == 15) {
            uint32_t s;
            do {
                s = lzd_win_byte(w, in, (uint32_t)ip);
                ip++;
                if (ip > L - kLastLiteralsD) return -ip - 1;      // lz4.c:1177
                ml += (int32_t)s;
            } while (s == 255);
        }
        ml += kMinMatchD;
        if (op + ml > C - kLastLiteralsD) return -ip - 1;         // lz4.c:1186, 1225
        const int32_t src = op - off;                             // >= -D: the dictionary is contiguous in front
        LZD_SYNC();
        if (off == 0) {
            // a malformed stream the reference accepts: it copies bytes it leaves undefined
            // (the size only is defined; these stay what they are)
        } else if (off >= ml || off >= 64) {
            // every source byte of a 64-byte step is final before the step
            LZD_STRIDED(j, ml) out[op + j] = out[src + j];
        } else {
            // self-overlapping: byte j repeats the period-`off` pattern at src
            LZD_STRIDED(j, ml) out[op + j] = out[src + (j % off)];
        }
        LZD_SYNC();
        op += ml;
    }
    return -1;   // unreachable: the chain always ends in a terminal or failing sequence
}

// a parse record (lz_parse.h's uint2): x = pos | cand << 16, y = len -- a match of len bytes at
// window position pos from window position cand < pos
struct Rec {
    uint32_t x, y;
};

// Writes the sequences of n <= 64 records (stream order) after the literal run that starts at
// window position `anchor` to dst + op; `in` is the window (dictionary part, then the page).
// Literals and catch-up stay at or after `anchor`, so inside the page.  Returns false, with
// nothing written, if the bytes would pass cap.
LZD_FN bool emit_records(const Rec *rec, uint32_t n, uint32_t anchor, const uint8_t *in, uint8_t *dst, uint32_t &op,
                         uint32_t cap LZD_LANE_PARAM) {
    LZD_V(bool, sel);
    LZD_V(bool, longrun);
    LZD_V(uint32_t, lstart);
    LZD_V(uint32_t, lit);
    LZD_V(uint32_t, off);
    LZD_V(uint32_t, mc);
    LZD_V(uint32_t, enc);
    LZD_V(uint32_t, incl);
    LZD_EACH {
        D_(sel) = k < n;
        const Rec r = rec[D_(sel) ? k : 0u];
        const Rec rp = rec[k > 0u && D_(sel) ? k - 1u : 0u];
        const uint32_t pos = r.x & 0xFFFFu, cand = r.x >> 16, len = r.y & 0xFFFFu;
        const uint32_t prev_end = k == 0u ? anchor : (rp.x & 0xFFFFu) + (rp.y & 0xFFFFu);
        // catch-up (lz4.c:549): equal bytes before both positions, inside this literal run
        uint32_t room = pos - prev_end;
        if (room > cand) room = cand;
        if (room > kCatchUpD) room = kCatchUpD;
        uint32_t c = 0;
        if (D_(sel))
            while (c < room && in[pos - c - 1u] == in[cand - c - 1u]) c++;
        D_(lstart) = prev_end;
        D_(lit) = D_(sel) ? pos - c - prev_end : 0u;
        D_(off) = pos - cand;
        D_(mc) = len + c - (uint32_t)kMinMatchD;
        const uint32_t lext = D_(lit) >= 15u ? (D_(lit) - 15u) / 255u + 1u : 0u;
        const uint32_t mext = D_(mc) >= 15u ? (D_(mc) - 15u) / 255u + 1u : 0u;
        D_(enc) = D_(sel) ? 1u + lext + D_(lit) + 2u + mext : 0u;
        D_(longrun) = D_(sel) && D_(lit) > kLitLaneD;
    }
    lzd_incl_sum(enc, incl);
    const uint32_t et = LZD_AT(incl, 63u);
    if ((uint64_t)op + et > cap) return false;
    LZD_EACH {
        if (D_(sel)) {
            uint8_t *q = dst + op + (D_(incl) - D_(enc));
            const uint32_t l = D_(lit), m = D_(mc);
            *q++ = (uint8_t)(((l < 15u ? l : 15u) << 4) | (m < 15u ? m : 15u));
            if (l >= 15u) {
                uint32_t rest = l - 15u;
                for (; rest >= 255u; rest -= 255u) *q++ = 255;
                *q++ = (uint8_t)rest;
            }
            const uint32_t own = l < kLitLaneD ? l : kLitLaneD;
            for (uint32_t t = 0; t < own; t++) q[t] = in[D_(lstart) + t];
            q += l;
            *q++ = (uint8_t)D_(off);
            *q++ = (uint8_t)(D_(off) >> 8);
            if (m >= 15u) {
                uint32_t rest = m - 15u;
                for (; rest >= 255u; rest -= 255u) *q++ = 255;
                *q++ = (uint8_t)rest;
            }
        }
    }
    // the rest of the long literal runs, one run after another by the whole wave
    uint64_t longm = LZD_BALLOT(longrun);
    while (longm) {
        const uint32_t s = (uint32_t)__builtin_ctzll(longm);
        longm &= longm - 1u;
        const uint32_t l = LZD_AT(lit, s), ls = LZD_AT(lstart, s);
        const uint32_t lext = (l - 15u) / 255u + 1u;   // l > kLitLaneD >= 15
        uint8_t *q = dst + op + (LZD_AT(incl, s) - LZD_AT(enc, s)) + 1u + lext;
        const int32_t rest = (int32_t)(l - kLitLaneD);
        LZD_STRIDED(j, rest) q[kLitLaneD + (uint32_t)j] = in[ls + kLitLaneD + (uint32_t)j];
    }
    op += et;
    return true;
}

// the block's last literal run in[anchor, end) at dst + op; false if it does not fit cap
LZD_FN bool write_last_literals(const uint8_t *in, uint32_t anchor, uint32_t end, uint8_t *dst, uint32_t &op,
                                uint32_t cap LZD_LANE_PARAM) {
    const uint32_t lit = end - anchor;
    const uint32_t lext = lit >= 15u ? (lit - 15u) / 255u + 1u : 0u;
    const uint32_t total = 1u + lext + lit;
    if ((uint64_t)op + total > cap) return false;
    LZD_STRIDED(j, total) {
        uint32_t v;
        if (j == 0) v = (lit < 15u ? lit : 15u) << 4;
        else if ((uint32_t)j <= lext) v = (uint32_t)j == lext ? (lit - 15u) % 255u : 255u;
        else v = in[anchor + (uint32_t)j - 1u - lext];
        dst[op + (uint32_t)j] = (uint8_t)v;
    }
    op += total;
    return true;
}

}  // namespace lzd
