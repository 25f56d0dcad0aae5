// lz4_large_core.h -- the per-wave algorithms of the large-page LZ4 kernels
// (lz4_encode_large.hip, lz4_decode_large.hip): pages of 65,536 bytes up to
// TYCHE_LZ4_MAX_PAGE (4 MiB), which neither fit the 160 KiB of LDS nor the
// 16-bit positions of the small-page kernels.  Shared verbatim by the gfx950
// kernels and by the host emulator tools/lz4_large_emul.cpp, where the 64 lanes
// are an explicit loop, so that tests/test_lz4_large_emul.py proves the logic
// against the oracle on the CPU.
//
// Both directions keep a *ring* in LDS instead of the page: 128 KiB indexed by
// the position modulo its size, which always holds the 65,535 bytes an LZ4
// offset can reach back plus the bytes in flight.  Nothing is cut into
// segments, so there are no seams and nothing to join: an offset, a literal
// run or a match crosses any 64 KiB line the way it crosses any other byte.
//
//   decode_page  LZ4_decompress_safe (lz4.c:1089-1248) with its return value:
//                the walk of decode_page_serial (lz4_decode.hip), the stream
//                read through a refilled 16 KiB LDS window, the output written
//                to the ring and flushed to dst in aligned 16-byte stores.  dst
//                is never read, so it may be pinned host memory.
//   encode_page  a greedy parse in blocks of 64 positions (the scheme of
//                lz_parse.h: every lane hashes its position and takes the
//                candidate earlier blocks left in the table, or the nearest
//                lane below it with the same hash), the input ring
//                refilled ahead of the scan, 16-bit table entries holding the
//                position modulo 65,536, each sequence written to dst as it is
//                found.  The literals of a run that has left the ring (an
//                incompressible stretch longer than it) are read from the page
//                in HBM.
// Every loop carries a bound derived from the page or stream length, so a
// logic error ends in a wrong answer, never in a wave that does not finish.
//
// The includer defines LZL_HOST (1: lanes are loops over arrays; 0: SIMT, a
// `lane` variable in scope through LZL_LANE_ARG) and, for the device, includes
// lds_io.h first.
#pragma once
#include <stdint.h>
#include <string.h>

#if LZL_HOST
#define LZL_FN static inline
#define LZL_V(T, name) T name[64]                  // one value per lane
#define LZL_V2(T, name, N) T name[N][64]           // N values per lane
#define LZL_EACH for (uint32_t k = 0; k < 64u; k++)
#define V_(name) name[k]
#define V2_(name, r) name[r][k]
#define LZL_AT(name, i) name[i]                    // lane i's value, i wave-uniform
#define LZL_SHFL(name, i) name[i]                  // lane i's value, i per lane
#define LZL_BALLOT(name) lzl_ballot_host(name)
#define LZL_UNROLL
#define LZL_SYNC() do {} while (0)
#define LZL_LANE_PARAM
#define LZL_LANE_ARG
struct lzl_vec {
    uint8_t b[16];
};
LZL_FN uint64_t lzl_ballot_host(const bool *p) {
    uint64_t m = 0;
    for (uint32_t k = 0; k < 64u; k++) m |= (uint64_t)p[k] << k;
    return m;
}
// the 16 bytes at base + a; base[0, n) is all that exists (the kernel reads the whole aligned
// vector, which never crosses a page boundary; its bytes outside the range are never used)
LZL_FN lzl_vec lzl_gload16(const uint8_t *base, int64_t n, int64_t a) {
    lzl_vec v;
    for (int j = 0; j < 16; j++) v.b[j] = (a + j >= 0 && a + j < n) ? base[a + j] : 0;
    return v;
}
LZL_FN uint32_t lzl_gload8(const uint8_t *p) { return *p; }
LZL_FN void lzl_gstore16(uint8_t *p, const lzl_vec &v) { memcpy(p, v.b, 16); }
LZL_FN lzl_vec lzl_lds_ld16(const uint8_t *p) {
    lzl_vec v;
    memcpy(v.b, p, 16);
    return v;
}
LZL_FN void lzl_lds_st16(uint8_t *p, const lzl_vec &v) { memcpy(p, v.b, 16); }
#else
#define LZL_FN __device__ __forceinline__
#define LZL_V(T, name) T name
#define LZL_V2(T, name, N) T name[N]
#define LZL_EACH if (const uint32_t k = lane; true)
#define V_(name) name
#define V2_(name, r) name[r]
#define LZL_AT(name, i) tyche::rdlane((uint32_t)(name), i)
// (every LZL_SHFL stands where all 64 lanes execute it, never inside a per-lane condition)
#define LZL_SHFL(name, i) ((uint32_t)__shfl((int)(name), (int)(i)))
#define LZL_BALLOT(name) __ballot(name)
#define LZL_UNROLL _Pragma("unroll")
#define LZL_SYNC() __builtin_amdgcn_wave_barrier()
#define LZL_LANE_PARAM , uint32_t lane
#define LZL_LANE_ARG , lane
typedef tyche::u32x4 lzl_vec;
LZL_FN lzl_vec lzl_gload16(const uint8_t *base, int64_t, int64_t a) { return tyche::gload_nt((const tyche::u32x4 *)(base + a)); }
LZL_FN uint32_t lzl_gload8(const uint8_t *p) { return *(const __attribute__((address_space(1))) uint8_t *)(uintptr_t)p; }
LZL_FN void lzl_gstore16(uint8_t *p, const lzl_vec &v) { __builtin_nontemporal_store(v, (tyche::u32x4 *)p); }
LZL_FN lzl_vec lzl_lds_ld16(const uint8_t *p) { return *(const tyche::u32x4 *)p; }
LZL_FN void lzl_lds_st16(uint8_t *p, const lzl_vec &v) { *(tyche::u32x4 *)p = v; }
#endif

namespace lzl {

constexpr uint32_t kMaxPage = 4u << 20;              // TYCHE_LZ4_MAX_PAGE
constexpr uint32_t kRing = 128u << 10;               // the page ring (both directions)
constexpr uint32_t kRingMask = kRing - 1u;
constexpr uint32_t kWin = 16u << 10;                 // the decoder's stream window (a ring too)
constexpr uint32_t kWinMask = kWin - 1u;
constexpr uint32_t kRefillVecs = 8;                  // 16-byte vectors per lane and refill: 8 KiB per wave
constexpr uint32_t kRefill = kRefillVecs * 64u * 16u;
constexpr uint32_t kFlushAt = 16u << 10;             // unflushed output that triggers a flush
constexpr uint32_t kHashLog = 13;                    // the encoder's table: 8192 16-bit entries, as lz4.c's byU16
constexpr uint32_t kTableSize = 1u << kHashLog;
constexpr uint32_t kMinGain = 1;                     // a match must be this much longer than 4 bytes: one of 4 costs
                                                     // 3 bytes and a token's worth of broken literal run, and
                                                     // taking it hides the longer match one byte on
constexpr uint32_t kJump = 1024;                     // a match that ends this far past a block's start: the scan
                                                     // resumes 64 positions before its end, not at the next block

LZL_FN uint32_t ctz64(uint64_t m) { return (uint32_t)__builtin_ctzll(m); }
LZL_FN uint32_t hash4(uint32_t w) { return (w * 2654435761u) >> (32 - kHashLog); }

// The four bytes at ring index i .. i + 3 (modulo the ring), as aligned dwords.
LZL_FN uint32_t ring32(const uint8_t *ring, uint32_t i) {
    const uint32_t a = i & ~3u, s = 8u * (i & 3u);
    const uint32_t lo = *(const uint32_t *)(ring + (a & kRingMask)), hi = *(const uint32_t *)(ring + ((a + 4u) & kRingMask));
    return s ? (lo >> s) | (hi << (32u - s)) : lo;
}

// ------------------------------------------------------------------ decoder

// Positions are kept in two shifted spaces, so that a 16-byte vector aligned in
// global memory is aligned in LDS too: stream byte p lives at win[(p + a0) &
// kWinMask], a0 = src & 15; output byte p at ring[(p + d0) & kRingMask], d0 =
// dst & 15.
struct Dec {
    const uint8_t *src;
    uint8_t *dst;
    uint8_t *ring, *win;
    uint32_t L, C, a0, d0;
    uint32_t wtop;   // the window holds the shifted stream positions [wtop - kWin, wtop); a multiple of 16
    uint32_t fl;     // output bytes [0, fl) are in dst
};

// Stream bytes up to position `need` (exclusive), or to the stream's end, are
// in the window afterwards.  The caller's ip is never more than kWin - kRefill -
// 256 behind `need`.
LZL_FN void win_need(Dec &d, uint32_t need LZL_LANE_PARAM) {
    const uint32_t end = d.a0 + d.L;
    uint32_t want = need + d.a0;
    if (want > end) want = end;
    for (uint32_t r = 0; d.wtop < want && r <= d.L / kRefill + 1u; r++) {
        LZL_V2(lzl_vec, v, kRefillVecs);
        LZL_EACH {
            LZL_UNROLL
            for (uint32_t j = 0; j < kRefillVecs; j++) {
                const uint32_t t = d.wtop + 16u * (j * 64u + k);
                if (t < end) V2_(v, j) = lzl_gload16(d.src, (int64_t)d.L, (int64_t)t - (int64_t)d.a0);
            }
        }
        LZL_EACH {
            LZL_UNROLL
            for (uint32_t j = 0; j < kRefillVecs; j++) {
                const uint32_t t = d.wtop + 16u * (j * 64u + k);
                if (t < end) lzl_lds_st16(d.win + (t & kWinMask), V2_(v, j));
            }
        }
        d.wtop += kRefill;
        LZL_SYNC();
    }
}

// stream byte p (in the window); 0 at and past the stream's end
LZL_FN uint32_t sbyte(const Dec &d, uint32_t p) { return p < d.L ? d.win[(p + d.a0) & kWinMask] : 0u; }

// Output bytes [fl, op) go to dst: all of them when `final`, else up to the
// last 16-byte line of dst that is complete.  Aligned 16-byte stores but for
// the page's first and last bytes; dst is only ever written, below dst + C.
LZL_FN void flush(Dec &d, uint32_t op, bool final LZL_LANE_PARAM) {
    uint32_t end = op;
    if (!final) {
        const uint32_t e = (op + d.d0) & ~15u;
        end = e > d.d0 ? e - d.d0 : 0u;
    }
    if (end <= d.fl) return;
    if ((d.fl + d.d0) & 15u) {   // the bytes before dst's first 16-byte line (fl == 0 only)
        uint32_t he = ((d.fl + d.d0 + 15u) & ~15u) - d.d0;
        if (he > end) he = end;
        LZL_EACH {
            if (d.fl + k < he) d.dst[d.fl + k] = d.ring[(d.fl + k + d.d0) & kRingMask];
        }
        d.fl = he;
    }
    const uint32_t nvec = (end - d.fl) >> 4;
    for (uint32_t v0 = 0; v0 < nvec; v0 += 4u * 64u) {
        LZL_V2(lzl_vec, x, 4);
        LZL_EACH {
            LZL_UNROLL
            for (uint32_t j = 0; j < 4u; j++) {
                const uint32_t v = v0 + j * 64u + k;
                if (v < nvec) V2_(x, j) = lzl_lds_ld16(d.ring + ((d.fl + d.d0 + 16u * v) & kRingMask));
            }
        }
        LZL_EACH {
            LZL_UNROLL
            for (uint32_t j = 0; j < 4u; j++) {
                const uint32_t v = v0 + j * 64u + k;
                if (v < nvec) lzl_gstore16(d.dst + d.fl + 16u * v, V2_(x, j));
            }
        }
    }
    d.fl += 16u * nvec;
    if (d.fl < end) {   // final: the bytes after dst's last complete line (< 16)
        LZL_EACH {
            if (d.fl + k < end) d.dst[d.fl + k] = d.ring[(d.fl + k + d.d0) & kRingMask];
        }
        d.fl = end;
    }
}

// The stream src[0, L) into dst[0, C): the return of LZ4_decompress_safe(src,
// dst, L, C) -- the decoded size, or -(stream position) - 1 where the reference
// gives up (lz4.c:1147-1163, :1168, :1176, :1225).  ring: kRing bytes, win: kWin
// bytes, both 16-byte aligned.  After an error dst[0, C) holds an unspecified
// part of the output.
LZL_FN int32_t decode_page(const uint8_t *src, uint32_t L, uint8_t *dst, uint32_t C, uint8_t *ring,
                           uint8_t *win LZL_LANE_PARAM) {
    if (C == 0u) return (L == 1u && src[0] == 0u) ? 0 : -1;
    if (L == 0u) return -1;
    Dec d;
    d.src = src;
    d.dst = dst;
    d.ring = ring;
    d.win = win;
    d.L = L;
    d.C = C;
    d.a0 = (uint32_t)((uintptr_t)src & 15u);
    d.d0 = (uint32_t)((uintptr_t)dst & 15u);
    d.wtop = 0;
    d.fl = 0;
    uint32_t ip = 0, op = 0;
    for (uint32_t it = 0; it <= L; it++) {   // every sequence takes at least one stream byte
        // one read of the 64 stream bytes from the token on serves the token, short literals and
        // the offset (wbyte: a lane of it, or the window in LDS past its end)
        win_need(d, ip + 64u LZL_LANE_ARG);
        const uint32_t ip0 = ip;
        LZL_V(uint32_t, wv);
        LZL_EACH V_(wv) = sbyte(d, ip0 + k);
#define LZL_WBYTE(p) ((p) - ip0 < 64u ? (uint32_t)LZL_AT(wv, (p) - ip0) : sbyte(d, (p)))
        const uint32_t token = LZL_AT(wv, 0u);
        ip++;
        uint64_t lit = token >> 4;
        if (lit == 15u) {
            // do { s = *ip++; lit += s; } while (ip < iend - RUN_MASK && s == 255), 64 bytes per step
            bool more = true;
            for (uint32_t r = 0; more && r <= L / 64u + 1u; r++) {
                win_need(d, ip + 64u LZL_LANE_ARG);
                LZL_V(uint32_t, bv);
                LZL_V(bool, stop);
                LZL_EACH {
                    const uint32_t p = ip + k, b = sbyte(d, p);
                    V_(bv) = b;
                    V_(stop) = b != 255u || (uint64_t)p + 1u + 15u >= L;
                }
                const uint64_t B = LZL_BALLOT(stop);
                if (B) {
                    const uint32_t f = ctz64(B);
                    lit += 255u * f + LZL_AT(bv, f);
                    ip += f + 1u;
                    more = false;
                } else {
                    lit += 255u * 64u;
                    ip += 64u;
                }
            }
        }
        // the last literals, or an error (lz4.c:1147-1163)
        const bool last = (int64_t)op + (int64_t)lit > (int64_t)C - 12 || (int64_t)ip + (int64_t)lit > (int64_t)L - 8;
        if (last && ((uint64_t)ip + lit != L || (uint64_t)op + lit > C)) return -(int32_t)ip - 1;
        // the literals, 64 bytes per step: window -> ring
        uint32_t rem = (uint32_t)lit;   // <= L here
        if (rem && ip - ip0 + rem <= 64u) {   // all in the bytes already read
            const uint32_t sh = ip - ip0;
            LZL_EACH {
                if (k >= sh && k < sh + rem) ring[(op + k - sh + d.d0) & kRingMask] = (uint8_t)V_(wv);
            }
            LZL_SYNC();
            ip += rem;
            op += rem;
            rem = 0;
            if (op - d.fl >= kFlushAt) flush(d, op, false LZL_LANE_ARG);
        }
        for (uint32_t r = 0; rem && r <= L / 64u + 1u; r++) {
            const uint32_t n = rem < 64u ? rem : 64u;
            win_need(d, ip + n LZL_LANE_ARG);
            LZL_V(uint32_t, t);
            LZL_EACH V_(t) = sbyte(d, ip + k);
            LZL_EACH {
                if (k < n) ring[(op + k + d.d0) & kRingMask] = (uint8_t)V_(t);
            }
            LZL_SYNC();
            ip += n;
            op += n;
            rem -= n;
            if (op - d.fl >= kFlushAt) flush(d, op, false LZL_LANE_ARG);
        }
        if (last) {
            flush(d, op, true LZL_LANE_ARG);
            return (int32_t)op;
        }
        win_need(d, ip + 64u LZL_LANE_ARG);
        const uint32_t off = LZL_WBYTE(ip) | (LZL_WBYTE(ip + 1u) << 8);
#undef LZL_WBYTE
        ip += 2u;
        if (off > op) return -(int32_t)ip - 1;   // lz4.c:1168
        uint64_t ml = token & 15u;
        if (ml == 15u) {
            // do { s = *ip++; if (ip > iend - LASTLITERALS) error; ml += s; } while (s == 255)
            bool more = true;
            for (uint32_t r = 0; more && r <= L / 64u + 1u; r++) {
                win_need(d, ip + 64u LZL_LANE_ARG);
                LZL_V(uint32_t, bv);
                LZL_V(bool, err);
                LZL_V(bool, stop);
                LZL_EACH {
                    const uint32_t p = ip + k, b = sbyte(d, p);
                    V_(bv) = b;
                    V_(err) = (uint64_t)p + 1u + 5u > L;
                    V_(stop) = V_(err) || b != 255u;
                }
                const uint64_t B = LZL_BALLOT(stop), E = LZL_BALLOT(err);
                if (B) {
                    const uint32_t f = ctz64(B);
                    ip += f + 1u;
                    if ((E >> f) & 1ull) return -(int32_t)ip - 1;   // lz4.c:1176
                    ml += 255u * f + LZL_AT(bv, f);
                    more = false;
                } else {
                    ml += 255u * 64u;
                    ip += 64u;
                }
            }
        }
        ml += 4u;
        if ((int64_t)op + (int64_t)ml > (int64_t)C - 5) return -(int32_t)ip - 1;   // lz4.c:1225
        // the match, 64 bytes per step, from the ring into the ring.  Offsets below 64 repeat the
        // `off` bytes before the step's start: always the latest period, which is still in the ring
        // however long the match is.  (Offset 0 copies bytes the reference leaves undefined.)
        const uint32_t period = off ? off : 1u;
        rem = (uint32_t)ml;   // <= C here
        for (uint32_t r = 0; rem && r <= C / 64u + 1u; r++) {
            const uint32_t n = rem < 64u ? rem : 64u;
            LZL_V(uint32_t, t);
            LZL_EACH {
                const uint32_t s = op - off + (off >= 64u ? k : k % period);
                V_(t) = ring[(s + d.d0) & kRingMask];
            }
            LZL_SYNC();
            LZL_EACH {
                if (k < n) ring[(op + k + d.d0) & kRingMask] = (uint8_t)V_(t);
            }
            LZL_SYNC();
            op += n;
            rem -= n;
            if (op - d.fl >= kFlushAt) flush(d, op, false LZL_LANE_ARG);
        }
    }
    return -1;   // not reached: a stream of L bytes holds at most L sequences
}

// ------------------------------------------------------------------ encoder

// Page byte p lives at ring[(p + s0) & kRingMask], s0 = src & 15.
struct Enc {
    const uint8_t *src;
    uint8_t *dst;
    uint8_t *ring;
    uint32_t L, cap, s0;
    uint32_t rtop;   // the ring holds the shifted page positions [rtop - kRing, rtop); a multiple of 16
    uint32_t op;     // bytes of the stream so far (may pass cap: nothing is stored there, the result is 0)
};

// Page bytes up to position `need` (exclusive), or to the page's end, are in
// the ring afterwards.  Callers keep `need` within 8 KiB + 1 KiB of the oldest
// position they still read plus 65,535, so that history survives the refill.
LZL_FN void in_need(Enc &e, uint32_t need LZL_LANE_PARAM) {
    const uint32_t end = e.s0 + e.L;
    uint32_t want = need + e.s0;
    if (want > end) want = end;
    for (uint32_t r = 0; e.rtop < want && r <= e.L / kRefill + 1u; r++) {
        LZL_V2(lzl_vec, v, kRefillVecs);
        LZL_EACH {
            LZL_UNROLL
            for (uint32_t j = 0; j < kRefillVecs; j++) {
                const uint32_t t = e.rtop + 16u * (j * 64u + k);
                if (t < end) V2_(v, j) = lzl_gload16(e.src, (int64_t)e.L, (int64_t)t - (int64_t)e.s0);
            }
        }
        LZL_EACH {
            LZL_UNROLL
            for (uint32_t j = 0; j < kRefillVecs; j++) {
                const uint32_t t = e.rtop + 16u * (j * 64u + k);
                if (t < end) lzl_lds_st16(e.ring + (t & kRingMask), V2_(v, j));
            }
        }
        e.rtop += kRefill;
        LZL_SYNC();
    }
}

LZL_FN uint32_t in32(const Enc &e, uint32_t p) { return ring32(e.ring, p + e.s0); }
LZL_FN uint32_t in8(const Enc &e, uint32_t p) { return e.ring[(p + e.s0) & kRingMask]; }

LZL_FN void put(Enc &e, uint32_t j, uint32_t v) {
    if (j < e.cap) e.dst[j] = (uint8_t)v;
}

// n bytes at stream position e.op: `first`, then 255s, then `lastv` (a token or
// the offset's low byte, and the length bytes that follow it)
LZL_FN void put_run(Enc &e, uint32_t n, uint32_t first, uint32_t lastv LZL_LANE_PARAM) {
    for (uint32_t j0 = 0; j0 < n; j0 += 64u) {
        LZL_EACH {
            const uint32_t j = j0 + k;
            if (j < n) put(e, e.op + j, j == 0u ? first : j == n - 1u ? lastv : 255u);
        }
    }
    e.op += n;
}

// One sequence at e.op: token, literal-length bytes, the literals page[anchor,
// anchor + lit), and for a match the offset and the match-length bytes (mc =
// match length - 4).  Literals still in the ring come from it; the front of a
// run that has left it comes from the page in HBM.
LZL_FN void put_sequence(Enc &e, uint32_t anchor, uint32_t lit, bool match, uint32_t off, uint32_t mc LZL_LANE_PARAM) {
    const uint32_t llb = lit >= 15u ? (lit - 15u) / 255u + 1u : 0u;
    const uint32_t token = ((lit < 15u ? lit : 15u) << 4) | (match ? (mc < 15u ? mc : 15u) : 0u);
    put_run(e, 1u + llb, token, llb ? (lit - 15u) % 255u : token LZL_LANE_ARG);
    if (anchor + e.s0 + kRing >= e.rtop) {
        // the whole run is still in the ring (the choice is the wave's, not a lane's: a per-lane
        // choice of address space would make every one of these reads a flat load, which waits
        // for the stream's outstanding stores)
        for (uint32_t j0 = 0; j0 < lit; j0 += 64u) {
            LZL_EACH {
                const uint32_t j = j0 + k;
                if (j < lit) put(e, e.op + j, in8(e, anchor + j));
            }
        }
    } else {
        // its front has left the ring: all of it from the page in HBM, 512 bytes in flight
        for (uint32_t j0 = 0; j0 < lit; j0 += 8u * 64u) {
            LZL_V2(uint32_t, t, 8);
            LZL_EACH {
                LZL_UNROLL
                for (uint32_t r = 0; r < 8u; r++) {
                    const uint32_t j = j0 + r * 64u + k;
                    if (j < lit) V2_(t, r) = lzl_gload8(e.src + anchor + j);
                }
            }
            LZL_EACH {
                LZL_UNROLL
                for (uint32_t r = 0; r < 8u; r++) {
                    const uint32_t j = j0 + r * 64u + k;
                    if (j < lit) put(e, e.op + j, V2_(t, r));
                }
            }
        }
    }
    e.op += lit;
    if (match) {
        const uint32_t mlb = mc >= 15u ? (mc - 15u) / 255u + 1u : 0u;
        put_run(e, 1u, off & 0xFFu, off & 0xFFu LZL_LANE_ARG);
        put_run(e, 1u + mlb, off >> 8, mlb ? (mc - 15u) % 255u : off >> 8 LZL_LANE_ARG);
    }
}

// The page src[0, L) as one LZ4 block into dst[0, cap): its size, or 0 when it
// does not fit (nothing at or past dst + cap is written).  ring: kRing bytes,
// 16-byte aligned; table: kTableSize entries, zeroed.
//
// A table entry is the position modulo 65,536; the candidate of position q is
// q - ((q - entry) & 0xFFFF), the one position within an offset's reach that
// the entry can mean.  A stale or never-written entry names some other position
// there, and the four bytes read at it decide, as they do for a hash collision.
// When several lanes of a block share a slot the highest one stores (the others
// are masked), so the stream does not depend on the order stores land in.
LZL_FN int32_t encode_page(const uint8_t *src, uint32_t L, uint8_t *dst, uint32_t cap, uint8_t *ring,
                           uint16_t *table LZL_LANE_PARAM) {
    Enc e;
    e.src = src;
    e.dst = dst;
    e.ring = ring;
    e.L = L;
    e.cap = cap;
    e.s0 = (uint32_t)((uintptr_t)src & 15u);
    e.rtop = 0;
    e.op = 0;
    uint32_t anchor = 0;
    if (L >= 13u) {
        const uint32_t mflimit = L - 12u, matchlimit = L - 5u;
        uint32_t base = 0;
        // every round moves base up by at least 64
        for (uint32_t it = 0; base <= mflimit && it <= L / 64u + 1u; it++) {
            in_need(e, base + 64u + 8u LZL_LANE_ARG);
            LZL_V(uint32_t, w);
            LZL_V(uint32_t, h);
            LZL_V(bool, valid);
            LZL_EACH {
                V_(w) = in32(e, base + k);
                V_(valid) = base + k <= mflimit;
                V_(h) = hash4(V_(w));
            }
            // same: the valid lanes whose hash equals this lane's, one ballot per hash bit
            LZL_V(uint64_t, same);
            {
                const uint64_t V = LZL_BALLOT(valid);
                LZL_EACH V_(same) = V;
                for (uint32_t b = 0; b < kHashLog; b++) {
                    LZL_V(bool, bit);
                    LZL_EACH V_(bit) = ((V_(h) >> b) & 1u) != 0u;
                    const uint64_t bal = LZL_BALLOT(bit);
                    LZL_EACH V_(same) &= V_(bit) ? bal : ~bal;
                }
            }
            // the candidate: the nearest lane below with the same hash (it would have taken the
            // slot before this position looked), else -- or when that one's bytes differ -- what
            // earlier blocks left in the table
            LZL_V(uint32_t, pl);
            LZL_EACH {
                const uint64_t below = V_(same) & ((1ull << k) - 1ull);
                V_(pl) = below ? 63u - (uint32_t)__builtin_clzll(below) : k;
            }
            LZL_V(uint32_t, wl);
            LZL_EACH V_(wl) = LZL_SHFL(w, V_(pl));
            LZL_V(uint32_t, cand);
            LZL_V(bool, ok);
            LZL_EACH {
                const uint32_t q = base + k;
                const uint32_t dist = (q - table[V_(h)]) & 0xFFFFu;
                const bool near = V_(pl) != k && V_(wl) == V_(w);
                V_(cand) = near ? base + V_(pl) : q - dist;
                V_(ok) = V_(valid) && (near || (dist != 0u && dist <= q && in32(e, q - dist) == V_(w)));
            }
            LZL_SYNC();
            const uint64_t M = LZL_BALLOT(ok);
            uint32_t cur = anchor > base ? anchor : base;
            // the lanes inside a match, which leave the table alone (below)
            uint64_t cov = cur - base >= 64u ? ~0ull : (1ull << (cur - base)) - 1ull;
            for (uint32_t n = 0; n <= 64u; n++) {   // every round moves cur up
                if (cur - base >= 64u) break;
                const uint64_t Mm = M & ~((1ull << (cur - base)) - 1ull);
                if (!Mm) break;
                const uint32_t m = ctz64(Mm);
                uint32_t pos = base + m, cnd = LZL_AT(cand, m);
                // catch-up (lz4.c:549), at most 64 bytes
                uint32_t back;
                {
                    const uint32_t lim = pos - anchor < cnd ? pos - anchor : cnd;
                    LZL_V(bool, ne);
                    LZL_EACH V_(ne) = k >= lim || in8(e, pos - 1u - k) != in8(e, cnd - 1u - k);
                    const uint64_t B = LZL_BALLOT(ne);
                    back = B ? ctz64(B) : 64u;
                }
                // the match length past its first four bytes, 256 bytes per step, never past matchlimit
                uint32_t extra = 0;
                for (uint32_t step = 0; step <= L / 256u + 1u; step++) {
                    in_need(e, pos + 4u + 256u * step + 256u + 8u LZL_LANE_ARG);
                    LZL_V(uint32_t, nb);
                    LZL_V(bool, stop);
                    LZL_EACH {
                        const uint32_t dd = 4u + 256u * step + 4u * k, p = pos + dd;
                        uint32_t c = 0;
                        if (p < matchlimit) {
                            const uint32_t x = in32(e, p) ^ in32(e, cnd + dd);
                            c = x ? (uint32_t)__builtin_ctz(x) >> 3 : 4u;
                            if (c > matchlimit - p) c = matchlimit - p;
                        }
                        V_(nb) = c;
                        V_(stop) = c < 4u;
                    }
                    const uint64_t B = LZL_BALLOT(stop);
                    if (B) {
                        const uint32_t f = ctz64(B);
                        extra = 256u * step + 4u * f + LZL_AT(nb, f);
                        break;
                    }
                }
                const uint32_t end = pos + 4u + extra;
                if (back + extra < kMinGain) {
                    cur = pos + 1u;
                    continue;
                }
                pos -= back;
                cnd -= back;
                put_sequence(e, anchor, pos - anchor, true, pos - cnd, end - pos - 4u LZL_LANE_ARG);
                if (e.op > cap) return 0;
                anchor = end;
                cur = end;
                // pos + 1 .. end - 1 but end - 2 (lz4.c:615 puts that one in the table)
                const uint32_t a = pos + 1u > base ? pos + 1u - base : 0u, b = end - base;
                if (a < 64u) cov |= ~((1ull << a) - 1ull) & (b >= 64u ? ~0ull : (1ull << b) - 1ull);
                if (b >= 2u && b - 2u < 64u && end - 2u > pos) cov &= ~(1ull << (b - 2u));
            }
            // As in the reference, only the positions a search visited enter the table, not those
            // inside matches: on compressible pages that is a small part of all positions, so an
            // entry lives long enough for matches tens of KiB back to be found.
            LZL_EACH {
                if (V_(valid) && !((cov >> k) & 1ull) && !(V_(same) & ~cov & ~((2ull << k) - 1ull))) table[V_(h)] = (uint16_t)(base + k);
            }
            LZL_SYNC();
            base = anchor > base + kJump ? anchor - 64u : base + 64u;
        }
    }
    in_need(e, L LZL_LANE_ARG);
    put_sequence(e, anchor, L - anchor, false, 0u, 0u LZL_LANE_ARG);   // the last literals
    return e.op > cap ? 0 : (int32_t)e.op;
}

}  // namespace lzl
