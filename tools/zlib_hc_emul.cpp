// tools/zlib_hc_emul.cpp -- host emulator of the high-compression zlib parse
// (zlib_deflate_hc_kernel in tyche_amd/csrc/zlib_deflate_hc.hip, ZLIB_HC=1) for one
// page at a time: the kernel's own per-wave code (zlib_hc_core.h: bucket rings,
// the lower-lane candidate, the gain, the lazy walk, the backward extension) with
// the 64 lanes as explicit loops and ballots over arrays.  The page is staged as
// the kernel stages it: 64 zero bytes behind it and nothing more, next to a
// zeroed table and zeroed ring counters.  The records are the ones the kernel's
// sink stores for passes 2 and 3: (literal start, literal length, match length,
// distance).  TEST INFRASTRUCTURE: tests/test_zlib_hc_emul.py checks its records
// on the CPU, and tests/test_gpu_zlib_hc.py compares the symbols of the kernel's
// streams with them.
//
//   g++ -O2 -shared -fPIC -o tools/bin/libzlibhcemul.so tools/zlib_hc_emul.cpp
//   int zlibhc_emul_parse(const uint8_t *src, int L, uint32_t *recs, int cap, uint32_t *last_lit);
//     recs: cap quadruples (ls, ll, ml, dist); returns the number of records (the first cap are
//     written), or INT32_MIN for a bad argument; *last_lit: the literals after the last match.
//   int zlibhc_emul_trace(const uint8_t *src, int L, uint32_t *out, int cap);
//     out: cap blocks of 196 words (base, cursor at the block's start, the standing lanes' mask low
//     and high, then per lane gain + kGainBase, length, candidate); returns the number of blocks.
//
// -DZLH_HASH_LOG / ZLH_PROBE / ZLH_LEN_W / ZLH_FAR3 / ZLH_FAR4 / ZLH_LAZY1 / ZLH_LAZY2 /
// ZLH_LOWER_LANE / ZLH_INSERT_SKIPPED build the variants of profiles/README.md.
//
// With -DZLIB_HC_EMUL_MAIN it is a stand-alone program for sanitizer builds
// (g++ -O1 -g -fsanitize=address,undefined -DZLIB_HC_EMUL_MAIN): it replays a file of
// calls recorded by the test (ZLIB_HC_EMUL_RECORD=<file> in the test's environment) in
// exactly sized heap buffers, so that a read or write outside them is reported, and
// compares the record counts and a digest of the records with the recorded ones.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {
thread_local uint32_t *g_trace = nullptr;
thread_local int g_trace_cap = 0, g_trace_n = 0;
}  // namespace
#define ZLH_TRACE(base, gn, ln, cd, E, cursor)                                   \
    if (g_trace) {                                                               \
        if (g_trace_n < g_trace_cap) {                                           \
            uint32_t *t_ = g_trace + (size_t)196 * g_trace_n;                    \
            t_[0] = base, t_[1] = cursor, t_[2] = (uint32_t)(E), t_[3] = (uint32_t)((E) >> 32); \
            for (uint32_t k = 0; k < 64u; k++) t_[4 + 3 * k] = gn[k], t_[5 + 3 * k] = ln[k], t_[6 + 3 * k] = cd[k]; \
        }                                                                        \
        g_trace_n++;                                                             \
    }

#define ZLH_HOST 1
#include "../tyche_amd/csrc/zlib_hc_core.h"

namespace {
constexpr uint32_t kPadZ = 64;   // the zero bytes the kernel writes behind the page

int parse(const uint8_t *src, int L, uint32_t *recs, int cap, uint32_t *last_lit) {
    uint8_t *in = new uint8_t[(size_t)L + kPadZ];
    if (L) memcpy(in, src, (size_t)L);
    memset(in + L, 0, kPadZ);
    uint16_t *table = new uint16_t[zlh::kTableEntries]();
    uint8_t *cnt = new uint8_t[zlh::kBuckets]();
    zlh::Rec rec[64];
    int nrec = 0;
    auto sink = [&](const zlh::Rec *r, uint32_t n) -> bool {
        for (uint32_t i = 0; i < n; i++) {
            if (nrec < cap) {
                recs[4 * nrec] = r[i].x & 0xFFFFu;
                recs[4 * nrec + 1] = r[i].x >> 16;
                recs[4 * nrec + 2] = r[i].y & 0xFFFFu;
                recs[4 * nrec + 3] = r[i].y >> 16;
            }
            nrec++;
        }
        return true;
    };
    const uint32_t anchor = zlh::parse_page(in, (uint32_t)L, table, cnt, rec, sink);
    if (last_lit) *last_lit = (uint32_t)L - anchor;
    delete[] in;
    delete[] table;
    delete[] cnt;
    return nrec;
}
}  // namespace

extern "C" int zlibhc_emul_parse(const uint8_t *src, int L, uint32_t *recs, int cap, uint32_t *last_lit) {
    if (L < 0 || L > 65535 || cap < 0) return INT32_MIN;
    return parse(src, L, recs, cap, last_lit);
}

extern "C" int zlibhc_emul_trace(const uint8_t *src, int L, uint32_t *out, int cap) {
    if (L < 0 || L > 65535 || cap < 0) return INT32_MIN;
    g_trace = out;
    g_trace_cap = cap;
    g_trace_n = 0;
    parse(src, L, nullptr, 0, nullptr);
    g_trace = nullptr;
    return g_trace_n;
}

// the layout this library was built with
extern "C" void zlibhc_emul_layout(uint32_t *out) {
    out[0] = zlh::kWays;
    out[1] = zlh::kHashLog;
    out[2] = zlh::kProbe;
    out[3] = zlh::kLenW;
    out[4] = zlh::kFar3;
    out[5] = zlh::kFar4;
    out[6] = zlh::kLazy1;
    out[7] = zlh::kLazy2;
    out[8] = zlh::kGainBase;
    out[9] = zlh::kStride;
    out[10] = zlh::kBackMax;
}

#ifdef ZLIB_HC_EMUL_MAIN
// Record: u32 source length, u32 record count, u32 FNV-1a of the (ls, ll, ml, dist) words and the
// last literal run, u32 0, then the source bytes.
int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <recorded calls>\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    uint32_t h[4];
    long calls = 0, bad = 0;
    while (fread(h, sizeof(h), 1, f) == 1) {
        const uint32_t n = h[0];
        uint8_t *s = new uint8_t[(size_t)n + !n];
        if (n && fread(s, 1, n, f) != n) {
            fprintf(stderr, "truncated record\n");
            return 2;
        }
        const uint32_t cap = n / 3u + 1u;
        uint32_t *q = new uint32_t[(size_t)4 * cap];
        uint32_t lastl = 0;
        const int got = zlibhc_emul_parse(s, (int)n, q, (int)cap, &lastl);
        uint32_t d = 2166136261u;
        for (int i = 0; i < 4 * got && got <= (int)cap; i++) d = (d ^ q[i]) * 16777619u;
        d = (d ^ lastl) * 16777619u;
        if (got != (int)h[1] || d != h[2]) {
            bad++;
            fprintf(stderr, "call %ld: n %u: %d records, digest %08x; recorded %u, %08x\n", calls, n, got, d, h[1], h[2]);
        }
        calls++;
        delete[] s;
        delete[] q;
    }
    fclose(f);
    printf("%ld calls replayed, %ld differ\n", calls, bad);
    return bad ? 1 : 0;
}
#endif
