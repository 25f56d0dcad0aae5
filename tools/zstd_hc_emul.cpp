// tools/zstd_hc_emul.cpp -- host emulator of the high-compression zstd parse
// (zstd_parse_hc_kernel in tyche_amd/csrc/zstd_encode.hip, ZSTD_HC=1) for one
// page at a time: the kernel's own per-wave code (zstd_hc_core.h: bucket rings,
// repeat-offset candidates, the gain, the lazy walk) with the 64 lanes as explicit
// loops and ballots over arrays.  The page is staged as the kernel stages it: 64
// zero bytes behind it and nothing more, next to a zeroed table and zeroed ring
// counters.  The sink is pass A1's (parse_to_area_with): every record becomes a
// sequence (literal length, match length, offset) after the backward extension of
// lz_parse.h's decode_record / back_at.  TEST INFRASTRUCTURE:
// tests/test_zstd_hc_emul.py checks its sequences on the CPU, and
// tests/test_gpu_zstd_hc.py compares the sequences of the kernel's frames with it.
//
//   g++ -O2 -shared -fPIC -o tools/bin/libzstdhcemul.so tools/zstd_hc_emul.cpp
//   int zstdhc_emul_parse(const uint8_t *src, int L, uint32_t *seqs, int cap, uint32_t *last_lit);
//     seqs: cap triples (ll, ml, off); returns the number of sequences (the first cap are written),
//     or INT32_MIN for a bad argument; *last_lit: the literals after the last match.
//
// -DZHC_HASH_LOG / ZHC_PROBE / ZHC_REP_BONUS / ZHC_LAZY1 / ZHC_LAZY2 build the variants of
// profiles/README.md.
//
// With -DZSTD_HC_EMUL_MAIN it is a stand-alone program for sanitizer builds
// (g++ -O1 -g -fsanitize=address,undefined -DZSTD_HC_EMUL_MAIN): it replays a file of
// calls recorded by the test (ZSTD_HC_EMUL_RECORD=<file> in the test's environment) in
// exactly sized heap buffers, so that a read or write outside them is reported, and
// compares the sequence counts and a digest of the sequences with the recorded ones.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define ZHC_HOST 1
#include "../tyche_amd/csrc/zstd_hc_core.h"

namespace {
constexpr uint32_t kPadZ = 64;   // the zero bytes every zstd pass-A1 kernel writes behind the page

// lz_parse.h back_at: the equal bytes before pos and cand, up to 4; 0 when cand < 4
uint32_t back_at(const uint8_t *in, uint32_t pos, uint32_t cand) {
    if (cand < 4u) return 0;
    uint32_t n = 0;
    while (n < 4u && in[pos - 1u - n] == in[cand - 1u - n]) n++;
    return n;
}
}  // namespace

extern "C" int zstdhc_emul_parse(const uint8_t *src, int L, uint32_t *seqs, int cap, uint32_t *last_lit) {
    if (L < 0 || L > 65535 || cap < 0) return INT32_MIN;
    uint8_t *in = new uint8_t[(size_t)L + kPadZ];
    if (L) memcpy(in, src, (size_t)L);
    memset(in + L, 0, kPadZ);
    alignas(16) static thread_local uint16_t table[zhc::kTableEntries];
    static thread_local uint8_t cnt[zhc::kBuckets];
    memset(table, 0, sizeof(table));
    memset(cnt, 0, sizeof(cnt));
    zhc::Rec rec[64];
    int nseq = 0;
    auto sink = [&](const zhc::Rec *r, uint32_t n, uint32_t anchor) -> bool {
        uint32_t prev_end = anchor;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t pos = r[i].x & 0xFFFFu, cand = r[i].x >> 16, len = r[i].y & 0xFFFFu;
            uint32_t k = back_at(in, pos, cand);
            if (k > pos - prev_end) k = pos - prev_end;
            if (k > cand) k = cand;
            if (nseq < cap) {
                seqs[3 * nseq] = pos - k - prev_end;
                seqs[3 * nseq + 1] = len + k;
                seqs[3 * nseq + 2] = pos - cand;
            }
            nseq++;
            prev_end = pos + len;
        }
        return true;
    };
    const uint32_t anchor = zhc::parse_page(in, (uint32_t)L, table, cnt, rec, sink);
    *last_lit = (uint32_t)L - anchor;
    delete[] in;
    return nseq;
}

// the layout this library was built with: ways, hash log, probe bytes, repeat bonus, lazy margins
extern "C" void zstdhc_emul_layout(uint32_t *out) {
    out[0] = zhc::kWays;
    out[1] = zhc::kHashLog;
    out[2] = zhc::kProbe;
    out[3] = zhc::kRepBonus;
    out[4] = ZHC_LAZY1;
    out[5] = ZHC_LAZY2;
}

#ifdef ZSTD_HC_EMUL_MAIN
// Record: u32 source length, u32 sequence count, u32 FNV-1a of the (ll, ml, off) words and the
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
        const uint32_t cap = n / 4u + 1u;
        uint32_t *q = new uint32_t[(size_t)3 * cap];
        uint32_t lastl = 0;
        const int got = zstdhc_emul_parse(s, (int)n, q, (int)cap, &lastl);
        uint32_t d = 2166136261u;
        for (int i = 0; i < 3 * got && got <= (int)cap; i++) d = (d ^ q[i]) * 16777619u;
        d = (d ^ lastl) * 16777619u;
        if (got != (int)h[1] || d != h[2]) {
            bad++;
            fprintf(stderr, "call %ld: n %u: %d sequences, digest %08x; recorded %u, %08x\n", calls, n, got, d, h[1], h[2]);
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
