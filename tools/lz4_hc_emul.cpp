// tools/lz4_hc_emul.cpp -- host emulator of the high-compression LZ4 encoder
// (tyche_amd/csrc/lz4_encode_hc.hip, LZ4_HC=1) for one page at a time: the
// kernel's own per-wave code (lz4_hc_core.h: bucket rings, candidate probing,
// the lazy walk, the exact encoder's sequence writer) with the 64 lanes as
// explicit loops and ballots over arrays.  The page is staged as the kernel
// stages it, next to a zeroed table and zeroed ring counters.  TEST
// INFRASTRUCTURE: tests/test_lz4_hc_emul.py checks its streams on the CPU
// (round trip, end rules, limited output, ratio), and tests/test_gpu_lz4_hc.py
// compares the kernel's bytes with it.
//
//   g++ -O2 -shared -fPIC -o tools/bin/liblz4hcemul.so tools/lz4_hc_emul.cpp
//   int lz4hc_emul_compress(const uint8_t *src, int L, uint8_t *dst, int cap);
//
// -DLZH_WAYS_LOG / LZH_HASH_LOG / LZH_PROBE / LZH_INSERT_SKIPPED build the
// variants of the layout A/B (profiles/README.md).
//
// With -DLZ4_HC_EMUL_MAIN it is a stand-alone program for sanitizer builds
// (g++ -O1 -g -fsanitize=address,undefined -DLZ4_HC_EMUL_MAIN): it replays a
// file of calls recorded by the test (LZ4_HC_EMUL_RECORD=<file> in the test's
// environment) in exactly sized heap buffers, so that a read or write outside
// them is reported, and compares the return values with the recorded ones.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define LZH_HOST 1
#include "../tyche_amd/csrc/lz4_hc_core.h"

extern "C" int lz4hc_emul_compress(const uint8_t *src, int L, uint8_t *dst, int cap) {
    if (L < 0 || L > 65535 || cap < 0) return INT32_MIN;
    // exactly the page: the core reads no byte behind it
    uint8_t *in = new uint8_t[(size_t)L + !L];
    if (L) memcpy(in, src, (size_t)L);
    alignas(16) static thread_local uint16_t table[lzh::kTableEntries];
    static thread_local uint8_t cnt[lzh::kBuckets];
    memset(table, 0, sizeof(table));
    memset(cnt, 0, sizeof(cnt));
    const int rv = lzh::encode_page(in, (uint32_t)L, table, cnt, dst, (uint32_t)cap);
    delete[] in;
    return rv;
}

// the layout this library was built with: ways, hash log, probe bytes, skipped positions inserted
extern "C" void lz4hc_emul_layout(uint32_t *out) {
    out[0] = lzh::kWays;
    out[1] = lzh::kHashLog;
    out[2] = lzh::kProbe;
    out[3] = LZH_INSERT_SKIPPED;
}

#ifdef LZ4_HC_EMUL_MAIN
// Record: u32 source length, u32 capacity, i32 return value, u32 misalignment of the destination,
// then the source bytes.
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
        const uint32_t n = h[0], cap = h[1], da = h[3] & 15u;
        const int32_t want = (int32_t)h[2];
        uint8_t *s = new uint8_t[(size_t)n + !n], *d = new uint8_t[(size_t)cap + da + !(cap + da)];
        if (n && fread(s, 1, n, f) != n) {
            fprintf(stderr, "truncated record\n");
            return 2;
        }
        const int got = lz4hc_emul_compress(s, (int)n, d + da, (int)cap);
        if (got != want) {
            bad++;
            fprintf(stderr, "call %ld: n %u cap %u: got %d, recorded %d\n", calls, n, cap, got, want);
        }
        calls++;
        delete[] s;
        delete[] d;
    }
    fclose(f);
    printf("%ld calls replayed, %ld differ\n", calls, bad);
    return bad ? 1 : 0;
}
#endif
