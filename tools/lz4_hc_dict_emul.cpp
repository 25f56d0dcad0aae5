// tools/lz4_hc_dict_emul.cpp -- host emulator of the high-compression LZ4
// dictionary encoder (tyche_amd/csrc/lz4_encode_hc_dict.hip, LZ4_HC_DICT=1) for
// one page at a time: the kernel's own per-wave code (lz4_hc_core.h: seed_window,
// encode_window) with the 64 lanes as explicit loops.  The window is built as the
// kernel builds it -- the dictionary's last D' = D & ~63 bytes, then the page --
// and the rings start from the seed, computed here from the tail alone as the
// library computes it once per handle (lz4_hc_dict_seed.hip).  TEST
// INFRASTRUCTURE: tests/test_lz4_hc_dict_emul.py checks its streams on the CPU
// (block format, reach, restore, limited output, ratio), and
// tests/test_gpu_lz4_hc_dict.py compares the kernel's bytes with it.
//
//   g++ -O2 -shared -fPIC -o tools/bin/liblz4hcdictemul.so tools/lz4_hc_dict_emul.cpp
//   int lz4hc_dict_emul_compress(const uint8_t *dict, int D, const uint8_t *page, int L, uint8_t *dst, int cap);
//
// With -DLZ4_HC_DICT_EMUL_MAIN it is a stand-alone program for sanitizer builds
// (g++ -O1 -g -fsanitize=address,undefined -DLZ4_HC_DICT_EMUL_MAIN): it replays a
// file of calls recorded by the test (LZ4_HC_DICT_EMUL_RECORD=<file> in the
// test's environment) in exactly sized heap buffers, so that a read or write
// outside them is reported, and compares the return values with the recorded
// ones.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define LZH_HOST 1
#include "../tyche_amd/csrc/lz4_hc_core.h"

extern "C" int lz4hc_dict_emul_compress(const uint8_t *dict, int D, const uint8_t *page, int L, uint8_t *dst, int cap) {
    if (D < 0 || D > 32768 || L < 0 || (int64_t)D + L > 65536 || cap < 0) return INT32_MIN;
    const uint32_t Dp = (uint32_t)D & ~63u, W = Dp + (uint32_t)L;
    alignas(16) static thread_local uint16_t table[lzh::kTableEntries];
    static thread_local uint8_t cnt[lzh::kBuckets];
    memset(table, 0, sizeof(table));
    memset(cnt, 0, sizeof(cnt));
    {
        // the seed sees exactly the tail: it is built once per handle, before any page is known
        uint8_t *tail = new uint8_t[(size_t)Dp + !Dp];
        if (Dp) memcpy(tail, dict + ((uint32_t)D - Dp), Dp);
        lzh::seed_window(tail, Dp, table, cnt);
        delete[] tail;
    }
    // exactly the window: the core reads no byte behind it
    uint8_t *in = new uint8_t[(size_t)W + !W];
    if (Dp) memcpy(in, dict + ((uint32_t)D - Dp), Dp);
    if (L) memcpy(in + Dp, page, (size_t)L);
    const int rv = lzh::encode_window(in, Dp, W, table, cnt, dst, (uint32_t)cap);
    delete[] in;
    return rv;
}

// the seed of a dictionary (kTableEntries 16-bit ring slots, then kBuckets next-way counters): its size
extern "C" int lz4hc_dict_emul_seed(const uint8_t *dict, int D, uint8_t *out) {
    const size_t tb = lzh::kTableEntries * sizeof(uint16_t), n = tb + lzh::kBuckets;
    if (D < 0 || D > 32768) return INT32_MIN;
    const uint32_t Dp = (uint32_t)D & ~63u;
    std::vector<uint16_t> table(lzh::kTableEntries, 0);
    std::vector<uint8_t> cnt(lzh::kBuckets, 0);
    lzh::seed_window(dict + ((uint32_t)D - Dp), Dp, table.data(), cnt.data());
    memcpy(out, table.data(), tb);
    memcpy(out + tb, cnt.data(), lzh::kBuckets);
    return (int)n;
}

#ifdef LZ4_HC_DICT_EMUL_MAIN
// Record: u32 dictionary length, u32 page length, u32 capacity, i32 return value, u32 misalignment of
// the destination, then the dictionary's and the page's bytes.
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
    uint32_t h[5];
    long calls = 0, bad = 0;
    while (fread(h, sizeof(h), 1, f) == 1) {
        const uint32_t D = h[0], n = h[1], cap = h[2], da = h[4] & 15u;
        const int32_t want = (int32_t)h[3];
        uint8_t *dc = new uint8_t[(size_t)D + !D], *s = new uint8_t[(size_t)n + !n], *d = new uint8_t[(size_t)cap + da + !(cap + da)];
        if ((D && fread(dc, 1, D, f) != D) || (n && fread(s, 1, n, f) != n)) {
            fprintf(stderr, "truncated record\n");
            return 2;
        }
        const int got = lz4hc_dict_emul_compress(dc, (int)D, s, (int)n, d + da, (int)cap);
        if (got != want) {
            bad++;
            fprintf(stderr, "call %ld: D %u n %u cap %u: got %d, recorded %d\n", calls, D, n, cap, got, want);
        }
        calls++;
        delete[] dc;
        delete[] s;
        delete[] d;
    }
    fclose(f);
    printf("%ld calls replayed, %ld differ\n", calls, bad);
    return bad ? 1 : 0;
}
#endif
