// tools/lz4_large_emul.cpp -- host emulator of the large-page LZ4 kernels
// (tyche_amd/csrc/lz4_encode_large.hip, lz4_decode_large.hip) for one page at a
// time: the kernels' own per-wave code (lz4_large_core.h: ring addressing and
// flush, stream-window refill, the decoder's verdicts, the block scan, the
// sequences written as they are found, literals fetched from the page once
// they have left the ring) with the 64 lanes as explicit loops and ballots
// over arrays.  The rings and the table stand where the kernels keep them in
// LDS.  TEST INFRASTRUCTURE: tests/test_lz4_large_emul.py runs it against the
// oracle on the CPU, so the logic is checked before (and apart from) the GPU
// parity tests.
//
//   g++ -O2 -shared -fPIC -o tools/bin/liblz4largeemul.so tools/lz4_large_emul.cpp
//   int lz4_large_emul_decompress(const uint8_t *src, int L, uint8_t *dst, int C);
//   int lz4_large_emul_compress(const uint8_t *src, int L, uint8_t *dst, int cap);
//
// With -DLZ4_LARGE_EMUL_MAIN it is a stand-alone program for sanitizer builds
// (g++ -O1 -g -fsanitize=address,undefined -DLZ4_LARGE_EMUL_MAIN): it replays a
// file of calls recorded by the test (LZ4_LARGE_EMUL_RECORD=<file> in the
// test's environment) in exactly sized heap buffers, so that a read or write
// outside them is reported, and compares the return values with the recorded
// ones.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define LZL_HOST 1
#include "../tyche_amd/csrc/lz4_large_core.h"

namespace {
struct Lds {
    alignas(16) uint8_t ring[lzl::kRing];
    alignas(16) uint8_t win[lzl::kWin];
    alignas(16) uint16_t table[lzl::kTableSize];
};
Lds *lds() {
    static thread_local Lds *p = new Lds();
    return p;
}
}  // namespace

extern "C" int lz4_large_emul_decompress(const uint8_t *src, int L, uint8_t *dst, int C) {
    if (L < 0 || C < 0 || (uint32_t)C > lzl::kMaxPage) return INT32_MIN;
    Lds *m = lds();
    memset(m->ring, 0xEE, sizeof(m->ring));   // (nothing may depend on what the rings held before)
    memset(m->win, 0xEE, sizeof(m->win));
    return lzl::decode_page(src, (uint32_t)L, dst, (uint32_t)C, m->ring, m->win);
}

extern "C" int lz4_large_emul_compress(const uint8_t *src, int L, uint8_t *dst, int cap) {
    if (L < 0 || cap < 0 || (uint32_t)L > lzl::kMaxPage) return INT32_MIN;
    Lds *m = lds();
    memset(m->ring, 0xEE, sizeof(m->ring));
    memset(m->table, 0, sizeof(m->table));
    return lzl::encode_page(src, (uint32_t)L, dst, (uint32_t)cap, m->ring, m->table);
}

#ifdef LZ4_LARGE_EMUL_MAIN
// Record: u32 mode (0 decode, 1 encode), u32 source length, u32 capacity, i32 return value,
// u32 misalignment of the source, u32 of the destination, then the source bytes.
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
    uint32_t h[6];
    long calls = 0, bad = 0;
    while (fread(h, sizeof(h), 1, f) == 1) {
        const uint32_t mode = h[0], n = h[1], cap = h[2], sa = h[4] & 15u, da = h[5] & 15u;
        const int32_t want = (int32_t)h[3];
        // exactly sized heap buffers whose byte 0 stands at the recorded misalignment from a 16-byte
        // line (operator new[] returns 16-byte aligned blocks): the sanitizer sees every byte
        // read or written before or after them
        uint8_t *s = new uint8_t[(size_t)n + sa + !(n + sa)], *d = new uint8_t[(size_t)cap + da + !(cap + da)];
        if (((uintptr_t)s | (uintptr_t)d) & 15u) {
            fprintf(stderr, "allocations are not 16-byte aligned\n");
            return 2;
        }
        uint8_t *sp = s + sa, *dp = d + da;
        if (n && fread(sp, 1, n, f) != n) {
            fprintf(stderr, "truncated record\n");
            return 2;
        }
        const int got = mode ? lz4_large_emul_compress(sp, (int)n, dp, (int)cap)
                             : lz4_large_emul_decompress(sp, (int)n, dp, (int)cap);
        const bool ok = got == want;
        if (!ok) {
            bad++;
            fprintf(stderr, "call %ld: mode %u n %u cap %u: got %d, recorded %d\n", calls, mode, n, cap, got, want);
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
