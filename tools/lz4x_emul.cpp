// tools/lz4x_emul.cpp -- host emulator of the exact LZ4 encoder
// (tyche_amd/csrc/lz4_encode_exact.hip, LZ4_EXACT=1) for one page at a time: the
// kernel's own per-wave code (lz4_exact_core.h: search schedule, batch
// resolution with same-hash handling, catch-up, match counting, the step after
// a match, the limited-output checks, sequence emission) with the 64 lanes as
// explicit loops and ballots over arrays.  The page is staged as the kernel
// stages it: zero bytes behind it, a zeroed 8192-entry table.  TEST
// INFRASTRUCTURE: tests/test_lz4_exact_emul.py runs it against the oracle's
// LZ4_compress_default on the CPU, so the algorithm is checked before (and
// apart from) the GPU parity tests.
//
//   g++ -O2 -shared -fPIC -o tools/bin/liblz4xemul.so tools/lz4x_emul.cpp
//   int lz4x_emul_compress(const uint8_t *src, int L, uint8_t *dst, int cap);
#include <cstdint>
#include <cstring>
#include <vector>

#define LZX_HOST 1
#include "../tyche_amd/csrc/lz4_exact_core.h"

extern "C" int lz4x_emul_compress(const uint8_t *src, int L, uint8_t *dst, int cap) {
    if (L < 0 || L > 65535 || cap < 0) return INT32_MIN;
    std::vector<uint8_t> in((size_t)L + 64, 0);
    if (L) memcpy(in.data(), src, (size_t)L);
    static thread_local uint16_t table[lzx::kTableSize];
    memset(table, 0, sizeof(table));
    return lzx::encode_page(in.data(), (uint32_t)L, table, dst, (uint32_t)cap);
}

// the attempt schedule's closed form (for the test: compared with the steps summed one by one)
extern "C" uint32_t lz4x_emul_sched(uint32_t t) { return lzx::sched(t); }
