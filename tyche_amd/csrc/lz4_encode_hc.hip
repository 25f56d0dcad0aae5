// lz4_encode_hc.hip -- high-compression LZ4 block encode (LZ4_HC=1).
//
// The default encoder (lz4_encode.hip) is a greedy parse with one candidate per
// position.  This one looks at up to kWays + 1 candidates per position and
// chooses lazily between the matches at p, p + 1 and p + 2 (lz4_hc_core.h); it
// emits the same LZ4 block format, so every decoder here and the reference's
// LZ4_decompress_safe restore its streams unchanged.  Same contract as the
// default encoder: results[i] is the size, or 0 when the stream does not fit
// dst_capacity; nothing at or past dst + dst_capacity is written and dst is
// never read; src_len == 0 gives the one-byte block 0x00; a page above in_cap
// gets INT32_MIN and its destination is left alone.  The bytes depend on the
// page alone, and equal those of the host emulator tools/lz4_hc_emul.cpp.
//
// One 64-lane wave per page, looping over pages with the next page prefetched
// into registers (TYCHE_NEXT_PAGE, lds_io.h).  LDS per wave: the bucket table,
// 2^9 rings of 8 16-bit positions (8 KiB), the rings' 512 bytes of next-way
// counters, and the 16-byte vectors that hold the page (the encoder reads no
// byte past it): 25 KiB at 16 KiB pages, 6 pages per CU; 13 KiB at 4 KiB pages,
// 12 per CU; 73 KiB at 65,535 bytes, 2 per CU.  The kernel is bound by the
// latency of its dependent LDS reads, so its time follows the resident pages
// per CU (profiles/README.md: 1 / 2 / 3 / 4 pages per CU 102.6 / 53.7 / 37.9 /
// 30.2 ms with a 16 KiB table), which is why the table is no larger: 2^10 rings
// give ratio 3.059 instead of 3.054 at 30.2 instead of 22.4 ms.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine.h"
#include "lds_io.h"

#define LZH_HOST 0
#include "lz4_hc_core.h"

namespace tyche {

namespace {

constexpr uint32_t kWaveH = 64;
constexpr uint32_t kPrefetchVecH = 16;    // 16-byte vectors per lane prefetched for the next page (16 KiB)
constexpr size_t kTableBytesH = lzh::kTableEntries * sizeof(uint16_t);
constexpr size_t kCntBytesH = lzh::kBuckets;
static_assert(kTableBytesH % 16 == 0 && kCntBytesH % 16 == 0, "the table, the counters and the stage are cleared and read as 16-byte vectors");

__global__ __launch_bounds__(64) void lz4_encode_hc_kernel(tyche_batch_t b, uint32_t in_cap, unsigned *ctr) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x;
    uint16_t *table = (uint16_t *)smem;
    uint8_t *cnt = smem + kTableBytesH;
    uint8_t *stage = cnt + kCntBytesH;

    size_t page = blockIdx.x;
    if (page >= b.count) return;
    PageRef p = batch_page(b, page);
    uint32_t head = stage_in(p.src, p.src_len <= in_cap ? p.src_len : 0, stage, lane, kWaveH);
    for (;;) {
        const size_t next = claim_page(ctr, lane);   // dynamic assignment (engine.h)
        PageRef pn;
        TYCHE_NEXT_PAGE(kPrefetchVecH);
        if (next < b.count) {
            pn = batch_page(b, next);
            TYCHE_NEXT_PAGE_FETCH(kPrefetchVecH, kWaveH, pn.src, pn.src_len, in_cap, lane)
        }
        int32_t rv;
        if (p.src_len > in_cap) {
            rv = kResultTooLarge;
        } else {
            uint8_t *in = stage + head;
            // every page starts from an empty table: table and counters are one zeroed range
            for (uint32_t w = lane; w < (kTableBytesH + kCntBytesH) / 16; w += kWaveH) ((u32x4 *)smem)[w] = u32x4{0, 0, 0, 0};
            WAVE_SYNC();
            rv = lzh::encode_page(in, p.src_len, table, cnt, p.dst, p.dst_cap, lane);
        }
        if (lane == 0) b.results[page] = rv;
        if (next >= b.count) break;
        WAVE_SYNC();
        page = next;
        p = pn;
        head = nhead;
        TYCHE_NEXT_PAGE_INSTALL(kPrefetchVecH, kWaveH, p.src, p.src_len, in_cap, stage, lane)
    }
}

}  // namespace

hipError_t launch_lz4_encode_hc(const tyche_batch_t &b, uint32_t in_cap, hipStream_t s) {
    // table | ring counters | the 16-byte vectors that hold a page (stage_in: a page may start at any byte of its first vector)
    const size_t lds = kTableBytesH + kCntBytesH + ((in_cap + 15u + 15u) & ~15u);
    const size_t grid = page_grid((const void *)lz4_encode_hc_kernel, kWaveH, lds, b.count, "LZ4_HC_PAGES_PER_CU");
    WorkCounter ctr(s, grid < b.count);
    if (!ctr.get()) return hipErrorOutOfMemory;
    hipLaunchKernelGGL(lz4_encode_hc_kernel, dim3((unsigned)grid), dim3(kWaveH), lds, s, b, in_cap, ctr.get());
    return hipGetLastError();
}

}  // namespace tyche
