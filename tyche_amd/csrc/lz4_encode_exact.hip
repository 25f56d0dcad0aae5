// lz4_encode_exact.hip -- LZ4 block encode byte-identical to LZ4 1.7.5
// (LZ4_EXACT=1).
//
// The default encoder (lz4_encode.hip) emits a valid LZ4 block of its own
// parse.  This one emits the bytes, and returns the value, of the reference's
// LZ4_compress_default (lz4.c:697 -> LZ4_compress_generic lz4.c:459-656, byU16):
// results[i] and dst[0, results[i]) are what a host run of the vendored codec
// gives, so compressed pages can be compared, deduplicated or checksummed
// against host-compressed ones and comp_length accounting agrees.  Nothing at
// or past dst + dst_capacity is written.  src_len == 0 gives the one-byte block
// 0x00 (result 1; 0 when dst_capacity is 0), as the default encoder and the
// reference do.
//
// One 64-lane wave per page, looping over pages with the next page prefetched
// into registers (TYCHE_NEXT_PAGE, lds_io.h).  The page is staged in LDS next to the
// reference's table: 8192 16-bit positions (16 KiB), zeroed per page.  The
// encoder reads no byte past the page, so the stage is the 16-byte vectors that
// hold it: 32 KiB per wave at 16 KiB pages (4 pages per CU by LDS, one wave per
// SIMD), 48 KiB at 32 KiB (3), 80 KiB at 65,535 bytes (1).  The
// walk itself is serial by definition; lz4_exact_core.h says where the wave is
// used and is shared with the host emulator tools/lz4x_emul.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine.h"
#include "lds_io.h"

#define LZX_HOST 0
#include "lz4_exact_core.h"

namespace tyche {

namespace {

constexpr uint32_t kWaveX = 64;
constexpr uint32_t kPrefetchVecX = 16;    // 16-byte vectors per lane prefetched for the next page (16 KiB)
constexpr size_t kTableBytes = lzx::kTableSize * sizeof(uint16_t);

__global__ __launch_bounds__(64) void lz4_encode_exact_kernel(tyche_batch_t b, uint32_t in_cap, unsigned *ctr) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x;
    uint16_t *table = (uint16_t *)smem;
    uint8_t *stage = smem + kTableBytes;

    size_t page = blockIdx.x;
    if (page >= b.count) return;
    PageRef p = batch_page(b, page);
    uint32_t head = stage_in(p.src, p.src_len <= in_cap ? p.src_len : 0, stage, lane, kWaveX);
    for (;;) {
        const size_t next = claim_page(ctr, lane);   // dynamic assignment (engine.h)
        PageRef pn;
        TYCHE_NEXT_PAGE(kPrefetchVecX);
        if (next < b.count) {
            pn = batch_page(b, next);
            TYCHE_NEXT_PAGE_FETCH(kPrefetchVecX, kWaveX, pn.src, pn.src_len, in_cap, lane)
        }
        int32_t rv;
        if (p.src_len > in_cap) {
            rv = kResultTooLarge;
        } else {
            uint8_t *in = stage + head;
            // the reference's table starts zeroed for every page: an unwritten slot is candidate 0
            for (uint32_t w = lane; w < kTableBytes / 16; w += kWaveX) ((u32x4 *)table)[w] = u32x4{0, 0, 0, 0};
            WAVE_SYNC();
            rv = lzx::encode_page(in, p.src_len, table, p.dst, p.dst_cap, lane);
        }
        if (lane == 0) b.results[page] = rv;
        if (next >= b.count) break;
        WAVE_SYNC();
        page = next;
        p = pn;
        head = nhead;
        TYCHE_NEXT_PAGE_INSTALL(kPrefetchVecX, kWaveX, p.src, p.src_len, in_cap, stage, lane)
    }
}

}  // namespace

hipError_t launch_lz4_encode_exact(const tyche_batch_t &b, uint32_t in_cap, hipStream_t s) {
    // table | the 16-byte vectors that hold a page (stage_in: a page may start at any byte of its first vector)
    const size_t lds = kTableBytes + ((in_cap + 15u + 15u) & ~15u);
    const size_t grid = page_grid((const void *)lz4_encode_exact_kernel, kWaveX, lds, b.count, "LZ4_EXACT_PAGES_PER_CU");
    WorkCounter ctr(s, grid < b.count);
    if (!ctr.get()) return hipErrorOutOfMemory;
    hipLaunchKernelGGL(lz4_encode_exact_kernel, dim3((unsigned)grid), dim3(kWaveX), lds, s, b, in_cap, ctr.get());
    return hipGetLastError();
}

}  // namespace tyche
