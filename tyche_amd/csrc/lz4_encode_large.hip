// lz4_encode_large.hip -- LZ4 block encode of pages above 65,535 bytes, up to
// TYCHE_LZ4_MAX_PAGE (4 MiB): one standard LZ4 block per page, which
// LZ4_decompress_safe restores.
//
// The small-page encoders (lz4_encode.hip) stage the whole page in LDS and
// parse it with 16-bit positions; neither holds above 65,535 bytes.  Here one
// 64-lane wave slides a 128 KiB ring over the page (lz4_large_core.h): the
// parse always sees the 65,535 bytes an offset can reach, matches and literal
// runs cross any 64 KiB line like any other byte, and the stream is written to
// dst as it is found, every store checked against the capacity.  There are no
// segments and therefore no join.  LDS: the ring and a table of 8192 16-bit
// entries, 144 KiB, so one page per CU; the work is serial along a page and
// parallel across pages, which are claimed dynamically (engine.h).
//
// launch_lz4_encode sends a launch here when its declared maximum exceeds
// 65,535: a launch with per-page lengths first runs the small-page path with a
// maximum of 65,535 (which leaves INT32_MIN for the longer pages) and then this
// kernel with min_len = 65,536, which takes exactly those pages and leaves the
// others' results alone; small pages get the bytes they always got.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine.h"
#include "lds_io.h"

#define LZL_HOST 0
#include "lz4_large_core.h"

namespace tyche {

namespace {

constexpr size_t kEncLargeLds = lzl::kRing + lzl::kTableSize * sizeof(uint16_t);
static_assert(lzl::kMaxPage == TYCHE_LZ4_MAX_PAGE, "one limit");

__global__ __launch_bounds__(64) void lz4_encode_large_kernel(tyche_batch_t b, uint32_t in_cap, uint32_t min_len,
                                                              unsigned *ctr) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x;
    uint8_t *ring = smem;
    uint16_t *table = (uint16_t *)(smem + lzl::kRing);
    for (size_t page = blockIdx.x; page < b.count; page = claim_page(ctr, lane)) {
        const PageRef p = batch_page(b, page);
        if (p.src_len < min_len) continue;   // the small-page launch's
        int32_t rv = kResultTooLarge;
        if (p.src_len <= in_cap) {
            for (uint32_t w = lane; w < lzl::kTableSize * sizeof(uint16_t) / 16; w += 64u)
                ((u32x4 *)table)[w] = u32x4{0, 0, 0, 0};
            WAVE_SYNC();
            rv = lzl::encode_page(p.src, p.src_len, p.dst, p.dst_cap, ring, table, lane);
        }
        if (lane == 0) b.results[page] = rv;
        WAVE_SYNC();
    }
}

}  // namespace

hipError_t launch_lz4_encode_large(const tyche_batch_t &b, uint32_t in_cap, uint32_t min_len, hipStream_t s) {
    if (b.count == 0) return hipSuccess;
    if (in_cap > TYCHE_LZ4_MAX_PAGE) return hipErrorInvalidValue;
    const size_t grid = page_grid((const void *)lz4_encode_large_kernel, 64, kEncLargeLds, b.count);
    WorkCounter ctr(s, grid < b.count);
    if (!ctr.get()) return hipErrorOutOfMemory;
    hipLaunchKernelGGL(lz4_encode_large_kernel, dim3((unsigned)grid), dim3(64), kEncLargeLds, s, b, in_cap, min_len,
                       ctr.get());
    return hipGetLastError();
}

}  // namespace tyche
