// lz4_decode_large.hip -- LZ4 block decode of launches whose page window and
// stream do not fit the 160 KiB of LDS together (every page above roughly 80
// KiB), up to a capacity of TYCHE_LZ4_MAX_PAGE (4 MiB) and a stream of its
// lz4_bound: exactly the launches launch_lz4_decode used to refuse.  Any valid
// block decodes, whoever wrote it -- the reference's byU32 encoder puts offsets
// up to 65,535 anywhere in a page.
//
// One 64-lane wave per page walks the stream as decode_page_serial does
// (lz4_decode.hip) with LZ4_decompress_safe's return values, but keeps neither
// the page nor the stream whole (lz4_large_core.h): the output goes to a 128
// KiB ring in LDS -- the last 65,535 bytes, which is all a match can reach, plus
// what is not yet flushed -- and leaves for dst in aligned 16-byte stores; the
// stream comes through a 16 KiB window refilled 8 KiB at a time.  dst is only
// ever written, below dst + capacity, so it may be pinned host memory (the host
// path's direct output); the lane decoder, which reads its output back, stays
// barred there.  LDS: 144 KiB, one page per CU (the 68 + 8 KiB layout that
// would fit two needs a ring that is no power of two; not done).  Pages are
// claimed dynamically.  Every page of such a launch decodes here, small ones
// included: the result does not depend on the route.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine.h"
#include "lds_io.h"

#define LZL_HOST 0
#include "lz4_large_core.h"

namespace tyche {

namespace {

constexpr size_t kDecLargeLds = lzl::kRing + lzl::kWin;

__global__ __launch_bounds__(64) void lz4_decode_large_kernel(tyche_batch_t b, uint32_t in_cap, uint32_t out_cap,
                                                              unsigned *ctr) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x;
    uint8_t *ring = smem;
    uint8_t *win = smem + lzl::kRing;
    for (size_t page = blockIdx.x; page < b.count; page = claim_page(ctr, lane)) {
        const PageRef p = batch_page(b, page);
        int32_t rv = kResultTooLarge;
        if (p.src_len <= in_cap && p.dst_cap <= out_cap) rv = lzl::decode_page(p.src, p.src_len, p.dst, p.dst_cap, ring, win, lane);
        if (lane == 0) b.results[page] = rv;
        WAVE_SYNC();
    }
}

}  // namespace

hipError_t launch_lz4_decode_large(const tyche_batch_t &b, uint32_t in_cap, uint32_t out_cap, hipStream_t s) {
    if (b.count == 0) return hipSuccess;
    if (out_cap > TYCHE_LZ4_MAX_PAGE || in_cap > lz4_bound(TYCHE_LZ4_MAX_PAGE)) return hipErrorInvalidValue;
    const size_t grid = page_grid((const void *)lz4_decode_large_kernel, 64, kDecLargeLds, b.count);
    WorkCounter ctr(s, grid < b.count);
    if (!ctr.get()) return hipErrorOutOfMemory;
    hipLaunchKernelGGL(lz4_decode_large_kernel, dim3((unsigned)grid), dim3(64), kDecLargeLds, s, b, in_cap, out_cap,
                       ctr.get());
    return hipGetLastError();
}

}  // namespace tyche
