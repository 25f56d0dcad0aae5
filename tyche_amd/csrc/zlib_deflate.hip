// zlib_deflate.hip -- the default zlib encoder's kernel and launch; the per-wave
// code is zlib_deflate_core.h.
#include "zlib_deflate_core.h"

namespace tyche {
namespace {

__global__ __launch_bounds__(64) void zlib_deflate_kernel(tyche_batch_t b, uint32_t in_cap, unsigned *ctr, uint8_t *ws,
                                                          uint32_t ws_stride) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x;
    uint16_t *table = (uint16_t *)smem;
    uint32_t *stage_bits = (uint32_t *)(smem + kTableSlots * sizeof(uint16_t));
    uint8_t *map = (uint8_t *)(stage_bits + kStageWords);
    uint2 *rec = (uint2 *)(map + kWave);
    uint8_t *stage = (uint8_t *)(rec + kWave);
    const size_t stride = gridDim.x;

    size_t page = blockIdx.x;
    if (page >= b.count) return;
    PageRef p = batch_page(b, page);
    uint32_t head = stage_in(p.src, p.src_len <= in_cap ? p.src_len : 0, stage, lane, kWave);
    for (;;) {
        const size_t next = ctr ? claim_page(ctr, lane) : page + stride;   // dynamic assignment (engine.h)
        PageRef pn;
        TYCHE_NEXT_PAGE(kPrefetchVec);
        if (next < b.count) {
            pn = batch_page(b, next);
            TYCHE_NEXT_PAGE_FETCH(kPrefetchVec, kWave, pn.src, pn.src_len, in_cap, lane)
        }
        int32_t rv;
        if (p.src_len > in_cap) {
            rv = kResultTooLarge;
        } else {
            uint8_t *in = stage + head;
            in[p.src_len + lane] = 0;
            WAVE_SYNC();
            rv = encode_page<false>(in, p.src_len, table, map, rec, stage_bits, p.dst, p.dst_cap,
                                    ws ? ws + (size_t)blockIdx.x * ws_stride : nullptr, ws_stride, lane);
        }
        if (lane == 0) b.results[page] = rv;
        if (next >= b.count) break;
        WAVE_SYNC();
        page = next;
        p = pn;
        head = nhead;
        TYCHE_NEXT_PAGE_INSTALL(kPrefetchVec, kWave, p.src, p.src_len, in_cap, stage, lane)
    }
}

}  // namespace

hipError_t launch_zlib_deflate(const tyche_batch_t &b, uint32_t in_cap, hipStream_t s) {
    if (knob("ZLIB_HC", 0) != 0) return launch_zlib_deflate_hc(b, in_cap, s);
    if (b.count == 0) return hipSuccess;
    if (in_cap > 65535u) return hipErrorInvalidValue;    // 16-bit positions in the parse
    const size_t lds = kTableSlots * sizeof(uint16_t) + kStageWords * 4 + kWave + kWave * 8 +
                       ((in_cap + 16u + kPad + 15u) & ~15u);
    const size_t grid = page_grid((const void *)zlib_deflate_kernel, kWave, lds, b.count);
    WorkCounter ctr(s, grid < b.count);
    if (!ctr.get()) return hipErrorOutOfMemory;
    // per-wave record scratch: L / 3 + 2 records of 8 bytes (each record but the
    // last covers a match of >= 3 bytes)
    const uint32_t ws_stride = ((in_cap / 3u + 3u) * 8u + 255u) & ~255u;
    ScratchLease ws(s, grid * (size_t)ws_stride);
    if (!ws.get()) return hipErrorOutOfMemory;   // the kernel writes its records there
    hipLaunchKernelGGL(zlib_deflate_kernel, dim3((unsigned)grid), dim3(kWave), lds, s, b, in_cap, ctr.get(),
                       (uint8_t *)ws.get(), ws_stride);
    return hipGetLastError();
}

}  // namespace tyche
