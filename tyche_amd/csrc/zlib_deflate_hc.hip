// zlib_deflate_hc.hip -- the high-compression zlib encoder's kernel and launch
// (ZLIB_HC=1); the per-wave code is zlib_deflate_core.h with zlib_hc_core.h's
// parse as pass 1.
#include "zlib_deflate_core.h"
#define ZLH_HOST 0
#include "zlib_hc_core.h"

namespace tyche {
namespace {

// ---- the high-compression encoder (ZLIB_HC=1): pass 1 is zlib_hc_core.h's parse -- 2^9 bucket
// rings of the 16 latest positions, the nearest lower lane of the block, the candidate of the
// highest gain (length against the distance's extra bits) and a two-step lazy rule on gains, the
// same text as the host emulator tools/zlib_hc_emul.cpp -- in front of the unchanged passes 2 and
// 3.  One wave per page, the page loop and next-page prefetch of zlib_deflate_kernel.
//
// LDS: [ rings 16,384 | ring counters 512 | bit staging 512 | symbol map 64 | 64 records 512 | the
// page's vectors | 64 zero bytes ]: 22.1 KiB at 4 KiB pages (7 per CU), 34.1 KiB at 16 KiB (4 per
// CU), 50.1 KiB at 32 KiB (3 per CU), 82.1 KiB at 65,535 bytes (1 per CU).  Once the parse is done
// the rings' first 8 KiB are the histograms, codes and the fixed-code fallback's table.
// the high-compression parse's rings and ring counters (zlib_hc_core.h)
constexpr size_t kHcTableBytes = zlh::kTableEntries * sizeof(uint16_t);
constexpr size_t kHcCntBytes = zlh::kBuckets;

// Pass 1 of the high-compression encoder (declared in zlib_deflate_core.h): zlib_hc_core.h's parse of in[0, L), its records
// stored downwards from recs (record i at recs[-1 - i], at most room of them).  Returns
// (anchor of the last literal run or 0xFFFFFFFF when the records did not fit, records stored).
// A function of its own, not inlined: passes 2 and 3 then compile in the kernel as they do in
// the default one, with their arrays and closures in registers.
__device__ __noinline__ uint2 hc_pass1(const uint8_t *in, uint32_t L, uint16_t *table, uint8_t *cnt, uint2 *rec, uint2 *recs,
                                       uint32_t room, uint32_t lane) {
    // every page starts from empty rings: table and counters are one zeroed range
    for (uint32_t w = lane; w < (kHcTableBytes + kHcCntBytes) / 16; w += kWave) ((u32x4 *)table)[w] = u32x4{0, 0, 0, 0};
    WAVE_SYNC();
    uint32_t nrec = 0;
    // (the parse's records are the stored ones: its own backward extension, no distance beyond the window)
    auto sink = [&](const uint2 *r, uint32_t n) __attribute__((always_inline)) -> bool {
        if (nrec + n > room) return false;
        if (lane < n) recs[-1 - (int32_t)(nrec + lane)] = r[lane];
        nrec += n;
        return true;
    };
    const uint32_t anchor = zlh::parse_page(in, L, table, cnt, rec, sink, lane);
    return make_uint2(anchor, nrec);
}

constexpr size_t kHcFront = kHcTableBytes + kHcCntBytes + kStageWords * 4 + kWave + kWave * 8;
// (the next page's first 8 KiB wait in registers, half of the default kernel's window: the parse
// needs the registers, and the rest of a longer page is loaded at the install)
constexpr uint32_t kHcPrefetchVec = 8;
static_assert(kHcTableBytes % 16 == 0 && kHcCntBytes % 16 == 0, "rings and counters are cleared as 16-byte vectors");
static_assert(kHcTableBytes >= kTableSlots * sizeof(uint16_t), "passes 2 and 3 and the fallback reuse the rings");
__global__ __launch_bounds__(64) void zlib_deflate_hc_kernel(tyche_batch_t b, uint32_t in_cap, unsigned *ctr, uint8_t *ws,
                                                             uint32_t ws_stride) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x;
    uint16_t *table = (uint16_t *)smem;
    uint8_t *cnt = smem + kHcTableBytes;
    uint32_t *stage_bits = (uint32_t *)(cnt + kHcCntBytes);
    uint8_t *map = (uint8_t *)(stage_bits + kStageWords);
    uint2 *rec = (uint2 *)(map + kWave);
    uint8_t *stage = smem + kHcFront;
    const size_t stride = gridDim.x;

    size_t page = blockIdx.x;
    if (page >= b.count) return;
    PageRef p = batch_page(b, page);
    uint32_t head = stage_in(p.src, p.src_len <= in_cap ? p.src_len : 0, stage, lane, kWave);
    for (;;) {
        const size_t next = ctr ? claim_page(ctr, lane) : page + stride;   // dynamic assignment (engine.h)
        PageRef pn;
        TYCHE_NEXT_PAGE(kHcPrefetchVec);
        if (next < b.count) {
            pn = batch_page(b, next);
            TYCHE_NEXT_PAGE_FETCH(kHcPrefetchVec, kWave, pn.src, pn.src_len, in_cap, lane)
        }
        int32_t rv;
        if (p.src_len > in_cap) {
            rv = kResultTooLarge;
        } else {
            uint8_t *in = stage + head;
            const uint32_t L = p.src_len;
            in[L + lane] = 0;
            WAVE_SYNC();
            rv = encode_page<true>(in, L, table, map, rec, stage_bits, p.dst, p.dst_cap,
                                   ws ? ws + (size_t)blockIdx.x * ws_stride : nullptr, ws_stride, lane, cnt);
        }
        if (lane == 0) b.results[page] = rv;
        if (next >= b.count) break;
        WAVE_SYNC();
        page = next;
        p = pn;
        head = nhead;
        TYCHE_NEXT_PAGE_INSTALL(kHcPrefetchVec, kWave, p.src, p.src_len, in_cap, stage, lane)
    }
}

}  // namespace

// TYCHE_ZLIB_HC=1: every zlib compress launch to the high-compression kernel above.
// ZLIB_HC_PAGES_PER_CU caps the resident pages per CU (occupancy A/B; 0: what fits).
hipError_t launch_zlib_deflate_hc(const tyche_batch_t &b, uint32_t in_cap, hipStream_t s) {
    if (b.count == 0) return hipSuccess;
    if (in_cap > 65535u) return hipErrorInvalidValue;    // 16-bit positions in the parse
    const size_t lds = kHcFront + ((in_cap + 16u + kPad + 15u) & ~15u);
    const size_t grid = page_grid((const void *)zlib_deflate_hc_kernel, kWave, lds, b.count, "ZLIB_HC_PAGES_PER_CU");
    WorkCounter ctr(s, grid < b.count);
    if (!ctr.get()) return hipErrorOutOfMemory;
    const uint32_t ws_stride = ((in_cap / 3u + 3u) * 8u + 255u) & ~255u;   // L / 3 + 2 records, as the default encoder
    ScratchLease ws(s, grid * (size_t)ws_stride);
    if (!ws.get()) return hipErrorOutOfMemory;   // the kernel writes its records there
    hipLaunchKernelGGL(zlib_deflate_hc_kernel, dim3((unsigned)grid), dim3(kWave), lds, s, b, in_cap, ctr.get(),
                       (uint8_t *)ws.get(), ws_stride);
    return hipGetLastError();
}

}  // namespace tyche
