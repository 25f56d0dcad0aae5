// lz4_encode_hc_dict.hip -- high-compression LZ4 block encode against a shared
// dictionary (LZ4_HC_DICT=1): lz4_encode_hc.hip's parse over lz4_encode_dict.hip's
// window.
//
// The dictionary's last D' = D & ~63 bytes followed by the page are one window of
// W = D' + L <= 65536 bytes, window position p at LDS byte p, as in the default
// dictionary encoder; lz4_hc_core.h's encode_window parses the page [D', W) with
// candidates anywhere in the window.  The block is an ordinary dictionary block:
// lz4_decode_dict.hip and LZ4_decompress_safe_usingDict restore it.  Same
// contract as lz4_encode_dict_kernel: results[i] is the size, or 0 when the
// stream does not fit dst_capacity; nothing at or past dst + dst_capacity is
// written and dst is never read; src_len == 0 gives the block 0x00; a page above
// in_cap gets INT32_MIN and its destination is left alone; per_page skips the
// pages the dictionary does not reach.  The bytes depend on the page and the
// dictionary alone, and equal those of the host emulator
// tools/lz4_hc_dict_emul.cpp.
//
// One 64-lane wave per page, looping over pages it claims.  Per page the wave
// stages  [ rings | next-way counters | dictionary tail | page ]  in LDS:
//   * where the plain HC kernel zeroes its table, this one copies the handle's
//     seed (lz4_hc_dict_seed.hip: what inserting the tail's positions 0 .. D' - 4
//     leaves in a zeroed table, 8 KiB of rings and 512 B of counters, built once
//     per handle on the host by the core's own host build); the three positions
//     whose 4 bytes run into the page are inserted per page by encode_window;
//   * the tail comes from the handle's image for this page's src & 15 shift, the
//     16 shifted images lz4_encode_dict_kernel uses: the page is staged by whole
//     16-byte vectors (stage_in), so the tail has to end at any of 16 byte shifts.
// No next page is prefetched: the page's first vector and the dictionary's last
// bytes share 16 bytes of LDS, so the install order is page, then dictionary, as
// in the other dictionary encoders.
//
// LDS per page: 8,192 + 512 + D' + the page's vectors (L + 15 + 15, rounded down
// to 16): 16,912 B at D = 4 KiB and 4 KiB pages (9 pages per CU), 29,200 B at
// 16 KiB pages (5 per CU), 74,272 B at the window's limit (2 per CU).  The table
// is the plain HC kernel's and no larger for the plain HC kernel's reason: the
// time follows the resident pages per CU.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine.h"
#include "lds_io.h"

#define LZH_HOST 0
#include "lz4_hc_core.h"

namespace tyche {

namespace {

constexpr uint32_t kWaveHD = 64;
constexpr uint32_t kWindowMaxHD = 65536;
constexpr size_t kTableBytesHD = lzh::kTableEntries * sizeof(uint16_t);
constexpr size_t kSeedBytesHD = kTableBytesHD + lzh::kBuckets;   // rings | next-way counters
static_assert(kSeedBytesHD % 16 == 0, "the seed is copied as 16-byte vectors");

__global__ __launch_bounds__(64) void lz4_encode_hc_dict_kernel(tyche_batch_t b, uint32_t in_cap, Lz4DictDev d,
                                                                 const u32x4 *seed, uint32_t per_page, unsigned *ctr) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x;
    uint16_t *table = (uint16_t *)smem;
    uint8_t *cnt = smem + kTableBytesHD;
    uint8_t *dstage = smem + kSeedBytesHD;       // the dictionary tail's vectors
    uint8_t *stage = dstage + d.enc_len;         // the page's vectors (enc_len is a multiple of 64)
    const uint32_t DE = d.enc_len;

    for (size_t page = blockIdx.x; page < b.count; page = claim_page(ctr, lane)) {
        const PageRef p = batch_page(b, page);
        if (per_page && (uint64_t)p.src_len + d.dlen > kWindowMaxHD) continue;
        if (p.src_len > in_cap) {
            if (lane == 0) b.results[page] = kResultTooLarge;
            continue;
        }
        WAVE_SYNC();
        // the page first: its first vector also holds up to 15 bytes in front of the page, which
        // the dictionary's last bytes then replace
        const uint32_t head = stage_in(p.src, p.src_len, stage, lane, kWaveHD);
        {
            const u32x4 *g = (const u32x4 *)(d.enc + (size_t)head * d.enc_stride);
            u32x4 *l = (u32x4 *)dstage;
            const uint32_t nvec = DE >> 4;       // whole vectors; the last, partial one goes by bytes
            for (uint32_t v = lane; v < nvec; v += kWaveHD) l[v] = g[v];
            if (DE && lane < head) stage[lane] = d.enc[(size_t)head * d.enc_stride + DE + lane];
            // every page starts from the dictionary's rings and counters
            for (uint32_t w = lane; w < kSeedBytesHD / 16; w += kWaveHD) ((u32x4 *)smem)[w] = seed[w];
        }
        WAVE_SYNC();
        const int32_t rv = lzh::encode_window(dstage + head, DE, DE + p.src_len, table, cnt, p.dst, p.dst_cap, lane);
        if (lane == 0) b.results[page] = rv;
    }
}

}  // namespace

hipError_t launch_lz4_encode_hc_dict(const tyche_batch_t &b, uint32_t in_cap, const Lz4DictDev &d, const void *seed,
                                     bool per_page, hipStream_t s) {
    if (b.count == 0) return hipSuccess;
    if (!seed || (uint64_t)in_cap + d.dlen > kWindowMaxHD || d.enc_len > d.dlen || (d.enc_len & 63u)) return hipErrorInvalidValue;
    // rings | counters | dictionary tail | the 16-byte vectors that hold a page (stage_in: a page may start at any byte of its first vector)
    const size_t lds = kSeedBytesHD + d.enc_len + ((in_cap + 15u + 15u) & ~15u);
    const size_t grid = page_grid((const void *)lz4_encode_hc_dict_kernel, kWaveHD, lds, b.count, "LZ4_HC_DICT_PAGES_PER_CU");
    WorkCounter ctr(s, grid < b.count);
    if (!ctr.get()) return hipErrorOutOfMemory;
    hipLaunchKernelGGL(lz4_encode_hc_dict_kernel, dim3((unsigned)grid), dim3(kWaveHD), lds, s, b, in_cap, d, (const u32x4 *)seed,
                       per_page ? 1u : 0u, ctr.get());
    return hipGetLastError();
}

}  // namespace tyche
