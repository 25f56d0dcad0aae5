// zlib_deflate_dict.hip -- batched zlib encode with a shared dictionary
// (tyche_zlib_compress_batch_dict, and the host entry points once a process-wide
// zlib dictionary is installed); the per-wave code is zlib_deflate_core.h's
// encode_page<false, true>.  A translation unit of its own, as the high-compression
// encoder is: a second caller of encode_page in zlib_deflate.hip would change the
// default kernel's inlining and registers.
//
// A dictionary of D bytes followed by a page of L bytes is one deflate window
// (L + D <= 65536, so window positions stay 16 bits): the stream is what
// deflateSetDictionary + deflate(Z_FINISH) produce in kind -- header 78 3F and
// DICTID, the adler32 of all D bytes, then the default encoder's one final block
// whose distances may reach min(32768, position + D) back, then the adler32 of the
// page alone -- and what inflateSetDictionary + inflate restore.
//
// One 64-lane wave per page, looping over pages it claims.  Per page the wave
// stages  [ table | bit staging | map | records | dictionary tail | page | zero pad ]:
//   * the dictionary's last D' = D & ~63 bytes stand right before the page's first
//     byte (the handle's image holds them at all 16 byte shifts a page's first
//     vector can have, Lz4DictDev::enc), so window position p is LDS byte p and
//     lz_parse.h's parse_page runs unchanged from start = D', as in
//     lz4_encode_dict.hip and zstd_parse_dict_kernel;
//   * the table -- 512 buckets of 8 positions, keyed by 3 bytes -- starts as a copy
//     of the handle's seeded table (zlib_dict_seed_table below, 8 KiB, built once per
//     handle on the host): hashing the tail per page would cost D'/64 parse steps per
//     page, a quarter of a 16 KiB page's own at D = 4 KiB and as many as the page's at
//     D = 16 KiB, for a table that is the same for every page;
//   * the records leave pass 1 as page positions (encode_page), so the tree and code
//     passes are the plain encoder's.
// The page loop is lz4_encode_dict_kernel's (no next-page prefetch: the page's first
// vector and the dictionary's last bytes share 16 bytes of LDS, so the install order
// is page, then dictionary).
//
// LDS: 8,192 table + 512 bit staging + 64 map + 512 records + D' + the page's
// vectors (L + 16, rounded up to 16) + 64 zero bytes.  With 160 KiB per CU:
//     page      D = 4 KiB            D = 16 KiB
//     4 KiB     17,552 B   9 / CU    29,840 B   5 / CU
//     16 KiB    29,840 B   5 / CU    42,128 B   3 / CU
//     32 KiB    46,224 B   3 / CU    58,512 B   2 / CU
// (the plain encoder: 13,456 / 25,744 / 42,128 bytes, 12 / 6 / 3 per CU by LDS; 74,896 bytes, 2 per
// CU, at the window's limit.  148 VGPRs allow 12 waves per CU, so the LDS decides.)
#include "zlib_deflate_core.h"

#include <vector>

namespace tyche {
namespace {

constexpr size_t kFrontZD = kTableSlots * sizeof(uint16_t) + kStageWords * 4 + kWave + kWave * 8;
static_assert(kFrontZD % 16 == 0, "the dictionary tail is copied as 16-byte vectors");
static_assert(kWays == 8 && kMin3 && !kRep, "the seeded table is hashed for parse_page<false, true, 8>");

// per_page: the host entry points' reach rule -- a page with src_len + D > 65536 is not this
// kernel's (its result is left alone: another launch over the same batch owns it)
__global__ __launch_bounds__(64) void zlib_deflate_dict_kernel(tyche_batch_t b, uint32_t in_cap, Lz4DictDev d,
                                                               const uint32_t *seed, uint32_t per_page, unsigned *ctr,
                                                               uint8_t *ws, uint32_t ws_stride) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x;
    uint16_t *table = (uint16_t *)smem;
    uint32_t *stage_bits = (uint32_t *)(smem + kTableSlots * sizeof(uint16_t));
    uint8_t *map = (uint8_t *)(stage_bits + kStageWords);
    uint2 *rec = (uint2 *)(map + kWave);
    uint8_t *dstage = smem + kFrontZD;           // the dictionary tail's vectors
    const uint32_t DE = d.enc_len;               // a multiple of 64
    uint8_t *stage = dstage + DE;                // the page's vectors

    for (size_t page = blockIdx.x; page < b.count; page = ctr ? claim_page(ctr, lane) : page + gridDim.x) {
        const PageRef p = batch_page(b, page);
        if (per_page && (uint64_t)p.src_len + d.dlen > 65536u) continue;
        if (p.src_len > in_cap) {
            if (lane == 0) b.results[page] = kResultTooLarge;
            continue;
        }
        WAVE_SYNC();
        // the page first: its first vector also holds up to 15 bytes in front of the page, which
        // the dictionary's last bytes then replace
        const uint32_t head = stage_in(p.src, p.src_len, stage, lane, kWave);
        {
            const u32x4 *g = (const u32x4 *)(d.enc + (size_t)head * d.enc_stride);
            u32x4 *l = (u32x4 *)dstage;
            for (uint32_t v = lane; v < (DE >> 4); v += kWave) l[v] = g[v];
            if (DE && lane < head) stage[lane] = d.enc[(size_t)head * d.enc_stride + DE + lane];
            const u32x4 *gt = (const u32x4 *)seed;
            for (uint32_t w = lane; w < kTableSlots / 8; w += kWave) ((u32x4 *)table)[w] = gt[w];
        }
        WAVE_SYNC();
        uint8_t *in = stage + head;              // the page; window position 0 is in - DE
        in[p.src_len + lane] = 0;                // the parse's zero pad
        WAVE_SYNC();
        const int32_t rv = encode_page<false, true>(in, p.src_len, table, map, rec, stage_bits, p.dst, p.dst_cap,
                                                    ws + (size_t)blockIdx.x * ws_stride, ws_stride, lane, nullptr, DE,
                                                    d.adler);
        if (lane == 0) b.results[page] = rv;
    }
}

}  // namespace

// The dictionary parse's table as a page finds it: 8 positions per bucket of the dictionary tail's
// n = D & ~63 bytes, keyed as parse_page<false, true, 8> keys its own inserts (bucket_of<8> of 3 bytes),
// for every position whose three bytes lie inside the tail, most recent first.  A bucket that more
// than 8 positions fall into keeps 8 of them at evenly spaced ranks, its latest and its earliest
// included: a 16 KiB tail puts 32 positions into a bucket, and with the 8 latest kept nothing in its
// first three quarters could ever be found, while the page's own inserts push out the oldest way
// first whatever is kept.  An empty way is position 0, as in a zeroed table (a candidate is verified
// by its bytes).
size_t zlib_dict_seed_bytes() { return kTableSlots * sizeof(uint16_t); }
void zlib_dict_seed_table(const uint8_t *tail, uint32_t n, void *table_out) {
    constexpr uint32_t nb = kTableSlots / kWays;
    static_assert(nb == 512, "bucket_of<8>: the high 9 bits of the product");
    uint16_t *T = (uint16_t *)table_out;
    std::fill(T, T + kTableSlots, (uint16_t)0);
    std::vector<std::vector<uint16_t>> in_bucket(nb);
    for (uint32_t j = 0; j + 3u <= n; j++) {
        const uint32_t v = (uint32_t)tail[j] | ((uint32_t)tail[j + 1] << 8) | ((uint32_t)tail[j + 2] << 16);
        in_bucket[(v * 2654435761u) >> 23].push_back((uint16_t)j);
    }
    for (uint32_t h = 0; h < nb; h++) {
        const std::vector<uint16_t> &p = in_bucket[h];   // ascending
        const uint32_t m = (uint32_t)p.size();
        for (uint32_t w = 0; w < std::min(m, (uint32_t)kWays); w++) {
            // way w: rank m - 1 (the latest) down to rank 0
            const uint32_t rank = m <= (uint32_t)kWays ? m - 1u - w : ((kWays - 1u - w) * (m - 1u) + (kWays - 1u) / 2u) / (kWays - 1u);
            T[h * kWays + w] = p[rank];
        }
    }
}

// seed: the handle's seeded table on this device.  per_page: pages beyond the reach are skipped; else
// in_cap + D must not exceed 65,536.  ZLIB_HC is not asked: a dictionary call is the dictionary encoder's.
hipError_t launch_zlib_deflate_dict(const tyche_batch_t &b, uint32_t in_cap, const Lz4DictDev &d, const void *seed,
                                    bool per_page, hipStream_t s) {
    if (b.count == 0) return hipSuccess;
    if ((uint64_t)in_cap + d.dlen > 65536u || in_cap > 65535u || d.enc_len > d.dlen || (d.enc_len & 63u) || !seed)
        return hipErrorInvalidValue;
    const size_t lds = kFrontZD + d.enc_len + ((in_cap + 16u + kPad + 15u) & ~15u);
    const size_t grid = page_grid((const void *)zlib_deflate_dict_kernel, kWave, lds, b.count);
    WorkCounter ctr(s, grid < b.count);
    if (!ctr.get()) return hipErrorOutOfMemory;
    // per-wave record scratch, as launch_zlib_deflate: L / 3 + 2 records of 8 bytes
    const uint32_t ws_stride = ((in_cap / 3u + 3u) * 8u + 255u) & ~255u;
    ScratchLease ws(s, grid * (size_t)ws_stride);
    if (!ws.get()) return hipErrorOutOfMemory;   // the kernel writes its records there
    hipLaunchKernelGGL(zlib_deflate_dict_kernel, dim3((unsigned)grid), dim3(kWave), lds, s, b, in_cap, d,
                       (const uint32_t *)seed, per_page ? 1u : 0u, grid < b.count ? ctr.get() : nullptr, (uint8_t *)ws.get(),
                       ws_stride);
    return hipGetLastError();
}

}  // namespace tyche
