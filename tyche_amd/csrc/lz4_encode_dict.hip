// lz4_encode_dict.hip -- batched LZ4 block encode with a shared dictionary
// (tyche_lz4_compress_batch_dict, and the host entry points once a process-wide
// dictionary is installed).
//
// A dictionary of D bytes followed by a page of L bytes is one LZ4 window
// (L + D <= 65536): the page becomes a standard LZ4 block whose offsets may
// reach back into the dictionary, exactly what LZ4_decompress_safe_usingDict
// (lz4.c:1382) restores -- the reference's stream mode (LZ4_loadDict +
// LZ4_compress_fast_continue, lz4.c:936, 987) with a parse of our own.
//
// One 64-lane wave per page, looping over pages it claims.  Per page the wave
// stages  [ table | records | dictionary tail | page ]  in LDS:
//   * the dictionary's last D' = D & ~63 bytes stand right before the page's
//     first byte, so window position p is LDS byte p and lz_parse.h's parse_page
//     runs unchanged from start = D' (its "earlier bytes are history" mode: the
//     split encoders' second waves use it the same way);
//   * the table -- 2^12 16-bit window positions, the size of the reference's
//     stream-mode table -- starts as the handle's read-only dictionary table
//     (every dictionary position hashed by its 5 bytes as the reference's
//     stream mode does, the last of equal hashes kept; built once on the host,
//     8 KiB), so a page's first positions find the dictionary
//     without any seeding work per page, and the page's own positions then
//     replace dictionary entries as the reference's single table does;
//   * the page is staged by whole 16-byte vectors (stage_in: it lands at byte
//     src & 15 of its first vector), so the dictionary has to end at any of 16
//     byte shifts: the handle's device image holds the tail at all 16 (D' + 16
//     bytes each), and the one for this page is copied by vectors too.  It stays
//     in L2 for the whole batch.
// The parse's records go through lz4_dict_core.h's emission (offsets are window
// distances, whichever side of the seam the candidate is on).  The end-of-block
// rules are the plain encoder's: the last match starts at or before L-12 and
// ends at or before L-5 of the page.
//
// LDS per page: 8 KiB table + 512 B records + D' + 16 + the page's vectors + 64
// zero bytes -- 28.6 KiB at D = 4 KiB, L = 16 KiB: 5 pages per CU (the plain
// four-wave encoder: 31.5 KiB and 5).
#include <hip/hip_runtime.h>

#define TYCHE_HASH_LOG 12   // lz_parse.h's table in this translation unit: lzd::kHashLogD
#define TYCHE_PARSE_HASH5 1 // keyed by 5 bytes (lz_parse.h), as the handle's dictionary table is

#include <algorithm>

#include "engine.h"
#include "lds_io.h"
#include "lz_parse.h"

#define LZD_HOST 0
#include "lz4_dict_core.h"

namespace tyche {

namespace {

using lzp::kWave;
static_assert(lzp::kHashLog == lzd::kHashLogD, "the handle's dictionary table is hashed for this parse");
constexpr uint32_t kPadD = 64;
constexpr size_t kTableBytesD = lzd::kTableSizeD * sizeof(uint16_t);
constexpr size_t kRecBytesD = kWave * sizeof(uint2);

// LDS in front of the window: table | records
constexpr size_t kFrontD = kTableBytesD + kRecBytesD;

__host__ __device__ inline uint32_t page_vec_bytes(uint32_t in_cap) { return (in_cap + 16u + kPadD + 15u) & ~15u; }

// per_page: the host entry points' reach rule -- a page with src_len + D > 65536 is not this
// kernel's (its result is left alone: another launch over the same batch owns it)
__global__ __launch_bounds__(64) void lz4_encode_dict_kernel(tyche_batch_t b, uint32_t in_cap, Lz4DictDev d,
                                                              uint32_t per_page, unsigned *ctr) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x;
    uint16_t *table = (uint16_t *)smem;
    uint2 *rec = (uint2 *)(smem + kTableBytesD);
    uint8_t *dstage = smem + kFrontD;            // the dictionary tail's vectors (enc_len + 16 bytes)
    uint8_t *stage = dstage + d.enc_len;         // the page's vectors (enc_len is a multiple of 64)
    const uint32_t DE = d.enc_len;

    for (size_t page = blockIdx.x; page < b.count; page = claim_page(ctr, lane)) {
        const PageRef p = batch_page(b, page);
        if (per_page && (uint64_t)p.src_len + d.dlen > lzd::kWindowMax) continue;
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
            const uint32_t nvec = DE >> 4;       // whole vectors; the last, partial one goes by bytes
            for (uint32_t v = lane; v < nvec; v += kWave) l[v] = g[v];
            if (DE && lane < head) stage[lane] = d.enc[(size_t)head * d.enc_stride + DE + lane];
            const u32x4 *gt = (const u32x4 *)d.table;
            for (uint32_t w = lane; w < kTableBytesD / 16; w += kWave) ((u32x4 *)table)[w] = gt[w];
        }
        WAVE_SYNC();
        uint8_t *in = dstage + head;             // window position 0
        const uint32_t W = DE + p.src_len;       // the window's end
        in[W + lane] = 0;                        // the parse's zero pad
        WAVE_SYNC();
        uint32_t op = 0;
        auto sink = [&](const uint2 *rr, uint32_t n, uint32_t anchor) -> bool {
            const bool ok = lzd::emit_records((const lzd::Rec *)rr, n, anchor, in, p.dst, op, p.dst_cap, lane);
            WAVE_SYNC();
            return ok;
        };
        const uint32_t anchor = lzp::parse_page(in, W, table, rec, lane, sink, DE);
        int32_t rv = 0;
        if (anchor != 0xFFFFFFFFu && lzd::write_last_literals(in, anchor, W, p.dst, op, p.dst_cap, lane)) rv = (int32_t)op;
        if (lane == 0) b.results[page] = rv;
    }
}

}  // namespace

hipError_t launch_lz4_encode_dict(const tyche_batch_t &b, uint32_t in_cap, const Lz4DictDev &d, bool per_page,
                                  hipStream_t s) {
    if (b.count == 0) return hipSuccess;
    if ((uint64_t)in_cap + d.dlen > lzd::kWindowMax || d.enc_len > d.dlen || (d.enc_len & 63u)) return hipErrorInvalidValue;
    const size_t lds = kFrontD + d.enc_len + page_vec_bytes(in_cap);
    const size_t grid = page_grid((const void *)lz4_encode_dict_kernel, kWave, lds, b.count);
    WorkCounter ctr(s, grid < b.count);
    if (!ctr.get()) return hipErrorOutOfMemory;
    hipLaunchKernelGGL(lz4_encode_dict_kernel, dim3((unsigned)grid), dim3(kWave), lds, s, b, in_cap, d,
                       per_page ? 1u : 0u, ctr.get());
    return hipGetLastError();
}

}  // namespace tyche
