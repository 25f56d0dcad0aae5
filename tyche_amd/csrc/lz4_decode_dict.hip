// lz4_decode_dict.hip -- batched LZ4 block decode with a shared dictionary
// (tyche_lz4_decompress_batch_dict, and the host entry points once a
// process-wide dictionary is installed): results[i] and the bytes are those of
// LZ4_decompress_safe_usingDict(stream, dst, n, capacity, dict, D) (lz4.c:1382).
//
// One kernel for every batch size: one 64-lane wave per workgroup, looping over
// the pages it claims, in the shape of lz4_decode_serial_kernel.  LDS holds
//     [ dictionary | output window | stream + 64 zero bytes ]
// with the dictionary's D bytes ending where the window starts (a 16-byte line),
// so a match that begins in the dictionary and runs over the seam -- an
// overlapping one included -- is the same copy as any other.  The dictionary is
// staged once per workgroup, not per page: the decoder only reads it.  The walk
// and its verdicts are lz4_dict_core.h's decode_page, shared with the host
// emulator; the page leaves LDS once, whole, so dst may be pinned host memory.
//
// LDS per workgroup: D rounded up to 16 + the largest capacity + the longest
// stream + 80: 36.2 KiB at D = 4 KiB and 16 KiB pages (4 workgroups per CU),
// 131.5 KiB at the 65,536-byte limit of dictionary + page (1 per CU).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine.h"
#include "lds_io.h"

#define LZD_HOST 0
#include "lz4_dict_core.h"

namespace tyche {

namespace {

constexpr uint32_t kWaveD = 64;
constexpr uint32_t kPadD = 64;   // zeroed tail after the staged stream

// per_page: the host entry points' reach rule -- a page with dst_cap + D > 65536 is not this
// kernel's (its result is left alone: another launch over the same batch owns it)
__global__ __launch_bounds__(64) void lz4_decode_dict_kernel(tyche_batch_t b, uint32_t in_cap, uint32_t out_cap,
                                                              Lz4DictDev d, uint32_t per_page, unsigned *ctr) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x;
    uint8_t *out = smem + d.dpad;                              // the page's window; the dictionary ends here
    uint8_t *stage = out + ((out_cap + 15u) & ~15u);
    {
        // d.dec: dpad bytes, the dictionary right-aligned in them
        const u32x4 *g = (const u32x4 *)d.dec;
        u32x4 *l = (u32x4 *)smem;
        for (uint32_t v = lane; v < (d.dpad >> 4); v += kWaveD) l[v] = g[v];
    }
    for (size_t page = blockIdx.x; page < b.count; page = claim_page(ctr, lane)) {
        const PageRef p = batch_page(b, page);
        if (per_page && (uint64_t)p.dst_cap + d.dlen > lzd::kWindowMax) continue;
        if (p.src_len > in_cap || p.dst_cap > out_cap) {
            if (lane == 0) b.results[page] = kResultTooLarge;
            continue;
        }
        WAVE_SYNC();
        const uint32_t head = stage_in(p.src, p.src_len, stage, lane, kWaveD);
        uint8_t *in = stage + head;
        WAVE_SYNC();
        in[p.src_len + lane] = 0;
        WAVE_SYNC();
        const int32_t rv = lzd::decode_page(in, (int32_t)p.src_len, out, (int32_t)p.dst_cap, (int32_t)d.dlen, lane);
        WAVE_SYNC();
        if (rv > 0) stage_out(p.dst, out, (uint32_t)rv, lane, kWaveD);
        if (lane == 0) b.results[page] = rv;
    }
}

}  // namespace

hipError_t launch_lz4_decode_dict(const tyche_batch_t &b, uint32_t in_cap, uint32_t out_cap, const Lz4DictDev &d,
                                  bool per_page, hipStream_t s) {
    if (b.count == 0) return hipSuccess;
    if ((uint64_t)out_cap + d.dlen > lzd::kWindowMax || d.dpad < d.dlen || (d.dpad & 15u)) return hipErrorInvalidValue;
    const size_t lds = d.dpad + ((out_cap + 15u) & ~15u) + ((in_cap + 16u + kPadD + 15u) & ~15u);
    if (lds > 160u * 1024u) return hipErrorInvalidValue;   // (a declared stream maximum beyond any the window can need)
    const size_t grid = page_grid((const void *)lz4_decode_dict_kernel, kWaveD, lds, b.count);
    WorkCounter ctr(s, grid < b.count);
    if (!ctr.get()) return hipErrorOutOfMemory;
    hipLaunchKernelGGL(lz4_decode_dict_kernel, dim3((unsigned)grid), dim3(kWaveD), lds, s, b, in_cap, out_cap, d,
                       per_page ? 1u : 0u, ctr.get());
    return hipGetLastError();
}

}  // namespace tyche
