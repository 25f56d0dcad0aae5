// pack.hip -- the packed compressed-page store (tyche_pack_batch):
// gathers the streams a compress batch left in its slots into one arena, each at
// its compressed size.  The rule and the copy's geometry are pack_core.h's,
// shared with tyche_pack_plan and the host emulator tools/pack_emul.cpp.
//
// Four launches on the caller's stream, none waiting for another workgroup (no
// look-back, no flags: each launch starts when the one before it has finished):
//   sums    one 256-thread workgroup per kScanPages pages adds up their rooms
//           (round_up(len, align)) into one 64-bit tile sum
//   scan    ONE workgroup turns the tile sums into exclusive prefixes, kFanIn per
//           round with a running carry, then decides the append (pk::decide) from
//           state[] and writes the pk::Plan into the launch's scratch
//   apply   the sums grid again: every page's offset = o_0 + tile prefix + the
//           prefix inside the tile; writes offsets[], lengths[], and -- one lane
//           of workgroup 0, plain vector stores -- state[]
//   copy    one-wave workgroups claim destination tiles of kTile bytes from a
//           WorkCounter (pk::copy_tile); a refused batch has no tiles and the
//           kernel reads that from the Plan and returns at once
// Scratch of one call: Plan (64 B) | one uint64 per sums workgroup.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "lds_io.h"
#include "byte_funnel.h"

#define PK_HOST 0
#include "pack_core.h"

namespace tyche {

namespace {

constexpr uint32_t kPlanBytes = 64;
static_assert(sizeof(pk::Plan) <= kPlanBytes, "the tile sums follow the Plan in the scratch");

typedef unsigned long long u64;

// exclusive prefix of v over the workgroup's 256 threads and their total; buf: 2 x 256 entries
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t *buf, uint32_t t, uint64_t *total) {
    uint32_t cur = 0;
    buf[t] = v;
    __syncthreads();
#pragma unroll
    for (uint32_t d = 1; d < pk::kScanThreads; d <<= 1) {
        const uint64_t x = buf[cur + t] + (t >= d ? buf[cur + t - d] : 0u);
        cur ^= pk::kScanThreads;
        buf[cur + t] = x;
        __syncthreads();
    }
    const uint64_t incl = buf[cur + t];
    *total = buf[cur + pk::kScanThreads - 1u];
    __syncthreads();   // buf is free again
    return incl - v;
}

__global__ __launch_bounds__(pk::kScanThreads) void pack_sums_kernel(const int32_t *results, uint32_t n, uint32_t max_length,
                                                                     uint32_t align, uint64_t *sums) {
    __shared__ uint64_t buf[2 * pk::kScanThreads];
    const uint32_t t = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * pk::kScanPages;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < pk::kPagesPerThread; k++) {
        const uint64_t i = first + k * pk::kScanThreads + t;
        if (i < n) v += pk::room(results[i], max_length, align);
    }
    uint64_t total;
    (void)block_scan(v, buf, t, &total);
    if (t == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(pk::kScanThreads) void pack_scan_kernel(uint64_t *sums, uint32_t nsums, const int32_t *results,
                                                                     uint32_t n, uint32_t max_length, uint32_t align,
                                                                     uint64_t capacity, uint32_t skew, const uint64_t *state,
                                                                     pk::Plan *plan) {
    __shared__ uint64_t buf[2 * pk::kScanThreads];
    const uint32_t t = threadIdx.x;
    uint64_t carry = 0;
    for (uint32_t c = 0; c < nsums; c += pk::kFanIn) {
        const uint32_t i = c + t;
        const uint64_t v = i < nsums ? sums[i] : 0u;
        uint64_t total;
        const uint64_t ex = block_scan(v, buf, t, &total);
        if (i < nsums) sums[i] = carry + ex;
        carry += total;
    }
    if (t == 0) *plan = pk::decide(state[0], state[1], carry, pk::page_len(results[n - 1u], max_length), align, capacity, skew);
}

__global__ __launch_bounds__(pk::kScanThreads) void pack_apply_kernel(const int32_t *results, uint32_t n, uint32_t max_length,
                                                                      uint32_t align, const uint64_t *sums, const pk::Plan *plan,
                                                                      uint64_t *state, uint64_t *offsets, uint32_t *lengths) {
    __shared__ uint64_t buf[2 * pk::kScanThreads];
    const uint32_t t = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * pk::kScanPages + (uint64_t)t * pk::kPagesPerThread;
    uint32_t len[pk::kPagesPerThread];
    uint64_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < pk::kPagesPerThread; k++) {
        len[k] = first + k < n ? pk::page_len(results[first + k], max_length) : 0u;
        v += pk::round_up(len[k], align);
    }
    uint64_t total;
    uint64_t o = plan->base + sums[blockIdx.x] + block_scan(v, buf, t, &total);
#pragma unroll
    for (uint32_t k = 0; k < pk::kPagesPerThread; k++) {
        if (first + k < n) {
            offsets[first + k] = o;
            lengths[first + k] = len[k];
        }
        o += pk::round_up(len[k], align);
    }
    if (blockIdx.x == 0 && t == 0) {
        state[0] = plan->state0;
        state[1] = plan->end;
    }
}

// ---- the copy
typedef __attribute__((address_space(1))) u32x4 g_u32x4_w;

struct CopyOps {
    const tyche_pack_t &p;
    uint32_t lane;

    __device__ __forceinline__ uint32_t probes_true(uint32_t a, uint32_t b, uint32_t step, uint64_t lo) const {
        const uint32_t at = pk::probe_at(a, step, lane);
        const bool holds = at < b && p.offsets[at] <= lo;
        return (uint32_t)__popcll(__ballot(holds));
    }
    __device__ __forceinline__ void page(uint32_t i, uint64_t *o, uint32_t *len) const {
        *o = ld_meta(p.offsets, i);
        *len = ld_meta(p.lengths, i);
    }
    // bytes [skip, skip + n) of page i's stream to arena + dst: the head and the tail of the piece
    // byte by byte (lanes 0..15 and 16..31), the whole destination lines between them as one 16-byte
    // store each, from the two aligned 16-byte source lines that hold their bytes
    __device__ __forceinline__ void copy(uint32_t i, uint32_t skip, uint64_t dst, uint32_t n) const {
        const uint64_t so = p.src_offsets ? ld_meta(p.src_offsets, i) : (uint64_t)i * p.src_stride;
        const uint8_t *s = (const uint8_t *)p.src + so + skip;
        uint8_t *d = (uint8_t *)p.arena + dst;
        const pk::Split sp = pk::split_piece((uint32_t)((uintptr_t)d & 15u), n);
        if (lane < sp.head) d[lane] = s[lane];
        const uint32_t body = sp.head + sp.lines * pk::kLine;
        if (lane >= 16u && lane - 16u < sp.tail) d[body + lane - 16u] = s[body + lane - 16u];
        if (sp.lines == 0) return;
        const uint8_t *sb = s + sp.head;
        const uint32_t shift = (uint32_t)((uintptr_t)sb & 15u);   // the same for every line of the piece
        const u32x4 *g = (const u32x4 *)(sb - shift);
        u32x4 *out = (u32x4 *)(d + sp.head);
        if (shift == 0) {
            uint32_t v = lane;
            for (; v + 3u * 64u < sp.lines; v += 4u * 64u) {   // 4 loads in flight per lane
                const u32x4 x0 = gload_nt(g + v), x1 = gload_nt(g + v + 64u), x2 = gload_nt(g + v + 128u),
                            x3 = gload_nt(g + v + 192u);
                __builtin_nontemporal_store(x0, (g_u32x4_w *)(uintptr_t)(out + v));
                __builtin_nontemporal_store(x1, (g_u32x4_w *)(uintptr_t)(out + v + 64u));
                __builtin_nontemporal_store(x2, (g_u32x4_w *)(uintptr_t)(out + v + 128u));
                __builtin_nontemporal_store(x3, (g_u32x4_w *)(uintptr_t)(out + v + 192u));
            }
            for (; v < sp.lines; v += 64u) __builtin_nontemporal_store(gload_nt(g + v), (g_u32x4_w *)(uintptr_t)(out + v));
            return;
        }
        // line v takes bytes [shift, shift + 16) of source lines v and v + 1; with shift > 0 the last
        // source line read still holds the last byte of the piece's whole lines
        const bool hi8 = shift >= 8u;
        const uint32_t r = shift & 7u;
        uint32_t v = lane;
        for (; v + 64u < sp.lines; v += 2u * 64u) {   // 4 loads in flight per lane
            const u32x4 a0 = gload_nt(g + v), b0 = gload_nt(g + v + 1u), a1 = gload_nt(g + v + 64u), b1 = gload_nt(g + v + 65u);
            __builtin_nontemporal_store(funnel16(a0, b0, hi8, r), (g_u32x4_w *)(uintptr_t)(out + v));
            __builtin_nontemporal_store(funnel16(a1, b1, hi8, r), (g_u32x4_w *)(uintptr_t)(out + v + 64u));
        }
        for (; v < sp.lines; v += 64u)
            __builtin_nontemporal_store(funnel16(gload_nt(g + v), gload_nt(g + v + 1u), hi8, r), (g_u32x4_w *)(uintptr_t)(out + v));
    }
    // bytes [8 * hi8 + r, + 16) of the 32 bytes a : b
    static __device__ __forceinline__ u32x4 funnel16(u32x4 a, u32x4 b, bool hi8, uint32_t r) {
        const uint64_t q0 = (uint64_t)a.x | ((uint64_t)a.y << 32), q1 = (uint64_t)a.z | ((uint64_t)a.w << 32);
        const uint64_t q2 = (uint64_t)b.x | ((uint64_t)b.y << 32), q3 = (uint64_t)b.z | ((uint64_t)b.w << 32);
        const uint64_t lo = funnel8(hi8 ? q1 : q0, hi8 ? q2 : q1, r);
        const uint64_t hi = funnel8(hi8 ? q2 : q1, hi8 ? q3 : q2, r);
        u32x4 o;
        o.x = (uint32_t)lo;
        o.y = (uint32_t)(lo >> 32);
        o.z = (uint32_t)hi;
        o.w = (uint32_t)(hi >> 32);
        return o;
    }
};

__global__ __launch_bounds__(64) void pack_copy_kernel(tyche_pack_t p, const pk::Plan *plan, uint32_t skew, unsigned *counter) {
    const uint32_t lane = threadIdx.x;
    pk::Plan pl;
    pl.base = ld_meta(&plan->base, 0);
    pl.end = ld_meta(&plan->end, 0);
    pl.first_tile = ld_meta(&plan->first_tile, 0);
    pl.ntiles = ld_meta(&plan->ntiles, 0);   // 0 when the batch is refused
    pl.stored = 1;
    pl.state0 = 0;
    CopyOps ops{p, lane};
    for (size_t k = blockIdx.x; k < pl.ntiles; k = claim_page(counter, lane)) pk::copy_tile(ops, pl, (uint32_t)k, skew, (uint32_t)p.count);
}

}  // namespace

hipError_t launch_pack(const tyche_pack_t &p, hipStream_t s, const char **step) {
    const uint32_t n = (uint32_t)p.count;
    const uint32_t nsums = (n + pk::kScanPages - 1u) / pk::kScanPages;
    const uint32_t skew = (uint32_t)((uintptr_t)p.arena & pk::kSkewMask);
    *step = "workspace";
    ScratchLease scratch(s, kPlanBytes + (size_t)nsums * sizeof(uint64_t));
    uint8_t *base = (uint8_t *)scratch.get();
    if (!base) return hipErrorOutOfMemory;
    pk::Plan *plan = (pk::Plan *)base;
    uint64_t *sums = (uint64_t *)(base + kPlanBytes);
    hipError_t e;
    *step = "plan launches";
    hipLaunchKernelGGL(pack_sums_kernel, dim3(nsums), dim3(pk::kScanThreads), 0, s, p.results, n, p.max_length, p.align, sums);
    hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(pk::kScanThreads), 0, s, sums, nsums, p.results, n, p.max_length, p.align,
                       p.arena_capacity, skew, (const uint64_t *)p.state, plan);
    hipLaunchKernelGGL(pack_apply_kernel, dim3(nsums), dim3(pk::kScanThreads), 0, s, p.results, n, p.max_length, p.align,
                       (const uint64_t *)sums, (const pk::Plan *)plan, p.state, p.offsets, p.lengths);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // The copy's grid is sized on the host, which knows neither o_0 nor end: from the most tiles a
    // stored batch can have -- the arena's, or with a declared max_length the batch's own.
    uint64_t most = p.arena_capacity / pk::kTile + 2u;
    if (p.max_length) most = std::min<uint64_t>(most, ((uint64_t)n * pk::round_up(p.max_length, p.align) + p.align) / pk::kTile + 2u);
    *step = "copy launch";
    const size_t grid = page_grid((const void *)pack_copy_kernel, 64, 0, (size_t)std::min<uint64_t>(most, 1u << 30));
    WorkCounter counter(s);
    if (!counter.get()) return hipErrorOutOfMemory;
    hipLaunchKernelGGL(pack_copy_kernel, dim3((unsigned)grid), dim3(64), 0, s, p, (const pk::Plan *)plan, skew, counter.get());
    return hipGetLastError();
}

uint64_t pack_plan_host(size_t n, const int32_t *results, uint32_t max_length, uint32_t align, uint64_t capacity,
                        uint64_t state[2], uint64_t *offsets, uint32_t *lengths) {
    if (n == 0) return state[1];
    uint64_t o = pk::round_up(state[1], align), total = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t len = pk::page_len(results[i], max_length);
        if (offsets) offsets[i] = o + total;
        if (lengths) lengths[i] = len;
        total += pk::round_up(len, align);
    }
    const pk::Plan pl = pk::decide(state[0], state[1], total, pk::page_len(results[n - 1], max_length), align, capacity, 0);
    state[0] = pl.state0;
    state[1] = pl.end;
    return pl.end;
}

}  // namespace tyche
