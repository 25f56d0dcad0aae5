// page_order.hip -- the ordering pass of the lane-per-page launches: a stable
// counting sort of the batch's pages by descending stream-length bin inside
// windows of consecutive pages (the rule, the geometry and the slot map are
// page_order_core.h's, shared with the host emulator tools/page_order_emul.cpp).
//
// Three launches on the caller's stream, none waiting for another workgroup:
//   hist     one wave per tile of kTile pages counts its pages per key in LDS and
//            writes the kBins counts to hist[tile][key]
//   scan     one workgroup per window, one thread per key: the exclusive prefix of
//            the key's counts over the window's tiles (in place), then the
//            exclusive prefix of the keys' totals into base[window][key]
//   scatter  the tile's wave starts its LDS counters at window start + base + tile
//            prefix and walks its pages 64 at a time in page order: lanes with
//            the same key rank themselves by ballots, the last of them advances
//            the counter.  No global atomic; the result depends on the lengths
//            alone.
// Scratch of one pass (page_order_work_bytes): hist | base.
#include <hip/hip_runtime.h>

#include "engine.h"

#define PO_HOST 0
#include "page_order_core.h"

namespace tyche {

namespace {

constexpr uint32_t kSteps = po::kTile / po::kLanes;
static_assert(po::kTile % po::kLanes == 0 && po::kBins % po::kLanes == 0, "whole steps of one wave");
static_assert(po::kBins == 512, "the scatter's ballots cover 9 key bits; the scan runs one thread per key");

__global__ __launch_bounds__(64) void page_order_hist_kernel(const uint32_t *lengths, uint32_t in_cap, uint32_t shift, po::Geo g,
                                                             uint32_t *hist) {
    __shared__ uint32_t cnt[po::kBins];
    const uint32_t lane = threadIdx.x, tile = blockIdx.x;
    for (uint32_t k = lane; k < po::kBins; k += po::kLanes) cnt[k] = 0;
    __syncthreads();
    uint32_t first, end;
    po::tile_bounds(g, tile, &first, &end);
#pragma unroll 8
    for (uint32_t s = 0; s < kSteps; s++) {
        const uint64_t i = (uint64_t)first + s * po::kLanes + lane;
        if (i < end) atomicAdd(&cnt[po::rank_key(lengths[i], in_cap, shift)], 1u);
    }
    __syncthreads();
    for (uint32_t k = lane; k < po::kBins; k += po::kLanes) hist[(size_t)tile * po::kBins + k] = cnt[k];
}

__global__ __launch_bounds__(po::kBins) void page_order_scan_kernel(po::Geo g, uint32_t *hist, uint32_t *base) {
    __shared__ uint32_t buf[2 * po::kBins];
    const uint32_t k = threadIdx.x, w = blockIdx.x;
    uint32_t run = 0;
    uint32_t *p = hist + (size_t)w * g.tpw * po::kBins + k;
#pragma unroll 8
    for (uint32_t j = 0; j < g.tpw; j++) {
        const uint32_t v = p[(size_t)j * po::kBins];
        p[(size_t)j * po::kBins] = run;
        run += v;
    }
    uint32_t cur = 0;
    buf[k] = run;
    __syncthreads();
#pragma unroll
    for (uint32_t d = 1; d < po::kBins; d <<= 1) {
        const uint32_t x = buf[cur + k] + (k >= d ? buf[cur + k - d] : 0u);
        cur ^= po::kBins;
        buf[cur + k] = x;
        __syncthreads();
    }
    base[(size_t)w * po::kBins + k] = buf[cur + k] - run;
}

__global__ __launch_bounds__(64) void page_order_scatter_kernel(const uint32_t *lengths, uint32_t in_cap, uint32_t shift, po::Geo g,
                                                                const uint32_t *hist, const uint32_t *base, uint32_t *order) {
    __shared__ uint32_t cnt[po::kBins];
    const uint32_t lane = threadIdx.x, tile = blockIdx.x;
    uint32_t first, end;
    po::tile_bounds(g, tile, &first, &end);
    if (first >= end) return;
    const uint32_t w = tile / g.tpw, w0 = po::window_first(g, w);
    for (uint32_t k = lane; k < po::kBins; k += po::kLanes)
        cnt[k] = w0 + base[(size_t)w * po::kBins + k] + hist[(size_t)tile * po::kBins + k];
    uint32_t key[kSteps];
#pragma unroll
    for (uint32_t s = 0; s < kSteps; s++) {
        const uint64_t i = (uint64_t)first + s * po::kLanes + lane;
        key[s] = i < end ? po::rank_key(lengths[i], in_cap, shift) : 0u;
    }
    __syncthreads();
    const uint64_t below = ((uint64_t)1 << lane) - 1u;
#pragma unroll
    for (uint32_t s = 0; s < kSteps; s++) {
        const uint64_t i = (uint64_t)first + s * po::kLanes + lane;
        const bool valid = i < end;
        if (__ballot(valid) == 0) break;   // (wave-uniform: the tile's pages are consecutive)
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (uint32_t bit = 0; bit < 9; bit++) {
            const bool one = (key[s] >> bit) & 1u;
            const uint64_t m = __ballot(valid && one);
            peers &= one ? m : ~m;
        }
        const uint32_t at = valid ? cnt[key[s]] : 0u;
        __syncthreads();
        if (valid && (peers >> lane) == 1u) cnt[key[s]] = at + (uint32_t)__popcll(peers);   // the last of its peers
        __syncthreads();
        const uint32_t pos = at + (uint32_t)__popcll(peers & below);
        if (valid && pos < g.count) order[pos] = (uint32_t)i;
    }
}

}  // namespace

bool page_order_fits(size_t count, uint32_t window) {
    return count > 0 && count <= 0x7FFFFFFFu && po::geometry_ok((uint32_t)count, window);
}

size_t page_order_work_bytes(size_t count, uint32_t window) {
    const po::Geo g = po::geometry((uint32_t)count, window);
    return ((size_t)g.ntiles + g.nwin) * po::kBins * sizeof(uint32_t);
}

hipError_t launch_page_order(const uint32_t *lengths, size_t count, uint32_t in_cap, uint32_t window, uint32_t *order, void *work,
                             hipStream_t s) {
    const po::Geo g = po::geometry((uint32_t)count, window);
    const uint32_t shift = po::bin_shift(in_cap);
    uint32_t *hist = (uint32_t *)work, *base = hist + (size_t)g.ntiles * po::kBins;
    page_order_hist_kernel<<<g.ntiles, 64, 0, s>>>(lengths, in_cap, shift, g, hist);
    page_order_scan_kernel<<<g.nwin, po::kBins, 0, s>>>(g, hist, base);
    page_order_scatter_kernel<<<g.ntiles, 64, 0, s>>>(lengths, in_cap, shift, g, hist, base, order);
    return hipGetLastError();
}

}  // namespace tyche

// Diagnostic and test hook: runs only the ordering pass over batch->src_lengths on the default
// stream, waits, and copies the order to out (batch->count host entries).  0, or 1 when the batch
// has no src_lengths or no ordinary count, or 2 for a device error.
extern "C" int tyche_debug_lz4_page_order(const tyche_batch_t *batch, uint32_t in_cap, uint32_t window, uint32_t *out) {
    using namespace tyche;
    if (!batch || !out || !batch->src_lengths || batch->count == 0 || !page_order_fits(batch->count, window)) return 1;
    const size_t order_bytes = (batch->count * sizeof(uint32_t) + 255u) & ~(size_t)255u;
    ScratchLease ws(nullptr, order_bytes + page_order_work_bytes(batch->count, window));
    if (!ws.get()) return 2;
    uint32_t *order = (uint32_t *)ws.get();
    if (launch_page_order(batch->src_lengths, batch->count, in_cap, window, order, (uint8_t *)ws.get() + order_bytes, nullptr) !=
        hipSuccess)
        return 2;
    return hipMemcpy(out, order, batch->count * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess ? 0 : 2;
}
