// lz4_dict_train.hip -- trains a shared LZ4 dictionary from a device-resident
// batch of sample pages (tyche_lz4_dict_train_batch).  The
// per-page and per-segment steps are lz4_train_core.h's, shared with the host
// emulator tools/lz4_train_emul.cpp; this file stages pages, hands them out and
// strings the passes together.
//
// Device memory of one training, sized from the batch before the first launch:
//   state (64 B) | table: 2^20 uint32 document frequencies, 4 MiB |
//   picks: dict_len / 128 segments in order of selection | ub: one uint32 per page
// Launches, all on the caller's stream, none waiting for another workgroup:
//   count   256-thread workgroups claim pages from a counter; a page is staged in
//           LDS beside a 2^18-bit bitmap (32 KiB) indexed by the key's own hash, a
//           quarter of the key space per walk, which lets only a page's first
//           occurrence of a key reach the table's integer atomicAdd.  Pages above the declared maximum raise a flag and
//           the pages' total length is summed, for the rules the host checks next.
//   per round (dict_len / 128 times, enqueued back to back):
//     score  workgroups claim pages; thread 0 passes over pages that cannot beat
//            the round's best so far (lz4_train_core.h: cannot_win).  A page is
//            staged, its positions' g summed per block of 8 into LDS, each
//            candidate summed from 16 LDS entries, and the page's best raised into
//            the round's best with one 64-bit atomicMax.
//     apply  one workgroup: copies the winning segment to picks, zeroes its
//            keys' slots, resets the round's best and the page counter.  A best of
//            0 sets `done`, which makes every later launch return at once.
// Integer atomics only: the bytes do not depend on arrival order.
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <vector>

#include "engine.h"
#include "lds_io.h"

#define LZT_HOST 0
#include "lz4_train_core.h"

namespace tyche {

namespace {

constexpr uint32_t kThreadsT = 256;
constexpr size_t kTableBytesT = (size_t)lzt::kTableSize * sizeof(uint32_t);
constexpr size_t kBitmapBytesT = (size_t)lzt::kBitmapWords * sizeof(uint32_t);

struct TrainState {
    unsigned long long best;          // the round's best candidate (lzt::pack_best), 0: none yet
    unsigned long long total_bytes;   // sum of the page lengths (count pass)
    uint32_t count_ctr, round_ctr;    // page claims of the count pass / of the current round
    uint32_t picks, done, too_long, pad;
    uint32_t reserved[6];
};
static_assert(sizeof(TrainState) == 64, "the state block's size is part of the scratch layout");

__host__ __device__ inline uint32_t stage_bytes(uint32_t in_cap) { return (in_cap + 16u + 15u) & ~15u; }
// The workgroup's control words open the dynamic LDS (no static __shared__: with any, raising the
// kernel's dynamic-LDS limit to the CU's whole 160 KiB is refused, prepare_launch).
struct Ctl {
    unsigned long long best;   // score pass: the page's best candidate
    uint32_t page, pad;        // the page thread 0 handed out
};
static_assert(sizeof(Ctl) == 16, "what follows the control words stays 16-byte aligned");

struct SrcRef {
    const uint8_t *src;
    uint32_t len;
};
__device__ inline SrcRef sample_page(const tyche_batch_t &b, uint32_t i) {
    const uint64_t so = b.src_offsets ? ld_meta(b.src_offsets, i) : (uint64_t)i * b.src_stride;
    return SrcRef{(const uint8_t *)b.src + so, b.src_lengths ? ld_meta(b.src_lengths, i) : b.src_length};
}

__global__ __launch_bounds__(kThreadsT) void lz4_train_count_kernel(tyche_batch_t b, uint32_t in_cap, uint32_t *table,
                                                                    TrainState *st) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Ctl *ctl = (Ctl *)smem;
    uint32_t *bitmap = (uint32_t *)(smem + sizeof(Ctl));
    uint8_t *stage = smem + sizeof(Ctl) + kBitmapBytesT;
    const uint32_t t = threadIdx.x, count = (uint32_t)b.count;
    for (uint32_t i = t; i < lzt::kBitmapWords; i += kThreadsT) bitmap[i] = 0;
    __syncthreads();
    for (uint32_t page = blockIdx.x; page < count;) {
        const SrcRef p = sample_page(b, page);
        if (p.len > in_cap) {
            if (t == 0) st->too_long = 1;
        } else {
            if (t == 0) atomicAdd(&st->total_bytes, (unsigned long long)p.len);
            const uint32_t head = stage_in(p.src, p.len, stage, t, kThreadsT);
            __syncthreads();
            lzt::count_page(stage + head, p.len, bitmap, table, t, kThreadsT);
        }
        if (t == 0) ctl->page = atomicAdd(&st->count_ctr, 1u) + gridDim.x;
        __syncthreads();
        page = ctl->page;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreadsT) void lz4_train_score_kernel(tyche_batch_t b, uint32_t in_cap, const uint32_t *table,
                                                                    uint32_t *ub, TrainState *st) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if (st->done) return;
    Ctl *ctl = (Ctl *)smem;
    uint8_t *stage = smem + sizeof(Ctl);
    lzt::Blk *blk = (lzt::Blk *)(smem + sizeof(Ctl) + stage_bytes(in_cap));
    const uint32_t t = threadIdx.x, count = (uint32_t)b.count;
    bool first = true;
    for (;;) {
        if (t == 0) {
            // the next page worth scoring: every claim advances the counter, so this ends
            uint32_t page = first ? blockIdx.x : atomicAdd(&st->round_ctr, 1u) + gridDim.x;
            while (page < count) {
                const uint32_t len = sample_page(b, page).len;
                const unsigned long long so_far = __hip_atomic_load(&st->best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (len >= lzt::kSeg && len <= in_cap && !lzt::cannot_win(ub[page], page, so_far)) break;
                page = atomicAdd(&st->round_ctr, 1u) + gridDim.x;
            }
            ctl->page = page;
            ctl->best = 0;
        }
        first = false;
        __syncthreads();
        const uint32_t page = ctl->page;
        if (page >= count) break;
        const SrcRef p = sample_page(b, page);
        const uint32_t head = stage_in(p.src, p.len, stage, t, kThreadsT);
        __syncthreads();
        lzt::score_page(stage + head, p.len, table, blk, page, &ctl->best, t, kThreadsT);
        if (t == 0) {
            const unsigned long long mine = ctl->best;
            ub[page] = (uint32_t)(mine >> 32);
            if (mine) atomicMax(&st->best, mine);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(lzt::kSeg) void lz4_train_apply_kernel(tyche_batch_t b, uint32_t *table, uint8_t *picks,
                                                                    uint32_t rounds, TrainState *st) {
    if (st->done) return;
    const unsigned long long best = st->best;
    const uint32_t k = st->picks, t = threadIdx.x;
    __syncthreads();   // everyone has read the state before thread 0 rewrites it
    if (best == 0 || k >= rounds) {
        if (t == 0) st->done = 1;
        return;
    }
    const SrcRef p = sample_page(b, lzt::best_page(best));
    lzt::apply_segment(p.src + lzt::best_start(best), table, picks + (size_t)k * lzt::kSeg, t, lzt::kSeg);
    if (t == 0) {
        st->picks = k + 1u;
        st->best = 0;
        st->round_ctr = 0;
    }
}

}  // namespace

hipError_t train_lz4_dict(const tyche_batch_t &b, uint32_t in_cap, uint32_t dict_len, hipStream_t s, uint8_t *dict_out,
                          TrainResult *res) {
    *res = TrainResult{};
    const uint32_t rounds = dict_len / lzt::kSeg;
    res->step = "arguments";
    if (b.count == 0 || b.count > lzt::kMaxPages || in_cap > lzt::kMaxPage || rounds == 0 || dict_len > TYCHE_LZ4_DICT_MAX)
        return hipErrorInvalidValue;
    const uint32_t count = (uint32_t)b.count;
    const size_t picks_bytes = (size_t)rounds * lzt::kSeg;
    const size_t ub_off = sizeof(TrainState) + kTableBytesT + picks_bytes;
    res->step = "workspace";
    ScratchLease scratch(s, ub_off + (size_t)count * sizeof(uint32_t));
    uint8_t *base = (uint8_t *)scratch.get();
    if (!base) return hipErrorOutOfMemory;
    TrainState *st = (TrainState *)base;
    uint32_t *table = (uint32_t *)(base + sizeof(TrainState));
    uint8_t *picks = base + sizeof(TrainState) + kTableBytesT;
    uint32_t *ub = (uint32_t *)(base + ub_off);
    hipError_t e;
    res->step = "clearing the workspace";
    if ((e = hipMemsetAsync(base, 0, ub_off, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(ub, 0xFF, (size_t)count * sizeof(uint32_t), s)) != hipSuccess) return e;

    const size_t lds_count = sizeof(Ctl) + kBitmapBytesT + stage_bytes(in_cap);
    const size_t grid_count = page_grid((const void *)lz4_train_count_kernel, kThreadsT, lds_count, count);
    res->step = "count pass";
    hipLaunchKernelGGL(lz4_train_count_kernel, dim3((unsigned)grid_count), dim3(kThreadsT), lds_count, s, b, in_cap, table, st);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    TrainState h;
    if ((e = hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    res->total_bytes = h.total_bytes;
    res->too_long = h.too_long != 0;
    if (res->too_long || h.total_bytes > TYCHE_LZ4_TRAIN_MAX_BYTES) return hipSuccess;   // the caller names the rule

    const size_t lds_score = sizeof(Ctl) + stage_bytes(in_cap) + ((size_t)in_cap / lzt::kStep + 1u) * sizeof(lzt::Blk);   // key_blocks(in_cap) entries
    const size_t grid_score = page_grid((const void *)lz4_train_score_kernel, kThreadsT, lds_score, count);
    res->step = "rounds";
    for (uint32_t r = 0; r < rounds; r++) {
        hipLaunchKernelGGL(lz4_train_score_kernel, dim3((unsigned)grid_score), dim3(kThreadsT), lds_score, s, b, in_cap, table,
                           ub, st);
        hipLaunchKernelGGL(lz4_train_apply_kernel, dim3(1), dim3(lzt::kSeg), 0, s, b, table, picks, rounds, st);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    res->step = "reading the picks back";
    std::vector<uint8_t> taken(picks_bytes);
    if ((e = hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(taken.data(), picks, picks_bytes, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    const uint32_t n = std::min(h.picks, rounds);
    for (uint32_t k = 0; k < n; k++)   // the first pick ends the dictionary
        memcpy(dict_out + (size_t)k * lzt::kSeg, taken.data() + (size_t)(n - 1u - k) * lzt::kSeg, lzt::kSeg);
    res->dict_len = n * lzt::kSeg;
    return hipSuccess;
}

}  // namespace tyche
