// engine.h -- internal interface between the C-ABI layer (engine.hip) and the
// gfx950 kernel files (the lz4_*, zlib_* and zstd_* .hip files, pagegen.hip):
// their launchers, the batch's page metadata, and the launch plumbing they
// share -- grid sizing, dynamic page assignment, scratch leases, knobs.
// The host batch pipeline is a translation unit of its own, host_batch.hip (its
// interface to engine.hip: host_batch.h; its chunk plan: host_chunk_core.h), and
// so is the shared-dictionary layer, dict.hip (its interface to engine.hip: dict.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>

#include "../../include/tyche_codec.h"

namespace tyche {

// results[i] value for a page that does not fit the launch's LDS sizing
// (caller passed max_src_length / dst_capacity smaller than a page's sizes)
constexpr int32_t kResultTooLarge = INT32_MIN;

// LZ4 block-format constants (lz4.c:264-281)
constexpr int kMinMatch = 4;
constexpr int kLastLiterals = 5;
constexpr int kMfLimit = 12;
constexpr int kRunMask = 15;

__host__ __device__ inline uint32_t lz4_bound(uint32_t n) {
    return n > 0x7E000000u ? 0u : n + n / 255u + 16u;  // LZ4_COMPRESSBOUND, lz4.h:148
}
// zstd 1.1.2 ZSTD_compressBound (zstd_compress.c:37): FSE_compressBound(n) + 12
inline uint32_t zstd_bound(uint32_t n) { return n + (n >> 7) + 512u + 12u; }
// zlib 1.2.8 compressBound (compress.c:74-78)
inline uint32_t zlib_bound(uint32_t n) { return n + (n >> 12) + (n >> 14) + (n >> 25) + 13u; }

// in_cap for a decode batch: the largest stream length (or a bound for unknown lengths)
inline uint32_t decode_in_cap(const tyche_batch_t &b, uint32_t fallback) {
    uint32_t in_cap = b.src_lengths ? b.max_src_length : b.src_length;
    if (b.src_lengths && in_cap == 0) in_cap = fallback;
    return in_cap;
}
// in_cap for an encode batch: the largest page length, 65,535 when per-page lengths come without a maximum
inline uint32_t encode_in_cap(const tyche_batch_t &b) { return decode_in_cap(b, 65535u); }

// page i of a batch
struct PageRef {
    const uint8_t *src;
    uint32_t src_len;
    uint8_t *dst;
    uint32_t dst_cap;
};

// Per-page metadata is never written by a kernel: read it through the constant
// address space so a wave-uniform index becomes a scalar load (s_load, its own
// lgkmcnt counter) instead of a vector load whose in-order vmcnt wait would also
// drain the previous page's output stores.
template <typename T>
__device__ __forceinline__ T ld_meta(const T *p, size_t i) {
    return ((const __attribute__((address_space(4))) T *)(uintptr_t)p)[i];
}

__device__ inline PageRef batch_page(const tyche_batch_t &b, size_t i) {
    PageRef r;
    uint64_t so = b.src_offsets ? ld_meta(b.src_offsets, i) : (uint64_t)i * b.src_stride;
    uint64_t dof = b.dst_offsets ? ld_meta(b.dst_offsets, i) : (uint64_t)i * b.dst_stride;
    r.src = (const uint8_t *)b.src + so;
    r.src_len = b.src_lengths ? ld_meta(b.src_lengths, i) : b.src_length;
    r.dst = (uint8_t *)b.dst + dof;
    r.dst_cap = b.dst_capacities ? ld_meta(b.dst_capacities, i) : b.dst_capacity;
    return r;
}

// The codec kernels run one 64-lane wave per workgroup: LDS ordering between
// lanes needs no s_barrier, and __syncthreads()'s workgroup fence would wait for
// every outstanding global load (the next page's prefetch) -- a code-motion
// barrier is all that is required.
#define WAVE_SYNC() __builtin_amdgcn_wave_barrier()

// Resident workgroups of `threads` threads per CU for a kernel at `lds` bytes
// of dynamic LDS, as the runtime computes it (LDS granules, VGPRs, the per-CU
// limits).  The page loops size their grids to exactly this: one more workgroup
// per CU than fits would run after a resident one finished its whole share of
// pages.  If the runtime gives no answer: what the LDS allows for one-wave
// workgroups, 1 for larger ones.
size_t blocks_per_cu(const void *kernel, uint32_t threads, size_t lds);
// The grid of a page-loop launch over `count` pages: prepare_launch, then
// min(count, CUs x blocks_per_cu), the blocks per CU capped by the knob
// `cap_knob` (a *_PAGES_PER_CU name; a literal, as knob() wants) when it is
// set above 0.  The grid claims pages when it is smaller than count.  A batch of
// no more pages than CUs takes one workgroup per page whatever fits, so the
// occupancy is not asked for: the restore path pays no host call here.
size_t page_grid(const void *kernel, uint32_t threads, size_t lds, size_t count, const char *cap_knob = nullptr);

hipError_t launch_lz4_decode(const tyche_batch_t &b, uint32_t in_cap, uint32_t out_cap, hipStream_t s,
                             bool allow_lane = true);
bool lz4_lane_decode_wanted(size_t count, uint32_t in_cap, uint32_t out_cap);
hipError_t launch_lz4_decode_lane(const tyche_batch_t &b, uint32_t in_cap, uint32_t out_cap, hipStream_t s);
// large batches, round 4: one page per quad, chunked (lz4_decode_quad.hip)
hipError_t launch_lz4_decode_quad(const tyche_batch_t &b, uint32_t in_cap, uint32_t out_cap, hipStream_t s);
// large batches, round 4: one page per lane, chunked, aligned LDS (lz4_decode_lc.hip)
hipError_t launch_lz4_decode_lc(const tyche_batch_t &b, uint32_t in_cap, uint32_t out_cap, hipStream_t s);
// The page order of a lane-per-page launch (page_order.hip; the rule is page_order_core.h's): order[]
// becomes the permutation of [0, count) that sorts every window of `window` consecutive pages (0: the
// whole batch) by descending bin of min(lengths[i], in_cap), equal bins in page order.  `work` is device
// scratch of page_order_work_bytes; page_order_fits says whether a batch can be ordered at all (its
// count fits the 32-bit entries and its window does not make the pass's tables unreasonably large).
bool page_order_fits(size_t count, uint32_t window);
size_t page_order_work_bytes(size_t count, uint32_t window);
hipError_t launch_page_order(const uint32_t *lengths, size_t count, uint32_t in_cap, uint32_t window, uint32_t *order, void *work,
                             hipStream_t s);
hipError_t launch_lz4_encode(const tyche_batch_t &b, uint32_t in_cap, hipStream_t s);
// LZ4_EXACT=1: the bytes and return value of LZ4 1.7.5's LZ4_compress_default (lz4_encode_exact.hip)
hipError_t launch_lz4_encode_exact(const tyche_batch_t &b, uint32_t in_cap, hipStream_t s);
// LZ4_HC=1: the same block format from a better parse -- 8-way bucket rings in LDS and a two-step lazy
// choice, one wave per page (lz4_encode_hc.hip; in_cap <= 65535).  64K x 16 KiB bench pages: ratio 3.053
// against 2.618, 86.2 ms against the default encoder's 3.8 ms and LZ4_EXACT's 53.7 ms; the decoders restore
// its streams unchanged, in 0.86x the time (profiles/lz4_hc_time.log).
hipError_t launch_lz4_encode_hc(const tyche_batch_t &b, uint32_t in_cap, hipStream_t s);
// pages above 65,535 bytes, up to TYCHE_LZ4_MAX_PAGE (lz4_encode_large.hip): the pages of at least min_len
// bytes; the results of shorter ones are left alone
hipError_t launch_lz4_encode_large(const tyche_batch_t &b, uint32_t in_cap, uint32_t min_len, hipStream_t s);
// launches beyond the LDS of the other decoders, up to TYCHE_LZ4_MAX_PAGE (lz4_decode_large.hip)
hipError_t launch_lz4_decode_large(const tyche_batch_t &b, uint32_t in_cap, uint32_t out_cap, hipStream_t s);
// A shared LZ4 dictionary's image on one device (dict.hip builds and uploads it once per handle
// and device): `dec` is dpad bytes (a multiple of 16) with the dictionary's dlen bytes at their end;
// `table` the 4,096 16-bit positions of the encoder's read-only dictionary table; `enc` 16 images
// of enc_stride = enc_len + 16 bytes, image h holding the dictionary's last enc_len = dlen & ~63
// bytes from byte h on (zeros around them).  `adler` is the adler32 of the dlen bytes, computed on
// the host when the handle is made: zlib's DICTID.
struct Lz4DictDev {
    const uint8_t *dec;
    const uint16_t *table;
    const uint8_t *enc;
    uint32_t dlen, dpad, enc_len, enc_stride, adler;
};
// LZ4 with a shared dictionary (lz4_encode_dict.hip, lz4_decode_dict.hip): dictionary + page is one
// window of at most 65,536 bytes.  per_page: pages beyond that reach are skipped, their results
// left alone (the host entry points run the plain kernels over the same batch for them); else
// in_cap / out_cap + dlen must not exceed it.
hipError_t launch_lz4_encode_dict(const tyche_batch_t &b, uint32_t in_cap, const Lz4DictDev &d, bool per_page,
                                  hipStream_t s);
hipError_t launch_lz4_decode_dict(const tyche_batch_t &b, uint32_t in_cap, uint32_t out_cap, const Lz4DictDev &d,
                                  bool per_page, hipStream_t s);
// LZ4_HC_DICT=1: the dictionary encoder's window and contract with LZ4_HC's parse -- 8-way bucket rings
// that start from the handle's seed, lz4_hc_dict_seed_bytes() bytes that lz4_hc_dict_seed_table computes
// on the host from the dictionary's last d.enc_len bytes (lz4_hc_dict_seed.hip; dict.hip builds and
// uploads it at the handle's first such compress on a device), and a two-step lazy choice, one wave per
// page (lz4_encode_hc_dict.hip).  The block is an ordinary dictionary block: launch_lz4_decode_dict
// restores it.
size_t lz4_hc_dict_seed_bytes();
void lz4_hc_dict_seed_table(const uint8_t *tail, uint32_t n, void *table_out);
hipError_t launch_lz4_encode_hc_dict(const tyche_batch_t &b, uint32_t in_cap, const Lz4DictDev &d, const void *seed,
                                     bool per_page, hipStream_t s);
// Trains a shared LZ4 dictionary of up to dict_len bytes (128 .. TYCHE_LZ4_DICT_MAX) from the batch's source
// pages on stream s and waits for it (lz4_dict_train.hip; the dst fields are ignored).  dict_out: dict_len
// host bytes.  hipSuccess with res->too_long (a page above in_cap <= 65535) or res->total_bytes above
// TYCHE_LZ4_TRAIN_MAX_BYTES means the training stopped after its count pass: the caller names the rule.
struct TrainResult {
    uint32_t dict_len = 0;   // bytes written to dict_out: 128 x picks, 0 when the pages share nothing
    bool too_long = false;
    uint64_t total_bytes = 0;
    const char *step = "";   // what was being done when an error is returned
};
hipError_t train_lz4_dict(const tyche_batch_t &b, uint32_t in_cap, uint32_t dict_len, hipStream_t s, uint8_t *dict_out,
                          TrainResult *res);
// The packed store (pack.hip; the rule is pack_core.h's): plan launches and the tiled copy of one
// tyche_pack_batch call (arguments already checked, count > 0); *step names what was being done when
// an error is returned.  pack_plan_host is the same rule over host arrays (tyche_pack_plan).
hipError_t launch_pack(const tyche_pack_t &p, hipStream_t s, const char **step);
uint64_t pack_plan_host(size_t n, const int32_t *results, uint32_t max_length, uint32_t align, uint64_t capacity,
                        uint64_t state[2], uint64_t *offsets, uint32_t *lengths);
hipError_t launch_zstd_encode(const tyche_batch_t &b, uint32_t in_cap, hipStream_t s);
// ZSTD_HC=1: the same frame format from a better parse -- the 8-way bucket rings of LZ4_HC, both repeat
// offsets as candidates, the candidate of the highest gain (4 * length - highbit(offset + 1)) and a two-step
// lazy choice on gains, as pass A1 of the four-pass encode for every batch size (zstd_encode.hip,
// zstd_hc_core.h; in_cap <= 65535).  launch_zstd_encode goes here when the knob is set.
hipError_t launch_zstd_encode_hc(const tyche_batch_t &b, uint32_t in_cap, hipStream_t s);
hipError_t launch_zlib_deflate(const tyche_batch_t &b, uint32_t in_cap, hipStream_t s);
// ZLIB_HC=1: the same stream format from a better parse -- 2^9 bucket rings of the 16 latest positions, the
// nearest lower lane, the candidate of the highest gain (length against the distance's extra bits) and a
// two-step lazy rule on gains (zlib_deflate_hc_kernel, zlib_hc_core.h; in_cap <= 65535) in front of the
// default encoder's tree and code passes.  launch_zlib_deflate goes here when the knob is set.
hipError_t launch_zlib_deflate_hc(const tyche_batch_t &b, uint32_t in_cap, hipStream_t s);
hipError_t launch_zlib_inflate(const tyche_batch_t &b, uint32_t out_cap, hipStream_t s);
hipError_t launch_zstd_decode(const tyche_batch_t &b, uint32_t in_cap, uint32_t out_cap, hipStream_t s);
// zstd with a shared raw-content dictionary (zstd_encode.hip, zstd_decode.hip): dictionary + page is
// one window of at most 65,536 bytes, the frame an ordinary one whose offsets may reach into the
// dictionary (ZSTD_compress_usingDict / ZSTD_decompress_usingDict).  The handle and its device image
// are the LZ4 dictionary's (Lz4DictDev: raw bytes are codec-agnostic); the encoder also takes the
// handle's seeded table, zstd_dict_seed_bytes() bytes that zstd_dict_seed_table computes on the host
// from the dictionary's last d.enc_len bytes (dict.hip builds and uploads it at the handle's first
// zstd compress on a device).  per_page as for LZ4: pages beyond the reach are skipped, their results
// left alone; else in_cap / out_cap + dlen must not exceed the window.
size_t zstd_dict_seed_bytes();
void zstd_dict_seed_table(const uint8_t *tail, uint32_t n, void *table_out);
hipError_t launch_zstd_encode_dict(const tyche_batch_t &b, uint32_t in_cap, const Lz4DictDev &d, const void *seed,
                                   bool per_page, hipStream_t s);
hipError_t launch_zstd_decode_dict(const tyche_batch_t &b, uint32_t in_cap, uint32_t out_cap, const Lz4DictDev &d,
                                   bool per_page, hipStream_t s);
// zlib with a shared dictionary (zlib_deflate_dict.hip; zlib_inflate.hip's zlib_inflate_dict_kernel):
// dictionary + page is one window of at most 65,536 bytes, the stream what deflateSetDictionary /
// inflateSetDictionary produce and take (header 78 3F and DICTID = d.adler; a page whose coded stream
// would not beat the stored form is the plain stored stream).  The handle and its image are the LZ4
// dictionary's; the encoder also takes a seeded table of its own, zlib_dict_seed_bytes() bytes that
// zlib_dict_seed_table computes on the host from the dictionary's last d.enc_len bytes.  The decoder
// is the serial one for every batch size and ignores in_cap.  per_page as for LZ4.
size_t zlib_dict_seed_bytes();
void zlib_dict_seed_table(const uint8_t *tail, uint32_t n, void *table_out);
hipError_t launch_zlib_deflate_dict(const tyche_batch_t &b, uint32_t in_cap, const Lz4DictDev &d, const void *seed,
                                    bool per_page, hipStream_t s);
hipError_t launch_zlib_inflate_dict(const tyche_batch_t &b, uint32_t in_cap, uint32_t out_cap, const Lz4DictDev &d,
                                    bool per_page, hipStream_t s);
// Dynamic page assignment.  The codec kernels run one-wave workgroups that loop
// over pages; when a CU holds a number of waves that is not a multiple of its 4
// SIMDs, the waves sharing a SIMD run slower than the lone ones, and static
// striding (page += gridDim.x) leaves the lone waves idle at the end.  Instead
// each wave starts at blockIdx.x and then claims pages from a per-launch
// counter.  A WorkCounter leases one zeroed device counter for one launch on
// stream s: constructed just before the launch (an async memset on s), it is
// returned to the device's pool when it goes out of scope, right after the
// launch call, as an event recorded on s -- the counter is handed out again
// only once that event has completed, i.e. once the kernel that claims pages
// from it has finished, whatever stream or thread asks next.
//
// claims = false: the launch's grid covers all its pages, so no wave ever claims
// one (every claim returns >= gridDim.x >= count whatever the counter holds):
// the counter is a shared scratch word, with no memset and no event -- two
// fewer stream operations on the small-batch latency path.
class WorkCounter {
  public:
    explicit WorkCounter(hipStream_t s, bool claims = true);
    ~WorkCounter();
    WorkCounter(const WorkCounter &) = delete;
    WorkCounter &operator=(const WorkCounter &) = delete;
    unsigned *get() const { return p_; }   // nullptr if no counter could be allocated

  private:
    hipStream_t s_;
    int dev_ = -1, idx_ = -1;
    unsigned *p_ = nullptr;
};
// A device scratch buffer of at least `bytes` for one launch on stream s,
// returned to the device's pool when it goes out of scope (right after the
// launch) as an event on s, and handed out again only once that event has
// completed -- the WorkCounter scheme for kernels that need workspace.
class ScratchLease {
  public:
    ScratchLease(hipStream_t s, size_t bytes);
    ~ScratchLease();
    ScratchLease(const ScratchLease &) = delete;
    ScratchLease &operator=(const ScratchLease &) = delete;
    void *get() const { return p_; }   // nullptr if no buffer could be allocated

  private:
    hipStream_t s_;
    int dev_ = -1, idx_ = -1;
    void *p_ = nullptr;
};
// Bytes held by the current device's scratch pool in leases no launch uses
// (freed on demand: callers sizing work by hipMemGetInfo may count them as free).
size_t scratch_idle_bytes();
// Per-device, thread-safe launch preparation: raises `kernel`'s dynamic-LDS
// limit to the CU's 160 KiB once per (device, kernel) and returns the current
// device's CU count.
size_t prepare_launch(const void *kernel);
// Tunables and kernel-path switches: TYCHE_<name> from the environment (read
// once per name), overridden in-process by tyche_set_knob -- read on every
// launch, so one process can A/B the paths (the parity tests switch them this
// way rather than with setenv, which would race getenv in other threads).
long knob(const char *name, long dflt);
__device__ __forceinline__ size_t claim_page(unsigned *counter, uint32_t lane) {
    unsigned v = 0;
    if (lane == 0) v = atomicAdd(counter, 1u);
    return (size_t)__builtin_amdgcn_readfirstlane(v) + gridDim.x;
}

hipError_t launch_pagegen(void *dst, uint64_t stride, uint32_t page_len, uint64_t seed, uint64_t first,
                          size_t count, uint32_t dist, hipStream_t s);

}  // namespace tyche
