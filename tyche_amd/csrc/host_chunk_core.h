// host_chunk_core.h -- the chunk plan of the host batch path (host_batch.hip) and the layout of a
// chunk's page table in a staging slot's meta buffer.  Plain C++, no HIP: host_batch.hip runs it
// and tools/host_chunk_emul.cpp exposes it to tests/test_host_chunk_emul.py, which holds it to a
// Python restatement of the rule.
//
// The rule (up16(x): x rounded up to 16):
//   chunk_bytes = max(1, HOST_CHUNK_MB) << 20
//   tot_in = sum up16(src_len), tot_out = sum up16(dst_cap), est = (tot_in + tot_out) / chunk_bytes
//   est >= 3 gates the async scatter and the ramp (each also has its knob)
//   quarter = max(chunk_bytes / 4, 1 MiB)
//   a chunk's limit is chunk_bytes; with the ramp on and rem = max(rem_in, rem_out), the bytes not
//   yet in a chunk: quarter for the first chunk, rem - quarter for a later one when
//   quarter < rem <= chunk_bytes + quarter
//   a chunk takes its first page whatever its size, then pages while both its input and its
//   output bytes stay within the limit
//   chunk c goes through staging slot c % kSlots
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace tyche {

constexpr int kSlots = 4;   // round 3: 4 x 32 MiB (was 3 x 64 MiB): the host path waited on streams ~30 % of a call

inline size_t up16(size_t x) { return (x + 15) & ~size_t(15); }

inline size_t host_chunk_bytes(long chunk_mb) { return (size_t)(chunk_mb > 1 ? chunk_mb : 1) << 20; }

// pages [first, first + count) of a host batch: their staged bytes and longest lengths
struct HostChunk {
    size_t first, count;
    size_t in_bytes, out_bytes;   // sums of up16(src_len), up16(dst_cap)
    uint32_t max_in, max_out;
};

// Cuts a batch into chunks of ~chunk_bytes of input AND of output capacity: a decompress batch's
// output is ~2.6x its input, so cutting by input alone made 3 chunks of 170 MiB of D2H each out
// of a 32K-page batch, too few to overlap the two copy directions.  Ramp: the first and the last
// chunk are a quarter chunk, so the pipeline fills (H2D + kernel before the first D2H) and drains
// (the last D2H + scatter, which nothing overlaps) on small chunks.
class ChunkCutter {
  public:
    ChunkCutter(size_t n, const uint32_t *src_len, const uint32_t *dst_cap, size_t chunk_bytes, bool ramp_wanted)
        : n_(n), src_len_(src_len), dst_cap_(dst_cap), chunk_bytes_(chunk_bytes) {
        whole_ = HostChunk{0, n, 0, 0, 0, 0};
        for (size_t j = 0; j < n; j++) take(whole_, j);
        rem_in_ = whole_.in_bytes;
        rem_out_ = whole_.out_bytes;
        ramp_ = ramp_wanted && pipelined();
    }
    const HostChunk &whole() const { return whole_; }   // the batch as one chunk (the zero-copy path)
    size_t estimate() const { return (whole_.in_bytes + whole_.out_bytes) / chunk_bytes_; }
    bool pipelined() const { return estimate() >= 3; }   // enough chunks for the async scatter and the ramp
    bool ramp() const { return ramp_; }
    size_t limit_of_next() const {
        if (!ramp_) return chunk_bytes_;
        const size_t quarter = chunk_bytes_ / 4 > (size_t(1) << 20) ? chunk_bytes_ / 4 : size_t(1) << 20;
        const size_t rem = rem_in_ > rem_out_ ? rem_in_ : rem_out_;
        if (cut_ == 0) return quarter;
        if (rem <= chunk_bytes_ + quarter && rem > quarter) return rem - quarter;
        return chunk_bytes_;
    }
    // the next chunk; false when every page has been handed out
    bool next(HostChunk *out) {
        if (first_ >= n_) return false;
        const size_t limit = limit_of_next();
        HostChunk c{first_, 0, 0, 0, 0, 0};
        size_t last = first_;
        while (last < n_ && (last == first_ || (c.in_bytes + up16(src_len_[last]) <= limit &&
                                                c.out_bytes + up16(dst_cap_[last]) <= limit)))
            take(c, last++);
        rem_in_ -= c.in_bytes;
        rem_out_ -= c.out_bytes;
        first_ = last;
        cut_++;
        *out = c;
        return true;
    }

  private:
    void take(HostChunk &c, size_t j) const {
        c.count = j + 1 - c.first;
        c.in_bytes += up16(src_len_[j]);
        c.out_bytes += up16(dst_cap_[j]);
        if (src_len_[j] > c.max_in) c.max_in = src_len_[j];
        if (dst_cap_[j] > c.max_out) c.max_out = dst_cap_[j];
    }
    size_t n_;
    const uint32_t *src_len_, *dst_cap_;
    size_t chunk_bytes_;
    HostChunk whole_;
    size_t rem_in_ = 0, rem_out_ = 0;   // bytes of the batch not yet in a chunk
    size_t first_ = 0, cut_ = 0;
    bool ramp_ = false;
};

// A chunk's page table in a meta buffer: soff[k] u64, doff[k] u64, slen[k] u32, dcap[k] u32,
// res[k] i32.  The kernels read the first four (meta_head_bytes) and write res.
struct ChunkMeta {
    uint64_t *soff, *doff;
    uint32_t *slen, *dcap;
    int32_t *res;
};
inline size_t meta_bytes(size_t k) { return k * 28 + 64; }
inline size_t meta_head_bytes(size_t k) { return k * 24; }
// the five arrays of a k-page chunk in the meta buffer at `base` (any address space: nothing is read)
inline ChunkMeta meta_at(void *base, size_t k) {
    ChunkMeta m;
    m.soff = (uint64_t *)base;
    m.doff = m.soff + k;
    m.slen = (uint32_t *)(m.doff + k);
    m.dcap = m.slen + k;
    m.res = (int32_t *)(m.dcap + k);
    return m;
}
// fills the table of k pages with the given lengths and capacities: offsets are the running up16 sums
inline ChunkMeta meta_fill(void *base, size_t k, const uint32_t *src_len, const uint32_t *dst_cap) {
    const ChunkMeta m = meta_at(base, k);
    size_t so = 0, dof = 0;
    for (size_t j = 0; j < k; j++) {
        m.soff[j] = so;
        m.doff[j] = dof;
        m.slen[j] = src_len[j];
        m.dcap[j] = dst_cap[j];
        so += up16(src_len[j]);
        dof += up16(dst_cap[j]);
    }
    return m;
}

}  // namespace tyche
