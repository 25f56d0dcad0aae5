// tools/pack_emul.cpp -- host emulator of the packed store (tyche_amd/csrc/pack.hip;
// tyche_pack_batch): pack_core.h compiled for the host.  The plan runs in the
// kernels' three steps -- a sum per kScanPages pages, the scan of those sums in
// rounds of kFanIn with a carry, the apply step -- and the decision is
// pk::decide.  The copy then runs tile by tile through pk::copy_tile, the
// kernel's own tile -> page -> piece walk, with the search's 64 probes of a round
// taken one after another and every piece split at the destination's 16-byte
// lines as on the device; the bytes of a part are moved with memcpy, at their
// exact length, so a sanitizer build sees any byte read outside a stream or
// written outside [o_i, o_i + len_i).  (The device moves whole lines through
// registers from the aligned source lines around them; what it stores is these
// bytes.)
// TEST INFRASTRUCTURE: tests/test_pack_emul.py holds it to the numpy restatement
// of the rule (tests/pack_cases.py) on the CPU, and tests/test_gpu_pack.py holds
// the kernels to its bytes.
//
//   g++ -O2 -shared -fPIC -o tools/bin/libpackemul.so tools/pack_emul.cpp
//   int pack_emul(const uint8_t *src, const uint64_t *src_offsets, uint64_t src_stride, const int32_t *results,
//                 uint32_t n, uint32_t max_length, uint8_t *arena, uint64_t capacity, uint32_t align, uint32_t skew,
//                 uint64_t state[2], uint64_t *offsets, uint32_t *lengths);
// `skew` stands for the device arena's address & 127 (the host arena may lie
// anywhere).  Returns 1 when the batch was stored, 0 when refused, -1 for
// arguments the engine refuses.  pack_emul_constants gives T, S, the fan-in and
// the probes per round.
//
// With -DPACK_EMUL_MAIN it is a stand-alone program for sanitizer builds
// (g++ -O1 -g -fsanitize=address,undefined -DPACK_EMUL_MAIN): it replays a file
// of calls recorded by the test (PACK_EMUL_RECORD=<file> in the test's
// environment), every stream in a heap block of exactly its length at source
// misalignments 0, 1 and 15 and the arena in a block of exactly its capacity,
// and compares offsets, lengths, state and every arena byte with the recorded
// ones.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define PK_HOST 1
#include "../tyche_amd/csrc/pack_core.h"

namespace {

struct HostOps {
    const uint8_t *src;
    const uint64_t *src_offsets;
    uint64_t src_stride;
    uint8_t *arena;
    uint32_t skew;
    const uint64_t *offsets;
    const uint32_t *lengths;

    uint32_t probes_true(uint32_t a, uint32_t b, uint32_t step, uint64_t lo) const {
        uint32_t c = 0;
        for (uint32_t lane = 0; lane < pk::kProbes; lane++) {
            const uint32_t at = pk::probe_at(a, step, lane);
            c += at < b && offsets[at] <= lo;
        }
        return c;
    }
    void page(uint32_t i, uint64_t *o, uint32_t *len) const {
        *o = offsets[i];
        *len = lengths[i];
    }
    void copy(uint32_t i, uint32_t skip, uint64_t dst, uint32_t n) const {
        const uint8_t *s = src + (src_offsets ? src_offsets[i] : (uint64_t)i * src_stride) + skip;
        uint8_t *d = arena + dst;
        const pk::Split sp = pk::split_piece((uint32_t)((dst + skew) & (pk::kLine - 1u)), n);
        memcpy(d, s, sp.head);
        for (uint32_t v = 0; v < sp.lines; v++) memcpy(d + sp.head + v * pk::kLine, s + sp.head + v * pk::kLine, pk::kLine);
        const uint32_t body = sp.head + sp.lines * pk::kLine;
        memcpy(d + body, s + body, sp.tail);
    }
};

}  // namespace

extern "C" void pack_emul_constants(uint32_t out[4]) {
    out[0] = pk::kTile;
    out[1] = pk::kScanPages;
    out[2] = pk::kFanIn;
    out[3] = pk::kProbes;
}

extern "C" int pack_emul(const uint8_t *src, const uint64_t *src_offsets, uint64_t src_stride, const int32_t *results,
                         uint32_t n, uint32_t max_length, uint8_t *arena, uint64_t capacity, uint32_t align, uint32_t skew,
                         uint64_t state[2], uint64_t *offsets, uint32_t *lengths) {
    if (!pk::align_ok(align, 4096u) || skew > pk::kSkewMask) return -1;
    if (n == 0) return 1;
    // sums
    const uint32_t nsums = (n + pk::kScanPages - 1u) / pk::kScanPages;
    std::vector<uint64_t> sums(nsums, 0);
    for (uint32_t i = 0; i < n; i++) sums[i / pk::kScanPages] += pk::room(results[i], max_length, align);
    // scan: rounds of kFanIn sums, a carry between the rounds
    uint64_t carry = 0;
    for (uint32_t c = 0; c < nsums; c += pk::kFanIn) {
        uint64_t run = 0;
        for (uint32_t t = 0; t < pk::kFanIn && c + t < nsums; t++) {
            const uint64_t v = sums[c + t];
            sums[c + t] = carry + run;
            run += v;
        }
        carry += run;
    }
    const pk::Plan pl = pk::decide(state[0], state[1], carry, pk::page_len(results[n - 1u], max_length), align, capacity, skew);
    // apply
    for (uint32_t blk = 0; blk < nsums; blk++) {
        uint64_t o = pl.base + sums[blk];
        for (uint32_t i = blk * pk::kScanPages; i < n && i < (blk + 1u) * pk::kScanPages; i++) {
            const uint32_t len = pk::page_len(results[i], max_length);
            offsets[i] = o;
            lengths[i] = len;
            o += pk::round_up(len, align);
        }
    }
    state[0] = pl.state0;
    state[1] = pl.end;
    // copy (a refused batch has no tiles)
    HostOps ops{src, src_offsets, src_stride, arena, skew, offsets, lengths};
    for (uint32_t k = 0; k < pl.ntiles; k++) pk::copy_tile(ops, pl, k, skew, n);
    return (int)pl.stored;
}

#ifdef PACK_EMUL_MAIN
// Record: u32 n, max_length, align, skew; u64 capacity, state in [2], state out [2]; i32 stored;
// results (i32 each); every stream's bytes (len_i each, in page order); offsets (u64 each);
// lengths (u32 each); the arena's `capacity` bytes after the call (0xA5 where nothing was stored).
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <recorded calls>\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    long calls = 0, runs = 0, bad = 0;
    uint32_t h[4];
    while (fread(h, sizeof(h), 1, f) == 1) {
        const uint32_t n = h[0], max_length = h[1], align = h[2], skew = h[3];
        uint64_t q[5];
        int32_t stored = 0;
        bool ok = rd(f, q, sizeof(q)) && rd(f, &stored, 4);
        std::vector<int32_t> results(n + !n);
        ok = ok && rd(f, results.data(), (size_t)n * 4);
        std::vector<std::vector<uint8_t>> streams(n);
        for (uint32_t i = 0; ok && i < n; i++) {
            streams[i].resize(pk::page_len(results[i], max_length));
            ok = rd(f, streams[i].data(), streams[i].size());
        }
        std::vector<uint64_t> want_off(n + !n);
        std::vector<uint32_t> want_len(n + !n);
        std::vector<uint8_t> want_arena(q[0]);
        ok = ok && rd(f, want_off.data(), (size_t)n * 8) && rd(f, want_len.data(), (size_t)n * 4) &&
             rd(f, want_arena.data(), want_arena.size());
        if (!ok) {
            fprintf(stderr, "truncated record\n");
            return 2;
        }
        for (uint32_t mis : {0u, 1u, 15u}) {
            // every stream in a block of its own that ends where the stream ends
            std::vector<uint8_t *> blocks(n);
            std::vector<uint64_t> offs(n + !n);
            const uint8_t *base = nullptr;
            for (uint32_t i = 0; i < n; i++) {
                const size_t len = streams[i].size();
                blocks[i] = (uint8_t *)malloc(len + mis + !(len + mis));
                if (len) memcpy(blocks[i] + mis, streams[i].data(), len);
                if (!base || blocks[i] + mis < base) base = blocks[i] + mis;
            }
            // (pointer differences between blocks, from the lowest: the emulator only adds them back)
            for (uint32_t i = 0; i < n; i++) offs[i] = (uint64_t)(blocks[i] + mis - base);
            uint8_t *arena = (uint8_t *)malloc(q[0] + !q[0]);
            memset(arena, 0xA5, q[0]);
            uint64_t state[2] = {q[1], q[2]};
            std::vector<uint64_t> off(n + !n);
            std::vector<uint32_t> len(n + !n);
            const int got = pack_emul(base, offs.data(), 0, results.data(), n, max_length, arena, q[0], align, skew, state,
                                      off.data(), len.data());
            if (got != stored || state[0] != q[3] || state[1] != q[4] ||
                (n && (memcmp(off.data(), want_off.data(), (size_t)n * 8) || memcmp(len.data(), want_len.data(), (size_t)n * 4))) ||
                (q[0] && memcmp(arena, want_arena.data(), q[0]))) {
                bad++;
                fprintf(stderr, "call %ld, misalignment %u: n %u align %u: differs from the record\n", calls, mis, n, align);
            }
            runs++;
            free(arena);
            for (uint32_t i = 0; i < n; i++) free(blocks[i]);
        }
        calls++;
    }
    fclose(f);
    printf("%ld calls replayed at 3 misalignments (%ld runs), %ld differ\n", calls, runs, bad);
    return bad ? 1 : 0;
}
#endif
