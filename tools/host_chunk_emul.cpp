// tools/host_chunk_emul.cpp -- the host batch path's chunk plan and page-table layout
// (tyche_amd/csrc/host_chunk_core.h, run by host_batch.hip) behind a C interface.
// TEST INFRASTRUCTURE: tests/test_host_chunk_emul.py holds it to a Python restatement of the
// rule, and tests/test_host_engine.py holds the engine's chunk counter to its cuts.
//
//   g++ -O2 -shared -fPIC -o tools/bin/libhostchunkemul.so tools/host_chunk_emul.cpp
//   size_t host_chunk_cut(size_t n, const uint32_t *src_len, const uint32_t *dst_cap, long chunk_mb, int ramp_wanted,
//                         uint64_t *chunks, uint64_t *limits, uint64_t info[4]);
// cuts the batch: chunks gets {first, count, in_bytes, out_bytes, max_in, max_out} per chunk and
// limits the limit each was cut under (room for n of each); info gets {chunk_bytes, est, ramp,
// kSlots}.  Returns the number of chunks.
//   size_t host_chunk_meta(void *base, size_t k, const uint32_t *src_len, const uint32_t *dst_cap, uint64_t at[5]);
// fills a k-page table at base (meta_bytes(k) bytes, the return value) and gives the byte offsets
// of soff, doff, slen, dcap and res from base.
//
// With -DHOST_CHUNK_EMUL_MAIN it is a stand-alone program for sanitizer builds
// (g++ -O1 -g -fsanitize=address,undefined -DHOST_CHUNK_EMUL_MAIN): a seeded sweep of batches, the
// length arrays and the meta buffer in heap blocks of exactly their sizes, every cut checked to
// partition the batch within its limits and every table to hold the running sums.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../tyche_amd/csrc/host_chunk_core.h"

using namespace tyche;

extern "C" size_t host_chunk_cut(size_t n, const uint32_t *src_len, const uint32_t *dst_cap, long chunk_mb, int ramp_wanted,
                                 uint64_t *chunks, uint64_t *limits, uint64_t info[4]) {
    ChunkCutter cut(n, src_len, dst_cap, host_chunk_bytes(chunk_mb), ramp_wanted != 0);
    info[0] = host_chunk_bytes(chunk_mb);
    info[1] = cut.estimate();
    info[2] = cut.ramp();
    info[3] = kSlots;
    size_t c = 0;
    for (HostChunk ch;; c++) {
        const uint64_t limit = cut.limit_of_next();
        if (!cut.next(&ch)) break;
        limits[c] = limit;
        const uint64_t row[6] = {ch.first, ch.count, ch.in_bytes, ch.out_bytes, ch.max_in, ch.max_out};
        for (int f = 0; f < 6; f++) chunks[c * 6 + f] = row[f];
    }
    return c;
}

extern "C" size_t host_chunk_meta(void *base, size_t k, const uint32_t *src_len, const uint32_t *dst_cap, uint64_t at[5]) {
    const ChunkMeta m = meta_fill(base, k, src_len, dst_cap);
    const uint8_t *b = (const uint8_t *)base;
    at[0] = (uint64_t)((const uint8_t *)m.soff - b);
    at[1] = (uint64_t)((const uint8_t *)m.doff - b);
    at[2] = (uint64_t)((const uint8_t *)m.slen - b);
    at[3] = (uint64_t)((const uint8_t *)m.dcap - b);
    at[4] = (uint64_t)((const uint8_t *)m.res - b);
    return meta_bytes(k);
}

#ifdef HOST_CHUNK_EMUL_MAIN
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below) {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_rng >> 33) % below);
}

int main() {
    long batches = 0, bad = 0;
    for (int round = 0; round < 400; round++) {
        const size_t n = 1 + rnd(round % 8 == 0 ? 4000 : 300);
        static const uint32_t tops[5] = {64, 4096, 16384, 65536, 1u << 20};
        const uint32_t top = tops[rnd(5)];
        uint32_t *sl = (uint32_t *)malloc(n * 4), *dc = (uint32_t *)malloc(n * 4);
        for (size_t i = 0; i < n; i++) {
            sl[i] = rnd(6) == 0 ? 0 : rnd(top + 1);
            dc[i] = rnd(9) == 0 ? 0 : rnd(top + 1);
        }
        static const long mbs[5] = {0, 1, 2, 4, 32};
        const long mb = mbs[rnd(5)];
        for (int ramp = 0; ramp < 2; ramp++) {
            uint64_t *chunks = (uint64_t *)malloc(n * 48), *limits = (uint64_t *)malloc(n * 8), info[4];
            const size_t nc = host_chunk_cut(n, sl, dc, mb, ramp, chunks, limits, info);
            size_t at = 0;
            bool ok = nc >= 1 && nc <= n;
            for (size_t c = 0; ok && c < nc; c++) {
                const uint64_t *ch = chunks + c * 6;
                ok = ch[0] == at && ch[1] >= 1 && (ch[1] == 1 || (ch[2] <= limits[c] && ch[3] <= limits[c]));
                const size_t k = (size_t)ch[1];
                void *meta = malloc(meta_bytes(k));
                uint64_t where[5];
                host_chunk_meta(meta, k, sl + at, dc + at, where);
                const ChunkMeta m = meta_at(meta, k);
                size_t so = 0, dof = 0;
                for (size_t j = 0; ok && j < k; j++) {
                    ok = m.soff[j] == so && m.doff[j] == dof && m.slen[j] == sl[at + j] && m.dcap[j] == dc[at + j];
                    m.res[j] = 0;   // the kernels' array lies inside the block too
                    so += up16(sl[at + j]);
                    dof += up16(dc[at + j]);
                }
                ok = ok && so == ch[2] && dof == ch[3] && where[4] + k * 4 <= meta_bytes(k);
                free(meta);
                at += k;
            }
            ok = ok && at == n;
            if (!ok) {
                bad++;
                fprintf(stderr, "round %d ramp %d: n %zu chunk_mb %ld: bad cut\n", round, ramp, n, mb);
            }
            batches++;
            free(chunks);
            free(limits);
        }
        free(sl);
        free(dc);
    }
    printf("%ld batches cut, %ld bad\n", batches, bad);
    return bad ? 1 : 0;
}
#endif
