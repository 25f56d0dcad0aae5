// tools/lz4_train_emul.cpp -- host emulator of the shared-dictionary trainer
// (tyche_amd/csrc/lz4_dict_train.hip): the kernels' own per-page and per-segment
// code from lz4_train_core.h, one "thread" walking every strided loop, driven
// by the loops the launches stand for -- the count pass over all pages, then per
// round the score pass over the pages that can still win and the apply step.
// Every page is read in place, at its exact length, so a sanitizer build sees a
// read outside it.
// TEST INFRASTRUCTURE: tests/test_lz4_train_emul.py runs it against the numpy
// restatement of the algorithm (tests/lz4_train_cases.py) on the CPU, and
// tests/test_gpu_lz4_train.py holds the GPU to its bytes.
//
//   g++ -O2 -shared -fPIC -o tools/bin/liblz4trainemul.so tools/lz4_train_emul.cpp
//   int lz4_train_emul(const uint8_t *src, const uint64_t *offsets, const uint32_t *lengths, uint32_t n,
//                      uint32_t dict_len, uint8_t *out);
// returns the dictionary's length (a multiple of 128, at most dict_len; 0: the pages share
// nothing) with its bytes in out[0 .. length), or -1 for arguments the engine refuses.
//
// With -DLZ4_TRAIN_EMUL_MAIN it is a stand-alone program for sanitizer builds
// (g++ -O1 -g -fsanitize=address,undefined -DLZ4_TRAIN_EMUL_MAIN): it replays a
// file of calls recorded by the test (LZ4_TRAIN_EMUL_RECORD=<file> in the test's
// environment), every page in a heap block of exactly its length at each source
// misalignment 0..15, and compares the dictionaries with the recorded ones.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define LZT_HOST 1
#include "../tyche_amd/csrc/lz4_train_core.h"

extern "C" int lz4_train_emul(const uint8_t *src, const uint64_t *offsets, const uint32_t *lengths, uint32_t n,
                              uint32_t dict_len, uint8_t *out) {
    if (n == 0 || n > lzt::kMaxPages || dict_len < lzt::kSeg || dict_len > 32768u) return -1;
    uint32_t longest = 0;
    for (uint32_t i = 0; i < n; i++) longest = lengths[i] > longest ? lengths[i] : longest;
    if (longest > lzt::kMaxPage) return -1;
    std::vector<uint32_t> table(lzt::kTableSize, 0), bitmap(lzt::kBitmapWords, 0), ub(n, 0xFFFFFFFFu);
    std::vector<lzt::Blk> blk(lzt::key_blocks(longest) + 1u);
    for (uint32_t i = 0; i < n; i++) lzt::count_page(src + offsets[i], lengths[i], bitmap.data(), table.data(), 0, 1);
    const uint32_t rounds = dict_len / lzt::kSeg;
    std::vector<uint8_t> picks((size_t)rounds * lzt::kSeg);
    uint32_t npicks = 0;
    for (uint32_t r = 0; r < rounds; r++) {
        unsigned long long best = 0;
        for (uint32_t i = 0; i < n; i++) {
            if (lengths[i] < lzt::kSeg || lzt::cannot_win(ub[i], i, best)) continue;
            unsigned long long mine = 0;
            lzt::score_page(src + offsets[i], lengths[i], table.data(), blk.data(), i, &mine, 0, 1);
            ub[i] = (uint32_t)(mine >> 32);
            lzt_max64(&best, mine);
        }
        if (best == 0) break;
        const uint8_t *seg = src + offsets[lzt::best_page(best)] + lzt::best_start(best);
        lzt::apply_segment(seg, table.data(), picks.data() + (size_t)npicks * lzt::kSeg, 0, 1);
        npicks++;
    }
    // the first pick ends the dictionary
    for (uint32_t k = 0; k < npicks; k++)
        memcpy(out + (size_t)k * lzt::kSeg, picks.data() + (size_t)(npicks - 1u - k) * lzt::kSeg, lzt::kSeg);
    return (int)(npicks * lzt::kSeg);
}

#ifdef LZ4_TRAIN_EMUL_MAIN
// Record: u32 page count, u32 requested dictionary length, i32 returned length, the page lengths
// (u32 each), the pages' bytes one after another, then the returned dictionary.
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
    uint32_t h[3];
    long calls = 0, runs = 0, bad = 0;
    while (fread(h, sizeof(h), 1, f) == 1) {
        const uint32_t n = h[0], D = h[1];
        const int32_t want = (int32_t)h[2];
        std::vector<uint32_t> lens(n + !n);
        if (n && fread(lens.data(), 4, n, f) != n) {
            fprintf(stderr, "truncated record\n");
            return 2;
        }
        std::vector<std::vector<uint8_t>> pages(n);
        for (uint32_t i = 0; i < n; i++) {
            pages[i].resize(lens[i]);
            if (lens[i] && fread(pages[i].data(), 1, lens[i], f) != lens[i]) {
                fprintf(stderr, "truncated record\n");
                return 2;
            }
        }
        std::vector<uint8_t> dict(want > 0 ? want : 0);
        if (want > 0 && fread(dict.data(), 1, (size_t)want, f) != (size_t)want) {
            fprintf(stderr, "truncated record\n");
            return 2;
        }
        for (uint32_t mis = 0; mis < 16u; mis++) {
            // every page in a block of its own: exactly its bytes, `mis` bytes into the allocation's alignment
            std::vector<uint8_t *> blocks(n);
            std::vector<uint64_t> offs(n + !n);
            const uint8_t *base = nullptr;
            for (uint32_t i = 0; i < n; i++) {
                // the page ends where the block ends, so a read past it leaves the allocation (and at
                // mis = 0 so does a read in front of it)
                blocks[i] = (uint8_t *)malloc((size_t)lens[i] + mis + !(lens[i] + mis));
                uint8_t *p = blocks[i] + mis;
                if (lens[i]) memcpy(p, pages[i].data(), lens[i]);
                if (i == 0) base = p;
                offs[i] = (uint64_t)(p - base);   // (pointer differences between blocks: the emulator only adds them back)
            }
            uint8_t *out = new uint8_t[D + !D];
            const int got = lz4_train_emul(base, offs.data(), lens.data(), n, D, out);
            if (got != want || (got > 0 && memcmp(out, dict.data(), (size_t)got) != 0)) {
                bad++;
                fprintf(stderr, "call %ld, misalignment %u: n %u D %u: got %d, recorded %d (or other bytes)\n", calls, mis, n,
                        D, got, want);
            }
            runs++;
            delete[] out;
            for (uint32_t i = 0; i < n; i++) free(blocks[i]);
        }
        calls++;
    }
    fclose(f);
    printf("%ld calls replayed at 16 misalignments (%ld runs), %ld differ\n", calls, runs, bad);
    return bad ? 1 : 0;
}
#endif
