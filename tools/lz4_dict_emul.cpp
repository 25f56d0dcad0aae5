// tools/lz4_dict_emul.cpp -- host emulator of the shared-dictionary LZ4 kernels
// (tyche_amd/csrc/lz4_decode_dict.hip, lz4_encode_dict.hip) for one page at a
// time: the kernels' own per-wave code from lz4_dict_core.h (the decoder with its
// verdicts; the encoder's emission of parse records and the closing literal run)
// with the 64 lanes as explicit loops.  The buffers stand where the kernels keep
// them in LDS: [dictionary | output window] for the decoder, [dictionary tail |
// page | 64 zero bytes] and the handle's dictionary table for the encoder.
// TEST INFRASTRUCTURE: tests/test_lz4_dict_emul.py runs it against the reference
// on the CPU, so the logic is checked before (and apart from) the GPU tests.
//
// The encoder's parse on the GPU is lz_parse.h's wave-parallel parse_page, which
// is SIMT code; here a plain greedy parse with the same table (2^12 slots, the
// dictionary's entries first, the page's own replacing them) and the same
// end-of-block rules stands in for it and hands its records to the emission in
// batches, as parse_page does.  The streams therefore differ from the GPU's in
// which matches they hold, not in how a record becomes bytes.
//
//   g++ -O2 -shared -fPIC -o tools/bin/liblz4dictemul.so tools/lz4_dict_emul.cpp
//   int lz4_dict_emul_decompress(const uint8_t *dict, int D, const uint8_t *src, int L, uint8_t *dst, int C);
//   int lz4_dict_emul_compress(const uint8_t *dict, int D, const uint8_t *src, int L, uint8_t *dst, int cap);
//
// With -DLZ4_DICT_EMUL_MAIN it is a stand-alone program for sanitizer builds
// (g++ -O1 -g -fsanitize=address,undefined -DLZ4_DICT_EMUL_MAIN): it replays a
// file of calls recorded by the test (LZ4_DICT_EMUL_RECORD=<file> in the test's
// environment) in exactly sized heap buffers and compares the return values
// with the recorded ones.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define LZD_HOST 1
#include "../tyche_amd/csrc/lz4_dict_core.h"

extern "C" int lz4_dict_emul_decompress(const uint8_t *dict, int D, const uint8_t *src, int L, uint8_t *dst, int C) {
    if (D < 0 || L < 0 || C < 0 || (uint32_t)D > lzd::kDictMax || (uint32_t)C + (uint32_t)D > lzd::kWindowMax) return INT32_MIN;
    // exactly sized, so that a sanitizer build sees a read or write outside the window or the
    // staged stream (the kernel pads the stream with 64 zero bytes)
    std::vector<uint8_t> win((size_t)D + (size_t)C + !(D + C), 0xEE), in((size_t)L + 64, 0);
    if (D) memcpy(win.data(), dict, (size_t)D);
    if (L) memcpy(in.data(), src, (size_t)L);
    const int32_t rv = lzd::decode_page(in.data(), L, win.data() + D, C, D);
    if (rv > 0) memcpy(dst, win.data() + D, (size_t)rv);
    return rv;
}

extern "C" int lz4_dict_emul_compress(const uint8_t *dict, int D, const uint8_t *src, int L, uint8_t *dst, int cap) {
    if (D < 0 || L < 0 || cap < 0 || (uint32_t)D > lzd::kDictMax || (uint32_t)L + (uint32_t)D > lzd::kWindowMax) return INT32_MIN;
    const uint32_t DE = lzd::enc_dict_len((uint32_t)D), W = DE + (uint32_t)L;
    std::vector<uint8_t> in((size_t)W + 64, 0);
    if (DE) memcpy(in.data(), dict + (D - (int)DE), DE);
    if (L) memcpy(in.data() + DE, src, (size_t)L);
    // the handle's dictionary table (dict.hip dict_create), then the page's positions over it
    std::vector<uint16_t> table(lzd::kTableSizeD, 0);
    auto word = [&](uint32_t p) {
        uint32_t v;
        memcpy(&v, in.data() + p, 4);
        return v;
    };
    for (uint32_t j = 0; j + 5u <= DE; j++) table[lzd::hash5(in.data() + j)] = (uint16_t)j;
    uint32_t op = 0, anchor = DE;
    std::vector<lzd::Rec> rec;
    uint32_t batch_anchor = anchor;
    auto flush = [&]() -> bool {
        if (rec.empty()) return true;
        const bool ok = lzd::emit_records(rec.data(), (uint32_t)rec.size(), batch_anchor, in.data(), dst, op, (uint32_t)cap);
        rec.clear();
        return ok;
    };
    if (W >= 13u && DE + 12u <= W) {
        const uint32_t mflimit = W - 12u, matchlimit = W - 5u;
        for (uint32_t pos = DE; pos <= mflimit;) {
            const uint32_t v = word(pos), h = lzd::hash5(in.data() + pos), cand = table[h];
            table[h] = (uint16_t)pos;
            if (cand < pos && word(cand) == v) {
                uint32_t len = 4;
                while (pos + len < matchlimit && in[pos + len] == in[cand + len]) len++;
                if (pos + len > matchlimit) len = matchlimit - pos;
                if (len >= 4u) {
                    if (rec.empty()) batch_anchor = anchor;
                    rec.push_back(lzd::Rec{pos | (cand << 16), len});
                    pos += len;
                    anchor = pos;
                    // batches of varying sizes, 1..64, as the parse's hand-offs vary
                    if (rec.size() >= 1u + (pos * 7u) % 64u && !flush()) return 0;
                    continue;
                }
            }
            pos++;
        }
    }
    if (!flush()) return 0;
    if (!lzd::write_last_literals(in.data(), anchor, W, dst, op, (uint32_t)cap)) return 0;
    return (int)op;
}

#ifdef LZ4_DICT_EMUL_MAIN
// Record: u32 mode (0 decode, 1 encode), u32 dictionary length, u32 source length, u32 capacity,
// i32 return value, then the dictionary and the source bytes.
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
    uint32_t h[5];
    long calls = 0, bad = 0;
    while (fread(h, sizeof(h), 1, f) == 1) {
        const uint32_t mode = h[0], D = h[1], n = h[2], cap = h[3];
        const int32_t want = (int32_t)h[4];
        uint8_t *dict = new uint8_t[D + !D], *s = new uint8_t[n + !n], *d = new uint8_t[cap + !cap];
        if ((D && fread(dict, 1, D, f) != D) || (n && fread(s, 1, n, f) != n)) {
            fprintf(stderr, "truncated record\n");
            return 2;
        }
        const int got = mode ? lz4_dict_emul_compress(dict, (int)D, s, (int)n, d, (int)cap)
                             : lz4_dict_emul_decompress(dict, (int)D, s, (int)n, d, (int)cap);
        if (got != want) {
            bad++;
            fprintf(stderr, "call %ld: mode %u D %u n %u cap %u: got %d, recorded %d\n", calls, mode, D, n, cap, got, want);
        }
        calls++;
        delete[] dict;
        delete[] s;
        delete[] d;
    }
    fclose(f);
    printf("%ld calls replayed, %ld differ\n", calls, bad);
    return bad ? 1 : 0;
}
#endif
