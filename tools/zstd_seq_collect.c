/* tools/zstd_seq_collect.c -- the sequences of one zstd frame, through the oracle's decoder
 * (oracle/zstd_oracle.c built with -DZSTD_SEQ_TRACE, whose decode_sequences reports every
 * sequence it decodes).  TEST INFRASTRUCTURE: tests/zstd_hc_cases.py builds it into
 * tools/bin/libzstdseqcollect.so, and tests/test_gpu_zstd_hc.py compares the sequences of the
 * high-compression encoder's frames with the host emulator's (tools/zstd_hc_emul.cpp).
 *
 *   gcc -O2 -shared -fPIC -DZSTD_SEQ_TRACE -Ioracle -o tools/bin/libzstdseqcollect.so \
 *       tools/zstd_seq_collect.c oracle/zstd_oracle.c
 *   int zstd_seq_collect(const uint8_t *frame, int n, uint8_t *out, int out_cap, uint32_t *seqs, int cap, int *nseq);
 *     the decoder's return value; seqs: the first cap (ll, ml, off) triples, *nseq: how many there were.
 * Not thread safe: the trace hook writes to one collector.
 */
#include <stddef.h>
#include <stdint.h>
#include "oracle.h"

static uint32_t *g_seqs;
static int g_cap, g_n;

void zstd_seq_trace(uint32_t llc, uint32_t mlc, uint32_t ofc, size_t ll, size_t ml, size_t off) {
    (void)llc; (void)mlc; (void)ofc;
    if (g_n < g_cap) {
        g_seqs[3 * g_n] = (uint32_t)ll;
        g_seqs[3 * g_n + 1] = (uint32_t)ml;
        g_seqs[3 * g_n + 2] = (uint32_t)off;
    }
    g_n++;
}

int zstd_seq_collect(const uint8_t *frame, int n, uint8_t *out, int out_cap, uint32_t *seqs, int cap, int *nseq) {
    g_seqs = seqs;
    g_cap = cap;
    g_n = 0;
    const int r = oracle_zstd_decompress(frame, n, out, out_cap);
    *nseq = g_n;
    g_seqs = 0;
    g_cap = 0;
    return r;
}
