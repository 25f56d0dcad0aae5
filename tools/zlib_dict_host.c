/* zlib_dict_host.c -- the reference's zlib 1.2.8 with a preset dictionary on host threads, for
 * profiles/zlib_dict_time.log: deflateSetDictionary + deflate(Z_FINISH) at level 1 and
 * inflateSetDictionary + inflate(Z_FINISH) over PAGES dist-0 bench pages of PLEN bytes (pagegen.h, seed
 * 20170303, pages 0..), the dictionary the first D bytes of page PAGES + 5 at 32 KiB -- the inputs of
 * tools/time_zlib_dict.py.  Wall clock, the median of 3 passes.  Links the library oracle/_ref holds:
 *
 *   gcc -O2 -std=gnu99 -pthread -o tools/bin/zlib_dict_host tools/zlib_dict_host.c \
 *       -Loracle/_ref -ltyche_ref -Wl,-rpath,'$ORIGIN/../../oracle/_ref'
 *   tools/bin/zlib_dict_host PAGES PLEN D THREADS
 */
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../tyche_amd/csrc/pagegen.h"

/* zlib.h's z_stream and the calls used, as zlib 1.2.8 declares them */
typedef struct {
    const unsigned char *next_in; unsigned avail_in; unsigned long total_in;
    unsigned char *next_out; unsigned avail_out; unsigned long total_out;
    const char *msg; void *state; void *zalloc, *zfree, *opaque; int data_type; unsigned long adler, reserved;
} zs_t;
int deflateInit_(zs_t *, int, const char *, int);
int deflateSetDictionary(zs_t *, const unsigned char *, unsigned);
int deflate(zs_t *, int);
int deflateEnd(zs_t *);
int inflateInit_(zs_t *, const char *, int);
int inflateSetDictionary(zs_t *, const unsigned char *, unsigned);
int inflate(zs_t *, int);
int inflateEnd(zs_t *);

static size_t g_n, g_plen, g_d, g_slot;
static int g_threads, g_decode;
static uint8_t *g_pages, *g_comp, *g_back, g_dict[32768];
static uint32_t *g_len;

static void *work(void *arg) {
    const size_t t = (size_t)arg;
    for (size_t i = t; i < g_n; i += (size_t)g_threads) {
        zs_t s;
        memset(&s, 0, sizeof(s));
        if (!g_decode) {
            if (deflateInit_(&s, 1, "1.2.8", (int)sizeof(s)) || deflateSetDictionary(&s, g_dict, (unsigned)g_d)) abort();
            s.next_in = g_pages + i * g_plen; s.avail_in = (unsigned)g_plen;
            s.next_out = g_comp + i * g_slot; s.avail_out = (unsigned)g_slot;
            if (deflate(&s, 4) != 1) abort();
            g_len[i] = (uint32_t)s.total_out;
            deflateEnd(&s);
        } else {
            if (inflateInit_(&s, "1.2.8", (int)sizeof(s))) abort();
            s.next_in = g_comp + i * g_slot; s.avail_in = g_len[i];
            s.next_out = g_back + i * g_plen; s.avail_out = (unsigned)g_plen;
            if (inflate(&s, 4) != 2 || inflateSetDictionary(&s, g_dict, (unsigned)g_d) || inflate(&s, 4) != 1) abort();
            inflateEnd(&s);
        }
    }
    return NULL;
}

static double pass(int decode) {
    pthread_t th[256];
    struct timespec a, b;
    g_decode = decode;
    clock_gettime(CLOCK_MONOTONIC, &a);
    for (int t = 0; t < g_threads; t++) pthread_create(&th[t], NULL, work, (void *)(size_t)t);
    for (int t = 0; t < g_threads; t++) pthread_join(th[t], NULL);
    clock_gettime(CLOCK_MONOTONIC, &b);
    return (b.tv_sec - a.tv_sec) * 1e3 + (b.tv_nsec - a.tv_nsec) / 1e6;
}

static double median3(int decode) {
    double v[3];
    for (int k = 0; k < 3; k++) v[k] = pass(decode);
    for (int i = 0; i < 3; i++)
        for (int j = i + 1; j < 3; j++)
            if (v[j] < v[i]) { double x = v[i]; v[i] = v[j]; v[j] = x; }
    return v[1];
}

int main(int argc, char **argv) {
    if (argc != 5) return fprintf(stderr, "usage: %s PAGES PLEN D THREADS\n", argv[0]), 2;
    g_n = (size_t)atol(argv[1]); g_plen = (size_t)atol(argv[2]); g_d = (size_t)atol(argv[3]); g_threads = atoi(argv[4]);
    if (g_d < 1 || g_d > 32768 || g_threads < 1 || g_threads > 256 || g_plen < 1 || g_plen > 65535) return 2;
    g_slot = g_plen + g_plen / 1000 + 64;
    g_pages = malloc(g_n * g_plen); g_comp = malloc(g_n * g_slot); g_back = malloc(g_n * g_plen); g_len = malloc(g_n * 4);
    if (!g_pages || !g_comp || !g_back || !g_len) return 1;
    pg_page_t p;
    for (size_t i = 0; i < g_n; i++) {
        pg_page_init(&p, 20170303ull, i, (uint32_t)g_plen, 0);
        for (size_t k = 0; k < g_plen; k++) g_pages[i * g_plen + k] = (uint8_t)pg_page_byte(&p, (uint32_t)k);
    }
    pg_page_init(&p, 20170303ull, g_n + 5, 32768, 0);
    for (size_t k = 0; k < g_d; k++) g_dict[k] = (uint8_t)pg_page_byte(&p, (uint32_t)k);
    const double enc = median3(0), dec = median3(1);
    if (memcmp(g_pages, g_back, g_n * g_plen)) return fprintf(stderr, "round trip failed\n"), 1;
    double total = 0;
    for (size_t i = 0; i < g_n; i++) total += g_len[i];
    printf("{\"what\": \"reference zlib 1.2.8 with dictionary, host\", \"pages\": %zu, \"page_len\": %zu, \"dict\": %zu, "
           "\"threads\": %d, \"deflate_ms\": %.1f, \"inflate_ms\": %.1f, \"ratio\": %.4f}\n",
           g_n, g_plen, g_d, g_threads, enc, dec, (double)g_n * g_plen / total);
    return 0;
}
