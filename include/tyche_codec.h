/*
 * include/tyche_codec.h -- C ABI of the MI355X page-codec engine (libtyche_codec.so).
 *
 * Drop-in replacement for tyche's codec boundary (reference src/buffer.h:67-68,
 * src/buffer.c:159-281): the same `Buffer` struct, the same buffer__* symbols
 * and signatures, the same compressor IDs (src/globals.h:16-19) and error codes
 * (src/globals.h:35-58), and the same ownership rules (compress returns a
 * free()-able *compressed_data; decompress swaps buf->data in place).  The
 * codec work runs as HIP kernels on gfx950; nothing here falls back to a CPU
 * codec.  Additional entry points expose the batch engine that the sweep
 * (list.c:824-838, 1039-1063) and restore (list.c:563-589) paths call with many
 * pages at once, and the device-resident batch API measured by bench.py.
 *
 * Plain C types only; no torch, no HIP types (streams are passed as void*).
 */
#ifndef TYCHE_CODEC_H_
#define TYCHE_CODEC_H_

#include <pthread.h>
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- compressor IDs: src/globals.h:16-19 -------------------------------- */
#define TYCHE_NO_COMPRESSOR_ID   0
#define TYCHE_LZ4_COMPRESSOR_ID  1
#define TYCHE_ZLIB_COMPRESSOR_ID 2
#define TYCHE_ZSTD_COMPRESSOR_ID 3

/* ---- error codes: src/globals.h:35-58 ----------------------------------- */
#define TYCHE_E_OK                          0
#define TYCHE_E_GENERIC                     1
#define TYCHE_E_BUFFER_NOT_FOUND          120
#define TYCHE_E_BUFFER_MISSING_DATA       123
#define TYCHE_E_BUFFER_ALREADY_COMPRESSED 124
#define TYCHE_E_BUFFER_ALREADY_DECOMPRESSED 125
#define TYCHE_E_BUFFER_COMPRESSION_PROBLEM 126
#define TYCHE_E_NO_MEMORY                 150
#define TYCHE_E_BAD_ARGS                  190
/* engine-specific (outside the reference's range): the HIP engine itself failed
 * (no device, launch failure, codec not built for the device) */
#define TYCHE_E_DEVICE                    199

/* ---- Buffer: identical layout to src/buffer.h:23-58 --------------------- */
typedef enum buffer_flags {
    dirty = 1 << 0,
    pending_sweep = 1 << 1,
    updating = 1 << 2,
    removing = 1 << 3,
    removed = 1 << 4,
    compressing = 1 << 5,
    compressed = 1 << 6,
} buffer_flags;

typedef uint32_t bufferid_t;
typedef uint8_t popularity_t;
typedef struct buffer Buffer;
struct buffer {
    Buffer *next;
    bufferid_t id;
    uint16_t ref_count;
    buffer_flags flags;
    popularity_t popularity;
    pthread_mutex_t lock;
    uint32_t comp_cost;     /* ns spent in compress+decompress (wraps like the reference's uint32) */
    uint16_t comp_hits;     /* restores */
    uint32_t data_length;   /* uncompressed page length */
    uint32_t comp_length;   /* bytes in data when compressed, else 0 */
    void *data;             /* free()-compatible host heap */
};

/* ---- drop-in symbols: src/buffer.h:62-69 --------------------------------- */
int buffer__initialize(Buffer **buf, bufferid_t id, uint32_t size, void *data, char *page_filespec);
void buffer__destroy(Buffer *buf, const bool destroy_data);
void buffer__lock(Buffer *buf);
void buffer__unlock(Buffer *buf);
void buffer__release_pin(Buffer *buf);
/* replaces src/buffer.c:159-219: LZ4/zlib/zstd by compressor_id, on the GPU.
 * On a codec or device failure (126 / TYCHE_E_DEVICE) *compressed_data is set
 * to NULL (the reference leaves it at a leaked, unfilled block). */
int buffer__compress(Buffer *buf, void **compressed_data, int compressor_id, int compressor_level);
/* replaces src/buffer.c:227-281 */
int buffer__decompress(Buffer *buf, int compressor_id);
void buffer__copy(Buffer *src, Buffer *dst, bool copy_data);

/* ---- batch extension over Buffers (sweep / restore callers) -------------- */
/* Compress n buffers in one GPU batch.  Per buffer, status[i] and side effects
 * are exactly what buffer__compress would produce for it (compressed[i] is a
 * malloc'd block the caller owns when status[i]==0).  Returns 0, or
 * TYCHE_E_DEVICE / TYCHE_E_NO_MEMORY if the batch could not run at all.
 * Replaces the per-victim loop of list__compressor_start (src/list.c:1039-1063). */
int tyche_buffers_compress(Buffer **bufs, void **compressed, int *status, size_t n, int compressor_id,
                           int compressor_level);
/* Restore n compressed buffers in one GPU batch (the list__search restore of
 * src/list.c:563-589, coalesced); status[i] as buffer__decompress. */
int tyche_buffers_decompress(Buffer **bufs, int *status, size_t n, int compressor_id);

/* ---- restore queue: coalesced per-hit restores (src/list.c:563-589) ------- */
/* Starts the dispatcher threads (per codec, TYCHE_RESTORE_DISPATCHERS each,
 * default one per active device; they inherit the calling thread's device
 * choice) that batch concurrent tyche_buffer_restore calls: once a request
 * arrives a dispatcher of its codec waits up to max_wait_us for up to max_batch
 * requests of that codec, then runs one GPU decompress batch while the next
 * dispatcher collects.  Idempotent. */
int tyche_restore_queue_start(int max_batch, int max_wait_us);
/* Drains and stops the dispatcher. */
void tyche_restore_queue_stop(void);
/* Drop-in for buffer__decompress at the list__search restore site
 * (src/list.c:572): same status and side effects, but concurrent callers share
 * GPU launches.  Without a running queue it is buffer__decompress. */
int tyche_buffer_restore(Buffer *buf, int compressor_id);
/* Launches and buffers served so far. */
void tyche_restore_queue_stats(uint64_t *batches, uint64_t *buffers);
/* Launches so far by batch size: counts[k] = launches of 2^k .. 2^(k+1)-1
 * buffers (the last bucket takes every larger one); fills min(n, 11) buckets
 * and returns that count. */
int tyche_restore_queue_hist(uint64_t *counts, int n);

/* ---- device-resident batch API ------------------------------------------- */
/* Page i of the batch reads src + src_offsets[i] (or i*src_stride when
 * src_offsets is NULL) for src_lengths[i] (or src_length) bytes and writes at
 * most dst_capacities[i] (or dst_capacity) bytes to dst + dst_offsets[i] (or
 * i*dst_stride).  All pointers are device pointers on the current device.
 * results[i] (device int32):
 *   compress   -- compressed size, or 0 when the output does not fit
 *                 (LZ4_compress_default semantics, lz4.c:697, for every codec)
 *   decompress -- the codec's own verdict:
 *                 LZ4  LZ4_decompress_safe (lz4.c:1251): decoded size, or
 *                      -(input bytes consumed)-1 for a malformed stream;
 *                 zlib uncompress (uncompr.c:22): decoded length, or -3
 *                      (Z_DATA_ERROR) / -5 (Z_BUF_ERROR);
 *                 zstd ZSTD_decompress (zstd_decompress.c:1459): decoded size,
 *                      or a negative value wherever ZSTD_isError holds.
 *   INT32_MIN marks a page larger than the launch's declared maximum.
 * max_src_length (0 = unknown) bounds src lengths for LDS sizing.
 *
 * Page sizes.  LZ4 takes pages, and decodes into capacities, of up to
 * TYCHE_LZ4_MAX_PAGE bytes (streams up to tyche_compress_bound of that) at
 * every entry point, host and device, for any batch size: a compress batch
 * declares its maximum (src_length, or max_src_length beside src_lengths; 0
 * there keeps meaning "at most 65535"), and a declared maximum or a host page
 * above the limit is TYCHE_E_BAD_ARGS with the limit in tyche_last_error(); a
 * decode capacity above it is refused at the launch (TYCHE_E_DEVICE), as every
 * capacity beyond the decoders' reach always was.  tyche_decompress_host also
 * refuses (TYCHE_E_DEVICE, at the chunk that holds the first large page, the
 * rule in tyche_last_error()) a bulk batch that mixes the classes: one holding
 * a capacity above 65536 bytes beside more than 64 pages of at most that.  The
 * rule looks at the batch alone.  Such batches were always refused this way,
 * and a staging chunk is launched whole, so the small pages would share the
 * one-page-per-CU decoders of the large ones.  Pass large pages in calls of
 * their own; the Buffer entry points and the restore queue do so themselves.
 * A page above 65535 bytes still becomes one standard LZ4 block; in a batch that
 * mixes sizes, the pages of up to 65535 bytes get the bytes they would get
 * without the larger ones.  zlib and zstd compress pages of up to 65535 bytes
 * only (TYCHE_E_BAD_ARGS above), and so does LZ4 under LZ4_EXACT=1 (below).
 * `stream` is a hipStream_t (NULL = default stream); the call is asynchronous. */
#define TYCHE_LZ4_MAX_PAGE (4u << 20)   /* largest LZ4 page length and decode capacity */

/* Batch contract.  For every page of a device or host batch, on every kernel
 * path and in both directions: nothing outside [dst, dst + capacity) is
 * written; the bytes in [result, capacity) are unspecified afterwards (a codec
 * may use them as scratch); src is never written; no result and no output byte
 * depends on a byte outside [src, src + length), although whole 16-byte lines
 * around it may be read; and src and dst of every page may have any byte
 * alignment.  A page above the launch's declared maximum (INT32_MIN) leaves its
 * destination untouched.  For decompress that maximum is dst_capacity; a
 * stream longer than the declared max_src_length also gives INT32_MIN from LZ4
 * and zstd, while zlib inflate does not use the declared stream maximum and
 * returns its verdict.  Held by tests/test_gpu_batch_contract.py on the checked
 * layout of tests/batch_layout.py (guard bytes around every slot, chosen bytes
 * around every source, every alignment), which the decode helpers of
 * tests/test_gpu_lz4.py, test_gpu_zstd.py and test_gpu_zlib.py share. */
typedef struct tyche_batch {
    size_t count;
    const void *src;
    const uint64_t *src_offsets;
    const uint32_t *src_lengths;
    uint64_t src_stride;
    uint32_t src_length;
    uint32_t max_src_length;
    void *dst;
    const uint64_t *dst_offsets;
    const uint32_t *dst_capacities;
    uint64_t dst_stride;
    uint32_t dst_capacity;
    int32_t *results;
} tyche_batch_t;

int tyche_compress_batch(int compressor_id, int compressor_level, const tyche_batch_t *batch, void *stream);
int tyche_decompress_batch(int compressor_id, const tyche_batch_t *batch, void *stream);
/* worst-case compressed size for n input bytes: LZ4_compressBound (lz4.h:148),
 * compressBound (zlib compress.c:74-78) or ZSTD_compressBound (zstd_compress.c:37) */
uint32_t tyche_compress_bound(int compressor_id, uint32_t n);

/* ---- packed store: compressed pages at their compressed size --------------- */
/* tyche_compress_batch leaves page i's stream in a slot of tyche_compress_bound
 * bytes.  tyche_pack_batch appends the streams of one such batch to an arena, one
 * after another, and returns where each went; every decoder reads them there
 * through src_offsets / src_lengths (tyche_batch_t), at any alignment.
 *
 * The rule (pack_core.h; tyche_pack_plan is the same code on host arrays):
 *   len_i = results[i] if 0 < results[i] and (max_length == 0 or results[i] <=
 *           max_length), else 0 -- 0, INT32_MIN and every negative result mean
 *           "no stream", and so does a result above a declared max_length;
 *   o_0 = round_up(state[1], align), o_{i+1} = round_up(o_i + len_i, align): a
 *           zero-length page takes no room;
 *   offsets[i] = o_i and lengths[i] = len_i are always written;
 *   end = o_{n-1} + len_{n-1}, not rounded; for count == 0, end = state[1] and
 *           nothing is read or written;
 *   the batch is stored iff no earlier append into this state was refused
 *           (state[0] == state[1] on entry) and end <= arena_capacity;
 *   stored:  every stream is copied to arena + o_i, state[0] = state[1] = end;
 *   refused: no arena byte is written, state[0] stays, state[1] = end.
 * Refusal is sticky: after one refused append every later one is refused too, so
 * an arena never has holes, and state[1] says how large an arena would have held
 * everything.  The invariant a caller relies on: page i is in the arena iff
 * offsets[i] + lengths[i] <= state[0] after the call.  A fresh store has state
 * {0, 0}.  The decision is made on the device: appends chain on a stream with no
 * host round trip, and the call never synchronises.
 *
 * Contract, beside the batch contract above: nothing outside [arena + o_i, arena
 * + o_i + len_i) is written -- not the alignment gaps, not the bytes before o_0,
 * not the bytes at or past end; src is never written; no arena byte depends on a
 * source byte outside [src_i, src_i + len_i) (the slots' tails hold codec
 * scratch), although whole 16-byte lines around a stream may be read; src_i,
 * arena and state[1] may have any byte alignment; arena must not overlap src.
 * Page i's stream is at src + src_offsets[i], or src + i * src_stride when
 * src_offsets is NULL.
 *
 * Refused with TYCHE_E_BAD_ARGS, the rule and the number in tyche_last_error(),
 * before any device call: align zero, not a power of two or above
 * TYCHE_PACK_MAX_ALIGN; count > 0 with src, results, arena, state, offsets or
 * lengths NULL; count above TYCHE_PACK_MAX_PAGES (2^28: page indices are 32-bit
 * in the kernels, the five 64-probe rounds of the copy's search reach 2^30, and
 * the one-workgroup scan of the tile sums takes count / 2^18 rounds).  No device
 * or a failed launch is TYCHE_E_DEVICE.  tyche_pack_plan returns end, or
 * UINT64_MAX for the same bad arguments (offsets and lengths may be NULL there).
 *
 * Compaction after evictions is the same call: src = the old arena, src_offsets
 * = the surviving pages' offsets, results = their lengths (the same 32-bit
 * values), arena = a second arena, a fresh state. */
#define TYCHE_PACK_MAX_ALIGN 4096u
#define TYCHE_PACK_MAX_PAGES (1u << 28)
typedef struct tyche_pack {
    size_t count;
    /* where the streams are: the dst side of the compress batch that wrote them */
    const void *src;
    const uint64_t *src_offsets;
    uint64_t src_stride;
    const int32_t *results;   /* device: compress results; <= 0 (0, INT32_MIN, any negative) = no stream */
    uint32_t max_length;      /* 0 = none; a result above it counts as no stream */
    void *arena;
    uint64_t arena_capacity;
    uint32_t align;           /* power of two, 1..TYCHE_PACK_MAX_ALIGN */
    uint64_t *state;          /* device, 2 words: state[0] = used, state[1] = wanted */
    uint64_t *offsets;        /* device, count entries, out */
    uint32_t *lengths;        /* device, count entries, out */
} tyche_pack_t;
/* asynchronous on `stream` (a hipStream_t, NULL = default stream), no host sync */
int tyche_pack_batch(const tyche_pack_t *p, void *stream);
/* the same rule on host arrays, no GPU: for tests and for callers that size an arena */
uint64_t tyche_pack_plan(size_t n, const int32_t *results, uint32_t max_length, uint32_t align, uint64_t capacity,
                         uint64_t state[2], uint64_t *offsets, uint32_t *lengths);

/* ---- LZ4 with a shared dictionary ----------------------------------------- */
/* The engine compresses every page on its own; a dictionary is a common prefix
 * that a page's matches may reach into (LZ4_loadDict + LZ4_compress_fast_continue
 * / LZ4_decompress_safe_usingDict, lz4.c:936, 987, 1382).
 *
 * The window.  A dictionary of D bytes followed by a page of L bytes is one LZ4
 * window.  The compressed page is a standard LZ4 block whose offsets may reach
 * back as far as the first dictionary byte (offset <= position + D): exactly what
 * LZ4_decompress_safe_usingDict(stream, dst, n, L, dict, D) restores.  The
 * end-of-block rules are unchanged.  Compress results are the size, or 0 when the
 * stream does not fit the capacity; decompress results are
 * LZ4_decompress_safe_usingDict's value (the decoded size, or -(input bytes
 * consumed)-1 at the same point of a malformed stream; an offset of exactly
 * position + D is legal, one more is the error; offset 0 is treated as the plain
 * decoders treat it: the size is defined, the copied bytes are not).  INT32_MIN
 * marks a page above the launch's declared maximum, as in tyche_*_batch.  The
 * encoder matches against the dictionary's last D & ~63 bytes; the decoder honours
 * all D.  tyche_compress_bound is unchanged.
 *
 * Reach.  The dictionary applies to a page when L + D <= 65536 (window positions
 * fit 16 bits).  Device-resident calls: a compress launch whose declared maximum
 * (src_length, or max_src_length beside src_lengths; 0 there still means 65535)
 * plus D exceeds 65536, and a decompress launch whose dst_capacity plus D does, is
 * TYCHE_E_BAD_ARGS with the rule and both numbers in tyche_last_error().  Host
 * entry points with a process-wide dictionary (tyche_lz4_use_dict, or
 * TYCHE_LZ4_DICT below) apply the rule per page -- compress to src_lengths[i],
 * decompress to dst_capacities[i]; for Buffers both are data_length, so the two
 * directions always agree.  A page outside the reach takes the path, and gets the
 * bytes, it has without a dictionary (pages above 65535 bytes included); a batch
 * that mixes the classes runs as two launches over the same batch.  One
 * consequence: a raw tyche_decompress_host caller must pass the page length as the
 * capacity, as Buffers do, or a dictionary stream may land on a plain decoder and
 * get its error verdict -- a failed restore, never wrong bytes.  Pages written
 * with a dictionary need the same dictionary to be restored.
 *
 * Without a dictionary (tyche_lz4_use_dict never called or given NULL, no
 * TYCHE_LZ4_DICT, and the plain tyche_*_batch calls) nothing changes: the kernels
 * launched, the bytes and the results are the same.  LZ4_EXACT=1 and a dictionary
 * do not combine: a compress call that has both is TYCHE_E_BAD_ARGS.  zstd and
 * zlib each have calls and a process-wide slot of their own for the same handle
 * ("zstd with a shared dictionary", "zlib with a shared dictionary" below), which
 * nothing here touches.
 *
 * TYCHE_LZ4_DICT=<file> in the environment: the file's bytes become the
 * process-wide dictionary at the first LZ4 host-path call.  A file that is
 * unreadable, empty or longer than TYCHE_LZ4_DICT_MAX makes every LZ4 host call
 * fail with TYCHE_E_BAD_ARGS and the reason; it is never silently ignored.  A
 * tyche_lz4_use_dict call replaces whatever the variable named.
 *
 * Lifetime and threads.  A handle is immutable after creation; the engine uploads
 * it once per device, lazily and under a lock.  tyche_lz4_dict_destroy drops the
 * caller's reference; a handle installed process-wide, or used by a launch still
 * in flight, lives until that use ends. */
#define TYCHE_LZ4_DICT_MAX 32768u
typedef struct tyche_lz4_dict tyche_lz4_dict_t;
/* host bytes, copied; 1..TYCHE_LZ4_DICT_MAX bytes, else NULL with the rule in tyche_last_error() */
tyche_lz4_dict_t *tyche_lz4_dict_create(const void *bytes, uint32_t len);
void tyche_lz4_dict_destroy(tyche_lz4_dict_t *d);
uint32_t tyche_lz4_dict_length(const tyche_lz4_dict_t *d);
/* device-resident batches, same tyche_batch_t and result rules as tyche_*_batch */
int tyche_lz4_compress_batch_dict(const tyche_lz4_dict_t *d, const tyche_batch_t *batch, void *stream);
int tyche_lz4_decompress_batch_dict(const tyche_lz4_dict_t *d, const tyche_batch_t *batch, void *stream);
/* process-wide dictionary of the host entry points (Buffer API, tyche_buffers_*, host batches,
 * restore queue, multi-device fan-out); NULL removes it.  Holds a reference of its own. */
int tyche_lz4_use_dict(const tyche_lz4_dict_t *d);
/* copies min(cap, length) dictionary bytes out; returns the length */
uint32_t tyche_lz4_dict_bytes(const tyche_lz4_dict_t *d, void *out, uint32_t cap);
/* a new reference to the process-wide dictionary (tyche_lz4_dict_destroy drops it), or NULL */
tyche_lz4_dict_t *tyche_lz4_current_dict(void);

/* ---- zstd with a shared dictionary ---------------------------------------- */
/* The handle is the LZ4 one: a dictionary's bytes are raw content for both codecs, so a handle
 * made by tyche_lz4_dict_create or by the trainer serves zstd as it is (tyche_dict_t is the
 * codec-neutral name of the type).  What the reference does with such bytes is the contract
 * (ZSTD_compress_usingDict / ZSTD_decompress_usingDict of its zstd 1.1.2, raw-content mode):
 *
 * The window.  A dictionary of D bytes followed by a page of L bytes is one window.  The compressed
 * page is an ordinary zstd frame -- single segment, content size, no dictionary ID, no checksum: the
 * header the engine always writes, and nothing in it says that a dictionary is needed -- whose
 * offsets may reach back as far as the first dictionary byte (offset <= position + D; one more is
 * the error it is to the reference, zstd_decompress.c:831).  The repeat offsets start at {1, 4, 8} as
 * always.  Compress results are the plain encoder's: the size, or 0 when the frame does not fit the
 * capacity; nothing is written at or past the capacity; src_len == 0 as without a dictionary;
 * INT32_MIN above the launch's declared maximum; never longer than tyche_compress_bound; the bytes
 * depend on the page and the dictionary alone (not on the batch, its size or its layout).
 * Decompress results are ZSTD_decompress_usingDict's: the decoded size, or a negative value wherever
 * ZSTD_isError holds; INT32_MIN above the launch's maximum (dst_capacity, or a stream longer than the
 * declared max_src_length).  The encoder matches against the dictionary's last D & ~63 bytes (a
 * dictionary below 64 bytes gives the bytes of a plain frame from the same parse); the decoder
 * honours all D.  A frame written with a dictionary needs it to be restored: the plain decoders and
 * ZSTD_decompress return an error for it as soon as a match reaches the dictionary.  There is no
 * checksum, so a wrong dictionary of any length gives the right size and wrong bytes (or an error),
 * exactly as LZ4's does -- keep the dictionary with the pages it wrote.
 *
 * Reach.  As for LZ4: the dictionary applies to a page when L + D <= 65536.  Device-resident calls:
 * a compress launch whose declared maximum (src_length, or max_src_length beside src_lengths; 0
 * there still means 65535) plus D exceeds 65536, and a decompress launch whose dst_capacity plus D
 * does, is TYCHE_E_BAD_ARGS before any device call, with the rule and both numbers in
 * tyche_last_error().  Host entry points (Buffer API, tyche_buffers_*, host batches, restore queue,
 * multi-device fan-out) with a process-wide zstd dictionary (tyche_zstd_use_dict, or TYCHE_ZSTD_DICT
 * below) apply the rule per page -- compress to src_lengths[i], decompress to dst_capacities[i]; a
 * page outside the reach takes the path, and gets the bytes, it has without a dictionary; a batch
 * that mixes the classes runs as two launches over the same batch.  As for LZ4, a raw
 * tyche_decompress_host caller must pass the page length as the capacity, as Buffers do, or a
 * dictionary frame may land on the plain decoder and get its error verdict -- a failed restore, never
 * wrong bytes.
 *
 * Structured dictionaries.  Bytes that begin with 37 A4 30 EC (ZSTD_DICT_MAGIC) are a structured
 * (entropy-table) dictionary to the reference, which this engine does not implement: a handle of at
 * least 4 bytes that begins so is TYCHE_E_BAD_ARGS from every call below, with "structured
 * dictionaries are not supported" in tyche_last_error().  The LZ4 calls keep accepting such a handle.
 *
 * One kernel decodes every batch size (one wave per page, the dictionary in LDS in front of the
 * window); the split multi-pass decoder of large plain batches has no dictionary variant, and the
 * encoder always runs its four passes (DESIGN.md 3.4a has what large batches pay for that).
 *
 * The process-wide zstd dictionary is a slot of its own: tyche_lz4_use_dict and the TYCHE_LZ4_DICT*
 * variables do not touch it, and it does not touch LZ4.  Without one (tyche_zstd_use_dict never
 * called or given NULL, no TYCHE_ZSTD_DICT, and the plain tyche_*_batch calls) nothing changes: the
 * kernels launched, the bytes and the results are the same.  compressor_level stays ignored.
 *
 * TYCHE_ZSTD_DICT=<file> in the environment: the file's bytes become the process-wide zstd
 * dictionary at the first zstd host-path call.  A file that is unreadable, empty, longer than
 * TYCHE_LZ4_DICT_MAX or structured makes every zstd host call fail with TYCHE_E_BAD_ARGS and the
 * reason; it is never silently ignored.  A tyche_zstd_use_dict call replaces whatever it named. */
typedef tyche_lz4_dict_t tyche_dict_t;   /* the same handle, for both codecs */
/* device-resident batches, same tyche_batch_t and result rules as tyche_*_batch */
int tyche_zstd_compress_batch_dict(const tyche_dict_t *d, const tyche_batch_t *batch, void *stream);
int tyche_zstd_decompress_batch_dict(const tyche_dict_t *d, const tyche_batch_t *batch, void *stream);
/* process-wide zstd dictionary of the host entry points; NULL removes it.  Holds a reference of its own. */
int tyche_zstd_use_dict(const tyche_dict_t *d);
/* a new reference to the process-wide zstd dictionary (tyche_lz4_dict_destroy drops it), or NULL */
tyche_dict_t *tyche_zstd_current_dict(void);

/* ---- zlib with a shared dictionary ---------------------------------------- */
/* The same handle again, as a zlib preset dictionary: what the reference's zlib 1.2.8 does with the
 * bytes is the contract (deflateSetDictionary / inflateSetDictionary).  The reach rule, the lifetime
 * rules and the per-page behaviour of the host entry points are those of the zstd section above, with
 * tyche_zlib_use_dict, TYCHE_ZLIB_DICT and "zlib" in the reach text; what differs:
 *
 * Every handle is accepted: raw bytes are raw bytes to zlib, also those that begin with zstd's magic.
 *
 * The stream.  Header 78 3F, then DICTID, the adler32 of all D dictionary bytes, big-endian (what
 * deflate.c writes at level 1 once a dictionary is set); then the default encoder's one final block,
 * dynamic or fixed, whichever is smaller; then the adler32 of the page alone.  A distance may be at
 * most min(32768, position + D).  The encoder matches against the dictionary's last D & ~63 bytes; the
 * decoder honours all D.  Every coded stream carries FDICT and DICTID, also when no match reaches the
 * dictionary.  The stored form is the one exception: with a DICTID it would be L + 15 bytes, above
 * tyche_compress_bound for pages below 8192 bytes (zlib itself overruns compressBound there), so a page
 * whose coded stream -- its 4 DICTID bytes counted -- would not be smaller than the stored form gets
 * the plain encoder's stored stream, 78 01 and stored blocks, byte for byte: no DICTID, no dictionary
 * match, restored by every zlib decoder with or without a dictionary.  So a stream is never longer
 * than tyche_compress_bound and a capacity of exactly the bound never gives 0.  An empty page is not
 * stored: it gets the default's empty block behind the dictionary header (12 bytes).  Compress results
 * are the default zlib encoder's: the size, or 0 when the stream does not fit the capacity; nothing
 * outside the slot is written; INT32_MIN above the launch's declared maximum, the slot left alone;
 * the bytes depend on the page and the dictionary alone.
 *
 * Decode verdicts are uncompress's with the dictionary offered when inflate asks for it: inflateInit,
 * inflate(Z_FINISH); on Z_NEED_DICT inflateSetDictionary (a failure is Z_DATA_ERROR) and
 * inflate(Z_FINISH) again; then uncompr.c's mapping -- the decoded length, -3 or -5.  So a plain
 * stream (no FDICT) decodes as ever and may not reach the dictionary (inflate never asked for it);
 * any valid FLG with FDICT and the right DICTID decodes; a DICTID that is not this dictionary's
 * adler32, or a stream that ends inside it, is -3; a distance of position + D is legal and one more
 * is -3.  A wrong dictionary is therefore an error, never wrong bytes -- which neither LZ4 nor zstd
 * can say.  The plain decoders keep giving -3 for an FDICT stream.  INT32_MIN only above the
 * launch's dst_capacity (no stream maximum is used, as for plain zlib inflate).
 *
 * ZLIB_HC=1 loses where a dictionary reaches: tyche_zlib_compress_batch_dict ignores the knob, and
 * with a process-wide dictionary the pages in reach take the dictionary encoder, the others HC.
 * One serial one-wave kernel decodes every batch size.  The slot is zlib's own: the
 * LZ4 and zstd calls and variables do not touch it, nor it theirs; without a zlib dictionary nothing
 * changes.
 *
 * TYCHE_ZLIB_DICT=<file>: as TYCHE_ZSTD_DICT -- read once at the first zlib host-path call; a file
 * that is unreadable, empty or longer than TYCHE_LZ4_DICT_MAX makes every zlib host call fail with
 * TYCHE_E_BAD_ARGS and the reason; never silently ignored; tyche_zlib_use_dict replaces it. */
int tyche_zlib_compress_batch_dict(const tyche_dict_t *d, const tyche_batch_t *batch, void *stream);
int tyche_zlib_decompress_batch_dict(const tyche_dict_t *d, const tyche_batch_t *batch, void *stream);
/* process-wide zlib dictionary of the host entry points; NULL removes it.  Holds a reference of its own. */
int tyche_zlib_use_dict(const tyche_dict_t *d);
/* a new reference to the process-wide zlib dictionary (tyche_lz4_dict_destroy drops it), or NULL */
tyche_dict_t *tyche_zlib_current_dict(void);

/* ---- training a dictionary from sample pages ------------------------------ */
/* The trainer picks the 128-byte segments of the sample pages whose 8-byte keys occur in the most
 * other pages, one segment per round, each round discounting what earlier picks already cover
 * (DESIGN.md 3.3d has the algorithm, which defines the bytes: they depend on the pages, their order
 * and dict_len alone, not on the device, the batch layout or the run).  The dictionary is
 * 128 x picks <= dict_len bytes long, the most valuable segment last, where every page can reach it.
 * It runs on the GPU; nothing falls back to the CPU.
 *
 * tyche_lz4_dict_train_batch trains on a device-resident batch (src, src_offsets | src_stride,
 * src_lengths | src_length, count and, beside src_lengths, max_src_length, 0 there meaning 65535;
 * the dst fields and results are ignored) on `stream`, waits for it, and returns a new handle --
 * an ordinary immutable dictionary handle, as from tyche_lz4_dict_create.  tyche_lz4_dict_train_host
 * does the same from host pages.  NULL with the rule and the numbers in tyche_last_error() when:
 * dict_len is outside 128..TYCHE_LZ4_DICT_MAX; count is 0 or above TYCHE_LZ4_TRAIN_MAX_PAGES; a page
 * (or the declared maximum) is above 65535 bytes; the pages hold more than TYCHE_LZ4_TRAIN_MAX_BYTES
 * in total; there is no usable device; or nothing was picked ("the sample pages share no content":
 * no 8-byte key occurs in two pages).
 *
 * TYCHE_LZ4_DICT_AUTO=<bytes> in the environment (opt-in; 128..TYCHE_LZ4_DICT_MAX): the host LZ4
 * compress entry points (buffer__compress, tyche_buffers_compress, tyche_compress_host) copy the
 * pages they are given -- those of at least 128 bytes that the dictionary will reach, length +
 * <bytes> <= 65536 -- into a sample buffer until TYCHE_LZ4_DICT_AUTO_PAGES pages (default 256) or
 * TYCHE_LZ4_TRAIN_MAX_BYTES are collected, compressing exactly as without a dictionary meanwhile.
 * The call that completes the sample trains after its own pages are compressed and installs the
 * result process-wide, once; concurrent callers never wait for the training and compress plain
 * until the install is visible.  A plain block is also a valid dictionary block (its offsets never
 * reach the dictionary), so pages compressed before the install restore through the dictionary
 * decoder afterwards.  If training yields nothing, auto mode ends, the process stays plain and
 * the reason is in tyche_last_error() on the training thread.  The trainer never replaces an
 * installed dictionary: a tyche_lz4_use_dict call made while samples are collected (or while the
 * training runs) ends auto mode and wins.  TYCHE_LZ4_DICT and TYCHE_LZ4_DICT_AUTO both set, or a
 * malformed value, make every LZ4 host call fail with TYCHE_E_BAD_ARGS and the reason; LZ4_EXACT=1
 * with auto mode is the does-not-combine error above. */
#define TYCHE_LZ4_TRAIN_MAX_BYTES (64u << 20)
#define TYCHE_LZ4_TRAIN_MAX_PAGES (1u << 19)
tyche_lz4_dict_t *tyche_lz4_dict_train_batch(const tyche_batch_t *samples, uint32_t dict_len, void *stream);
tyche_lz4_dict_t *tyche_lz4_dict_train_host(size_t n, const void *const *src, const uint32_t *src_lengths,
                                            uint32_t dict_len);

/* ---- host batch API (pinned staging + H2D -> kernels -> D2H) ------------- */
/* Same per-page semantics as the device batch, with host pointers.  Used by
 * the Buffer entry points and by the PCIe-inclusive measurement. */
int tyche_compress_host(int compressor_id, int compressor_level, size_t n, const void *const *src,
                        const uint32_t *src_lengths, void *const *dst, const uint32_t *dst_capacities,
                        int32_t *results);
int tyche_decompress_host(int compressor_id, size_t n, const void *const *src, const uint32_t *src_lengths,
                          void *const *dst, const uint32_t *dst_capacities, int32_t *results);

/* ---- runtime ------------------------------------------------------------- */
/* The reference is one process whose compressor pool (src/list.c:142-168,
 * opts.cpu_count threads, src/manager.c:85) and workers call the codec
 * concurrently; it has no notion of devices.  By default the host entry points
 * (Buffer API, host batches, restore queue) therefore use every visible gfx950
 * device (the first TYCHE_DEVICES of them when that is set): a host batch of at
 * least two parts' worth of input is cut into contiguous page ranges of about
 * equal input bytes, one per device, run concurrently (tyche_plan_split); a
 * smaller one goes whole to the device with the fewest batches in flight, so
 * concurrent per-page callers spread over all devices.  tyche_set_device(d)
 * pins the calling thread to device d instead; TYCHE_ALL_DEVICES undoes that.
 * The device-resident batch API always runs on the caller's current device. */
#define TYCHE_ALL_DEVICES (-1)
int tyche_device_count(void);
/* pins the calling thread's host-path work to `device`, or TYCHE_ALL_DEVICES (default) */
int tyche_set_device(int device);
/* devices the calling thread's host-path work is spread over (1 when pinned) */
int tyche_active_devices(void);
/* The fan-out plan of a host batch (exported so it can be checked without a
 * GPU): splits n pages into at most ndev contiguous ranges of about equal input
 * bytes, each holding at least min_part_bytes of input (0 = no minimum).
 * Writes cuts[0..k] (cuts[0] = 0, cuts[k] = n; cuts needs ndev + 1 entries)
 * and returns the number of ranges k >= 1.  The engine uses
 * min_part_bytes = TYCHE_FANOUT_MIN_BYTES (default 64 MiB, one staging chunk). */
size_t tyche_plan_split(size_t n, const uint32_t *src_lengths, int ndev, uint64_t min_part_bytes, size_t *cuts);
/* Kernel-path switches and tunables (names without the TYCHE_ prefix, e.g.
 * "LZ4_LANE_MIN", "ZLIB_PAR"): the library reads TYCHE_<name> from the
 * environment once and checks for an override on every launch.  Set / drop an
 * in-process override; for tests and A/B timing.  No knob changes a decode
 * result; encoder-shape knobs (LZ4_ENC_WAVES, ZSTD_PARSE_WAVES, ZSTD_FSE_LOG)
 * change the compressed bytes and ratio, never whether they decode to the page.
 * A fourth, LZ4_EXACT (default 0), sends every LZ4 compress launch (pages of up
 * to 65535 bytes, every entry point) to the exact encoder: results[i] and the
 * bytes are those of LZ4 1.7.5's LZ4_compress_default(src, dst, src_len,
 * dst_capacity), including its 0 when a capacity below LZ4_compressBound fails
 * one of its conservative checks, and nothing at or past dst + dst_capacity is
 * written.  src_len == 0 gives the one-byte block 0x00 (result 1; 0 when
 * dst_capacity is 0), as the default encoder does; a page above the launch's
 * maximum still gives INT32_MIN.  It changes the bytes and the time (about 14x
 * the default encoder's), never the decode result.  It is a promise about the
 * reference's byU16 regime only: with the knob on, an LZ4 compress launch whose
 * declared maximum (or a host page) exceeds 65535 bytes fails with
 * TYCHE_E_BAD_ARGS instead of being given another encoder's bytes.
 * A fifth, LZ4_HC (default 0), sends every LZ4 compress launch -- the batch and
 * host calls, buffer__compress, tyche_buffers_compress, the multi-device
 * fan-out -- to the high-compression encoder for its pages of up to 65535
 * bytes: the same LZ4 block format from a better parse (8 candidates per
 * position and a lazy choice), so every decoder restores the streams unchanged.
 * The batch contract is the default encoder's: results[i] is the size, or 0
 * when the stream does not fit dst_capacity; nothing at or past dst +
 * dst_capacity is written; src_len == 0 gives the block 0x00; INT32_MIN above
 * the launch's maximum; a stream is never longer than tyche_compress_bound; the
 * bytes depend on the page alone.  It changes the bytes, the ratio (11-20 %
 * fewer bytes on the 16 KiB bench pages) and the time (about 23x the default
 * encoder's at 16 KiB pages, 10x at 4 KiB), never the decode result.  It is a
 * ratio mode, not a byte promise, so unlike LZ4_EXACT it never makes a launch
 * fail: pages above 65535 bytes keep the large-page encoder and the bytes they
 * have without the knob, also in a launch that mixes sizes.  LZ4_EXACT=1
 * together with LZ4_HC=1 is TYCHE_E_BAD_ARGS from every LZ4 compress call (they
 * contradict each other; tyche_last_error() says so).  A dictionary wins where
 * it reaches: tyche_lz4_compress_batch_dict ignores the knob; with a
 * process-wide dictionary the pages it reaches take the dictionary encoder as
 * without the knob and the others take HC; while TYCHE_LZ4_DICT_AUTO collects
 * its sample, plain pages take HC.  zlib and zstd ignore the knob.
 * A sixth, ZSTD_HC (default 0), sends every zstd compress launch -- the batch
 * and host calls, buffer__compress, tyche_buffers_compress, the multi-device
 * fan-out -- to the high-compression encoder for its pages of up to 65535
 * bytes: the same frame format (single segment, content size, no checksum)
 * from a better parse (8 ring candidates and the repeat offsets per position,
 * chosen by gain, a two-step lazy walk), always through the four-pass encode,
 * so a page's bytes depend on the page alone and every decoder restores the
 * frames unchanged.  The batch contract is the default zstd encoder's:
 * results[i] is the frame's size, or 0 when it does not fit dst_capacity (zstd
 * may also give 0 at or just above the size: its scratch sits in the slot's
 * tail); nothing outside the slot is written; src_len == 0 gives the frame the
 * default encoder gives; INT32_MIN above the launch's maximum, the slot left
 * alone; a frame is never longer than tyche_compress_bound; a declared maximum
 * above 65535 stays TYCHE_E_BAD_ARGS.  It changes the bytes, the ratio (3.0 /
 * 4.3 / 6.4 % fewer bytes on the 4 / 16 / 32 KiB bench pages) and the time
 * (4.1x / 5.1x / 11.0x the default encoder's), never the decode result.
 * compressor_level stays ignored.  A dictionary wins where it reaches:
 * tyche_zstd_compress_batch_dict ignores the knob; with a process-wide zstd
 * dictionary the pages it reaches take the dictionary encoder as without the
 * knob and the others take HC.  LZ4 and zlib ignore the knob; LZ4_HC and
 * ZSTD_HC are independent.  Of the zstd encoder's shape knobs ZSTD_FSE_LOG and
 * ZSTD_SCRATCH_MB keep their effect under it, the parse and split knobs have
 * none.
 * A seventh, ZLIB_HC (default 0), sends every zlib compress launch -- the batch
 * and host calls, buffer__compress, tyche_buffers_compress, the multi-device
 * fan-out -- to the high-compression encoder for its pages of up to 65535
 * bytes: the same stream (header 78 01 -- FLEVEL is informational, inflate does
 * not read it -- one block, adler32) from a better parse (the 16 latest
 * positions of each of 512 buckets and the nearest equal position of the block
 * as candidates, the one of the highest gain 3 * length - extra bits of the
 * distance, no 3-byte match beyond 2048 bytes, a two-step lazy walk) in front
 * of the default encoder's tree and code passes, so a page's bytes depend on the
 * page alone and every decoder restores the streams unchanged.  The batch
 * contract is the default zlib encoder's: results[i] is the stream's size, or 0
 * when it does not fit dst_capacity; nothing outside the slot is written;
 * src_len == 0 gives the stream the default encoder gives; INT32_MIN above the
 * launch's maximum, the slot left alone; a stream is never longer than
 * tyche_compress_bound; a declared maximum above 65535 stays TYCHE_E_BAD_ARGS.
 * It changes the bytes, the ratio (6.2 / 8.9 / 9.7 % fewer bytes on the 4 / 16 /
 * 32 KiB bench pages) and the time (3.0x / 5.9x / 4.4x the default encoder's),
 * never the decode result.  compressor_level stays ignored.  LZ4 and zstd ignore
 * the knob, zlib ignores LZ4_HC and ZSTD_HC; ZLIB_HC_PAGES_PER_CU caps the
 * resident pages per CU (an occupancy A/B, 0: what fits).
 * An eighth, LZ4_HC_DICT (default 0), independent of LZ4_HC, sends every LZ4
 * page that a dictionary reaches (length + dictionary <= 65536) to the
 * high-compression dictionary encoder: tyche_lz4_compress_batch_dict, and with
 * a process-wide dictionary (tyche_lz4_use_dict, TYCHE_LZ4_DICT, or one
 * installed by TYCHE_LZ4_DICT_AUTO) tyche_compress_host, buffer__compress,
 * tyche_buffers_compress and every device of the multi-device fan-out.  It is
 * LZ4_HC's parse over the dictionary encoder's window (8 ring candidates per
 * position, the rings seeded from the dictionary once per handle, a two-step
 * lazy choice), and the contract is the dictionary encoder's, as under "LZ4
 * with a shared dictionary": a standard block whose offsets may reach into the
 * dictionary, restored by tyche_lz4_decompress_batch_dict and
 * LZ4_decompress_safe_usingDict with the same dictionary; results[i] the size,
 * or 0 when the stream does not fit dst_capacity; nothing at or past dst +
 * dst_capacity written; src_len == 0 gives 0x00; INT32_MIN above the launch's
 * maximum; no stream longer than tyche_compress_bound; the bytes depend on the
 * page and the dictionary alone.  Pages outside the reach, and every page
 * while TYCHE_LZ4_DICT_AUTO collects its sample, are as without the knob:
 * LZ4_HC alone decides their encoder.  Without a dictionary the knob does
 * nothing; with the knob at 0, LZ4_HC=1 beside a dictionary is as above.  It
 * never makes a launch fail, and LZ4_EXACT=1 with a dictionary stays
 * TYCHE_E_BAD_ARGS.  zstd and zlib ignore the knob.
 * LZ4_HC_DICT_PAGES_PER_CU caps the resident pages per CU (an occupancy A/B,
 * 0: what fits).
 * Two are test hooks: FAIL_COMPRESS_EVERY=N fails every Nth compress launch
 * (TYCHE_E_DEVICE, the device-failure test) and LOG_ERRORS=1 prints engine
 * errors to stderr. */
int tyche_set_knob(const char *name, long value);
int tyche_clear_knob(const char *name);
/* Diagnostics: host-path stage clocks since the last call, then reset -- out[0..6] = ns waiting for
 * streams, ns scattering, ns gathering, ns enqueuing, bytes gathered, bytes scattered, chunks.
 * Returns the number of values written (at most n). */
int tyche_host_profile(uint64_t *out, int n);
/* message for the last TYCHE_E_DEVICE on this thread */
const char *tyche_last_error(void);
/* 1 if the library's gfx950 code object is usable on the calling thread's
 * (first) device */
int tyche_device_ready(void);

/* ---- synthetic input (bench/tests; same generator as the host copy) ------ */
/* fills `count` pages of page_len bytes at dst + i*stride on the device */
int tyche_pagegen(void *dst, uint64_t stride, uint32_t page_len, uint64_t seed, uint64_t first, size_t count,
                  uint32_t dist, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TYCHE_CODEC_H_ */
