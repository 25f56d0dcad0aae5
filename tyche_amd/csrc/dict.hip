// dict.hip -- the shared-dictionary layer of libtyche_codec.so: the handle and its device copies, the
// process-wide slot of each codec (LZ4, zstd, zlib) with its environment variable,
// TYCHE_LZ4_DICT_AUTO, the training glue, the reach rule of the host path (dict.h) and every
// extern "C" dictionary symbol of include/tyche_codec.h.  Host code only; the kernels it launches are
// engine.h's.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "dict.h"

using namespace tyche;

// A handle is immutable after creation: the bytes, the encoder's dictionary table and the device
// image (engine.h: Lz4DictDev) are built once on the host; the image is uploaded to a device the
// first time a launch there needs it, under the handle's lock.  References: the creator's (dropped
// by tyche_lz4_dict_destroy), each process-wide slot's, and one per host call that runs with a
// process-wide dictionary.  The last one frees the device copies with hipFree, which returns only
// once the device has finished the work submitted before it -- a launch still in flight on a
// caller's stream keeps reading valid memory until it ends.
namespace {
// host bytes and their copy on each device that has used them (under the handle's lock)
struct DevBlob {
    std::vector<uint8_t> host;
    uint8_t *dev[kMaxDevices] = {};
    // the copy on device `at`, the current one, uploaded on first use; `what` names the blob in the error
    hipError_t on(int at, const char *what, const uint8_t **out) {
        if (!dev[at]) {
            uint8_t *p = nullptr;
            hipError_t e = hipMalloc((void **)&p, host.size());
            if (e != hipSuccess) return fail((std::string("hipMalloc(") + what + ")").c_str(), e), e;
            if ((e = hipMemcpy(p, host.data(), host.size(), hipMemcpyHostToDevice)) != hipSuccess) {
                (void)hipFree(p);
                return fail((std::string("hipMemcpy(") + what + ")").c_str(), e), e;
            }
            dev[at] = p;
        }
        *out = dev[at];
        return hipSuccess;
    }
};
}  // namespace

struct tyche_lz4_dict {
    std::atomic<long> refs{1};
    uint32_t len = 0, dpad = 0, enc_len = 0, enc_stride = 0;
    uint32_t adler = 1;   // adler32 of the bytes: zlib's DICTID
    std::mutex mu;
    DevBlob image;   // dec (dpad) | table (8 KiB) | enc (16 x enc_stride)
    // the zstd and the zlib encoder's seeded tables and the LZ4_HC_DICT encoder's seeded rings (engine.h:
    // zstd_dict_seed_table, zlib_dict_seed_table, lz4_hc_dict_seed_table; the seed kind - 1 indexes them),
    // each built at the handle's first compress of that kind and uploaded to a device at its first one
    // there: users of other codecs and modes pay nothing for it
    DevBlob seeds[3];
    const uint8_t *bytes() const { return image.host.data() + (dpad - len); }
};

namespace {
constexpr int kLz4 = TYCHE_LZ4_COMPRESSOR_ID, kZstd = TYCHE_ZSTD_COMPRESSOR_ID, kZlib = TYCHE_ZLIB_COMPRESSOR_ID;   // for dict_codec
enum { kSeedNone = 0, kSeedZstd = 1, kSeedZlib = 2, kSeedLz4Hc = 3 };   // DictCodec::seed; encode_seed
constexpr size_t kDictTableBytes = 4096 * sizeof(uint16_t);
// the encoder's table key (lz_parse.h's hash5 at TYCHE_HASH_LOG 12, lz4_encode_dict.hip): 5 bytes
inline uint32_t dict_hash(const uint8_t *p) {
    uint64_t x = 0;
    memcpy(&x, p, 5);
    return (uint32_t)((x * 0xCF1BBCDCB7A56463ull) >> 52);
}

void dict_retain(const tyche_lz4_dict *d) { const_cast<tyche_lz4_dict *>(d)->refs.fetch_add(1); }
void dict_release(const tyche_lz4_dict *cd) {
    tyche_lz4_dict *d = const_cast<tyche_lz4_dict *>(cd);
    if (!d || d->refs.fetch_sub(1) != 1) return;
    DeviceGuard keep;
    for (int i = 0; i < kMaxDevices; i++)
        if ((d->image.dev[i] || d->seeds[0].dev[i] || d->seeds[1].dev[i] || d->seeds[2].dev[i]) && hipSetDevice(i) == hipSuccess)
            for (DevBlob *b : {&d->image, &d->seeds[0], &d->seeds[1], &d->seeds[2]})
                if (b->dev[i]) (void)hipFree(b->dev[i]);
    delete d;
}

// The handle's image on the current device and, where `seed` is asked for, the seeded table of kind
// `which` (kSeedZstd, kSeedZlib, kSeedLz4Hc) there, each uploaded on first use.  A failure is returned and named
// in the thread's error text.
hipError_t dict_on_device(const tyche_lz4_dict *cd, Lz4DictDev *out, const void **seed, int which) {
    tyche_lz4_dict *d = const_cast<tyche_lz4_dict *>(cd);
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return fail("hipGetDevice", e), e;
    if (dev < 0 || dev >= kMaxDevices) return fail_msg("selected device out of range"), hipErrorInvalidDevice;
    std::lock_guard<std::mutex> g(d->mu);
    const uint8_t *p = nullptr;
    if ((e = d->image.on(dev, "dictionary", &p)) != hipSuccess) return e;
    out->dec = p;
    out->table = (const uint16_t *)(p + d->dpad);
    out->enc = p + d->dpad + kDictTableBytes;
    out->dlen = d->len;
    out->dpad = d->dpad;
    out->enc_len = d->enc_len;
    out->enc_stride = d->enc_stride;
    out->adler = d->adler;
    if (!seed || which == kSeedNone) return hipSuccess;
    DevBlob &sb = d->seeds[which - 1];
    if (sb.host.empty()) {
        const uint8_t *tail = d->image.host.data() + (d->dpad - d->enc_len);
        sb.host.resize(which == kSeedZlib ? zlib_dict_seed_bytes() : which == kSeedLz4Hc ? lz4_hc_dict_seed_bytes() : zstd_dict_seed_bytes());
        if (which == kSeedZlib) zlib_dict_seed_table(tail, d->enc_len, sb.host.data());
        else if (which == kSeedLz4Hc) lz4_hc_dict_seed_table(tail, d->enc_len, sb.host.data());
        else zstd_dict_seed_table(tail, d->enc_len, sb.host.data());
    }
    if ((e = sb.on(dev, "dictionary table", &p)) != hipSuccess) return e;
    *seed = p;
    return hipSuccess;
}

tyche_lz4_dict *dict_create(const void *bytes, uint32_t len) {
    if (!bytes || len == 0 || len > TYCHE_LZ4_DICT_MAX) {
        set_thread_error("an LZ4 dictionary holds 1 to TYCHE_LZ4_DICT_MAX (" + std::to_string(TYCHE_LZ4_DICT_MAX) +
                         ") bytes; got " + (bytes ? std::to_string(len) : std::string("NULL")));
        return nullptr;
    }
    tyche_lz4_dict *d = new tyche_lz4_dict();
    const uint8_t *src = (const uint8_t *)bytes;
    d->len = len;
    d->dpad = (len + 15u) & ~15u;
    d->enc_len = len & ~63u;
    d->enc_stride = d->enc_len + 16u;
    std::vector<uint8_t> &image = d->image.host;
    image.assign((size_t)d->dpad + kDictTableBytes + 16u * (size_t)d->enc_stride, 0);
    memcpy(image.data() + (d->dpad - len), src, len);
    uint32_t a = 1, b = 0;   // adler32.c:65
    for (uint32_t j = 0; j < len; j++) {
        a = (a + src[j]) % 65521u;
        b = (b + a) % 65521u;
    }
    d->adler = (b << 16) | a;
    // every position of the encoder's part whose 5 hashed bytes lie inside it, the last of equal hashes kept
    // (window position j = byte j of the part); an empty slot is position 0, as in a zeroed table
    const uint8_t *tail = src + (len - d->enc_len);
    uint16_t *table = (uint16_t *)(image.data() + d->dpad);
    for (uint32_t j = 0; j + 5u <= d->enc_len; j++) table[dict_hash(tail + j)] = (uint16_t)j;
    uint8_t *enc = image.data() + d->dpad + kDictTableBytes;
    for (uint32_t h = 0; h < 16u; h++) memcpy(enc + (size_t)h * d->enc_stride + h, tail, d->enc_len);
    return d;
}

int bad_args(const std::string &m) {
    set_thread_error(m);
    return TYCHE_E_BAD_ARGS;
}
int dict_exact_conflict() {
    return bad_args("LZ4_EXACT=1 and an LZ4 dictionary do not combine: exact mode promises LZ4_compress_default's bytes");
}
// The bytes are raw content for both codecs; what zstd adds is a rule: bytes that begin with
// ZSTD_DICT_MAGIC would be a structured dictionary to the reference, which this engine does not
// implement: refused, never read as raw content.
bool zdict_structured(const tyche_lz4_dict *d) {
    static const uint8_t magic[4] = {0x37, 0xA4, 0x30, 0xEC};
    return d->len >= 4u && memcmp(d->bytes(), magic, 4) == 0;
}
int zdict_structured_error() {
    return bad_args("zstd dictionary: the bytes begin with ZSTD_DICT_MAGIC (37 A4 30 EC), a structured (entropy-table) "
                    "dictionary; structured dictionaries are not supported, only raw content");
}
// the device-batch calls' refusals that come before count == 0
int lz4_precheck(const tyche_lz4_dict *, bool decode) {
    return !decode && knob("LZ4_EXACT", 0) != 0 ? dict_exact_conflict() : TYCHE_E_OK;
}
int zstd_precheck(const tyche_lz4_dict *d, bool) { return zdict_structured(d) ? zdict_structured_error() : TYCHE_E_OK; }
int zlib_precheck(const tyche_lz4_dict *, bool) { return TYCHE_E_OK; }   // raw bytes are raw bytes to zlib: every handle
// (a seed was asked for: LZ4_HC_DICT was set when the launch read it, encode_seed)
hipError_t lz4_encode_dict(const tyche_batch_t &b, uint32_t in_cap, const Lz4DictDev &d, const void *seed, bool per_page, hipStream_t s) {
    return seed ? launch_lz4_encode_hc_dict(b, in_cap, d, seed, per_page, s) : launch_lz4_encode_dict(b, in_cap, d, per_page, s);
}
uint32_t lz4_stream_bound(uint32_t n) { return lz4_bound(n); }
uint32_t zstd_stream_bound(uint32_t n) { return zstd_bound(n); }
uint32_t zlib_stream_bound(uint32_t n) { return zlib_bound(n); }
}  // namespace

struct tyche::DictCodec {
    const char *name, *label;   // in the reach text; in the launch labels
    const char *env;            // <file>: the process-wide dictionary, read once
    bool (*refuses)(const tyche_lz4_dict *);                 // a handle this codec cannot take (NULL: takes every one)
    int (*precheck)(const tyche_lz4_dict *, bool decode);
    uint32_t (*bound)(uint32_t);
    int seed;                   // the seeded table of the handle's that the encoder takes (kSeedNone: none; encode_seed)
    hipError_t (*encode)(const tyche_batch_t &, uint32_t in_cap, const Lz4DictDev &, const void *seed, bool per_page, hipStream_t);
    hipError_t (*decode)(const tyche_batch_t &, uint32_t in_cap, uint32_t out_cap, const Lz4DictDev &, bool per_page, hipStream_t);
};
const DictCodec &tyche::dict_codec(int compressor_id) {
    static const DictCodec codecs[3] = {
        {"LZ4", "lz4", "TYCHE_LZ4_DICT", nullptr, lz4_precheck, lz4_stream_bound, kSeedNone, lz4_encode_dict, launch_lz4_decode_dict},
        {"zstd", "zstd", "TYCHE_ZSTD_DICT", zdict_structured, zstd_precheck, zstd_stream_bound, kSeedZstd, launch_zstd_encode_dict,
         launch_zstd_decode_dict},
        {"zlib", "zlib", "TYCHE_ZLIB_DICT", nullptr, zlib_precheck, zlib_stream_bound, kSeedZlib, launch_zlib_deflate_dict,
         launch_zlib_inflate_dict}};
    return codecs[compressor_id == kZstd ? 1 : compressor_id == kZlib ? 2 : 0];
}

namespace {
// The seeded table an encode launch asks for, read once per launch: the codec's own, and for LZ4 the
// HC rings when LZ4_HC_DICT is set (the knob chooses lz4_encode_dict's kernel through it) -- zstd and
// zlib never read the knob.
int encode_seed(const DictCodec &c) {
    return &c == &dict_codec(kLz4) ? (knob("LZ4_HC_DICT", 0) != 0 ? kSeedLz4Hc : kSeedNone) : c.seed;
}
// TYCHE_LZ4_DICT_AUTO: the host compress calls collect sample pages (packed in `sample`, their
// lengths in `sample_len`) until `pages` pages or TYCHE_LZ4_TRAIN_MAX_BYTES; the call that
// completes the sample takes it away (kTraining) and trains outside the lock.  Only the LZ4 slot
// has one, under its lock.
struct AutoTrain {
    enum { kOff, kCollecting, kTraining } state = kOff;
    uint32_t len = 0;
    size_t pages = 256;
    std::vector<uint8_t> sample;
    std::vector<uint32_t> sample_len;
    void end() {
        state = kOff;
        std::vector<uint8_t>().swap(sample);
        std::vector<uint32_t>().swap(sample_len);
    }
};
// The process-wide dictionary of a codec's host entry points.  Heap state that is never destroyed: a
// restore dispatcher may still run a batch at exit().  Each codec has its own:
// neither tyche_<codec>_use_dict nor the codec's variables touch another's.
struct DictSlot {
    const DictCodec &c;
    AutoTrain *const autos;   // NULL: the codec has no auto mode
    std::mutex mu;
    const tyche_lz4_dict *d = nullptr;
    bool env_done = false;
    std::string env_error;   // the variable named a file that cannot serve: every host call of the codec fails with it
};
DictSlot &dict_slot(const DictCodec &c) {
    static DictSlot &lz4 = *new DictSlot{dict_codec(kLz4), new AutoTrain}, &zstd = *new DictSlot{dict_codec(kZstd), nullptr},
                    &zlib = *new DictSlot{dict_codec(kZlib), nullptr};
    return &c == &dict_codec(kLz4) ? lz4 : &c == &dict_codec(kZstd) ? zstd : zlib;
}
// TYCHE_LZ4_DICT_AUTO=<bytes> [TYCHE_LZ4_DICT_AUTO_PAGES=<pages>] (slot locked): false when unset
bool auto_env_locked(DictSlot &S, const char *path) {
    const char *a = getenv("TYCHE_LZ4_DICT_AUTO");
    if (!a || !*a) return false;
    if (path && *path) {
        S.env_error = "TYCHE_LZ4_DICT and TYCHE_LZ4_DICT_AUTO are both set: name a dictionary file or have one trained, not both";
        return true;
    }
    char *end = nullptr;
    const long v = strtol(a, &end, 10);
    if (end == a || *end || v < 128 || v > (long)TYCHE_LZ4_DICT_MAX) {
        S.env_error = std::string("TYCHE_LZ4_DICT_AUTO: \"") + a + "\" is not a dictionary length of 128 to TYCHE_LZ4_DICT_MAX (" +
                      std::to_string(TYCHE_LZ4_DICT_MAX) + ") bytes";
        return true;
    }
    if (const char *np = getenv("TYCHE_LZ4_DICT_AUTO_PAGES"); np && *np) {
        const long k = strtol(np, &end, 10);
        if (end == np || *end || k < 1 || k > (long)TYCHE_LZ4_TRAIN_MAX_PAGES) {
            S.env_error = std::string("TYCHE_LZ4_DICT_AUTO_PAGES: \"") + np + "\" is not a page count of 1 to TYCHE_LZ4_TRAIN_MAX_PAGES (" +
                          std::to_string(TYCHE_LZ4_TRAIN_MAX_PAGES) + ")";
            return true;
        }
        S.autos->pages = (size_t)k;
    }
    S.autos->len = (uint32_t)v;
    S.autos->state = AutoTrain::kCollecting;
    return true;
}
// the codec's variable = <file>, read once (slot locked)
void dict_env_locked(DictSlot &S) {
    if (S.env_done) return;
    S.env_done = true;
    const char *path = getenv(S.c.env);
    if (S.autos && auto_env_locked(S, path)) return;
    if (!path || !*path) return;
    const std::string var = std::string(S.c.env) + ": ";
    std::vector<uint8_t> buf(TYCHE_LZ4_DICT_MAX + 1u);
    FILE *f = fopen(path, "rb");
    if (!f) {
        S.env_error = var + "cannot read " + path;
        return;
    }
    const size_t n = fread(buf.data(), 1, buf.size(), f);
    fclose(f);
    if (n == 0 || n > TYCHE_LZ4_DICT_MAX) {
        S.env_error = var + path + (n == 0 ? " is empty" : " is longer than TYCHE_LZ4_DICT_MAX (" +
                      std::to_string(TYCHE_LZ4_DICT_MAX) + " bytes)");
        return;
    }
    tyche_lz4_dict *d = dict_create(buf.data(), (uint32_t)n);
    if (d && S.c.refuses && S.c.refuses(d)) {
        dict_release(d);
        S.env_error = var + path + " begins with ZSTD_DICT_MAGIC (37 A4 30 EC), a structured "
                      "dictionary; structured dictionaries are not supported, only raw content";
        return;
    }
    S.d = d;
}
int dict_use(const DictCodec &c, const tyche_lz4_dict *d) {
    if (d && c.refuses && c.refuses(d)) return zdict_structured_error();
    DictSlot &S = dict_slot(c);
    const tyche_lz4_dict *old;
    {
        std::lock_guard<std::mutex> g(S.mu);
        S.env_done = true;   // an explicit choice replaces whatever the codec's variable names
        S.env_error.clear();
        if (S.autos) S.autos->end();   // and ends TYCHE_LZ4_DICT_AUTO: a training still running will not install
        old = S.d;
        if (d) dict_retain(d);
        S.d = d;
    }
    dict_release(old);
    return TYCHE_E_OK;
}
tyche_lz4_dict *dict_current(const DictCodec &c) {
    DictSlot &S = dict_slot(c);
    std::lock_guard<std::mutex> g(S.mu);
    dict_env_locked(S);
    if (S.d) dict_retain(S.d);
    return const_cast<tyche_lz4_dict *>(S.d);
}

int dict_reach_error(const DictCodec &c, bool decode, uint32_t cap, uint32_t dlen) {
    return bad_args(std::string(c.name) + " dictionary reach: the launch's largest " + (decode ? "capacity" : "page") + " (" +
                    std::to_string(cap) + ") plus the dictionary (" + std::to_string(dlen) + " bytes) exceeds 65536");
}
// the six tyche_<codec>_<direction>_batch_dict calls
int batch_dict(const DictCodec &c, bool decode, const tyche_lz4_dict *d, const tyche_batch_t *batch, hipStream_t s) {
    if (!d || !batch) return TYCHE_E_BAD_ARGS;
    if (int rc = c.precheck(d, decode)) return rc;
    if (batch->count == 0) return TYCHE_E_OK;
    if (!batch->src || !batch->dst || !batch->results) return TYCHE_E_BAD_ARGS;
    const uint32_t cap = decode ? batch->dst_capacity : encode_in_cap(*batch);
    if ((uint64_t)cap + d->len > 65536u) return dict_reach_error(c, decode, cap, d->len);
    DeviceGuard keep;
    if (int rc = stream_device(s)) return rc;
    Lz4DictDev img;
    const void *seed = nullptr;
    const int which = decode ? kSeedNone : encode_seed(c);
    if (dict_on_device(d, &img, which ? &seed : nullptr, which) != hipSuccess) return TYCHE_E_DEVICE;
    hipError_t e;
    if (decode)
        // (a declared stream maximum is only a bound -- a slot width, say: above the longest stream a
        // 65,536-byte window can need it is taken as that, and a page whose stream is longer still gets
        // INT32_MIN)
        e = c.decode(*batch, std::min(decode_in_cap(*batch, c.bound(cap)), c.bound(65536u)), cap, img, false, s);
    else
        e = compress_launch_fails() ? hipErrorLaunchFailure   // the FAIL_COMPRESS_EVERY test hook, as launch_encode
                                    : c.encode(*batch, cap, img, seed, false, s);
    if (e != hipSuccess) return fail((std::string(c.label) + " dictionary " + (decode ? "decode" : "encode") + " launch").c_str(), e);
    return TYCHE_E_OK;
}
}  // namespace

// ---- the host entry points' side (dict.h)
int tyche::DictHold::get(const DictCodec &c) {
    DictSlot &S = dict_slot(c);
    std::lock_guard<std::mutex> g(S.mu);
    dict_env_locked(S);
    if (!S.env_error.empty()) return bad_args(S.env_error);
    if (S.d) dict_retain(S.d);
    d = S.d;
    return TYCHE_E_OK;
}
tyche::DictHold::~DictHold() { dict_release(d); }

hipError_t tyche::DictUploadNote::upload(const tyche_lz4_dict *d, Lz4DictDev *img, const void **seed, int which) {
    const hipError_t why = dict_on_device(d, img, seed, which);
    if (why == hipSuccess) return why;
    std::lock_guard<std::mutex> g(mu);
    if (msg.empty()) msg = thread_error();
    return why;
}
int tyche::DictUploadNote::finish(int rc) {
    if (rc != TYCHE_E_OK && !msg.empty()) {
        set_thread_error(msg);
        log_error(msg);
    }
    return rc;
}

hipError_t tyche::dict_launch(const DictCodec &c, bool decode, const tyche_lz4_dict *d, DictUploadNote &note,
                              const tyche_batch_t &b, hipStream_t s, bool host_dst, LaunchRef plain) {
    Lz4DictDev img;
    const void *seed = nullptr;
    const int which = decode ? kSeedNone : encode_seed(c);
    if (const hipError_t ue = note.upload(d, &img, which ? &seed : nullptr, which)) return ue;
    const uint32_t reach = 65536u - d->len, longest = std::max(b.max_src_length, 1u);
    const uint32_t in_cap = decode ? std::min(b.max_src_length, c.bound(65536u)) : longest;   // (a stream bound, as batch_dict's)
    const uint32_t cap = decode ? b.dst_capacity : longest;
    auto launch = [&](uint32_t limit, bool per_page) {
        return decode ? c.decode(b, in_cap, limit, img, per_page, s) : c.encode(b, limit, img, seed, per_page, s);
    };
    // (FAIL_COMPRESS_EVERY counts a compress launch once: here, or in the plain launch's launch_encode)
    if (cap <= reach) return !decode && compress_launch_fails() ? hipErrorLaunchFailure : launch(cap, false);
    const hipError_t e = plain(b, s, host_dst);
    if (e != hipSuccess) return e;
    return launch(reach, true);
}

int tyche::lz4_host_compress_rules(const tyche_lz4_dict *d, size_t n, const void *const *src, const uint32_t *src_lengths,
                                   AutoSample *out) {
    if (d) return knob("LZ4_EXACT", 0) != 0 ? dict_exact_conflict() : TYCHE_E_OK;
    DictSlot &S = dict_slot(dict_codec(kLz4));
    AutoTrain &A = *S.autos;
    std::lock_guard<std::mutex> g(S.mu);
    if (A.state == AutoTrain::kOff) return TYCHE_E_OK;
    if (knob("LZ4_EXACT", 0) != 0) return dict_exact_conflict();
    if (A.state != AutoTrain::kCollecting) return TYCHE_E_OK;
    bool full = false;
    for (size_t i = 0; i < n && !full; i++) {
        const uint32_t L = src_lengths[i];
        if (L < 128u || (uint64_t)L + A.len > 65536u) continue;
        if (A.sample.size() + L > TYCHE_LZ4_TRAIN_MAX_BYTES) {
            full = true;
            break;
        }
        const uint8_t *p = (const uint8_t *)src[i];
        A.sample.insert(A.sample.end(), p, p + L);
        A.sample_len.push_back(L);
        full = A.sample_len.size() >= A.pages;
    }
    if (!full) return TYCHE_E_OK;
    out->dict_len = A.len;
    out->data.swap(A.sample);
    out->len.swap(A.sample_len);
    A.state = AutoTrain::kTraining;
    return TYCHE_E_OK;
}

// ---- training (lz4_dict_train.hip).  The rules that need no device come first, so that they read
// the same with and without one; each names itself and its numbers in the thread's error text.
namespace {
std::nullptr_t train_refuse(const std::string &m) {
    set_thread_error(m);
    log_error(m);
    return nullptr;
}
bool train_args_ok(uint32_t dict_len, size_t count) {
    if (dict_len < 128u || dict_len > TYCHE_LZ4_DICT_MAX)
        return train_refuse("LZ4 dictionary training: dict_len (" + std::to_string(dict_len) + ") must be 128 to TYCHE_LZ4_DICT_MAX (" +
                            std::to_string(TYCHE_LZ4_DICT_MAX) + ") bytes"), false;
    if (count == 0) return train_refuse("LZ4 dictionary training: count is 0, there are no sample pages"), false;
    if (count > TYCHE_LZ4_TRAIN_MAX_PAGES)
        return train_refuse("LZ4 dictionary training: " + std::to_string(count) + " sample pages are more than TYCHE_LZ4_TRAIN_MAX_PAGES (" +
                            std::to_string(TYCHE_LZ4_TRAIN_MAX_PAGES) + ")"), false;
    return true;
}
std::nullptr_t train_page_too_long(const std::string &which, uint64_t len) {
    return train_refuse("LZ4 dictionary training: " + which + " (" + std::to_string(len) + " bytes) is above 65535 bytes");
}
std::nullptr_t train_too_many_bytes(uint64_t total) {
    return train_refuse("LZ4 dictionary training: the sample pages hold " + std::to_string(total) +
                        " bytes, more than TYCHE_LZ4_TRAIN_MAX_BYTES (" + std::to_string(TYCHE_LZ4_TRAIN_MAX_BYTES) + ")");
}
// the batch is on the current device, its arguments checked
tyche_lz4_dict *train_on_device(const tyche_batch_t &b, uint32_t in_cap, uint32_t dict_len, hipStream_t s) {
    std::vector<uint8_t> bytes(dict_len);
    TrainResult r;
    const hipError_t e = train_lz4_dict(b, in_cap, dict_len, s, bytes.data(), &r);
    if (e != hipSuccess) return fail((std::string("lz4 dictionary training (") + r.step + ")").c_str(), e), nullptr;
    if (r.too_long)
        return train_refuse("LZ4 dictionary training: a sample page is longer than the batch's declared maximum (" +
                            std::to_string(in_cap) + " bytes; at most 65535)");
    if (r.total_bytes > TYCHE_LZ4_TRAIN_MAX_BYTES) return train_too_many_bytes(r.total_bytes);
    if (r.dict_len == 0)
        return train_refuse("LZ4 dictionary training: the sample pages share no content (no 8-byte key occurs in two of the " +
                            std::to_string(b.count) + " pages), so there is nothing to put into a dictionary");
    return dict_create(bytes.data(), r.dict_len);
}
// n pages packed one after another in `data`
tyche_lz4_dict *train_packed(const uint8_t *data, const uint32_t *lens, size_t n, uint32_t dict_len) {
    DeviceGuard keep;
    int dev = 0;
    if (current_device(&dev) != TYCHE_E_OK || ensure_device(dev) != TYCHE_E_OK) return nullptr;
    uint64_t total = 0;
    uint32_t longest = 0;
    std::vector<uint64_t> offs(n);
    for (size_t i = 0; i < n; i++) {
        offs[i] = total;
        total += lens[i];
        longest = std::max(longest, lens[i]);
    }
    const size_t data_bytes = ((size_t)total + 15u) & ~(size_t)15u, off_bytes = n * sizeof(uint64_t);
    uint8_t *dm = nullptr;
    hipError_t e = hipMalloc((void **)&dm, data_bytes + 16u + off_bytes + n * sizeof(uint32_t));
    if (e != hipSuccess) return fail("hipMalloc(sample pages)", e), nullptr;
    uint64_t *d_off = (uint64_t *)(dm + data_bytes + 16u);
    uint32_t *d_len = (uint32_t *)(dm + data_bytes + 16u + off_bytes);
    if ((total && (e = hipMemcpy(dm, data, (size_t)total, hipMemcpyHostToDevice)) != hipSuccess) ||
        (e = hipMemcpy(d_off, offs.data(), off_bytes, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(d_len, lens, n * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) {
        (void)hipFree(dm);
        return fail("hipMemcpy(sample pages)", e), nullptr;
    }
    tyche_batch_t b = {};
    b.count = n;
    b.src = dm;
    b.src_offsets = d_off;
    b.src_lengths = d_len;
    b.max_src_length = longest;
    tyche_lz4_dict *d = train_on_device(b, std::max(longest, 1u), dict_len, nullptr);
    (void)hipFree(dm);
    return d;
}
}  // namespace

void tyche::auto_train_and_install(const AutoSample &a) {
    tyche_lz4_dict *d = train_packed(a.data.data(), a.len.data(), a.len.size(), a.dict_len);
    DictSlot &S = dict_slot(dict_codec(kLz4));
    {
        std::lock_guard<std::mutex> g(S.mu);
        if (S.autos->state == AutoTrain::kTraining) {
            S.autos->state = AutoTrain::kOff;
            if (d && !S.d) {
                S.d = d;   // the slot takes the creator's reference
                d = nullptr;
            }
        }
    }
    dict_release(d);
}

extern "C" {

tyche_lz4_dict_t *tyche_lz4_dict_create(const void *bytes, uint32_t len) { return dict_create(bytes, len); }

void tyche_lz4_dict_destroy(tyche_lz4_dict_t *d) { dict_release(d); }

uint32_t tyche_lz4_dict_length(const tyche_lz4_dict_t *d) { return d ? d->len : 0u; }

uint32_t tyche_lz4_dict_bytes(const tyche_lz4_dict_t *d, void *out, uint32_t cap) {
    if (!d) return 0u;
    if (out && cap) memcpy(out, d->bytes(), std::min(cap, d->len));
    return d->len;
}

int tyche_lz4_use_dict(const tyche_lz4_dict_t *d) { return dict_use(dict_codec(kLz4), d); }
int tyche_zstd_use_dict(const tyche_dict_t *d) { return dict_use(dict_codec(kZstd), d); }
int tyche_zlib_use_dict(const tyche_dict_t *d) { return dict_use(dict_codec(kZlib), d); }
tyche_lz4_dict_t *tyche_lz4_current_dict(void) { return dict_current(dict_codec(kLz4)); }
tyche_dict_t *tyche_zstd_current_dict(void) { return dict_current(dict_codec(kZstd)); }
tyche_dict_t *tyche_zlib_current_dict(void) { return dict_current(dict_codec(kZlib)); }

int tyche_lz4_compress_batch_dict(const tyche_lz4_dict_t *d, const tyche_batch_t *batch, void *stream) {
    return batch_dict(dict_codec(kLz4), false, d, batch, (hipStream_t)stream);
}
int tyche_lz4_decompress_batch_dict(const tyche_lz4_dict_t *d, const tyche_batch_t *batch, void *stream) {
    return batch_dict(dict_codec(kLz4), true, d, batch, (hipStream_t)stream);
}
int tyche_zstd_compress_batch_dict(const tyche_dict_t *d, const tyche_batch_t *batch, void *stream) {
    return batch_dict(dict_codec(kZstd), false, d, batch, (hipStream_t)stream);
}
int tyche_zstd_decompress_batch_dict(const tyche_dict_t *d, const tyche_batch_t *batch, void *stream) {
    return batch_dict(dict_codec(kZstd), true, d, batch, (hipStream_t)stream);
}

int tyche_zlib_compress_batch_dict(const tyche_dict_t *d, const tyche_batch_t *batch, void *stream) {
    return batch_dict(dict_codec(kZlib), false, d, batch, (hipStream_t)stream);
}
int tyche_zlib_decompress_batch_dict(const tyche_dict_t *d, const tyche_batch_t *batch, void *stream) {
    return batch_dict(dict_codec(kZlib), true, d, batch, (hipStream_t)stream);
}

tyche_lz4_dict_t *tyche_lz4_dict_train_batch(const tyche_batch_t *samples, uint32_t dict_len, void *stream) {
    if (!samples) return train_refuse("LZ4 dictionary training: samples is NULL");
    if (!train_args_ok(dict_len, samples->count)) return nullptr;
    if (!samples->src) return train_refuse("LZ4 dictionary training: samples->src is NULL");
    const uint32_t in_cap = encode_in_cap(*samples);
    if (in_cap > 65535u) return train_page_too_long(samples->src_lengths ? "the batch's declared maximum" : "src_length", in_cap);
    if (!samples->src_lengths && (uint64_t)samples->count * in_cap > TYCHE_LZ4_TRAIN_MAX_BYTES)
        return train_too_many_bytes((uint64_t)samples->count * in_cap);
    DeviceGuard keep;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return fail_msg("no HIP device available (the codec runs only on the GPU)"), nullptr;
    if (stream_device((hipStream_t)stream)) return nullptr;
    return train_on_device(*samples, std::max(in_cap, 1u), dict_len, (hipStream_t)stream);
}

tyche_lz4_dict_t *tyche_lz4_dict_train_host(size_t n, const void *const *src, const uint32_t *src_lengths,
                                            uint32_t dict_len) {
    if (!train_args_ok(dict_len, n)) return nullptr;
    if (!src || !src_lengths) return train_refuse("LZ4 dictionary training: src or src_lengths is NULL");
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) {
        if (src_lengths[i] > 65535u) return train_page_too_long("page " + std::to_string(i), src_lengths[i]);
        total += src_lengths[i];
    }
    if (total > TYCHE_LZ4_TRAIN_MAX_BYTES) return train_too_many_bytes(total);
    std::vector<uint8_t> data((size_t)total);
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        if (src_lengths[i]) memcpy(data.data() + at, src[i], src_lengths[i]);
        at += src_lengths[i];
    }
    return train_packed(data.data(), src_lengths, n, dict_len);
}

}  // extern "C"
