// engine.hip -- the C ABI of libtyche_codec.so (declared in include/tyche_codec.h).
//
// Drop-in for tyche's codec boundary, src/buffer.c:159-281: buffer__compress /
// buffer__decompress keep the reference's argument checks, their order, the
// error codes, the free()-compatible ownership and the comp_length /
// comp_cost / comp_hits side effects, but the codec runs as gfx950 kernels.
// The batch entry points let the sweep (src/list.c:1039-1063) and restore
// (src/list.c:563-589) callers hand over many pages per launch, and the
// device-resident API is what bench.py measures.  The entry points that start
// and end in host memory hand their launch to run_host (host_batch.hip).
//
// There is no CPU codec in this library: if the HIP device or the gfx950 code
// object is unavailable every codec entry point returns an error.
#include <hip/hip_runtime.h>
#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "dict.h"
#include "engine.h"
#include "host_batch.h"

#include <immintrin.h>

using namespace tyche;

namespace {
// ------------------------------------------------------------- work counters
// One pool of device counters per device.  An entry is free, leased (between
// WorkCounter's constructor and destructor), or released: an event recorded on
// the launch stream after the kernel that claims pages from it.  A released
// entry is handed out again only when its event has completed, so a counter is
// never reset while a kernel on any stream still claims from it.
struct CounterPool {
    struct Entry {
        unsigned *p;
        hipEvent_t ev;
        int state;   // 0 free, 1 leased, 2 released (event pending)
    };
    std::mutex mu;
    std::vector<Entry> e;
    size_t cursor = 0;
    unsigned *junk = nullptr;   // shared by launches whose grid covers all their pages
};
CounterPool *const g_counters = new CounterPool[kMaxDevices];   // never destroyed (restore dispatchers may run at exit)
constexpr size_t kCounterBlock = 64;
}  // namespace

tyche::WorkCounter::WorkCounter(hipStream_t s, bool claims) : s_(s) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return;
    CounterPool &P = g_counters[dev];
    std::lock_guard<std::mutex> g(P.mu);
    if (!claims) {
        // the grid covers every page: each claim returns >= gridDim.x >= count whatever the
        // counter holds, so one shared, never-reset counter serves every such launch (no
        // memset on the stream, no event)
        if (!P.junk && hipMalloc((void **)&P.junk, sizeof(unsigned)) != hipSuccess) P.junk = nullptr;
        p_ = P.junk;
        return;
    }
    const size_t n = P.e.size();
    size_t take = n;
    for (size_t k = 0; k < n; k++) {   // from the oldest release on: those are done first
        const size_t i = (P.cursor + k) % n;
        CounterPool::Entry &x = P.e[i];
        if (x.state == 1) continue;
        if (x.state == 2 && hipEventQuery(x.ev) != hipSuccess) continue;   // its kernel may still run
        take = i;
        break;
    }
    if (take == n) {   // all in use: one more block
        unsigned *blk = nullptr;
        if (hipMalloc((void **)&blk, kCounterBlock * sizeof(unsigned)) != hipSuccess) return;
        for (size_t j = 0; j < kCounterBlock; j++) {
            hipEvent_t ev;
            if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) break;
            P.e.push_back({blk + j, ev, 0});
        }
        if (P.e.size() == n) return;
    }
    CounterPool::Entry &x = P.e[take];
    if (hipMemsetAsync(x.p, 0, sizeof(unsigned), s) != hipSuccess) return;
    x.state = 1;
    P.cursor = take + 1;
    dev_ = dev;
    idx_ = (int)take;
    p_ = x.p;
}

tyche::WorkCounter::~WorkCounter() {
    if (idx_ < 0) return;
    CounterPool &P = g_counters[dev_];
    std::lock_guard<std::mutex> g(P.mu);
    CounterPool::Entry &x = P.e[(size_t)idx_];
    if (hipEventRecord(x.ev, s_) == hipSuccess) {
        x.state = 2;
    } else {
        (void)hipStreamSynchronize(s_);   // no event: wait for the launch instead
        x.state = 0;
    }
}

namespace {
struct ScratchPool {
    struct Entry {
        void *p;
        size_t bytes;
        hipEvent_t ev;
        int state;   // 0 free, 1 leased, 2 released (event pending)
    };
    std::mutex mu;
    std::vector<Entry> e;
};
ScratchPool *const g_scratch = new ScratchPool[kMaxDevices];   // never destroyed (restore dispatchers may run at exit)
}  // namespace

// Leases are sized by the request (1 MiB granules) and reused best-fit, never
// for a request under a quarter of their size (a small launch must not pin a
// chunked zstd decode's gigabytes).  Idle entries beyond kPoolKeep bytes per
// device are freed, largest first, whenever a lease is taken, and a failed
// allocation frees every idle entry and tries once more.
constexpr size_t kPoolKeep = size_t(2) << 30;

namespace {
bool entry_idle(ScratchPool::Entry &x) {
    return x.state == 0 || (x.state == 2 && hipEventQuery(x.ev) == hipSuccess && ((x.state = 0), true));
}
// takes idle entries (largest first) out of the pool until it holds at most `keep` bytes; under
// P.mu.  The caller frees what it returns (free_entries) after releasing P.mu: hipFree synchronises
// the device, and neither the other streams nor the other lease requests should wait on that.
std::vector<ScratchPool::Entry> pool_trim(ScratchPool &P, size_t keep) {
    std::vector<ScratchPool::Entry> out;
    size_t total = 0;
    for (auto &x : P.e) total += x.bytes;
    while (total > keep) {
        size_t best = P.e.size();
        for (size_t i = 0; i < P.e.size(); i++)
            if (entry_idle(P.e[i]) && (best == P.e.size() || P.e[i].bytes > P.e[best].bytes)) best = i;
        if (best == P.e.size()) break;
        out.push_back(P.e[best]);
        total -= P.e[best].bytes;
        P.e.erase(P.e.begin() + (long)best);
    }
    return out;
}
void free_entries(const std::vector<ScratchPool::Entry> &v) {
    for (const auto &x : v) {
        (void)hipFree(x.p);
        (void)hipEventDestroy(x.ev);
    }
}
}  // namespace

size_t tyche::scratch_idle_bytes() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 0;
    ScratchPool &P = g_scratch[dev];
    std::lock_guard<std::mutex> g(P.mu);
    size_t idle = 0;
    for (auto &x : P.e)
        if (entry_idle(x)) idle += x.bytes;
    return idle;
}

tyche::ScratchLease::ScratchLease(hipStream_t s, size_t bytes) : s_(s) {
    if (bytes == 0) return;   // nothing asked: get() is null
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return;
    ScratchPool &P = g_scratch[dev];
    const size_t want = (std::max<size_t>(bytes, 1) + 0xFFFFF) & ~size_t(0xFFFFF);
    // test hook: each new value of the SCRATCH_OOM_SEQ knob makes one lease skip the pool and see its
    // first hipMalloc fail (a real, oversized request: the HIP error slot is set as by a real OOM)
    static std::atomic<long> oom_seq{0};
    const long seq = knob("SCRATCH_OOM_SEQ", 0);
    const bool force_oom = seq != 0 && oom_seq.exchange(seq) != seq;
    auto lease = [&](size_t i) {
        P.e[i].state = 1;
        dev_ = dev;
        idx_ = (int)i;
        p_ = P.e[i].p;
    };
    // best fit among idle entries of at most 4x the request; without one, the pool is trimmed and
    // the victims freed (outside the lock: hipFree synchronises the device) BEFORE the new
    // allocation, so device memory never holds both; then a second look (another thread may have
    // released a fitting entry meanwhile) and only then hipMalloc
    for (int pass = 0; pass < 2; pass++) {
        std::vector<ScratchPool::Entry> victims;
        {
            std::lock_guard<std::mutex> g(P.mu);
            size_t take = P.e.size();
            for (size_t i = 0; i < P.e.size(); i++) {
                ScratchPool::Entry &x = P.e[i];
                if (x.state == 1 || x.bytes < want || x.bytes / 4 > want) continue;
                if (!entry_idle(x)) continue;
                if (take == P.e.size() || x.bytes < P.e[take].bytes) take = i;
            }
            if (take < P.e.size() && !force_oom) {
                lease(take);
                return;
            }
            if (pass == 0) victims = pool_trim(P, kPoolKeep > want ? kPoolKeep - want : 0);
        }
        if (victims.empty()) break;
        free_entries(victims);
    }
    ScratchPool::Entry x{nullptr, want, nullptr, 0};
    if ((force_oom ? hipMalloc(&x.p, size_t(1) << 62) : hipMalloc(&x.p, x.bytes)) != hipSuccess) {
        // out of memory: every idle entry goes, then one more try.  The failed call's error stays in
        // the thread's HIP error slot, where the launch helpers' hipGetLastError() would report a
        // recovered allocation as a failed launch: clear it.
        (void)hipGetLastError();
        std::vector<ScratchPool::Entry> all;
        {
            std::lock_guard<std::mutex> g(P.mu);
            all = pool_trim(P, 0);
        }
        free_entries(all);
        if (hipMalloc(&x.p, x.bytes) != hipSuccess) {
            (void)hipGetLastError();   // reported by get() == nullptr: the caller's own error path
            return;
        }
    }
    if (hipEventCreateWithFlags(&x.ev, hipEventDisableTiming) != hipSuccess) {
        (void)hipFree(x.p);
        (void)hipGetLastError();
        return;
    }
    std::lock_guard<std::mutex> g(P.mu);
    P.e.push_back(x);
    lease(P.e.size() - 1);
}

tyche::ScratchLease::~ScratchLease() {
    if (idx_ < 0) return;
    ScratchPool &P = g_scratch[dev_];
    std::lock_guard<std::mutex> g(P.mu);
    // by address: pool_trim may have erased (idle) entries before this one since the lease
    size_t i = 0;
    while (i < P.e.size() && P.e[i].p != p_) i++;
    if (i == P.e.size()) return;
    ScratchPool::Entry &x = P.e[i];
    if (hipEventRecord(x.ev, s_) == hipSuccess) {
        x.state = 2;
    } else {
        (void)hipStreamSynchronize(s_);
        x.state = 0;
    }
}

size_t tyche::prepare_launch(const void *kernel) {
    static std::mutex &mu = *new std::mutex;   // never destroyed, like the pools (dispatchers at exit)
    static auto &raised = *new std::set<std::pair<int, const void *>>;
    static int cus[kMaxDevices] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= kMaxDevices) return 256;
    std::lock_guard<std::mutex> g(mu);
    if (cus[dev] == 0) {
        int n = 0;
        (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        cus[dev] = n > 0 ? n : 256;
    }
    if (raised.insert({dev, kernel}).second)
        (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    return (size_t)cus[dev];
}

size_t tyche::blocks_per_cu(const void *kernel, uint32_t threads, size_t lds) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, (int)threads, lds) == hipSuccess && n > 0) return (size_t)n;
    if (threads != 64) return 1;
    const size_t granted = (lds + 511u) & ~(size_t)511u;
    return granted ? std::max<size_t>(1, std::min<size_t>(32, (160 * 1024) / granted)) : 32;
}

size_t tyche::page_grid(const void *kernel, uint32_t threads, size_t lds, size_t count, const char *cap_knob) {
    const size_t ncu = prepare_launch(kernel);
    if (count <= ncu) return count;
    size_t per_cu = blocks_per_cu(kernel, threads, lds);
    const long cap_cu = cap_knob ? knob(cap_knob, 0) : 0;   // (occupancy A/B: resident pages per CU; 0: what fits)
    if (cap_cu > 0) per_cu = std::min<size_t>(per_cu, (size_t)cap_cu);
    return std::min<size_t>(count, ncu * per_cu);
}

namespace {
struct KnobTable {
    std::mutex mu;
    std::map<std::string, long> over;                    // tyche_set_knob
    std::map<std::string, std::pair<bool, long>> env;    // TYCHE_<name>: (present, value)
};
KnobTable &knob_table() {
    static KnobTable *t = new KnobTable;   // never destroyed: detached pool threads may still read it at exit
    return *t;
}
}  // namespace

namespace {
// Knobs are read on every launch (a restore reads ~10).  The table's lookups (mutex, string maps) cost
// ~0.1-0.3 us each, so each thread keeps what it read, keyed by the name's address (the call sites
// pass literals), until tyche_set_knob / tyche_clear_knob bump the generation.
std::atomic<uint64_t> g_knob_gen{1};
struct KnobSeen {
    const char *name;
    uint64_t gen;
    bool present;
    long value;
};
constexpr int kKnobCache = 64;
thread_local KnobSeen t_knobs[kKnobCache];
bool knob_slow(const char *name, long &value) {
    KnobTable &T = knob_table();
    std::lock_guard<std::mutex> g(T.mu);
    const auto o = T.over.find(name);
    if (o != T.over.end()) {
        value = o->second;
        return true;
    }
    auto e = T.env.find(name);
    if (e == T.env.end()) {
        const char *v = getenv((std::string("TYCHE_") + name).c_str());
        e = T.env.emplace(name, std::make_pair(v != nullptr && *v, v ? strtol(v, nullptr, 10) : 0L)).first;
    }
    value = e->second.second;
    return e->second.first;
}
}  // namespace

long tyche::knob(const char *name, long dflt) {
    const uint64_t gen = g_knob_gen.load(std::memory_order_acquire);
    const uint32_t h = (uint32_t)(((uintptr_t)name * 0x9E3779B97F4A7C15ull) >> 58);   // 6 bits
    for (int k = 0; k < 4; k++) {   // a short probe; a miss just takes the table
        KnobSeen &c = t_knobs[(h + (uint32_t)k) % kKnobCache];
        if (c.name == name && c.gen == gen) return c.present ? c.value : dflt;
        if (c.name == nullptr || c.gen != gen || k == 3) {
            long v = 0;
            const bool present = knob_slow(name, v);
            c = KnobSeen{name, gen, present, v};
            return present ? v : dflt;
        }
    }
    return dflt;   // (unreachable)
}

namespace {

// -1: the host API spreads work over every usable device (the default);
// >= 0: tyche_set_device pinned the calling thread to that device
thread_local int t_device = -1;
thread_local std::string t_error;

bool device_is_gfx950(int dev) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}
}  // namespace

// TYCHE_LOG_ERRORS=1: every engine failure is also printed to stderr (one
// "tyche-engine: ..." line), so a caller that drops the status -- list.c:1051
// keeps going on any rv but 124 -- still leaves a trace (the C1 tests fail on it).
// The line goes straight to fd 2 (one write): the reference app's stderr is a stdio
// stream it also prints progress to, and a buffered line would be lost when the
// app then crashes (the unchanged caller's lost page, test_c1_app.py).
void tyche::log_error(const std::string &m) {
    if (!knob("LOG_ERRORS", 0)) return;
    const std::string line = "tyche-engine: " + m + "\n";
    (void)!write(2, line.data(), line.size());
}

// ---- shared with the host pipeline (host_batch.h)
int tyche::fail(const char *what, hipError_t e) {
    t_error = std::string(what) + ": " + hipGetErrorString(e);
    log_error(t_error);
    return TYCHE_E_DEVICE;
}
int tyche::fail_msg(const std::string &m) {
    t_error = m;
    log_error(t_error);
    return TYCHE_E_DEVICE;
}
const std::string &tyche::thread_error() { return t_error; }
void tyche::set_thread_error(const std::string &m) { t_error = m; }
int tyche::pinned_device() { return t_device; }

uint64_t tyche::now_ns() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

const DeviceSet &tyche::device_set() {
    static DeviceSet &ds = *new DeviceSet([] {
        DeviceSet d;
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
            d.why = "no HIP device available (the codec runs only on the GPU)";
            return d;
        }
        // TYCHE_DEVICE_IDS: an explicit list ("0,1,2"; repeats allowed, which lets
        // one GPU rehearse the multi-device fan-out in tests)
        if (const char *ids = getenv("TYCHE_DEVICE_IDS")) {
            for (const char *p = ids; *p;) {
                char *end = nullptr;
                const long v = strtol(p, &end, 10);
                if (end == p) break;
                if (v >= 0 && v < n && v < kMaxDevices && device_is_gfx950((int)v)) d.ids.push_back((int)v);
                p = *end == ',' ? end + 1 : end;
            }
        } else {
            const char *env = getenv("TYCHE_DEVICES");
            const int want = env ? atoi(env) : n;
            for (int i = 0; i < n && (int)d.ids.size() < want && i < kMaxDevices; i++)
                if (device_is_gfx950(i)) d.ids.push_back(i);
        }
        if (d.ids.empty()) d.why = "no gfx950 device; libtyche_codec.so carries gfx950 code only";
        return d;
    }());   // never destroyed, like the pools
    return ds;
}

// makes `dev` current on this thread after checking it (cached per device)
int tyche::ensure_device(int dev) {
    static std::atomic<int> ok[kMaxDevices];   // 0 unknown, 1 gfx950, 2 unusable
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return fail_msg("no HIP device available (the codec runs only on the GPU)");
    if (dev < 0 || dev >= n || dev >= kMaxDevices) return fail_msg("selected device out of range");
    e = hipSetDevice(dev);
    if (e != hipSuccess) return fail("hipSetDevice", e);
    if (ok[dev].load() == 0) ok[dev].store(device_is_gfx950(dev) ? 1 : 2);
    if (ok[dev].load() != 1) return fail_msg("device is not gfx950; libtyche_codec.so carries gfx950 code only");
    return TYCHE_E_OK;
}

// the device for a thread's device-side work: its pinned one, the rank's, else the first of the set
int tyche::current_device(int *dev) {
    if (t_device >= 0 || rank_device() >= 0) {
        *dev = t_device >= 0 ? t_device : rank_device();
        return TYCHE_E_OK;
    }
    const DeviceSet &ds = device_set();
    if (ds.ids.empty()) return fail_msg(ds.why);
    *dev = ds.ids[0];
    return TYCHE_E_OK;
}

// Test hook (TYCHE_FAIL_COMPRESS_EVERY=N or the knob): every Nth encode launch
// fails as a lost device would, so the callers' TYCHE_E_DEVICE handling
// (list.c:1051-1060 and the INTEGRATION.md change) can be exercised.
bool tyche::compress_launch_fails() {
    static std::atomic<unsigned long> launches{0};
    const long every = knob("FAIL_COMPRESS_EVERY", 0);
    return every > 0 && (launches.fetch_add(1) + 1) % (unsigned long)every == 0;
}

// the encoder kernel for a codec id (valid_codec)
hipError_t tyche::launch_encode(int id, const tyche_batch_t &b, uint32_t in_cap, hipStream_t s) {
    if (compress_launch_fails()) return hipErrorLaunchFailure;
    if (id == TYCHE_ZSTD_COMPRESSOR_ID) return launch_zstd_encode(b, in_cap, s);
    if (id == TYCHE_ZLIB_COMPRESSOR_ID) return launch_zlib_deflate(b, in_cap, s);
    return launch_lz4_encode(b, in_cap, s);
}

// Launches, counters and scratch of the device-resident API follow the current
// device (hipGetDevice); a stream created on another device makes that device
// current for the call (DeviceGuard puts the caller's back).
int tyche::stream_device(hipStream_t s) {
    if (!s) return TYCHE_E_OK;
    int sd = -1, cur = -1;
    if (hipStreamGetDevice(s, &sd) != hipSuccess || sd < 0) return TYCHE_E_OK;
    if (hipGetDevice(&cur) == hipSuccess && cur == sd) return TYCHE_E_OK;
    hipError_t e = hipSetDevice(sd);
    return e == hipSuccess ? TYCHE_E_OK : fail("hipSetDevice (stream's device)", e);
}

namespace {
// codecs with a gfx950 kernel (all of them have one in both directions)
bool valid_codec(int id) {
    return id == TYCHE_LZ4_COMPRESSOR_ID || id == TYCHE_ZLIB_COMPRESSOR_ID || id == TYCHE_ZSTD_COMPRESSOR_ID;
}
// The largest page a compress launch may declare (and a host page may have): TYCHE_LZ4_MAX_PAGE
// for LZ4, whose large-page encoder takes over above 65,535 bytes; 65,535 for zlib and zstd
// (16-bit positions in their parses) and for LZ4 under LZ4_EXACT=1, which promises the reference's
// byU16 bytes and is never quietly given another encoder's.  Also where an LZ4 compress call with both
// LZ4_EXACT=1 and LZ4_HC=1 is refused, before any device work.
int check_page_limit(int id, uint32_t len) {
    if (id == TYCHE_LZ4_COMPRESSOR_ID && knob("LZ4_EXACT", 0) != 0 && knob("LZ4_HC", 0) != 0) {
        t_error = "LZ4_EXACT=1 and LZ4_HC=1 contradict each other: exact mode promises LZ4_compress_default's bytes, "
                  "HC mode another parse's";
        return TYCHE_E_BAD_ARGS;
    }
    if (len <= 65535u) return TYCHE_E_OK;
    if (id == TYCHE_LZ4_COMPRESSOR_ID) {
        if (knob("LZ4_EXACT", 0) != 0) {
            t_error = "LZ4_EXACT=1 covers pages of up to 65535 bytes only (the reference's byU16 regime)";
            return TYCHE_E_BAD_ARGS;
        }
        if (len <= TYCHE_LZ4_MAX_PAGE) return TYCHE_E_OK;
        t_error = "LZ4 pages above TYCHE_LZ4_MAX_PAGE (" + std::to_string(TYCHE_LZ4_MAX_PAGE) + " bytes) are not supported";
        return TYCHE_E_BAD_ARGS;
    }
    t_error = std::string(id == TYCHE_ZSTD_COMPRESSOR_ID ? "zstd" : "zlib") + " pages above 65535 bytes are not supported";
    return TYCHE_E_BAD_ARGS;
}

std::string codec_msg(int id) {
    if (id == TYCHE_ZLIB_COMPRESSOR_ID || id == TYCHE_ZSTD_COMPRESSOR_ID)
        return "compressor id " + std::to_string(id) + " has no gfx950 kernel for this direction in this build";
    return "unknown compressor id " + std::to_string(id);
}

constexpr size_t kBulkSmallMax = 64;   // pages of up to 65,536 bytes a raw LZ4 host decode batch may hold beside larger ones

}  // namespace

extern "C" {

// ------------------------------------------------------------------ runtime
int tyche_host_profile(uint64_t *out, int n) {
    return host_profile_read(out, n);
}

int tyche_set_knob(const char *name, long value) {
    if (!name || !*name) return TYCHE_E_BAD_ARGS;
    KnobTable &T = knob_table();
    std::lock_guard<std::mutex> g(T.mu);
    T.over[name] = value;
    g_knob_gen.fetch_add(1, std::memory_order_acq_rel);
    return TYCHE_E_OK;
}

int tyche_clear_knob(const char *name) {
    if (!name || !*name) return TYCHE_E_BAD_ARGS;
    KnobTable &T = knob_table();
    std::lock_guard<std::mutex> g(T.mu);
    T.over.erase(name);
    g_knob_gen.fetch_add(1, std::memory_order_acq_rel);
    return TYCHE_E_OK;
}

int tyche_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int tyche_set_device(int device) {
    if (device < TYCHE_ALL_DEVICES) return TYCHE_E_BAD_ARGS;
    t_device = device;
    return TYCHE_E_OK;
}

int tyche_active_devices(void) {
    if (t_device >= 0 || rank_device() >= 0) return 1;
    return (int)device_set().ids.size();
}

size_t tyche_plan_split(size_t n, const uint32_t *src_lengths, int ndev, uint64_t min_part_bytes, size_t *cuts) {
    cuts[0] = 0;
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) total += src_lengths[i];
    uint64_t parts = ndev > 0 ? (uint64_t)ndev : 1u;
    if (min_part_bytes > 0) parts = std::min<uint64_t>(parts, total / min_part_bytes);
    parts = std::min<uint64_t>(std::max<uint64_t>(parts, 1u), std::max<size_t>(n, 1u));
    size_t i = 0;
    uint64_t acc = 0;
    for (uint64_t p = 1; p < parts; p++) {   // part p-1 ends where the input bytes pass p/parts of the total
        const uint64_t goal = total / parts * p + (total % parts) * p / parts;
        while (i < n && acc < goal) acc += src_lengths[i++];
        cuts[p] = i;
    }
    cuts[parts] = n;
    size_t k = 1;   // drop empty parts
    for (uint64_t p = 1; p <= parts; p++)
        if (cuts[p] > cuts[k - 1]) cuts[k++] = cuts[p];
    if (k == 1) cuts[k++] = n;   // n == 0: one empty part
    return k - 1;
}

const char *tyche_last_error(void) { return t_error.c_str(); }

int tyche_device_ready(void) {
    DeviceGuard keep;
    int dev = 0;
    int rc = current_device(&dev);
    if (rc == TYCHE_E_OK) rc = ensure_device(dev);
    return rc == TYCHE_E_OK ? 1 : 0;
}

uint32_t tyche_compress_bound(int compressor_id, uint32_t n) {
    if (compressor_id == TYCHE_LZ4_COMPRESSOR_ID) return lz4_bound(n);
    if (compressor_id == TYCHE_ZLIB_COMPRESSOR_ID) return zlib_bound(n);
    if (compressor_id == TYCHE_ZSTD_COMPRESSOR_ID) return zstd_bound(n);
    return 0;
}

// ------------------------------------------------------- device-resident API (stream_device)
int tyche_compress_batch(int compressor_id, int compressor_level, const tyche_batch_t *batch, void *stream) {
    (void)compressor_level;   // level is fixed at 1 by tyche (src/options.c:68); LZ4 has no level
    if (!batch) return TYCHE_E_BAD_ARGS;
    if (!valid_codec(compressor_id)) { t_error = codec_msg(compressor_id); return TYCHE_E_BAD_ARGS; }
    if (batch->count == 0) return TYCHE_E_OK;
    if (!batch->src || !batch->dst || !batch->results) return TYCHE_E_BAD_ARGS;
    const uint32_t in_cap = encode_in_cap(*batch);
    if (int rc = check_page_limit(compressor_id, in_cap)) return rc;
    DeviceGuard keep;
    if (int rc = stream_device((hipStream_t)stream)) return rc;
    hipError_t e = launch_encode(compressor_id, *batch, in_cap, (hipStream_t)stream);
    if (e != hipSuccess) return fail("encode launch", e);
    return TYCHE_E_OK;
}

int tyche_decompress_batch(int compressor_id, const tyche_batch_t *batch, void *stream) {
    if (!batch) return TYCHE_E_BAD_ARGS;
    if (!valid_codec(compressor_id)) { t_error = codec_msg(compressor_id); return TYCHE_E_BAD_ARGS; }
    if (batch->count == 0) return TYCHE_E_OK;
    if (!batch->src || !batch->dst || !batch->results) return TYCHE_E_BAD_ARGS;
    DeviceGuard keep;
    if (int rc = stream_device((hipStream_t)stream)) return rc;
    uint32_t out_cap = batch->dst_capacity;
    if (compressor_id == TYCHE_ZLIB_COMPRESSOR_ID) {
        hipError_t e = launch_zlib_inflate(*batch, out_cap, (hipStream_t)stream);
        if (e != hipSuccess) return fail("zlib inflate launch", e);
        return TYCHE_E_OK;
    }
    if (compressor_id == TYCHE_ZSTD_COMPRESSOR_ID) {
        hipError_t e = launch_zstd_decode(*batch, decode_in_cap(*batch, zstd_bound(out_cap)), out_cap,
                                          (hipStream_t)stream);
        if (e != hipSuccess) return fail("zstd decode launch", e);
        return TYCHE_E_OK;
    }
    // (a declared stream maximum is only a bound -- a slot width, say: above the longest stream a
    // capacity of TYCHE_LZ4_MAX_PAGE can have it is taken as that, and a page whose stream is
    // longer still gets INT32_MIN)
    const uint32_t lz4_in_cap = std::min(decode_in_cap(*batch, lz4_bound(out_cap)), lz4_bound(TYCHE_LZ4_MAX_PAGE));
    hipError_t e = launch_lz4_decode(*batch, lz4_in_cap, out_cap, (hipStream_t)stream);
    if (e != hipSuccess && out_cap > TYCHE_LZ4_MAX_PAGE)
        return fail("lz4 decode launch (capacities above TYCHE_LZ4_MAX_PAGE, 4194304 bytes, are not supported)", e);
    if (e != hipSuccess) return fail("lz4 decode launch", e);
    return TYCHE_E_OK;
}

// --------------------------------------------------------------- packed store
// the argument rules shared by tyche_pack_batch and tyche_pack_plan; 0 or TYCHE_E_BAD_ARGS with the reason
static int pack_args(const char *what, size_t count, uint32_t align, bool missing) {
    if (align == 0 || (align & (align - 1u)) != 0 || align > TYCHE_PACK_MAX_ALIGN) {
        t_error = std::string(what) + ": align must be a power of two from 1 to TYCHE_PACK_MAX_ALIGN (" +
                  std::to_string(TYCHE_PACK_MAX_ALIGN) + "), got " + std::to_string(align);
        return TYCHE_E_BAD_ARGS;
    }
    if (count > TYCHE_PACK_MAX_PAGES) {
        t_error = std::string(what) + ": count may be at most TYCHE_PACK_MAX_PAGES (" + std::to_string(TYCHE_PACK_MAX_PAGES) +
                  "), got " + std::to_string(count);
        return TYCHE_E_BAD_ARGS;
    }
    if (count > 0 && missing) {
        t_error = std::string(what) + ": a batch of " + std::to_string(count) + " pages needs " +
                  (strcmp(what, "tyche_pack_plan") == 0 ? "results and state" : "src, results, arena, state, offsets and lengths") +
                  " (one is NULL)";
        return TYCHE_E_BAD_ARGS;
    }
    return TYCHE_E_OK;
}

int tyche_pack_batch(const tyche_pack_t *p, void *stream) {
    if (!p) {
        t_error = "tyche_pack_batch: the tyche_pack_t is NULL";
        return TYCHE_E_BAD_ARGS;
    }
    if (int rc = pack_args("tyche_pack_batch", p->count, p->align,
                           !p->src || !p->results || !p->arena || !p->state || !p->offsets || !p->lengths))
        return rc;
    if (p->count == 0) return TYCHE_E_OK;
    DeviceGuard keep;
    if (keep.saved < 0) return fail_msg("no HIP device available (the codec runs only on the GPU)");
    if (int rc = stream_device((hipStream_t)stream)) return rc;
    const char *step = "";
    hipError_t e = launch_pack(*p, (hipStream_t)stream, &step);
    if (e != hipSuccess) return fail((std::string("pack (") + step + ")").c_str(), e);
    return TYCHE_E_OK;
}

uint64_t tyche_pack_plan(size_t n, const int32_t *results, uint32_t max_length, uint32_t align, uint64_t capacity,
                         uint64_t state[2], uint64_t *offsets, uint32_t *lengths) {
    if (pack_args("tyche_pack_plan", n, align, !results || !state)) return UINT64_MAX;
    if (n == 0) return state ? state[1] : 0u;
    return pack_plan_host(n, results, max_length, align, capacity, state, offsets, lengths);
}

// ----------------------------------------------------------- host batch API
int tyche_compress_host(int compressor_id, int compressor_level, size_t n, const void *const *src,
                        const uint32_t *src_lengths, void *const *dst, const uint32_t *dst_capacities,
                        int32_t *results) {
    (void)compressor_level;
    if (!valid_codec(compressor_id)) { t_error = codec_msg(compressor_id); return TYCHE_E_BAD_ARGS; }
    if (n == 0) return TYCHE_E_OK;
    uint32_t longest = 0;
    for (size_t i = 0; i < n; i++) longest = std::max(longest, src_lengths[i]);
    if (int rc = check_page_limit(compressor_id, longest)) return rc;
    // LZ4's encoders only store to their destination (never read it back), so their streams may go
    // straight into the pinned staging arena (HOST_DIRECT_OUT=0: stage through HBM and D2H instead)
    const int direct = compressor_id == TYCHE_LZ4_COMPRESSOR_ID && knob("HOST_DIRECT_OUT", 1) ? kDirectAlways : kDirectNone;
    auto plain = [compressor_id](const tyche_batch_t &b, hipStream_t s, bool) {
        return launch_encode(compressor_id, b, std::max(b.max_src_length, 1u), s);
    };
    // with a process-wide dictionary (each codec's own): the reach rule, dict_launch
    const DictCodec *dc = &dict_codec(compressor_id);
    DictHold dict;
    AutoSample trained_from;   // TYCHE_LZ4_DICT_AUTO: the sample, when this call completed it
    if (int rc = dict.get(*dc)) return rc;
    if (compressor_id == TYCHE_LZ4_COMPRESSOR_ID)
        if (int rc = lz4_host_compress_rules(dict.d, n, src, src_lengths, &trained_from)) return rc;
    if (dict.d) {
        DictUploadNote note;
        return note.finish(run_host(n, src, src_lengths, dst, dst_capacities, results,
                                    [&](const tyche_batch_t &b, hipStream_t s, bool host_dst) {
                                        return dict_launch(*dc, false, dict.d, note, b, s, host_dst, plain);
                                    }, false, direct));
    }
    const int rc = run_host(n, src, src_lengths, dst, dst_capacities, results, plain, false, direct);
    // (compressed plain like every call before the install, then trained and installed)
    if (trained_from.dict_len) auto_train_and_install(trained_from);
    return rc;
}

int tyche_decompress_host(int compressor_id, size_t n, const void *const *src, const uint32_t *src_lengths,
                          void *const *dst, const uint32_t *dst_capacities, int32_t *results) {
    if (!valid_codec(compressor_id)) { t_error = codec_msg(compressor_id); return TYCHE_E_BAD_ARGS; }
    if (n == 0) return TYCHE_E_OK;
    // with a process-wide dictionary (each codec's own): the reach rule, dict_launch
    const DictCodec &dc = dict_codec(compressor_id);
    DictHold dict;
    DictUploadNote note;
    if (int rc = dict.get(dc)) return rc;
    if (compressor_id != TYCHE_LZ4_COMPRESSOR_ID) {
        const bool zlib = compressor_id == TYCHE_ZLIB_COMPRESSOR_ID;
        auto plain = [zlib](const tyche_batch_t &b, hipStream_t s, bool) {
            return zlib ? launch_zlib_inflate(b, b.dst_capacity, s) : launch_zstd_decode(b, b.max_src_length, b.dst_capacity, s);
        };
        return note.finish(run_host(n, src, src_lengths, dst, dst_capacities, results,
                                    [&](const tyche_batch_t &b, hipStream_t s, bool host_dst) {
                                        if (!dict.d) return plain(b, s, host_dst);
                                        return dict_launch(dc, true, dict.d, note, b, s, host_dst, plain);
                                    }, true));
    }
    // A capacity above TYCHE_LZ4_MAX_PAGE is refused by the launch of the chunk that holds it, as
    // every capacity beyond the decoders' LDS used to be: TYCHE_E_DEVICE, earlier chunks drained.
    // So is, at the chunk that holds its first large page, a bulk batch that mixes classes: one that
    // holds a capacity above 65,536 bytes beside more than kBulkSmallMax pages of at most that.  It
    // depends on the batch alone, not on where the chunks are cut.  Such batches were always refused
    // this way (tests/test_host_engine.py pins it with 12,000 small pages and one 1 MiB capacity),
    // and a chunk is launched whole, so the small pages would share the one-page-per-CU decoders
    // of the large ones.  The Buffer entry points and the restore queue split the classes
    // themselves (tyche_buffers_decompress); a few small pages beside large ones pass.
    size_t n_small = 0, n_large = 0;
    for (size_t i = 0; i < n; i++) (dst_capacities[i] <= 65536u ? n_small : n_large)++;
    const bool mixed_bulk = n_large > 0 && n_small > kBulkSmallMax;
    auto plain = [](const tyche_batch_t &b, hipStream_t s, bool host_dst) {
        return launch_lz4_decode(b, b.max_src_length, b.dst_capacity, s, !host_dst);
    };
    const int rc = note.finish(run_host(n, src, src_lengths, dst, dst_capacities, results,
                                        [&](const tyche_batch_t &b, hipStream_t s, bool host_dst) {
                                            if (mixed_bulk && b.dst_capacity > 65536u) return hipErrorInvalidValue;
                                            if (!dict.d) return plain(b, s, host_dst);
                                            return dict_launch(dc, true, dict.d, note, b, s, host_dst, plain);
                                        }, true, knob("HOST_DIRECT_OUT", 1) ? kDirectLz4Decode : kDirectNone));
    if (rc == TYCHE_E_DEVICE && mixed_bulk)
        t_error += " (an LZ4 host batch with a capacity above 65536 bytes beside more than " + std::to_string(kBulkSmallMax) +
                   " pages of at most that is refused: pass the large pages in a call of their own)";
    return rc;
}

// ------------------------------------------------------- Buffer entry points
int buffer__initialize(Buffer **buf, bufferid_t id, uint32_t size, void *data, char *page_filespec) {
    // src/buffer.c:61-109
    *buf = (Buffer *)malloc(sizeof(Buffer));
    if (*buf == NULL) return TYCHE_E_NO_MEMORY;
    memset(*buf, 0, sizeof(Buffer));
    pthread_mutex_init(&(*buf)->lock, NULL);
    (*buf)->id = id;
    if (page_filespec == NULL && size == 0 && data == NULL) return TYCHE_E_OK;
    if ((page_filespec != NULL) == (size > 0 || data != NULL)) return TYCHE_E_BAD_ARGS;
    if (page_filespec == NULL) {
        (*buf)->data = data;
        (*buf)->data_length = size;
        return TYCHE_E_OK;
    }
    FILE *fh = fopen(page_filespec, "rb");
    if (fh == NULL) return TYCHE_E_GENERIC;
    fseek(fh, 0, SEEK_END);
    (*buf)->data_length = (uint32_t)ftell(fh);
    rewind(fh);
    (*buf)->data = malloc((*buf)->data_length);
    if ((*buf)->data == NULL) { fclose(fh); return TYCHE_E_NO_MEMORY; }
    if (fread((*buf)->data, (*buf)->data_length, 1, fh) == 0) { fclose(fh); return TYCHE_E_GENERIC; }
    fclose(fh);
    return TYCHE_E_OK;
}

void buffer__destroy(Buffer *buf, const bool destroy_data) {
    // src/buffer.c:116-124
    if (destroy_data) free(buf->data);
    free(buf);
}

void buffer__lock(Buffer *buf) { pthread_mutex_lock(&buf->lock); }
void buffer__unlock(Buffer *buf) { pthread_mutex_unlock(&buf->lock); }
void buffer__release_pin(Buffer *buf) { __sync_fetch_and_add(&buf->ref_count, (uint16_t)-1); }

void buffer__copy(Buffer *src, Buffer *dst, bool copy_data) {
    // src/buffer.c:287-310
    dst->id = src->id;
    dst->ref_count = src->ref_count;
    dst->popularity = src->popularity;
    dst->comp_cost = src->comp_cost;
    dst->comp_hits = src->comp_hits;
    dst->data_length = src->data_length;
    dst->comp_length = src->comp_length;
    if (copy_data) {
        size_t n = src->comp_length > 0 ? src->comp_length : src->data_length;
        free(dst->data);
        dst->data = malloc(n);
        memcpy(dst->data, src->data, n);
    }
    dst->next = NULL;
}

// Pre-codec checks of buffer__compress, src/buffer.c:161-174, in the same order.
// Returns -1 when the buffer should go to the codec.
static int compress_precheck(Buffer *buf, int compressor_id) {
    if (compressor_id == TYCHE_NO_COMPRESSOR_ID) {
        if (buf == NULL) return TYCHE_E_BUFFER_NOT_FOUND;   // the reference dereferences NULL here
        buf->comp_length = buf->data_length;
        return TYCHE_E_OK;
    }
    if (buf == NULL) return TYCHE_E_BUFFER_NOT_FOUND;
    if (buf->data == NULL || buf->data_length == 0) return TYCHE_E_BUFFER_MISSING_DATA;
    if (buf->comp_length != 0) return TYCHE_E_BUFFER_ALREADY_COMPRESSED;
    return -1;
}

// src/buffer.c:229-240
static int decompress_precheck(Buffer *buf, int compressor_id) {
    if (compressor_id == TYCHE_NO_COMPRESSOR_ID) {
        if (buf == NULL) return TYCHE_E_BUFFER_NOT_FOUND;
        buf->comp_length = 0;
        return TYCHE_E_OK;
    }
    if (buf == NULL) return TYCHE_E_BUFFER_NOT_FOUND;
    if (buf->data == NULL || buf->data_length == 0) return TYCHE_E_BUFFER_MISSING_DATA;
    if (buf->comp_length == 0) return TYCHE_E_BUFFER_ALREADY_DECOMPRESSED;
    return -1;
}

int tyche_buffers_compress(Buffer **bufs, void **compressed, int *status, size_t n, int compressor_id,
                           int compressor_level) {
    std::vector<size_t> idx;
    idx.reserve(n);
    for (size_t i = 0; i < n; i++) {
        status[i] = compress_precheck(bufs[i], compressor_id);
        if (status[i] == -1) {
            if (!valid_codec(compressor_id) && compressor_id >= 1 && compressor_id <= 3) {
                t_error = codec_msg(compressor_id);
                status[i] = TYCHE_E_BUFFER_COMPRESSION_PROBLEM;
            } else if (!valid_codec(compressor_id)) {
                status[i] = TYCHE_E_OK;   // unknown id: the reference's if-chain falls through (buffer.c:176-218)
            } else {
                idx.push_back(i);
            }
        }
    }
    if (idx.empty()) return TYCHE_E_OK;
    const size_t m = idx.size();
    std::vector<const void *> src(m);
    std::vector<void *> dst(m);
    std::vector<uint32_t> slen(m), dcap(m);
    std::vector<int32_t> res(m);
    for (size_t k = 0; k < m; k++) {
        Buffer *b = bufs[idx[k]];
        src[k] = b->data;
        slen[k] = b->data_length;
        dcap[k] = tyche_compress_bound(compressor_id, b->data_length);   // the codec's bound (buffer.c:179, 191, 204)
        dst[k] = malloc(dcap[k]);
        if (!dst[k]) {
            for (size_t j = 0; j < k; j++) free(dst[j]);
            for (size_t j = 0; j < m; j++) {
                status[idx[j]] = TYCHE_E_NO_MEMORY;
                compressed[idx[j]] = NULL;
            }
            return TYCHE_E_NO_MEMORY;
        }
    }
    uint64_t t0 = now_ns();
    int rc = tyche_compress_host(compressor_id, compressor_level, m, src.data(), slen.data(), dst.data(),
                                 dcap.data(), res.data());
    uint64_t per = (now_ns() - t0) / m;
    for (size_t k = 0; k < m; k++) {
        Buffer *b = bufs[idx[k]];
        size_t i = idx[k];
        if (rc != TYCHE_E_OK || res[k] < 1) {
            // The reference leaks its output block here (buffer.c:185-186) and leaves
            // *compressed_data pointing at it; this frees it and sets NULL, so a caller
            // that ignores the status (list.c:1050-1058 installs the pointer on any
            // status but 124) never installs memory it does not own.
            free(dst[k]);
            compressed[i] = NULL;
            status[i] = rc != TYCHE_E_OK ? TYCHE_E_DEVICE : TYCHE_E_BUFFER_COMPRESSION_PROBLEM;
            continue;
        }
        compressed[i] = dst[k];
        b->comp_length = (uint32_t)res[k];
        b->comp_cost += (uint32_t)per;
        status[i] = TYCHE_E_OK;
    }
    return rc;
}

int tyche_buffers_decompress(Buffer **bufs, int *status, size_t n, int compressor_id) {
    std::vector<size_t> idx;
    idx.reserve(n);
    for (size_t i = 0; i < n; i++) {
        status[i] = decompress_precheck(bufs[i], compressor_id);
        if (status[i] == -1) {
            if (!valid_codec(compressor_id) && compressor_id >= 1 && compressor_id <= 3) {
                t_error = codec_msg(compressor_id);
                status[i] = TYCHE_E_BUFFER_COMPRESSION_PROBLEM;
            } else if (!valid_codec(compressor_id)) {
                // unknown id: the reference swaps in an unfilled malloc(data_length) block and
                // reports success (buffer.c:244-279); mirrored, with the block zeroed.
                Buffer *b = bufs[i];
                void *fresh = calloc(1, b->data_length);
                if (!fresh) { status[i] = TYCHE_E_NO_MEMORY; continue; }
                free(b->data);
                b->data = fresh;
                b->comp_hits++;
                b->comp_length = 0;
                status[i] = TYCHE_E_OK;
            } else {
                idx.push_back(i);
            }
        }
    }
    if (idx.empty()) return TYCHE_E_OK;
    const size_t m = idx.size();
    // LZ4: the buffers of up to 65,536 bytes first, the larger ones after them, each class in a host
    // batch of its own -- the small pages keep their decoders whatever shares the call (or the
    // restore queue's batch) with them, and only the large ones take the ring decoder
    size_t n_small = m;
    if (compressor_id == TYCHE_LZ4_COMPRESSOR_ID)
        n_small = (size_t)(std::stable_partition(idx.begin(), idx.end(),
                                                 [&](size_t i) { return bufs[i]->data_length <= 65536u; }) -
                           idx.begin());
    std::vector<const void *> src(m);
    std::vector<void *> dst(m);
    std::vector<uint32_t> slen(m), dcap(m);
    std::vector<int32_t> res(m);
    for (size_t k = 0; k < m; k++) {
        Buffer *b = bufs[idx[k]];
        src[k] = b->data;
        slen[k] = b->comp_length;
        dcap[k] = b->data_length;
        dst[k] = malloc(b->data_length);                             // buffer.c:246
        if (!dst[k]) {
            for (size_t j = 0; j < k; j++) free(dst[j]);
            for (size_t j = 0; j < m; j++) status[idx[j]] = TYCHE_E_NO_MEMORY;
            return TYCHE_E_NO_MEMORY;
        }
    }
    int rc_all = TYCHE_E_OK;
    for (int cls = 0; cls < 2; cls++) {
        const size_t k0 = cls ? n_small : 0, k1 = cls ? m : n_small;
        if (k0 == k1) continue;
        uint64_t t0 = now_ns();
        int rc = tyche_decompress_host(compressor_id, k1 - k0, src.data() + k0, slen.data() + k0, dst.data() + k0,
                                       dcap.data() + k0, res.data() + k0);
        uint64_t per = (now_ns() - t0) / (k1 - k0);
        if (rc != TYCHE_E_OK && rc_all == TYCHE_E_OK) rc_all = rc;
        for (size_t k = k0; k < k1; k++) {
            Buffer *b = bufs[idx[k]];
            size_t i = idx[k];
            // LZ4 accepts any rv >= 0 (buffer.c:251-253); zlib needs Z_OK and the exact length (:257-260);
            // zstd only !ZSTD_isError (:264-266)
            const bool bad = res[k] < 0 || (compressor_id == TYCHE_ZLIB_COMPRESSOR_ID && (uint32_t)res[k] != b->data_length);
            if (rc != TYCHE_E_OK || bad) {
                free(dst[k]);                           // the reference leaks here
                status[i] = rc != TYCHE_E_OK ? TYCHE_E_DEVICE : TYCHE_E_BUFFER_COMPRESSION_PROBLEM;
                continue;
            }
            free(b->data);
            b->data = dst[k];
            b->comp_hits++;
            b->comp_length = 0;
            b->comp_cost += (uint32_t)per;
            status[i] = TYCHE_E_OK;
        }
    }
    return rc_all;
}

int buffer__compress(Buffer *buf, void **compressed_data, int compressor_id, int compressor_level) {
    int status = TYCHE_E_OK;
    tyche_buffers_compress(&buf, compressed_data, &status, 1, compressor_id, compressor_level);
    return status;
}

int buffer__decompress(Buffer *buf, int compressor_id) {
    int status = TYCHE_E_OK;
    tyche_buffers_decompress(&buf, &status, 1, compressor_id);
    return status;
}

// ---------------------------------------------------------- restore queue
// list__search restores one page per hit, synchronously, under the buffer's
// lock (src/list.c:563-589).  The queue lets those concurrent per-hit restores
// share GPU launches: a caller enqueues its Buffer and blocks; a dispatcher
// thread takes whatever is queued (up to max_batch, after waiting at most
// max_wait_us for company once the first request arrives), runs one
// tyche_buffers_decompress over the batch, and wakes each caller with its
// buffer__decompress status.  Per-buffer semantics are unchanged.
//
// Each codec has its own queue and dispatchers (TYCHE_RESTORE_DISPATCHERS per
// codec, default two per device): a batch's latency is that of its slowest
// page (~0.04 ms for a 16 KiB LZ4 page on the single-page decoder, ~0.3 ms for
// zlib, tools/latency.c), so LZ4 restores never wait behind a zlib batch, and a
// second dispatcher collects the next batch while one runs: 2.53 vs 2.06 GiB/s of
// tools/cycle.c restores (round 5, r05_restore_dispatch.log; with the jump
// decoder and a shared wake-up round 2 had measured 1.70 vs 1.32 on one box and
// 1.12-1.24 vs 1.32-1.36 on another, r02_restore_dispatch.jsonl); 3-4 per codec
// oversubscribed the hardware queues then.
namespace {
constexpr int kQueueHistBuckets = 11;
// A restorer waits on its own request word (spin briefly, then futex), so a finished batch wakes
// exactly its callers -- a shared condition variable woke every blocked restorer (64 in the C5
// cycle) to re-take the queue mutex and find its request still pending.
// A request lives on its caller's stack; the futex word it is woken through does not: it is the
// caller's thread_local word (reset on entry), so the FUTEX_WAKE that follows the store -- which
// the waiter may already have seen and returned on -- still lands on a live word of that thread,
// never on a reused stack frame.  A wake that finds no waiter is a no-op, and every
// waiter re-checks its word in a loop, so a late wake is harmless.
struct RestoreReq {
    Buffer *buf;
    int status;
    std::atomic<int> *done;
    void wait() {
        for (int i = 0; i < 64; i++) {   // (a batch takes ~0.1 ms: spinning longer only takes CPU from the others)
            if (done->load(std::memory_order_acquire)) return;
            _mm_pause();
        }
        while (!done->load(std::memory_order_acquire))
            syscall(SYS_futex, (int *)done, FUTEX_WAIT_PRIVATE, 0, nullptr, nullptr, 0);
    }
    void wake() {
        std::atomic<int> *w = done;   // read before the store: the request may be gone after it
        w->store(1, std::memory_order_release);
        syscall(SYS_futex, (int *)w, FUTEX_WAKE_PRIVATE, 1, nullptr, nullptr, 0);
    }
};
thread_local std::atomic<int> t_restore_word{0};
struct RestoreQueue {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<RestoreReq *> q[4];   // by codec id (NO is restored by the caller)
    bool collecting[4] = {false, false, false, false};
    bool running = false, stop = false;
    int max_batch = 1024, max_wait_us = 50, device = -1;
    uint64_t batches = 0, buffers = 0;
    uint64_t hist[kQueueHistBuckets] = {};   // launches by batch size (power-of-two buckets)
    std::vector<std::thread> th;
    void loop(int codec) {
        (void)tyche_set_device(device);
        std::vector<RestoreReq *> take;
        std::vector<Buffer *> bufs;
        std::vector<int> st;
        std::vector<RestoreReq *> &cq = q[codec];
        // TYCHE_RESTORE_WAIT_IDLE (default 1): the wait for company applies only when this
        // dispatcher found its queue empty -- requests that queued up while its last batch ran
        // have waited a whole batch already and go out at once (0: every batch waits)
        const bool wait_idle_only = knob("RESTORE_WAIT_IDLE", 1) != 0;
        bool idle = true;
        for (;;) {
            {
                std::unique_lock<std::mutex> g(mu);
                if (cq.empty()) idle = true;
                cv.wait(g, [&] { return (stop && cq.empty()) || (!cq.empty() && !collecting[codec]); });
                if (cq.empty()) return;   // stopping
                collecting[codec] = true;
                if ((idle || !wait_idle_only) && (int)cq.size() < max_batch && max_wait_us > 0)
                    cv.wait_for(g, std::chrono::microseconds(max_wait_us),
                                [&] { return stop || (int)cq.size() >= max_batch; });
                const size_t k = std::min(cq.size(), (size_t)max_batch);
                take.assign(cq.begin(), cq.begin() + k);
                cq.erase(cq.begin(), cq.begin() + k);
                collecting[codec] = false;
            }
            cv.notify_all();   // the next dispatcher of this codec may collect
            bufs.resize(take.size());
            st.resize(take.size());
            for (size_t i = 0; i < take.size(); i++) bufs[i] = take[i]->buf;
            tyche_buffers_decompress(bufs.data(), st.data(), bufs.size(), codec);
            {
                std::lock_guard<std::mutex> g(mu);
                batches++;
                buffers += take.size();
                hist[std::min(kQueueHistBuckets - 1, 31 - __builtin_clz((unsigned)take.size()))]++;
                idle = cq.empty();
            }
            for (size_t i = 0; i < take.size(); i++) {
                take[i]->status = st[i];
                take[i]->wake();   // (the request lives on its caller's stack: not touched after this)
            }
        }
    }
};
// never destroyed: a process may exit without tyche_restore_queue_stop (the reference app's
// list__destroy can hang before it gets there), and destroying joinable dispatcher threads (or the
// mutex they wait on) at exit would abort the process in std::terminate
RestoreQueue &g_rq = *new RestoreQueue;
}  // namespace

int tyche_restore_queue_start(int max_batch, int max_wait_us) {
    std::lock_guard<std::mutex> g(g_rq.mu);
    if (g_rq.running) return TYCHE_E_OK;
    g_rq.max_batch = max_batch > 0 ? max_batch : 1024;
    g_rq.max_wait_us = max_wait_us >= 0 ? max_wait_us : 50;
    g_rq.device = t_device;
    g_rq.stop = false;
    for (bool &c : g_rq.collecting) c = false;
    g_rq.running = true;
    int k = (int)knob("RESTORE_DISPATCHERS", 2 * std::max(1, tyche_active_devices()));
    k = std::max(1, std::min(k, 64));
    for (int codec = 1; codec <= 3; codec++)
        for (int i = 0; i < k; i++) g_rq.th.emplace_back([codec] { g_rq.loop(codec); });
    return TYCHE_E_OK;
}

void tyche_restore_queue_stop(void) {
    {
        std::lock_guard<std::mutex> g(g_rq.mu);
        if (!g_rq.running) return;
        g_rq.stop = true;
    }
    g_rq.cv.notify_all();
    for (auto &t : g_rq.th) t.join();
    std::lock_guard<std::mutex> g(g_rq.mu);
    g_rq.th.clear();
    g_rq.running = false;
}

int tyche_buffer_restore(Buffer *buf, int compressor_id) {
    // NO and unknown ids need no GPU batch: the direct path gives the reference's answer
    if (compressor_id < 1 || compressor_id > 3) return buffer__decompress(buf, compressor_id);
    RestoreReq r;
    r.buf = buf;
    r.status = TYCHE_E_OK;
    t_restore_word.store(0, std::memory_order_relaxed);
    r.done = &t_restore_word;
    {
        std::unique_lock<std::mutex> g(g_rq.mu);
        if (!g_rq.running || g_rq.stop) {
            g.unlock();
            return buffer__decompress(buf, compressor_id);   // no queue: the direct path
        }
        g_rq.q[compressor_id].push_back(&r);
    }
    g_rq.cv.notify_all();   // the collecting dispatcher, whichever it is
    r.wait();
    return r.status;
}

void tyche_restore_queue_stats(uint64_t *batches, uint64_t *buffers) {
    std::lock_guard<std::mutex> g(g_rq.mu);
    if (batches) *batches = g_rq.batches;
    if (buffers) *buffers = g_rq.buffers;
}

int tyche_restore_queue_hist(uint64_t *counts, int n) {
    if (!counts || n <= 0) return 0;
    std::lock_guard<std::mutex> g(g_rq.mu);
    const int k = std::min(n, kQueueHistBuckets);
    for (int i = 0; i < k; i++) counts[i] = g_rq.hist[i];
    return k;
}

// ---------------------------------------------------------- synthetic input
int tyche_pagegen(void *dst, uint64_t stride, uint32_t page_len, uint64_t seed, uint64_t first, size_t count,
                  uint32_t dist, void *stream) {
    // device-resident like the batch API: runs on the caller's current device
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail_msg("no HIP device available (the codec runs only on the GPU)");
    int rc = ensure_device(dev);
    if (rc) return rc;
    hipError_t e = launch_pagegen(dst, stride, page_len, seed, first, count, dist, (hipStream_t)stream);
    if (e != hipSuccess) return fail("pagegen launch", e);
    return TYCHE_E_OK;
}

}  // extern "C"
