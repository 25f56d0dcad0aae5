// host_batch.hip -- the host batch pipeline behind every entry point that starts and ends in host
// memory (engine.hip: tyche_compress_host / tyche_decompress_host, the Buffer API, the restore
// queue): staging contexts, the copy pool, and run_host, which moves a batch through a launch
// chunk by chunk.  The chunk plan and the page-table layout are host_chunk_core.h's.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "engine.h"
#include "host_batch.h"
#include "host_chunk_core.h"

#include <immintrin.h>

using namespace tyche;

namespace {

// Diagnostic builds only (-DTYCHE_PROFILE, libtyche_codec_prof.so): TYCHE_HOST_DIAG bit 0 makes the
// host batch report the results without copying the page bytes out (prices the scatter copies).  The
// product library has no such switch, so a stray setting can never report success without the data
// (ADVICE r05).
bool host_diag_no_copy() {
#ifdef TYCHE_PROFILE
    return (tyche::knob("HOST_DIAG", 0) & 1) != 0;
#else
    return false;
#endif
}

// ---------------------------------------------------------------- host batches
// The Buffer API and the host batch entry points start and end in host memory
// (tyche's Buffer->data is malloc'd, src/buffer.c:181, 246).  A batch is cut
// into chunks of ~kChunkBytes of input that flow through a ring of kSlots
// staging slots, one HIP stream each:
//
//   host gather (thread pool memcpy into pinned) -> H2D -> kernel -> D2H -> host scatter
//
// so chunk c's gather overlaps chunk c-1's copies and kernel and chunk c-2's
// scatter; the two copy directions and the kernels of different slots run
// concurrently.  tyche calls the codec from its compressor pool and its
// worker threads at once (src/list.c:1051, 572; opts.cpu_count threads,
// src/options.c:64): the staging contexts are therefore a small per-device pool
// (TYCHE_HOST_CONTEXTS, default kContextsPerDevice) that a call borrows for its
// duration, not one per calling thread, so streams and pinned arenas stay
// bounded however many threads call in.
struct Arena {
    void *p = nullptr;
    void *dp = nullptr;   // host arenas: the device's address of the pinned buffer (zero-copy launches)
    size_t cap = 0;
    bool host = false;
    int grow(size_t need) {
        if (need <= cap) return TYCHE_E_OK;
        size_t n = std::max(need, cap * 2);
        n = (n + 4095) & ~size_t(4095);
        release();
        hipError_t e = host ? hipHostMalloc(&p, n, hipHostMallocDefault) : hipMalloc(&p, n);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(host ? "hipHostMalloc" : "hipMalloc", e);
        }
        if (host && hipHostGetDevicePointer(&dp, p, 0) != hipSuccess) dp = nullptr;
        cap = n;
        return TYCHE_E_OK;
    }
    void release() {
        if (p) {
            if (host) (void)hipHostFree(p); else (void)hipFree(p);
        }
        p = dp = nullptr;
        cap = 0;
    }
};

constexpr size_t kChunkBytes = size_t(32) << 20;
constexpr int kContextsPerDevice = 8;

struct Slot {
    hipStream_t stream = nullptr;
    Arena h_in, h_out, h_meta, d_in, d_out, d_meta;
    size_t first = 0, count = 0;   // pages of the chunk in flight
    bool busy = false;
    Slot() { h_in.host = h_out.host = h_meta.host = true; }
};

struct HostCtx {
    Slot slot[kSlots];
    int group = 0;   // hardware-queue group of slot 0's stream (see acquire_ctx)
    // waits for whatever the slots still hold and forgets it (error paths)
    void abandon() {
        for (Slot &s : slot)
            if (s.busy) {
                (void)hipStreamSynchronize(s.stream);
                s.busy = false;
            }
    }
};

struct CtxPool {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<HostCtx *> all, idle;
    std::vector<int> busy;   // leased contexts per hardware-queue group
};
CtxPool *const g_ctx = new CtxPool[kMaxDevices];   // never destroyed (restore dispatchers may run at exit)

// HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default), in
// creation order; kernels of streams that share a queue run one after the
// other (tools/probes/hwq.hip: with 24 streams, stream 0 overlaps streams
// 1-6 but serializes with 7, 11, 15, ...).  Two restore batches (an LZ4 and a
// zlib one, say) on contexts whose streams share a queue therefore wait for
// each other.  So a device's contexts are created together, their streams in
// an order that puts slot s of context i in group (i + s) mod Q -- the four
// slots of one context on four queues, for the chunk pipeline -- and a call
// borrows the idle context whose group has the fewest calls running.
int hw_queues() {
    static const int q = [] {
        const char *env = getenv("GPU_MAX_HW_QUEUES");
        const int v = env ? atoi(env) : 4;
        return v > 0 ? v : 4;
    }();
    return q;
}

int context_cap() {
    static const int cap = [] {
        const char *env = getenv("TYCHE_HOST_CONTEXTS");
        const int v = env ? atoi(env) : kContextsPerDevice;
        return v > 0 ? v : kContextsPerDevice;
    }();
    return cap;
}

// creates the device's contexts (under P.mu): stream k created goes to queue
// group k mod Q, and is given to the (context, slot) pair of that group
int create_contexts(CtxPool &P) {
    const int n = context_cap(), Q = hw_queues();
    std::vector<HostCtx *> cs;
    for (int i = 0; i < n; i++) {
        cs.push_back(new HostCtx);
        cs.back()->group = i % Q;
    }
    std::vector<bool> made((size_t)n * kSlots, false);
    for (int k = 0; k < n * kSlots; k++) {
        int pick = -1;
        for (int j = 0; j < n * kSlots && pick < 0; j++)
            if (!made[j] && ((j / kSlots) + (j % kSlots)) % Q == k % Q) pick = j;
        for (int j = 0; j < n * kSlots && pick < 0; j++)
            if (!made[j]) pick = j;
        made[pick] = true;
        hipError_t e = hipStreamCreateWithFlags(&cs[pick / kSlots]->slot[pick % kSlots].stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            for (HostCtx *c : cs) {
                for (Slot &t : c->slot)
                    if (t.stream) (void)hipStreamDestroy(t.stream);
                delete c;
            }
            return fail("hipStreamCreate", e);
        }
    }
    P.all = cs;
    P.idle = cs;
    P.busy.assign((size_t)Q, 0);
    return TYCHE_E_OK;
}

// borrows a staging context of device dev (current on this thread); waits while all are busy
int acquire_ctx(int dev, HostCtx **out) {
    CtxPool &P = g_ctx[dev];
    std::unique_lock<std::mutex> g(P.mu);
    if (P.all.empty()) {
        const int rc = create_contexts(P);
        if (rc) return rc;
    }
    P.cv.wait(g, [&] { return !P.idle.empty(); });
    // least-busy group; among equals the most recently released context (its
    // pinned and device arenas are already grown -- a fresh context pays
    // hipHostMalloc/hipMalloc for its staging slots on first use)
    size_t best = P.idle.size() - 1;
    for (size_t k = best; k-- > 0;)
        if (P.busy[(size_t)P.idle[k]->group] < P.busy[(size_t)P.idle[best]->group]) best = k;
    *out = P.idle[best];
    P.idle.erase(P.idle.begin() + (long)best);
    P.busy[(size_t)(*out)->group]++;
    return TYCHE_E_OK;
}
void release_ctx(int dev, HostCtx *c) {
    CtxPool &P = g_ctx[dev];
    {
        std::lock_guard<std::mutex> g(P.mu);
        P.busy[(size_t)c->group]--;
        P.idle.push_back(c);
    }
    P.cv.notify_one();
}

// A call's hold on a staging context.  Whatever its slots still hold when the call returns (a failed
// call's chunks in flight) is waited for before the context goes back to the pool, so a later call
// never scatters a failed call's chunk; a call that succeeded left no slot busy.
struct CtxLease {
    int dev;
    HostCtx *c = nullptr;
    explicit CtxLease(int d) : dev(d) {}
    int acquire() { return acquire_ctx(dev, &c); }
    ~CtxLease() {
        if (!c) return;
        c->abandon();
        release_ctx(dev, c);
    }
    CtxLease(const CtxLease &) = delete;
    CtxLease &operator=(const CtxLease &) = delete;
};

// Page copies between malloc'd Buffers and the pinned staging arenas.  The host
// path is bound by these copies (r03 stage clocks: gather + scatter ~10 of the
// 15 ms of a 32K-page decompress call), and a plain memcpy of a 16 KiB page
// reads its destination's lines before writing them (read-for-ownership): three
// DRAM transfers per byte.  Non-temporal 16-byte stores skip that read; the
// caller of a pool job fences once at its end (copy_fence) before handing the
// arena to a DMA or the caller.
inline void copy_nt(void *dst, const void *src, size_t n) {
    if (n < 512 || ((uintptr_t)dst & 15u)) {
        memcpy(dst, src, n);
        return;
    }
    __m128i *d = (__m128i *)dst;
    const __m128i *p = (const __m128i *)src;
    size_t k = n >> 6;
    for (; k; k--, d += 4, p += 4) {
        const __m128i a = _mm_loadu_si128(p), b = _mm_loadu_si128(p + 1), c = _mm_loadu_si128(p + 2),
                      e = _mm_loadu_si128(p + 3);
        _mm_stream_si128(d, a);
        _mm_stream_si128(d + 1, b);
        _mm_stream_si128(d + 2, c);
        _mm_stream_si128(d + 3, e);
    }
    const size_t done = n & ~(size_t)63;
    if (done < n) memcpy((uint8_t *)dst + done, (const uint8_t *)src + done, n - done);
}
inline void copy_fence() { _mm_sfence(); }

// A persistent worker pool for the host-side page copies (memcpy of scattered
// malloc'd pages into and out of pinned staging).  Several callers (one per
// device of a fanned-out batch, concurrent tyche threads) may run jobs at once:
// each caller works on its own job and idle workers join whichever job still
// has ranges left.
class CopyPool {
  public:
    static CopyPool &get() {
        // never destroyed: its detached workers wait on its condition variable until exit
        static CopyPool *p = new CopyPool;
        return *p;
    }
    // runs f(i) for i in [0, n), in contiguous ranges, on the pool and the caller
    template <typename F>
    void run(size_t n, F f) {
        if (n < 64 || workers_.empty()) {
            for (size_t i = 0; i < n; i++) f(i);
            copy_fence();
            return;
        }
        std::function<void(size_t, size_t)> body = [&f](size_t a, size_t b) {
            for (size_t i = a; i < b; i++) f(i);
            copy_fence();   // the job's non-temporal stores are globally visible before it completes
        };
        Job j;
        j.body = &body;
        j.n = n;
        {
            std::lock_guard<std::mutex> g(mu_);
            jobs_.push_back(&j);
        }
        cv_.notify_all();
        work(j);
        std::unique_lock<std::mutex> g(mu_);
        jobs_.erase(std::find(jobs_.begin(), jobs_.end(), &j));   // no worker joins it from now on
        done_cv_.wait(g, [&] { return j.active == 0; });
    }

  private:
    static constexpr size_t kGrain = 32;
    struct Job {
        const std::function<void(size_t, size_t)> *body = nullptr;
        size_t n = 0;
        std::atomic<size_t> next{0};
        int active = 0;   // workers inside work(); guarded by mu_
    };
    CopyPool() {
        unsigned t = std::thread::hardware_concurrency();
        const char *env = getenv("TYCHE_HOST_THREADS");
        unsigned want = env ? (unsigned)atoi(env) : std::min(16u, t ? t : 1u);
        for (unsigned i = 1; i < want; i++) workers_.emplace_back([this] { loop(); });
        for (auto &w : workers_) w.detach();
    }
    static void work(Job &j) {
        for (;;) {
            const size_t a = j.next.fetch_add(kGrain);
            if (a >= j.n) break;
            (*j.body)(a, std::min(j.n, a + kGrain));
        }
    }
    Job *open_job() {   // under mu_
        for (Job *j : jobs_)
            if (j->next.load() < j->n) return j;
        return nullptr;
    }
    void loop() {
        for (;;) {
            Job *j = nullptr;
            {
                // j->next advances outside the lock (callers and workers claim ranges with
                // fetch_add): pick the job once, in the predicate, and pin it there
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [&] { return (j = open_job()) != nullptr; });
                j->active++;
            }
            work(*j);
            {
                std::lock_guard<std::mutex> g(mu_);
                j->active--;
            }
            done_cv_.notify_all();
        }
    }
    std::vector<std::thread> workers_;
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    std::vector<Job *> jobs_;
};

std::atomic<int> g_inflight[kMaxDevices];   // host batches running per device

// Host-path stage clocks (diagnostics, tyche_host_profile): ns spent by calling threads waiting for a
// slot's stream, scattering results, gathering inputs, and enqueuing copies and kernels; bytes gathered
// and scattered.
enum { kHpWait, kHpScatter, kHpGather, kHpEnqueue, kHpGatherBytes, kHpScatterBytes, kHpChunks, kHpCount };
std::atomic<uint64_t> g_hprof[kHpCount];
struct HpClock {
    int slot;
    uint64_t t0;
    explicit HpClock(int s) : slot(s), t0(now_ns()) {}
    ~HpClock() { g_hprof[slot] += now_ns() - t0; }
};

// Zero-copy limit: a decompress batch of at most this many bytes (input plus
// output capacity) skips the device staging buffers -- the kernel reads the
// gathered streams and the page table from the pinned host arenas and writes
// results and pages straight back into them.  No H2D/D2H copies (two
// hipMemcpyAsync calls and two copy kernels each way saved on the restore
// path's small batches); the kernels stage their input in LDS with 16-byte
// loads and write whole 16-byte vectors, which PCIe carries well.
// TYCHE_ZERO_COPY_BYTES=0 turns it off.
size_t zero_copy_bytes() { return (size_t)std::max(0L, knob("ZERO_COPY_BYTES", 4L << 20)); }

// the pages of one run_host_batch call
struct HostPages {
    const void *const *src;
    const uint32_t *src_len;
    void *const *dst;
    const uint32_t *dst_cap;
    int32_t *results;
};

// The addresses a chunk's batch is built against: the slot's device arenas, or the device's
// addresses of its pinned ones.
struct ChunkBases {
    void *meta, *in, *out;
};

// Lays chunk ch out in slot S's pinned meta arena, gathers its sources into the pinned input arena
// (already grown) on the copy pool, and returns the batch a kernel at `at` sees.  counted: the
// gathered bytes go on the stage clocks.
tyche_batch_t stage_chunk(Slot &S, const HostChunk &ch, const HostPages &pg, const ChunkBases &at, bool counted) {
    const size_t k = ch.count;
    const ChunkMeta m = meta_fill(S.h_meta.p, k, pg.src_len + ch.first, pg.dst_cap + ch.first);
    uint8_t *hin = (uint8_t *)S.h_in.p;
    const void *const *src = pg.src + ch.first;
    {
        HpClock hc(kHpGather);
        CopyPool::get().run(k, [&](size_t j) {
            if (m.slen[j]) copy_nt(hin + m.soff[j], src[j], m.slen[j]);
        });
        if (counted) g_hprof[kHpGatherBytes] += ch.in_bytes;
    }
    S.first = ch.first;
    S.count = k;
    const ChunkMeta d = meta_at(at.meta, k);
    tyche_batch_t b{};
    b.count = k;
    b.src = at.in;
    b.src_offsets = d.soff;
    b.src_lengths = d.slen;
    b.max_src_length = ch.max_in;
    b.dst = at.out;
    b.dst_offsets = d.doff;
    b.dst_capacities = d.dcap;
    b.dst_capacity = ch.max_out;
    b.results = d.res;
    return b;
}

// Completes the chunk slot S holds: waits for its stream, then copies results and page bytes out on
// the copy pool.  counted: the scattered bytes and the chunk go on the stage clocks, and the profile
// build's HOST_DIAG switch applies (the zero-copy call passes false).
int scatter_chunk(Slot &S, const HostPages &pg, bool counted) {
    {
        HpClock hc(kHpWait);
        const hipError_t e = hipStreamSynchronize(S.stream);
        if (e != hipSuccess) return fail("hipStreamSynchronize", e);
    }
    HpClock hc(kHpScatter);
    const size_t k = S.count;
    const ChunkMeta m = meta_at(S.h_meta.p, k);
    const uint8_t *hout = (const uint8_t *)S.h_out.p;
    int32_t *results = pg.results + S.first;
    void *const *dst = pg.dst + S.first;
    const uint32_t *dst_cap = pg.dst_cap + S.first;
    std::atomic<uint64_t> moved{0};
    const bool no_copy = counted && host_diag_no_copy();
    CopyPool::get().run(k, [&](size_t j) {
        const int32_t r = m.res[j];
        results[j] = r;
        if (r > 0 && (uint32_t)r <= dst_cap[j] && !no_copy) {
            copy_nt(dst[j], hout + m.doff[j], (size_t)r);
            if (counted) moved.fetch_add((uint64_t)r, std::memory_order_relaxed);
        }
    });
    if (counted) {
        g_hprof[kHpScatterBytes] += moved.load();
        g_hprof[kHpChunks]++;
    }
    return TYCHE_E_OK;
}

// Finishes the chunks of one call, slot by slot in issue order.  With helpers (async finishing,
// round 3: with three or more chunks a helper thread waits for each slot's stream and scatters its
// results while the caller gathers and enqueues the next chunk -- the r03 stage clocks had the
// caller waiting on streams ~25 % of a call, between its copies) the slots queue up for the helper
// threads, and a slot is reused only after a helper has scattered it (busy false, under mu_).
// Without, the caller scatters a slot's previous chunk itself when it comes round to the slot again.
// HOST_FINISHERS helpers (default 1), each taking the next queued slot (chunks go to disjoint
// destinations, so their scatters may run in any order, on the shared copy pool).  Round 5: a
// second and third helper, so that one chunk's scatter overlaps the next one's wait, did not
// move decompress (32K pages, best of 5 interleaved: 34.2 / 33.7 / 31.7 GiB/s for 1 / 2 / 3,
// profiles/r05_host_probe.jsonl).
// The destructor lets the helpers finish what is queued, then stops and joins them: declared after
// the context lease, it runs before the lease drains the slots.
class Finisher {
  public:
    Finisher(HostCtx &c, const HostPages &pg, int helpers) : c_(c), pg_(pg), async_(helpers > 0) {
        for (int h = 0; h < helpers; h++) th_.emplace_back([this] { help(); });
    }
    ~Finisher() { stop(); }
    Finisher(const Finisher &) = delete;
    Finisher &operator=(const Finisher &) = delete;

    // returns once slot si's previous chunk has been scattered, or with the first failure
    int reserve(int si) {
        Slot &S = c_.slot[si];
        if (!async_) {
            if (!S.busy) return TYCHE_E_OK;
            S.busy = false;
            return scatter_chunk(S, pg_, true);
        }
        {
            std::unique_lock<std::mutex> g(mu_);
            cv_.wait(g, [&] { return !S.busy || rc_ != TYCHE_E_OK; });
            if (rc_ == TYCHE_E_OK) return TYCHE_E_OK;
        }
        return finish(0);
    }
    // from its first enqueued copy on, the slot must be drained on failure
    void mark_busy(int si) {
        std::lock_guard<std::mutex> g(mu_);
        c_.slot[si].busy = true;
    }
    // the slot's chunk is enqueued whole
    void submit(int si) {
        if (!async_) return;
        std::lock_guard<std::mutex> g(mu_);
        q_.push_back(si);
        cv_.notify_all();
    }
    // completes every chunk still in flight, next_si being the oldest slot; the call's result
    int finish(int next_si) {
        if (async_) {   // the helpers drain the queue, then stop
            stop();
            if (rc_ != TYCHE_E_OK) set_thread_error(err_);   // the helper's message, for the caller
            return rc_;
        }
        for (int j = 0; j < kSlots; j++)
            if (const int rc = reserve((next_si + j) % kSlots)) return rc;
        return TYCHE_E_OK;
    }

  private:
    void stop() {
        if (th_.empty()) return;
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
        th_.clear();
    }
    void help() {   // helper thread: sync, scatter, then free the slot
        for (;;) {
            int idx;
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [&] { return !q_.empty() || stop_ || rc_ != TYCHE_E_OK; });
                if (q_.empty() || rc_ != TYCHE_E_OK) return;
                idx = q_.front();
                q_.erase(q_.begin());
            }
            const int r = scatter_chunk(c_.slot[idx], pg_, true);
            std::lock_guard<std::mutex> g(mu_);
            if (r) {
                if (rc_ == TYCHE_E_OK) {
                    rc_ = r;
                    err_ = thread_error();   // the helper's thread-local message
                }
                cv_.notify_all();
                return;
            }
            c_.slot[idx].busy = false;
            cv_.notify_all();
        }
    }
    HostCtx &c_;
    const HostPages &pg_;
    const bool async_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<int> q_;   // slots to finish, in issue order
    bool stop_ = false;
    int rc_ = TYCHE_E_OK;   // the first failure and its message
    std::string err_;
    std::vector<std::thread> th_;
};

// Moves n host pages through `launch` on device dev, chunk by chunk (see
// above).  results[i] gets the kernel's per-page result; for results in
// (0, dst_cap[i]] that many output bytes land in dst[i].  On any failure the
// context's slots are drained before it goes back to the pool, so a later call
// never scatters a failed call's chunk.
int run_host_batch(int dev, size_t n, const HostPages &pg, LaunchRef launch, bool zc_ok, int direct_out) {
    DeviceGuard keep;   // the caller's device is current again on every return
    int rc = ensure_device(dev);
    if (rc) return rc;
    struct Inflight {
        int d;
        explicit Inflight(int dd) : d(dd) { g_inflight[d]++; }
        ~Inflight() { g_inflight[d]--; }
    } inflight(dev);
    CtxLease lease(dev);
    if ((rc = lease.acquire())) return rc;
    HostCtx &c = *lease.c;
    hipError_t e;
    ChunkCutter cut(n, pg.src_len, pg.dst_cap, host_chunk_bytes(knob("HOST_CHUNK_MB", (long)(kChunkBytes >> 20))),
                    knob("HOST_RAMP", 1) != 0);

    if (zc_ok && cut.whole().in_bytes + cut.whole().out_bytes <= zero_copy_bytes()) {
        const HostChunk &ch = cut.whole();
        Slot &S = c.slot[0];
        if ((rc = S.h_in.grow(ch.in_bytes + 16)) || (rc = S.h_out.grow(ch.out_bytes + 16)) ||
            (rc = S.h_meta.grow(meta_bytes(n))))
            return rc;
        if (S.h_in.dp && S.h_out.dp && S.h_meta.dp) {
            const tyche_batch_t b = stage_chunk(S, ch, pg, ChunkBases{S.h_meta.dp, S.h_in.dp, S.h_out.dp}, false);
            S.busy = true;
            {
                HpClock hc(kHpEnqueue);
                if ((e = launch(b, S.stream, true)) != hipSuccess) return fail("kernel launch", e);
            }
            S.busy = false;
            return scatter_chunk(S, pg, false);
        }
    }

    const bool async = cut.pipelined() && knob("HOST_ASYNC_SCATTER", 1) != 0;
    Finisher fin(c, pg, async ? (int)std::min(4L, std::max(1L, knob("HOST_FINISHERS", 1))) : 0);
    HostChunk ch;
    int si = 0;
    for (; cut.next(&ch); si = (si + 1) % kSlots) {
        const size_t k = ch.count;
        Slot &S = c.slot[si];
        if ((rc = fin.reserve(si))) return rc;   // the slot's previous chunk
        if ((rc = S.h_in.grow(ch.in_bytes + 16)) || (rc = S.h_out.grow(ch.out_bytes + 16)) ||
            (rc = S.h_meta.grow(meta_bytes(k))) || (rc = S.d_in.grow(ch.in_bytes + 16)) ||
            (rc = S.d_out.grow(ch.out_bytes + 16)) || (rc = S.d_meta.grow(meta_bytes(k))))
            return rc;
        // direct_out: the kernel writes its results straight into the pinned arena over PCIe, as
        // posted writes that overlap its own work, and no D2H of the arena follows.  LZ4 compress
        // (kDirectAlways): only the compressed bytes cross the link -- a D2H of the arena would move
        // every page's full capacity (16 KiB+ per 16 KiB page at ratio 2.6).  LZ4 decompress
        // (kDirectLz4Decode): the jump and wave decoders write each page once, whole, from LDS; the
        // lane decoder (chunks of >= kLaneMin pages) reads its own output back, so it keeps the D2H;
        // TYCHE_HOST_DIRECT_DECODE_MAX: chunks of more pages than this stage through HBM too.  The
        // choice is made once here and handed to the launch (host_dst), so a knob changed meanwhile
        // cannot put the lane decoder on a host destination.
        const bool direct = S.h_out.dp != nullptr &&
                            (direct_out == kDirectAlways ||
                             (direct_out == kDirectLz4Decode && !lz4_lane_decode_wanted(k, ch.max_in, ch.max_out) &&
                              (long)k <= knob("HOST_DIRECT_DECODE_MAX", 1L << 30)));
        const tyche_batch_t b =
            stage_chunk(S, ch, pg, ChunkBases{S.d_meta.p, S.d_in.p, direct ? S.h_out.dp : S.d_out.p}, true);
        HpClock enq(kHpEnqueue);
        // ---- H2D -> kernel -> D2H on the slot's stream
        fin.mark_busy(si);
        if ((e = hipMemcpyAsync(S.d_meta.p, S.h_meta.p, meta_head_bytes(k), hipMemcpyHostToDevice, S.stream)) != hipSuccess)
            return fail("hipMemcpyAsync(meta)", e);
        if (ch.in_bytes &&
            (e = hipMemcpyAsync(S.d_in.p, S.h_in.p, ch.in_bytes, hipMemcpyHostToDevice, S.stream)) != hipSuccess)
            return fail("hipMemcpyAsync(in)", e);
        if ((e = launch(b, S.stream, direct)) != hipSuccess) return fail("kernel launch", e);
        if ((e = hipMemcpyAsync(meta_at(S.h_meta.p, k).res, b.results, k * 4, hipMemcpyDeviceToHost, S.stream)) != hipSuccess)
            return fail("hipMemcpyAsync(results)", e);
        if (ch.out_bytes && !direct &&
            (e = hipMemcpyAsync(S.h_out.p, S.d_out.p, ch.out_bytes, hipMemcpyDeviceToHost, S.stream)) != hipSuccess)
            return fail("hipMemcpyAsync(out)", e);
        fin.submit(si);
    }
    return fin.finish(si);   // in issue order: si is the oldest slot
}

// minimum input bytes per device before a host batch is split across devices
uint64_t fanout_min_bytes() { return (uint64_t)std::max(0L, knob("FANOUT_MIN_BYTES", 64L << 20)); }

// the device with the fewest host batches in flight (ties rotate)
int pick_device(const std::vector<int> &ids) {
    static std::atomic<unsigned> rot{0};
    const unsigned r = rot++;
    int best = ids[r % ids.size()];
    for (size_t k = 0; k < ids.size(); k++) {
        const int d = ids[(r + k) % ids.size()];
        if (g_inflight[d].load() < g_inflight[best].load()) best = d;
    }
    return best;
}

}  // namespace

int tyche::host_profile_read(uint64_t *out, int n) {
    const int k = std::min(n, (int)kHpCount);
    for (int i = 0; i < k; i++) out[i] = g_hprof[i].exchange(0);
    return k;
}

// A process launched one per GPU (torch.distributed.run sets LOCAL_RANK and
// LOCAL_WORLD_SIZE) keeps its host work on its own device -- LOCAL_RANK modulo
// the visible devices, torch's convention, whichever thread calls.  Only
// LOCAL_RANK engages it (a launcher that sets WORLD_SIZE alone gets the
// fan-out, not device 0), a LOCAL_WORLD_SIZE of 1 does not (the node's only
// process may use every device), and TYCHE_DEVICES / TYCHE_DEVICE_IDS or the
// RANK_PIN knob (0, at any time through tyche_set_knob) turn it off, e.g. for a
// helper process that inherited a worker's environment.  -1: not pinned.
int tyche::rank_device() {
    static const int d = [] {
        if (getenv("TYCHE_DEVICES") || getenv("TYCHE_DEVICE_IDS")) return -1;
        const char *lr = getenv("LOCAL_RANK"), *lw = getenv("LOCAL_WORLD_SIZE");
        if (!lr || !*lr || (lw && atoi(lw) == 1)) return -1;
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return -1;
        return std::max(0, atoi(lr)) % n;
    }();
    return d >= 0 && knob("RANK_PIN", 1) != 0 ? d : -1;
}

// Host batch over the calling thread's devices: its pinned device, or the
// device set.  Batches of at least two parts' worth of input
// (tyche_plan_split) are cut into contiguous page ranges of about equal input
// bytes, one per device, run concurrently; smaller ones go whole to the least
// busy device, so concurrent small calls (tyche's per-page compressor pool and
// restores) spread over all devices.
int tyche::run_host(size_t n, const void *const *src, const uint32_t *src_len, void *const *dst, const uint32_t *dst_cap,
                    int32_t *results, LaunchRef launch, bool zc_ok, int direct_out) {
    const HostPages pg{src, src_len, dst, dst_cap, results};
    if (pinned_device() >= 0) return run_host_batch(pinned_device(), n, pg, launch, zc_ok, direct_out);
    if (rank_device() >= 0)   // one process per GPU: its own device only
        return run_host_batch(rank_device(), n, pg, launch, zc_ok, direct_out);
    const DeviceSet &ds = device_set();
    if (ds.ids.empty()) return fail_msg(ds.why);
    std::vector<size_t> cuts(ds.ids.size() + 1);
    const size_t parts = tyche_plan_split(n, src_len, (int)ds.ids.size(), fanout_min_bytes(), cuts.data());
    if (parts <= 1) return run_host_batch(pick_device(ds.ids), n, pg, launch, zc_ok, direct_out);
    std::vector<int> rcs(parts, TYCHE_E_OK);
    std::vector<std::string> errs(parts);
    std::vector<std::thread> th;
    auto part = [&](size_t p) {
        const size_t a = cuts[p], m = cuts[p + 1] - cuts[p];
        rcs[p] = run_host_batch(ds.ids[p], m, HostPages{src + a, src_len + a, dst + a, dst_cap + a, results + a}, launch,
                                zc_ok, direct_out);
        if (rcs[p]) errs[p] = thread_error();
    };
    for (size_t p = 1; p < parts; p++) th.emplace_back(part, p);
    part(0);
    for (auto &t : th) t.join();
    for (size_t p = 0; p < parts; p++)
        if (rcs[p]) {
            set_thread_error(errs[p]);
            return rcs[p];
        }
    return TYCHE_E_OK;
}
