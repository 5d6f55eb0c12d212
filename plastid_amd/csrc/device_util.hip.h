// device_util.hip.h -- the device plumbing every driver of the one translation unit of plastid_counts.hip shares: error
// reporting (fail, HIP_TRY, PC_TRY), device blocks recycled per engine (DevPool, DevBuf; the policy is pool_host.h, plain
// C++ tested on the CPU), the page-locked buffer, the transfer ring, lap events, the reservation of a phase's buffers
// (room), the drain of a failed step (DrainOnExit, finish_phase) and the one seam every hipcub call goes through
// (cub_need / cub_run_sized / cub_run).  Included by plastid_counts.hip ahead of its first use.
#ifndef PLASTID_DEVICE_UTIL_HIP_H
#define PLASTID_DEVICE_UTIL_HIP_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "plastid_counts.h"
#include "pool_host.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t err__ = (expr);                                                                 \
        if (err__ != hipSuccess)                                                                   \
            return fail(err__ == hipErrorOutOfMemory ? PC_ERR_NOMEM : PC_ERR_HIP, "%s failed: %s (%s:%d)", \
                        #expr, hipGetErrorString(err__), __FILE__, __LINE__);                      \
    } while (0)

#define PC_TRY(expr)                                                                               \
    do {                                                                                           \
        const int rc__ = (expr);                                                                   \
        if (rc__ != PC_OK) return rc__;                                                            \
    } while (0)

// The pool and the reservoir of pool_host.h over hipFree.
inline void device_free(void *p) { (void)hipFree(p); }
using BigReservoir = pcmem::BigReservoir<device_free>;
using DevPool = pcmem::DevPool<device_free>;

// The pool a DevBuf without one of its own takes its blocks from: set for the duration of an entry point that
// allocates on behalf of an engine (staging, the BAM decoder), so that every buffer made there -- temporaries and the
// arrays a staged file keeps -- is recycled through that engine's pool.  (All users of one pool enqueue on its engine's
// streams in an order the entry points fix with events, so a recycled block is ordered after its last use.)
static thread_local DevPool *tls_pool = nullptr;
struct PoolScope {
    DevPool *prev;
    explicit PoolScope(DevPool *p) : prev(tls_pool) { tls_pool = p; }
    ~PoolScope() { tls_pool = prev; }
};

template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevPool *pool = nullptr;   // set: blocks come from / return to this pool
    int pool_class = -1;       // size class of the current block, -1: plain hipMalloc, -2: a large block of `big_bytes`
    size_t big_bytes = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) {
            bool kept = false;
            if (pool && pool_class >= 0) kept = pool->give(p, pool_class);
            else if (pool && pool_class == -2) kept = pool->big_give(p, big_bytes);
            if (!kept) (void)hipFree(p);
        }
        p = nullptr;
        cap = 0;
        pool_class = -1;
        big_bytes = 0;
    }
    int reserve(size_t n) {
        if (n <= cap) return PC_OK;
        release();
        if (n == 0) return PC_OK;
        if (!pool) pool = tls_pool;
        if (pool) {
            const int c = pcmem::size_class(n * sizeof(T));
            if (c < pcmem::kClasses) {
                void *q = pool->take(c);
                if (!q && hipMalloc(&q, pcmem::class_bytes(c)) != hipSuccess) {
                    (void)hipGetLastError();
                    pool->drain(false);   // (what the pool and the reservoir hold may be what is missing)
                    HIP_TRY(hipMalloc(&q, pcmem::class_bytes(c)));
                }
                p = (T *)q;
                cap = pcmem::class_bytes(c) / sizeof(T);
                pool_class = c;
                return PC_OK;
            }
            const size_t rounded = pcmem::big_round(n * sizeof(T));
            void *q = pool->big_take(rounded);
            if (!q && hipMalloc(&q, rounded) != hipSuccess) {
                (void)hipGetLastError();
                pool->drain(false);   // (what the pool and the reservoir hold may be what is missing)
                HIP_TRY(hipMalloc(&q, rounded));
            }
            p = (T *)q;
            cap = rounded / sizeof(T);
            pool_class = -2;
            big_bytes = rounded;
            return PC_OK;
        }
        if (hipMalloc((void **)&p, n * sizeof(T)) != hipSuccess) {   // (no pool of its own: the reservoir of the current device may hold what is missing)
            (void)hipGetLastError();
            p = nullptr;
            int dev_now = 0;
            if (hipGetDevice(&dev_now) == hipSuccess) BigReservoir::get().free_all(dev_now);
            HIP_TRY(hipMalloc((void **)&p, n * sizeof(T)));
        }
        cap = n;
        return PC_OK;
    }
    int upload(const T *src, size_t n, hipStream_t s) {
        PC_TRY(reserve(n));
        if (n) HIP_TRY(hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
        return PC_OK;
    }
    int upload(const std::vector<T> &v, hipStream_t s) { return upload(v.data(), v.size(), s); }
    void swap(DevBuf &o) {
        std::swap(p, o.p); std::swap(cap, o.cap); std::swap(pool, o.pool); std::swap(pool_class, o.pool_class); std::swap(big_bytes, o.big_bytes);
    }
};

// Page-locked host buffer that only grows.
struct PinnedBuf {
    uint8_t *p = nullptr;
    size_t cap = 0;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    int reserve(size_t n) {
        if (n <= cap) return PC_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        const size_t want = pcmem::pinned_want(n);
        HIP_TRY(hipHostMalloc((void **)&p, want, hipHostMallocDefault));
        cap = want;
        return PC_OK;
    }
};

// A typed window into a block some DevBuf owns (the tables of a plan share one block and one upload).
template <typename T> struct DevView {
    T *p = nullptr;
};

// Caller-owned (pageable) host arrays <-> HBM at the rate of the PCIe link.  hipMemcpy to or from pageable memory pins
// the pages on the fly, on one thread inside the driver: 25 GB/s for memory the runtime has not seen before, whatever
// the number of calling threads or streams (scripts/ubench/upload_probe.hip; 57 GB/s from page-locked memory on the
// same box).  Here a few host threads move pieces of the arrays through a ring of page-locked slots, each piece with a
// DMA of its own: 53 - 55 GB/s.  Up: a thread takes the next piece, waits until its slot's previous piece has landed,
// copies the piece into the slot and queues the DMA.  Down: it queues the DMA into the slot, waits for it and copies the
// piece out.  Pieces are taken in order and there are more slots than threads, so nobody waits on a piece that has not
// been taken.
using pcmem::TransferJob;
struct TransferRing {
    static constexpr int kSlots = 12, kThreadsUp = 6, kThreadsDown = 10;   // (down: the destination's pages are often touched for the first time)
    static constexpr size_t kPiece = pcmem::kPiece;
    uint8_t *slot[kSlots] = {};
    hipEvent_t ev[kSlots] = {};
    hipStream_t stream = nullptr;
    std::mutex busy;   // one transfer at a time per device
    // One ring per device for the life of the process: page-locking its 192 MB costs as much as staging ten million
    // records, and engines come and go (one per BAMGenomeArray).
    static TransferRing &of(int device) {
        static std::mutex m;
        static std::map<int, TransferRing *> *rings = new std::map<int, TransferRing *>;   // (never destroyed: no HIP call during static destruction)
        std::lock_guard<std::mutex> g(m);
        TransferRing *&r = (*rings)[device];
        if (!r) r = new TransferRing;
        return *r;
    }
    // every job has landed when this returns; `down`: dst is host memory, src device memory.
    // Small transfers take the runtime's own path (`always`: the ring whatever the size)
    int run(int device, const std::vector<TransferJob> &jobs, size_t piece, bool always, bool down = false) {
        std::lock_guard<std::mutex> one(busy);
        HIP_TRY(hipSetDevice(device));
        if (!stream) HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        size_t total = 0;
        for (const auto &j : jobs) total += j.bytes;
        const pcmem::Route route = pcmem::transfer_route(total, always);
        if (route == pcmem::Route::none) return PC_OK;
        const hipMemcpyKind kind = down ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
        if (route == pcmem::Route::direct) {
            for (const auto &j : jobs)
                if (j.bytes) HIP_TRY(hipMemcpyAsync(j.dst, j.src, j.bytes, kind, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            return PC_OK;
        }
        piece = pcmem::clamp_piece(piece);
        std::vector<TransferJob> pieces;
        for (const auto &j : jobs) {
            if (j.bytes == 0) continue;
            // host memory that is page-locked already (hipHostMalloc, hipHostRegister, a pinned torch tensor) needs no ring
            hipPointerAttribute_t attr;
            const void *host_side = down ? j.dst : j.src;
            if (!always && hipPointerGetAttributes(&attr, host_side) == hipSuccess && attr.type == hipMemoryTypeHost) {
                HIP_TRY(hipMemcpyAsync(j.dst, j.src, j.bytes, kind, stream));
                continue;
            }
            (void)hipGetLastError();   // (an ordinary pointer: some runtimes report it as an error)
            pcmem::cut_job(pieces, j, piece);
        }
        const size_t np = pieces.size();
        for (int k = 0; k < kSlots && np > 0; ++k) {
            if (!slot[k]) HIP_TRY(hipHostMalloc((void **)&slot[k], kPiece, hipHostMallocDefault));
            if (!ev[k]) HIP_TRY(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
        }
        std::unique_ptr<std::atomic<uint8_t>[]> done(new std::atomic<uint8_t>[np]);   // up: DMA queued; down: copied out
        for (size_t k = 0; k < np; ++k) done[k].store(0, std::memory_order_relaxed);
        std::atomic<size_t> next{0};
        std::atomic<int> failed{0};
        std::mutex order;   // DMA and event of a piece are queued together
        auto work = [&]() {
            if (hipSetDevice(device) != hipSuccess) failed.store(1);
            for (;;) {
                const size_t p = next.fetch_add(1);
                if (p >= np) return;
                const int k = (int)(p % kSlots);
                if (p >= (size_t)kSlots) {   // the slot's previous piece
                    while (!done[p - kSlots].load(std::memory_order_acquire)) std::this_thread::yield();
                    if (!down && !failed.load() && hipEventSynchronize(ev[k]) != hipSuccess) failed.store(1);
                }
                if (!failed.load()) {
                    if (!down) std::memcpy(slot[k], pieces[p].src, pieces[p].bytes);
                    {
                        std::lock_guard<std::mutex> lk(order);
                        if (hipMemcpyAsync(down ? (void *)slot[k] : pieces[p].dst, down ? pieces[p].src : (const void *)slot[k], pieces[p].bytes, kind, stream) != hipSuccess ||
                            hipEventRecord(ev[k], stream) != hipSuccess)
                            failed.store(1);
                    }
                    if (down && !failed.load()) {
                        if (hipEventSynchronize(ev[k]) != hipSuccess) failed.store(1);
                        else std::memcpy(pieces[p].dst, slot[k], pieces[p].bytes);
                    }
                }
                done[p].store(1, std::memory_order_release);   // (also after a failure: whoever waits for this slot goes on and ends)
            }
        };
        int T = down ? kThreadsDown : kThreadsUp;
        if (const char *env = getenv("PC_STAGE_UPLOAD_THREADS")) T = std::max(1, std::min(kSlots - 1, atoi(env)));
        T = (int)std::min<size_t>((size_t)T, np);
        std::vector<std::thread> th;
        for (int t = 1; t < T; ++t) th.emplace_back(work);
        if (np > 0) work();
        for (auto &x : th) x.join();
        const hipError_t he = hipStreamSynchronize(stream);
        if (failed.load() || he != hipSuccess) { (void)hipGetLastError(); return fail(PC_ERR_HIP, "transfer ring: a copy failed"); }
        return PC_OK;
    }
};

double ms_between(hipEvent_t a, hipEvent_t b) { float t = 0.f; return hipEventElapsedTime(&t, a, b) == hipSuccess ? (double)t : 0.0; }
// The events that cut a call into laps: N events, destroyed on exit; lap k lies between events k and k + 1.
template <int N> struct LapEvents {
    hipEvent_t ev[N] = {};
    int create() {
        for (auto &x : ev) HIP_TRY(hipEventCreate(&x));
        return PC_OK;
    }
    ~LapEvents() { for (auto x : ev) if (x) (void)hipEventDestroy(x); }
    hipEvent_t operator[](int k) const { return ev[k]; }
    void laps(double *ms, int n) const { for (int k = 0; k < n; ++k) ms[k] = ms_between(ev[k], ev[k + 1]); }
};
// one more buffer of a phase, unless an earlier one has failed
template <typename Buf> void room(int &rc, Buf &buf, size_t n) { if (rc == PC_OK) rc = buf.reserve(n); }
// A step's temporaries are read by what it queued: an early return drains the stream before they go out of scope
// (disarmed behind the step's own synchronisation).  Declared BEHIND the host and device temporaries it covers.
// The phases of the decoders and writers use it; a staging phase, which collects the first error of its enqueues in a
// hipError_t, closes with finish_phase instead.
struct DrainOnExit {
    hipStream_t st; bool armed = true;
    ~DrainOnExit() { if (armed) (void)hipStreamSynchronize(st); }
};
// The end of a phase with work in flight: waits for the stream and reports the first error of the phase (`he`), of a
// launch, or of the wait.  `what` is a format that takes the error string, or none.
int finish_phase(hipStream_t st, hipError_t he, const char *what) {
    if (he == hipSuccess) he = hipGetLastError();
    const hipError_t waited = hipStreamSynchronize(st);
    if (he == hipSuccess) he = waited;
    return he == hipSuccess ? PC_OK : fail(PC_ERR_HIP, what, hipGetErrorString(he));
}
// A hipcub call is `call(tmp, bytes)`: with tmp null it says how many temporary bytes it needs, otherwise it runs.
// cub_run asks, grows `tmp` and runs (a grown block is recycled through the engine's pool in stream order: no
// synchronise).  Calls that share a temporary sized up front ask through cub_need -- `bytes`: the call's own answer,
// `most`: the largest so far -- and run through cub_run_sized, which asks nothing more; the temporary is a buffer, or
// a raw pointer into a block carved elsewhere.  A call whose count is known only after its temporary is sized is a
// function of the count that returns the lambda: asked at the bound, run at the count, the arguments written once.  A
// staging phase that collects its first error in a hipError_t for finish_phase runs through cub_enqueue.
template <typename Call> int cub_need(size_t &most, size_t &bytes, Call call) {
    bytes = 0;
    HIP_TRY(call((void *)nullptr, bytes));
    most = std::max(most, bytes);
    return PC_OK;
}
template <typename Call> hipError_t cub_enqueue(void *tmp, size_t bytes, Call call) { return call(tmp, bytes); }
template <typename Call> int cub_run_sized(void *tmp, size_t bytes, Call call) {
    HIP_TRY(cub_enqueue(tmp, bytes, call));
    return PC_OK;
}
template <typename T, typename Call> int cub_run_sized(DevBuf<T> &tmp, size_t bytes, Call call) { return cub_run_sized((void *)tmp.p, bytes, call); }
template <typename Tmp, typename Call> int cub_run(Tmp &tmp, Call call) {
    size_t most = 16, bytes = 0;
    PC_TRY(cub_need(most, bytes, call));
    PC_TRY(tmp.reserve(most));
    return cub_run_sized(tmp, bytes, call);
}

}   // namespace

#endif
