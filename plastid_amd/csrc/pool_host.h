// pool_host.h -- the policy of the device-memory plumbing (device_util.hip.h), free of HIP: size classes and rounding
// of pooled blocks, the give / take / trim accounting of the per-engine pool and the process-wide reservoir, the growth
// of the page-locked buffer, the cut of a transfer into pieces and the choice between the transfer ring, the pinned
// buffer and a direct copy.  The function that frees a device block is a template argument: device_util.hip.h passes
// hipFree, tests/pool_host_test.cpp a counting fake.  Plain C++, tested on the CPU.
#ifndef PLASTID_POOL_HOST_H
#define PLASTID_POOL_HOST_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <mutex>
#include <vector>

namespace pcmem {

using FreeFn = void (*)(void *);

constexpr int kMinShift = 8, kClasses = 18;   // 256 B .. 32 MiB
constexpr size_t kMaxCached = (size_t)512 << 20;
// Large blocks (> 32 MiB: the arrays of a staged file, the scratch of the BAM decoder) are kept too, by size rounded
// up to a quarter of a power of two, up to kBigLimit in all: on some hosts a hipMalloc / hipFree pair of a few
// hundred MB takes tens of milliseconds (measured: 60 ms per call on one box of the pool, < 1 ms on others), which a
// caller that stages file after file -- or the same file again -- would pay every time.
constexpr size_t kBigLimit = (size_t)64 << 30;
constexpr size_t kDefaultLimit = (size_t)4 << 30;   // what the reservoir keeps per device (PC_POOL_RESERVOIR_GB)
constexpr size_t kPiece = (size_t)16 << 20;         // one slot of the transfer ring
constexpr size_t kSmallRead = 256 * 1024;           // read-backs up to here come through the engine's pinned buffer

inline int size_class(size_t bytes) {
    int c = 0;
    while (c < kClasses && ((size_t)1 << (kMinShift + c)) < bytes) ++c;
    return c;   // kClasses: too large to pool
}
inline size_t class_bytes(int c) { return (size_t)1 << (kMinShift + c); }
inline size_t big_round(size_t bytes) {
    const int k = 63 - __builtin_clzll((unsigned long long)bytes);
    const size_t step = (size_t)1 << (k - 2);
    return (bytes + step - 1) / step * step;
}

// Device blocks that outlive their engine: an engine that goes away hands the idle blocks of its pool to this
// process-wide reservoir (per device, by size) instead of freeing them, and the pool of a later engine looks here
// before it allocates.  Engines come and go -- one per BAMGenomeArray, one per config in bench.py -- and on some
// boxes of the pool a hipMalloc that follows the hipFree of tens of GB takes SECONDS (measured round 5: 1.5 s and 2.1 s
// for the first large buffer of a staging call right after an engine of the same size was destroyed; milliseconds when
// nothing had been freed).  Only blocks of a destroyed engine get here -- its streams are drained by then, so nothing
// is in flight on them.
// What is kept is bounded: PC_POOL_RESERVOIR_GB per device (default 4: the tables of a few plans and a small file; a
// process that cycles through engines of tens of GB -- bench.py -- opts in to more), and when the LAST engine of a device
// is destroyed everything above that default is freed, so that another library in the process (torch, cupy) finds the
// HBM this one no longer uses.  pc_release_cached_memory frees all of it.
template <FreeFn Free> struct BigReservoir {
    std::mutex m;
    struct PerDevice { std::map<size_t, std::vector<void *>> big; size_t cached = 0; int engines = 0; };
    std::map<int, PerDevice> dev;   // keyed by the device id itself (no folding of ids onto a fixed table)
    size_t limit = kDefaultLimit;
    BigReservoir() { if (const char *env = getenv("PC_POOL_RESERVOIR_GB")) limit = (size_t)std::max(0ll, atoll(env)) << 30; }
    static BigReservoir &get() { static BigReservoir *r = new BigReservoir; return *r; }   // (never destroyed: no free during static destruction)
    void *take(int device, size_t rounded) {
        std::lock_guard<std::mutex> g(m);
        PerDevice &d = dev[device];
        auto it = d.big.find(rounded);
        if (it == d.big.end() || it->second.empty()) return nullptr;
        void *p = it->second.back();
        it->second.pop_back();
        d.cached -= rounded;
        return p;
    }
    bool give(int device, void *p, size_t rounded) {
        std::lock_guard<std::mutex> g(m);
        PerDevice &d = dev[device];
        if (d.cached + rounded > limit) return false;
        d.big[rounded].push_back(p);
        d.cached += rounded;
        return true;
    }
    // largest blocks first until at most `keep` bytes are left
    void trim_locked(PerDevice &d, size_t keep) {
        for (auto it = d.big.rbegin(); it != d.big.rend() && d.cached > keep; ++it)
            while (!it->second.empty() && d.cached > keep) {
                Free(it->second.back());
                it->second.pop_back();
                d.cached -= it->first;
            }
    }
    void free_all(int device) {   // (an allocation failed: what is kept here may be what is missing)
        std::lock_guard<std::mutex> g(m);
        trim_locked(dev[device], 0);
        dev[device].big.clear();
    }
    void engine_created(int device) { std::lock_guard<std::mutex> g(m); dev[device].engines += 1; }
    void engine_destroyed(int device) {   // the last one of the device: only the default amount stays
        std::lock_guard<std::mutex> g(m);
        PerDevice &d = dev[device];
        if (--d.engines <= 0) { d.engines = 0; trim_locked(d, std::min(limit, kDefaultLimit)); }
    }
};

// Per-engine cache of small device blocks.  A plan of one short segment is otherwise dominated by
// hipMalloc / hipFree (the latter synchronises the device): blocks up to 32 MiB are kept by
// power-of-two size class when a plan lets go of them and handed to the next one.  Every user of
// one pool enqueues on the same engine stream, so a recycled block is ordered after its last use.  (The one exception,
// the transfer ring's own stream, synchronises the engine stream before it touches pooled blocks: stage_upload.)
template <FreeFn Free> struct DevPool {
    std::mutex m;
    std::vector<void *> bins[kClasses];
    size_t cached = 0;
    std::map<size_t, std::vector<void *>> big;
    size_t big_cached = 0;
    int device = 0;
    BigReservoir<Free> *reservoir = &BigReservoir<Free>::get();   // (a test builds its own)
    void *take(int c) {
        {
            std::lock_guard<std::mutex> g(m);
            if (!bins[c].empty()) {
                void *p = bins[c].back();
                bins[c].pop_back();
                cached -= class_bytes(c);
                return p;
            }
        }
        return reservoir->take(device, class_bytes(c));
    }
    bool give(void *p, int c) {
        std::lock_guard<std::mutex> g(m);
        if (cached + class_bytes(c) > kMaxCached) return false;
        bins[c].push_back(p);
        cached += class_bytes(c);
        return true;
    }
    void *big_take(size_t rounded) {
        {
            std::lock_guard<std::mutex> g(m);
            auto it = big.find(rounded);
            if (it != big.end() && !it->second.empty()) {
                void *p = it->second.back();
                it->second.pop_back();
                big_cached -= rounded;
                return p;
            }
        }
        return reservoir->take(device, rounded);
    }
    bool big_give(void *p, size_t rounded) {
        std::lock_guard<std::mutex> g(m);
        if (big_cached + rounded > kBigLimit) return false;
        big[rounded].push_back(p);
        big_cached += rounded;
        return true;
    }
    // keep_big: the engine is going away with its streams drained -- its blocks go to the process-wide reservoir
    void drain(bool keep_big) {
        std::lock_guard<std::mutex> g(m);
        for (int c = 0; c < kClasses; ++c) {
            for (void *p : bins[c])
                if (!keep_big || !reservoir->give(device, p, class_bytes(c))) Free(p);
            bins[c].clear();
        }
        cached = 0;
        for (auto &kv : big)
            for (void *p : kv.second)
                if (!keep_big || !reservoir->give(device, p, kv.first)) Free(p);
        big.clear();
        big_cached = 0;
        if (!keep_big) reservoir->free_all(device);
    }
    ~DevPool() { drain(true); }
};

// the page-locked buffer only grows, by half more than asked: covers every short read-back (kSmallRead) from the start
inline size_t pinned_want(size_t n) { return std::max<size_t>(n + n / 2, 512 * 1024); }

// One copy of a transfer, and its cut into pieces of at most `piece` bytes (a slot of the ring holds kPiece).
struct TransferJob { void *dst; const void *src; size_t bytes; };
inline size_t clamp_piece(size_t piece) { return std::max<size_t>(1, std::min(piece, kPiece)); }
inline void cut_job(std::vector<TransferJob> &pieces, const TransferJob &j, size_t piece) {
    for (size_t off = 0; off < j.bytes; off += piece)
        pieces.push_back({(uint8_t *)j.dst + off, (const uint8_t *)j.src + off, std::min(piece, j.bytes - off)});
}

// TransferRing::run: small transfers take the runtime's own path (`always`: the ring whatever the size)
enum class Route { none, direct, ring, pinned };
inline Route transfer_route(size_t total, bool always) {
    if (total == 0) return Route::none;
    return total < 4 * kPiece && !always ? Route::direct : Route::ring;
}
// A read-back of `bytes` into caller-owned memory (`knob`: PC_STAGE_SLICE is set -- the ring for every size): the counts
// of a whole annotation through the ring, short vectors through the page-locked buffer, the rest directly.
inline Route read_route(size_t bytes, bool knob) {
    if (bytes >= 4 * kPiece || (bytes > 0 && knob)) return Route::ring;
    return bytes > 0 && bytes <= kSmallRead ? Route::pinned : Route::direct;
}

}   // namespace pcmem

#endif
