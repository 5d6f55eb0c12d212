// pool_host_test.cpp -- plastid_amd/csrc/pool_host.h on a machine without a GPU (tests/test_pool_host.py compiles it
// under the address and undefined-behaviour sanitizers and runs it).  Every expected value is a literal worked by hand
// from the pool, the page-locked buffer and the transfer ring as they stood in plastid_counts.hip before the header
// existed; none is produced by calling the header.  Device blocks are numbers that are never dereferenced, and the
// function that frees one is a fake that records its argument.  Prints "pool_host: ok".
#include "pool_host.h"

#include <cstdio>
#include <cstdint>
#include <vector>

using namespace pcmem;

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)
#define CHECK_EQ(got, want)                                                          \
    do {                                                                             \
        const long long g__ = (long long)(got), w__ = (long long)(want);             \
        if (g__ != w__) { fprintf(stderr, "%s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #got, g__, w__); ++failures; } \
    } while (0)

static const size_t KiB = (size_t)1 << 10, MiB = (size_t)1 << 20, GiB = (size_t)1 << 30;

static std::vector<void *> freed;
static void fake_free(void *p) { freed.push_back(p); }
static void *block(uintptr_t k) { return (void *)(k << 12); }
typedef BigReservoir<fake_free> Reservoir;
typedef DevPool<fake_free> Pool;

static void test_sizes() {
    CHECK_EQ(kMinShift, 8); CHECK_EQ(kClasses, 18);
    CHECK_EQ(kMaxCached, 512 * MiB); CHECK_EQ(kBigLimit, 64 * GiB); CHECK_EQ(kDefaultLimit, 4 * GiB);
    CHECK_EQ(kPiece, 16 * MiB); CHECK_EQ(kSmallRead, 256 * KiB);
    CHECK_EQ(size_class(1), 0);
    CHECK_EQ(size_class(256), 0);
    CHECK_EQ(size_class(257), 1);
    CHECK_EQ(size_class(512), 1);
    CHECK_EQ(size_class(32 * MiB), 17);
    CHECK_EQ(size_class(32 * MiB + 1), 18);   // kClasses: not pooled
    CHECK_EQ(size_class(GiB), 18);
    CHECK_EQ(class_bytes(0), 256); CHECK_EQ(class_bytes(1), 512); CHECK_EQ(class_bytes(17), 32 * MiB);
    // a quarter of the power of two below: 32 MiB .. 64 MiB in steps of 8 MiB, 1 GiB .. 2 GiB in steps of 256 MiB
    CHECK_EQ(big_round(32 * MiB + 1), 40 * MiB);
    CHECK_EQ(big_round(33 * MiB + 1), 40 * MiB);
    CHECK_EQ(big_round(40 * MiB), 40 * MiB);
    CHECK_EQ(big_round(40 * MiB + 1), 48 * MiB);
    CHECK_EQ(big_round(GiB), GiB);
    CHECK_EQ(big_round(GiB + 1), GiB + 256 * MiB);
    // the page-locked buffer: half more than asked, 512 KiB at least
    CHECK_EQ(pinned_want(1), 512 * KiB);
    CHECK_EQ(pinned_want(MiB), MiB + 512 * KiB);
    CHECK_EQ(pinned_want(256 * KiB), 512 * KiB);
}

static void test_pieces() {
    uint8_t *dst = (uint8_t *)block(1), *src = (uint8_t *)block(1 << 20);
    std::vector<TransferJob> pieces;
    cut_job(pieces, {dst, src, 40 * MiB}, 16 * MiB);
    CHECK_EQ(pieces.size(), 3);
    if (pieces.size() == 3) {
        const size_t off[3] = {0, 16 * MiB, 32 * MiB}, len[3] = {16 * MiB, 16 * MiB, 8 * MiB};
        for (int k = 0; k < 3; ++k) {
            CHECK((uint8_t *)pieces[k].dst == dst + off[k]); CHECK((const uint8_t *)pieces[k].src == src + off[k]); CHECK_EQ(pieces[k].bytes, len[k]);
        }
    }
    cut_job(pieces, {dst, src, 0}, 16 * MiB);   // an empty job adds nothing
    CHECK_EQ(pieces.size(), 3);
    cut_job(pieces, {dst, src, 3}, 1);
    CHECK_EQ(pieces.size(), 6);
    CHECK_EQ(pieces.back().bytes, 1); CHECK((uint8_t *)pieces.back().dst == dst + 2);
    CHECK_EQ(clamp_piece(0), 1);
    CHECK_EQ(clamp_piece(GiB), 16 * MiB);
    CHECK_EQ(clamp_piece(4096), 4096);
    // the ring from four slots' worth on, or always
    CHECK(transfer_route(64 * MiB - 1, false) == Route::direct);
    CHECK(transfer_route(64 * MiB, false) == Route::ring);
    CHECK(transfer_route(1, true) == Route::ring);
    CHECK(transfer_route(1, false) == Route::direct);
    CHECK(transfer_route(0, false) == Route::none);
    CHECK(transfer_route(0, true) == Route::none);
    // a read-back of the counts
    CHECK(read_route(256 * KiB, false) == Route::pinned);
    CHECK(read_route(256 * KiB + 8, false) == Route::direct);
    CHECK(read_route(8, false) == Route::pinned);
    CHECK(read_route(64 * MiB - 8, false) == Route::direct);
    CHECK(read_route(64 * MiB, false) == Route::ring);
    CHECK(read_route(8, true) == Route::ring);
    CHECK(read_route(0, true) == Route::direct);   // (nothing to copy: the caller only waits for the stream)
    CHECK(read_route(0, false) == Route::direct);
}

static void test_give_take() {
    Reservoir r;
    Pool pool;
    pool.reservoir = &r;
    pool.device = 3;
    freed.clear();
    // small blocks: 16 of 32 MiB fill the 512 MiB; the 17th is refused and left to the caller
    for (uintptr_t k = 1; k <= 16; ++k) CHECK(pool.give(block(k), 17));
    CHECK_EQ(pool.cached, 512 * MiB);
    CHECK(!pool.give(block(17), 17));
    CHECK_EQ(pool.cached, 512 * MiB); CHECK_EQ(freed.size(), 0);
    fake_free(block(17));   // (what DevBuf::release does with a refused block)
    CHECK_EQ(freed.size(), 1);
    CHECK(!pool.give(block(18), 0));   // 256 bytes more are too many as well
    // take after give: the same block, and the old count
    CHECK(pool.take(17) == block(16));
    CHECK_EQ(pool.cached, 480 * MiB);
    CHECK(pool.give(block(16), 17));
    CHECK_EQ(pool.cached, 512 * MiB);
    CHECK(pool.take(5) == nullptr);   // nothing of that class, nothing in the reservoir
    CHECK_EQ(pool.cached, 512 * MiB);
    // large blocks: 64 of 1 GiB, the 65th is refused
    for (uintptr_t k = 1; k <= 64; ++k) CHECK(pool.big_give(block(100 + k), GiB));
    CHECK_EQ(pool.big_cached, 64 * GiB);
    CHECK(!pool.big_give(block(165), GiB));
    CHECK(!pool.big_give(block(165), 40 * MiB));
    CHECK_EQ(pool.big_cached, 64 * GiB); CHECK_EQ(freed.size(), 1);
    CHECK(pool.big_take(GiB) == block(164));
    CHECK_EQ(pool.big_cached, 63 * GiB);
    CHECK(pool.big_take(40 * MiB) == nullptr);
    CHECK(pool.big_give(block(164), GiB));
    CHECK_EQ(pool.big_cached, 64 * GiB);
    // the reservoir: refused beyond its limit (4 GiB unless the environment says otherwise)
    CHECK_EQ(r.limit, 4 * GiB);
    for (uintptr_t k = 1; k <= 4; ++k) CHECK(r.give(3, block(200 + k), GiB));
    CHECK(!r.give(3, block(205), 256));
    CHECK(r.give(2, block(205), 256));   // (another device has its own count)
    CHECK_EQ(r.dev[3].cached, 4 * GiB);
    CHECK(r.take(3, GiB) == block(204));
    CHECK_EQ(r.dev[3].cached, 3 * GiB);
    CHECK(r.take(3, 2 * GiB) == nullptr);
    CHECK(r.give(3, block(204), GiB));
    CHECK_EQ(r.dev[3].cached, 4 * GiB);
    // a pool that has nothing of a size looks in the reservoir of its device
    CHECK(pool.big_take(GiB) == block(164));
    pool.big.clear(); pool.big_cached = 0;
    CHECK(pool.big_take(GiB) == block(204));
    CHECK_EQ(r.dev[3].cached, 3 * GiB);
    CHECK(pool.take(0) == nullptr);   // (device 2 holds the 256 bytes)
    // (emptied by hand, so that the destructor hands nothing on)
    for (auto &b : pool.bins) b.clear();
    pool.cached = 0;
    CHECK_EQ(freed.size(), 1);
}

static void test_trim() {
    Reservoir r;
    r.limit = 8 * GiB;
    freed.clear();
    CHECK(r.give(0, block(1), 512 * MiB)); CHECK(r.give(0, block(2), 512 * MiB));
    CHECK(r.give(0, block(3), GiB)); CHECK(r.give(0, block(4), GiB));
    CHECK(r.give(0, block(5), 2 * GiB));
    CHECK_EQ(r.dev[0].cached, 5 * GiB);
    // largest first: the 2 GiB block leaves 3 GiB, one of 1 GiB leaves 2 GiB <= 2.5 GiB -- and there it stops
    r.trim_locked(r.dev[0], 2 * GiB + 512 * MiB);
    CHECK_EQ(freed.size(), 2);
    if (freed.size() == 2) { CHECK(freed[0] == block(5)); CHECK(freed[1] == block(4)); }
    CHECK_EQ(r.dev[0].cached, 2 * GiB);
    r.trim_locked(r.dev[0], 2 * GiB);   // already there
    CHECK_EQ(freed.size(), 2);
    r.free_all(0);
    CHECK_EQ(freed.size(), 5); CHECK_EQ(r.dev[0].cached, 0); CHECK(r.dev[0].big.empty());
    if (freed.size() == 5) { CHECK(freed[2] == block(3)); CHECK(freed[3] == block(2)); CHECK(freed[4] == block(1)); }
}

static void test_engines() {
    Reservoir r;
    r.limit = 8 * GiB;
    freed.clear();
    r.engine_created(1); r.engine_created(1);
    for (uintptr_t k = 1; k <= 6; ++k) CHECK(r.give(1, block(k), GiB));
    r.engine_destroyed(1);   // one engine left: nothing goes
    CHECK_EQ(freed.size(), 0); CHECK_EQ(r.dev[1].cached, 6 * GiB);
    r.engine_destroyed(1);   // the last: min(8 GiB, 4 GiB) stay
    CHECK_EQ(freed.size(), 2); CHECK_EQ(r.dev[1].cached, 4 * GiB); CHECK_EQ(r.dev[1].engines, 0);
    // a limit below the default: that much stays
    Reservoir s;
    s.limit = 2 * GiB;
    freed.clear();
    s.engine_created(0);
    CHECK(s.give(0, block(1), GiB)); CHECK(s.give(0, block(2), GiB)); CHECK(!s.give(0, block(3), GiB));
    s.engine_destroyed(0);
    CHECK_EQ(freed.size(), 0); CHECK_EQ(s.dev[0].cached, 2 * GiB);
    s.limit = GiB;
    s.engine_created(0);
    s.engine_destroyed(0);
    CHECK_EQ(freed.size(), 1); CHECK_EQ(s.dev[0].cached, GiB);
    s.free_all(0);
    r.free_all(1);
}

static void test_drain() {
    Reservoir r;
    r.limit = 80 * MiB;
    freed.clear();
    {
        Pool pool;
        pool.reservoir = &r;
        pool.device = 0;
        CHECK(pool.give(block(1), 17)); CHECK(pool.give(block(2), 17)); CHECK(pool.give(block(3), 17));   // 3 x 32 MiB
        CHECK(pool.big_give(block(4), 40 * MiB));
        // the engine goes away: small classes first -- 32 and 64 MiB fit under 80 MiB, the third does not, nor do the 40 MiB
        pool.drain(true);
        CHECK_EQ(pool.cached, 0); CHECK_EQ(pool.big_cached, 0); CHECK(pool.big.empty());
        CHECK_EQ(r.dev[0].cached, 64 * MiB);
        CHECK_EQ(freed.size(), 2);
        if (freed.size() == 2) { CHECK(freed[0] == block(3)); CHECK(freed[1] == block(4)); }
        // the next engine's pool finds them
        CHECK(pool.take(17) == block(2));
        CHECK_EQ(r.dev[0].cached, 32 * MiB);
        CHECK(pool.give(block(2), 17));
        CHECK(pool.big_give(block(5), 48 * MiB));
        CHECK(r.give(1, block(6), 32 * MiB));   // another device's
        // an allocation failed: everything of the pool and of its device's reservoir goes
        freed.clear();
        pool.drain(false);
        CHECK_EQ(freed.size(), 3);
        if (freed.size() == 3) { CHECK(freed[0] == block(2)); CHECK(freed[1] == block(5)); CHECK(freed[2] == block(1)); }
        CHECK_EQ(pool.cached, 0); CHECK_EQ(pool.big_cached, 0);
        CHECK_EQ(r.dev[0].cached, 0); CHECK(r.dev[0].big.empty());
        CHECK_EQ(r.dev[1].cached, 32 * MiB);
        CHECK(pool.give(block(7), 0));   // (the destructor hands it to the reservoir)
    }
    CHECK_EQ(freed.size(), 3);
    CHECK_EQ(r.dev[0].cached, 256);
    r.free_all(0); r.free_all(1);
    CHECK_EQ(freed.size(), 5);
}

int main() {
    test_sizes();
    test_pieces();
    test_give_take();
    test_trim();
    test_engines();
    test_drain();
    if (failures) { fprintf(stderr, "pool_host: %d check(s) failed\n", failures); return 1; }
    printf("pool_host: ok\n");
    return 0;
}
