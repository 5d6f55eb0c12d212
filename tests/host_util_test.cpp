// CPU test of plastid_amd/csrc/host_util.h (compiled and run by tests/test_host_logic.py; test infrastructure).
#include <atomic>
#include <cstdio>
#include <random>
#include "host_util.h"

int main() {
    long bad = 0;
    // gallop_lower_bound == std::lower_bound for every hint
    std::mt19937_64 rng(5);
    for (int it = 0; it < 100000; ++it) {
        const size_t n = rng() % 40;
        std::vector<int> v(n);
        for (auto &x : v) x = (int)(rng() % 30);
        std::sort(v.begin(), v.end());
        const int key = (int)(rng() % 34) - 2;
        const size_t hint = n ? rng() % (n + 3) : 0;
        const size_t got = gallop_lower_bound(n, hint, [&](size_t i) { return v[i] < key; });
        const size_t want = (size_t)(std::lower_bound(v.begin(), v.end(), key) - v.begin());
        if (got != want) ++bad;
    }
    printf("gallop_lower_bound: bad %ld\n", bad);
    // parallel_chunks covers [0, n) exactly once, whatever the width (regions served by the pool)
    for (int r = 0; r < 4000; ++r) {
        const int T = 1 + r % 17;
        const int64_t n = r % 3 == 0 ? 5 : 1000 + r;
        std::vector<int> hit((size_t)n, 0);
        parallel_chunks(n, T, [&](int, int64_t b, int64_t e) { for (int64_t i = b; i < e; ++i) hit[(size_t)i] += 1; });
        for (int v : hit) if (v != 1) ++bad;
    }
    // nested regions and concurrent callers (the pool is taken: those regions spawn their own threads)
    std::atomic<long> total{0};
    std::vector<std::thread> callers;
    for (int c = 0; c < 4; ++c) callers.emplace_back([&] {
        for (int r = 0; r < 500; ++r)
            parallel_chunks(64, 8, [&](int, int64_t b, int64_t e) {
                parallel_chunks(e - b, 3, [&](int, int64_t b2, int64_t e2) { total += e2 - b2; });
            });
    });
    for (auto &t : callers) t.join();
    if (total.load() != 4L * 500 * 64) ++bad;
    printf("parallel_chunks: total %ld (want %ld)\n", total.load(), 4L * 500 * 64);
    // PodVec: resize keeps what was written, push_back works
    PodVec<int> pv;
    pv.resize(1000);
    for (int i = 0; i < 1000; ++i) pv[(size_t)i] = i;
    pv.push_back(7);
    pv.resize(2000);
    for (int i = 0; i < 1000; ++i) if (pv[(size_t)i] != i) ++bad;
    if (pv[1000] != 7) ++bad;
    // scan_contigs == a record-by-record walk: bounds of the sorted prefix, first record out of order / out of range
    for (int it = 0; it < 3000; ++it) {
        const int ntid = 1 + (int)(rng() % 9);
        const int64_t n = (int64_t)(rng() % (it % 50 == 0 ? 30000 : 300));
        std::vector<int32_t> tid((size_t)n);
        int32_t cur = 0;
        for (auto &x : tid) { if (rng() % 17 == 0) cur = std::min<int32_t>(ntid - 1, cur + (int32_t)(rng() % 3)); x = cur; }
        for (int d = (int)(rng() % 3); d > 0 && n > 0; --d)   // defects: a contig out of range, a step back
            tid[(size_t)(rng() % (uint64_t)n)] = (rng() & 1) ? (int32_t)(rng() % 5) - 2 : ntid + (int32_t)(rng() % 2);
        int64_t want_ok = n;
        for (int64_t i = 0; i < n; ++i)
            if (tid[(size_t)i] < 0 || tid[(size_t)i] >= ntid || (i > 0 && tid[(size_t)i] < tid[(size_t)i - 1])) { want_ok = i; break; }
        std::vector<int64_t> want((size_t)ntid + 1, want_ok), got;
        for (int t = 0; t <= ntid; ++t)
            for (int64_t i = 0; i < want_ok; ++i)
                if (tid[(size_t)i] >= t) { want[(size_t)t] = i; break; }
        const int64_t got_ok = scan_contigs(tid.data(), n, ntid, 1 + it % 7, got);
        if (got_ok != want_ok || got != want) ++bad;
    }
    printf("scan_contigs: bad %ld\n", bad);
    // choose_window: the window sizes the published numbers were measured with, and the knob's limits
    {
        int64_t g = 0;
        if (choose_window(1, 2, 21031, 33373947ull, 0, &g) != 2048 || g != 3072) ++bad;          // C2 / C3: dense, stranded
        if (choose_window(1, 2, 479339, 91633228ull, 0, &g) != 768) ++bad;                       // C4: exons, a quarter of a window or less
        if (choose_window(1, 1, 10, 100000ull, 0, &g) != 4096 || g != 6144) ++bad;               // one strand mode: capped at 4 096
        if (choose_window(11, 2, 479339, 91633228ull, 0, &g) != 768 || g != 837) ++bad;          // C5: 16-bit bins, 36 KiB, multiples of 256
        if (choose_window(36, 2, 100, 100000ull, 0, &g) != 256) ++bad;                           // many rows: never below 256
        if (choose_window(3, 1, 100, 100000ull, 0, &g) != 4096) ++bad;
        if (choose_window(11, 2, 100, 100000ull, 512, &g) != 512) ++bad;                         // PC_TILE_G within twice the budget
        if (choose_window(11, 2, 100, 100000ull, 4096, &g) != 768) ++bad;                        // ... and beyond it: ignored
        if (choose_window(1, 2, 0, 0ull, 0, &g) != 2048) ++bad;                                  // no intervals: not sparse
    }
    printf("choose_window: bad %ld\n", bad);
    // choose_halo: the expected values are worked out from the definitions (the 99.5% span quantile, clamped to 64 .. 1024;
    // the longest span inside it; the aligned lengths of the two streams)
    {
        typedef std::vector<int64_t> H;
        auto same = [](const StageHalo &h, int wcap, int W, int Wg, int s0, int s1, int t0, int t1) {
            return h.wcap == wcap && h.W == W && h.Wg == Wg && h.slen_min == s0 && h.slen_max == s1 && h.tlen_min == t0 && h.tlen_max == t1;
        };
        const H zero(1026, 0), nolen(256, 0);
        auto spans = [&](std::initializer_list<std::pair<int, int64_t>> at) { H h = zero; for (auto &p : at) h[(size_t)p.first] += p.second; return h; };
        // no records: need 0 records, reached at span 0 -> the floor of 64; nothing inside the halo
        if (!same(choose_halo(zero, zero, zero, nolen, 65536, -1, 0, 255), 64, 1, 1, 0, 0, 0, 0)) ++bad;
        // 1 000 records of span 30: need 995, reached at 30 -> 64; longest span 30
        if (!same(choose_halo(spans({{30, 1000}}), zero, zero, nolen, 65536, -1, 1000, 255), 64, 30, 1, 0, 0, 0, 0)) ++bad;
        // 995 + 5: need 1000 - 5 = 995, the 995 records of span 30 suffice; 500 is outside the halo of 64
        if (!same(choose_halo(spans({{30, 995}, {500, 5}}), zero, zero, nolen, 65536, -1, 1000, 255), 64, 30, 1, 0, 0, 0, 0)) ++bad;
        // 994 + 6: 994 < 995, reached only at 500 -> halo 500, and 500 is the longest span inside it
        if (!same(choose_halo(spans({{30, 994}, {500, 6}}), zero, zero, nolen, 65536, -1, 1000, 255), 500, 500, 1, 0, 0, 0, 0)) ++bad;
        // the quantile is not reached at 1 024 (bin 1 025: every longer span): capped at 1 024
        if (!same(choose_halo(spans({{1025, 10}}), zero, zero, nolen, 65536, -1, 10, 255), 1024, 1, 1, 0, 0, 0, 0)) ++bad;
        if (!same(choose_halo(spans({{40, 900}, {1025, 100}}), zero, zero, nolen, 65536, -1, 1000, 255), 1024, 40, 1, 0, 0, 0, 0)) ++bad;
        // span 50 occurs only among wide records: W stays 30; one record of that span that is not wide raises it
        if (!same(choose_halo(spans({{30, 997}, {50, 3}}), zero, spans({{50, 3}}), nolen, 65536, -1, 1000, 255), 64, 30, 1, 0, 0, 0, 0)) ++bad;
        if (!same(choose_halo(spans({{30, 997}, {50, 3}}), zero, spans({{50, 2}}), nolen, 65536, -1, 1000, 255), 64, 50, 1, 0, 0, 0, 0)) ++bad;
        // gapped records of span 45 (inside the halo of 64: need 1002 - 5 = 997 <= 1000) set Wg; of span 100 (outside) they do not
        if (!same(choose_halo(spans({{30, 1000}, {45, 2}}), spans({{45, 2}}), zero, nolen, 65536, -1, 1002, 255), 64, 45, 45, 0, 0, 0, 0)) ++bad;
        if (!same(choose_halo(spans({{30, 1000}, {100, 2}}), spans({{100, 2}}), zero, nolen, 65536, -1, 1002, 255), 64, 30, 1, 0, 0, 0, 0)) ++bad;
        // no single-run record, a run stream with reads of 20 .. 90: tlen from rmin / rmax, slen 0 / 0
        if (!same(choose_halo(spans({{300, 1000}}), spans({{300, 1000}}), zero, nolen, 20, 90, 1000, 255), 300, 300, 300, 0, 0, 20, 90)) ++bad;
        // single-run records of 28, 33 and 200 under a halo of 64: the stream carries 28 .. 33; with the run stream's 10 .. 40: 10 .. 40
        H len1 = nolen;
        len1[28] = 5; len1[33] = 7; len1[200] = 1;
        if (!same(choose_halo(spans({{30, 1000}}), zero, zero, len1, 10, 40, 1000, 255), 64, 30, 1, 28, 33, 10, 40)) ++bad;
        // ... under a halo of 500 the stream's own limit binds: 200 is carried, and with a limit of 100 it is not
        if (!same(choose_halo(spans({{30, 994}, {500, 6}}), zero, zero, len1, 65536, -1, 1000, 255), 500, 500, 1, 28, 200, 28, 200)) ++bad;
        if (!same(choose_halo(spans({{30, 994}, {500, 6}}), zero, zero, len1, 65536, -1, 1000, 100), 500, 500, 1, 28, 33, 28, 33)) ++bad;
    }
    printf("choose_halo: bad %ld\n", bad);
    // lin_layout (buckets of 2^7 = 128 positions): bucket count of the furthest position a read of the contig touches, plus one
    {
        std::vector<int64_t> off;
        // contig 0: last start 300, furthest end 330 (exclusive) -> position 329, bucket 2: 3 + 1 entries; contig 1: no
        // records, one entry; contig 2: last start 100 but a read that ends at 1 000 -> position 999, bucket 7: 8 + 1
        if (lin_layout({0, 4, 4, 9}, {300, -1, 100}, {330, 0, 1000}, 7, off) != 14 || off != std::vector<int64_t>({0, 4, 5, 14})) ++bad;
        // a contig without records ignores whatever its slots hold
        if (lin_layout({0, 0}, {77777, }, {99999}, 7, off) != 1 || off != std::vector<int64_t>({0, 1})) ++bad;
        // the last bucket boundary: 127 is the last position of bucket 0, 128 the first of bucket 1 -- by the start and by the end
        if (lin_layout({0, 1}, {127}, {100}, 7, off) != 2) ++bad;
        if (lin_layout({0, 1}, {128}, {100}, 7, off) != 3) ++bad;
        if (lin_layout({0, 1}, {0}, {128}, 7, off) != 2) ++bad;
        if (lin_layout({0, 1}, {0}, {129}, 7, off) != 3) ++bad;
        if (lin_layout({0, 1}, {0}, {1}, 7, off) != 2 || off != std::vector<int64_t>({0, 2})) ++bad;
        // another shift: position 1 023 is bucket 0 of 1 024, position 1 024 bucket 1
        if (lin_layout({0, 2}, {1023}, {1024}, 10, off) != 2 || lin_layout({0, 2}, {1024}, {1025}, 10, off) != 3) ++bad;
    }
    printf("lin_layout: bad %ld\n", bad);
    printf("host_util: %s\n", bad ? "FAILED" : "ok");
    return bad != 0;
}
