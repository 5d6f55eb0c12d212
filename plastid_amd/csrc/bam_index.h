// The host half of the BAI index build (pc_bam_index_finish): from the runs of records with one bin, the linear arrays and
// the per-reference counts to the finished index and its bytes -- hts_idx_finish (kent/src/htslib/hts.c:1277-1291) with
// update_loff's forward fill (:1193-1209) and compress_binning (:1230-1275), then the layout of hts_idx_save for BAI
// (:1395-1457; SAM specification 5.2).  No GPU call: the kernels of index_kernels.hip.h, or a test, supply the inputs.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <utility>
#include <vector>

struct pc_bam_index {
    int32_t n_ref = 0;
    std::vector<uint8_t> bytes;   // the .bai file
    // records, placed records, runs before the finish, chunks after it, bins, linear entries, n_no_coor, mapped
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // upload, inflate, chain, fields, index kernels, read-back, host finish, total
    double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

namespace pcidxhost {

typedef std::pair<uint64_t, uint64_t> Chunk;
struct Bin { uint32_t id; bool alive; std::vector<Chunk> chunks; };

constexpr uint32_t kMetaBin = 37450u;
constexpr uint64_t kMinMarkerDist = 0x10000;   // HTS_MIN_MARKER_DIST: a bin that spans fewer BGZF file bytes moves into its parent

inline uint32_t level_first(int l) { return (uint32_t)(((1u << (3 * l)) - 1u) / 7u); }

inline void put32(std::vector<uint8_t> &o, uint32_t v) { for (int k = 0; k < 4; ++k) o.push_back((uint8_t)(v >> (8 * k))); }
inline void put64(std::vector<uint8_t> &o, uint64_t v) { for (int k = 0; k < 8; ++k) o.push_back((uint8_t)(v >> (8 * k))); }

// compress_binning for one reference; `bins` ascending by id
inline void compress(std::vector<Bin> &bins) {
    auto find = [&](uint32_t id) -> Bin * {
        auto it = std::lower_bound(bins.begin(), bins.end(), id, [](const Bin &b, uint32_t x) { return b.id < x; });
        return it != bins.end() && it->id == id && it->alive ? &*it : nullptr;
    };
    auto by_begin = [](const Chunk &a, const Chunk &b) { return a.first < b.first; };
    for (int l = 5; l > 0; --l) {
        // (hts.c:1241 visits every bin of this level or deeper; the deeper ones that are still here stayed for a reason
        // that holds -- their span, or a parent that does not exist -- so only the level's own bins can change)
        const uint32_t lo = level_first(l), hi = level_first(l + 1);
        auto it = std::lower_bound(bins.begin(), bins.end(), lo, [](const Bin &b, uint32_t x) { return b.id < x; });
        for (; it != bins.end() && it->id < hi; ++it) {
            if (!it->alive) continue;
            std::vector<Chunk> &c = it->chunks;
            if (l < 5 && c.size() > 1) std::stable_sort(c.begin(), c.end(), by_begin);
            if ((int64_t)(c.back().second >> 16) - (int64_t)(c.front().first >> 16) >= (int64_t)kMinMarkerDist) continue;
            Bin *parent = find((it->id - 1) >> 3);
            if (!parent) continue;
            parent->chunks.insert(parent->chunks.end(), c.begin(), c.end());
            std::vector<Chunk>().swap(c);
            it->alive = false;
        }
    }
    if (!bins.empty() && bins[0].id == 0 && bins[0].alive) std::stable_sort(bins[0].chunks.begin(), bins[0].chunks.end(), by_begin);
    for (Bin &b : bins) {   // adjacent chunks that touch one BGZF member become one
        if (!b.alive) continue;
        std::vector<Chunk> &c = b.chunks;
        size_t m = 0;
        for (size_t l = 1; l < c.size(); ++l) {
            if (c[m].second >> 16 >= c[l].first >> 16) { if (c[m].second < c[l].second) c[m].second = c[l].second; }
            else c[++m] = c[l];
        }
        c.resize(c.empty() ? 0 : m + 1);
    }
}

// 0, or a message
inline const char *finish(int n_ref, int64_t n_runs, const int32_t *run_tid, const uint32_t *run_bin, const uint64_t *run_beg, const uint64_t *run_end,
                          const int64_t *lin_start, const uint64_t *linear, const uint64_t *ref_beg, const uint64_t *ref_end,
                          const int64_t *ref_mapped, const int64_t *ref_unmapped, int64_t n_no_coor, pc_bam_index &out) {
    if (n_ref < 0 || n_runs < 0 || n_no_coor < 0) return "pc_bam_index_finish: negative count";
    if (n_runs > 0 && (!run_tid || !run_bin || !run_beg || !run_end)) return "pc_bam_index_finish: NULL run array";
    if (n_ref > 0 && (!lin_start || !ref_beg || !ref_end || !ref_mapped || !ref_unmapped)) return "pc_bam_index_finish: NULL reference array";
    if (n_ref > 0 && (lin_start[0] != 0 || (lin_start[n_ref] > 0 && !linear))) return "pc_bam_index_finish: bad linear arrays";
    for (int t = 0; t < n_ref; ++t)
        if (lin_start[t + 1] < lin_start[t] || lin_start[t + 1] - lin_start[t] > ((int64_t)1 << 15) || ref_mapped[t] < 0 || ref_unmapped[t] < 0)
            return "pc_bam_index_finish: bad linear arrays or counts";
    bool sorted = true;
    for (int64_t k = 0; k < n_runs; ++k) {
        if (run_tid[k] < 0 || run_tid[k] >= n_ref || run_bin[k] >= kMetaBin) return "pc_bam_index_finish: run with a reference id or bin out of range";
        if (run_end[k] < run_beg[k]) return "pc_bam_index_finish: run that ends before it begins";
        if (ref_mapped[run_tid[k]] + ref_unmapped[run_tid[k]] == 0) return "pc_bam_index_finish: run of a reference without records";
        if (k > 0 && (run_tid[k] < run_tid[k - 1] || (run_tid[k] == run_tid[k - 1] && run_bin[k] < run_bin[k - 1]))) sorted = false;
    }
    // (tid, bin) order, file order kept inside a bin
    std::vector<int64_t> order;
    if (!sorted) {
        order.resize((size_t)n_runs);
        std::iota(order.begin(), order.end(), (int64_t)0);
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
            return run_tid[a] != run_tid[b] ? run_tid[a] < run_tid[b] : run_bin[a] < run_bin[b];
        });
    }
    auto at = [&](int64_t k) { return sorted ? k : order[(size_t)k]; };
    std::vector<uint8_t> &o = out.bytes;
    o.clear();
    o.reserve((size_t)(16 + 16 * n_runs + 8 * (n_ref ? lin_start[n_ref] : 0) + 48 * (int64_t)n_ref));
    o.insert(o.end(), {'B', 'A', 'I', 1});
    put32(o, (uint32_t)n_ref);
    int64_t k = 0, n_chunks = 0, n_bins = 0, placed = 0, mapped = 0;
    std::vector<Bin> bins;
    for (int t = 0; t < n_ref; ++t) {
        bins.clear();
        for (; k < n_runs && run_tid[at(k)] == t; ++k) {
            const int64_t r = at(k);
            if (bins.empty() || bins.back().id != run_bin[r]) bins.push_back(Bin{run_bin[r], true, {}});
            bins.back().chunks.emplace_back(run_beg[r], run_end[r]);
        }
        compress(bins);
        const bool has = ref_mapped[t] + ref_unmapped[t] > 0;
        uint32_t n_bin = has ? 1u : 0u;
        for (const Bin &b : bins) n_bin += b.alive ? 1u : 0u;
        put32(o, n_bin);
        for (const Bin &b : bins) {
            if (!b.alive) continue;
            put32(o, b.id); put32(o, (uint32_t)b.chunks.size());
            for (const Chunk &c : b.chunks) { put64(o, c.first); put64(o, c.second); }
            n_chunks += (int64_t)b.chunks.size(); ++n_bins;
        }
        if (has) {
            put32(o, kMetaBin); put32(o, 2u);
            put64(o, ref_beg[t]); put64(o, ref_end[t]); put64(o, (uint64_t)ref_mapped[t]); put64(o, (uint64_t)ref_unmapped[t]);
        }
        const int64_t n_intv = lin_start[t + 1] - lin_start[t];
        put32(o, (uint32_t)n_intv);
        uint64_t last = ref_beg[t];   // the leading windows no record covers: the offset of the reference's first record
        for (int64_t w = 0; w < n_intv; ++w) {
            const uint64_t v = linear[lin_start[t] + w];
            if (v) last = v;
            put64(o, last);
        }
        placed += ref_mapped[t] + ref_unmapped[t]; mapped += ref_mapped[t];
    }
    put64(o, (uint64_t)n_no_coor);
    out.n_ref = n_ref;
    out.stats[0] = placed + n_no_coor; out.stats[1] = placed; out.stats[2] = n_runs; out.stats[3] = n_chunks; out.stats[4] = n_bins;
    out.stats[5] = n_ref ? lin_start[n_ref] : 0; out.stats[6] = n_no_coor; out.stats[7] = mapped;
    return nullptr;
}

} // namespace pcidxhost
