// The host half of the index build (pc_bam_index_finish, pc_bam_index_finish_csi): from the runs of records with one bin,
// the linear arrays (BAI) or the runs' loff (CSI) and the per-reference counts to the finished index and its bytes --
// hts_idx_finish (kent/src/htslib/hts.c:1277-1291) with update_loff's forward fill (:1193-1209; for a CSI done on the
// GPU) and compress_binning (:1230-1275), then the layout of hts_idx_save (:1395-1457, 1484-1499; SAM specification 5.2,
// 5.3).  No GPU call: the kernels of index_kernels.hip.h, or a test, supply the inputs.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <utility>
#include <vector>

#include "index_shape.h"

struct pc_bam_index {
    int32_t n_ref = 0;
    std::vector<uint8_t> bytes;   // the .bai file, or the payload of the .csi file (what its BGZF members inflate to)
    // records, placed records, runs before the finish, chunks after it, bins, linear entries (CSI: windows held on the device), n_no_coor, mapped
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // upload, inflate, chain, fields, index kernels, read-back, host finish, total
    double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

namespace pcidxhost {

typedef std::pair<uint64_t, uint64_t> Chunk;
struct Bin { uint32_t id; bool alive; std::vector<Chunk> chunks; uint64_t loff; };

constexpr uint32_t kMetaBin = 37450u;          // BAI: n_bins + 1 of 5 levels
using pcshape::kBaiLvls;
using pcshape::level_first;
using pcshape::bin_count;
constexpr uint64_t kMinMarkerDist = 0x10000;   // HTS_MIN_MARKER_DIST: a bin that spans fewer BGZF file bytes moves into its parent


inline void put32(std::vector<uint8_t> &o, uint32_t v) { for (int k = 0; k < 4; ++k) o.push_back((uint8_t)(v >> (8 * k))); }
inline void put64(std::vector<uint8_t> &o, uint64_t v) { for (int k = 0; k < 8; ++k) o.push_back((uint8_t)(v >> (8 * k))); }

// compress_binning for one reference; `bins` ascending by id
inline void compress(std::vector<Bin> &bins, int n_lvls = kBaiLvls) {
    auto find = [&](uint32_t id) -> Bin * {
        auto it = std::lower_bound(bins.begin(), bins.end(), id, [](const Bin &b, uint32_t x) { return b.id < x; });
        return it != bins.end() && it->id == id && it->alive ? &*it : nullptr;
    };
    auto by_begin = [](const Chunk &a, const Chunk &b) { return a.first < b.first; };
    for (int l = n_lvls; l > 0; --l) {
        // (hts.c:1241 visits every bin of this level or deeper; the deeper ones that are still here stayed for a reason
        // that holds -- their span, or a parent that does not exist -- so only the level's own bins can change)
        const uint32_t lo = level_first(l), hi = level_first(l + 1);
        auto it = std::lower_bound(bins.begin(), bins.end(), lo, [](const Bin &b, uint32_t x) { return b.id < x; });
        for (; it != bins.end() && it->id < hi; ++it) {
            if (!it->alive) continue;
            std::vector<Chunk> &c = it->chunks;
            if (l < n_lvls && c.size() > 1) std::stable_sort(c.begin(), c.end(), by_begin);
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

// 0, or a message.  csi: the shape (min_shift, n_lvls) and run_loff are read, lin_start / linear are not; otherwise the reverse.
inline const char *finish_impl(bool csi, int min_shift, int n_lvls, int n_ref, int64_t n_runs, const int32_t *run_tid, const uint32_t *run_bin,
                               const uint64_t *run_beg, const uint64_t *run_end, const uint64_t *run_loff, const int64_t *lin_start, const uint64_t *linear,
                               const uint64_t *ref_beg, const uint64_t *ref_end, const int64_t *ref_mapped, const int64_t *ref_unmapped, int64_t n_no_coor,
                               pc_bam_index &out) {
    if (csi && (min_shift < 8 || min_shift > 30)) return "pc_bam_index_finish_csi: min_shift must lie in 8 .. 30";
    if (csi && (n_lvls < 0 || n_lvls > 8)) return "pc_bam_index_finish_csi: n_lvls must lie in 0 .. 8";
    if (n_ref < 0 || n_runs < 0 || n_no_coor < 0) return "pc_bam_index_finish: negative count";
    if (n_runs > 0 && (!run_tid || !run_bin || !run_beg || !run_end || (csi && !run_loff))) return "pc_bam_index_finish: NULL run array";
    if (n_ref > 0 && ((!csi && !lin_start) || !ref_beg || !ref_end || !ref_mapped || !ref_unmapped)) return "pc_bam_index_finish: NULL reference array";
    if (!csi && n_ref > 0 && (lin_start[0] != 0 || (lin_start[n_ref] > 0 && !linear))) return "pc_bam_index_finish: bad linear arrays";
    for (int t = 0; t < n_ref; ++t)
        if ((!csi && (lin_start[t + 1] < lin_start[t] || lin_start[t + 1] - lin_start[t] > ((int64_t)1 << 15))) || ref_mapped[t] < 0 || ref_unmapped[t] < 0)
            return "pc_bam_index_finish: bad linear arrays or counts";
    const uint32_t bin_limit = csi ? bin_count(n_lvls) : kMetaBin, meta_bin = csi ? bin_count(n_lvls) + 1u : kMetaBin;
    bool sorted = true;
    for (int64_t k = 0; k < n_runs; ++k) {
        if (run_tid[k] < 0 || run_tid[k] >= n_ref || run_bin[k] >= bin_limit) return "pc_bam_index_finish: run with a reference id or bin out of range";
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
    o.reserve((size_t)(32 + (csi ? 24 : 16) * n_runs + 8 * (n_ref && !csi ? lin_start[n_ref] : 0) + 56 * (int64_t)n_ref));
    if (csi) {
        o.insert(o.end(), {'C', 'S', 'I', 1});
        put32(o, (uint32_t)min_shift); put32(o, (uint32_t)n_lvls); put32(o, 0u);   // l_aux
    } else o.insert(o.end(), {'B', 'A', 'I', 1});
    put32(o, (uint32_t)n_ref);
    int64_t k = 0, n_chunks = 0, n_bins = 0, placed = 0, mapped = 0;
    std::vector<Bin> bins;
    for (int t = 0; t < n_ref; ++t) {
        bins.clear();
        for (; k < n_runs && run_tid[at(k)] == t; ++k) {
            const int64_t r = at(k);
            if (bins.empty() || bins.back().id != run_bin[r]) bins.push_back(Bin{run_bin[r], true, {}, csi ? run_loff[r] : 0});
            bins.back().chunks.emplace_back(run_beg[r], run_end[r]);
        }
        compress(bins, csi ? n_lvls : kBaiLvls);
        const bool has = ref_mapped[t] + ref_unmapped[t] > 0;
        uint32_t n_bin = has ? 1u : 0u;
        for (const Bin &b : bins) n_bin += b.alive ? 1u : 0u;
        put32(o, n_bin);
        for (const Bin &b : bins) {
            if (!b.alive) continue;
            put32(o, b.id);
            if (csi) put64(o, b.loff);
            put32(o, (uint32_t)b.chunks.size());
            for (const Chunk &c : b.chunks) { put64(o, c.first); put64(o, c.second); }
            n_chunks += (int64_t)b.chunks.size(); ++n_bins;
        }
        if (has) {
            put32(o, meta_bin);
            if (csi) put64(o, 0);
            put32(o, 2u);
            put64(o, ref_beg[t]); put64(o, ref_end[t]); put64(o, (uint64_t)ref_mapped[t]); put64(o, (uint64_t)ref_unmapped[t]);
        }
        if (!csi) {
            const int64_t n_intv = lin_start[t + 1] - lin_start[t];
            put32(o, (uint32_t)n_intv);
            uint64_t last = ref_beg[t];   // the leading windows no record covers: the offset of the reference's first record
            for (int64_t w = 0; w < n_intv; ++w) {
                const uint64_t v = linear[lin_start[t] + w];
                if (v) last = v;
                put64(o, last);
            }
        }
        placed += ref_mapped[t] + ref_unmapped[t]; mapped += ref_mapped[t];
    }
    put64(o, (uint64_t)n_no_coor);
    out.n_ref = n_ref;
    out.stats[0] = placed + n_no_coor; out.stats[1] = placed; out.stats[2] = n_runs; out.stats[3] = n_chunks; out.stats[4] = n_bins;
    out.stats[5] = n_ref && !csi ? lin_start[n_ref] : 0; out.stats[6] = n_no_coor; out.stats[7] = mapped;
    return nullptr;
}

inline const char *finish(int n_ref, int64_t n_runs, const int32_t *run_tid, const uint32_t *run_bin, const uint64_t *run_beg, const uint64_t *run_end,
                          const int64_t *lin_start, const uint64_t *linear, const uint64_t *ref_beg, const uint64_t *ref_end,
                          const int64_t *ref_mapped, const int64_t *ref_unmapped, int64_t n_no_coor, pc_bam_index &out) {
    return finish_impl(false, 14, kBaiLvls, n_ref, n_runs, run_tid, run_bin, run_beg, run_end, nullptr, lin_start, linear, ref_beg, ref_end, ref_mapped,
                       ref_unmapped, n_no_coor, out);
}

// the CSI of shape (min_shift, n_lvls); run_loff: per run the loff of its bin (the runs of one bin carry one value)
inline const char *finish_csi(int min_shift, int n_lvls, int n_ref, int64_t n_runs, const int32_t *run_tid, const uint32_t *run_bin, const uint64_t *run_beg,
                              const uint64_t *run_end, const uint64_t *run_loff, const uint64_t *ref_beg, const uint64_t *ref_end,
                              const int64_t *ref_mapped, const int64_t *ref_unmapped, int64_t n_no_coor, pc_bam_index &out) {
    return finish_impl(true, min_shift, n_lvls, n_ref, n_runs, run_tid, run_bin, run_beg, run_end, run_loff, nullptr, nullptr, ref_beg, ref_end, ref_mapped,
                       ref_unmapped, n_no_coor, out);
}

} // namespace pcidxhost
