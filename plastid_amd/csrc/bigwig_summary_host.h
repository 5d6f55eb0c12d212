// bigwig_summary_host.h -- BINNED SUMMARIES of a bigWig file, the model: what the summary reader of Kent's library
// (bigWigSummaryArray: kent/src/lib/bbiRead.c:18-40 and :405-760, bwgQuery.c:155-287 and :364-394, hmmstats.c:33-46) gives,
// restated, bit for bit.  The functions below that carry PC_BW_HD are the ones the kernels of bigwig_summary_kernels.hip.h
// call: the device runs the model's arithmetic.  Every product and every sum is a statement of its own, so the order of
// the operations does not hang on -ffp-contract.
// A query is (chromId, start, end, n_bins), start < end < 2^31, n_bins >= 1.
//   1. LEVEL (choose_level): want = ((end - start) / n_bins) / 2; want <= 1: the items; otherwise the level with the
//      greatest reduction <= want (the first of equals in header order), the items when there is none.
//   2. BIN EDGES (bin_edge): e_i = start + (uint64)(end - start) (i + 1) / n_bins; bin i is [e_(i-1), e_i), e_(-1) = start.
//   3. FROM A LEVEL (slice): the records of the chromId in file order; the walk of a bin begins at the first record with
//      end > binStart and goes on while start < binEnd; min and max start from the record the walk begins at; a record with
//      overlap > 0 adds f = overlap / (end - start) of its validCount, sum and sum of squares (the float32 fields widened
//      first); count > 0: valid = (uint32)ceil(count), norm = valid / count, the sums times norm; otherwise no data.
//   4. FROM THE ITEMS (slice): the items of the contig in file order, each CLIPPED to [start, end); an empty bin is one
//      position wide; size: the clipped length, f = overlap / size, w = size f; count += w, sum += val w, sumsq += val val
//      w; the element as in 3 without the guard -- 0 / 0 gives valid = 0, which reads as no data.
//   5. VALUES (value_of): mean = sum / valid; min, max; coverage = (n_bins / (end - start)) valid; std = sqrt(v), v =
//      sumsq - sum sum / valid, over valid - 1 when valid > 1.  A bin with valid = 0 has no data: the caller's fill.
// "The first record with end > binStart" is a position in Kent's list.  It is a SEARCH here (first_end_above), which is
// the same thing only where starts and ends do not decrease within a contig and a contig's records stand together --
// true of every level and every item list Kent's writer and ours produce.  index_table checks it once per table; a table
// that fails is not summarized (kOrderText).  A record with end <= start or a chromId outside the tree fails it too.
// An element without data is all zeros here (Kent leaves the items' path with NaN sums there and reads only valid).
// A count of 2^32 or more gives valid = 2^32 - 1 (Kent's cast is undefined there).
// Plain C++17, HIP-free: tests/bigwig_summary_host_test.cpp compiles it under the sanitizers.
#pragma once
#include <cmath>

#include "bigwig_write_host.h"

namespace pcbws {

struct ZoomRec { uint32_t chrom, start, end, valid; float mn, mx, sum, sumsq; };     // the file's 32-byte record, as it is
struct ItemRec { uint32_t chrom, start, end; float value; };                         // one item of any section type
struct Element { uint32_t valid; double mn, mx, sum, sumsq; };
enum { kMean = 0, kMin, kMax, kCoverage, kStd, kKinds };
constexpr int kItems = -1;                   // the "level" of the items
constexpr uint32_t kMaxCoord = 0x7fffffffu;  // start < end <= this
constexpr const char *kOrderText = "summarize needs records in coordinate order";

// ---------------------------------------------------------------- rules 1 and 2
PC_BW_HD inline int choose_level(const uint32_t *reduction, int nlevels, uint32_t start, uint32_t end, uint32_t n_bins) {
    const uint32_t want = ((end - start) / n_bins) / 2u;
    if (want <= 1u) return kItems;
    int best = kItems;
    for (int k = 0; k < nlevels; ++k)
        if (reduction[k] <= want && (best < 0 || reduction[k] > reduction[best])) best = k;
    return best;
}
PC_BW_HD inline uint32_t bin_edge(uint32_t start, uint32_t end, uint32_t i, uint32_t n_bins) {
    return start + (uint32_t)((uint64_t)(end - start) * ((uint64_t)i + 1u) / (uint64_t)n_bins);
}
PC_BW_HD inline uint32_t bin_start(uint32_t start, uint32_t end, uint32_t i, uint32_t n_bins) { return i ? bin_edge(start, end, i - 1u, n_bins) : start; }

// ---------------------------------------------------------------- rules 3 and 4
// the first k of [lo, hi) with r[k].end > pos (hi: none), ends not decreasing
template <typename R> PC_BW_HD inline int64_t first_end_above(const R *r, int64_t lo, int64_t hi, uint32_t pos) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (r[mid].end > pos) hi = mid; else lo = mid + 1;
    }
    return lo;
}
PC_BW_HD inline Element no_data() { Element el; el.valid = 0u; el.mn = 0.0; el.mx = 0.0; el.sum = 0.0; el.sumsq = 0.0; return el; }
// normalizeCount of bbiRead.c
PC_BW_HD inline Element element_of(double count, double mn, double mx, double sum, double sumsq) {
    const double up = ceil(count);
    Element el;
    el.valid = up >= 4294967296.0 ? 0xffffffffu : (uint32_t)up;
    if (el.valid == 0u) return no_data();
    const double norm = (double)el.valid / count;
    el.mn = mn; el.mx = mx;
    el.sum = sum * norm;
    el.sumsq = sumsq * norm;
    return el;
}
// Bin [bs, be) of a query [qs, qe) over the records r[lo, hi) of the query's contig.
PC_BW_HD inline Element slice(const ZoomRec *r, int64_t lo, int64_t hi, uint32_t, uint32_t, uint32_t bs, uint32_t be) {
    int64_t k = first_end_above(r, lo, hi, bs);
    if (k >= hi) return no_data();
    double mn = (double)r[k].mn, mx = (double)r[k].mx, sum = 0.0, sumsq = 0.0, count = 0.0;
    for (; k < hi; ++k) {
        const ZoomRec z = r[k];
        if (z.start >= be) break;
        const int64_t overlap = (int64_t)(z.end < be ? z.end : be) - (int64_t)(z.start > bs ? z.start : bs);
        if (overlap <= 0) continue;
        const double f = (double)overlap / (double)(uint32_t)(z.end - z.start);
        const double c = (double)z.valid * f, s = (double)z.sum * f, q = (double)z.sumsq * f;
        count = count + c;
        sum = sum + s;
        sumsq = sumsq + q;
        if (mx < (double)z.mx) mx = (double)z.mx;
        if (mn > (double)z.mn) mn = (double)z.mn;
    }
    if (!(count > 0.0)) return no_data();
    return element_of(count, mn, mx, sum, sumsq);
}
PC_BW_HD inline Element slice(const ItemRec *r, int64_t lo, int64_t hi, uint32_t qs, uint32_t qe, uint32_t bs, uint32_t be) {
    if (be == bs) be = bs + 1u;
    // (an item's end is above bs iff its clipped end is: bs < qe)
    int64_t k = first_end_above(r, lo, hi, bs);
    if (k >= hi) return no_data();
    double mn = (double)r[k].value, mx = mn, sum = 0.0, sumsq = 0.0, count = 0.0;
    for (; k < hi; ++k) {
        const ItemRec it = r[k];
        const uint32_t cs = it.start > qs ? it.start : qs, ce = it.end < qe ? it.end : qe;
        if (cs >= be) break;
        const int64_t overlap = (int64_t)(ce < be ? ce : be) - (int64_t)(cs > bs ? cs : bs);
        if (overlap <= 0) continue;
        const double val = (double)it.value;
        const double size = (double)(int32_t)(ce - cs);
        const double f = (double)overlap / size;
        const double w = size * f;
        const double s = val * w, vv = val * val;
        const double q = vv * w;
        count = count + w;
        sum = sum + s;
        sumsq = sumsq + q;
        if (mx < val) mx = val;
        if (mn > val) mn = val;
    }
    return element_of(count, mn, mx, sum, sumsq);   // (0 / 0: valid = 0, no data)
}

// ---------------------------------------------------------------- rule 5
// The value of an element with valid > 0.  (sqrt is the host's: the kinds are derived from the elements there.)
inline double value_of(const Element &el, int kind, uint32_t start, uint32_t end, uint32_t n_bins) {
    const double n = (double)el.valid;
    switch (kind) {
    case kMean: return el.sum / n;
    case kMin: return el.mn;
    case kMax: return el.mx;
    case kCoverage: { const double factor = (double)n_bins / (double)(end - start); return factor * n; }
    default: {
        const double sq = el.sum * el.sum;
        const double part = sq / n;
        double v = el.sumsq - part;
        if (el.valid > 1u) v = v / (double)(el.valid - 1u);
        return sqrt(v);
    }
    }
}

// ---------------------------------------------------------------- the order check and the ranges of the contigs
// What record k says about its table, given its neighbours (the kernel k_bbi_index runs this per lane): bit 0 the table is
// not in coordinate order, bit 1 a run of its chromId begins here, bit 2 one ends here.
template <typename R> PC_BW_HD inline unsigned index_record(const R *r, int64_t n, int64_t k, uint32_t nids) {
    const R c = r[k];
    unsigned out = 0u;
    if (c.end <= c.start || c.chrom >= nids) out |= 1u;
    if (k == 0 || r[k - 1].chrom != c.chrom) out |= 2u;
    else if (c.start < r[k - 1].start || c.end < r[k - 1].end) out |= 1u;
    if (k + 1 == n || r[k + 1].chrom != c.chrom) out |= 4u;
    return out;
}
struct Ranges {
    std::vector<int64_t> lo, hi;           // by chromId: its records [lo, hi); none: 0, 0
    bool ordered = true;
};
template <typename R> inline void index_table(const R *r, int64_t n, uint32_t nids, Ranges &g) {
    g.lo.assign(nids, 0); g.hi.assign(nids, 0); g.ordered = true;
    std::vector<uint32_t> runs(nids, 0u);
    for (int64_t k = 0; k < n; ++k) {
        const unsigned what = index_record(r, n, k, nids);
        if (what & 1u) g.ordered = false;
        if (r[k].chrom >= nids) continue;
        if (what & 2u) { g.lo[r[k].chrom] = k; if (++runs[r[k].chrom] > 1u) g.ordered = false; }
        if (what & 4u) g.hi[r[k].chrom] = k + 1;
    }
}

// ---------------------------------------------------------------- the blocks of a level
// The blocks of level `level` in the order of its R-tree's walk, checked as read_zoom_level checks them, into a BigWig
// that holds nothing else (blocks, data_lo / data_hi, uncompress_buf): what the inflate of the device import takes.
inline std::string level_blocks(const uint8_t *image, uint64_t size, uint32_t uncompress_buf, const std::vector<pcbww::ZoomHeader> &levels, int64_t level, pcbw::BigWig &out) {
    out = pcbw::BigWig();
    if (level < 0 || level >= (int64_t)levels.size()) return "zoom level " + std::to_string(level) + " of " + std::to_string(levels.size());
    const pcbww::ZoomHeader &z = levels[(size_t)level];
    const std::string lvl = "zoom level " + std::to_string(level) + ": ";
    if (uncompress_buf > pcbw::kMaxInflated) return pcbw::defect_text(pcbw::kBwBufSize);
    out.uncompress_buf = uncompress_buf;
    pcbw::detail::Walk w{image, size};
    if (pcbw::rd64(image + z.index + 8) != 0) pcbw::detail::walk_index(w, z.index + 48, 0, out);
    if (w.defect == pcbw::kBwIndexNodeOutside) return lvl + "a node of the index lies outside the file";
    if (w.defect) return lvl + pcbw::defect_text(w.defect);
    if (out.blocks.size() >= ((size_t)1 << 31) - 1) return lvl + pcbw::defect_text(pcbw::kBwTreeNodes);
    out.data_lo = out.blocks.empty() ? 0 : ~(uint64_t)0;
    for (size_t b = 0; b < out.blocks.size(); ++b) {
        pcbw::Block &k = out.blocks[b];
        const std::string blk = lvl + "block " + std::to_string(b) + ": ";
        if (!w.inside(k.off, k.size)) return blk + pcbw::defect_text(pcbw::kBwBlockOutside);
        if (k.size > (uncompress_buf ? pcbw::kMaxBlockBytes : (uint64_t)pcbw::kMaxInflated)) return blk + pcbw::defect_text(pcbw::kBwBlockLarge);
        if (uncompress_buf) {
            const uint8_t *p = image + k.off;
            if (k.size < 6 || (p[0] & 15u) != 8u || (p[0] >> 4) > 7u || (((uint32_t)p[0] << 8) | p[1]) % 31u != 0u || (p[1] & 0x20u)) return blk + pcbw::defect_text(pcbw::kBwZlibHeader);
            const uint8_t *t = p + k.size - 4;
            k.adler = ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | (uint32_t)t[3];
        } else if (k.size % pcbww::kZoomRecordBytes != 0u) return blk + "not a whole number of 32-byte records";
        if (k.off < out.data_lo) out.data_lo = k.off;
        if (k.off + k.size > out.data_hi) out.data_hi = k.off + k.size;
    }
    return std::string();
}

// ---------------------------------------------------------------- the serial model over a file image
// One table: the records of a level, or the items (level kItems), with the ranges of its contigs.
struct HostTable {
    bool loaded = false;
    std::vector<ZoomRec> zoom;
    std::vector<ItemRec> items;
    Ranges ranges;
    int64_t queries = 0;
};
// The host's reader of a file: tables are read when a query first selects them.  Every function returns what is wrong
// (empty: nothing), to stand behind "<path>: bigWig: ".
struct HostSummary {
    const uint8_t *image = nullptr;
    uint64_t size = 0;
    pcbw::BigWig f;
    std::vector<pcbww::ZoomHeader> levels;
    std::vector<uint32_t> reduction;
    std::vector<HostTable> tables;         // [0] the items, [1 + k] level k

    std::string open(const uint8_t *image_, uint64_t size_) {
        image = image_; size = size_;
        const unsigned long long d = pcbw::parse(image, size, f);
        if (d != pcbw::kNoDefect) {
            // (defect_message's text behind its "<path>: bigWig: ")
            const std::string m = pcbw::defect_message("", d);
            return m.substr(m.find("bigWig: ") + 8);
        }
        const std::string bad = pcbww::zoom_headers(image, size, levels);
        if (!bad.empty()) return bad;
        reduction.clear();
        for (const pcbww::ZoomHeader &z : levels) reduction.push_back(z.reduction);
        tables.assign(levels.size() + 1, HostTable());
        return std::string();
    }
    template <typename Inflate> std::string load(int level, Inflate inflate) {
        HostTable &t = tables[(size_t)(level + 1)];
        if (t.loaded) return std::string();
        const uint32_t nids = (uint32_t)f.of_id.size();
        if (level == kItems) {
            pcbw::ItemTable it;
            pcbw::read_items(image, size, inflate, it);
            if (it.defect != pcbw::kNoDefect) {
                const std::string m = pcbw::defect_message("", it.defect);
                return m.substr(m.find("bigWig: ") + 8);
            }
            t.items.resize(it.chrom.size());
            for (size_t k = 0; k < it.chrom.size(); ++k)
                t.items[k] = ItemRec{f.chroms[(size_t)it.chrom[k]].id, (uint32_t)it.start[k], (uint32_t)it.stop[k], (float)it.value[k]};
            index_table(t.items.data(), (int64_t)t.items.size(), nids, t.ranges);
        } else {
            pcbww::ZoomTable zt;
            const std::string bad = pcbww::read_zoom_level(image, size, f.uncompress_buf, levels, level, inflate, zt);
            if (!bad.empty()) return bad;
            t.zoom.resize(zt.chrom.size());
            for (size_t k = 0; k < zt.chrom.size(); ++k) t.zoom[k] = ZoomRec{zt.chrom[k], zt.start[k], zt.end[k], zt.valid[k], zt.mn[k], zt.mx[k], zt.sum[k], zt.sumsq[k]};
            index_table(t.zoom.data(), (int64_t)t.zoom.size(), nids, t.ranges);
        }
        t.loaded = true;
        return std::string();
    }
    // nq queries of n_bins bins each: contig[q] the place in f.chroms (-1: the file lacks it: no data), into
    // out[q * n_bins + bin].
    template <typename Inflate> std::string summarize(int64_t nq, const int32_t *contig, const uint32_t *start, const uint32_t *end, uint32_t n_bins, Inflate inflate, Element *out) {
        for (int64_t q = 0; q < nq; ++q) {
            Element *o = out + q * (int64_t)n_bins;
            for (uint32_t i = 0; i < n_bins; ++i) o[i] = no_data();
            if (contig[q] < 0 || contig[q] >= (int32_t)f.chroms.size()) continue;
            const int level = choose_level(reduction.data(), (int)reduction.size(), start[q], end[q], n_bins);
            const std::string bad = load(level, inflate);
            if (!bad.empty()) return bad;
            HostTable &t = tables[(size_t)(level + 1)];
            if (!t.ranges.ordered) return kOrderText;
            t.queries += 1;
            const uint32_t id = f.chroms[(size_t)contig[q]].id;
            const int64_t lo = t.ranges.lo[id], hi = t.ranges.hi[id];
            for (uint32_t i = 0; i < n_bins; ++i) {
                const uint32_t bs = bin_start(start[q], end[q], i, n_bins), be = bin_edge(start[q], end[q], i, n_bins);
                o[i] = level == kItems ? slice(t.items.data(), lo, hi, start[q], end[q], bs, be) : slice(t.zoom.data(), lo, hi, start[q], end[q], bs, be);
            }
        }
        return std::string();
    }
};

// what is wrong with the arguments of a query (empty: nothing)
inline std::string check_queries(int64_t nq, const int64_t *start, const int64_t *end, int64_t n_bins) {
    if (n_bins < 1 || n_bins > (int64_t)kMaxCoord) return "n_bins " + std::to_string(n_bins) + " is not in 1 .. 2^31 - 1";
    for (int64_t q = 0; q < nq; ++q) {
        if (start[q] < 0 || end[q] > (int64_t)kMaxCoord || start[q] > (int64_t)kMaxCoord) return "query " + std::to_string(q) + ": a coordinate below 0 or at or beyond 2^31";
        if (start[q] >= end[q]) return "query " + std::to_string(q) + ": start >= end";
    }
    return std::string();
}

}   // namespace pcbws
