// bigwig_write_host.h -- WRITING bigWig files (revision 21), host side: what the host writer (bam_stager.cpp,
// pb_bigwig_write_*) and the device export (bigwig_writer.hip.h, pc_track_export_bigwig) share.  HIP-free.
//   - which cells are written and how they group into items (written, same_item; the kernels compile them);
//   - the 24-byte section header (put_section_header; the kernels compile it);
//   - the total summary and the order its minimum and maximum are taken in (float_key);
//   - THE CONTAINER around the blocks (build_container): little-endian, version 4, laid out as
//     tests/bigwig_writer.py lays its files out, which Kent's readers read:
//       64-byte header | 24 bytes per zoom level | total summary (40 bytes, when the file has items) | chromosome B+ tree |
//       u64 section count | the blocks back to back | R-tree (48-byte header, bulk-loaded over the sections in file order) |
//       per zoom level: u32 record count, its blocks back to back, its R-tree | the magic;
//   - ZOOM LEVELS (below: "zoom levels"): the per-window functions, which the kernels compile, the plan of the window
//     grid, the 32-byte record, and the reader of a level (zoom_headers, read_zoom_level);
//   - the serial writer over one contig's cells at a time (HostWriter), which is the model of the device export.
// Cells: a cell is written iff its value != 0.0 (NaN is, -0.0 is not).  Neighbouring written cells of one contig form one
// item while their float64 values compare equal (a NaN is an item of its own); the value is cast to float32
// round-to-nearest-even AFTERWARDS, so two doubles that cast alike stay two items.  Every items_per_slot consecutive items
// of a contig make one bedGraph section (type 1); sections never span contigs.  Contigs stand in the sorted order of
// their names (bytes), the chromosome id is the place in it, and every contig is in the tree, with or without items.
// Not written: variableStep / fixedStep sections, bigBed, byte-swapped files; nothing is appended to a file.
//
// ZOOM LEVELS (zoom != 0; zoom == 0 writes zoomLevels = 0 and today's bytes).  Kent's reducer (bbiWrite.c) starts its
// windows where the data does; here windows lie on a FIXED GRID, so that every window is a function of the items alone
// and the device gives the serial model's bytes.  Kent's readers take either.
//   - Reductions: r_k = r0 x 4^k, at most 10 levels, r_k <= 2^30.  r0 is given (8 .. 2^24) or automatic:
//     r0 = 4 x max(10, V / N) capped at 2^20, N the file's items and V its total validCount (integer division).
//   - Window w of level k on a contig covers [w r_k, min((w + 1) r_k, size)); a contig has ceil(size / r_k) of them.
//   - Level 0 comes from the ITEMS (their float32 values, in the order of the contig): a window takes its overlap o with
//     every item: valid += o, sum = sum + v o, sumsq = sumsq + v v o in float64 with v = (double)value (summary_add's
//     formulas); min and max through float_key, NaN takes no part (no number at all: both are NaN).
//   - Level k + 1 comes from level k's float64 accumulators, not from the rounded records: the four children 4w .. 4w + 3
//     of the same contig in order, the empty ones (valid == 0, or beyond the contig's last window) skipped: the first
//     that is not empty is taken as it is, every later one is added to it: valid exactly, min and max by key,
//     sum = sum + child's sum, sumsq likewise -- ((c0 + c1) + c2) + c3.
//   - A window yields a record iff valid > 0.  A record is 32 bytes: chromId, start, end, validCount u32, then minVal,
//     maxVal, sumData, sumSquares f32.  The casts to float32 happen here alone, round to nearest even; a NaN sum is
//     written as 0x7fc00000, and so are min and max when no value is a number.
//   - Level 0 is written whenever the file has items; level k >= 1 iff it has fewer records than level k - 1; the first
//     that has not ends the pyramid.  A file without items has no levels and is the zoom == 0 file.
//   - Records stand in (chromId, start) order.  Every min(items_per_slot, 768) consecutive records of a contig form one
//     block (768 x 32 bytes is within the encoder's 24 600-byte input); blocks never span contigs.  A block is stored, or
//     goes through the encoder in the mode of the data sections.  uncompressBufSize is the largest raw section or block.
//   - The zoom header of level k at 64 + 24 k: reductionLevel u32, reserved u32, dataOffset u64 (the u32 record count),
//     indexOffset u64 (the level's R-tree, of the same form and fan-out as the unzoomed one).
//   - Refused (zoom_plan): a window grid of 2^31 - 1 windows or more over all levels (the scans count in int).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "bigwig_host.h"
#include "deflate_host.h"

namespace pcbww {

constexpr uint32_t kMaxItemsPerSlot = 2048u;   // 24 + 2 048 x 12 bytes: the largest input of the encoder
constexpr uint32_t kMinBlockSize = 2u, kMaxBlockSize = 65535u;   // a node counts its children in 16 bits
constexpr uint32_t kSummaryBytes = 40u, kItemBytes = 12u;

PC_BW_HD inline bool written(double v) { return v != 0.0; }
PC_BW_HD inline bool same_item(double a, double b) { return a == b; }

PC_BW_HD inline void put16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
PC_BW_HD inline void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
PC_BW_HD inline void put64(uint8_t *p, uint64_t v) { put32(p, (uint32_t)v); put32(p + 4, (uint32_t)(v >> 32)); }
PC_BW_HD inline uint32_t float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
PC_BW_HD inline float bits_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
PC_BW_HD inline uint64_t double_bits(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }

// chromId, first start, last end, itemStep 0, itemSpan 0, type 1, reserved 0, u16 itemCount
PC_BW_HD inline void put_section_header(uint8_t *p, uint32_t chrom, uint32_t start, uint32_t end, uint32_t count) {
    put32(p, chrom); put32(p + 4, start); put32(p + 8, end); put32(p + 12, 0u); put32(p + 16, 0u);
    p[20] = 1u; p[21] = 0u; put16(p + 22, count);
}
PC_BW_HD inline void put_item(uint8_t *p, uint32_t start, uint32_t end, float value) { put32(p, start); put32(p + 4, end); put32(p + 8, float_bits(value)); }

// The order the summary's minimum and maximum are taken in: a total order of the float32 values that are not NaN
// (-0.0 below +0.0), so that the result does not depend on the order of a reduction.  NaN takes no part (kNoKey).
constexpr uint32_t kNoKeyMin = 0xffffffffu, kNoKeyMax = 0u;
PC_BW_HD inline bool float_is_nan(float f) { return f != f; }
PC_BW_HD inline uint32_t float_key(float f) {
    const uint32_t u = float_bits(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
PC_BW_HD inline float key_float(uint32_t k) { return bits_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// validCount = sum of (end - start); min and max of the float32 values (NaN: when no value is a number); sumData = sum of
// value x (end - start), sumSquares = sum of value^2 x (end - start), in float64 over the float32 values
struct Summary {
    uint64_t valid = 0;
    uint32_t kmin = kNoKeyMin, kmax = kNoKeyMax;
    double sum = 0.0, sumsq = 0.0;
};
PC_BW_HD inline void summary_add(Summary &s, uint32_t start, uint32_t end, float value) {
    const double w = (double)(end - start), v = (double)value;
    s.valid += (uint64_t)(end - start);
    if (!float_is_nan(value)) {
        const uint32_t k = float_key(value);
        if (k < s.kmin) s.kmin = k;
        if (k > s.kmax) s.kmax = k;
    }
    s.sum = s.sum + v * w; s.sumsq = s.sumsq + v * v * w;
}
inline void put_summary(uint8_t *p, const Summary &s) {
    const double nan = bits_float(0x7fc00000u);
    const double mn = s.kmin == kNoKeyMin ? nan : (double)key_float(s.kmin), mx = s.kmax == kNoKeyMax ? nan : (double)key_float(s.kmax);
    put64(p, s.valid); put64(p + 8, double_bits(mn)); put64(p + 16, double_bits(mx)); put64(p + 24, double_bits(s.sum)); put64(p + 32, double_bits(s.sumsq));
}

// what is refused before anything is built; empty: nothing
inline std::string check_params(int64_t items_per_slot, int64_t block_size) {
    if (items_per_slot < 1 || items_per_slot > (int64_t)kMaxItemsPerSlot) return "items_per_slot outside 1 .. 2048";
    if (block_size < (int64_t)kMinBlockSize || block_size > (int64_t)kMaxBlockSize) return "block_size outside 2 .. 65535";
    return std::string();
}

struct WContig { std::string name; uint32_t size; };                 // in sorted order: the id is the place
struct WSection { uint32_t chrom, start, end; uint64_t size; };      // size: the bytes of its block in the file

// ---------------------------------------------------------------- zoom levels: windows and records (host and device)
constexpr int kZoomMaxLevels = 10;
constexpr int64_t kZoomNone = 0, kZoomAuto = -1, kZoomMinFirst = 8, kZoomMaxFirst = (int64_t)1 << 24;
constexpr uint32_t kZoomMaxReduction = 1u << 30, kZoomAutoCap = 1u << 20;
constexpr uint32_t kZoomRecordBytes = 32u, kZoomMaxBlockRecords = 768u, kZoomHeaderBytes = 24u, kZoomNanBits = 0x7fc00000u;

inline std::string check_zoom(int64_t zoom) {
    if (zoom == kZoomNone || zoom == kZoomAuto || (zoom >= kZoomMinFirst && zoom <= kZoomMaxFirst)) return std::string();
    return "zoom is none of 0 (no zoom levels), -1 (automatic), 8 .. 16777216 (the first reduction)";
}
// r0 of a file of `items` items (> 0) that cover `valid` positions
inline uint32_t zoom_first_reduction(int64_t zoom, uint64_t items, uint64_t valid) {
    if (zoom > 0) return (uint32_t)zoom;
    const uint64_t r = 4u * std::max<uint64_t>(10u, items ? valid / items : 0u);
    return (uint32_t)std::min<uint64_t>(r, kZoomAutoCap);
}
inline uint32_t zoom_block_records(uint32_t items_per_slot) { return std::min(items_per_slot, kZoomMaxBlockRecords); }

// what a window has gathered; a window's width is at most 2^30, so valid fits 32 bits
struct ZoomAcc {
    uint32_t valid = 0, kmin = kNoKeyMin, kmax = kNoKeyMax;
    double sum = 0.0, sumsq = 0.0;
};
// an item of `value` overlaps the window in o > 0 positions
PC_BW_HD inline void zoom_add_overlap(ZoomAcc &a, uint32_t o, float value) {
    const double w = (double)o, v = (double)value;
    a.valid += o;
    if (!float_is_nan(value)) {
        const uint32_t k = float_key(value);
        if (k < a.kmin) a.kmin = k;
        if (k > a.kmax) a.kmax = k;
    }
    a.sum = a.sum + v * w; a.sumsq = a.sumsq + v * v * w;
}
// Window [ws, we) of level 0 over the items [lo, hi) of its contig (sorted, disjoint): the first item whose end lies
// beyond ws by bisection, then the items in order while they start in front of we.
PC_BW_HD inline ZoomAcc zoom_window0(const uint32_t *item_start, const uint32_t *item_end, const float *item_value, int64_t lo, int64_t hi, uint32_t ws, uint32_t we) {
    int64_t a = lo, b = hi;
    while (a < b) {
        const int64_t m = a + (b - a) / 2;
        if (item_end[m] > ws) b = m; else a = m + 1;
    }
    ZoomAcc acc;
    for (int64_t i = a; i < hi && item_start[i] < we; ++i) {
        const uint32_t s = item_start[i] > ws ? item_start[i] : ws, e = item_end[i] < we ? item_end[i] : we;
        zoom_add_overlap(acc, e - s, item_value[i]);
    }
    return acc;
}
// the next child of a parent window, in order
PC_BW_HD inline void zoom_merge(ZoomAcc &p, const ZoomAcc &c) {
    if (c.valid == 0u) return;
    if (p.valid == 0u) { p = c; return; }
    p.valid += c.valid;
    if (c.kmin < p.kmin) p.kmin = c.kmin;
    if (c.kmax > p.kmax) p.kmax = c.kmax;
    p.sum = p.sum + c.sum; p.sumsq = p.sumsq + c.sumsq;
}
PC_BW_HD inline uint32_t zoom_cast(double d) { return d != d ? kZoomNanBits : float_bits((float)d); }
// the record's eight little-endian words
PC_BW_HD inline void zoom_record_words(uint32_t *w, uint32_t chrom, uint32_t start, uint32_t end, const ZoomAcc &a) {
    w[0] = chrom; w[1] = start; w[2] = end; w[3] = a.valid;
    w[4] = a.kmin == kNoKeyMin ? kZoomNanBits : float_bits(key_float(a.kmin));
    w[5] = a.kmax == kNoKeyMax ? kZoomNanBits : float_bits(key_float(a.kmax));
    w[6] = zoom_cast(a.sum); w[7] = zoom_cast(a.sumsq);
}
PC_BW_HD inline void put_zoom_record(uint8_t *p, uint32_t chrom, uint32_t start, uint32_t end, const ZoomAcc &a) {
    uint32_t w[8];
    zoom_record_words(w, chrom, start, end, a);
    for (int k = 0; k < 8; ++k) put32(p + 4 * k, w[k]);
}

// The window grid of all candidate levels.  Windows are numbered over all levels: level k starts at level_off[k], and
// within it the contigs stand in order, contig c at row(k)[c] (row(k)[K] == level_off[k + 1]).
struct ZoomGrid {
    int levels, K;
    uint32_t r[kZoomMaxLevels];
    int64_t level_off[kZoomMaxLevels + 1];
};
// the level of window p < level_off[levels]
PC_BW_HD inline int zoom_level_of(const ZoomGrid &g, int64_t p) {
    int k = 0;
    while (k + 1 < g.levels && p >= g.level_off[k + 1]) ++k;
    return k;
}
// the contig of window p of a level whose row is `row`: the last c < K with row[c] <= p (a contig without windows never is)
PC_BW_HD inline int zoom_contig_of(const int64_t *row, int K, int64_t p) {
    int a = 0, b = K - 1;
    while (a < b) {
        const int m = a + (b - a + 1) / 2;
        if (row[m] <= p) a = m; else b = m - 1;
    }
    return a;
}
PC_BW_HD inline int64_t zoom_windows(uint32_t size, uint32_t r) { return (int64_t)(((uint64_t)size + r - 1u) / r); }

struct ZoomPlan {
    ZoomGrid g;
    std::vector<int64_t> rows;     // levels x (K + 1)
    const int64_t *row(int k) const { return rows.data() + (size_t)k * (size_t)(g.K + 1); }
    int64_t windows() const { return g.level_off[g.levels]; }
};
// empty, or what is refused
inline std::string zoom_plan(const std::vector<WContig> &contigs, uint32_t r0, ZoomPlan &z) {
    z.g.levels = 0; z.g.K = (int)contigs.size();
    for (uint64_t r = r0; z.g.levels < kZoomMaxLevels && r <= kZoomMaxReduction; r *= 4u) z.g.r[z.g.levels++] = (uint32_t)r;
    for (int k = z.g.levels; k < kZoomMaxLevels; ++k) z.g.r[k] = 0u;
    z.rows.assign((size_t)z.g.levels * (size_t)(z.g.K + 1), 0);
    int64_t at = 0;
    for (int k = 0; k < z.g.levels; ++k) {
        z.g.level_off[k] = at;
        for (int c = 0; c < z.g.K; ++c) {
            z.rows[(size_t)k * (size_t)(z.g.K + 1) + (size_t)c] = at;
            at += zoom_windows(contigs[(size_t)c].size, z.g.r[k]);
            if (at >= (int64_t)0x7ffffffe) return "zoom: 2^31 - 2 windows or more over the levels at a first reduction of " + std::to_string(r0) + ": the windows are counted in 31 bits";
        }
        z.rows[(size_t)k * (size_t)(z.g.K + 1) + (size_t)z.g.K] = at;
    }
    for (int k = z.g.levels; k <= kZoomMaxLevels; ++k) z.g.level_off[k] = at;
    return std::string();
}
// The levels that are written, from the records in front of every (level, contig) -- rec[k (K + 1) + c], counted over
// all levels, rec[k (K + 1) + K]: those in front of level k + 1 -- : level 0, then every level with fewer records than
// the one below it.
inline int zoom_levels_written(const ZoomPlan &z, const std::vector<int64_t> &rec) {
    const size_t row = (size_t)z.g.K + 1;
    int n = 0;
    int64_t below = 0;
    for (int k = 0; k < z.g.levels; ++k) {
        const int64_t have = rec[(size_t)k * row + row - 1] - rec[(size_t)k * row];
        if (k > 0 && have >= below) break;
        below = have; ++n;
    }
    return n;
}
// a block of a level: its contig, its records, the first of them (counted over all levels)
struct ZoomBlock { uint32_t chrom, count; uint64_t first; };
inline void zoom_cut_blocks(const ZoomPlan &z, const std::vector<int64_t> &rec, int k, uint32_t per_block, std::vector<ZoomBlock> &out) {
    const size_t row = (size_t)z.g.K + 1;
    for (int c = 0; c < z.g.K; ++c) {
        const int64_t first = rec[(size_t)k * row + (size_t)c], cnt = rec[(size_t)k * row + (size_t)c + 1] - first;
        for (int64_t a = 0; a < cnt; a += per_block) out.push_back({(uint32_t)c, (uint32_t)std::min<int64_t>(per_block, cnt - a), (uint64_t)(first + a)});
    }
}

// ---------------------------------------------------------------- the container
// A tree over n leaves with at most `fanout` items per node, root first, level by level, every node `isLeaf u8, reserved
// u8, count u16` and its items; the first node stands at first_offset.  leaf(i, dst) writes leaf i's item of leaf_size
// bytes; node(lo, hi, child_offset, dst) the item of node_size bytes of a child that holds leaves [lo, hi).
template <typename Leaf, typename Node> void write_tree(std::vector<uint8_t> &out, uint64_t n, uint32_t fanout, size_t leaf_size, size_t node_size,
                                                        uint64_t first_offset, Leaf leaf, Node node) {
    if (n == 0) return;
    const uint64_t f = fanout < 1u ? 1u : fanout;
    std::vector<uint64_t> cnt{(n + f - 1) / f}, span{f};      // from the leaf level up: nodes, leaves under a full node
    while (cnt.back() > 1) { cnt.push_back((cnt.back() + f - 1) / f); span.push_back(span.back() * f); }
    const int L = (int)cnt.size();
    std::vector<uint64_t> base((size_t)L);                      // where every level starts in the file
    uint64_t at = first_offset;
    for (int j = L - 1; j >= 0; --j) {
        base[(size_t)j] = at;
        at += 4u * cnt[(size_t)j] + (j == 0 ? leaf_size * n : node_size * cnt[(size_t)j - 1]);
    }
    const size_t out0 = out.size();
    out.resize(out0 + (size_t)(at - first_offset));
    uint8_t *p = out.data() + out0;
    for (int j = L - 1; j >= 0; --j) {
        const uint64_t below = j == 0 ? n : cnt[(size_t)j - 1];
        const size_t item = j == 0 ? leaf_size : node_size;
        for (uint64_t k = 0; k < cnt[(size_t)j]; ++k) {
            const uint64_t c0 = k * f, c1 = std::min(below, c0 + f);
            p[0] = j == 0 ? 1u : 0u; p[1] = 0u; put16(p + 2, (uint32_t)(c1 - c0));
            p += 4;
            for (uint64_t c = c0; c < c1; ++c, p += item) {
                if (j == 0) leaf(c, p);
                else node(c * span[(size_t)j - 1], std::min(n, (c + 1) * span[(size_t)j - 1]), base[(size_t)j - 1] + c * (4u + f * (j == 1 ? leaf_size : node_size)), p);
            }
        }
    }
}

// The R-tree at `index` over sections whose blocks stand back to back from first_block on: the 48-byte header and the nodes.
inline void write_rtree(std::vector<uint8_t> &out, const std::vector<WSection> &sections, uint32_t block_size, uint64_t index, uint64_t first_block) {
    std::vector<uint64_t> off(sections.size());
    uint64_t at = first_block;
    for (size_t s = 0; s < sections.size(); ++s) { off[s] = at; at += sections[s].size; }
    // the bounds of sections [lo, hi): the lowest (chrom, start) and the highest (chrom, end)
    auto bounds = [&](uint64_t lo, uint64_t hi, uint8_t *p) {
        uint64_t a = ~0ull, b = 0;
        for (uint64_t s = lo; s < hi; ++s) {
            a = std::min(a, ((uint64_t)sections[(size_t)s].chrom << 32) | sections[(size_t)s].start);
            b = std::max(b, ((uint64_t)sections[(size_t)s].chrom << 32) | sections[(size_t)s].end);
        }
        if (lo >= hi) a = 0;
        put32(p, (uint32_t)(a >> 32)); put32(p + 4, (uint32_t)a); put32(p + 8, (uint32_t)(b >> 32)); put32(p + 12, (uint32_t)b);
    };
    out.assign(48, 0);
    put32(out.data(), pcbw::kCirMagic); put32(out.data() + 4, block_size); put64(out.data() + 8, (uint64_t)sections.size());
    bounds(0, (uint64_t)sections.size(), out.data() + 16);
    put64(out.data() + 32, index); put32(out.data() + 40, 1u);
    write_tree(out, (uint64_t)sections.size(), block_size, 32, 24, index + 48,
               [&](uint64_t i, uint8_t *p) { bounds(i, i + 1, p); put64(p + 16, off[(size_t)i]); put64(p + 24, sections[(size_t)i].size); },
               [&](uint64_t lo, uint64_t hi, uint64_t child, uint8_t *p) { bounds(lo, hi, p); put64(p + 16, child); });
}

// What stands in front of the blocks (header, zoom headers, summary, chromosome tree, section count) and behind them
// (R-tree), and for every zoom level what stands in front of its blocks (the record count) and behind them (its R-tree);
// the magic ends the last piece.  The file is front | blocks | back | { zoom.front | its blocks | zoom.back }.
// summary: null for a file without items (totalSummaryOffset = 0).  uncompress_buf: the largest raw section or zoom block, 0: stored blocks.
struct ZoomLevel { uint32_t reduction; uint64_t records; std::vector<WSection> blocks; };
struct ZoomPiece { std::vector<uint8_t> front, back; uint64_t data_offset = 0, index_offset = 0, block_bytes = 0; };
struct Container {
    std::vector<uint8_t> front, back;
    uint64_t block_bytes = 0;
    std::vector<ZoomPiece> zoom;
    uint64_t total() const {
        uint64_t n = front.size() + block_bytes + back.size();
        for (const ZoomPiece &z : zoom) n += z.front.size() + z.block_bytes + z.back.size();
        return n;
    }
};
inline void build_container(const std::vector<WContig> &contigs, const std::vector<WSection> &sections, uint32_t block_size, uint32_t uncompress_buf,
                            const Summary *summary, Container &c, const std::vector<ZoomLevel> &zoom = std::vector<ZoomLevel>()) {
    const uint64_t zoom_bytes = (uint64_t)kZoomHeaderBytes * zoom.size();
    const uint64_t summary_off = summary ? 64u + zoom_bytes : 0u, chrom_tree = 64u + zoom_bytes + (summary ? kSummaryBytes : 0u);
    size_t key = 1;
    for (const WContig &g : contigs) key = std::max(key, g.name.size());
    const uint32_t chrom_fan = (uint32_t)std::max<size_t>(1, std::min<size_t>(block_size, contigs.size()));
    std::vector<uint8_t> tree(32, 0);
    put32(tree.data(), pcbw::kBptMagic); put32(tree.data() + 4, chrom_fan); put32(tree.data() + 8, (uint32_t)key); put32(tree.data() + 12, 8u);
    put64(tree.data() + 16, (uint64_t)contigs.size());
    write_tree(tree, (uint64_t)contigs.size(), chrom_fan, key + 8, key + 8, chrom_tree + 32,
               [&](uint64_t i, uint8_t *p) {
                   memset(p, 0, key); memcpy(p, contigs[(size_t)i].name.data(), contigs[(size_t)i].name.size());
                   put32(p + key, (uint32_t)i); put32(p + key + 4, contigs[(size_t)i].size);
               },
               [&](uint64_t lo, uint64_t, uint64_t child, uint8_t *p) {
                   memset(p, 0, key); memcpy(p, contigs[(size_t)lo].name.data(), contigs[(size_t)lo].name.size());
                   put64(p + key, child);
               });
    const uint64_t data = chrom_tree + tree.size();
    uint64_t index = data + 8;
    for (const WSection &s : sections) index += s.size;
    c.block_bytes = index - (data + 8);
    c.front.assign(64 + (size_t)zoom_bytes, 0);
    put32(c.front.data(), pcbw::kBigWigMagic); put16(c.front.data() + 4, 4u); put16(c.front.data() + 6, (uint32_t)zoom.size());
    put64(c.front.data() + 8, chrom_tree); put64(c.front.data() + 16, data); put64(c.front.data() + 24, index);
    put64(c.front.data() + 44, summary_off); put32(c.front.data() + 52, uncompress_buf);      // (fieldCount, definedFieldCount, autoSqlOffset, the reserved word: 0)
    if (summary) { c.front.resize(c.front.size() + kSummaryBytes); put_summary(c.front.data() + summary_off, *summary); }
    c.front.insert(c.front.end(), tree.begin(), tree.end());
    c.front.resize(c.front.size() + 8);
    put64(c.front.data() + c.front.size() - 8, (uint64_t)sections.size());
    write_rtree(c.back, sections, block_size, index, data + 8);
    uint64_t at = index + c.back.size();
    c.zoom.assign(zoom.size(), ZoomPiece());
    for (size_t k = 0; k < zoom.size(); ++k) {
        ZoomPiece &z = c.zoom[k];
        z.data_offset = at;
        z.front.assign(4, 0);
        put32(z.front.data(), (uint32_t)zoom[k].records);
        for (const WSection &s : zoom[k].blocks) z.block_bytes += s.size;
        z.index_offset = at + 4 + z.block_bytes;
        write_rtree(z.back, zoom[k].blocks, block_size, z.index_offset, at + 4);
        at = z.index_offset + z.back.size();
        uint8_t *h = c.front.data() + 64 + (size_t)kZoomHeaderBytes * k;
        put32(h, zoom[k].reduction); put32(h + 4, 0u); put64(h + 8, z.data_offset); put64(h + 16, z.index_offset);
    }
    std::vector<uint8_t> &last = c.zoom.empty() ? c.back : c.zoom.back().back;
    last.resize(last.size() + 4);
    put32(last.data() + last.size() - 4, pcbw::kBigWigMagic);
}

// ---------------------------------------------------------------- reading zoom levels
// The zoom headers of a file that pcbw::parse has accepted, and one level's records in file order, walked through the
// level's R-tree.  Both return what is wrong (empty: nothing), to stand behind "<path>: bigWig: ".
struct ZoomHeader { uint32_t reduction; uint64_t data, index; uint32_t records; };
inline std::string zoom_headers(const uint8_t *image, uint64_t size, std::vector<ZoomHeader> &out) {
    out.clear();
    if (size < 64) return pcbw::defect_text(pcbw::kBwTooShort);
    const uint64_t n = pcbw::rd16(image + 6);
    if (64u + (uint64_t)kZoomHeaderBytes * n > size) return "the zoom headers lie outside the file";
    for (uint64_t k = 0; k < n; ++k) {
        const uint8_t *h = image + 64 + kZoomHeaderBytes * k;
        ZoomHeader z{pcbw::rd32(h), pcbw::rd64(h + 8), pcbw::rd64(h + 16), 0u};
        const std::string lvl = "zoom level " + std::to_string(k) + ": ";
        if (z.reduction == 0u) return lvl + "a reduction of 0";
        if (z.data > size || size - z.data < 4) return lvl + "the record count lies outside the file";
        if (z.index > size || size - z.index < 48) return lvl + "the index lies outside the file";
        if (pcbw::rd32(image + z.index) != pcbw::kCirMagic) return lvl + "the index has a wrong magic";
        z.records = pcbw::rd32(image + z.data);
        out.push_back(z);
    }
    return std::string();
}
struct ZoomTable {
    std::vector<uint32_t> chrom, start, end, valid;
    std::vector<float> mn, mx, sum, sumsq;
    int64_t blocks = 0, bytes_inflated = 0, largest = 0;
};
// inflate: as pcbw::read_items takes it.  uncompress_buf: the file's (0: the blocks are stored).
template <typename Inflate> std::string read_zoom_level(const uint8_t *image, uint64_t size, uint32_t uncompress_buf, const std::vector<ZoomHeader> &levels, int64_t level,
                                                        Inflate inflate, ZoomTable &t) {
    t = ZoomTable();
    if (level < 0 || level >= (int64_t)levels.size()) return "zoom level " + std::to_string(level) + " of " + std::to_string(levels.size());
    const ZoomHeader &z = levels[(size_t)level];
    const std::string lvl = "zoom level " + std::to_string(level) + ": ";
    if (uncompress_buf > pcbw::kMaxInflated) return pcbw::defect_text(pcbw::kBwBufSize);
    pcbw::BigWig blocks;
    pcbw::detail::Walk w{image, size};
    if (pcbw::rd64(image + z.index + 8) != 0) pcbw::detail::walk_index(w, z.index + 48, 0, blocks);
    if (w.defect == pcbw::kBwIndexNodeOutside) return lvl + "a node of the index lies outside the file";
    if (w.defect) return lvl + pcbw::defect_text(w.defect);
    std::vector<uint8_t> buf((size_t)uncompress_buf + 1);
    for (size_t b = 0; b < blocks.blocks.size(); ++b) {
        const pcbw::Block &k = blocks.blocks[b];
        const std::string blk = lvl + "block " + std::to_string(b) + ": ";
        if (!w.inside(k.off, k.size)) return blk + pcbw::defect_text(pcbw::kBwBlockOutside);
        const uint8_t *p = image + k.off;
        uint64_t len = k.size;
        if (uncompress_buf) {
            if (k.size > pcbw::kMaxBlockBytes) return blk + pcbw::defect_text(pcbw::kBwBlockLarge);
            if (k.size < 6 || (p[0] & 15u) != 8u || (p[0] >> 4) > 7u || (((uint32_t)p[0] << 8) | p[1]) % 31u != 0u || (p[1] & 0x20u)) return blk + pcbw::defect_text(pcbw::kBwZlibHeader);
            size_t produced = 0;
            if (inflate(p + 2, (size_t)(k.size - 6), buf.data(), (size_t)uncompress_buf, produced) != 0) return blk + pcbw::defect_text(pcbw::kBwDeflate);
            const uint8_t *q = p + k.size - 4;
            uint32_t a = 1, s2 = 0;
            pcbw::adler_bytes(buf.data(), produced, a, s2);
            if (((s2 << 16) | a) != (((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3])) return blk + pcbw::defect_text(pcbw::kBwAdler);
            p = buf.data(); len = produced;
            t.bytes_inflated += (int64_t)produced;
        }
        if (len % kZoomRecordBytes != 0u) return blk + "not a whole number of 32-byte records";
        t.largest = std::max<int64_t>(t.largest, (int64_t)len);
        for (uint64_t i = 0; i < len; i += kZoomRecordBytes) {
            const uint8_t *r = p + i;
            t.chrom.push_back(pcbw::rd32(r)); t.start.push_back(pcbw::rd32(r + 4)); t.end.push_back(pcbw::rd32(r + 8)); t.valid.push_back(pcbw::rd32(r + 12));
            t.mn.push_back(pcbw::rdf32(r + 16)); t.mx.push_back(pcbw::rdf32(r + 20)); t.sum.push_back(pcbw::rdf32(r + 24)); t.sumsq.push_back(pcbw::rdf32(r + 28));
        }
    }
    t.blocks = (int64_t)blocks.blocks.size();
    if (t.chrom.size() != (size_t)z.records) return lvl + "the blocks hold " + std::to_string(t.chrom.size()) + " records, the level's count says " + std::to_string(z.records);
    return std::string();
}

// ---------------------------------------------------------------- the serial writer
// Contigs are added in any order (name, reported length, the cells of the strand); finish() sorts them, walks the cells,
// cuts the sections, encodes them with the model encoder (pcdeflate::encode), builds the zoom levels window by window
// and lays the file out.
struct HostWriter {
    struct In { std::string name; int64_t length; std::vector<double> cells; };
    struct LevelStats { int64_t reduction, records, blocks, raw_bytes, file_bytes; };
    uint32_t items_per_slot = 1024, block_size = 256;
    int compress = 1;                        // 0: stored sections, else the encoder's mode (pcdeflate::kFixed, kDynamic)
    int64_t zoom = kZoomNone;                // kZoomNone, kZoomAuto, or the first reduction
    std::vector<In> in;
    std::vector<uint8_t> image;
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // contigs, items, sections, raw bytes, block bytes, sections as stored, fixed, dynamic blocks
    std::vector<LevelStats> zoom_stats;
    std::string error;

    // the written levels: their blocks (encoded or stored) into zblocks[k], their tables into levels
    bool build_zoom(const std::vector<WContig> &contigs, const std::vector<int64_t> &item_first, const std::vector<uint32_t> &istart, const std::vector<uint32_t> &iend,
                    const std::vector<float> &ival, const Summary &sm, std::vector<ZoomLevel> &levels, std::vector<std::vector<uint8_t>> &zblocks, uint32_t &largest) {
        ZoomPlan z;
        const std::string bad = zoom_plan(contigs, zoom_first_reduction(zoom, (uint64_t)ival.size(), sm.valid), z);
        if (!bad.empty()) { error = bad; return false; }
        const int K = z.g.K;
        std::vector<ZoomAcc> acc((size_t)z.windows());
        for (int c = 0; c < K; ++c) {
            const int64_t nw = z.row(0)[c + 1] - z.row(0)[c];
            for (int64_t w = 0; w < nw; ++w) {
                const uint64_t ws = (uint64_t)w * z.g.r[0], we = std::min<uint64_t>(ws + z.g.r[0], contigs[(size_t)c].size);
                acc[(size_t)(z.row(0)[c] + w)] = zoom_window0(istart.data(), iend.data(), ival.data(), item_first[(size_t)c], item_first[(size_t)c + 1], (uint32_t)ws, (uint32_t)we);
            }
        }
        for (int k = 1; k < z.g.levels; ++k)
            for (int c = 0; c < K; ++c) {
                const int64_t nw = z.row(k)[c + 1] - z.row(k)[c], below = z.row(k - 1)[c + 1] - z.row(k - 1)[c];
                for (int64_t w = 0; w < nw; ++w) {
                    ZoomAcc p;
                    for (int64_t j = 4 * w; j < 4 * w + 4 && j < below; ++j) zoom_merge(p, acc[(size_t)(z.row(k - 1)[c] + j)]);
                    acc[(size_t)(z.row(k)[c] + w)] = p;
                }
            }
        std::vector<int64_t> rec(z.rows.size());
        int64_t n = 0;
        for (int k = 0; k < z.g.levels; ++k)
            for (int c = 0; c <= K; ++c) {
                rec[(size_t)k * (size_t)(K + 1) + (size_t)c] = n;
                if (c < K) for (int64_t p = z.row(k)[c]; p < z.row(k)[c + 1]; ++p) n += acc[(size_t)p].valid > 0u;
            }
        const int nlev = zoom_levels_written(z, rec);
        const uint32_t per_block = zoom_block_records(items_per_slot);
        std::vector<uint8_t> raw;
        for (int k = 0; k < nlev; ++k) {
            std::vector<ZoomBlock> blocks;
            zoom_cut_blocks(z, rec, k, per_block, blocks);
            ZoomLevel lv{z.g.r[k], (uint64_t)(rec[(size_t)k * (size_t)(K + 1) + (size_t)K] - rec[(size_t)k * (size_t)(K + 1)]), {}};
            std::vector<uint8_t> out;
            LevelStats st{(int64_t)z.g.r[k], (int64_t)lv.records, (int64_t)blocks.size(), 0, 0};
            size_t b = 0;
            for (int c = 0; c < K; ++c) {
                uint32_t count = 0;
                for (int64_t p = z.row(k)[c]; p < z.row(k)[c + 1]; ++p) {
                    if (acc[(size_t)p].valid == 0u) continue;
                    if (!count) raw.clear();
                    const uint64_t ws = (uint64_t)(p - z.row(k)[c]) * z.g.r[k], we = std::min<uint64_t>(ws + z.g.r[k], contigs[(size_t)c].size);
                    raw.resize(raw.size() + kZoomRecordBytes);
                    put_zoom_record(raw.data() + raw.size() - kZoomRecordBytes, (uint32_t)c, (uint32_t)ws, (uint32_t)we, acc[(size_t)p]);
                    if (++count < blocks[b].count) continue;
                    const size_t before = out.size();
                    if (compress) pcdeflate::encode(raw.data(), (uint32_t)raw.size(), out, (uint32_t)compress, nullptr);
                    else out.insert(out.end(), raw.begin(), raw.end());
                    lv.blocks.push_back({(uint32_t)c, pcbw::rd32(raw.data() + 4), pcbw::rd32(raw.data() + raw.size() - kZoomRecordBytes + 8), (uint64_t)(out.size() - before)});
                    st.raw_bytes += (int64_t)raw.size(); largest = std::max<uint32_t>(largest, (uint32_t)raw.size());
                    count = 0; ++b;
                }
            }
            st.file_bytes = (int64_t)out.size();
            levels.push_back(std::move(lv)); zblocks.push_back(std::move(out)); zoom_stats.push_back(st);
        }
        return true;
    }

    bool finish() {
        const std::string bad_zoom = check_zoom(zoom);
        if (!bad_zoom.empty()) { error = bad_zoom; return false; }
        std::sort(in.begin(), in.end(), [](const In &a, const In &b) { return a.name < b.name; });
        std::vector<WContig> contigs;
        std::vector<WSection> sections;
        std::vector<uint8_t> blocks, raw;
        std::vector<int64_t> item_first;       // (zoom) the items in front of every contig, and the items themselves
        std::vector<uint32_t> istart, iend;
        std::vector<float> ival;
        Summary sm;
        uint64_t nitems = 0, raw_bytes = 0, by_type[3] = {0, 0, 0};
        uint32_t largest = 0;
        zoom_stats.clear();
        for (size_t c = 0; c < in.size(); ++c) {
            const int64_t size = std::max<int64_t>(in[c].length, (int64_t)in[c].cells.size());
            if (size >= ((int64_t)1 << 32)) { error = "contig " + in[c].name + " has 2^32 positions or more"; return false; }
            if (c > 0 && in[c].name == in[c - 1].name) { error = "contig " + in[c].name + " given twice"; return false; }
            contigs.push_back({in[c].name, (uint32_t)size});
            item_first.push_back((int64_t)nitems);
            const std::vector<double> &v = in[c].cells;
            const int64_t n = (int64_t)v.size();
            uint32_t count = 0;
            auto flush = [&]() {
                if (!count) return;
                const uint32_t first = pcbw::rd32(raw.data() + 24), last = pcbw::rd32(raw.data() + 24 + (size_t)(count - 1) * kItemBytes + 4);
                put_section_header(raw.data(), (uint32_t)c, first, last, count);
                const size_t before = blocks.size();
                if (compress) {
                    uint32_t type = pcdeflate::kFixed;
                    pcdeflate::encode(raw.data(), (uint32_t)raw.size(), blocks, (uint32_t)compress, &type);
                    ++by_type[type];
                } else blocks.insert(blocks.end(), raw.begin(), raw.end());
                sections.push_back({(uint32_t)c, first, last, (uint64_t)(blocks.size() - before)});
                raw_bytes += raw.size(); largest = std::max<uint32_t>(largest, (uint32_t)raw.size());
                count = 0;
            };
            for (int64_t i = 0; i < n;) {
                if (!written(v[(size_t)i])) { ++i; continue; }
                int64_t j = i + 1;
                while (j < n && same_item(v[(size_t)j], v[(size_t)i])) ++j;
                if (!count) raw.assign(24, 0);
                raw.resize(raw.size() + kItemBytes);
                const float f = (float)v[(size_t)i];
                put_item(raw.data() + raw.size() - kItemBytes, (uint32_t)i, (uint32_t)j, f);
                summary_add(sm, (uint32_t)i, (uint32_t)j, f);
                if (zoom != kZoomNone) { istart.push_back((uint32_t)i); iend.push_back((uint32_t)j); ival.push_back(f); }
                ++nitems;
                if (++count == items_per_slot) flush();
                i = j;
            }
            flush();
        }
        item_first.push_back((int64_t)nitems);
        if (nitems >= ((uint64_t)1 << 31)) { error = "2^31 items or more"; return false; }
        std::vector<ZoomLevel> levels;
        std::vector<std::vector<uint8_t>> zblocks;
        if (zoom != kZoomNone && nitems > 0 && !build_zoom(contigs, item_first, istart, iend, ival, sm, levels, zblocks, largest)) return false;
        Container box;
        build_container(contigs, sections, block_size, compress ? largest : 0u, nitems ? &sm : nullptr, box, levels);
        image = box.front;
        image.insert(image.end(), blocks.begin(), blocks.end());
        image.insert(image.end(), box.back.begin(), box.back.end());
        for (size_t k = 0; k < levels.size(); ++k) {
            image.insert(image.end(), box.zoom[k].front.begin(), box.zoom[k].front.end());
            image.insert(image.end(), zblocks[k].begin(), zblocks[k].end());
            image.insert(image.end(), box.zoom[k].back.begin(), box.zoom[k].back.end());
        }
        stats[0] = (int64_t)contigs.size(); stats[1] = (int64_t)nitems; stats[2] = (int64_t)sections.size(); stats[3] = (int64_t)raw_bytes;
        stats[4] = (int64_t)blocks.size(); stats[5] = (int64_t)by_type[pcdeflate::kStored]; stats[6] = (int64_t)by_type[pcdeflate::kFixed]; stats[7] = (int64_t)by_type[pcdeflate::kDynamic];
        return true;
    }
};

}   // namespace pcbww
