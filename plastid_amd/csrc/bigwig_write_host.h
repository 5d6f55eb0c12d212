// bigwig_write_host.h -- WRITING bigWig files (revision 19), host side: what the host writer (bam_stager.cpp,
// pb_bigwig_write_*) and the device export (bigwig_writer.hip.h, pc_track_export_bigwig) share.  HIP-free.
//   - which cells are written and how they group into items (written, same_item; the kernels compile them);
//   - the 24-byte section header (put_section_header; the kernels compile it);
//   - the total summary and the order its minimum and maximum are taken in (float_key);
//   - THE CONTAINER around the blocks (build_container): little-endian, version 4, zoomLevels = 0, laid out as
//     tests/bigwig_writer.py lays its files out, which Kent's readers read:
//       64-byte header | total summary (40 bytes, when the file has items) | chromosome B+ tree | u64 section count |
//       the blocks back to back | R-tree (48-byte header, bulk-loaded over the sections in file order) | the magic;
//   - the serial writer over one contig's cells at a time (HostWriter), which is the model of the device export.
// Cells: a cell is written iff its value != 0.0 (NaN is, -0.0 is not).  Neighbouring written cells of one contig form one
// item while their float64 values compare equal (a NaN is an item of its own); the value is cast to float32
// round-to-nearest-even AFTERWARDS, so two doubles that cast alike stay two items.  Every items_per_slot consecutive items
// of a contig make one bedGraph section (type 1); sections never span contigs.  Contigs stand in the sorted order of
// their names (bytes), the chromosome id is the place in it, and every contig is in the tree, with or without items.
// Not written: zoom levels, variableStep / fixedStep sections, bigBed, byte-swapped files; nothing is appended to a file.
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

// What stands in front of the blocks (header, summary, chromosome tree, section count) and behind them (R-tree, magic).
// summary: null for a file without items (totalSummaryOffset = 0).  uncompress_buf: the largest raw section, 0: stored blocks.
struct Container { std::vector<uint8_t> front, back; uint64_t block_bytes = 0; };
inline void build_container(const std::vector<WContig> &contigs, const std::vector<WSection> &sections, uint32_t block_size, uint32_t uncompress_buf,
                            const Summary *summary, Container &c) {
    const uint64_t summary_off = summary ? 64u : 0u, chrom_tree = 64u + (summary ? kSummaryBytes : 0u);
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
    std::vector<uint64_t> off(sections.size());
    uint64_t at = data + 8;
    for (size_t s = 0; s < sections.size(); ++s) { off[s] = at; at += sections[s].size; }
    const uint64_t index = at;
    c.block_bytes = index - (data + 8);
    c.front.assign(64, 0);
    uint8_t *h = c.front.data();
    put32(h, pcbw::kBigWigMagic); put16(h + 4, 4u); put16(h + 6, 0u); put64(h + 8, chrom_tree); put64(h + 16, data); put64(h + 24, index);
    put64(h + 44, summary_off); put32(h + 52, uncompress_buf);      // (fieldCount, definedFieldCount, autoSqlOffset, the reserved word: 0)
    if (summary) { c.front.resize(64 + kSummaryBytes); put_summary(c.front.data() + 64, *summary); }
    c.front.insert(c.front.end(), tree.begin(), tree.end());
    c.front.resize(c.front.size() + 8);
    put64(c.front.data() + c.front.size() - 8, (uint64_t)sections.size());
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
    c.back.assign(48, 0);
    put32(c.back.data(), pcbw::kCirMagic); put32(c.back.data() + 4, block_size); put64(c.back.data() + 8, (uint64_t)sections.size());
    bounds(0, (uint64_t)sections.size(), c.back.data() + 16);
    put64(c.back.data() + 32, index); put32(c.back.data() + 40, 1u);
    write_tree(c.back, (uint64_t)sections.size(), block_size, 32, 24, index + 48,
               [&](uint64_t i, uint8_t *p) { bounds(i, i + 1, p); put64(p + 16, off[(size_t)i]); put64(p + 24, sections[(size_t)i].size); },
               [&](uint64_t lo, uint64_t hi, uint64_t child, uint8_t *p) { bounds(lo, hi, p); put64(p + 16, child); });
    c.back.resize(c.back.size() + 4);
    put32(c.back.data() + c.back.size() - 4, pcbw::kBigWigMagic);
}

// ---------------------------------------------------------------- the serial writer
// Contigs are added in any order (name, reported length, the cells of the strand); finish() sorts them, walks the cells,
// cuts the sections, encodes them with the model encoder (pcdeflate::encode) and lays the file out.
struct HostWriter {
    struct In { std::string name; int64_t length; std::vector<double> cells; };
    uint32_t items_per_slot = 1024, block_size = 256;
    int compress = 1;                        // 0: stored sections, else the encoder's mode (pcdeflate::kFixed, kDynamic)
    std::vector<In> in;
    std::vector<uint8_t> image;
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // contigs, items, sections, raw bytes, block bytes, sections as stored, fixed, dynamic blocks
    std::string error;

    bool finish() {
        std::sort(in.begin(), in.end(), [](const In &a, const In &b) { return a.name < b.name; });
        std::vector<WContig> contigs;
        std::vector<WSection> sections;
        std::vector<uint8_t> blocks, raw;
        Summary sm;
        uint64_t nitems = 0, raw_bytes = 0, by_type[3] = {0, 0, 0};
        uint32_t largest = 0;
        for (size_t c = 0; c < in.size(); ++c) {
            const int64_t size = std::max<int64_t>(in[c].length, (int64_t)in[c].cells.size());
            if (size >= ((int64_t)1 << 32)) { error = "contig " + in[c].name + " has 2^32 positions or more"; return false; }
            if (c > 0 && in[c].name == in[c - 1].name) { error = "contig " + in[c].name + " given twice"; return false; }
            contigs.push_back({in[c].name, (uint32_t)size});
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
                ++nitems;
                if (++count == items_per_slot) flush();
                i = j;
            }
            flush();
        }
        if (nitems >= ((uint64_t)1 << 31)) { error = "2^31 items or more"; return false; }
        Container box;
        build_container(contigs, sections, block_size, compress ? largest : 0u, nitems ? &sm : nullptr, box);
        image = box.front;
        image.insert(image.end(), blocks.begin(), blocks.end());
        image.insert(image.end(), box.back.begin(), box.back.end());
        stats[0] = (int64_t)contigs.size(); stats[1] = (int64_t)nitems; stats[2] = (int64_t)sections.size(); stats[3] = (int64_t)raw_bytes;
        stats[4] = (int64_t)blocks.size(); stats[5] = (int64_t)by_type[pcdeflate::kStored]; stats[6] = (int64_t)by_type[pcdeflate::kFixed]; stats[7] = (int64_t)by_type[pcdeflate::kDynamic];
        return true;
    }
};

}   // namespace pcbww
