// bigwig_host.h -- THE bigWig CONTAINER, host side: the one reader of the host path (bam_stager.cpp, pb_bigwig_read) and of
// the device import (bigwig_decoder.hip.h), whose kernels run the section and item decoders below.  The contract is Kent's
// reader as the reference links it (kent/src/lib/bbiRead.c, bPlusTree.c, cirTree.c, bwgQuery.c:155-285) restated:
//   - a 64-byte header: magic 0x888FFC26, version u16, zoomLevels u16, chromTreeOffset, unzoomedDataOffset,
//     unzoomedIndexOffset u64, fieldCount, definedFieldCount u16, asOffset, totalSummaryOffset u64, uncompressBufSize u32,
//     extensionOffset u64.  Zoom levels, the total summary and the extension are not read;
//   - the chromosome B+ tree (magic 0x78CA8C91, blockSize, keySize, valSize u32, itemCount u64, 8 reserved bytes; a node
//     is isLeaf u8, reserved u8, count u16, then count x {key[keySize], chromId u32, chromSize u32} in a leaf and
//     {key[keySize], childOffset u64} above): the contigs in the order of a depth-first walk, bbiChromList's order;
//   - the unzoomed R-tree (magic 0x2468ACE0, 48-byte header; a node is isLeaf u8, reserved u8, count u16, then count x
//     {startChromIx, startBase, endChromIx, endBase u32, offset u64, size u64} in a leaf and the same without size above):
//     one leaf item per data block, the blocks in the order of the walk -- the order both Kent readers apply them in;
//   - uncompressBufSize > 0: every block is a zlib stream (RFC 1950: CMF, FLG, raw DEFLATE, Adler-32 big-endian) that
//     inflates to AT MOST uncompressBufSize bytes -- the inflated size is stored nowhere; == 0: the blocks are stored;
//   - a block is a section: chromId, start, end, itemStep, itemSpan u32, type u8, reserved u8, itemCount u16, then the
//     items -- type 1 bedGraph {start, end u32, value f32}, 2 variableStep {start u32, value f32} (end = start + itemSpan),
//     3 fixedStep {value f32} (start = section start + i * itemStep, end = start + itemSpan) -- which end exactly where the
//     block does (bwgQuery.c asserts it).  Values widen to float64.
// What is refused (defect_message; "<path>: bigWig: <what>", the lowest (block, item) first, file structure before blocks):
// a wrong magic (bigBed's named), a byte-swapped file, a version below 3, tree nodes or blocks outside the file, a zlib
// header that is not CM = 8 without FDICT, a block too large for the inflate kernel, a section of unknown type, a section
// whose 24 + itemCount x itemsize is not the block's inflated length, an item with end <= start, a chromId outside the
// tree, an end beyond the contig's size, a failed Adler-32, a DEFLATE error.
// THE LIMITS come from k_bgzf_inflate (bam_kernels.hip.h), which counts the bits of its input and the bytes of its output
// in 32 bits: bit position = 8 x (byte position) must stay below 2^32 with the 84 bytes a batch stages ahead and the 8 it
// may read behind the end, so a compressed block holds at most kMaxBlockBytes = 2^28 bytes (half of what the arithmetic
// admits); the output position plus a window (2 KiB) and a maximal match (258) must not wrap, so uncompressBufSize is at
// most kMaxInflated = 2^30.  A stored block is bounded by kMaxInflated alone.
// The section and item functions carry PC_BW_HD: __host__ __device__ under hipcc, nothing under a host compiler.
// Plain C++17 (no HIP, no zlib: the caller passes the inflate function): tests/bigwig_host_test.cpp compiles it on a
// machine without a GPU, under the sanitizers.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define PC_BW_HD __host__ __device__
#else
#define PC_BW_HD
#endif

namespace pcbw {

constexpr uint32_t kBigWigMagic = 0x888FFC26u, kBigBedMagic = 0x8789F2EBu, kBptMagic = 0x78CA8C91u, kCirMagic = 0x2468ACE0u;
constexpr uint64_t kMaxBlockBytes = (uint64_t)1 << 28;
constexpr uint32_t kMaxInflated = (uint32_t)1 << 30;
constexpr uint32_t kMaxChromId = (uint32_t)1 << 22;     // (the track's sort key holds 22 bits of contig)
constexpr int kSectionHeader = 24;
constexpr int kMaxTreeDepth = 32;

enum {
    kBwOk = 0,
    // the file's structure (found before any block is read)
    kBwTooShort = 1, kBwBigBed, kBwSwapped, kBwMagic, kBwVersion, kBwChromTreeOutside, kBwChromTreeMagic, kBwChromTreeVal, kBwChromNodeOutside,
    kBwChromId, kBwTreeNodes, kBwTreeDepth, kBwIndexOutside, kBwIndexMagic, kBwIndexNodeOutside, kBwBufSize,
    kBwBlockOutside, kBwBlockLarge, kBwZlibHeader,
    // a block's content
    kBwDeflate, kBwAdler, kBwSectionShort, kBwSectionType, kBwSectionLength, kBwSectionChrom, kBwItemEmpty, kBwItemBeyond,
    kBwCodeEnd
};

inline const char *defect_text(int code) {
    switch (code) {
    case kBwTooShort: return "shorter than the 64-byte header";
    case kBwBigBed: return "this is a bigBed file (magic 0x8789F2EB), not a bigWig";
    case kBwSwapped: return "byte-swapped (big-endian) files are not read";
    case kBwMagic: return "not a bigWig file (magic is not 0x888FFC26)";
    case kBwVersion: return "version below 3";
    case kBwChromTreeOutside: return "the chromosome tree lies outside the file";
    case kBwChromTreeMagic: return "the chromosome tree has a wrong magic";
    case kBwChromTreeVal: return "the chromosome tree's values are not (id, size) pairs of 8 bytes, or its keys are empty";
    case kBwChromNodeOutside: return "a node of the chromosome tree lies outside the file";
    case kBwChromId: return "a chromosome id of 2^22 or more, or one given twice";
    case kBwTreeNodes: return "a tree of more nodes than the file can hold";
    case kBwTreeDepth: return "a tree deeper than 32 levels";
    case kBwIndexOutside: return "the unzoomed index lies outside the file";
    case kBwIndexMagic: return "the unzoomed index has a wrong magic";
    case kBwIndexNodeOutside: return "a node of the unzoomed index lies outside the file";
    case kBwBufSize: return "uncompressBufSize beyond 2^30";
    case kBwBlockOutside: return "the block lies outside the file";
    case kBwBlockLarge: return "the block is larger than 2^28 bytes (2^30 when stored)";
    case kBwZlibHeader: return "not a zlib stream of CM = 8 without FDICT";
    case kBwDeflate: return "DEFLATE error";
    case kBwAdler: return "Adler-32 mismatch";
    case kBwSectionShort: return "shorter than a section header";
    case kBwSectionType: return "section of unknown type";
    case kBwSectionLength: return "the items do not end where the block does";
    case kBwSectionChrom: return "chromId outside the chromosome tree";
    case kBwItemEmpty: return "end <= start";
    case kBwItemBeyond: return "end beyond the contig's size";
    }
    return "unknown defect";
}

// A defect as one word that orders them: block (31 bits; structure defects stand in front of every block) << 32 |
// item + 1 (0: the block as a whole) << 8 | code.  kNoDefect: none.
constexpr unsigned long long kNoDefect = ~0ull;
PC_BW_HD inline unsigned long long block_defect(int64_t block, int code) { return ((unsigned long long)(block + 1) << 32) | (unsigned long long)code; }
PC_BW_HD inline unsigned long long item_defect(int64_t block, uint32_t item, int code) {
    return ((unsigned long long)(block + 1) << 32) | ((unsigned long long)(item + 1u) << 8) | (unsigned long long)code;
}
inline unsigned long long file_defect(int code) { return (unsigned long long)code; }

inline std::string defect_message(const char *path, unsigned long long d) {
    const int code = (int)(d & 0xffu);
    const long long block = (long long)(d >> 32) - 1;
    const unsigned item = (unsigned)((d >> 8) & 0xffffffu);
    char where[64];
    where[0] = 0;
    if (block >= 0 && item) snprintf(where, sizeof(where), "block %lld item %u: ", block, item - 1u);
    else if (block >= 0) snprintf(where, sizeof(where), "block %lld: ", block);
    return std::string(path ? path : "<memory>") + ": bigWig: " + where + defect_text(code);
}

// ---------------------------------------------------------------- little-endian fields
PC_BW_HD inline uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
PC_BW_HD inline uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
PC_BW_HD inline uint64_t rd64(const uint8_t *p) { return (uint64_t)rd32(p) | ((uint64_t)rd32(p + 4) << 32); }
PC_BW_HD inline float rdf32(const uint8_t *p) {
    const uint32_t u = rd32(p);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// ---------------------------------------------------------------- sections and items (host and device)
struct Section {
    uint32_t chrom_id, start, end, step, span;
    uint32_t type, count;
};
struct Item {
    int64_t start, stop;
    double value;
};
// what the items know of a chromosome id: the contig's place in the chromosome list (-1: no such id) and its size
struct ChromOfId { int32_t contig; uint32_t size; };

PC_BW_HD inline Section section_header(const uint8_t *p) {
    Section s;
    s.chrom_id = rd32(p); s.start = rd32(p + 4); s.end = rd32(p + 8); s.step = rd32(p + 12); s.span = rd32(p + 16);
    s.type = p[20]; s.count = rd16(p + 22);
    return s;
}
PC_BW_HD inline uint32_t item_bytes(uint32_t type) { return type == 1u ? 12u : (type == 2u ? 8u : (type == 3u ? 4u : 0u)); }
// A block of `len` bytes (its inflated length) as a section: its header into s, the defect of the block as a whole.
// Nothing behind the first 24 bytes is read.
PC_BW_HD inline int check_section(const uint8_t *p, uint64_t len, const ChromOfId *ids, uint32_t nids, Section &s) {
    s.chrom_id = 0; s.start = 0; s.end = 0; s.step = 0; s.span = 0; s.type = 0; s.count = 0;
    if (len < (uint64_t)kSectionHeader) return kBwSectionShort;
    s = section_header(p);
    if (item_bytes(s.type) == 0u) { s.count = 0; return kBwSectionType; }
    if ((uint64_t)kSectionHeader + (uint64_t)s.count * item_bytes(s.type) != len) { s.count = 0; return kBwSectionLength; }
    if (s.chrom_id >= nids || ids[s.chrom_id].contig < 0) { s.count = 0; return kBwSectionChrom; }
    return kBwOk;
}
// item i of a checked section whose items start at `items` (the block + 24)
PC_BW_HD inline Item section_item(const Section &s, const uint8_t *items, uint32_t i) {
    Item it;
    if (s.type == 1u) {
        const uint8_t *q = items + (size_t)i * 12u;
        it.start = (int64_t)rd32(q); it.stop = (int64_t)rd32(q + 4); it.value = (double)rdf32(q + 8);
    } else if (s.type == 2u) {
        const uint8_t *q = items + (size_t)i * 8u;
        it.start = (int64_t)rd32(q); it.stop = it.start + (int64_t)s.span; it.value = (double)rdf32(q + 4);
    } else {
        it.start = (int64_t)s.start + (int64_t)i * (int64_t)s.step; it.stop = it.start + (int64_t)s.span; it.value = (double)rdf32(items + (size_t)i * 4u);
    }
    return it;
}
PC_BW_HD inline int check_item(const Item &it, uint32_t chrom_size) {
    if (it.stop <= it.start) return kBwItemEmpty;
    if (it.stop > (int64_t)chrom_size) return kBwItemBeyond;
    return kBwOk;
}

// Adler-32 (RFC 1950) of a piece, and of a concatenation from its pieces' sums: a = 1 + sum of bytes, b = sum of the
// running a's, both mod 65521.  a(AB) = a(A) + a(B) - 1, b(AB) = b(A) + b(B) + len(B) x (a(A) - 1).
constexpr uint32_t kAdlerMod = 65521u;
constexpr uint32_t kAdlerNmax = 5552u;       // zlib's NMAX: the most bytes 32-bit sums take between reductions
PC_BW_HD inline void adler_bytes(const uint8_t *p, uint64_t n, uint32_t &a, uint32_t &b) {
    while (n) {
        const uint32_t k = n < (uint64_t)kAdlerNmax ? (uint32_t)n : kAdlerNmax;
        for (uint32_t i = 0; i < k; ++i) { a += p[i]; b += a; }
        a %= kAdlerMod; b %= kAdlerMod;
        p += k; n -= k;
    }
}
// (a1, b1) of A, (a2, b2) of B with |B| = len2, each sum from (1, 0): the sums of AB
PC_BW_HD inline void adler_combine(uint32_t &a1, uint32_t &b1, uint32_t a2, uint32_t b2, uint64_t len2) {
    const uint64_t rem = len2 % kAdlerMod;
    const uint64_t b = (uint64_t)b1 + (uint64_t)b2 + rem * (uint64_t)((a1 + kAdlerMod - 1u) % kAdlerMod);
    a1 = (a1 + a2 + kAdlerMod - 1u) % kAdlerMod;
    b1 = (uint32_t)(b % kAdlerMod);
}

// ---------------------------------------------------------------- the file
struct Chrom { std::string name; uint32_t id, size; };
// One data block.  off / size: its bytes in the file.  Compressed: the raw DEFLATE stream is [off + 2, off + size - 4) and
// `adler` its trailer.
struct Block { uint64_t off, size; uint32_t adler; };
struct BigWig {
    uint32_t version = 0, zoom_levels = 0, uncompress_buf = 0;
    uint64_t chrom_tree = 0, data = 0, index = 0;
    std::vector<Chrom> chroms;             // bbiChromList order
    std::vector<ChromOfId> of_id;          // by chromId
    std::vector<Block> blocks;             // index order
    uint64_t data_lo = 0, data_hi = 0;     // the bytes that hold the blocks: [data_lo, data_hi)
    bool compressed() const { return uncompress_buf != 0; }
    // bytes of the slot a block inflates into (a multiple of 16)
    uint64_t slot_bytes() const { return ((uint64_t)uncompress_buf + 15u) & ~(uint64_t)15u; }
};

namespace detail {
struct Walk {
    const uint8_t *image; uint64_t size; uint64_t nodes = 0; int defect = kBwOk;
    bool inside(uint64_t off, uint64_t n) const { return off <= size && n <= size - off; }
    bool count_node() { return ++nodes <= size / 4 + 1; }
};
inline void walk_chroms(Walk &w, uint64_t off, uint32_t key_size, int depth, BigWig &f) {
    if (w.defect) return;
    if (depth > kMaxTreeDepth) { w.defect = kBwTreeDepth; return; }
    if (!w.count_node()) { w.defect = kBwTreeNodes; return; }
    if (!w.inside(off, 4)) { w.defect = kBwChromNodeOutside; return; }
    const bool leaf = w.image[off] != 0;
    const uint64_t count = rd16(w.image + off + 2), item = (uint64_t)key_size + 8u;
    if (!w.inside(off + 4, count * item)) { w.defect = kBwChromNodeOutside; return; }
    for (uint64_t k = 0; k < count && !w.defect; ++k) {
        const uint8_t *p = w.image + off + 4 + k * item;
        if (!leaf) { walk_chroms(w, rd64(p + key_size), key_size, depth + 1, f); continue; }
        Chrom c;
        c.name.assign((const char *)p, strnlen((const char *)p, key_size));
        c.id = rd32(p + key_size); c.size = rd32(p + key_size + 4);
        if (c.id >= kMaxChromId) { w.defect = kBwChromId; return; }
        if (f.of_id.size() <= c.id) f.of_id.resize((size_t)c.id + 1, ChromOfId{-1, 0u});
        if (f.of_id[c.id].contig >= 0) { w.defect = kBwChromId; return; }
        f.of_id[c.id] = ChromOfId{(int32_t)f.chroms.size(), c.size};
        f.chroms.push_back(c);
    }
}
inline void walk_index(Walk &w, uint64_t off, int depth, BigWig &f) {
    if (w.defect) return;
    if (depth > kMaxTreeDepth) { w.defect = kBwTreeDepth; return; }
    if (!w.count_node()) { w.defect = kBwTreeNodes; return; }
    if (!w.inside(off, 4)) { w.defect = kBwIndexNodeOutside; return; }
    const bool leaf = w.image[off] != 0;
    const uint64_t count = rd16(w.image + off + 2), item = leaf ? 32u : 24u;
    if (!w.inside(off + 4, count * item)) { w.defect = kBwIndexNodeOutside; return; }
    for (uint64_t k = 0; k < count && !w.defect; ++k) {
        const uint8_t *p = w.image + off + 4 + k * item;
        if (leaf) f.blocks.push_back(Block{rd64(p + 16), rd64(p + 24), 0u});
        else walk_index(w, rd64(p + 16), depth + 1, f);
    }
}
}   // namespace detail

// The header, the chromosome list and the block table of a file image.  Returns kNoDefect, or the first defect.
inline unsigned long long parse(const uint8_t *image, uint64_t size, BigWig &f) {
    f = BigWig();
    if (size < 64) return file_defect(size >= 4 && rd32(image) == kBigBedMagic ? kBwBigBed : kBwTooShort);
    const uint32_t magic = rd32(image);
    if (magic == kBigBedMagic) return file_defect(kBwBigBed);
    if (magic == __builtin_bswap32(kBigWigMagic) || magic == __builtin_bswap32(kBigBedMagic)) return file_defect(kBwSwapped);
    if (magic != kBigWigMagic) return file_defect(kBwMagic);
    f.version = rd16(image + 4); f.zoom_levels = rd16(image + 6);
    f.chrom_tree = rd64(image + 8); f.data = rd64(image + 16); f.index = rd64(image + 24);
    f.uncompress_buf = rd32(image + 52);
    if (f.version < 3) return file_defect(kBwVersion);
    detail::Walk w{image, size};
    if (!w.inside(f.chrom_tree, 32)) return file_defect(kBwChromTreeOutside);
    const uint8_t *ct = image + f.chrom_tree;
    if (rd32(ct) != kBptMagic) return file_defect(kBwChromTreeMagic);
    const uint32_t key_size = rd32(ct + 8), val_size = rd32(ct + 12);
    if (val_size != 8 || key_size == 0 || key_size > 65536u) return file_defect(kBwChromTreeVal);
    if (rd64(ct + 16) != 0) detail::walk_chroms(w, f.chrom_tree + 32, key_size, 0, f);   // (an empty tree has no root node)
    if (w.defect) return file_defect(w.defect);
    if (!w.inside(f.index, 48)) return file_defect(kBwIndexOutside);
    if (rd32(image + f.index) != kCirMagic) return file_defect(kBwIndexMagic);
    w.nodes = 0;
    if (rd64(image + f.index + 8) != 0) detail::walk_index(w, f.index + 48, 0, f);
    if (w.defect) return file_defect(w.defect);
    if (f.uncompress_buf > kMaxInflated) return file_defect(kBwBufSize);
    if (f.blocks.size() >= ((size_t)1 << 31) - 1) return file_defect(kBwTreeNodes);
    f.data_lo = f.blocks.empty() ? 0 : ~(uint64_t)0;
    for (size_t b = 0; b < f.blocks.size(); ++b) {
        Block &k = f.blocks[b];
        if (!w.inside(k.off, k.size)) return block_defect((int64_t)b, kBwBlockOutside);
        if (k.size > (f.compressed() ? kMaxBlockBytes : (uint64_t)kMaxInflated)) return block_defect((int64_t)b, kBwBlockLarge);
        if (f.compressed()) {
            const uint8_t *p = image + k.off;
            // RFC 1950: CM = 8, CINFO <= 7, FCHECK, no preset dictionary; the Adler-32 is big-endian
            if (k.size < 6 || (p[0] & 15u) != 8u || (p[0] >> 4) > 7u || (((uint32_t)p[0] << 8) | p[1]) % 31u != 0u || (p[1] & 0x20u)) return block_defect((int64_t)b, kBwZlibHeader);
            const uint8_t *t = p + k.size - 4;
            k.adler = ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | (uint32_t)t[3];
        }
        if (k.off < f.data_lo) f.data_lo = k.off;
        if (k.off + k.size > f.data_hi) f.data_hi = k.off + k.size;
    }
    return kNoDefect;
}

// ---------------------------------------------------------------- the serial reader
// The items of a file in file order, as columns; `block`: the block an item came from.
struct ItemTable {
    BigWig file;
    std::vector<int32_t> chrom;            // place in file.chroms
    std::vector<int64_t> start, stop;
    std::vector<double> value;
    std::vector<int32_t> block;
    int64_t by_type[3] = {0, 0, 0};        // items of bedGraph, variableStep and fixedStep sections
    int64_t bytes_inflated = 0;
    unsigned long long defect = kNoDefect;
};

// inflate(src, n, dst, cap, produced): a raw DEFLATE stream of exactly n bytes into at most cap; 0: fine, otherwise a
// DEFLATE error (a stream that ends before its n-th byte or runs beyond it included).
template <typename Inflate> void read_items(const uint8_t *image, uint64_t size, Inflate inflate, ItemTable &t) {
    t = ItemTable();
    t.defect = parse(image, size, t.file);
    if (t.defect != kNoDefect) return;
    const BigWig &f = t.file;
    std::vector<uint8_t> buf((size_t)f.uncompress_buf + 1);
    for (size_t b = 0; b < f.blocks.size(); ++b) {
        const Block &k = f.blocks[b];
        const uint8_t *p = image + k.off;
        uint64_t len = k.size;
        if (f.compressed()) {
            size_t produced = 0;
            if (inflate(p + 2, (size_t)(k.size - 6), buf.data(), (size_t)f.uncompress_buf, produced) != 0) { t.defect = block_defect((int64_t)b, kBwDeflate); return; }
            uint32_t a = 1, s2 = 0;
            adler_bytes(buf.data(), produced, a, s2);
            if (((s2 << 16) | a) != k.adler) { t.defect = block_defect((int64_t)b, kBwAdler); return; }
            p = buf.data(); len = produced;
            t.bytes_inflated += (int64_t)produced;
        }
        Section s;
        const int err = check_section(p, len, f.of_id.data(), (uint32_t)f.of_id.size(), s);
        if (err) { t.defect = block_defect((int64_t)b, err); return; }
        const ChromOfId c = f.of_id[s.chrom_id];
        for (uint32_t i = 0; i < s.count; ++i) {
            const Item it = section_item(s, p + kSectionHeader, i);
            const int ie = check_item(it, c.size);
            if (ie) { t.defect = item_defect((int64_t)b, i, ie); return; }
            t.chrom.push_back(c.contig); t.start.push_back(it.start); t.stop.push_back(it.stop); t.value.push_back(it.value);
            t.block.push_back((int32_t)b);
        }
        t.by_type[s.type - 1] += s.count;
    }
}

}   // namespace pcbw
