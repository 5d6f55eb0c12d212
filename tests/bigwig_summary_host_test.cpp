// The summary model of plastid_amd/csrc/bigwig_summary_host.h as a program, for the sanitizers
// (tests/test_bigwig_summary_host.py compiles it with -fsanitize=address,undefined), over hand-built images:
//   - a record that spans the whole query: a level whose header is patched to a reduction of 2, one record [0, 8), the
//     query [1, 7): the overlap factor 6 / 8 scales validCount and both sums, exactly;
//   - an empty level (record count and R-tree item count patched to 0): no data, nothing read;
//   - a truncated level block, stored (not a whole number of records) and compressed (the stream ends early): refused
//     with a message, by the model's reader and by level_blocks;
//   - the items' path beside it: clipped items, a bin wider than its data, more bins than positions, a query beyond the
//     contig; records out of order: index_table says so and summarize refuses; the argument checks.
#include <zlib.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bigwig_summary_host.h"

static int zlib_raw_inflate(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t &produced) {
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) return 1;
    zs.next_in = const_cast<Bytef *>(src); zs.avail_in = (uInt)n;
    zs.next_out = dst; zs.avail_out = (uInt)cap;
    const int rc = inflate(&zs, Z_FINISH);
    produced = (size_t)zs.total_out;
    const bool whole = rc == Z_STREAM_END && zs.avail_in == 0;
    inflateEnd(&zs);
    return whole ? 0 : 1;
}

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

namespace ws = pcbws;

static void put32(uint8_t *p, uint32_t v) { for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(v >> (8 * k)); }
static void put64(uint8_t *p, uint64_t v) { for (int k = 0; k < 8; ++k) p[k] = (uint8_t)(v >> (8 * k)); }

// one contig "x" of `size` positions: 2.0 on [0, 8), 3.0 on [10, 13); zoom levels from a first reduction of 8
static std::vector<uint8_t> write_file(uint32_t size, int compress) {
    pcbww::HostWriter w;
    w.items_per_slot = 4; w.block_size = 4; w.compress = compress; w.zoom = 8;
    std::vector<double> cells(size, 0.0);
    for (uint32_t i = 0; i < 8 && i < size; ++i) cells[i] = 2.0;
    for (uint32_t i = 10; i < 13 && i < size; ++i) cells[i] = 3.0;
    w.in.push_back({"x", (int64_t)size, cells});
    if (!w.finish()) { printf("the writer failed: %s\n", w.error.c_str()); exit(1); }
    return w.image;
}

static std::string query(const std::vector<uint8_t> &image, int32_t contig, uint32_t start, uint32_t end, uint32_t n_bins, std::vector<ws::Element> &out, int *level = nullptr) {
    ws::HostSummary s;
    std::string bad = s.open(image.data(), image.size());
    if (!bad.empty()) return "open: " + bad;
    if (level) *level = ws::choose_level(s.reduction.data(), (int)s.reduction.size(), start, end, n_bins);
    out.assign(n_bins, ws::Element());
    return s.summarize(1, &contig, &start, &end, n_bins, zlib_raw_inflate, out.data());
}

int main() {
    std::vector<ws::Element> el;
    int level = 0;
    // ---- a record that spans the whole query
    {
        std::vector<uint8_t> image = write_file(8, 0);
        std::vector<pcbww::ZoomHeader> levels;
        CHECK(pcbww::zoom_headers(image.data(), image.size(), levels).empty() && levels.size() >= 1 && levels[0].records == 1, "one record at level 0");
        put32(image.data() + 64, 2u);       // the level's reduction: 8 -> 2
        std::string bad = query(image, 0, 1, 7, 1, el, &level);
        CHECK(bad.empty(), "%s", bad.c_str());
        CHECK(level == 0, "want 3 selects the level of reduction 2, got %d", level);
        CHECK(el[0].valid == 6u && el[0].mn == 2.0 && el[0].mx == 2.0 && el[0].sum == 12.0 && el[0].sumsq == 24.0, "6 / 8 of (8, 16, 32): %u %g %g", el[0].valid, el[0].sum, el[0].sumsq);
        CHECK(ws::value_of(el[0], ws::kMean, 1, 7, 1) == 2.0 && ws::value_of(el[0], ws::kCoverage, 1, 7, 1) == 1.0 && ws::value_of(el[0], ws::kStd, 1, 7, 1) == 0.0, "the values");
        // two bins, the second beyond the record: no data there
        bad = query(image, 0, 2, 14, 2, el, &level);
        CHECK(bad.empty() && level == 0, "two bins of 6: %s", bad.c_str());
        CHECK(el[0].valid == 6u && el[0].sum == 12.0 && el[1].valid == 0u && el[1].sum == 0.0, "the bin behind the record is empty");
        // the items of the same file: clipped, more bins than positions, beyond the contig, a contig the file lacks
        bad = query(image, 0, 6, 9, 1, el, &level);
        CHECK(bad.empty() && level == ws::kItems && el[0].valid == 2u && el[0].sum == 4.0 && el[0].sumsq == 8.0, "the item clipped to [6, 8)");
        bad = query(image, 0, 6, 9, 7, el, &level);
        CHECK(bad.empty() && level == ws::kItems, "seven bins over three positions");
        // (edges 6 6 7 7 8 8 9 behind the start 6: an empty bin is one position wide; the data ends at 8)
        CHECK(el[0].valid == 1u && el[1].valid == 1u && el[2].valid == 1u && el[3].valid == 1u && el[4].valid == 1u && el[5].valid == 0u && el[6].valid == 0u, "empty bins take one position");
        bad = query(image, 0, 100, 140, 4, el);
        CHECK(bad.empty() && el[0].valid == 0u && el[3].valid == 0u, "beyond the contig");
        bad = query(image, -1, 0, 8, 2, el);
        CHECK(bad.empty() && el[0].valid == 0u, "a contig the file lacks");
    }
    // ---- an empty level
    {
        std::vector<uint8_t> image = write_file(64, 0);
        std::vector<pcbww::ZoomHeader> levels;
        CHECK(pcbww::zoom_headers(image.data(), image.size(), levels).empty() && !levels.empty(), "levels");
        put32(image.data() + levels[0].data, 0u);
        put64(image.data() + levels[0].index + 8, 0u);
        std::string bad = query(image, 0, 0, 64, 2, el, &level);
        CHECK(bad.empty(), "an empty level: %s", bad.c_str());
        CHECK(level == 0 && el[0].valid == 0u && el[1].valid == 0u, "an empty level has no data");
        pcbw::BigWig blocks;
        CHECK(ws::level_blocks(image.data(), image.size(), 0u, levels, 0, blocks).empty() && blocks.blocks.empty(), "level_blocks of an empty level");
        CHECK(!ws::level_blocks(image.data(), image.size(), 0u, levels, (int64_t)levels.size(), blocks).empty(), "a level the file lacks");
    }
    // ---- a truncated level block, stored and compressed
    for (int compress = 0; compress < 2; ++compress) {
        std::vector<uint8_t> image = write_file(64, compress);
        pcbw::BigWig f;
        CHECK(pcbw::parse(image.data(), image.size(), f) == pcbw::kNoDefect, "the file parses");
        std::vector<pcbww::ZoomHeader> levels;
        CHECK(pcbww::zoom_headers(image.data(), image.size(), levels).empty() && !levels.empty(), "levels");
        std::string bad = query(image, 0, 0, 64, 2, el, &level);
        CHECK(bad.empty() && level == 0 && el[0].valid > 0u, "whole: %s", bad.c_str());
        uint8_t *leaf = image.data() + levels[0].index + 48;
        CHECK(leaf[0] == 1 && pcbw::rd16(leaf + 2) >= 1, "the level's root is a leaf");
        const uint64_t size = pcbw::rd64(leaf + 4 + 24);
        CHECK(size > 9, "the block holds bytes");
        put64(leaf + 4 + 24, size - 5);
        bad = query(image, 0, 0, 64, 2, el, &level);
        CHECK(!bad.empty() && bad.find("zoom level 0: block 0: ") == 0, "a truncated block (compress %d) is refused: '%s'", compress, bad.c_str());
        pcbw::BigWig blocks;
        const std::string lb = ws::level_blocks(image.data(), image.size(), f.uncompress_buf, levels, 0, blocks);
        CHECK(compress ? lb.empty() : lb == bad, "level_blocks: '%s'", lb.c_str());       // (a compressed block's length shows when it inflates)
        // the items of that file are still read
        bad = query(image, 0, 9, 14, 1, el, &level);
        CHECK(bad.empty() && level == ws::kItems && el[0].valid == 3u && el[0].mn == 3.0 && el[0].sum == 9.0, "the items beside a broken level");
    }
    // ---- the order check
    {
        const ws::ItemRec sorted[4] = {{0, 0, 5, 1.f}, {0, 5, 9, 2.f}, {2, 1, 3, 1.f}, {2, 3, 4, 1.f}};
        ws::Ranges g;
        ws::index_table(sorted, 4, 3, g);
        CHECK(g.ordered && g.lo[0] == 0 && g.hi[0] == 2 && g.lo[1] == 0 && g.hi[1] == 0 && g.lo[2] == 2 && g.hi[2] == 4, "ranges");
        const ws::ItemRec back[3] = {{0, 4, 9, 1.f}, {0, 2, 10, 2.f}, {0, 11, 12, 1.f}};
        ws::index_table(back, 3, 1, g);
        CHECK(!g.ordered, "a start that decreases");
        const ws::ItemRec nested[2] = {{0, 2, 9, 1.f}, {0, 3, 5, 2.f}};
        ws::index_table(nested, 2, 1, g);
        CHECK(!g.ordered, "an end that decreases");
        const ws::ItemRec split[3] = {{0, 2, 9, 1.f}, {1, 3, 5, 2.f}, {0, 10, 12, 1.f}};
        ws::index_table(split, 3, 2, g);
        CHECK(!g.ordered, "a contig in two runs");
        const ws::ItemRec outside[1] = {{7, 2, 9, 1.f}};
        ws::index_table(outside, 1, 2, g);
        CHECK(!g.ordered, "a chromId outside the tree");
        ws::index_table(sorted, 0, 3, g);
        CHECK(g.ordered, "an empty table is in order");
        CHECK(ws::first_end_above(sorted, 0, 2, 4) == 0 && ws::first_end_above(sorted, 0, 2, 5) == 1 && ws::first_end_above(sorted, 0, 2, 9) == 2, "the search");
    }
    // ---- rules 1, 2 and the arguments
    {
        const uint32_t red[4] = {140, 560, 2240, 560};
        CHECK(ws::choose_level(red, 4, 0, 3, 1) == ws::kItems && ws::choose_level(red, 4, 0, 279, 1) == ws::kItems && ws::choose_level(red, 4, 0, 280, 1) == 0, "the first level");
        CHECK(ws::choose_level(red, 4, 0, 1120, 1) == 1 && ws::choose_level(red, 4, 5, 0x7fffffffu, 1) == 2 && ws::choose_level(red, 0, 0, 1000000, 1) == ws::kItems, "ties, the top, no levels");
        CHECK(ws::bin_edge(3, 0x7fffffffu, 6, 7) == 0x7fffffffu && ws::bin_start(3, 10, 0, 3) == 3u && ws::bin_edge(3, 10, 0, 3) == 5u && ws::bin_edge(3, 10, 1, 3) == 7u, "edges");
        const int64_t s[2] = {0, 5}, e[2] = {4, 5}, big[1] = {(int64_t)1 << 31};
        CHECK(ws::check_queries(1, s, e, 3).empty() && !ws::check_queries(2, s, e, 3).empty() && !ws::check_queries(1, s, e, 0).empty() && !ws::check_queries(1, s, big, 1).empty(), "arguments");
    }
    printf("ok\n");
    return 0;
}
