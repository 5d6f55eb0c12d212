// The zoom levels of plastid_amd/csrc/bigwig_write_host.h as a program, for the sanitizers (tests/test_bigwig_zoom_host.py
// compiles it with -fsanitize=address,undefined):
//   - the serial model (HostWriter with zoom) over integer-valued contigs, every level read back through zoom_headers /
//     read_zoom_level and compared with a restatement position by position: a window's validCount, minimum, maximum, sum
//     and sum of squares straight from the cells it covers (exact for small integers, whatever the order);
//   - the container: the zoom headers' offsets follow one another from the end of the unzoomed R-tree to the magic, and
//     uncompressBufSize covers every block; zoom = 0 and a file without items carry no level;
//   - the parser: every truncation of a small zoomed file, and every byte of its zoom headers, record counts and zoom
//     R-trees changed three ways, reads or is refused -- never anything else.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bigwig_write_host.h"

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

static uint32_t g_seed = 12345u;
static uint32_t rnd(uint32_t n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }

struct Case { std::vector<pcbww::HostWriter::In> in; };

static Case make_case(int which) {
    Case c;
    const double values[4] = {1.0, 2.0, 3.0, 5.0};
    auto cells = [&](size_t n, uint32_t gap) {
        std::vector<double> v(n, 0.0);
        for (size_t i = 0; i < n;) {
            const size_t len = 1 + rnd(6);
            const double x = values[rnd(4)];
            for (size_t j = i; j < i + len && j < n; ++j) v[j] = x;
            i += len + (rnd(3) == 0 ? rnd(gap) : 0);
        }
        return v;
    };
    if (which == 0) {          // the edges of a grid of 8: shorter than a window, k r0, k r0 + 1, an empty contig, 769 windows
        c.in.push_back({"d_plus1", 25, cells(25, 4)});
        c.in.push_back({"a_short", 5, {0.0, 2.0, 2.0, 0.0, 1.0}});
        c.in.push_back({"c_empty", 40, std::vector<double>(40, 0.0)});
        c.in.push_back({"b_exact", 24, cells(24, 4)});
        c.in.push_back({"e_769", 769 * 8 + 3, cells(769 * 8, 3)});
        c.in.push_back({"f_beyond", 10, cells(37, 40)});
    } else if (which == 1) {   // sparse data on a longer contig
        c.in.push_back({"chr1", 50000, cells(48000, 900)});
        c.in.push_back({"chr2", 513, cells(513, 30)});
    } else {                   // a small file for the damage loop
        c.in.push_back({"x", 70, cells(70, 6)});
        c.in.push_back({"y", 9, cells(9, 2)});
    }
    return c;
}

// the levels of one file against the cells, position by position
static int check_file(const Case &cs, const std::vector<uint8_t> &image, int64_t zoom, uint32_t ips, int compress, const char *what) {
    pcbw::BigWig f;
    CHECK(pcbw::parse(image.data(), image.size(), f) == pcbw::kNoDefect, "%s: the file does not parse", what);
    std::vector<pcbww::ZoomHeader> levels;
    std::string bad = pcbww::zoom_headers(image.data(), image.size(), levels);
    CHECK(bad.empty(), "%s: %s", what, bad.c_str());
    CHECK(levels.size() == f.zoom_levels && !levels.empty() && levels.size() <= 10, "%s: %zu levels", what, levels.size());
    std::vector<pcbww::HostWriter::In> in = cs.in;
    std::sort(in.begin(), in.end(), [](const pcbww::HostWriter::In &a, const pcbww::HostWriter::In &b) { return a.name < b.name; });
    uint64_t items = 0, valid = 0;
    for (const auto &g : in)
        for (size_t i = 0; i < g.cells.size(); ++i)
            if (g.cells[i] != 0.0) { ++valid; items += i == 0 || g.cells[i - 1] != g.cells[i]; }
    const uint32_t r0 = zoom > 0 ? (uint32_t)zoom : (uint32_t)std::min<uint64_t>(4 * std::max<uint64_t>(10, valid / items), 1u << 20);
    size_t below = 0;
    uint64_t at = 0;
    for (size_t k = 0; k < levels.size(); ++k) {
        const uint64_t r = (uint64_t)r0 << (2 * k);
        CHECK(levels[k].reduction == r, "%s: level %zu has reduction %u", what, k, levels[k].reduction);
        if (k) CHECK(levels[k].data == at, "%s: level %zu starts at %llu, the level below ended at %llu", what, k, (unsigned long long)levels[k].data, (unsigned long long)at);
        pcbww::ZoomTable t;
        bad = pcbww::read_zoom_level(image.data(), image.size(), f.uncompress_buf, levels, (int64_t)k, zlib_raw_inflate, t);
        CHECK(bad.empty(), "%s: %s", what, bad.c_str());
        CHECK(!compress || t.largest <= (int64_t)f.uncompress_buf, "%s: a block of %lld bytes, uncompressBufSize %u", what, (long long)t.largest, f.uncompress_buf);
        CHECK(t.largest <= (int64_t)(32u * std::min(ips, 768u)), "%s: a block of %lld bytes", what, (long long)t.largest);
        size_t row = 0;
        for (size_t c = 0; c < in.size(); ++c) {
            const uint64_t size = std::max<uint64_t>((uint64_t)in[c].length, in[c].cells.size());
            for (uint64_t ws = 0; ws < size; ws += r) {
                const uint64_t we = std::min(ws + r, size);
                uint64_t n = 0;
                double lo = 0, hi = 0, sum = 0, sumsq = 0;
                for (uint64_t p = ws; p < we && p < in[c].cells.size(); ++p) {
                    const double v = in[c].cells[p];
                    if (v == 0.0) continue;
                    if (!n || v < lo) lo = v;
                    if (!n || v > hi) hi = v;
                    ++n; sum += v; sumsq += v * v;
                }
                if (!n) continue;
                CHECK(row < t.chrom.size(), "%s: level %zu holds %zu records, the cells give more", what, k, t.chrom.size());
                CHECK(t.chrom[row] == c && t.start[row] == ws && t.end[row] == we && t.valid[row] == n, "%s: level %zu record %zu: (%u, %u, %u, %u)", what, k, row,
                      t.chrom[row], t.start[row], t.end[row], t.valid[row]);
                CHECK(t.mn[row] == (float)lo && t.mx[row] == (float)hi && t.sum[row] == (float)sum && t.sumsq[row] == (float)sumsq, "%s: level %zu record %zu: the values", what, k, row);
                ++row;
            }
        }
        CHECK(row == t.chrom.size() && row == levels[k].records, "%s: level %zu holds %zu records, the cells give %zu", what, k, t.chrom.size(), row);
        CHECK(k == 0 || row < below, "%s: level %zu has %zu records, the level below %zu", what, k, row, below);
        below = row;
        // the level ends with its R-tree: the highest byte of a node
        at = levels[k].index + 48;
        std::vector<uint64_t> todo{levels[k].index + 48};
        while (!todo.empty()) {
            const uint64_t off = todo.back();
            todo.pop_back();
            const bool leaf = image[off] != 0;
            const uint64_t count = pcbw::rd16(image.data() + off + 2);
            at = std::max(at, off + 4 + count * (leaf ? 32u : 24u));
            if (!leaf) for (uint64_t j = 0; j < count; ++j) todo.push_back(pcbw::rd64(image.data() + off + 4 + j * 24 + 16));
        }
    }
    CHECK(at + 4 == image.size() && pcbw::rd32(image.data() + at) == pcbw::kBigWigMagic, "%s: the last level ends at %llu of %zu", what, (unsigned long long)at, image.size());
    return 0;
}

static bool write(const Case &cs, int64_t zoom, uint32_t ips, uint32_t bs, int compress, pcbww::HostWriter &w) {
    w = pcbww::HostWriter();
    w.items_per_slot = ips; w.block_size = bs; w.compress = compress; w.zoom = zoom;
    w.in = cs.in;
    return w.finish();
}

// reads or is refused; the sanitizers judge the rest
static long try_read(const std::vector<uint8_t> &image) {
    pcbw::BigWig f;
    if (pcbw::parse(image.data(), image.size(), f) != pcbw::kNoDefect) return 0;
    std::vector<pcbww::ZoomHeader> levels;
    if (!pcbww::zoom_headers(image.data(), image.size(), levels).empty()) return 0;
    long read = 0;
    for (size_t k = 0; k < levels.size(); ++k) {
        pcbww::ZoomTable t;
        read += pcbww::read_zoom_level(image.data(), image.size(), f.uncompress_buf, levels, (int64_t)k, zlib_raw_inflate, t).empty();
    }
    return read;
}

int main() {
    pcbww::HostWriter w;
    for (int which = 0; which < 2; ++which) {
        const Case cs = make_case(which);
        for (int64_t zoom : {(int64_t)8, (int64_t)-1, (int64_t)64})
            for (uint32_t ips : {1u, 2u, 1024u})
                for (uint32_t bs : {2u, 256u})
                    for (int compress = 0; compress <= 2; ++compress) {
                        char what[96];
                        snprintf(what, sizeof(what), "case %d zoom %lld ips %u bs %u compress %d", which, (long long)zoom, ips, bs, compress);
                        CHECK(write(cs, zoom, ips, bs, compress, w), "%s: %s", what, w.error.c_str());
                        if (check_file(cs, w.image, zoom, ips, compress, what)) return 1;
                        CHECK(w.zoom_stats.size() == pcbw::rd16(w.image.data() + 6), "%s: the statistics", what);
                    }
        // zoom = 0: no level, and the bytes in front of the zoom headers' place are the same file's
        CHECK(write(cs, 0, 1024, 256, 1, w) && pcbw::rd16(w.image.data() + 6) == 0 && w.zoom_stats.empty(), "zoom 0 wrote a level");
    }
    {   // what is refused, and a file without items
        Case none;
        none.in.push_back({"e", 50, std::vector<double>(50, 0.0)});
        CHECK(write(none, -1, 1024, 256, 1, w), "%s", w.error.c_str());
        const std::vector<uint8_t> zoomed = w.image;
        CHECK(write(none, 0, 1024, 256, 1, w) && w.image == zoomed, "a file without items differs under zoom");
        for (int64_t bad : {(int64_t)7, (int64_t)-2, ((int64_t)1 << 24) + 1, (int64_t)1}) CHECK(!write(none, bad, 1024, 256, 1, w) && !w.error.empty(), "zoom %lld was taken", (long long)bad);
        pcbww::ZoomPlan z;
        CHECK(!pcbww::zoom_plan({{"huge", 0xffffffffu}, {"huge2", 0xffffffffu}, {"huge3", 0xffffffffu}, {"huge4", 0xffffffffu}}, 8, z).empty(), "a grid of 2^31 windows was planned");
        CHECK(pcbww::zoom_plan({{"a", 100u}, {"b", 0u}, {"c", 7u}}, 8, z).empty() && z.g.levels == 10 && z.windows() == 14 + 5 + 2 * 8, "the plan of a small grid: %lld windows", (long long)z.windows());
        CHECK(pcbww::zoom_contig_of(z.row(0), 3, 12) == 0 && pcbww::zoom_contig_of(z.row(0), 3, 13) == 2 && pcbww::zoom_level_of(z.g, 14) == 1, "window to contig");
    }
    // damage: every truncation, and every byte of the zoom headers and of everything behind the unzoomed R-tree, three ways
    const Case small = make_case(2);
    long read = 0, tried = 0;
    for (int compress = 0; compress <= 1; ++compress) {
        CHECK(write(small, 8, 2, 2, compress, w), "%s", w.error.c_str());
        const std::vector<uint8_t> image = w.image;
        const long whole = try_read(image);
        CHECK(whole >= 2, "the small file holds %ld levels", whole);
        std::vector<pcbww::ZoomHeader> levels;
        CHECK(pcbww::zoom_headers(image.data(), image.size(), levels).empty(), "the small file's headers");
        for (size_t n = 0; n < image.size(); ++n) {
            // (a copy of exactly n bytes: a read behind the truncated image is a read behind the allocation)
            std::vector<uint8_t> cutv(image.begin(), image.begin() + (long)n);
            read += try_read(cutv); ++tried;
        }
        std::vector<size_t> spots;
        for (size_t i = 6; i < 8; ++i) spots.push_back(i);
        for (size_t i = 52; i < 64 + 24 * levels.size(); ++i) spots.push_back(i);
        for (size_t i = (size_t)levels[0].data; i < image.size(); ++i) spots.push_back(i);
        for (size_t i : spots)
            for (uint8_t x : {(uint8_t)0x01, (uint8_t)0x80, (uint8_t)0xff}) {
                std::vector<uint8_t> v = image;
                v[i] ^= x;
                read += try_read(v); ++tried;
            }
    }
    printf("ok: %ld damaged images, %ld levels still read\n", tried, read);
    return 0;
}
