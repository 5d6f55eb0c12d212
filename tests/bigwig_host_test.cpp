// plastid_amd/csrc/bigwig_host.h as a program, for the sanitizers (tests/test_bigwig_host.py compiles it with
// -fsanitize=address,undefined where the compiler has them):
//   bigwig_host_test SMALL.bw [FILE.bw:ITEMS ...]
// every FILE reads without a defect and gives ITEMS items; SMALL reads, and so does -- or is refused, never anything
// else -- every truncation of it and every image with one byte changed (three ways); the Adler-32 of bigwig_host.h and
// its combination rule against zlib's at the lengths where the sums are reduced.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "bigwig_host.h"

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

static std::vector<uint8_t> slurp(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

static int adler_checks() {
    const size_t lens[] = {0, 1, 63, 64, 65, 5551, 5552, 5553, 11104, 65536, 200000};
    for (size_t n : lens) {
        std::vector<uint8_t> v(n, 0xff);
        for (size_t i = 0; i < n; i += 7) v[i] = (uint8_t)(i * 31);
        uint32_t a = 1, b = 0;
        pcbw::adler_bytes(v.data(), n, a, b);
        const uint32_t want = (uint32_t)adler32(adler32(0L, Z_NULL, 0), v.data(), (uInt)n);
        CHECK(((b << 16) | a) == want, "adler_bytes of %zu bytes", n);
        // every split into two pieces at a few places, combined
        for (size_t cutp : {(size_t)0, n / 3, n / 2, n}) {
            uint32_t a1 = 1, b1 = 0, a2 = 1, b2 = 0;
            pcbw::adler_bytes(v.data(), cutp, a1, b1);
            pcbw::adler_bytes(v.data() + cutp, n - cutp, a2, b2);
            pcbw::adler_combine(a1, b1, a2, b2, n - cutp);
            CHECK(((b1 << 16) | a1) == want, "adler_combine of %zu + %zu bytes", cutp, n - cutp);
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: bigwig_host_test SMALL.bw [FILE.bw:ITEMS ...]\n"); return 2; }
    if (adler_checks()) return 1;
    pcbw::ItemTable t;
    for (int k = 2; k < argc; ++k) {
        const std::string arg = argv[k];
        const size_t colon = arg.rfind(':');
        const std::vector<uint8_t> image = slurp(arg.substr(0, colon));
        pcbw::read_items(image.data(), image.size(), zlib_raw_inflate, t);
        CHECK(t.defect == pcbw::kNoDefect, "%s", pcbw::defect_message(arg.c_str(), t.defect).c_str());
        CHECK((long long)t.chrom.size() == atoll(arg.c_str() + colon + 1), "%s: %zu items", arg.c_str(), t.chrom.size());
        for (size_t i = 0; i < t.chrom.size(); ++i)
            CHECK(t.start[i] < t.stop[i] && t.stop[i] <= (int64_t)t.file.chroms[(size_t)t.chrom[i]].size, "%s: item %zu", arg.c_str(), i);
    }
    const std::vector<uint8_t> small = slurp(argv[1]);
    pcbw::read_items(small.data(), small.size(), zlib_raw_inflate, t);
    CHECK(t.defect == pcbw::kNoDefect && !t.chrom.empty(), "the small file does not read");
    const size_t items = t.chrom.size();
    long refused = 0, read = 0;
    for (size_t n = 0; n < small.size(); ++n) {
        // (a copy of exactly n bytes: a read behind the truncated image is a read behind the allocation)
        std::vector<uint8_t> cutv(small.begin(), small.begin() + (long)n);
        pcbw::read_items(cutv.data(), cutv.size(), zlib_raw_inflate, t);
        if (t.defect == pcbw::kNoDefect) ++read; else ++refused;
        CHECK(t.defect == pcbw::kNoDefect || !pcbw::defect_message("x", t.defect).empty(), "truncation %zu", n);
    }
    // (the file ends with the magic and, in front of it, the index: a cut inside either is noticed or cuts nothing that is read)
    for (size_t i = 0; i < small.size(); ++i)
        for (uint8_t x : {(uint8_t)0xff, (uint8_t)0x01, (uint8_t)0x80}) {
            std::vector<uint8_t> v(small);
            v[i] ^= x;
            pcbw::read_items(v.data(), v.size(), zlib_raw_inflate, t);
            if (t.defect == pcbw::kNoDefect) {
                ++read;
                for (size_t k = 0; k < t.chrom.size(); ++k)
                    CHECK(t.chrom[k] >= 0 && (size_t)t.chrom[k] < t.file.chroms.size() && t.start[k] < t.stop[k] &&
                          t.stop[k] <= (int64_t)t.file.chroms[(size_t)t.chrom[k]].size, "byte %zu ^ %u: item %zu", i, (unsigned)x, k);
            } else ++refused;
        }
    printf("bigwig_host: ok (%zu items; %ld damaged images refused, %ld read)\n", items, refused, read);
    return 0;
}
