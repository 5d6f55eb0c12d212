// deflate_dynamic_host_test.cpp -- the DYNAMIC mode of the model encoder of csrc/deflate_host.h as a program of its own,
// built under the address and undefined-behaviour sanitizers (tests/test_deflate_dynamic_host.py).
//   argv[1]: a file of inputs -- u32 count, then per input u32 length and the bytes.  Every input is encoded in dynamic mode
//            and in fixed mode; zlib's uncompress must return it from the dynamic stream, the trailer must be zlib's
//            Adler-32, the dynamic stream is never longer than the fixed one, equals it when its block is not dynamic, the
//            reported block type is the BTYPE in the stream, and encoding twice gives the same bytes.
//   argv[2]: a file of counts -- u32 cases, then per case u32 n, u32 limit and n u32 counts.  build_code must give a complete
//            code within the limit, lengths exactly for the used symbols (after padding), never growing with (count,
//            symbol), and leave the counts as they came.
// Then cl_order against RFC 1951's list and the extra-bit functions against the tables.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>
#include <zlib.h>

#include "deflate_host.h"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static const uint32_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint32_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
static const uint32_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

static bool read_u32(FILE *f, uint32_t &v) { return fread(&v, 4, 1, f) == 1; }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s inputs.bin counts.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t count = 0;
    if (!read_u32(f, count)) return 2;
    size_t by_type[3] = {0, 0, 0}, dynamic_bytes = 0, fixed_bytes = 0;
    for (uint32_t k = 0; k < count; ++k) {
        uint32_t n = 0;
        if (!read_u32(f, n)) return 2;
        std::vector<uint8_t> raw(n);   // (exactly n bytes: a read past the input is the sanitizer's)
        if (n && fread(raw.data(), 1, n, f) != n) return 2;
        std::vector<uint8_t> a, b, fx;
        uint32_t type = 99u, fixed_type = 99u;
        pcdeflate::encode(raw.data(), n, a, pcdeflate::kDynamic, &type);
        pcdeflate::encode(raw.data(), n, b, pcdeflate::kDynamic);
        pcdeflate::encode(raw.data(), n, fx, pcdeflate::kFixed, &fixed_type);
        CHECK(a == b, "input %u: two encodings differ", k);
        CHECK(type <= 2u && fixed_type <= 1u, "input %u: block types %u, %u", k, type, fixed_type);
        CHECK(a.size() <= fx.size() && a.size() <= (size_t)n + 11, "input %u: %zu bytes, fixed mode %zu, from %u", k, a.size(), fx.size(), n);
        CHECK(a.size() >= 6 && a[0] == 0x78 && a[1] == 0x01 && (a[2] & 1u) == 1u && ((a[2] >> 1) & 3u) == type, "input %u: header", k);
        if (type == pcdeflate::kDynamic) CHECK(a.size() < fx.size(), "input %u: a dynamic block of %zu bytes against %zu", k, a.size(), fx.size());
        else CHECK(a == fx && type == fixed_type, "input %u: not dynamic, and not the fixed mode's stream", k);
        std::vector<uint8_t> back((size_t)n + 1);
        uLongf got = (uLongf)back.size();
        const int rc = uncompress(back.data(), &got, a.data(), (uLong)a.size());
        CHECK(rc == Z_OK && got == n && (n == 0 || memcmp(back.data(), raw.data(), n) == 0), "input %u: uncompress gave %d, %lu bytes", k, rc, (unsigned long)got);
        const uint32_t ad = (uint32_t)adler32(adler32(0L, Z_NULL, 0), raw.data(), n);
        const uint8_t *t = a.data() + a.size() - 4;
        CHECK((((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3]) == ad, "input %u: Adler-32", k);
        if (type <= 2u) ++by_type[type];
        dynamic_bytes += a.size(); fixed_bytes += fx.size();
    }
    fclose(f);

    f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    uint32_t cases = 0;
    if (!read_u32(f, cases)) return 2;
    for (uint32_t k = 0; k < cases; ++k) {
        uint32_t n = 0, limit = 0;
        if (!read_u32(f, n) || !read_u32(f, limit) || n < 2 || n > pcdeflate::kLitSyms) return 2;
        std::vector<uint32_t> counts(n), weight(n), codes(n);
        if (fread(counts.data(), 4, n, f) != n) return 2;
        const std::vector<uint32_t> before = counts;
        std::vector<uint16_t> order(n), parent(2 * (size_t)n), depth(n);   // (exactly what build_code says it needs)
        std::vector<uint8_t> lengths(n, 0xEE);
        uint32_t bl_count[16], next_code[16];
        pcdeflate::build_code(counts.data(), n, limit, order.data(), weight.data(), parent.data(), depth.data(), bl_count, next_code, lengths.data(), codes.data());
        CHECK(counts == before, "case %u: the counts changed", k);
        std::vector<uint32_t> padded = before;
        size_t used = 0;
        for (uint32_t s = 0; s < n; ++s) used += padded[s] != 0;
        for (uint32_t s = 0; s < n && used < 2; ++s)
            if (!padded[s]) { padded[s] = 1; ++used; }
        uint64_t kraft = 0;
        std::vector<std::pair<std::pair<uint32_t, uint32_t>, uint32_t>> by_key;
        for (uint32_t s = 0; s < n; ++s) {
            CHECK((lengths[s] != 0) == (padded[s] != 0) && lengths[s] <= limit, "case %u: symbol %u of count %u has length %u", k, s, before[s], lengths[s]);
            if (lengths[s] && lengths[s] <= limit) kraft += (uint64_t)1 << (limit - lengths[s]);
            if (padded[s]) by_key.push_back({{padded[s], s}, lengths[s]});
            CHECK((codes[s] >> 16) == lengths[s] && (codes[s] & 0xffffu) < (1u << lengths[s]), "case %u: code of symbol %u", k, s);
        }
        CHECK(kraft == (uint64_t)1 << limit, "case %u: Kraft sum %llu of %llu", k, (unsigned long long)kraft, (unsigned long long)1 << limit);
        std::sort(by_key.begin(), by_key.end());
        for (size_t i = 1; i < by_key.size(); ++i) CHECK(by_key[i - 1].second >= by_key[i].second, "case %u: length grows with (count, symbol) at %zu", k, i);
        // canonical: among equal lengths the codes rise with the symbol; a shorter length's codes lie below
        for (uint32_t s = 0; s < n; ++s)
            for (uint32_t t = s + 1; t < n; ++t)
                if (lengths[s] && lengths[s] == lengths[t])
                    CHECK(pcdeflate::bit_reverse(codes[s] & 0xffffu, lengths[s]) < pcdeflate::bit_reverse(codes[t] & 0xffffu, lengths[t]), "case %u: codes of %u and %u", k, s, t);
    }
    fclose(f);

    for (uint32_t i = 0; i < 19; ++i) CHECK(pcdeflate::cl_order(i) == kClOrder[i], "cl_order(%u) = %u", i, pcdeflate::cl_order(i));
    for (uint32_t s = 0; s < 257; ++s) CHECK(pcdeflate::length_extra_bits(s) == 0, "symbol %u", s);
    for (uint32_t s = 257; s < 286; ++s) CHECK(pcdeflate::length_extra_bits(s) == kLenExtra[s - 257], "symbol %u", s);
    for (uint32_t c = 0; c < 30; ++c) CHECK(pcdeflate::distance_extra_bits(c) == kDistExtra[c], "distance code %u", c);
    for (uint32_t s = 0; s < 286; ++s) CHECK(pcdeflate::fixed_length(s) == pcdeflate::fixed_symbol(s).n, "fixed length of %u", s);

    printf("deflate_dynamic_host: %u inputs: %zu stored, %zu fixed, %zu dynamic blocks; %zu bytes against %zu in fixed mode; %u count cases\n", count, by_type[0], by_type[1],
           by_type[2], dynamic_bytes, fixed_bytes, cases);
    if (fails) { printf("deflate_dynamic_host: %d FAILED\n", fails); return 1; }
    printf("deflate_dynamic_host: ok\n");
    return 0;
}
