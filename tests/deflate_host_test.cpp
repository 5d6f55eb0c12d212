// deflate_host_test.cpp -- the model encoder of csrc/deflate_host.h as a program of its own, built under the address and
// undefined-behaviour sanitizers (tests/test_deflate_host.py).  argv[1]: a file of inputs -- u32 count, then per input u32
// length and the bytes.  Every input is encoded; zlib's uncompress must return it, the trailer must be zlib's Adler-32 of
// it, the stream may not exceed the input by more than 11 bytes, and encoding twice gives the same bytes.  Then the codes:
// every length 3 .. 258 and every distance 1 .. 32 768 through length_code / distance_code against the tables of RFC 1951.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <zlib.h>

#include "deflate_host.h"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++fails; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static const uint32_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const uint32_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint32_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
static const uint32_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s inputs.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    size_t smaller = 0, stored_n = 0;
    for (uint32_t k = 0; k < count; ++k) {
        uint32_t n = 0;
        if (fread(&n, 4, 1, f) != 1) return 2;
        std::vector<uint8_t> raw(n);   // (exactly n bytes: a read past the input is the sanitizer's)
        if (n && fread(raw.data(), 1, n, f) != n) return 2;
        std::vector<uint8_t> a, b;
        bool stored = false;
        pcdeflate::encode(raw.data(), n, a, &stored);
        pcdeflate::encode(raw.data(), n, b);
        CHECK(a == b, "input %u: two encodings differ", k);
        CHECK(a.size() <= (size_t)n + 11, "input %u: %zu bytes from %u", k, a.size(), n);
        CHECK(a.size() >= 6 && a[0] == 0x78 && a[1] == 0x01, "input %u: header", k);
        std::vector<uint8_t> back((size_t)n + 1);
        uLongf got = (uLongf)back.size();
        const int rc = uncompress(back.data(), &got, a.data(), (uLong)a.size());
        CHECK(rc == Z_OK && got == n && (n == 0 || memcmp(back.data(), raw.data(), n) == 0), "input %u: uncompress gave %d, %lu bytes", k, rc, (unsigned long)got);
        const uint32_t ad = (uint32_t)adler32(adler32(0L, Z_NULL, 0), raw.data(), n);
        const uint8_t *t = a.data() + a.size() - 4;
        CHECK((((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3]) == ad, "input %u: Adler-32", k);
        CHECK(pcdeflate::adler32(raw.data(), n) == ad, "input %u: adler32 of the header", k);
        CHECK(stored == (a.size() == (size_t)n + 11), "input %u: stored flag", k);
        smaller += a.size() < n; stored_n += stored;
    }
    fclose(f);
    for (uint32_t len = 3; len <= 258; ++len) {
        uint32_t s, e, ne;
        pcdeflate::length_code(len, s, e, ne);
        CHECK(s >= 257 && s <= 285 && ne == kLenExtra[s - 257] && kLenBase[s - 257] + e == len && e < (1u << ne), "length %u -> %u + %u / %u", len, s, e, ne);
        if (len < 258) CHECK(s < 285 && kLenBase[s - 257 + 1] > len, "length %u takes symbol %u", len, s);
    }
    for (uint32_t d = 1; d <= 32768; ++d) {
        uint32_t c, e, ne;
        pcdeflate::distance_code(d, c, e, ne);
        CHECK(c < 30 && ne == kDistExtra[c] && kDistBase[c] + e == d && e < (1u << ne), "distance %u -> %u + %u / %u", d, c, e, ne);
    }
    // the fixed code is a prefix code of the lengths RFC 1951 3.2.6 gives
    for (uint32_t s = 0; s < 288; ++s) {
        const pcdeflate::Bits b = pcdeflate::fixed_symbol(s);
        const uint32_t want = s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8));
        CHECK(b.n == want && b.value < (1u << b.n), "symbol %u", s);
    }
    printf("deflate_host: %u inputs, %zu smaller than their input, %zu stored\n", count, smaller, stored_n);
    if (fails) { printf("deflate_host: %d FAILED\n", fails); return 1; }
    printf("deflate_host: ok\n");
    return 0;
}
