// deflate_host.h -- the zlib ENCODER of this project, stated once (revision 19).  HIP-free: the host library compiles it
// as the serial model encoder (pcdeflate::encode, exported as pb_deflate_zlib), deflate_kernels.hip.h compiles its hash,
// its codes and its limits into k_zlib_deflate.  Device bytes equal model bytes, byte for byte.
//
// An input of n <= kMaxInput bytes becomes one RFC 1950 stream: 78 01, a DEFLATE body of ONE block, Adler-32 big-endian.
//
// The rule, serially:
//   candidate   for every position p with p + 4 <= n: the NEAREST earlier position q < p whose four bytes hash alike
//               (hash4: 12 bits of the little-endian word times 2654435761).  Every position enters the search, whether a
//               token starts there or not, so cand(p) is a function of the bytes alone.
//   match       when the four bytes at q equal those at p: the length is extended byte by byte (the source may run into
//               its own output: distance 1 is a run) up to min(258, n - p).  Matches are 4 .. 258 long; no candidate, or
//               a hash collision, leaves a literal.
//   parse       greedy from position 0: a match at p is taken whole, the next token starts at p + length.
//   code        the fixed Huffman tables (BTYPE = 01): 3 header bits, the tokens, the 7-bit end of block.
//   fallback    when the coded body is not smaller than a stored block (5 + n bytes), the body IS one stored block
//               (BTYPE = 00).  So a stream never exceeds n + 11 bytes.
// Dynamic codes (BTYPE = 10) are not built.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define PC_DF_HD __host__ __device__
#else
#define PC_DF_HD
#endif

namespace pcdeflate {

constexpr uint32_t kMaxInput = 24600u;       // one bedGraph section of 2 048 items: 24 + 2 048 x 12
constexpr uint32_t kHashBits = 12u;
constexpr uint32_t kMinMatch = 4u, kMaxMatch = 258u;
constexpr uint32_t kStreamOverhead = 11u;    // 2 header + 5 stored-block header + 4 trailer: the most a stream adds
constexpr uint32_t kSlotPad = 16u;           // stream k is produced into a slot of len[k] + 16 bytes
constexpr uint8_t kCmf = 0x78u, kFlg = 0x01u;
constexpr uint32_t kAdlerMod = 65521u;

PC_DF_HD inline uint32_t hash4(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) {
    const uint32_t w = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    return (w * 2654435761u) >> (32u - kHashBits);
}

PC_DF_HD inline uint32_t floor_log2(uint32_t x) {   // x >= 1
    uint32_t k = 0;
    while (x >>= 1) ++k;
    return k;
}
PC_DF_HD inline uint32_t bit_reverse(uint32_t code, uint32_t nbits) {
    uint32_t r = 0;
    for (uint32_t k = 0; k < nbits; ++k) r |= ((code >> k) & 1u) << (nbits - 1u - k);
    return r;
}

// A token as the bits it adds to the stream, first bit lowest.  At most 31 bits (8 + 5 of a length, 5 + 13 of a distance).
struct Bits { uint32_t value, n; };

// the fixed literal/length code of symbol s (0 .. 287), already reversed into stream order
PC_DF_HD inline Bits fixed_symbol(uint32_t s) {
    if (s < 144u) return Bits{bit_reverse(0x30u + s, 8u), 8u};
    if (s < 256u) return Bits{bit_reverse(0x190u + (s - 144u), 9u), 9u};
    if (s < 280u) return Bits{bit_reverse(s - 256u, 7u), 7u};
    return Bits{bit_reverse(0xC0u + (s - 280u), 8u), 8u};
}
PC_DF_HD inline Bits literal_bits(uint32_t byte) { return fixed_symbol(byte); }
PC_DF_HD inline Bits end_of_block_bits() { return fixed_symbol(256u); }

// the length symbol of len (3 .. 258), its extra bits and their count (RFC 1951 3.2.5)
PC_DF_HD inline void length_code(uint32_t len, uint32_t &symbol, uint32_t &extra, uint32_t &nextra) {
    const uint32_t x = len - 3u;
    if (len == 258u) { symbol = 285u; extra = 0u; nextra = 0u; }
    else if (x < 8u) { symbol = 257u + x; extra = 0u; nextra = 0u; }
    else {
        const uint32_t e = floor_log2(x) - 2u;
        symbol = 261u + 4u * e + ((x >> e) & 3u); extra = x & ((1u << e) - 1u); nextra = e;
    }
}
// the distance code of dist (1 .. 32 768), its extra bits and their count
PC_DF_HD inline void distance_code(uint32_t dist, uint32_t &code, uint32_t &extra, uint32_t &nextra) {
    const uint32_t y = dist - 1u;
    if (y < 4u) { code = y; extra = 0u; nextra = 0u; }
    else {
        const uint32_t nb = floor_log2(y), e = nb - 1u;
        code = 2u * nb + ((y >> e) & 1u); extra = y & ((1u << e) - 1u); nextra = e;
    }
}
PC_DF_HD inline Bits match_bits(uint32_t len, uint32_t dist) {
    uint32_t ls, le, ln, dc, de, dn;
    length_code(len, ls, le, ln);
    distance_code(dist, dc, de, dn);
    Bits b = fixed_symbol(ls);
    b.value |= le << b.n; b.n += ln;
    b.value |= bit_reverse(dc, 5u) << b.n; b.n += 5u;
    b.value |= de << b.n; b.n += dn;
    return b;
}

// the length of the match of position p against the candidate q < p: 0 when the first four bytes differ
PC_DF_HD inline uint32_t match_length(const uint8_t *raw, uint32_t n, uint32_t q, uint32_t p) {
    if (raw[q] != raw[p] || raw[q + 1] != raw[p + 1] || raw[q + 2] != raw[p + 2] || raw[q + 3] != raw[p + 3]) return 0u;
    const uint32_t most = n - p < kMaxMatch ? n - p : kMaxMatch;
    uint32_t l = kMinMatch;
    while (l < most && raw[q + l] == raw[p + l]) ++l;
    return l;
}

// bytes of the fixed-coded body of `bits` bits, and whether the stream takes it (else: the stored block)
PC_DF_HD inline bool takes_fixed(uint64_t bits, uint32_t n) { return (bits + 7u) / 8u < 5ull + n; }

inline uint32_t adler32(const uint8_t *p, size_t n) {
    uint32_t a = 1u, b = 0u;
    while (n) {
        const size_t k = n < 5552u ? n : 5552u;
        for (size_t i = 0; i < k; ++i) { a += p[i]; b += a; }
        a %= kAdlerMod; b %= kAdlerMod;
        p += k; n -= k;
    }
    return (b << 16) | a;
}

// per-position matches of `raw`: len[p] (0: a literal) and dist[p]
inline void find_matches(const uint8_t *raw, uint32_t n, std::vector<uint16_t> &len, std::vector<uint16_t> &dist) {
    len.assign(n, 0); dist.assign(n, 0);
    std::vector<int32_t> head((size_t)1 << kHashBits, -1);
    for (uint32_t p = 0; p + 4u <= n; ++p) {
        const uint32_t h = hash4(raw[p], raw[p + 1], raw[p + 2], raw[p + 3]);
        const int32_t q = head[h];
        head[h] = (int32_t)p;
        if (q < 0) continue;
        const uint32_t l = match_length(raw, n, (uint32_t)q, p);
        if (l) { len[p] = (uint16_t)l; dist[p] = (uint16_t)(p - (uint32_t)q); }
    }
}

// The model encoder: the zlib stream of raw[0, n), n <= kMaxInput, appended to `out`.  *stored (when given): the body is
// the stored block.
inline void encode(const uint8_t *raw, uint32_t n, std::vector<uint8_t> &out, bool *stored = nullptr) {
    std::vector<uint16_t> len, dist;
    find_matches(raw, n, len, dist);
    std::vector<uint8_t> body;
    uint64_t acc = 0;
    uint32_t nacc = 0;
    uint64_t total = 0;
    auto put = [&](Bits b) {
        acc |= (uint64_t)b.value << nacc; nacc += b.n; total += b.n;
        while (nacc >= 8u) { body.push_back((uint8_t)acc); acc >>= 8; nacc -= 8u; }
    };
    put(Bits{3u, 3u});   // BFINAL = 1, BTYPE = 01
    for (uint32_t p = 0; p < n;) {
        if (len[p]) { put(match_bits(len[p], dist[p])); p += len[p]; }
        else { put(literal_bits(raw[p])); ++p; }
    }
    put(end_of_block_bits());
    if (nacc) body.push_back((uint8_t)acc);
    const bool fixed = takes_fixed(total, n);
    if (stored) *stored = !fixed;
    out.push_back(kCmf); out.push_back(kFlg);
    if (fixed) out.insert(out.end(), body.begin(), body.end());
    else {
        out.push_back(1u);   // BFINAL = 1, BTYPE = 00
        out.push_back((uint8_t)(n & 255u)); out.push_back((uint8_t)(n >> 8));
        out.push_back((uint8_t)(~n & 255u)); out.push_back((uint8_t)((~n >> 8) & 255u));
        out.insert(out.end(), raw, raw + n);
    }
    const uint32_t ad = adler32(raw, n);
    out.push_back((uint8_t)(ad >> 24)); out.push_back((uint8_t)(ad >> 16)); out.push_back((uint8_t)(ad >> 8)); out.push_back((uint8_t)ad);
}

}   // namespace pcdeflate
