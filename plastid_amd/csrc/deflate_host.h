// deflate_host.h -- the zlib ENCODER of this project, stated once (revision 20).  HIP-free: the host library compiles it
// as the serial model encoder (pcdeflate::encode, exported as pb_deflate_zlib / pb_deflate_zlib_mode),
// deflate_kernels.hip.h compiles its hash, its codes, its trees and its limits into k_zlib_deflate.  Device bytes equal
// model bytes, byte for byte.
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
//   code        mode kFixed: the fixed Huffman tables (BTYPE = 01): 3 header bits, the tokens, the 7-bit end of block.
//               mode kDynamic: the tokens are the same; the block's own codes (BTYPE = 10) are built as below.
//   fallback    when the coded body is not smaller than a stored block (5 + n bytes), the body IS one stored block
//               (BTYPE = 00).  So a stream never exceeds n + 11 bytes.
//
// The dynamic codes (mode kDynamic), every step a function of the token sequence alone:
//   histograms  literal/length symbols 0 .. 285 (the end of block once) and distance codes 0 .. 29.
//   padding     an alphabet with fewer than two used symbols: the lowest-numbered unused symbols count 1 until two are
//               used (pad_counts; zlib's build_tree does the same), so every code below is COMPLETE (Kraft sum 1).  The
//               padded symbols get a length and never occur.
//   order       the used symbols ascending by the total order (count, symbol): rank_of.
//   merge       Huffman's merge in the two-queue form over that order: the two lightest of (next leaf, next internal node)
//               are joined, a leaf before an internal node of equal weight (lengths_from_order).
//   limit       depths above the limit (15, 15, 7 for literal/length, distance, code-length alphabet) count at the limit;
//               the Kraft sum then exceeds 1 by e units of 2^-limit, and e times the deepest leaf above the limit goes
//               one level down and takes one leaf of the limit level as its sibling (the step of zlib's gen_bitlen, each
//               takes off one unit).  Then the lengths are handed out by level, longest first, in (count, symbol) order:
//               length never grows with (count, symbol), and without a clamped depth the cost is the optimal one.
//   codes       canonical (RFC 1951 3.2.2): canonical_code.
//   header      HLIT, HDIST trimmed of trailing zero lengths (minima 257, 1); the HLIT + HDIST lengths as ONE sequence
//               run-length coded by zlib's scan_tree rule (scan_lengths: a run of a non-zero length is the length once,
//               then 16 for 3 .. 6 repeats; zeros go out as 17 for 3 .. 10 and 18 for 11 .. 138; shorter runs verbatim);
//               the code-length code over those symbols (limit 7), its lengths in the permuted order, HCLEN trimmed
//               (minimum 4).
//   choice      the body sizes in bytes are known from histograms and lengths before a bit goes out.  The body is the
//               dynamic one iff it is smaller than the fixed body AND smaller than the stored block (choose_block);
//               else the fixed body by takes_fixed, else the stored block.  So a dynamic-mode stream is never longer
//               than the fixed-mode stream of the same input.
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
constexpr uint32_t kStored = 0u, kFixed = 1u, kDynamic = 2u;   // BTYPE of a stream's block; kFixed and kDynamic are also the modes
constexpr uint32_t kLitSyms = 286u, kDistSyms = 30u, kClSyms = 19u;
constexpr uint32_t kLitLimit = 15u, kDistLimit = 15u, kClLimit = 7u;
constexpr uint32_t kEndOfBlock = 256u;

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

// ---------------------------------------------------------------- dynamic codes (the header comment states the rule)
// extra bits behind a literal/length symbol and behind a distance code
PC_DF_HD inline uint32_t length_extra_bits(uint32_t s) { return (s < 265u || s == 285u) ? 0u : (s - 261u) >> 2; }
PC_DF_HD inline uint32_t distance_extra_bits(uint32_t c) { return c < 4u ? 0u : (c >> 1) - 1u; }
PC_DF_HD inline uint32_t fixed_length(uint32_t s) { return s < 144u ? 8u : (s < 256u ? 9u : (s < 280u ? 7u : 8u)); }
// the order in which the code-length code lengths stand in the header: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
PC_DF_HD inline uint32_t cl_order(uint32_t i) {
    if (i < 3u) return 16u + i;
    const uint32_t k = i - 3u;
    return k == 0u ? 0u : ((k & 1u) ? 8u + (k - 1u) / 2u : 8u - k / 2u);
}

// `used` of the n counts are non-zero.  Until two are: the lowest-numbered zero count becomes 1; padded[0 .. 1] name those
// symbols (n: none) so that the caller can take the counts back once the lengths stand.  Returns the used symbols (>= 2).
PC_DF_HD inline uint32_t pad_counts(uint32_t *counts, uint32_t n, uint32_t used, uint32_t *padded) {
    padded[0] = n; padded[1] = n;
    for (uint32_t s = 0; used < 2u && s < n; ++s)
        if (!counts[s]) {
            counts[s] = 1u; ++used;
            if (padded[0] == n) padded[0] = s; else padded[1] = s;
        }
    return used;
}
PC_DF_HD inline void unpad_counts(uint32_t *counts, uint32_t n, const uint32_t *padded) {
    if (padded[0] < n) counts[padded[0]] = 0u;
    if (padded[1] < n) counts[padded[1]] = 0u;
}

// the place of the used symbol s in the order (count, symbol) of the used symbols
PC_DF_HD inline uint32_t rank_of(const uint32_t *counts, uint32_t n, uint32_t s) {
    const uint32_t c = counts[s];
    uint32_t r = 0;
    for (uint32_t t = 0; t < n; ++t) {
        const uint32_t ct = counts[t];
        r += (ct != 0u && (ct < c || (ct == c && t < s))) ? 1u : 0u;
    }
    return r;
}

// Code lengths of the m >= 2 used symbols order[0, m) (ascending by (count, symbol); 2^limit >= m): merge, limit, levels.
// lengths[] of the unused symbols is the caller's (0).  Scratch: weight[m], parent[2 m], depth[m], bl_count[16]; bl_count
// leaves as the number of codes of every length.
PC_DF_HD inline void lengths_from_order(const uint32_t *counts, const uint16_t *order, uint32_t m, uint32_t limit, uint32_t *weight, uint16_t *parent,
                                        uint16_t *depth, uint32_t *bl_count, uint8_t *lengths) {
    // nodes: the leaves 0 .. m - 1 in order, the internal nodes m .. 2 m - 2 as they are made (their weights never fall)
    uint32_t li = 0u, ii = 0u;
    for (uint32_t made = 0u; made + 1u < m; ++made) {
        uint32_t w = 0u;
        for (uint32_t pick = 0u; pick < 2u; ++pick) {
            const uint32_t lw = li < m ? counts[order[li]] : 0u;
            if (li < m && (ii >= made || lw <= weight[ii])) { w += lw; parent[li++] = (uint16_t)(m + made); }
            else { w += weight[ii]; parent[m + ii++] = (uint16_t)(m + made); }
        }
        weight[made] = w;
    }
    depth[m - 2u] = 0u;                                  // the root
    for (uint32_t i = m - 2u; i-- > 0u;) depth[i] = (uint16_t)(depth[parent[m + i] - m] + 1u);
    for (uint32_t b = 0u; b < 16u; ++b) bl_count[b] = 0u;
    uint32_t kraft = 0u;                                 // in units of 2^-limit
    for (uint32_t j = 0u; j < m; ++j) {
        uint32_t d = depth[parent[j] - m] + 1u;
        if (d > limit) d = limit;
        ++bl_count[d];
        kraft += 1u << (limit - d);
    }
    for (uint32_t excess = kraft - (1u << limit); excess > 0u; --excess) {
        uint32_t bits = limit - 1u;
        while (bits > 0u && !bl_count[bits]) --bits;
        if (!bits) break;                                // (2^limit >= m: a leaf above the limit level exists)
        --bl_count[bits]; bl_count[bits + 1u] += 2u; --bl_count[limit];
    }
    uint32_t j = 0u;
    for (uint32_t bits = limit; bits > 0u; --bits)
        for (uint32_t k = bl_count[bits]; k > 0u; --k) lengths[order[j++]] = (uint8_t)bits;
}

// the first code of every length (RFC 1951 3.2.2) from the number of codes of every length
PC_DF_HD inline void first_codes(const uint32_t *bl_count, uint32_t *next_code) {
    uint32_t code = 0u;
    next_code[0] = 0u;
    for (uint32_t b = 1u; b < 16u; ++b) { code = (code + (b > 1u ? bl_count[b - 1u] : 0u)) << 1; next_code[b] = code; }
}
// the canonical code of symbol s as a table entry: the code in stream order (reversed) | length << 16; 0 for length 0
PC_DF_HD inline uint32_t canonical_code(const uint8_t *lengths, const uint32_t *next_code, uint32_t s) {
    const uint32_t l = lengths[s];
    if (!l) return 0u;
    uint32_t code = next_code[l];
    for (uint32_t t = 0u; t < s; ++t) code += lengths[t] == l ? 1u : 0u;
    return bit_reverse(code, l) | (l << 16);
}

// The whole way from n counts (at least `used` of them non-zero is the caller's count) to lengths and code table, serially:
// padding, order, merge, limit, levels, canonical codes.  lengths[n], codes[n] (may be null); scratch as lengths_from_order
// plus order[n], next_code[16].  The counts are left as they came.
PC_DF_HD inline void build_code(uint32_t *counts, uint32_t n, uint32_t limit, uint16_t *order, uint32_t *weight, uint16_t *parent, uint16_t *depth,
                                uint32_t *bl_count, uint32_t *next_code, uint8_t *lengths, uint32_t *codes) {
    uint32_t used = 0u, padded[2];
    for (uint32_t s = 0u; s < n; ++s) { used += counts[s] ? 1u : 0u; lengths[s] = 0u; }
    const uint32_t m = pad_counts(counts, n, used, padded);
    for (uint32_t s = 0u; s < n; ++s)
        if (counts[s]) order[rank_of(counts, n, s)] = (uint16_t)s;
    lengths_from_order(counts, order, m, limit, weight, parent, depth, bl_count, lengths);
    unpad_counts(counts, n, padded);
    first_codes(bl_count, next_code);
    if (codes)
        for (uint32_t s = 0u; s < n; ++s) codes[s] = canonical_code(lengths, next_code, s);
}

// The run-length code of the `total` code lengths seq(0 .. total - 1): emit(symbol, extra bits, their count) per symbol.
template <class Seq, class Emit>
PC_DF_HD inline void scan_lengths(Seq seq, uint32_t total, Emit emit) {
    uint32_t prevlen = 0xffffu, nextlen = seq(0u), count = 0u;
    uint32_t max_count = nextlen ? 7u : 138u, min_count = nextlen ? 4u : 3u;
    for (uint32_t i = 0u; i < total; ++i) {
        const uint32_t curlen = nextlen;
        nextlen = i + 1u < total ? seq(i + 1u) : 0xffffu;
        if (++count < max_count && curlen == nextlen) continue;
        if (count < min_count) { for (uint32_t k = 0u; k < count; ++k) emit(curlen, 0u, 0u); }
        else if (curlen != 0u) {
            if (curlen != prevlen) { emit(curlen, 0u, 0u); --count; }
            emit(16u, count - 3u, 2u);
        }
        else if (count <= 10u) emit(17u, count - 3u, 3u);
        else emit(18u, count - 11u, 7u);
        count = 0u; prevlen = curlen;
        if (nextlen == 0u) { max_count = 138u; min_count = 3u; }
        else if (curlen == nextlen) { max_count = 6u; min_count = 3u; }
        else { max_count = 7u; min_count = 4u; }
    }
}

// What the header of a dynamic block says beside the two length tables.
struct DynHeader { uint32_t hlit, hdist, hclen, bits; };   // bits: the 14 + 3 HCLEN + the coded lengths (not BFINAL, BTYPE)

// From the two length tables: HLIT, HDIST, the code-length code (cl_lengths[19], cl_codes[19]), HCLEN and the header's bits.
// Scratch: cl_counts[19] and the scratch of build_code for 19 symbols.
PC_DF_HD inline DynHeader plan_header(const uint8_t *lit_lengths, const uint8_t *dist_lengths, uint32_t *cl_counts, uint16_t *order, uint32_t *weight,
                                      uint16_t *parent, uint16_t *depth, uint32_t *bl_count, uint32_t *next_code, uint8_t *cl_lengths, uint32_t *cl_codes) {
    DynHeader h;
    h.hlit = kLitSyms; h.hdist = kDistSyms; h.hclen = kClSyms;
    while (h.hlit > 257u && !lit_lengths[h.hlit - 1u]) --h.hlit;
    while (h.hdist > 1u && !dist_lengths[h.hdist - 1u]) --h.hdist;
    for (uint32_t s = 0u; s < kClSyms; ++s) cl_counts[s] = 0u;
    uint32_t extra = 0u;
    const uint32_t hlit = h.hlit;
    scan_lengths([&](uint32_t i) -> uint32_t { return i < hlit ? lit_lengths[i] : dist_lengths[i - hlit]; }, h.hlit + h.hdist,
                 [&](uint32_t sym, uint32_t, uint32_t nextra) { ++cl_counts[sym]; extra += nextra; });
    build_code(cl_counts, kClSyms, kClLimit, order, weight, parent, depth, bl_count, next_code, cl_lengths, cl_codes);
    while (h.hclen > 4u && !cl_lengths[cl_order(h.hclen - 1u)]) --h.hclen;
    h.bits = 14u + 3u * h.hclen + extra;
    for (uint32_t s = 0u; s < kClSyms; ++s) h.bits += cl_counts[s] * cl_lengths[s];
    return h;
}

// The header's bits in stream order through put(value, count): HLIT, HDIST, HCLEN, the code-length code lengths, the lengths.
template <class Put>
PC_DF_HD inline void emit_header(const DynHeader &h, const uint8_t *lit_lengths, const uint8_t *dist_lengths, const uint8_t *cl_lengths, const uint32_t *cl_codes,
                                 Put put) {
    put(h.hlit - 257u, 5u); put(h.hdist - 1u, 5u); put(h.hclen - 4u, 4u);
    for (uint32_t i = 0u; i < h.hclen; ++i) put((uint32_t)cl_lengths[cl_order(i)], 3u);
    const uint32_t hlit = h.hlit;
    scan_lengths([&](uint32_t i) -> uint32_t { return i < hlit ? lit_lengths[i] : dist_lengths[i - hlit]; }, h.hlit + h.hdist,
                 [&](uint32_t sym, uint32_t ex, uint32_t nextra) {
                     const uint32_t c = cl_codes[sym];
                     put((c & 0xffffu) | (ex << (c >> 16)), (c >> 16) + nextra);
                 });
}

// bits a symbol adds under the dynamic and under the fixed code, extra bits included, for `count` occurrences
PC_DF_HD inline void add_literal_bits(uint32_t s, uint32_t count, uint32_t length, uint32_t &dynamic_bits, uint32_t &fixed_bits) {
    dynamic_bits += count * (length + length_extra_bits(s)); fixed_bits += count * (fixed_length(s) + length_extra_bits(s));
}
PC_DF_HD inline void add_distance_bits(uint32_t c, uint32_t count, uint32_t length, uint32_t &dynamic_bits, uint32_t &fixed_bits) {
    dynamic_bits += count * (length + distance_extra_bits(c)); fixed_bits += count * (5u + distance_extra_bits(c));
}

// The block a dynamic-mode stream takes, from the bits of the two coded bodies (BFINAL and BTYPE included).
PC_DF_HD inline uint32_t choose_block(uint64_t dynamic_bits, uint64_t fixed_bits, uint32_t n) {
    if ((dynamic_bits + 7u) / 8u < (fixed_bits + 7u) / 8u && takes_fixed(dynamic_bits, n)) return kDynamic;
    return takes_fixed(fixed_bits, n) ? kFixed : kStored;
}

// a token under the dynamic tables, in two parts of at most 20 and 28 bits: the length symbol with its extra bits (or the
// literal), then the distance code with its extra bits (n = 0 for a literal)
PC_DF_HD inline Bits dynamic_literal_bits(const uint32_t *lit_codes, uint32_t byte) { return Bits{lit_codes[byte] & 0xffffu, lit_codes[byte] >> 16}; }
PC_DF_HD inline void dynamic_match_bits(const uint32_t *lit_codes, const uint32_t *dist_codes, uint32_t len, uint32_t dist, Bits &first, Bits &second) {
    uint32_t ls, le, ln, dc, de, dn;
    length_code(len, ls, le, ln);
    distance_code(dist, dc, de, dn);
    const uint32_t lc = lit_codes[ls], dcode = dist_codes[dc];
    first = Bits{(lc & 0xffffu) | (le << (lc >> 16)), (lc >> 16) + ln};
    second = Bits{(dcode & 0xffffu) | (de << (dcode >> 16)), (dcode >> 16) + dn};
}

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

// The model encoder: the zlib stream of raw[0, n), n <= kMaxInput, in `mode` (kFixed, kDynamic) appended to `out`.
// *btype (when given): the block the body is (kStored, kFixed, kDynamic).
inline void encode(const uint8_t *raw, uint32_t n, std::vector<uint8_t> &out, uint32_t mode, uint32_t *btype = nullptr) {
    std::vector<uint16_t> len, dist;
    find_matches(raw, n, len, dist);
    uint32_t type = kFixed;
    uint64_t fixed_total = 0, dynamic_total = 0;
    std::vector<uint32_t> lit_counts(kLitSyms, 0u), dist_counts(kDistSyms, 0u), lit_codes(kLitSyms, 0u), dist_codes(kDistSyms, 0u);
    std::vector<uint8_t> lit_lengths(kLitSyms, 0u), dist_lengths(kDistSyms, 0u);
    uint8_t cl_lengths[kClSyms];
    uint32_t cl_codes[kClSyms], cl_counts[kClSyms];
    DynHeader hdr{};
    if (mode == kDynamic) {
        for (uint32_t p = 0; p < n;) {
            if (len[p]) {
                uint32_t ls, le, ln, dc, de, dn;
                length_code(len[p], ls, le, ln);
                distance_code(dist[p], dc, de, dn);
                ++lit_counts[ls]; ++dist_counts[dc];
                p += len[p];
            } else ++lit_counts[raw[p++]];
        }
        ++lit_counts[kEndOfBlock];
        uint16_t order[kLitSyms], parent[2u * kLitSyms], depth[kLitSyms];
        uint32_t weight[kLitSyms], bl_count[16], next_code[16];
        build_code(lit_counts.data(), kLitSyms, kLitLimit, order, weight, parent, depth, bl_count, next_code, lit_lengths.data(), lit_codes.data());
        build_code(dist_counts.data(), kDistSyms, kDistLimit, order, weight, parent, depth, bl_count, next_code, dist_lengths.data(), dist_codes.data());
        hdr = plan_header(lit_lengths.data(), dist_lengths.data(), cl_counts, order, weight, parent, depth, bl_count, next_code, cl_lengths, cl_codes);
        uint32_t db = 0u, fb = 0u;
        for (uint32_t s = 0; s < kLitSyms; ++s) add_literal_bits(s, lit_counts[s], lit_lengths[s], db, fb);
        for (uint32_t c = 0; c < kDistSyms; ++c) add_distance_bits(c, dist_counts[c], dist_lengths[c], db, fb);
        dynamic_total = 3ull + hdr.bits + db; fixed_total = 3ull + fb;
        type = choose_block(dynamic_total, fixed_total, n);
    }
    std::vector<uint8_t> body;
    uint64_t acc = 0;
    uint32_t nacc = 0;
    uint64_t total = 0;
    auto put = [&](Bits b) {
        acc |= (uint64_t)b.value << nacc; nacc += b.n; total += b.n;
        while (nacc >= 8u) { body.push_back((uint8_t)acc); acc >>= 8; nacc -= 8u; }
    };
    if (type == kDynamic) {
        put(Bits{5u, 3u});   // BFINAL = 1, BTYPE = 10
        emit_header(hdr, lit_lengths.data(), dist_lengths.data(), cl_lengths, cl_codes, [&](uint32_t value, uint32_t count) { put(Bits{value, count}); });
        for (uint32_t p = 0; p < n;) {
            if (len[p]) {
                Bits a, b;
                dynamic_match_bits(lit_codes.data(), dist_codes.data(), len[p], dist[p], a, b);
                put(a); put(b);
                p += len[p];
            } else put(dynamic_literal_bits(lit_codes.data(), raw[p++]));
        }
        put(dynamic_literal_bits(lit_codes.data(), kEndOfBlock));
    } else if (mode != kDynamic || type == kFixed) {
        put(Bits{3u, 3u});   // BFINAL = 1, BTYPE = 01
        for (uint32_t p = 0; p < n;) {
            if (len[p]) { put(match_bits(len[p], dist[p])); p += len[p]; }
            else { put(literal_bits(raw[p])); ++p; }
        }
        put(end_of_block_bits());
        if (mode != kDynamic) type = takes_fixed(total, n) ? kFixed : kStored;
    }
    if (nacc) body.push_back((uint8_t)acc);
    if (btype) *btype = type;
    out.push_back(kCmf); out.push_back(kFlg);
    if (type != kStored) out.insert(out.end(), body.begin(), body.end());
    else {
        out.push_back(1u);   // BFINAL = 1, BTYPE = 00
        out.push_back((uint8_t)(n & 255u)); out.push_back((uint8_t)(n >> 8));
        out.push_back((uint8_t)(~n & 255u)); out.push_back((uint8_t)((~n >> 8) & 255u));
        out.insert(out.end(), raw, raw + n);
    }
    const uint32_t ad = adler32(raw, n);
    out.push_back((uint8_t)(ad >> 24)); out.push_back((uint8_t)(ad >> 16)); out.push_back((uint8_t)(ad >> 8)); out.push_back((uint8_t)ad);
}

// the fixed mode, as before dynamic codes were built.  *stored (when given): the body is the stored block.
inline void encode(const uint8_t *raw, uint32_t n, std::vector<uint8_t> &out, bool *stored = nullptr) {
    uint32_t type = kFixed;
    encode(raw, n, out, kFixed, &type);
    if (stored) *stored = type == kStored;
}

}   // namespace pcdeflate
