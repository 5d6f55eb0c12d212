// deflate_kernels.hip.h -- the zlib ENCODER on the GPU (revision 20), the mirror image of k_zlib_inflate.
//   k_zlib_deflate    ONE WORKGROUP of 256 lanes PER INPUT of at most pcdeflate::kMaxInput bytes -> one RFC 1950 stream in
//                     the input's slot of len + 16 bytes, its size and how far its block fell back (0: the mode's own
//                     codes, 1: dynamic -> fixed or fixed -> stored, 2: dynamic -> stored: BTYPE = mode - steps).  A
//                     template on the mode (kFixed, kDynamic); the fixed instantiation is the kernel as it was.  The
//                     bytes are those of pcdeflate::encode (deflate_host.h states the rule), whatever the lane timing:
//       match     the input in LDS; positions in ORDERED CHUNKS of 256.  A lane's candidate is the nearest earlier
//                 position of equal hash: inside the chunk found by walking the chunk's hashes backwards, in front of it
//                 read from the head table, which a chunk updates (atomicMax of position + 1: max commutes) only after
//                 every lane has read it.  The lane verifies and extends its match byte by byte;
//       parse     the greedy chain from position 0 over next(p) = p + max(1, len(p)): every lane resolves the chain
//                 inside its own segment of ceil(n / 256) positions backwards (exit(p): where the chain from p leaves the
//                 segment), lane 0 hops the 256 segments, then every lane knows where the chain enters its segment;
//       code      a lane adds the bits of its segment's tokens, the exclusive sum over the lanes gives every lane its
//                 bit offset, and the bits are merged into zeroed LDS words with atomic OR (OR commutes);
//       trailer   Adler-32 per segment, combined in order (adler_combine of bigwig_host.h, as k_zlib_adler).
//                     The dynamic instantiation goes its own way between parse and code:
//       histogram every lane walks its segment's tokens and adds to LDS counters (atomic add: add commutes);
//       order     a rank sort on (count, symbol): a lane per symbol counts the keys below its own (rank_of);
//       trees     lengths_from_order of deflate_host.h on lane 0 (literal/length) and lane 64 (distance); the canonical
//                 codes a lane per symbol; the code-length code and the header's size on lane 0 (plan_header);
//       choice    the bits of both bodies from the histograms, a lane per symbol; choose_block;
//       code      as above under the chosen tables; lane 0 writes the header's bits in front, lane 64 the end of block.
//                 The trees' scratch lies in the dead exits; histograms, lengths and code tables take 3 KiB of their own.
//   k_huffman_lengths one workgroup: the order step and build_code's length function for a caller's counts (the seam
//                     pc_huffman_lengths, through which the length limit is tested on the device).
//   k_deflate_compact one workgroup per stream: slot -> its place in the contiguous output (the exclusive sum of the sizes).
// LDS: 24 616 (input) + 24 608 (lengths) + 49 200 (distances) + 49 200 (head table and chunk hashes, then the exits, then
// the output words) + 4 KiB of per-lane words = 151 720 of the 163 840 bytes of a CU: one workgroup per CU.  The dynamic
// instantiation: 3 024 bytes more (154 752).
// No input makes the kernel touch memory outside [off, off + len) of the image and the stream's slot.
// Part of the one translation unit of plastid_counts.hip.
#pragma once
#include "bigwig_host.h"
#include "deflate_host.h"

// Section builds for experiments only (never the product library; the streams are still valid, but no longer the model's):
// PC_DEFLATE_SKIP bit 0 leaves out the walk over the chunk's hashes (candidates come from the head table alone), bit 1 the
// verification and extension of matches (every byte is a literal).  profiles/track_text/NOTES.md has the laps.
#ifndef PC_DEFLATE_SKIP
#define PC_DEFLATE_SKIP 0
#endif
// PC_DEFLATE_DYN_SKIP, for the dynamic instantiation alone (these streams are NOT valid: only the laps are read): bit 0 leaves
// out merge, depths, limit and levels (every used symbol gets 9 or 5 bits), bit 1 the code-length code and the header
// (planned and written), bit 2 the rank sort and the canonical codes (with bit 0).
#ifndef PC_DEFLATE_DYN_SKIP
#define PC_DEFLATE_DYN_SKIP 0
#endif

namespace pcdeflate {

constexpr int kDefWG = 256;
constexpr uint32_t kNone = 0xffffffffu;

__device__ inline uint32_t token_step(uint32_t len8) { return len8 ? len8 + 3u : 1u; }

// (PC_DEFLATE_DYN_SKIP bit 0) every used symbol takes `length` bits
__device__ inline void flat_lengths(const uint32_t *counts, uint32_t n, uint32_t length, uint32_t *bl_count, uint8_t *lengths) {
    uint32_t used = 0u;
    for (uint32_t s = 0u; s < n; ++s)
        if (counts[s]) { lengths[s] = (uint8_t)length; ++used; }
    for (uint32_t b = 0u; b < 16u; ++b) bl_count[b] = b == length ? used : 0u;
}

// bits into the zeroed words at bit offset o (count <= 32)
__device__ inline void or_bits(uint32_t *words, uint32_t o, uint32_t value, uint32_t count) {
    if (!count) return;
    const uint64_t v = (uint64_t)value << (o & 31u);
    atomicOr(&words[o >> 5], (uint32_t)v);
    if ((uint32_t)(v >> 32)) atomicOr(&words[(o >> 5) + 1u], (uint32_t)(v >> 32));
}

// the places of the trees' scratch in s_u (uint32 units): per alphabet order | parent | depth | weight | bl_count | next_code
struct TreeScratch {
    uint16_t *order, *parent, *depth;
    uint32_t *weight, *bl_count, *next_code;
    __device__ TreeScratch(uint32_t *base, uint32_t n) {   // n even
        order = (uint16_t *)base; parent = order + n; depth = parent + 2u * n;
        weight = base + 2u * n; bl_count = weight + n; next_code = bl_count + 16u;
    }
    static constexpr uint32_t words(uint32_t n) { return 3u * n + 32u; }
};

template <uint32_t MODE>
__global__ __launch_bounds__(kDefWG) void k_zlib_deflate(const uint8_t *__restrict__ image, const int64_t *__restrict__ off, const int64_t *__restrict__ len,
                                                         const uint64_t *__restrict__ slot_off, int64_t nstreams, uint8_t *__restrict__ slots,
                                                         unsigned long long *__restrict__ out_len, uint32_t *__restrict__ fell_back) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[kMaxInput + 16u];
    __shared__ __attribute__((aligned(16))) uint8_t s_len[kMaxInput + 8u];      // match length - 3 (1 .. 255), 0: a literal
    __shared__ __attribute__((aligned(16))) uint16_t s_dist[kMaxInput];
    __shared__ __attribute__((aligned(16))) uint32_t s_u[kMaxInput / 2u];       // head + hashes | exits (u16) | output words
    __shared__ uint32_t s_entry[kDefWG], s_bits[kDefWG], s_a[kDefWG], s_b[kDefWG];
    __shared__ uint32_t s_adler;
    const int64_t k = (int64_t)blockIdx.x;
    if (k >= nstreams) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t n = (uint32_t)len[k];           // (the host refuses a longer input than kMaxInput)
    const uint8_t *src = image + off[k];
    uint8_t *dst = slots + slot_off[k];
    uint32_t *head = s_u, *hs = s_u + (1u << kHashBits);
    uint16_t *s_exit = (uint16_t *)s_u;

    for (uint32_t i = tid; i < n; i += kDefWG) s_in[i] = src[i];
    for (uint32_t i = tid; i < (1u << kHashBits); i += kDefWG) head[i] = 0u;
    __syncthreads();

    // ---- match: ordered chunks
    for (uint32_t c0 = 0; c0 < n; c0 += kDefWG) {
        const uint32_t p = c0 + tid;
        const bool valid = p + 4u <= n;
        uint32_t h = kNone, prev = 0u;             // prev: the candidate + 1
        if (valid) {
            h = hash4(s_in[p], s_in[p + 1], s_in[p + 2], s_in[p + 3]);
            prev = head[h];
        }
        hs[tid] = h;
        __syncthreads();
        if (valid && !(PC_DEFLATE_SKIP & 1))
            for (int j = (int)tid - 1; j >= 0; --j)
                if (hs[j] == h) { prev = c0 + (uint32_t)j + 1u; break; }
        __syncthreads();
        if (valid) atomicMax(&head[h], p + 1u);
        if (p < n) {
            const uint32_t l = (prev && !(PC_DEFLATE_SKIP & 2)) ? match_length(s_in, n, prev - 1u, p) : 0u;
            s_len[p] = l ? (uint8_t)(l - 3u) : (uint8_t)0;
            s_dist[p] = l ? (uint16_t)(p - (prev - 1u)) : (uint16_t)0;
        }
        __syncthreads();
    }

    // ---- parse: the chain inside every segment, backwards; then across the segments
    const uint32_t seg = n ? (n + kDefWG - 1u) / kDefWG : 1u;
    const uint32_t lo = tid * seg < n ? tid * seg : n, hi = lo + seg < n ? lo + seg : n;
    for (uint32_t p = hi; p > lo;) {
        --p;
        const uint32_t nx = p + token_step(s_len[p]);
        s_exit[p] = (uint16_t)(nx >= hi ? nx : s_exit[nx]);
    }
    {   // Adler-32 of the segment (at most 97 bytes: no sum overflows)
        uint32_t a = 1u, b = 0u;
        for (uint32_t p = lo; p < hi; ++p) { a += s_in[p]; b += a; }
        s_a[tid] = a % kAdlerMod; s_b[tid] = b % kAdlerMod;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t e = 0u;
        for (uint32_t s = 0; s < (uint32_t)kDefWG; ++s) {
            const uint32_t slo = s * seg < n ? s * seg : n, shi = slo + seg < n ? slo + seg : n;
            if (e >= slo && e < shi) { s_entry[s] = e; e = s_exit[e]; }
            else s_entry[s] = kNone;
        }
    }
    if (tid == 64) {   // (another wave than the chain's)
        uint32_t ca = 1u, cb = 0u;
        for (uint32_t s = 0; s < (uint32_t)kDefWG; ++s) {
            const uint32_t slo = s * seg < n ? s * seg : n, shi = slo + seg < n ? slo + seg : n;
            pcbw::adler_combine(ca, cb, s_a[s], s_b[s], (uint64_t)(shi - slo));
        }
        s_adler = (cb << 16) | ca;
    }
    __syncthreads();

    const uint32_t entry = s_entry[tid];
    if constexpr (MODE == kDynamic) {
        __shared__ uint32_t s_lcnt[kLitSyms + 2u], s_dcnt[kDistSyms + 2u], s_lcode[kLitSyms + 2u], s_dcode[kDistSyms + 2u], s_ccode[kClSyms + 1u];
        __shared__ uint8_t s_llen[kLitSyms + 2u], s_dlen[kDistSyms + 2u], s_clen[kClSyms + 1u];
        __shared__ uint32_t s_used[2], s_pad[4], s_tot[2];
        __shared__ DynHeader s_hdr;
        const TreeScratch tl(s_u, kLitSyms + 2u), td(s_u + TreeScratch::words(kLitSyms + 2u), kDistSyms + 2u),
            tc(s_u + TreeScratch::words(kLitSyms + 2u) + TreeScratch::words(kDistSyms + 2u), kClSyms + 1u);
        uint32_t *cl_counts = s_u + TreeScratch::words(kLitSyms + 2u) + TreeScratch::words(kDistSyms + 2u) + TreeScratch::words(kClSyms + 1u);
        // ---- histogram (the exits are read: s_u is free until the output words)
        for (uint32_t s = tid; s < kLitSyms; s += kDefWG) { s_lcnt[s] = 0u; s_llen[s] = 0u; }
        if (tid < kDistSyms) { s_dcnt[tid] = 0u; s_dlen[tid] = 0u; }
        if (tid < 2u) { s_used[tid] = 0u; s_tot[tid] = 0u; }
        __syncthreads();
        if (entry != kNone)
            for (uint32_t p = entry; p < hi;) {
                const uint32_t l8 = s_len[p];
                if (l8) {
                    uint32_t ls, le, ln, dc, de, dn;
                    length_code(l8 + 3u, ls, le, ln);
                    distance_code(s_dist[p], dc, de, dn);
                    atomicAdd(&s_lcnt[ls], 1u); atomicAdd(&s_dcnt[dc], 1u);
                } else atomicAdd(&s_lcnt[s_in[p]], 1u);
                p += token_step(l8);
            }
        if (tid == 0) atomicAdd(&s_lcnt[kEndOfBlock], 1u);
        __syncthreads();
        // ---- padding and order
        for (uint32_t s = tid; s < kLitSyms; s += kDefWG)
            if (s_lcnt[s]) atomicAdd(&s_used[0], 1u);
        if (tid < kDistSyms && s_dcnt[tid]) atomicAdd(&s_used[1], 1u);
        __syncthreads();
        if (tid == 0) s_used[0] = pad_counts(s_lcnt, kLitSyms, s_used[0], s_pad);
        if (tid == 64) s_used[1] = pad_counts(s_dcnt, kDistSyms, s_used[1], s_pad + 2);
        __syncthreads();
        if (!(PC_DEFLATE_DYN_SKIP & 4)) {
            for (uint32_t s = tid; s < kLitSyms; s += kDefWG)
                if (s_lcnt[s]) tl.order[rank_of(s_lcnt, kLitSyms, s)] = (uint16_t)s;
            if (tid >= 64u && tid < 64u + kDistSyms && s_dcnt[tid - 64u]) td.order[rank_of(s_dcnt, kDistSyms, tid - 64u)] = (uint16_t)(tid - 64u);
        }
        __syncthreads();
        // ---- merge, limit, levels: one lane per tree, on two waves
        if (tid == 0) {
            if (PC_DEFLATE_DYN_SKIP & 1) flat_lengths(s_lcnt, kLitSyms, 9u, tl.bl_count, s_llen);
            else lengths_from_order(s_lcnt, tl.order, s_used[0], kLitLimit, tl.weight, tl.parent, tl.depth, tl.bl_count, s_llen);
            unpad_counts(s_lcnt, kLitSyms, s_pad);
            first_codes(tl.bl_count, tl.next_code);
        }
        if (tid == 64) {
            if (PC_DEFLATE_DYN_SKIP & 1) flat_lengths(s_dcnt, kDistSyms, 5u, td.bl_count, s_dlen);
            else lengths_from_order(s_dcnt, td.order, s_used[1], kDistLimit, td.weight, td.parent, td.depth, td.bl_count, s_dlen);
            unpad_counts(s_dcnt, kDistSyms, s_pad + 2);
            first_codes(td.bl_count, td.next_code);
        }
        __syncthreads();
        // ---- canonical codes and the bits of both bodies, a lane per symbol; the code-length code on lane 0
        {
            uint32_t db = 0u, fb = 0u;
            for (uint32_t s = tid; s < kLitSyms; s += kDefWG) {
                s_lcode[s] = (PC_DEFLATE_DYN_SKIP & 4) ? (s_llen[s] ? s | (9u << 16) : 0u) : canonical_code(s_llen, tl.next_code, s);
                add_literal_bits(s, s_lcnt[s], s_llen[s], db, fb);
            }
            if (tid >= 64u && tid < 64u + kDistSyms) {
                const uint32_t c = tid - 64u;
                s_dcode[c] = (PC_DEFLATE_DYN_SKIP & 4) ? (s_dlen[c] ? c | (5u << 16) : 0u) : canonical_code(s_dlen, td.next_code, c);
                add_distance_bits(c, s_dcnt[c], s_dlen[c], db, fb);
            }
            if (db) atomicAdd(&s_tot[0], db);
            if (fb) atomicAdd(&s_tot[1], fb);
        }
        if (tid == 0)
            s_hdr = (PC_DEFLATE_DYN_SKIP & 2) ? DynHeader{kLitSyms, kDistSyms, kClSyms, 14u + 3u * kClSyms}
                                              : plan_header(s_llen, s_dlen, cl_counts, tc.order, tc.weight, tc.parent, tc.depth, tc.bl_count, tc.next_code, s_clen, s_ccode);
        __syncthreads();
        const DynHeader hdr = s_hdr;
        const uint32_t dynamic_bits = 3u + hdr.bits + s_tot[0], fixed_bits = 3u + s_tot[1];
        const uint32_t type = choose_block(dynamic_bits, fixed_bits, n);
        // ---- code: bits of the segment's tokens under the chosen tables, their exclusive sum
        uint32_t mine = 0u;
        if (entry != kNone && type != kStored)
            for (uint32_t p = entry; p < hi;) {
                const uint32_t l8 = s_len[p];
                if (type == kFixed) mine += l8 ? match_bits(l8 + 3u, s_dist[p]).n : literal_bits(s_in[p]).n;
                else if (l8) {
                    Bits a, b;
                    dynamic_match_bits(s_lcode, s_dcode, l8 + 3u, s_dist[p], a, b);
                    mine += a.n + b.n;
                } else mine += s_lcode[s_in[p]] >> 16;
                p += token_step(l8);
            }
        s_bits[tid] = mine;
        __syncthreads();
        uint32_t before = 0u;
        for (uint32_t s = 0; s < tid; ++s) before += s_bits[s];
        const uint32_t total_bits = type == kDynamic ? dynamic_bits : fixed_bits;
        const uint32_t body = type == kStored ? 5u + n : (total_bits + 7u) / 8u;
        const uint32_t adler = s_adler;
        if (tid == 0) {
            dst[0] = kCmf; dst[1] = kFlg;
            uint8_t *t = dst + 2u + body;
            t[0] = (uint8_t)(adler >> 24); t[1] = (uint8_t)(adler >> 16); t[2] = (uint8_t)(adler >> 8); t[3] = (uint8_t)adler;
            out_len[k] = (unsigned long long)(2u + body + 4u);
            fell_back[k] = kDynamic - type;
        }
        if (type == kStored) {   // (uniform) one stored block
            if (tid == 0) {
                dst[2] = 1u; dst[3] = (uint8_t)(n & 255u); dst[4] = (uint8_t)(n >> 8); dst[5] = (uint8_t)(~n & 255u); dst[6] = (uint8_t)((~n >> 8) & 255u);
            }
            for (uint32_t i = tid; i < n; i += kDefWG) dst[7u + i] = s_in[i];
            return;
        }
        // (the trees' scratch is read: its bytes become the output words; body < 5 + n bytes, and one word of room behind them)
        uint32_t *words = s_u;
        const uint32_t nwords = body / 4u + 2u;
        for (uint32_t i = tid; i < nwords; i += kDefWG) words[i] = 0u;
        __syncthreads();
        const uint32_t first = type == kDynamic ? 3u + hdr.bits : 3u;
        if (tid == 0) {
            atomicOr(&words[0], 1u | (type << 1));   // BFINAL = 1, BTYPE
            if (type == kDynamic && !(PC_DEFLATE_DYN_SKIP & 2)) {
                uint32_t o = 3u;
                emit_header(hdr, s_llen, s_dlen, s_clen, s_ccode, [&](uint32_t value, uint32_t count) { or_bits(words, o, value, count); o += count; });
            }
        }
        if (tid == 64 && type == kDynamic) or_bits(words, total_bits - (s_lcode[kEndOfBlock] >> 16), s_lcode[kEndOfBlock] & 0xffffu, s_lcode[kEndOfBlock] >> 16);
        if (entry != kNone) {
            uint32_t o = first + before;
            for (uint32_t p = entry; p < hi;) {
                const uint32_t l8 = s_len[p];
                if (type == kFixed) {
                    const Bits b = l8 ? match_bits(l8 + 3u, s_dist[p]) : literal_bits(s_in[p]);
                    or_bits(words, o, b.value, b.n);
                    o += b.n;
                } else if (l8) {
                    Bits a, b;
                    dynamic_match_bits(s_lcode, s_dcode, l8 + 3u, s_dist[p], a, b);
                    or_bits(words, o, a.value, a.n);
                    or_bits(words, o + a.n, b.value, b.n);
                    o += a.n + b.n;
                } else {
                    const uint32_t c = s_lcode[s_in[p]];
                    or_bits(words, o, c & 0xffffu, c >> 16);
                    o += c >> 16;
                }
                p += token_step(l8);
            }
        }
        __syncthreads();
        const uint8_t *wb = (const uint8_t *)words;
        for (uint32_t i = tid; i < body; i += kDefWG) dst[2u + i] = wb[i];
        return;
    }

    // ---- code: bits of the segment's tokens, their exclusive sum, the fixed-or-stored decision
    uint32_t mine = 0u;
    if (entry != kNone)
        for (uint32_t p = entry; p < hi;) {
            const uint32_t l8 = s_len[p];
            mine += l8 ? match_bits(l8 + 3u, s_dist[p]).n : literal_bits(s_in[p]).n;
            p += token_step(l8);
        }
    s_bits[tid] = mine;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
    for (uint32_t s = 0; s < (uint32_t)kDefWG; ++s) {
        const uint32_t v = s_bits[s];
        all += v;
        if (s < tid) before += v;
    }
    const uint32_t total_bits = 3u + all + 7u;
    const bool fixed = takes_fixed(total_bits, n);
    const uint32_t body = fixed ? (total_bits + 7u) / 8u : 5u + n;
    const uint32_t adler = s_adler;
    if (tid == 0) {
        dst[0] = kCmf; dst[1] = kFlg;
        uint8_t *t = dst + 2u + body;
        t[0] = (uint8_t)(adler >> 24); t[1] = (uint8_t)(adler >> 16); t[2] = (uint8_t)(adler >> 8); t[3] = (uint8_t)adler;
        out_len[k] = (unsigned long long)(2u + body + 4u);
        fell_back[k] = fixed ? 0u : 1u;
    }
    if (!fixed) {   // (uniform) one stored block
        if (tid == 0) {
            dst[2] = 1u; dst[3] = (uint8_t)(n & 255u); dst[4] = (uint8_t)(n >> 8); dst[5] = (uint8_t)(~n & 255u); dst[6] = (uint8_t)((~n >> 8) & 255u);
        }
        for (uint32_t i = tid; i < n; i += kDefWG) dst[7u + i] = s_in[i];
        return;
    }
    // (the exits are read: their bytes become the output words; body < 5 + n bytes, and one word of room behind them)
    uint32_t *words = s_u;
    const uint32_t nwords = body / 4u + 2u;
    for (uint32_t i = tid; i < nwords; i += kDefWG) words[i] = 0u;
    __syncthreads();
    if (tid == 0) atomicOr(&words[0], 3u);   // BFINAL = 1, BTYPE = 01; the end of block is seven zero bits
    if (entry != kNone) {
        uint32_t o = 3u + before;
        for (uint32_t p = entry; p < hi;) {
            const uint32_t l8 = s_len[p];
            const Bits b = l8 ? match_bits(l8 + 3u, s_dist[p]) : literal_bits(s_in[p]);
            const uint64_t v = (uint64_t)b.value << (o & 31u);
            atomicOr(&words[o >> 5], (uint32_t)v);
            if ((uint32_t)(v >> 32)) atomicOr(&words[(o >> 5) + 1u], (uint32_t)(v >> 32));
            o += b.n;
            p += token_step(l8);
        }
    }
    __syncthreads();
    const uint8_t *wb = (const uint8_t *)words;
    for (uint32_t i = tid; i < body; i += kDefWG) dst[2u + i] = wb[i];
}

// One workgroup per stream: the slot's bytes to their place in the contiguous output.
__global__ __launch_bounds__(256) void k_deflate_compact(const uint8_t *__restrict__ slots, const uint64_t *__restrict__ slot_off,
                                                         const unsigned long long *__restrict__ out_len, const unsigned long long *__restrict__ out_off,
                                                         int64_t nstreams, uint8_t *__restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x;
    if (k >= nstreams) return;
    const uint8_t *src = slots + slot_off[k];
    uint8_t *dst = out + out_off[k];
    const uint32_t n = (uint32_t)out_len[k];
    for (uint32_t i = threadIdx.x; i < n; i += 256u) dst[i] = src[i];
}

// One workgroup: the code lengths of n counts (2 .. 286) under `limit` (2^limit >= n), as pcdeflate::build_code gives them.
__global__ __launch_bounds__(kDefWG) void k_huffman_lengths(const uint32_t *__restrict__ counts, uint32_t n, uint32_t limit, uint8_t *__restrict__ lengths) {
    __shared__ uint32_t s_cnt[kLitSyms + 2u], s_scratch[TreeScratch::words(kLitSyms + 2u)], s_used, s_pad[2];
    __shared__ uint8_t s_lengths[kLitSyms + 2u];
    const uint32_t tid = threadIdx.x;
    const TreeScratch t(s_scratch, kLitSyms + 2u);
    if (tid == 0) s_used = 0u;
    for (uint32_t s = tid; s < n; s += kDefWG) { s_cnt[s] = counts[s]; s_lengths[s] = 0u; }
    __syncthreads();
    for (uint32_t s = tid; s < n; s += kDefWG)
        if (s_cnt[s]) atomicAdd(&s_used, 1u);
    __syncthreads();
    if (tid == 0) s_used = pad_counts(s_cnt, n, s_used, s_pad);
    __syncthreads();
    for (uint32_t s = tid; s < n; s += kDefWG)
        if (s_cnt[s]) t.order[rank_of(s_cnt, n, s)] = (uint16_t)s;
    __syncthreads();
    if (tid == 0) lengths_from_order(s_cnt, t.order, s_used, limit, t.weight, t.parent, t.depth, t.bl_count, s_lengths);
    __syncthreads();
    for (uint32_t s = tid; s < n; s += kDefWG) lengths[s] = s_lengths[s];
}

}   // namespace pcdeflate
