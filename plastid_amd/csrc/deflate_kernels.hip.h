// deflate_kernels.hip.h -- the zlib ENCODER on the GPU (revision 19), the mirror image of k_zlib_inflate.
//   k_zlib_deflate    ONE WORKGROUP of 256 lanes PER INPUT of at most pcdeflate::kMaxInput bytes -> one RFC 1950 stream in
//                     the input's slot of len + 16 bytes, its size and whether it fell back to the stored block.  The
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
//   k_deflate_compact one workgroup per stream: slot -> its place in the contiguous output (the exclusive sum of the sizes).
// LDS: 24 616 (input) + 24 608 (lengths) + 49 200 (distances) + 49 200 (head table and chunk hashes, then the exits, then
// the output words) + 4 KiB of per-lane words = 151 720 of the 163 840 bytes of a CU: one workgroup per CU.
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

namespace pcdeflate {

constexpr int kDefWG = 256;
constexpr uint32_t kNone = 0xffffffffu;

__device__ inline uint32_t token_step(uint32_t len8) { return len8 ? len8 + 3u : 1u; }

__global__ __launch_bounds__(kDefWG) void k_zlib_deflate(const uint8_t *__restrict__ image, const int64_t *__restrict__ off, const int64_t *__restrict__ len,
                                                         const uint64_t *__restrict__ slot_off, int64_t nstreams, uint8_t *__restrict__ slots,
                                                         unsigned long long *__restrict__ out_len, uint32_t *__restrict__ stored) {
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

    // ---- code: bits of the segment's tokens, their exclusive sum, the fixed-or-stored decision
    const uint32_t entry = s_entry[tid];
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
        stored[k] = fixed ? 0u : 1u;
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

}   // namespace pcdeflate
