// SAM text on the GPU: the kernels in front of and behind the shared record placement of bam_decoder.hip.h.  The body of
// the file (everything behind the '@' header lines) lies in HBM as it is on disk.  Line starts: the '\n' bytes of every
// fixed tile are counted, an exclusive sum over the tiles gives each tile's first line number, and a second pass writes
// the 64-bit start of every line.  k_sam_fields: one lane per line runs sam_parse_line of sam_host.h -- the source the host
// reader runs -- and leaves a pcbam::RecOut with the meanings k_bam_fields gives it.  k_sam_columns is k_bam_columns with the
// CIGAR walked again as text.  Every byte access lies in [0, body_len); each step is one launch.
// Part of the one translation unit of plastid_counts.hip (behind bam_kernels.hip.h: RecOut).
#pragma once
#include "sam_host.h"

namespace pcsam {

constexpr int kSamTile = 4096;                  // bytes of the body per workgroup of the two line-start kernels
constexpr int kSamTileThreads = 256;
constexpr int kSamBytesPerThread = kSamTile / kSamTileThreads;

// '\n' bytes of every tile
__global__ __launch_bounds__(kSamTileThreads) void k_sam_count_lines(const uint8_t *__restrict__ body, uint64_t body_len, uint32_t *__restrict__ tile_lines) {
    const uint64_t at = (uint64_t)blockIdx.x * kSamTile + (uint64_t)threadIdx.x * kSamBytesPerThread;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < kSamBytesPerThread; ++k)
        if (at + k < body_len) c += body[at + k] == (uint8_t)'\n' ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    __shared__ uint32_t s_c[kSamTileThreads / 64];
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_lines[blockIdx.x] = s_c[0] + s_c[1] + s_c[2] + s_c[3];
}

// line_start[k + 1] = the byte behind the k-th '\n' of the body (line_start[0] = 0 is the host's); tile_first[t]: '\n'
// bytes in front of tile t.  `cap`: entries of line_start.
__global__ __launch_bounds__(kSamTileThreads) void k_sam_line_starts(const uint8_t *__restrict__ body, uint64_t body_len, const uint32_t *__restrict__ tile_first,
                                                                     uint64_t *__restrict__ line_start, uint64_t cap) {
    const uint64_t at = (uint64_t)blockIdx.x * kSamTile + (uint64_t)threadIdx.x * kSamBytesPerThread;
    uint32_t mask = 0;
#pragma unroll
    for (int k = 0; k < kSamBytesPerThread; ++k)
        if (at + k < body_len && body[at + k] == (uint8_t)'\n') mask |= 1u << k;
    const uint32_t mine = (uint32_t)__popc(mask);
    // exclusive sum of `mine` over the workgroup: within the wave by shuffles, across the four waves through LDS
    uint32_t incl = mine;
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    __shared__ uint32_t s_w[kSamTileThreads / 64];
    if (lane == 63) s_w[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t before = incl - mine;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) before += s_w[w];
    uint64_t line = (uint64_t)tile_first[blockIdx.x] + before + 1;
    while (mask) {
        const int k = __ffs(mask) - 1;
        mask &= mask - 1u;
        if (line < cap) line_start[line] = at + (uint64_t)k + 1;
        ++line;
    }
}

// One lane per line: line i is [line_start[i], line_start[i + 1] - 1) (the table has one entry behind the last line).
__global__ __launch_bounds__(256) void k_sam_fields(const uint8_t *__restrict__ body, uint64_t body_len, const uint64_t *__restrict__ line_start, int64_t nrec,
                                                    SamRefs refs, pcbam::RecOut *recs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrec) return;
    uint64_t b = line_start[i], e = line_start[i + 1] - 1;
    if (e > body_len) e = body_len;
    if (b > e) b = e;
    SamRec r;
    sam_parse_line(body + b, body + e, refs, r);
    pcbam::RecOut o;
    o.tid = r.tid; o.spos = r.spos; o.pos = r.pos; o.L = r.L; o.nruns = r.nruns; o.flag = r.flag; o.err = r.err; o.placed = r.placed;
    o.lseq = r.lseq; o.mapq = r.mapq; o.end = r.end;
    recs[i] = o;
}

// the runs of a multi-run record, written from `at` on (never more than `room` of them)
struct RunWriter {
    int32_t *blk_start, *blk_len;
    int64_t at, room;
    int64_t *k;                                 // runs begun so far
    PC_SAM_HD void operator()(int64_t ref, uint32_t len, bool new_run) const {
        if (new_run) {
            *k += 1;
            if (*k <= room) { blk_start[at + *k - 1] = (int32_t)ref; blk_len[at + *k - 1] = 0; }
        }
        if (*k >= 1 && *k <= room) blk_len[at + *k - 1] += (int32_t)len;
    }
};

// columns of the staged (placed) lines at their scanned indices; runs of the multi-run ones at theirs (k_bam_columns for text)
__global__ __launch_bounds__(256) void k_sam_columns(const uint8_t *__restrict__ body, uint64_t body_len, const uint64_t *__restrict__ line_start,
                                                     const pcbam::RecOut *__restrict__ recs, int64_t nrec,
                                                     const uint32_t *__restrict__ staged_at, const uint32_t *__restrict__ run_at,
                                                     int32_t *tid, int32_t *pos, uint16_t *alen, uint8_t *flags, uint8_t *nblk,
                                                     int32_t *blk_start, int32_t *blk_len, uint32_t *wide_flag,
                                                     uint16_t *flag16, uint8_t *mapq, int32_t *lseq, uint16_t *nh) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrec) return;
    const pcbam::RecOut o = recs[i];
    if (o.placed != 1) return;
    const uint32_t k = staged_at[i];
    const bool wide = o.L > 65535u || o.nruns > 255u || (o.L == 65535u && o.nruns == 255u);
    tid[k] = o.tid;
    pos[k] = o.spos;
    alen[k] = wide ? (uint16_t)65535 : (uint16_t)o.L;
    flags[k] = (o.flag & 0x10) ? 1 : 0;
    nblk[k] = wide ? (uint8_t)255 : (uint8_t)o.nruns;
    flag16[k] = o.flag;
    mapq[k] = (uint8_t)o.mapq;
    nh[k] = (uint16_t)(o.mapq >> 16);
    lseq[k] = o.lseq;
    if (wide) wide_flag[k] = 1u;
    if (o.nruns < 2u) return;
    uint64_t b = line_start[i], e = line_start[i + 1] - 1;
    if (e > body_len) e = body_len;
    if (b > e) b = e;
    const uint8_t *le = body + e;
    if (le > body + b && le[-1] == (uint8_t)'\r') --le;
    const uint8_t *cb, *ce;
    sam_cigar_field(body + b, le, cb, ce);
    int64_t begun = 0;
    RunWriter w{blk_start, blk_len, (int64_t)run_at[i], (int64_t)o.nruns, &begun};
    (void)sam_walk_cigar(cb, ce, (int64_t)o.pos, w);
}

} // namespace pcsam
