// bigwig_kernels.hip.h -- bigWig files on the GPU (revision 18).  The container is bigwig_host.h's (the host walks the
// header and the two trees: a few KiB); the data blocks -- independent zlib streams of a few KiB each, or stored sections --
// go to HBM as they are and
//   k_zlib_inflate    (bam_kernels.hip.h) the zlib instantiation of the BGZF inflate: ONE WAVE PER BLOCK into a slot of
//                     uncompressBufSize bytes (rounded to 16), the bytes produced into a per-block length;
//   k_zlib_adler      ONE WAVE PER BLOCK: Adler-32 of the produced bytes against the stream's trailer.  The block is cut
//                     into 64 contiguous slices, a lane each (16-byte loads; the sums reduced mod 65521 before 32 bits can
//                     overflow: every 5552 bytes at the latest, zlib's NMAX), combined in order by
//                     b(AB) = b(A) + b(B) + |B| (a(A) - 1);
//   k_bw_sections     one lane per block: the section header against the block's produced length (check_section of
//                     bigwig_host.h) -> the block's item count (0 with a defect) and the lowest defect;
//   item_at           (device function, shared with k_bbi_items of bigwig_summary_kernels.hip.h) an item's block by
//                     bisection over the exclusive sum of the counts, the item decoded and checked by the host reader's
//                     functions;
//   k_bw_items        one lane per item: item_at -> the line record (contig, start, stop, (double) float32) that
//                     k_track_keys and the kernels behind it consume;
//   k_track_gather_acc / k_track_scale   BigWigGenomeArray.get: out = out + cells, one launch per reader in reader order
//                     (every reader cuts its own items: its contigs and extents are its own), then v / sum * 1e6;
//   k_track_sum_tiles the fixed-tree sum over ranges of cells (BigWigReader.sum()).
// No input makes a kernel read outside its buffers: a block's bytes are read below its produced length only, and an item
// is decoded only when 24 + itemCount x itemsize IS that length.
// Part of the one translation unit of plastid_counts.hip (behind track_kernels.hip.h).
#pragma once
#include "bigwig_host.h"

namespace pcbw {

constexpr int kInfZlibHeader = 12;     // pc_inflate_zlib: the status of a stream whose header the host refuses

__global__ __launch_bounds__(64) void k_zlib_adler(const uint8_t *__restrict__ out, const pcbam::Member *__restrict__ members, int nmembers,
                                                   const uint32_t *__restrict__ produced, uint32_t *__restrict__ status) {
    __shared__ uint32_t pa[64], pb[64], pn[64];
    const int m = (int)blockIdx.x;
    if (m >= nmembers) return;
    if (status[m] != 0u) return;            // (uniform: the stream did not inflate)
    const pcbam::Member mb = members[m];
    const int lane = threadIdx.x & 63;
    const uint32_t len = produced[m];
    const uint8_t *p = out + mb.uoff;       // (a multiple of 16, as every slice start below)
    const uint32_t slice = (((len + 63u) >> 6) + 15u) & ~15u;
    const uint64_t lo64 = (uint64_t)lane * slice;
    const uint32_t lo = lo64 < (uint64_t)len ? (uint32_t)lo64 : len;
    const uint32_t hi = (uint64_t)lo + slice < (uint64_t)len ? lo + slice : len;
    uint32_t a = 1u, b = 0u, run = 0u;
    for (uint32_t q = lo; q < hi;) {
        if (hi - q >= 16u) {
            const uint4 v = *(const uint4 *)(p + q);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) { a += (w[k] >> (8 * j)) & 255u; b += a; }
            q += 16u; run += 16u;
        } else {
            a += p[q]; b += a;
            ++q; ++run;
        }
        if (run + 16u > kAdlerNmax) { a %= kAdlerMod; b %= kAdlerMod; run = 0u; }
    }
    pa[lane] = a % kAdlerMod; pb[lane] = b % kAdlerMod; pn[lane] = hi - lo;
    __syncthreads();
    if (lane == 0) {
        uint32_t ca = pa[0], cb = pb[0];
        for (int k = 1; k < 64; ++k) adler_combine(ca, cb, pa[k], pb[k], pn[k]);
        if (((cb << 16) | ca) != mb.crc) status[m] = (uint32_t)pcbam::kInfCrc;
    }
}

// counters of one import, in HBM
struct BwCounters {
    unsigned long long first_err;     // the lowest defect (block_defect / item_defect), kNoDefect: none
    unsigned long long by_type[3];    // items of bedGraph, variableStep and fixedStep sections
    unsigned long long bytes;         // bytes the blocks inflated to (stored blocks: their sizes)
};

// One lane per block.  Block b is bytes [off[b], off[b] + len[b]) of `data`; status (null: stored blocks): what the
// inflate and the Adler check left.  count[b]: its items, 0 with a defect.
__global__ __launch_bounds__(256) void k_bw_sections(const uint8_t *__restrict__ data, const uint64_t *__restrict__ off, const uint32_t *__restrict__ len,
                                                     const uint32_t *__restrict__ status, int64_t nblocks, const ChromOfId *__restrict__ ids, uint32_t nids,
                                                     uint32_t *__restrict__ count, BwCounters *__restrict__ cnt) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= nblocks) return;
    int err = kBwOk;
    Section s;
    s.count = 0; s.type = 0;
    if (status && status[b] != 0u) err = status[b] == (uint32_t)pcbam::kInfCrc ? kBwAdler : kBwDeflate;
    else err = check_section(data + off[b], (uint64_t)len[b], ids, nids, s);
    if (err != kBwOk) { atomicMin(&cnt->first_err, block_defect(b, err)); count[b] = 0u; return; }
    count[b] = s.count;
    if (s.count) atomicAdd(&cnt->by_type[s.type - 1u], (unsigned long long)s.count);
    atomicAdd(&cnt->bytes, (unsigned long long)len[b]);
}

// Item i of a file: its block b (first[b]: items in front of block b, the exclusive sum of the counts; blocks without
// items share their successor's sum: the last block whose sum is <= i is the one that holds item i), its place k in the
// block, the section, the item decoded and checked by the host reader's functions, the contig of its chromId.
struct ItemAt { int b; uint32_t k; Section s; Item it; ChromOfId c; int err; };
__device__ inline ItemAt item_at(const uint8_t *__restrict__ data, const uint64_t *__restrict__ off, const uint32_t *__restrict__ first, int64_t nblocks, int64_t i,
                                 const ChromOfId *__restrict__ ids) {
    ItemAt a;
    a.b = pctrack::last_at_or_below((int)nblocks, i, [first](int k) { return (int64_t)first[k]; });
    const uint8_t *p = data + off[a.b];
    a.s = section_header(p);
    a.c = ids[a.s.chrom_id];
    a.k = (uint32_t)(i - (int64_t)first[a.b]);
    a.it = section_item(a.s, p + kSectionHeader, a.k);
    a.err = check_item(a.it, a.c.size);
    return a;
}

// One lane per item.  The record of item i goes to out[i], the track's contig of it to contig_of[i] (-1 with a defect),
// its class (a bedGraph line) to cls[i].
__global__ __launch_bounds__(256) void k_bw_items(const uint8_t *__restrict__ data, const uint64_t *__restrict__ off, const uint32_t *__restrict__ first,
                                                  int64_t nblocks, int64_t nitems, const ChromOfId *__restrict__ ids, pctrack::LineRec *__restrict__ out,
                                                  int32_t *__restrict__ contig_of, uint8_t *__restrict__ cls, BwCounters *__restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nitems) return;
    const ItemAt a = item_at(data, off, first, nblocks, i, ids);
    pctrack::LineRec r;
    r.start = a.it.start; r.stop = a.it.stop; r.value = a.it.value;
    out[i] = r;
    cls[i] = (uint8_t)pctrack::kBed;
    contig_of[i] = a.err == kBwOk ? a.c.contig : -1;
    if (a.err != kBwOk) atomicMin(&cnt->first_err, item_defect(a.b, a.k, a.err));
}

// k_track_gather that accumulates: out = out + cell for the positions an item covers inside its track's extent (the
// others add the 0.0 of the reference's fill, which changes no value the sum can hold but -0.0: out starts at +0.0).
__global__ __launch_bounds__(pcdense::kGatherWG) void k_track_gather_acc(const pcdense::Item *__restrict__ items, const double *__restrict__ cells,
                                                                          double *__restrict__ out) {
    const pcdense::Item it = items[blockIdx.x];
    const int t = (int)threadIdx.x;
    double v[pcdense::kPerLane];
#pragma unroll
    for (int k = 0; k < pcdense::kPerLane; ++k) {
        const int i = t + k * pcdense::kGatherWG;
        v[k] = (i >= it.lo && i < it.hi) ? cells[it.cell0 + i] : 0.0;
    }
    double *dst = out + it.out_off;
#pragma unroll
    for (int k = 0; k < pcdense::kPerLane; ++k) {
        const int i = t + k * pcdense::kGatherWG;
        if (i < it.len) dst[(int64_t)it.step * i] = dst[(int64_t)it.step * i] + v[k];
    }
}
// the two normalisation orders: order 0 v / sum * 1e6 (BigWigGenomeArray, genome_array.py:1212), 1: 1e6 * v / sum (GenomeArray, :1528)
__global__ __launch_bounds__(256) void k_track_scale(double *__restrict__ out, int64_t n, double sum, int order) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = order == 0 ? out[i] / sum * 1e6 : 1e6 * out[i] / sum;
}

// Fixed-tree sum over tiles of cells: block b adds cells [cell0, cell0 + n) of its tile (n <= kSumTile) as
// k_track_sum_partial does; k_track_sum_final adds the partials.  The order depends on the ranges alone.
struct SumTile { int64_t cell0; int64_t n; };
__global__ __launch_bounds__(256) void k_track_sum_tiles(const SumTile *__restrict__ tiles, const double *__restrict__ cells, double *__restrict__ partial) {
    const SumTile t = tiles[blockIdx.x];
    double v = 0.0;
    for (int k = 0; k < pctrack::kSumTile / 256; ++k) {
        const int64_t p = (int64_t)k * 256 + threadIdx.x;
        if (p < t.n) v = v + cells[t.cell0 + p];
    }
    const double r = pctrack::block_tree_sum(v);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

}   // namespace pcbw
