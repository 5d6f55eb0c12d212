// bigwig_write_kernels.hip.h -- one strand slot of a track as the sections of a bigWig file (revision 19).  The source is
// the cells of the slot's contigs in the sorted order of their names, one ExRange (track_table.h) per contig over a
// common cell index e; what is written and how cells group into items is bigwig_write_host.h's (written, same_item).
//   k_bww_flags       cell e heads an item: it is written and the cell in front of it (in its contig) does not compare
//                     equal -- k_export_flags without the zero runs.  Their exclusive sum numbers the items; k_export_bases
//                     gives the items in front of every contig;
//   k_bww_items       per written cell: a head stores the item's start and float32 value, a tail (the next cell differs, or
//                     the contig ends) its end -- the tail's item is the last head at or in front of it: idx + flag - 1.
//                     Each goes twice: into the item columns, and into the item's 12 bytes of its section in the raw
//                     buffer, where section s of the file stands at 24 s + 12 x (items in front of it);
//   k_bww_headers     one lane per section: the 24-byte header in front of its items, the section's bounds for the host's
//                     R-tree, and offset and length of the section as an input of k_zlib_deflate;
//   k_bww_summary     the total summary in a fixed tree: a workgroup per tile of kSummaryTile items (every lane its strided
//                     items in order, the lanes by halving), k_bww_summary_final over the partials.  validCount is an
//                     integer sum and min / max are taken over float_key, so atomics in any order give them.
// The raw buffer is the input of the encoder, or the blocks themselves when the file is not compressed.
// Part of the one translation unit of plastid_counts.hip.
#pragma once
#include "bigwig_write_host.h"

namespace pcbww {

// a section of the file: its contig's id, its first item and its item count
struct DevSection { uint32_t chrom, count; uint64_t first; };
// sum and sum of squares of a tile (or of all), and the order-free parts
struct DevSummary { unsigned long long valid; uint32_t kmin, kmax; double sum, sumsq; };
constexpr int kSummaryTile = 256 * 16;

__global__ __launch_bounds__(256) void k_bww_flags(const pctrack::ExRange *__restrict__ ranges, int K, int64_t E, const double *__restrict__ cells,
                                                   uint32_t *__restrict__ flags) {
#pragma unroll
    for (int k = 0; k < pctrack::kExportTile / 256; ++k) {
        const int64_t e = (int64_t)blockIdx.x * pctrack::kExportTile + k * 256 + threadIdx.x;
        if (e >= E) continue;
        const pctrack::ExRange r = ranges[pctrack::ex_range_of(ranges, K, e)];
        const int64_t j = e - r.e0;
        const double v = cells[r.cell0 + j];
        flags[e] = (written(v) && (j == 0 || !same_item(cells[r.cell0 + j - 1], v))) ? 1u : 0u;
    }
}

// sec_first[c]: sections in front of contig c; ranges[c].run_base: items in front of it
__global__ __launch_bounds__(256) void k_bww_items(const pctrack::ExRange *__restrict__ ranges, int K, int64_t E, const double *__restrict__ cells,
                                                   const uint32_t *__restrict__ flags, const uint32_t *__restrict__ idx, const int64_t *__restrict__ sec_first,
                                                   uint32_t items_per_slot, uint32_t *__restrict__ item_start, uint32_t *__restrict__ item_end,
                                                   float *__restrict__ item_value, uint8_t *__restrict__ raw) {
#pragma unroll
    for (int k = 0; k < pctrack::kExportTile / 256; ++k) {
        const int64_t e = (int64_t)blockIdx.x * pctrack::kExportTile + k * 256 + threadIdx.x;
        if (e >= E) continue;
        const int c = pctrack::ex_range_of(ranges, K, e);
        const pctrack::ExRange r = ranges[c];
        const int64_t j = e - r.e0;
        const double v = cells[r.cell0 + j];
        if (!written(v)) continue;
        const uint32_t head = flags[e];
        const bool tail = j + 1 == r.n || !same_item(v, cells[r.cell0 + j + 1]);
        if (!head && !tail) continue;
        const int64_t i = (int64_t)idx[e] + (int64_t)head - 1;                      // the item of this cell
        const int64_t s = sec_first[c] + (i - r.run_base) / (int64_t)items_per_slot;
        uint8_t *p = raw + 24 * (s + 1) + 12 * i;                                     // (a multiple of 4)
        if (head) {
            const float f = (float)v;
            item_start[i] = (uint32_t)j; item_value[i] = f;
            *(uint32_t *)p = (uint32_t)j; *(uint32_t *)(p + 8) = float_bits(f);
        }
        if (tail) { item_end[i] = (uint32_t)(j + 1); *(uint32_t *)(p + 4) = (uint32_t)(j + 1); }
    }
}

__global__ __launch_bounds__(256) void k_bww_headers(const DevSection *__restrict__ sections, int64_t nsec, const uint32_t *__restrict__ item_start,
                                                     const uint32_t *__restrict__ item_end, uint8_t *__restrict__ raw, uint32_t *__restrict__ sec_start,
                                                     uint32_t *__restrict__ sec_end, int64_t *__restrict__ in_off, int64_t *__restrict__ in_len) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= nsec) return;
    const DevSection d = sections[s];
    const uint32_t a = item_start[d.first], b = item_end[d.first + d.count - 1u];
    const int64_t at = 24 * s + 12 * (int64_t)d.first;
    put_section_header(raw + at, d.chrom, a, b, d.count);
    sec_start[s] = a; sec_end[s] = b;
    in_off[s] = at; in_len[s] = 24 + 12 * (int64_t)d.count;
}

__device__ __forceinline__ double bww_tree_sum(double *s, double v) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + w];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}
// partial[b]: sum and sum of squares of tile b; total: valid, kmin, kmax by atomics (set to 0, kNoKeyMin, kNoKeyMax before)
__global__ __launch_bounds__(256) void k_bww_summary(const uint32_t *__restrict__ item_start, const uint32_t *__restrict__ item_end, const float *__restrict__ item_value,
                                                     int64_t nitems, DevSummary *__restrict__ partial, DevSummary *__restrict__ total) {
    __shared__ double sh[256];
    Summary m;
    const int64_t base = (int64_t)blockIdx.x * kSummaryTile;
    for (int k = 0; k < kSummaryTile / 256; ++k) {
        const int64_t i = base + (int64_t)k * 256 + threadIdx.x;
        if (i < nitems) summary_add(m, item_start[i], item_end[i], item_value[i]);
    }
    const double sum = bww_tree_sum(sh, m.sum), sumsq = bww_tree_sum(sh, m.sumsq);
    if (threadIdx.x == 0) { partial[blockIdx.x].sum = sum; partial[blockIdx.x].sumsq = sumsq; }
    if (m.valid) atomicAdd(&total->valid, (unsigned long long)m.valid);
    if (m.kmin != kNoKeyMin) atomicMin(&total->kmin, m.kmin);
    if (m.kmax != kNoKeyMax) atomicMax(&total->kmax, m.kmax);
}
__global__ __launch_bounds__(256) void k_bww_summary_final(const DevSummary *__restrict__ partial, int64_t n, DevSummary *__restrict__ total) {
    __shared__ double sh[256];
    double a = 0.0, b = 0.0;
    for (int64_t p = threadIdx.x; p < n; p += 256) { a = a + partial[p].sum; b = b + partial[p].sumsq; }
    const double sum = bww_tree_sum(sh, a), sumsq = bww_tree_sum(sh, b);
    if (threadIdx.x == 0) { total->sum = sum; total->sumsq = sumsq; }
}

}   // namespace pcbww
