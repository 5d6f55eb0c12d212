// bigwig_zoom_kernels.hip.h -- the zoom levels of a bigWig file from the item columns of the export (revision 21).  What a
// level is -- the window grid, the per-window functions, the record -- is bigwig_write_host.h's ("zoom levels"): the
// kernels compile zoom_window0, zoom_merge and zoom_record_words from it, so a window is the serial model's to the bit.
// Windows are numbered over all candidate levels (ZoomGrid): level k starts at level_off[k]; inside a level the contigs
// stand in order, contig c of level k at rows[k (K + 1) + c] -- an exclusive sum of ceil(size / r_k), made on the host.
// The accumulators are dense per-window columns (ZoomColumns: 28 bytes a window), level k + 1 a quarter of level k.
//   k_bwz_level0    one lane per window of level 0: its contig by bisection in the level's row, the first item of the
//                   contig whose end lies beyond the window's start by bisection in the item columns, then the items in
//                   order while they start in front of the window's end (sorted and disjoint: at most r0 of them);
//   k_bwz_reduce    one lane per window of level k >= 1: its four children of level k - 1 in order;
//                   both store the window's flag (valid > 0); the exclusive sum of the flags over all levels numbers
//                   the records, and k_bwz_bases reads the sum at the start of every (level, contig): the record counts
//                   the host cuts the blocks and ends the pyramid by;
//   k_bwz_records   one lane per window of the written levels: a window with data stores its 32-byte record at its number
//                   -- the raw blocks back to back, each the input of k_zlib_deflate or a block of the file as it is;
//   k_bwz_blocks    one lane per block: its bounds for the level's R-tree, its offset and length as an encoder input.
// Part of the one translation unit of plastid_counts.hip.
#pragma once
#include "bigwig_write_host.h"

namespace pcbww {

struct ZoomColumns { uint32_t *valid, *kmin, *kmax; double *sum, *sumsq; };

__device__ __forceinline__ ZoomAcc bwz_load(const ZoomColumns &col, int64_t p) {
    ZoomAcc a;
    a.valid = col.valid[p]; a.kmin = col.kmin[p]; a.kmax = col.kmax[p]; a.sum = col.sum[p]; a.sumsq = col.sumsq[p];
    return a;
}
__device__ __forceinline__ void bwz_store(const ZoomColumns &col, uint32_t *__restrict__ flags, int64_t p, const ZoomAcc &a) {
    col.valid[p] = a.valid; col.kmin[p] = a.kmin; col.kmax[p] = a.kmax; col.sum[p] = a.sum; col.sumsq[p] = a.sumsq;
    flags[p] = a.valid > 0u ? 1u : 0u;
}

// rows: the grid's rows (level 0 first); sizes: K contig sizes; item_first: the items in front of every contig (K + 1)
__global__ __launch_bounds__(256) void k_bwz_level0(ZoomGrid g, const int64_t *__restrict__ rows, const uint32_t *__restrict__ sizes, const int64_t *__restrict__ item_first,
                                                    const uint32_t *__restrict__ item_start, const uint32_t *__restrict__ item_end, const float *__restrict__ item_value,
                                                    ZoomColumns col, uint32_t *__restrict__ flags) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= g.level_off[1]) return;
    const int c = zoom_contig_of(rows, g.K, p);
    const uint64_t ws = (uint64_t)(p - rows[c]) * g.r[0];
    const uint64_t we = ws + g.r[0] < (uint64_t)sizes[c] ? ws + g.r[0] : (uint64_t)sizes[c];
    bwz_store(col, flags, p, zoom_window0(item_start, item_end, item_value, item_first[c], item_first[c + 1], (uint32_t)ws, (uint32_t)we));
}

// level k >= 1 from level k - 1
__global__ __launch_bounds__(256) void k_bwz_reduce(ZoomGrid g, int k, const int64_t *__restrict__ rows, ZoomColumns col, uint32_t *__restrict__ flags) {
    const int64_t p = g.level_off[k] + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= g.level_off[k + 1]) return;
    const int64_t *row = rows + (size_t)k * (size_t)(g.K + 1), *under = rows + (size_t)(k - 1) * (size_t)(g.K + 1);
    const int c = zoom_contig_of(row, g.K, p);
    const int64_t first = 4 * (p - row[c]), below = under[c + 1] - under[c];
    ZoomAcc a;
    for (int64_t j = first; j < first + 4 && j < below; ++j) zoom_merge(a, bwz_load(col, under[c] + j));
    bwz_store(col, flags, p, a);
}

// out[j] = idx[rows[j]]: the records in front of every (level, contig) and, at a row's end, in front of the next level
__global__ __launch_bounds__(256) void k_bwz_bases(const int64_t *__restrict__ rows, int64_t n, const uint32_t *__restrict__ idx, int64_t *__restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n) out[j] = (int64_t)idx[rows[j]];
}

// windows [0, nwin) are those of the written levels; raw: 32 bytes per record, 16-byte aligned
__global__ __launch_bounds__(256) void k_bwz_records(ZoomGrid g, int64_t nwin, const int64_t *__restrict__ rows, const uint32_t *__restrict__ sizes, ZoomColumns col,
                                                     const uint32_t *__restrict__ flags, const uint32_t *__restrict__ idx, uint8_t *__restrict__ raw) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= nwin || !flags[p]) return;
    const int k = zoom_level_of(g, p);
    const int64_t *row = rows + (size_t)k * (size_t)(g.K + 1);
    const int c = zoom_contig_of(row, g.K, p);
    const uint64_t ws = (uint64_t)(p - row[c]) * g.r[k];
    const uint64_t we = ws + g.r[k] < (uint64_t)sizes[c] ? ws + g.r[k] : (uint64_t)sizes[c];
    uint32_t w[8];
    zoom_record_words(w, (uint32_t)c, (uint32_t)ws, (uint32_t)we, bwz_load(col, p));
    uint4 *dst = (uint4 *)(raw + (size_t)idx[p] * kZoomRecordBytes);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

__global__ __launch_bounds__(256) void k_bwz_blocks(const ZoomBlock *__restrict__ blocks, int64_t nblk, const uint8_t *__restrict__ raw, uint32_t *__restrict__ blk_start,
                                                    uint32_t *__restrict__ blk_end, int64_t *__restrict__ in_off, int64_t *__restrict__ in_len) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= nblk) return;
    const ZoomBlock d = blocks[b];
    const uint32_t *first = (const uint32_t *)(raw + (size_t)d.first * kZoomRecordBytes), *last = (const uint32_t *)(raw + (size_t)(d.first + d.count - 1u) * kZoomRecordBytes);
    blk_start[b] = first[1]; blk_end[b] = last[2];
    in_off[b] = (int64_t)d.first * (int64_t)kZoomRecordBytes; in_len[b] = (int64_t)d.count * (int64_t)kZoomRecordBytes;
}

}   // namespace pcbww
