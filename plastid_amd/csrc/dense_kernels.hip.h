// dense_kernels.hip.h -- the kernels of the dense vector of a staged file (dense_host.h says what it is; dense_for_plan
// and count_dense in plastid_counts.hip build and use it).
//   build:  k_dense_narrow     int64 counts of the whole extent -> 16-bit cells, escapes counted
//           k_dense_overflow   the escaped cells as (cell index, count) pairs, in any order (sorted by the caller)
//   plan:   k_dense_seg_items  items per segment; k_dense_items: the item descriptors (dense_host.h, cut_item)
//   count:  k_dense_gather     one 256-thread workgroup per item: descriptor, cells, stores
// Included behind pc_kernels.hip.h (out_conv, OutT_, GatherSeg).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dense_host.h"
#include "plan_tables.h"

namespace pcdense {

constexpr int kGatherWG = 256;
constexpr int kPerLane = kItemLen / kGatherWG;   // 8 positions per lane

// 16-bit cells from the int64 counts of the build's plan; *n_escaped += cells that hold kEscape or more
__global__ __launch_bounds__(256) void k_dense_narrow(const int64_t *__restrict__ src, int64_t n, uint16_t *__restrict__ cells, uint32_t *__restrict__ n_escaped) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t v = src[i];
    const bool esc = v >= (int64_t)kEscape;
    cells[i] = esc ? (uint16_t)kEscape : (uint16_t)v;
    if (esc) atomicAdd(n_escaped, 1u);
}

// the escaped cells; `cap`: entries the lists hold (the count k_dense_narrow left)
__global__ __launch_bounds__(256) void k_dense_overflow(const int64_t *__restrict__ src, int64_t n, uint32_t *__restrict__ cursor, uint32_t cap,
                                                        uint32_t *__restrict__ key, uint32_t *__restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t v = src[i];
    if (v < (int64_t)kEscape) return;
    const uint32_t j = atomicAdd(cursor, 1u);
    if (j < cap) { key[j] = (uint32_t)i; val[j] = (uint32_t)v; }
}

// segment s of the plan as cut_item wants it.  tid / strand: the caller's arrays; cell_off / ext: the file's layout
__device__ __forceinline__ SegIn seg_in(const pc::GatherSeg &g, int32_t tid, uint8_t strand, int ntid, const int64_t *__restrict__ cell_off,
                                        const int64_t *__restrict__ ext) {
    SegIn s;
    s.out_off = g.out_off; s.len = g.len; s.clip_lo = g.clip_lo; s.clip_hi = g.clip_hi; s.start = g.start; s.step = g.step;
    s.known = tid >= 0 && tid < ntid && g.clip_hi > g.clip_lo;
    if (s.known) {
        s.cell_base = cell_off[2 * (int64_t)tid + ((strand & 3) == PC_STRAND_REV ? 1 : 0)];   // (mode_of: an eligible plan has '+' and '-' only)
        s.ext = ext[tid];
    }
    return s;
}

// cnt[s] = items of segment s (cnt[nseg] is the caller's zero: the exclusive sum leaves the total there)
__global__ __launch_bounds__(256) void k_dense_seg_items(const pc::GatherSeg *__restrict__ gsegs, int64_t nseg, uint32_t *__restrict__ cnt) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < nseg) cnt[s] = (uint32_t)items_of(gsegs[s].len);
}

// one thread per segment writes the segment's items at[s] .. at[s + 1) (a segment is a few items: an exon, a gene)
__global__ __launch_bounds__(256) void k_dense_items(const pc::GatherSeg *__restrict__ gsegs, const int32_t *__restrict__ tid, const uint8_t *__restrict__ strand,
                                                     int64_t nseg, int ntid, const int64_t *__restrict__ cell_off, const int64_t *__restrict__ ext,
                                                     const uint32_t *__restrict__ at, Item *__restrict__ items) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= nseg) return;
    const SegIn in = seg_in(gsegs[s], tid[s], strand[s], ntid, cell_off, ext);
    const uint32_t a = at[s], n = at[s + 1] - a;
    for (uint32_t k = 0; k < n; ++k) items[a + k] = cut_item(in, (int64_t)k);
}

// the count of an escaped cell: binary search of the sorted overflow list (every escaped cell is in it)
__device__ __forceinline__ uint32_t overflow_count(uint32_t cell, const uint32_t *__restrict__ key, const uint32_t *__restrict__ val, uint32_t n) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (key[mid] < cell) lo = mid + 1; else hi = mid;
    }
    return (lo < n && key[lo] == cell) ? val[lo] : kEscape;
}

// One workgroup per item: the descriptor (one wave-uniform 32-byte load), every cell of the lane, then the stores.  Lane
// t serves positions t, t + 256, ...: a wave loads 128 consecutive bytes of cells and stores 512 consecutive bytes of
// output per instruction.  Positions outside [lo, hi) -- clipped, beyond the extent, unknown contig -- are zero.
template <int OUTMODE>
__global__ __launch_bounds__(kGatherWG) void k_dense_gather(const Item *__restrict__ items, const uint16_t *__restrict__ cells, const uint32_t *__restrict__ ovf_key,
                                                            const uint32_t *__restrict__ ovf_val, uint32_t n_ovf,
                                                            typename pc::OutT_<OUTMODE>::type *__restrict__ out, double norm_sum) {
    const Item it = items[blockIdx.x];
    const int t = (int)threadIdx.x;
    uint32_t v[kPerLane];
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
        const int i = t + k * kGatherWG;
        v[k] = (i >= it.lo && i < it.hi) ? (uint32_t)cells[it.cell0 + i] : 0u;
    }
    typename pc::OutT_<OUTMODE>::type *dst = out + it.out_off;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
        const int i = t + k * kGatherWG;
        if (i < it.len) {
            uint32_t c = v[k];
            if (c == kEscape) c = overflow_count((uint32_t)(it.cell0 + i), ovf_key, ovf_val, n_ovf);
            dst[(int64_t)it.step * i] = pc::out_conv<OUTMODE>(c, norm_sum);
        }
    }
}

} // namespace pcdense
