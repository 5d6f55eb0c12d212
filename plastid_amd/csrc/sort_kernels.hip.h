// Coordinate sort at decode (PC_BAM_SORT): the kernels around the one stable radix sort that lets a whole-file open stage
// a BAM file in any record order.  k_bam_columns writes record i at staged_at[i] and its runs from run_at[i]; a sorted open
// only fills those two arrays by rank in the sorted order instead of by rank in the file.  Part of the one translation
// unit of plastid_counts.hip (behind bam_kernels.hip.h: RecOut and the kRec* codes).
#pragma once

namespace pcbam {

// The sort key: reference id in the top 31 bits, POS + 1 in the 32 bits below, the reverse-strand bit of FLAG lowest --
// the order (tid, POS, reverse) of a coordinate sorter.  Records without a reference get all ones: below bit
// 33 + bits(n_ref - 1), all the sort looks at, that is still larger than any placed record's key (POS + 1 <= 2^31).
constexpr int kSortLowBits = 33;
__device__ __forceinline__ uint64_t sort_key(const RecOut &o) {
    if (!o.placed) return ~0ull;
    return ((uint64_t)(uint32_t)o.tid << kSortLowBits) | ((uint64_t)((uint32_t)o.pos + 1u) << 1) | (uint64_t)((o.flag >> 4) & 1u);
}
// key bits the sort has to look at for a header of n_ref references
inline int sort_key_bits(uint32_t n_ref) {
    int bits = kSortLowBits;
    for (uint32_t v = n_ref ? n_ref - 1u : 0u; v; v >>= 1) ++bits;
    return bits < 64 ? bits : 64;
}

// first_err with a sort: a record's own defects come first, lowest file index first (as in a file-order open); a pair that
// breaks the order of the first aligned positions comes behind them, a truncated last record behind everything
__device__ __forceinline__ unsigned long long sort_defect(int64_t i, uint32_t code) {
    const unsigned long long rank = (code == kRecTruncated || code == kRecBadSize) ? 2ull : (code == kRecDeletionOrder ? 1ull : 0ull);
    return (rank << 62) | ((unsigned long long)i << 8) | (unsigned long long)code;
}

// One thread per record: its key and its own index (the values of the sort).  *disorder is raised where k_bam_order's
// (tid, POS) test would refuse the record against the one in front (whatever defects of their own the two have): a file
// that raises nothing is staged in file order, by the kernels of an open without a sort.
__global__ __launch_bounds__(256) void k_bam_sort_keys(const RecOut *__restrict__ recs, int64_t nrec, uint64_t *__restrict__ keys,
                                                       uint32_t *__restrict__ index, unsigned long long *disorder) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int dis = 0;
    if (i < nrec) {
        const RecOut o = recs[i];
        keys[i] = sort_key(o);
        index[i] = (uint32_t)i;
        if (o.placed && i > 0) {
            const RecOut pr = recs[i - 1];
            dis = (!pr.placed || o.tid < pr.tid || (o.tid == pr.tid && o.pos < pr.pos)) ? 1 : 0;
        }
    }
    __shared__ int s_dis[4];
    const int any = __any(dis);
    if ((threadIdx.x & 63) == 0) s_dis[threadIdx.x >> 6] = any;
    __syncthreads();
    if (threadIdx.x == 0 && (s_dis[0] | s_dis[1] | s_dis[2] | s_dis[3])) atomicOr(disorder, 1ull);
}

// One thread per sorted rank k, source record i = perm[k] (perm[k] is also the record's number in the file).  Placed
// records come first in the sorted order, so k is the staged index; staged_at[i] arrives as the record's rank among
// the placed records of the file (the scan of a file-order open) and leaves as k, and *moved counts where the two differ.
// runs_sorted[k]: what k_bam_scan_inputs puts into runs[i].  Defects: the record's own, and the first aligned positions
// of sorted neighbours of one reference out of order (k_bam_order's test, here on the sorted order).
__global__ __launch_bounds__(256) void k_bam_sort_rank(const RecOut *__restrict__ recs, int64_t nrec, const uint32_t *__restrict__ perm,
                                                       uint32_t *staged_at, uint32_t *__restrict__ runs_sorted, unsigned long long *first_err,
                                                       unsigned long long *moved) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int mv = 0;
    if (k < nrec) {
        const int64_t i = (int64_t)perm[k];
        const RecOut o = recs[i];
        uint32_t r = 0;
        if (o.placed) {
            mv = staged_at[i] != (uint32_t)k ? 1 : 0;
            staged_at[i] = (uint32_t)k;
            if (o.nruns >= 2u) r = o.nruns;
        }
        runs_sorted[k] = r;
        if (o.err) atomicMin(first_err, sort_defect(i, o.err));
        else if (o.placed && k > 0) {
            const int64_t j = (int64_t)perm[k - 1];
            const RecOut pr = recs[j];
            if (pr.placed && pr.err == kRecOk && pr.tid == o.tid && pr.spos > o.spos) atomicMin(first_err, sort_defect(i < j ? i : j, kRecDeletionOrder));
        }
    }
    __shared__ unsigned s_mv[4];
    const unsigned n = (unsigned)__popcll(__ballot(mv));
    if ((threadIdx.x & 63) == 0) s_mv[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = s_mv[0] + s_mv[1] + s_mv[2] + s_mv[3];
        if (t) atomicAdd(moved, (unsigned long long)t);
    }
}

// run_at of the source records from the exclusive sum over runs_sorted
__global__ __launch_bounds__(256) void k_bam_sort_run_at(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ run_sorted_at, int64_t nrec,
                                                         uint32_t *__restrict__ run_at) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < nrec) run_at[perm[k]] = run_sorted_at[k];
}

} // namespace pcbam
