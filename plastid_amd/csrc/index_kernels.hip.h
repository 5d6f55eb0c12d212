// The BAI index of a BAM file from the records the decoder has in HBM (bam_kernels.hip.h: k_bam_chain's record starts,
// k_bam_fields' RecOut): what htslib's sam_index_build pushes record by record (kent/src/htslib/sam.c:470-496,
// hts_idx_push hts.c:1293-1351), restated as streaming kernels over the records in file order.  BAI: min_shift 14, 5 levels
// (SAM specification section 5.1.1, 5.2).  The host finishes the index (bam_index.h).  Every kernel: one thread per
// record (or run, or reference), 256 per workgroup, plain stores -- each output element has exactly one writer.
#pragma once
#include "bam_kernels.hip.h"

namespace pcidx {

constexpr uint64_t kNoKey = ~0ull;            // the key of a record that belongs to no bin (unplaced)
constexpr int64_t kBaiReach = (int64_t)1 << 29;   // the coordinates a 5-level index with 16 kb leaves can hold
constexpr uint32_t kMetaBin = 37450u;         // samtools' pseudo-bin: ((1 << 18) - 1) / 7 + 1

// the bin of [beg, end) (SAM specification 5.3, reg2bin; hts_reg2bin with min_shift 14, n_lvls 5)
__host__ __device__ __forceinline__ uint32_t reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0u;
}

// Record i -> what the index needs of it (thread nrec writes the closing entries).
//   key[i]     tid << 32 | bin of [POS, bam_endpos) (kNoKey: unplaced); bam_endpos = POS + the reference length of the
//              CIGAR (M D N = X) when FLAG 0x4 is unset and there is a CIGAR, else POS + 1 (sam.c:338-344) -- not
//              RecOut.end, which stops at the last ALIGNED base
//   voff[i]    the virtual offset bgzf_tell gives at the record's first byte (bgzf.c:569-572): blk[2 m] << 16 when the
//              record starts the member, blk[2 m + 1] << 16 | offset in the payload otherwise; voff[nrec] = blk[2 nm] << 16
//   win_a[i]   first 16 kb window; cov[i] = tid << 32 | (last window + 1) for a placed record with FLAG 0x4 unset, else 0
//   mapped[i]  1 for those records
// blk: per member {file offset of the first gzip header whose payload begins where this member's does, file offset of the
// member's own header}; entry nm: where the stream ends.  *beyond is set when a record reaches past 2^29.
__global__ __launch_bounds__(256) void k_idx_keys(const uint8_t *__restrict__ stream, const pcbam::Member *__restrict__ members,
                                                  const uint64_t *__restrict__ blk, const uint64_t *__restrict__ rec_base,
                                                  const uint32_t *__restrict__ rec_off, int nmembers, int64_t nrec,
                                                  const uint32_t *__restrict__ rec_member, const pcbam::RecOut *__restrict__ recs,
                                                  uint64_t *key, uint64_t *voff, int32_t *win_a, uint64_t *cov, uint32_t *mapped,
                                                  uint32_t *beyond) {
    using namespace pcbam;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > nrec) return;
    if (i == nrec) { voff[i] = blk[2 * (size_t)nmembers] << 16; cov[i] = 0; mapped[i] = 0u; return; }
    int m = (int)rec_member[i >> 8];
    while (m + 1 < nmembers && (int64_t)rec_base[m + 1] <= i) ++m;
    const uint32_t in_member = rec_off[(size_t)m * kMaxRecPerMember + (size_t)(i - (int64_t)rec_base[m])];
    voff[i] = in_member ? (blk[2 * (size_t)m + 1] << 16 | in_member) : blk[2 * (size_t)m] << 16;
    const RecOut o = recs[i];
    uint64_t k = kNoKey, c = 0;
    int32_t a = 0;
    uint32_t mp = 0u;
    if (o.placed && o.err == kRecOk) {   // (a record with a defect is reported by the decoder's checks; its bytes are not read again)
        const bool is_mapped = !(o.flag & 0x4);
        const uint8_t *r = stream + members[m].uoff + in_member + 4;
        const uint32_t l_name = r[8], n_cig = ld16(r + 12);
        int64_t end = (int64_t)o.pos + 1;
        if (is_mapped && n_cig) {
            const uint8_t *cig = r + 32 + l_name;
            int64_t rlen = 0;
            for (uint32_t q = 0; q < n_cig; ++q) {
                const uint32_t v = ld32(cig + 4 * q), op = v & 15u;
                if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) rlen += v >> 4;
            }
            end = (int64_t)o.pos + rlen;
        }
        if (end > kBaiReach) { *beyond = 1u; end = kBaiReach; }   // (refused by the host; the same value from every writer)
        // (a CIGAR without reference bases gives end == POS: hts_reg2bin and insert_to_l take it as it is -- the bin of
        // [POS, POS - 1], no window written, n_intv up to POS >> 14 -- and so do reg2bin and the window range here)
        k = (uint64_t)(uint32_t)o.tid << 32 | reg2bin(o.pos, end);
        a = (int32_t)(o.pos >> 14);
        if (is_mapped) { c = (uint64_t)(uint32_t)o.tid << 32 | (uint64_t)(((end - 1) >> 14) + 1); mp = 1u; }
    }
    key[i] = k; win_a[i] = a; cov[i] = c; mapped[i] = mp;
}

// Run heads (a run: consecutive placed records with one key) and the first / last record of every reference.
// head has nrec + 1 entries (the last 0); ref_first / ref_last are preset to -1.
__global__ __launch_bounds__(256) void k_idx_heads(const uint64_t *__restrict__ key, int64_t nrec, uint32_t *head, int64_t *ref_first,
                                                   int64_t *ref_last) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > nrec) return;
    if (i == nrec) { head[i] = 0u; return; }
    const uint64_t k = key[i];
    const uint64_t prev = i > 0 ? key[i - 1] : kNoKey, next = i + 1 < nrec ? key[i + 1] : kNoKey;
    head[i] = (k != kNoKey && (i == 0 || k != prev)) ? 1u : 0u;
    if (k == kNoKey) return;
    const uint32_t tid = (uint32_t)(k >> 32);
    if (i == 0 || (uint32_t)(prev >> 32) != tid) ref_first[tid] = i;
    if ((uint32_t)(next >> 32) != tid) ref_last[tid] = i;   // (kNoKey's high word is no reference id)
}

// slot[i] = run heads before record i (an exclusive sum of head).  A head writes its run's key and begin and closes the
// run before it; the record behind the last placed one (or the closing entry) closes the last run.
__global__ __launch_bounds__(256) void k_idx_runs(const uint64_t *__restrict__ key, const uint64_t *__restrict__ voff,
                                                  const uint32_t *__restrict__ head, const uint32_t *__restrict__ slot, int64_t nrec,
                                                  uint64_t *run_key, uint64_t *run_beg, uint64_t *run_end) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > nrec) return;
    const uint32_t s = slot[i];
    const uint64_t at = voff[i];
    if (head[i]) {
        run_key[s] = key[i]; run_beg[s] = at;
        if (s > 0) run_end[s - 1] = at;
    } else if (s > 0 && i > 0 && key[i - 1] != kNoKey && (i == nrec || key[i] == kNoKey)) run_end[s - 1] = at;
}

// the runs in (tid, bin) order: order[j] = the slot of the j-th run of the stable sort by key
__global__ __launch_bounds__(256) void k_idx_gather(const uint64_t *__restrict__ sorted_key, const uint32_t *__restrict__ order,
                                                    const uint64_t *__restrict__ run_beg, const uint64_t *__restrict__ run_end, int64_t nruns,
                                                    int32_t *tid, uint32_t *bin, uint64_t *beg, uint64_t *end) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nruns) return;
    const uint64_t k = sorted_key[j];
    const uint32_t s = order[j];
    tid[j] = (int32_t)(k >> 32); bin[j] = (uint32_t)k; beg[j] = run_beg[s]; end[j] = run_end[s];
}

// Per reference, from its first and last record: the pseudo-bin's file range [offset of its first record, offset of the
// first record behind its last), its mapped / unmapped counts (mapped_before: exclusive sum of mapped) and n_intv, the
// windows its linear index has: covered[i] is the exclusive running maximum of cov, so covered[last + 1] carries
// tid << 32 | (highest covered window + 1) when a mapped record of this reference set it.
__global__ __launch_bounds__(256) void k_idx_ref_stats(int n_ref, const int64_t *__restrict__ ref_first, const int64_t *__restrict__ ref_last,
                                                       const uint64_t *__restrict__ voff, const uint32_t *__restrict__ mapped_before,
                                                       const uint64_t *__restrict__ covered, uint64_t *ref_beg, uint64_t *ref_end,
                                                       int64_t *ref_mapped, int64_t *ref_unmapped, int32_t *n_intv) {
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= n_ref) return;
    const int64_t f = ref_first[t], l = ref_last[t];
    if (f < 0) { ref_beg[t] = 0; ref_end[t] = 0; ref_mapped[t] = 0; ref_unmapped[t] = 0; n_intv[t] = 0; return; }
    const int64_t nm = (int64_t)mapped_before[l + 1] - (int64_t)mapped_before[f];
    const uint64_t c = covered[l + 1];
    ref_beg[t] = voff[f]; ref_end[t] = voff[l + 1];
    ref_mapped[t] = nm; ref_unmapped[t] = (l - f + 1) - nm;
    n_intv[t] = (uint32_t)(c >> 32) == (uint32_t)t ? (int32_t)(uint32_t)c : 0;
}

// The linear index (insert_to_l, hts.c:1150-1169: a window keeps the offset of the first mapped record that covers it).
// The file is sorted, so the earlier mapped records of a reference cover, of the windows from this record's first on,
// exactly those below the running maximum of (last window + 1): the record writes the rest of its own.  lin_base[tid]:
// where the reference's windows start in `linear` (preset to 0 = not covered).
__global__ __launch_bounds__(256) void k_idx_linear(const uint64_t *__restrict__ cov, const uint64_t *__restrict__ covered,
                                                    const int32_t *__restrict__ win_a, const uint64_t *__restrict__ voff, int64_t nrec,
                                                    const int64_t *__restrict__ lin_base, uint64_t *linear) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrec) return;
    const uint64_t c = cov[i];
    if (!c) return;   // (not counted, or tid 0 with no window)
    const uint32_t tid = (uint32_t)(c >> 32);
    const uint64_t before = covered[i];
    int64_t w = win_a[i];
    if ((uint32_t)(before >> 32) == tid && (int64_t)(uint32_t)before > w) w = (int64_t)(uint32_t)before;
    const int64_t w_end = (int64_t)(uint32_t)c;
    const uint64_t at = voff[i];
    uint64_t *out = linear + lin_base[tid];
    for (; w < w_end; ++w) out[w] = at;
}

} // namespace pcidx
