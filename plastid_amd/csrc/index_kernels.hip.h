// The BAI or CSI index of a BAM file from the records the decoder has in HBM (bam_kernels.hip.h: k_bam_chain's record starts,
// k_bam_fields' RecOut): what htslib's sam_index_build pushes record by record (kent/src/htslib/sam.c:470-496,
// hts_idx_push hts.c:1293-1351), restated as streaming kernels over the records in file order.  The index shape is
// (min_shift, n_lvls): leaves of 2^min_shift positions, n_lvls levels of 8 children below the root; BAI is (14, 5)
// (SAM specification section 5.1.1, 5.2), a CSI takes its depth from the longest reference (5.3).  The host finishes the
// index (bam_index.h); for a CSI the linear windows stay in HBM and end as one offset per bin (k_idx_first_window, a
// running maximum, k_idx_loff).  Every kernel: one thread per record (or run, or reference), 256 per workgroup, plain
// stores -- each output element has exactly one writer.
#pragma once
#include "bam_kernels.hip.h"
#include "index_shape.h"

namespace pcidx {

constexpr uint64_t kNoKey = ~0ull;            // the key of a record that belongs to no bin (unplaced)
constexpr int64_t kBaiReach = (int64_t)1 << 29;   // the coordinates a 5-level index with 16 kb leaves can hold
constexpr uint32_t kMetaBin = 37450u;         // samtools' pseudo-bin: ((1 << 18) - 1) / 7 + 1

using pcshape::kBaiShift;
using pcshape::kBaiLvls;
using pcshape::level_first;
constexpr int kMinShiftLo = 8, kMinShiftHi = 30;   // the leaf sizes a CSI build accepts: at most 8 levels for 32-bit coordinates, bins below 2^27
constexpr int64_t kMaxWindows = (int64_t)1 << 28;  // the windows of all references a CSI build holds in HBM (8 bytes each, twice)

// the bin of [beg, end) (SAM specification 5.3, reg2bin; hts_reg2bin): from the leaves up, the first level at which
// beg and end - 1 share a bin
__host__ __device__ __forceinline__ uint32_t reg2bin(int64_t beg, int64_t end, int min_shift, int n_lvls) {
    --end;
    int s = min_shift;
    for (int l = n_lvls; l > 0; --l, s += 3)
        if (beg >> s == end >> s) return (uint32_t)(level_first(l) + (uint32_t)(beg >> s));
    return 0u;
}

// Record i -> what the index needs of it (thread nrec writes the closing entries).
//   key[i]     tid << 32 | bin of [POS, bam_endpos) (kNoKey: unplaced); bam_endpos = POS + the reference length of the
//              CIGAR (M D N = X) when FLAG 0x4 is unset and there is a CIGAR, else POS + 1 (sam.c:338-344) -- not
//              RecOut.end, which stops at the last ALIGNED base
//   voff[i]    the virtual offset bgzf_tell gives at the record's first byte (bgzf.c:569-572): blk[2 m] << 16 when the
//              record starts the member, blk[2 m + 1] << 16 | offset in the payload otherwise; voff[nrec] = blk[2 nm] << 16
//   win_a[i]   first window (2^min_shift positions); cov[i] = tid << 32 | (last window + 1) for a placed record with FLAG 0x4 unset, else 0
//   mapped[i]  1 for those records
// blk: per member {file offset of the first gzip header whose payload begins where this member's does, file offset of the
// member's own header}; entry nm: where the stream ends.  *beyond is set when a record reaches past the index's reach,
// 2^(min_shift + 3 n_lvls).  kBai: the shape is the BAI's constants and the two arguments are not read.
template <bool kBai>
__global__ __launch_bounds__(256) void k_idx_keys(const uint8_t *__restrict__ stream, const pcbam::Member *__restrict__ members,
                                                  const uint64_t *__restrict__ blk, const uint64_t *__restrict__ rec_base,
                                                  const uint32_t *__restrict__ rec_off, int nmembers, int64_t nrec,
                                                  const uint32_t *__restrict__ rec_member, const pcbam::RecOut *__restrict__ recs,
                                                  uint64_t *key, uint64_t *voff, int32_t *win_a, uint64_t *cov, uint32_t *mapped,
                                                  uint32_t *beyond, int min_shift_arg, int n_lvls_arg) {
    using namespace pcbam;
    const int min_shift = kBai ? kBaiShift : min_shift_arg, n_lvls = kBai ? kBaiLvls : n_lvls_arg;
    const int64_t reach = (int64_t)1 << (min_shift + 3 * n_lvls);
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
        if (end > reach) { *beyond = 1u; end = reach; }   // (refused by the host; the same value from every writer)
        // (a CIGAR without reference bases gives end == POS: hts_reg2bin and insert_to_l take it as it is -- the bin of
        // [POS, POS - 1], no window written, n_intv up to POS >> min_shift -- and so do reg2bin and the window range here)
        k = (uint64_t)(uint32_t)o.tid << 32 | reg2bin(o.pos, end, min_shift, n_lvls);
        a = (int32_t)((int64_t)o.pos >> min_shift);
        if (is_mapped) { c = (uint64_t)(uint32_t)o.tid << 32 | (uint64_t)(((end - 1) >> min_shift) + 1); mp = 1u; }
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

// ---- CSI only: the windows never leave HBM; every bin takes the offset of its first window (update_loff, hts.c:1193-1221)

// The windows in front of a reference's first covered one take the offset of its first record (offset0: the pseudo-bin's
// file begin): written into the reference's first window where k_idx_linear left it uncovered.  The file is sorted, so
// the covered values never decrease along `linear`, from one reference to the next either, and none lies below the
// first record of its reference: an inclusive running maximum over the whole array then is the forward fill.
__global__ __launch_bounds__(256) void k_idx_first_window(int n_ref, const int32_t *__restrict__ n_intv, const int64_t *__restrict__ lin_base,
                                                          const uint64_t *__restrict__ ref_beg, uint64_t *linear) {
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= n_ref || n_intv[t] <= 0) return;
    uint64_t *w = linear + lin_base[t];
    if (*w == 0) *w = ref_beg[t];
}

// Run j of the sorted runs -> loff of its bin: the filled window at the bin's first leaf (hts_bin_bot), 0 when the
// reference's windows end before it (a reference with placed-unmapped records only has none).
__global__ __launch_bounds__(256) void k_idx_loff(const int32_t *__restrict__ tid, const uint32_t *__restrict__ bin, int64_t nruns, int n_lvls,
                                                  const int32_t *__restrict__ n_intv, const int64_t *__restrict__ lin_base,
                                                  const uint64_t *__restrict__ filled, uint64_t *loff) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nruns) return;
    const uint32_t b = bin[j];
    int level = 0;
    while (level < n_lvls && b >= level_first(level + 1)) ++level;
    const int64_t bot = (int64_t)(b - level_first(level)) << (3 * (n_lvls - level));
    const int t = tid[j];
    loff[j] = bot < (int64_t)n_intv[t] ? filled[lin_base[t] + bot] : 0;
}

} // namespace pcidx
