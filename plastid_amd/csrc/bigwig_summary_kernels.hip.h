// bigwig_summary_kernels.hip.h -- binned summaries of a bigWig file on the GPU (revision 23).  The arithmetic is
// bigwig_summary_host.h's: the kernels call its PC_BW_HD functions.  A TABLE is the records of one zoom level (ZoomRec, the
// file's 32-byte record as it is) or the items of the file (ItemRec, 16 bytes), in file order, in HBM:
//   k_bbi_zoom_records  one lane per record: its block by bisection over the exclusive sum of the blocks' record counts,
//                       the 32 bytes read field by field (a stored block lies at any offset of the file) into one ZoomRec;
//   k_bbi_items         one lane per item: located, decoded and checked as k_bw_items' (pcbw::item_at) -> ItemRec, the
//                       lowest defect;
//   k_bbi_index         one lane per record: index_record -> the table's order flag, and per chromId the number of runs
//                       and the bounds of (the last of) them;
//   k_bbi_summarize     ONE LANE PER (query, bin), a zoom and an items instantiation: the bin's edges, a binary search for
//                       the first record of the walk inside the contig's range, the ordered walk (slice), the five element
//                       fields into five columns of one output buffer.  A lane walks its bin serially: the sums are
//                       order-exact.  A record is one 16- or 32-byte load; neighbouring lanes walk neighbouring records.
// No input makes a kernel read outside its buffers: a record is read inside [lo, hi) of its contig only, bounds the host
// takes from k_bbi_index's output and checks against the table's size; a block's bytes are read below its inflated
// length only.  Every store is a plain vector store.
// Part of the one translation unit of plastid_counts.hip (behind bigwig_kernels.hip.h).
#pragma once
#include "bigwig_summary_host.h"

namespace pcbws {

// first[b]: records in front of block b (nblocks + 1 entries); block b's bytes stand at data + off[b]
__global__ __launch_bounds__(256) void k_bbi_zoom_records(const uint8_t *__restrict__ data, const uint64_t *__restrict__ off, const uint32_t *__restrict__ first,
                                                          int64_t nblocks, int64_t nrec, ZoomRec *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrec) return;
    const int b = pctrack::last_at_or_below((int)nblocks, i, [first](int k) { return (int64_t)first[k]; });
    const uint8_t *p = data + off[b] + (uint64_t)(i - (int64_t)first[b]) * pcbww::kZoomRecordBytes;
    ZoomRec r;
    r.chrom = pcbw::rd32(p); r.start = pcbw::rd32(p + 4); r.end = pcbw::rd32(p + 8); r.valid = pcbw::rd32(p + 12);
    r.mn = pcbw::rdf32(p + 16); r.mx = pcbw::rdf32(p + 20); r.sum = pcbw::rdf32(p + 24); r.sumsq = pcbw::rdf32(p + 28);
    out[i] = r;
}

// As k_bw_items (pcbw::item_at), into ItemRec.  ids: by chromId, contig >= 0 for an id of the tree.
__global__ __launch_bounds__(256) void k_bbi_items(const uint8_t *__restrict__ data, const uint64_t *__restrict__ off, const uint32_t *__restrict__ first,
                                                   int64_t nblocks, int64_t nitems, const pcbw::ChromOfId *__restrict__ ids, ItemRec *__restrict__ out,
                                                   pcbw::BwCounters *__restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nitems) return;
    const pcbw::ItemAt a = pcbw::item_at(data, off, first, nblocks, i, ids);
    ItemRec r;
    r.chrom = a.s.chrom_id; r.start = (uint32_t)a.it.start; r.end = (uint32_t)a.it.stop; r.value = (float)a.it.value;   // (the float32 of the file, widened and back)
    out[i] = r;
    if (a.err != pcbw::kBwOk) atomicMin(&cnt->first_err, pcbw::item_defect(a.b, a.k, a.err));
}

// flag[0]: the table is not in coordinate order.  runs / lo / hi: by chromId (nids of each), zeroed by the caller.
template <typename R>
__global__ __launch_bounds__(256) void k_bbi_index(const R *__restrict__ recs, int64_t n, uint32_t nids, uint32_t *__restrict__ flag, uint32_t *__restrict__ runs,
                                                   int64_t *__restrict__ lo, int64_t *__restrict__ hi) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const unsigned what = index_record(recs, n, k, nids);
    if (what & 1u) atomicOr(flag, 1u);
    const uint32_t c = recs[k].chrom;
    if (c >= nids) return;
    if (what & 2u) { lo[c] = k; atomicAdd(&runs[c], 1u); }
    if (what & 4u) hi[c] = k + 1;
}

// One query of a launch: its bounds, the records [lo, hi) of its contig, and its place in the caller's order.
struct DevQuery { uint32_t start, end; int64_t lo, hi, q; };

// out: five columns of `total` doubles (validCount, min, max, sum, sum of squares); lane (g, bin) writes element
// qs[g].q * n_bins + bin of each.
template <typename R>
__global__ __launch_bounds__(256) void k_bbi_summarize(const R *__restrict__ recs, const DevQuery *__restrict__ qs, int64_t nlanes, uint32_t n_bins, int64_t total,
                                                       double *__restrict__ out) {
    const int64_t lane = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (lane >= nlanes) return;
    const int64_t g = lane / (int64_t)n_bins;
    const uint32_t bin = (uint32_t)(lane - g * (int64_t)n_bins);
    const DevQuery q = qs[g];
    const uint32_t bs = bin_start(q.start, q.end, bin, n_bins), be = bin_edge(q.start, q.end, bin, n_bins);
    const Element el = slice(recs, q.lo, q.hi, q.start, q.end, bs, be);
    const int64_t o = q.q * (int64_t)n_bins + (int64_t)bin;
    out[o] = (double)el.valid;
    out[total + o] = el.mn;
    out[2 * total + o] = el.mx;
    out[3 * total + o] = el.sum;
    out[4 * total + o] = el.sumsq;
}

}   // namespace pcbws
