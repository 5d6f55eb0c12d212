// dense_host.h -- host arithmetic of the DENSE VECTOR of a staged file (dense_kernels.hip.h, dense_for_plan in
// plastid_counts.hip): one 16-bit cell per (contig, strand, position) that holds what a count under the engine's point
// rule, size filter and FLAG / MAPQ / NH filters returns for that position.  Under a point rule that value does not
// depend on the query, so a steady count of a '+' / '-' plan is a copy with widening: the plan's segments are cut into
// ITEMS of at most kItemLen positions and one workgroup serves one item (a batch of kBatch = 1).
// Here: the extent of a contig and the cell offsets, the eligibility decision, the cutting of a segment into items, the
// pairing of an item's output elements and the batches.
// Plain C++17 (no HIP): tests/dense_host_test.cpp and tests/dense_batches_test.cpp compile it on a machine without a
// GPU; cut_item, pair_cut, pair_slot and batches_of are the very functions the kernels and their launch call.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PCDENSE_HD __host__ __device__
#else
#define PCDENSE_HD
#endif

namespace pcdense {

constexpr int kItemLen = 2048;               // positions of an item: 256 lanes x 8
constexpr uint32_t kEscape = 65535u;         // cell value "see the overflow list" (every count >= 65 535)
constexpr int64_t kBytesPerCell = 2;
// The build counts the whole extent into an int64 block of the engine's pool (8 bytes per cell) before it narrows it.
// The block may take 1 GiB: 2^27 cells, a genome of 67 M nt on both strands -- five yeasts, half a fly.  A human-scale
// file (6.2 G cells) is refused here before its 50 GB block is ever asked for; its streams are far smaller anyway.
constexpr int64_t kBuildBlockCap = (int64_t)1 << 30;

// positions [0, extent) of a contig have cells; every other position counts zero.  `declared`: the length the header
// names (0: none known), `furthest_end`: the furthest aligned end among the staged reads (0: no read)
PCDENSE_HD inline int64_t extent(int64_t declared, int64_t furthest_end) {
    const int64_t d = declared > 0 ? declared : 0, f = furthest_end > 0 ? furthest_end : 0;
    return d > f ? d : f;
}

// cell_off[2 * t + s]: first cell of contig t on strand s (0 '+', 1 '-'); cell_off[2 * ntid]: all cells.  `ext`: the
// extents.  Returns the cell count.
inline int64_t layout(int ntid, const int64_t *ext, int64_t *cell_off) {
    int64_t at = 0;
    for (int t = 0; t < ntid; ++t)
        for (int s = 0; s < 2; ++s) { cell_off[2 * t + s] = at; at += ext[t]; }
    cell_off[2 * ntid] = at;
    return at;
}

// What the decision looks at.  The first block restates the plan conditions of the canonical stream.
struct PlanIn {
    int nfiles = 0;
    bool point_rule = false;     // fiveprime, threeprime or variable
    int rows = 1;
    uint32_t modes = 0;          // strand modes of the plan's windows (bit 0 '+', bit 1 '-', bits 2, 3: unstranded)
    bool has_sums = false;       // some slice is summed (out_step 0)
    bool forbidden = false;      // PC_NO_DENSE, or the plan is the build's own
    int64_t cells = 0;
    int64_t stream_entries = 0;  // of the stream the vector replaces: canonical, else compact, else the records (4 bytes each)
};

inline bool plan_conditions(const PlanIn &p) {
    return !p.forbidden && p.nfiles == 1 && p.point_rule && p.rows == 1 && (p.modes & ~3u) == 0u && p.modes != 0u && !p.has_sums;
}
inline bool size_rule(int64_t cells, int64_t stream_entries) { return cells > 0 && cells * kBytesPerCell <= stream_entries * 4; }
inline bool build_fits(int64_t cells) { return cells * 8 <= kBuildBlockCap; }
inline bool eligible(const PlanIn &p) { return plan_conditions(p) && size_rule(p.cells, p.stream_entries) && build_fits(p.cells); }

// One segment of the plan as GatherSeg has it (plan_tables.h), with its contig and strand resolved: `known` false --
// unknown contig -- or an empty clip: all zero.
struct SegIn {
    int64_t out_off = 0;
    int64_t len = 0;
    int64_t clip_lo = 0, clip_hi = 0;   // segment-relative positions [clip_lo, clip_hi) lie on the contig's axis
    int64_t start = 0;                  // genomic coordinate of position 0
    int32_t step = 1;                   // +1 / -1: position i goes to out[out_off + step * i]
    bool known = false;
    int64_t cell_base = 0;              // first cell of (contig, strand)
    int64_t ext = 0;                    // extent of the contig
};

// position i of the item (0 <= i < len) goes to out[out_off + step * i]; it reads cells[cell0 + i] when lo <= i < hi
// and is zero otherwise.  lo == hi: all zero (cell0 is -1 then).
struct Item {
    int64_t out_off;
    int64_t cell0;
    int32_t len, step, lo, hi;
};
static_assert(sizeof(Item) == 32, "Item is 32 bytes in HBM");

PCDENSE_HD inline int64_t items_of(int64_t len) { return len > 0 ? (len + kItemLen - 1) / kItemLen : 0; }

// item k (0 <= k < items_of(s.len)) of segment s
PCDENSE_HD inline Item cut_item(const SegIn &s, int64_t k) {
    const int64_t a = k * kItemLen;                                      // first segment-relative position
    const int64_t n = s.len - a < kItemLen ? s.len - a : kItemLen;
    Item it;
    it.out_off = s.out_off + (int64_t)s.step * a;
    it.len = (int32_t)n; it.step = s.step; it.lo = 0; it.hi = 0; it.cell0 = -1;
    if (!s.known) return it;
    // readable positions of the segment: inside the clip and below the extent
    int64_t lo = s.clip_lo, hi = s.clip_hi;
    if (s.start + hi > s.ext) hi = s.ext - s.start;
    if (s.start + lo < 0) lo = -s.start;
    lo -= a; hi -= a;
    if (lo < 0) lo = 0;
    if (hi > n) hi = n;
    if (hi <= lo) return it;
    it.lo = (int32_t)lo; it.hi = (int32_t)hi;
    it.cell0 = s.cell_base + s.start + a;    // (may lie below the strand's first cell: only [lo, hi) is read)
    return it;
}

// ---- how the gather kernel serves an item: PAIRS of output elements that share one 16-byte aligned slot of the
// output (elements 2j and 2j + 1 of an 8-byte array whose base is 16-byte aligned), one 16-byte store each.  Which
// positions pair depends on the parity of the item's first output element and on the direction:
//   head   1: position 0 sits alone in its slot (its partner lies outside the item): one 8-byte store
//   pairs  pair p (0 <= p < pairs) holds positions i0 = head + 2 p and i0 + 1; the lower element of its slot is
//          out_off + i0 for step +1 (it takes position i0) and out_off - i0 - 1 for step -1 (it takes position i0 + 1)
//   tail   1: position len - 1 sits alone
// Cells are read 4 bytes at a time at even cell indices only: the cell block is 4-byte aligned and holds an even number
// of cells (two strands per contig), so the 4 bytes around a readable cell lie inside the block.
struct PairCut {
    int32_t head, pairs, tail;
};
PCDENSE_HD inline PairCut pair_cut(int64_t out_off, int32_t step, int32_t len) {
    PairCut c;
    c.head = (int32_t)((step > 0 ? out_off : out_off + 1) & 1);
    if (c.head > len) c.head = len;
    c.pairs = (len - c.head) >> 1;
    c.tail = (len - c.head) & 1;
    return c;
}
// the lower output element of pair p's slot
PCDENSE_HD inline int64_t pair_slot(int64_t out_off, int32_t step, const PairCut &c, int32_t p) {
    const int64_t i0 = c.head + 2 * (int64_t)p;
    return step > 0 ? out_off + i0 : out_off - i0 - 1;
}

// A workgroup of the gather serves a BATCH of kBatch consecutive items of the plan's item list (plan order; the last
// batch may be short): every descriptor and every cell of the batch is requested before the first store.  The product
// serves ONE item per workgroup: batches of 2, 4 and 8 were measured and are slower (profiles/dense_gather/NOTES.md);
// -DPC_DENSE_BATCH=<B> builds them for scripts/exp_dense_sections.py.
#ifndef PC_DENSE_BATCH
#define PC_DENSE_BATCH 1
#endif
constexpr int kBatch = PC_DENSE_BATCH;
PCDENSE_HD inline int64_t batches_of(int64_t n_items) { return (n_items + kBatch - 1) / kBatch; }

} // namespace pcdense
