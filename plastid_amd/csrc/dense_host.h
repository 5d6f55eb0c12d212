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

#include "count_host.h"

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

// What the decision looks at.  The first block is what the plan conditions of the canonical stream look at
// (count_host.h, stream_plan_conditions).
struct PlanIn {
    int nfiles = 0;
    int kind = -1;               // the mapping rule (PC_MAP_*): a point rule -- fiveprime, threeprime or variable
    int rows = 1;
    uint32_t modes = 0;          // strand modes of the plan's windows (bit 0 '+', bit 1 '-', bits 2, 3: unstranded)
    bool has_sums = false;       // some slice is summed (out_step 0)
    bool forbidden = false;      // PC_NO_DENSE, or the plan is the build's own
    int64_t cells = 0;
    int64_t stream_entries = 0;  // of the stream the vector replaces: canonical, else compact, else the records (4 bytes each)
};

inline bool plan_conditions(const PlanIn &p) {
    return !p.forbidden && pccount::stream_plan_conditions(p.nfiles, p.kind, p.rows, p.modes) && !p.has_sums;
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

// ---- the CHUNK form of a plan (k_dense_gather_chunks): the output vector is cut into aligned CHUNKS of kChunk
// elements -- chunk c is out[kChunk c, kChunk c + kChunk) -- and one workgroup writes one chunk, every element of it,
// zeros included: every lane is busy and every wave store covers whole 128-byte lines, whatever the segments are.  A
// SPAN is one segment in one chunk; a chunk's DESCRIPTOR names its spans in output order.  The form needs output
// ranges that do not overlap (the item form writes overlapping ranges in whatever order the workgroups run, which a
// chunk cannot reproduce); plans with overlaps keep the items.  Chunks of 1 024 elements were measured faster than of
// 2 048 (profiles/dense_chunks/NOTES.md); -DPC_DENSE_CHUNK=<elements> builds others for scripts/exp_dense_sections.py.
#ifndef PC_DENSE_CHUNK
#define PC_DENSE_CHUNK 1024
#endif
constexpr int kChunk = PC_DENSE_CHUNK;
constexpr int kRow = 128;                    // output elements of one wave store: 64 lanes x 16 bytes, eight lines
constexpr int kInlineSpans = 7;
static_assert(kChunk % (4 * kRow) == 0 && kChunk / kRow <= 32, "a chunk is whole rows for four waves; its rows are the bits of a word");

// Output elements [a, b) of the chunk (chunk-relative) belong to the span; [ra, rb) of them read a cell -- element e
// reads cell + dir (e - a) -- and the others are zero (clipped, beyond the extent, unknown contig).  ra == rb: none.
// Cells are below 2^32 (dense_for_plan); `cell` of a span whose first elements are not readable may have wrapped,
// and is used modulo 2^32 only.
// The four bounds are packed two to a word, so that a descriptor is read a word at a time.
struct Span {
    uint32_t ab, rr;     // a | b << 16, ra | rb << 16
    uint32_t cell;
    int32_t dir;
    PCDENSE_HD uint32_t a() const { return ab & 0xffffu; }
    PCDENSE_HD uint32_t b() const { return ab >> 16; }
    PCDENSE_HD uint32_t ra() const { return rr & 0xffffu; }
    PCDENSE_HD uint32_t rb() const { return rr >> 16; }
};
static_assert(sizeof(Span) == 16, "Span is 16 bytes in HBM");
// the chunk's first kInlineSpans spans; span s >= kInlineSpans is spans[ovf + s - kInlineSpans] of the plan's span array
// (which holds every span of every chunk in output order: span 0 of the chunk is spans[ovf - kInlineSpans])
struct ChunkDesc {
    uint32_t n, ovf, pad[2];
    Span s[kInlineSpans];
};
static_assert(sizeof(ChunkDesc) == 128, "a descriptor is one line");

PCDENSE_HD inline int64_t chunks_of(int64_t out_elems) { return (out_elems + kChunk - 1) / kChunk; }
// first output element of a segment (its range is [lo, lo + len))
PCDENSE_HD inline int64_t seg_out_lo(int64_t out_off, int32_t step, int64_t len) { return step > 0 ? out_off : out_off - len + 1; }
// spans of a segment: the chunks its output range meets
PCDENSE_HD inline int64_t spans_of(int64_t out_lo, int64_t len) { return len > 0 ? (out_lo + len - 1) / kChunk - out_lo / kChunk + 1 : 0; }
// an upper bound of a plan's spans from what the plan records of itself (every segment: its whole chunks and two ends)
inline bool spans_fit(int64_t nseg, int64_t covered) { return 2 * nseg + covered / kChunk < (int64_t)0xffffffffu; }

// span k (0 <= k < spans_of) of segment s: its part in chunk seg_out_lo / kChunk + k
PCDENSE_HD inline Span cut_span(const SegIn &s, int64_t k) {
    const int64_t lo = seg_out_lo(s.out_off, s.step, s.len), base = (lo / kChunk + k) * kChunk;
    const int64_t a = lo > base ? lo : base, b = lo + s.len < base + kChunk ? lo + s.len : base + kChunk;
    // readable positions of the segment, as cut_item has them
    int64_t plo = 0, phi = 0;
    if (s.known) {
        plo = s.clip_lo; phi = s.clip_hi;
        if (s.start + phi > s.ext) phi = s.ext - s.start;
        if (s.start + plo < 0) plo = -s.start;
        if (plo < 0) plo = 0;
        if (phi > s.len) phi = s.len;
    }
    // ... as output elements: position i is element out_off + step i
    int64_t ra = s.step > 0 ? s.out_off + plo : s.out_off - phi + 1, rb = s.step > 0 ? s.out_off + phi : s.out_off - plo + 1;
    if (ra < a) ra = a;
    if (rb > b) rb = b;
    if (phi <= plo || rb <= ra) ra = rb = a;
    Span sp;
    sp.ab = (uint32_t)(a - base) | (uint32_t)(b - base) << 16;
    sp.rr = (uint32_t)(ra - base) | (uint32_t)(rb - base) << 16;
    sp.dir = s.step > 0 ? 1 : -1;
    const int64_t pos = s.step > 0 ? a - s.out_off : s.out_off - a;     // the position that element a takes
    sp.cell = (uint32_t)(s.cell_base + s.start + pos);
    return sp;
}
PCDENSE_HD inline bool span_reads(const Span &s, uint32_t e) { return e >= s.ra() && e < s.rb(); }
PCDENSE_HD inline uint32_t span_cell(const Span &s, uint32_t e) { return s.cell + (uint32_t)s.dir * (e - s.a()); }
// How the kernel decides per ROW of kRow elements (kernel and CPU test call these).  span_rows: bit r is set where some
// element of row r of the chunk reads a cell through the span.  A row in the words of exactly one span of its chunk
// reads by that span's uniform base: element e reads cell base_cell(span_base(s), s.dir > 0, e) where span_reads says
// so.  Two cells share one 4-byte load where same_word says so (loads are at even cell indices).
PCDENSE_HD inline uint32_t span_rows(const Span &s) {
    const uint32_t ra = s.ra(), rb = s.rb();
    return ra < rb ? (2u << ((rb - 1u) / kRow)) - (1u << (ra / kRow)) : 0u;
}
PCDENSE_HD inline uint32_t span_base(const Span &s) { return s.cell - (uint32_t)s.dir * s.a(); }
PCDENSE_HD inline uint32_t base_cell(uint32_t base, bool up, uint32_t e) { return up ? base + e : base - e; }
PCDENSE_HD inline bool same_word(uint32_t x0, uint32_t x1) { return (x0 | 1u) == (x1 | 1u); }

// The table is built from the segments sorted by seg_out_lo (empty ones last).  Of two neighbours in that order:
// overlap -- any two ranges of a plan overlap only if two neighbours do
PCDENSE_HD inline bool out_overlap(int64_t prev_lo, int64_t prev_len, int64_t lo) { return prev_lo + prev_len > lo; }
// span k of a segment is the first span of its chunk: a later chunk of the segment starts inside the segment; the
// first one unless the segment before ends in that chunk (`prev_end`: where that one ends, -1: there is none)
PCDENSE_HD inline bool first_of_chunk(int64_t lo, int64_t k, int64_t prev_end) {
    return k > 0 || lo % kChunk == 0 || prev_end < 0 || (prev_end - 1) / kChunk < lo / kChunk;
}
// the descriptor of a chunk whose n spans are spans[first .. first + n), in output order
PCDENSE_HD inline ChunkDesc make_desc(const Span *spans, uint32_t first, uint32_t n) {
    ChunkDesc d;
    d.n = n; d.ovf = first + kInlineSpans; d.pad[0] = d.pad[1] = 0;
    for (int i = 0; i < kInlineSpans; ++i) {
        if ((uint32_t)i < n) d.s[i] = spans[first + i];
        else { d.s[i].ab = d.s[i].rr = 0; d.s[i].cell = 0; d.s[i].dir = 1; }
    }
    return d;
}

} // namespace pcdense
