// track_kernels.hip.h -- count tracks as text on the GPU (track_host.h says what a line means; track_decoder.hip.h drives
// the kernels).  The text lies in HBM as it is on disk; the line starts are those of sam_kernels.hip.h.
//   import:  k_track_classify       one lane per line: class and token count; the line is a state line candidate
//            k_track_states         a bedGraph line starts a state unless the header / bedGraph line before it is a
//                                   bedGraph line of the same name; the state lines are listed for the host
//            k_track_fields         one lane per line: governing record by bisection, start / stop / value; escaped lines,
//                                   the lowest defect
//            k_track_patch          the host's numbers of the escaped lines
//            k_track_keys           growth lines, per-contig furthest end and first yielding line; (contig, start) sort
//                                   keys of the lines that write cells
//            k_track_clusters       lines that overlap the running maximum end join the cluster of the line before
//            k_track_fill_short / k_track_fill    singleton clusters, in parallel
//            k_track_fill_ordered   clusters of several lines, every cell in file order
//   query:   k_track_gather         k_dense_gather over float64 cells
//            k_track_sum_partial / k_track_sum_final   fixed-tree sum
//   revision 16:
//   write:   k_track_set            the gather the other way: a fill, or a strided copy from an uploaded vector
//   combine: k_track_op             one lane per cell of the concatenated result, operands per slot with a length each
//            k_track_equal          the same walk as a reduction
//            k_track_nz_flags / k_track_nz_select   nonzero: flags, exclusive sum (caller), select
//   export:  k_export_slot_partial / k_export_slot_final   per slot: fixed-tree sum, first and last non-zero
//            k_export_flags / k_export_select / k_export_bases   run heads, the run table, runs in front of a contig
//            k_export_classify      the values that are not plain, listed for the host's repr
//            k_export_lengths / k_export_format   a byte length per line; every line's bytes at its offset
//   revision 17 (a counted plan's output, int64 or float64, as the source):
//   write:   k_track_set_counts     k_track_set reading the plan's output in HBM
//   export:  k_counts_flags         run heads of BAMGenomeArray's text: value changes and window borders; non-zero cells
//            k_counts_keep          bedGraph: the runs whose value is > 0 are the lines (flags for a second select)
//            k_counts_classify / k_counts_lengths / k_counts_format   as k_export_*, over the line -> run -> range
//                                   mapping of track_table.h (count_line_of)
// Every byte access lies in [0, text_len); every cell access inside the strand's extent.
// Part of the one translation unit of plastid_counts.hip (behind sam_kernels.hip.h and dense_kernels.hip.h).
#pragma once
#include "track_table.h"

namespace pctrack {

constexpr int kShortLen = 32;                  // lines up to this many positions are filled by one lane
constexpr unsigned long long kNoDefect = ~0ull;

// line i is [line_start[i], line_start[i + 1] - 1), clamped to the text
__device__ __forceinline__ void line_bounds(const uint64_t *__restrict__ line_start, uint64_t text_len, int64_t i, uint64_t &b, uint64_t &e) {
    b = line_start[i]; e = line_start[i + 1] - 1;
    if (e > text_len) e = text_len;
    if (b > e) b = e;
}
// (last_at_or_below, ex_range_of, ex_range_of_line: track_table.h -- the host's tests walk them too)
// flags in front of position p (p == n: all of them), from their exclusive sum idx
__device__ __forceinline__ int64_t flags_before(const uint32_t *__restrict__ flags, const uint32_t *__restrict__ idx, int64_t n, int64_t p) {
    return p < n ? (int64_t)idx[p] : (int64_t)idx[n - 1] + (int64_t)flags[n - 1];
}

// cls[i]: class | token count << 4.  sig[i]: i for a header or bedGraph line, -1 otherwise (max-scanned by the caller);
// is_data[i]: 1 for a data line (summed by the caller).
__global__ __launch_bounds__(256) void k_track_classify(const uint8_t *__restrict__ text, uint64_t text_len, const uint64_t *__restrict__ line_start, int64_t nline,
                                                        uint8_t *__restrict__ cls, int32_t *__restrict__ sig, uint32_t *__restrict__ is_data) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nline) return;
    uint64_t b, e;
    line_bounds(line_start, text_len, i, b, e);
    const LineClass c = classify_line(text + b, text + e);
    cls[i] = (uint8_t)(c.cls | (c.ntok << 4));
    sig[i] = (c.cls == kHeader || c.cls == kBed) ? (int32_t)i : -1;
    is_data[i] = c.cls == kData ? 1u : 0u;
}

// prev_sig[i]: the last header or bedGraph line in front of line i (-1: none).  State lines are appended to `state_lines`
// in any order (the host sorts them); *n_state counts them.
__global__ __launch_bounds__(256) void k_track_states(const uint8_t *__restrict__ text, uint64_t text_len, const uint64_t *__restrict__ line_start, int64_t nline,
                                                      const uint8_t *__restrict__ cls, const int32_t *__restrict__ prev_sig,
                                                      uint32_t *__restrict__ state_lines, uint32_t *__restrict__ n_state) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nline) return;
    const int c = cls[i] & 15;
    bool state = c == kHeader;
    if (c == kBed) {
        const int32_t j = prev_sig[i];
        state = true;
        if (j >= 0 && (cls[j] & 15) == kBed) {
            uint64_t b, e, pb, pe;
            line_bounds(line_start, text_len, i, b, e);
            line_bounds(line_start, text_len, j, pb, pe);
            state = !tok_equal(next_token(text + b, text + e), next_token(text + pb, text + pe));
        }
    }
    if (state) state_lines[atomicAdd(n_state, 1u)] = (uint32_t)i;
}

// What the import keeps of every line (24 bytes).
struct LineRec {
    int64_t start, stop;
    double value;
};

// counters of one import, in HBM
struct TrackCounters {
    unsigned long long first_err;     // (line << 8 | code) of the lowest defect, kNoDefect: none
    uint32_t n_state, n_yield, n_escaped, n_growth, n_long, n_multi, n_valid, pad;
};

// One lane per line.  contig_of[i]: the contig of a yielding line without a defect, -1 otherwise.  A line all of whose
// tokens are plain is checked here (check_fields); an escaped line is listed, and converted and checked by the host.
__global__ __launch_bounds__(256) void k_track_fields(const uint8_t *__restrict__ text, uint64_t text_len, const uint64_t *__restrict__ line_start, int64_t nline,
                                                      const uint8_t *__restrict__ cls, const uint32_t *__restrict__ data_index,
                                                      const StateRec *__restrict__ recs, int64_t nrec,
                                                      LineRec *__restrict__ out, int32_t *__restrict__ contig_of, uint32_t *__restrict__ escaped_lines,
                                                      TrackCounters *__restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nline) return;
    const int c = cls[i] & 15;
    contig_of[i] = -1;
    if (c != kBed && c != kData) return;
    const int64_t g = governing(recs, nrec, i);
    if (g < 0) return;
    uint64_t b, e;
    line_bounds(line_start, text_len, i, b, e);
    const LineClass lc = classify_line(text + b, text + e);
    const StateRec r = recs[g];
    const LineOut o = line_fields<FastOnly>(lc, &r, (int64_t)data_index[i]);
    if (!o.yields) return;
    atomicAdd(&cnt->n_yield, 1u);
    int err = o.err;
    if (err == kTrkOk && !o.escaped) err = check_fields(o);
    if (err != kTrkOk) { atomicMin(&cnt->first_err, ((unsigned long long)i << 8) | (unsigned long long)err); return; }
    if (o.escaped) { escaped_lines[atomicAdd(&cnt->n_escaped, 1u)] = (uint32_t)i; return; }
    LineRec lr;
    lr.start = o.start; lr.stop = o.stop; lr.value = o.value;
    out[i] = lr;
    contig_of[i] = o.contig;
}

// the host's numbers of the escaped lines
__global__ __launch_bounds__(256) void k_track_patch(const uint32_t *__restrict__ lines, const LineRec *__restrict__ vals, const int32_t *__restrict__ contigs,
                                                     uint32_t n, LineRec *__restrict__ out, int32_t *__restrict__ contig_of) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < n) { out[lines[k]] = vals[k]; contig_of[lines[k]] = contigs[k]; }
}

// One lane per line, on the final numbers.  len0[c]: the length contig c has before this call; a line whose end reaches it
// goes to growth_lines.  furthest[c]: max end of the lines that write cells; first_line[c]: min line that yields on c.
// key: the sort key of a line that writes cells (contig << 41 | start; kNoKey for every other line).
constexpr uint64_t kNoKey = ~0ull;
__global__ __launch_bounds__(256) void k_track_keys(const LineRec *__restrict__ recs, const int32_t *__restrict__ contig_of, const uint8_t *__restrict__ cls,
                                                    int64_t nline, const int64_t *__restrict__ len0, int ncontig,
                                                    unsigned long long *__restrict__ furthest, uint32_t *__restrict__ first_line,
                                                    uint32_t *__restrict__ growth_lines, uint64_t *__restrict__ key, uint32_t *__restrict__ idx,
                                                    TrackCounters *__restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    // (every lane of the wave stays to the end: the wave folds its lines before it touches the per-contig words)
    bool yields = false, writes = false;
    int32_t t = -1;
    LineRec r;
    r.start = 0; r.stop = 0; r.value = 0.0;
    if (i < nline) {
        const int c = cls[i] & 15;
        uint64_t k = kNoKey;
        if (c == kBed || c == kData) {
            t = contig_of[i];
            yields = t >= 0 && t < ncontig;
            if (yields) {
                r = recs[i];
                if (r.stop >= len0[t]) growth_lines[atomicAdd(&cnt->n_growth, 1u)] = (uint32_t)i;
                writes = r.stop > r.start;                      // an empty interval writes nothing
                if (writes) { atomicAdd(&cnt->n_valid, 1u); k = ((uint64_t)t << 41) | (uint64_t)r.start; }
            }
        }
        key[i] = k;
        idx[i] = (uint32_t)i;
    }
    // the lines of a wave are neighbours in the file and nearly always on one contig: one atomic pair per wave then
    const unsigned long long m = __ballot(yields);
    if (m == 0ull) return;
    const int leader = __ffsll((long long)m) - 1;
    const int32_t t_lead = __shfl(t, leader, 64);
    if (__ballot(yields && t != t_lead) == 0ull) {
        uint32_t mn = yields ? (uint32_t)i : kNoLine;
        unsigned long long mx = writes ? (unsigned long long)r.stop : 0ull;
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t a = __shfl_xor(mn, o, 64);
            const unsigned long long b = __shfl_xor(mx, o, 64);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
        }
        if ((int)(threadIdx.x & 63) == leader) {
            atomicMin(&first_line[t_lead], mn);
            if (mx) atomicMax(&furthest[t_lead], mx);
        }
    } else if (yields) {
        atomicMin(&first_line[t], (uint32_t)i);
        if (writes) atomicMax(&furthest[t], (unsigned long long)r.stop);
    }
}

// Sorted order (key, idx), nv lines with a key.  end_key[k] = contig << 41 | stop, max-scanned exclusively by the caller.
__global__ __launch_bounds__(256) void k_track_end_keys(const uint64_t *__restrict__ key, const uint32_t *__restrict__ idx, const LineRec *__restrict__ recs,
                                                        int64_t nv, uint64_t *__restrict__ end_key) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nv) return;
    end_key[k] = (key[k] & ~(((uint64_t)1 << 41) - 1)) | (uint64_t)recs[idx[k]].stop;
}

// head[k] = k when sorted line k starts a cluster -- it does not begin below the furthest end of the lines in front of it
// on its contig -- and 0 otherwise (max-scanned inclusively by the caller: the cluster's first line)
__global__ __launch_bounds__(256) void k_track_clusters(const uint64_t *__restrict__ key, const uint64_t *__restrict__ prev_end, int64_t nv,
                                                        int32_t *__restrict__ head) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nv) return;
    const uint64_t mask = ((uint64_t)1 << 41) - 1;
    bool overlaps = false;
    if (k > 0) {
        const uint64_t p = prev_end[k];
        overlaps = (p >> 41) == (key[k] >> 41) && (key[k] & mask) < (p & mask);
    }
    head[k] = overlaps ? 0 : (int32_t)k;
}

// Singleton clusters: short lines are filled here, long ones listed; lines of larger clusters are listed as
// (cluster << 32 | line) keys for the ordered pass.  cells: the strand's cells of every contig, cell_off[c] its first.
// kAssign (the three fill kernels; revision 18, the items of a bigWig file): a line WRITES its value instead of adding it --
// a singleton line as it is, and in a cluster every cell takes the value of the last line in file order that covers it
// (Kent's readers assign in file order: bwgQuery.c:155-285).  kAssign = false is the add of revisions 15 - 17.
template <bool kAssign>
__global__ __launch_bounds__(256) void k_track_fill_short(const uint32_t *__restrict__ idx, const int32_t *__restrict__ head, int64_t nv,
                                                          const LineRec *__restrict__ recs, const int32_t *__restrict__ contig_of,
                                                          const int64_t *__restrict__ cell_off, double *__restrict__ cells,
                                                          uint32_t *__restrict__ long_lines, uint64_t *__restrict__ multi_keys, TrackCounters *__restrict__ cnt) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nv) return;
    const uint32_t i = idx[k];
    const bool single = head[k] == (int32_t)k && (k + 1 == nv || head[k + 1] == (int32_t)(k + 1));
    if (!single) { multi_keys[atomicAdd(&cnt->n_multi, 1u)] = ((uint64_t)(uint32_t)head[k] << 32) | (uint64_t)i; return; }
    const LineRec r = recs[i];
    const int64_t n = r.stop - r.start;
    if (n > kShortLen) { long_lines[atomicAdd(&cnt->n_long, 1u)] = i; return; }
    double *dst = cells + cell_off[contig_of[i]] + r.start;
    for (int64_t p = 0; p < n; ++p) dst[p] = kAssign ? r.value : dst[p] + r.value;
}

// one workgroup per long singleton line, item by item (2 048 positions: 256 lanes x 8)
template <bool kAssign>
__global__ __launch_bounds__(256) void k_track_fill(const uint32_t *__restrict__ long_lines, const LineRec *__restrict__ recs, const int32_t *__restrict__ contig_of,
                                                    const int64_t *__restrict__ cell_off, double *__restrict__ cells) {
    const uint32_t i = long_lines[blockIdx.x];
    const LineRec r = recs[i];
    double *dst = cells + cell_off[contig_of[i]] + r.start;
    const int64_t n = r.stop - r.start;
    for (int64_t a = 0; a < n; a += pcdense::kItemLen)
#pragma unroll
        for (int k = 0; k < pcdense::kPerLane; ++k) {
            const int64_t p = a + threadIdx.x + k * 256;
            if (p < n) dst[p] = kAssign ? r.value : dst[p] + r.value;
        }
}

// Clusters of several lines.  multi_keys: (cluster << 32 | line), sorted, so that a cluster's lines stand together in
// file order.  One workgroup per entry; the one at a cluster's first entry serves the cluster: every lane takes cells of
// the cluster's extent and adds the lines that cover the cell in file order.  Quadratic in the cluster (cells x lines),
// exact for any overlap.
template <bool kAssign>
__global__ __launch_bounds__(256) void k_track_fill_ordered(const uint64_t *__restrict__ multi_keys, uint32_t nm, const LineRec *__restrict__ recs,
                                                            const int32_t *__restrict__ contig_of, const int64_t *__restrict__ cell_off,
                                                            double *__restrict__ cells) {
    const uint32_t k0 = blockIdx.x;
    const uint64_t cluster = multi_keys[k0] >> 32;
    if (k0 > 0 && (multi_keys[k0 - 1] >> 32) == cluster) return;
    uint32_t k1 = k0;
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    while (k1 < nm && (multi_keys[k1] >> 32) == cluster) {
        const LineRec r = recs[(uint32_t)multi_keys[k1]];
        lo = r.start < lo ? r.start : lo;
        hi = r.stop > hi ? r.stop : hi;
        ++k1;
    }
    double *base = cells + cell_off[contig_of[(uint32_t)multi_keys[k0]]];
    for (int64_t p = lo + threadIdx.x; p < hi; p += 256) {
        double v = base[p];
        for (uint32_t k = k0; k < k1; ++k) {
            const LineRec r = recs[(uint32_t)multi_keys[k]];
            if (p >= r.start && p < r.stop) v = kAssign ? r.value : v + r.value;
        }
        base[p] = v;
    }
}

// k_dense_gather over float64 cells: one workgroup per item.  normalize: 1e6 * v / sum (the reference's order for this
// class, genome_array.py:1528).
__global__ __launch_bounds__(pcdense::kGatherWG) void k_track_gather(const pcdense::Item *__restrict__ items, const double *__restrict__ cells,
                                                                      double *__restrict__ out, int normalize, double sum) {
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
        if (i < it.len) dst[(int64_t)it.step * i] = normalize ? 1e6 * v[k] / sum : v[k];
    }
}

// Fixed-tree sum: block b adds cells [b * kSumTile, (b + 1) * kSumTile) -- every lane its strided cells in order, then the
// lanes by halving -- and one workgroup adds the partials the same way.  The order depends on n alone.
constexpr int kSumTile = 256 * 64;
__device__ __forceinline__ double block_tree_sum(double v) {
    __shared__ double s[256];
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
__global__ __launch_bounds__(256) void k_track_sum_partial(const double *__restrict__ cells, int64_t n, double *__restrict__ partial) {
    const int64_t base = (int64_t)blockIdx.x * kSumTile;
    double v = 0.0;
    for (int k = 0; k < kSumTile / 256; ++k) {
        const int64_t p = base + (int64_t)k * 256 + threadIdx.x;
        if (p < n) v = v + cells[p];
    }
    const double r = block_tree_sum(v);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}
__global__ __launch_bounds__(256) void k_track_sum_final(const double *__restrict__ partial, int64_t n, double *__restrict__ out) {
    double v = 0.0;
    for (int64_t p = threadIdx.x; p < n; p += 256) v = v + partial[p];
    const double r = block_tree_sum(v);
    if (threadIdx.x == 0) *out = r;
}

// ---------------------------------------------------------------- writes (pc_track_set)

// k_track_gather the other way: position i of the item, lo <= i < hi, takes values[out_off + step * i] (values null: the
// scalar).  One launch serves every segment of a chain.
__global__ __launch_bounds__(pcdense::kGatherWG) void k_track_set(const pcdense::Item *__restrict__ items, double *__restrict__ cells,
                                                                   const double *__restrict__ values, double scalar) {
    const pcdense::Item it = items[blockIdx.x];
    const int t = (int)threadIdx.x;
#pragma unroll
    for (int k = 0; k < pcdense::kPerLane; ++k) {
        const int i = t + k * pcdense::kGatherWG;
        if (i >= it.lo && i < it.hi) cells[it.cell0 + i] = values ? values[it.out_off + (int64_t)it.step * i] : scalar;
    }
}

// ---------------------------------------------------------------- arithmetic and equality (pc_track_combine, pc_track_equal)

// the OpSlot (track_table.h) of output cell i: the last one with out0 <= i (empty slots share their out0 with the slot behind them)
__device__ __forceinline__ int op_slot_of(const OpSlot *__restrict__ slots, int nslot, int64_t i) {
    return last_at_or_below(nslot, i, [slots](int k) { return slots[k].out0; });
}

enum { kOpAdd = 0, kOpSub = 1, kOpMul = 2 };

// out[i] = a op b over the concatenated output cells; b_cells null: the scalar
__global__ __launch_bounds__(256) void k_track_op(const OpSlot *__restrict__ slots, int nslot, int64_t total, const double *__restrict__ a_cells,
                                                  const double *__restrict__ b_cells, int has_b, double scalar, int op, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const OpSlot s = slots[op_slot_of(slots, nslot, i)];
    const int64_t j = i - s.out0;
    const double va = (s.a0 >= 0 && j < s.an) ? a_cells[s.a0 + j] : 0.0;
    const double vb = has_b ? ((s.b0 >= 0 && j < s.bn) ? b_cells[s.b0 + j] : 0.0) : scalar;
    out[i] = op == kOpAdd ? va + vb : op == kOpSub ? va - vb : va * vb;
}

// *differs |= 1 when some position is non-zero in one operand only, or non-zero in both and not within tol
__global__ __launch_bounds__(256) void k_track_equal(const OpSlot *__restrict__ slots, int nslot, int64_t total, const double *__restrict__ a_cells,
                                                     const double *__restrict__ b_cells, double tol, uint32_t *__restrict__ differs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const OpSlot s = slots[op_slot_of(slots, nslot, i)];
    const int64_t j = i - s.out0;
    const double va = (s.a0 >= 0 && j < s.an) ? a_cells[s.a0 + j] : 0.0;
    const double vb = (s.b0 >= 0 && j < s.bn) ? b_cells[s.b0 + j] : 0.0;
    const bool na = va != 0.0, nb = vb != 0.0;
    if (na != nb || (na && !(fabs(va - vb) <= tol))) atomicOr(differs, 1u);
}

// ---------------------------------------------------------------- nonzero (pc_track_nonzero)

// NaN is non-zero, -0.0 is not
__global__ __launch_bounds__(256) void k_track_nz_flags(const double *__restrict__ cells, int64_t n, uint32_t *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flags[i] = cells[i] != 0.0 ? 1u : 0u;
}
// out[idx[i]] = position of cell i on its slot; slot_start: first cell of every slot, ascending
__global__ __launch_bounds__(256) void k_track_nz_select(const uint32_t *__restrict__ flags, const uint32_t *__restrict__ idx, int64_t n,
                                                         const int64_t *__restrict__ slot_start, int nslot, int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flags[i]) return;
    out[idx[i]] = i - slot_start[last_at_or_below(nslot, i, [slot_start](int k) { return slot_start[k]; })];
}
// out[k] = flags in front of cell at[k] (at[k] == n: all of them), from the exclusive sum idx
__global__ __launch_bounds__(256) void k_track_pick(const uint32_t *__restrict__ flags, const uint32_t *__restrict__ idx, int64_t n,
                                                    const int64_t *__restrict__ at, int m, int64_t *__restrict__ out) {
    const int k = (int)(blockIdx.x * 256u + threadIdx.x);
    if (k >= m) return;
    out[k] = flags_before(flags, idx, n, at[k]);
}

// ---------------------------------------------------------------- export (pc_track_export)

constexpr int kExportTile = 2048;        // T: cells one workgroup covers in the run-head kernel (256 lanes x 8)
constexpr int kFormatRuns = 256;         // R: lines one workgroup formats, one per lane
constexpr uint32_t kNotListed = 0xffffffffu;

// Per exported slot (SlotCells -> SlotStat, track_table.h): the fixed-tree sum is k_track_sum_partial's tree over the slot's
// own cells.
// grid (max tiles, slots): block (x, y) adds tile x of slot y
__global__ __launch_bounds__(256) void k_export_slot_partial(const SlotCells *__restrict__ slots, const double *__restrict__ cells, int64_t max_tiles,
                                                             double *__restrict__ partial, SlotStat *__restrict__ stat) {
    const SlotCells s = slots[blockIdx.y];
    const int64_t base = (int64_t)blockIdx.x * kSumTile;
    if (base >= s.n) return;                               // (uniform over the workgroup)
    double v = 0.0;
    unsigned long long first = ~0ull, last1 = 0ull;
    for (int k = 0; k < kSumTile / 256; ++k) {
        const int64_t p = base + (int64_t)k * 256 + threadIdx.x;
        if (p < s.n) {
            const double c = cells[s.cell0 + p];
            v = v + c;
            if (c != 0.0) { if (first == ~0ull) first = (unsigned long long)p; last1 = (unsigned long long)p + 1ull; }
        }
    }
    const double r = block_tree_sum(v);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * max_tiles + blockIdx.x] = r;
    if (first != ~0ull) { atomicMin(&stat[blockIdx.y].first, first); atomicMax(&stat[blockIdx.y].last1, last1); }
}
// one workgroup per slot adds the slot's partials
__global__ __launch_bounds__(256) void k_export_slot_final(const SlotCells *__restrict__ slots, const double *__restrict__ partial, int64_t max_tiles,
                                                           SlotStat *__restrict__ stat) {
    const int64_t nt = (slots[blockIdx.x].n + kSumTile - 1) / kSumTile;
    double v = 0.0;
    for (int64_t p = threadIdx.x; p < nt; p += 256) v = v + partial[(int64_t)blockIdx.x * max_tiles + p];
    const double r = block_tree_sum(v);
    if (threadIdx.x == 0) stat[blockIdx.x].sum = r;
}

// kind 0 (bedGraph): a cell heads a run when it is the contig's first export cell or differs (!=) from the cell in front
// of it -- read from HBM, so a run that began in an earlier tile needs nothing more; kind 1: when it is non-zero
__global__ __launch_bounds__(256) void k_export_flags(int kind, const ExRange *__restrict__ ranges, int K, int64_t E, const double *__restrict__ cells,
                                                      uint32_t *__restrict__ flags) {
#pragma unroll
    for (int k = 0; k < kExportTile / 256; ++k) {
        const int64_t e = (int64_t)blockIdx.x * kExportTile + k * 256 + threadIdx.x;
        if (e >= E) continue;
        const ExRange r = ranges[ex_range_of(ranges, K, e)];
        const int64_t j = e - r.e0;
        const double v = cells[r.cell0 + j];
        bool f;
        if (kind == 0) f = j == 0 || v != cells[r.cell0 + j - 1];
        else f = v != 0.0;
        flags[e] = f ? 1u : 0u;
    }
}
__global__ __launch_bounds__(256) void k_export_select(const uint32_t *__restrict__ flags, const uint32_t *__restrict__ idx, int64_t E, uint32_t *__restrict__ run_e) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < E && flags[e]) run_e[idx[e]] = (uint32_t)e;
}
// ranges[k].run_base for k = 0 .. K (entry K: the sentinel, all runs)
__global__ __launch_bounds__(256) void k_export_bases(const uint32_t *__restrict__ flags, const uint32_t *__restrict__ idx, int64_t E, ExRange *__restrict__ ranges, int K) {
    const int k = (int)(blockIdx.x * 256u + threadIdx.x);
    if (k > K) return;
    ranges[k].run_base = flags_before(flags, idx, E, ranges[k].e0);
}
// The values of the runs that are not plain are listed for the host (any order); listed_slot[r]: the run's place in the
// list, kNotListed otherwise.
__global__ __launch_bounds__(256) void k_export_classify(const ExRange *__restrict__ ranges, int K, const uint32_t *__restrict__ run_e, int64_t R,
                                                         const double *__restrict__ cells, uint32_t *__restrict__ listed_slot, double *__restrict__ listed_val,
                                                         uint32_t *__restrict__ n_listed) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const int64_t e = (int64_t)run_e[r];
    const ExRange g = ranges[ex_range_of(ranges, K, e)];
    const double v = cells[g.cell0 + (e - g.e0)];
    uint32_t s = kNotListed;
    if (value_class(v) == kValListed) { s = atomicAdd(n_listed, 1u); listed_val[s] = v; }
    listed_slot[r] = s;
}

struct ExportView {
    int kind;
    const ExRange *ranges; int K;
    const uint32_t *run_e;
    const double *cells;
    const uint8_t *names;
    const uint32_t *listed_slot;
    const uint8_t *strs, *lens;        // text (kReprMax bytes apart) and length of every listed value
};
// line L of the text into the sink: the length kernel counts what the format kernel stores
template <typename Sink> __device__ __forceinline__ void export_line(Sink &s, const ExportView &x, int64_t L) {
    const int k = ex_range_of_line(x.ranges, x.K, L);
    const ExRange g = x.ranges[k];
    const uint8_t *name = x.names + g.name_off;
    if (L == g.run_base + k) {
        if (x.kind == 0) put_bed_lead(s, name, (int64_t)g.name_len, g.pos0); else put_var_header(s, name, (int64_t)g.name_len);
        return;
    }
    const int64_t run = L - k - 1;
    const int64_t j = (int64_t)x.run_e[run] - g.e0;
    const double v = x.cells[g.cell0 + j];
    const uint32_t ls = x.listed_slot[run];
    const uint8_t *vt = ls != kNotListed ? x.strs + (int64_t)kReprMax * ls : nullptr;
    const int vl = ls != kNotListed ? (int)x.lens[ls] : 0;
    if (x.kind == 0) {
        const int64_t end = run + 1 < x.ranges[k + 1].run_base ? (int64_t)x.run_e[run + 1] - g.e0 : g.n;
        put_bed_line(s, name, (int64_t)g.name_len, g.pos0 + j, g.pos0 + end, v, vt, vl);
    } else put_var_line(s, g.pos0 + j, v, vt, vl);
}
__global__ __launch_bounds__(kFormatRuns) void k_export_lengths(ExportView x, int64_t nlines, int64_t *__restrict__ len) {
    const int64_t L = (int64_t)blockIdx.x * kFormatRuns + threadIdx.x;
    if (L >= nlines) return;
    CountSink s;
    s.n = 0;
    export_line(s, x, L);
    len[L] = s.n;
}
// every line's bytes at its offset; text has off[nlines - 1] + len[nlines - 1] bytes
__global__ __launch_bounds__(kFormatRuns) void k_export_format(ExportView x, int64_t nlines, const int64_t *__restrict__ off, uint8_t *__restrict__ text) {
    const int64_t L = (int64_t)blockIdx.x * kFormatRuns + threadIdx.x;
    if (L >= nlines) return;
    WriteSink s{text + off[L]};
    export_line(s, x, L);
}

// ---------------------------------------------------------------- writes from a counted plan (pc_track_set_counts)

// k_track_set reading HBM: position i of the item takes (double) of output element out_off + step * i of the plan
template <typename T>
__global__ __launch_bounds__(pcdense::kGatherWG) void k_track_set_counts(const pcdense::Item *__restrict__ items, double *__restrict__ cells, const T *__restrict__ out) {
    const pcdense::Item it = items[blockIdx.x];
    const int t = (int)threadIdx.x;
#pragma unroll
    for (int k = 0; k < pcdense::kPerLane; ++k) {
        const int i = t + k * pcdense::kGatherWG;
        if (i >= it.lo && i < it.hi) cells[it.cell0 + i] = (double)out[it.out_off + (int64_t)it.step * i];
    }
}

// ---------------------------------------------------------------- export of a counted plan (pc_counts_export)
// The ranges are those of count_ranges (track_table.h): export element e of range r is output element cell0 + (e - e0)
// of the plan, genomic position e - e0 of the range's contig.  T: the plan's output dtype, int64_t or double.

// run heads by count_is_head (track_table.h); the element in front is read from HBM: no carry across tiles
template <typename T>
__global__ __launch_bounds__(256) void k_counts_flags(int kind, uint32_t period, const ExRange *__restrict__ ranges, int K, int64_t E, const T *__restrict__ out,
                                                      uint32_t *__restrict__ flags) {
#pragma unroll
    for (int k = 0; k < kExportTile / 256; ++k) {
        const int64_t e = (int64_t)blockIdx.x * kExportTile + k * 256 + threadIdx.x;
        if (e >= E) continue;
        const ExRange r = ranges[ex_range_of(ranges, K, e)];
        flags[e] = count_is_head(kind, period, out + r.cell0, e - r.e0) ? 1u : 0u;
    }
}
// bedGraph: run r is a line by count_is_line (its value is > 0)
template <typename T>
__global__ __launch_bounds__(256) void k_counts_keep(const ExRange *__restrict__ ranges, int K, const uint32_t *__restrict__ run_e, int64_t R,
                                                     const T *__restrict__ out, uint32_t *__restrict__ keep) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const int64_t e = (int64_t)run_e[r];
    const ExRange g = ranges[ex_range_of(ranges, K, e)];
    keep[r] = count_is_line(out[g.cell0 + (e - g.e0)]) ? 1u : 0u;
}

template <typename T> struct CountView {
    int kind;
    const ExRange *ranges; int K;
    const uint32_t *run_e, *line_run;
    const T *out;
    const uint8_t *names;
    const uint32_t *listed_slot;       // per classified value (count_line_of: value_at); null: none is listed (int64)
    const uint8_t *strs, *lens;
};
// float64: the values of the lines that are not plain, listed for the host (any order); nvalues: lines (bedGraph) or
// runs (variableStep) -- count_line_of's value_at
__global__ __launch_bounds__(256) void k_counts_classify(CountView<double> x, int64_t nvalues, uint32_t *__restrict__ listed_slot, double *__restrict__ listed_val,
                                                         uint32_t *__restrict__ n_listed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvalues) return;
    int64_t e;
    if (x.kind == 0) e = (int64_t)x.run_e[x.line_run[i]]; else e = (int64_t)x.run_e[i];
    const ExRange g = x.ranges[ex_range_of(x.ranges, x.K, e)];
    const double v = x.out[g.cell0 + (e - g.e0)];
    uint32_t s = kNotListed;
    if (count_listed(v)) { s = atomicAdd(n_listed, 1u); listed_val[s] = v; }
    listed_slot[i] = s;
}
// line L of the text into the sink
template <typename Sink, typename T> __device__ __forceinline__ void count_line(Sink &s, const CountView<T> &x, int64_t L) {
    const CountLine c = count_line_of(x.kind, x.ranges, x.K, x.run_e, x.line_run, L);
    const ExRange g = x.ranges[c.k];
    const uint8_t *name = x.names + g.name_off;
    if (c.header) { put_var_header(s, name, (int64_t)g.name_len); return; }
    const T v = x.out[g.cell0 + c.j];
    const uint32_t ls = x.listed_slot ? x.listed_slot[c.value_at] : kNotListed;
    const uint8_t *vt = ls != kNotListed ? x.strs + (int64_t)kReprMax * ls : nullptr;
    const int vl = ls != kNotListed ? (int)x.lens[ls] : 0;
    if (x.kind == 0) put_count_bed_line(s, name, (int64_t)g.name_len, c.j, c.end, v, vt, vl);
    else put_count_var_line(s, c.j, v, vt, vl);
}
template <typename T>
__global__ __launch_bounds__(kFormatRuns) void k_counts_lengths(CountView<T> x, int64_t nlines, int64_t *__restrict__ len) {
    const int64_t L = (int64_t)blockIdx.x * kFormatRuns + threadIdx.x;
    if (L >= nlines) return;
    CountSink s;
    s.n = 0;
    count_line(s, x, L);
    len[L] = s.n;
}
template <typename T>
__global__ __launch_bounds__(kFormatRuns) void k_counts_format(CountView<T> x, int64_t nlines, const int64_t *__restrict__ off, uint8_t *__restrict__ text) {
    const int64_t L = (int64_t)blockIdx.x * kFormatRuns + threadIdx.x;
    if (L >= nlines) return;
    WriteSink s{text + off[L]};
    count_line(s, x, L);
}

} // namespace pctrack
