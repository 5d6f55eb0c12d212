// track_table.h -- THE CONTIG TABLE OF A COUNT TRACK: the host arithmetic of a pc_track (track_decoder.hip.h), which decides
// what the reference's chroms() and lengths() say and where every cell lies.  A track keeps its contigs by INTERNAL ID, in
// order of first mention; the PUBLIC order is the declared contigs, then the others by the first line (or write) that
// yields on them.  Cells: one block of float64, slot (id, strand) = id * nstrands + strand holds positions [0, ext) at
// [cell_off, cell_off + ext); an import or a write that reaches further grows the slot (plan_storage / commit).
// Here too: the layouts the entry points hand to the kernels -- gather / set items, the operand slots of a op b and of
// a == b, the ranges of an export, the shares of nonzero() -- as plain structs both sides see.
// Plain C++17 (no HIP), no device pointer: tests/track_table_host_test.cpp runs it on a machine without a GPU.
#pragma once
#include "dense_host.h"
#include "track_host.h"

#include <algorithm>

namespace pctrack {

// One (contig, strand) of a result: cells [out0, out0 + n) of the concatenated output; operand a has cells [a0, a0 + an)
// for its first an positions and zero behind them (a0 < 0: the operand lacks the slot); b alike.
struct OpSlot { int64_t out0, n, a0, an, b0, bn; };
// Per exported slot: its cells; the fixed-tree sum, first non-zero cell and last non-zero cell + 1 (0: none).
struct SlotCells { int64_t cell0, n; };
struct SlotStat { double sum; unsigned long long first, last1; };
// One written contig.  Its export cells are positions [pos0, pos0 + n) -- bedGraph: first to last non-zero; variableStep:
// every stored cell -- and stand at [e0, e0 + n) of the concatenated export domain; cell0: the cell of pos0.  run_base:
// runs (bedGraph) or non-zero cells (variableStep) in front of the contig; its header line is line run_base + k.
struct ExRange {
    int64_t e0, n, cell0, pos0, run_base;
    int32_t name_off, name_len;
};
// contig and end of an imported line that reaches its contig's length
struct GrowthLine { int64_t stop; uint32_t line; int32_t contig; };
constexpr uint32_t kNoLine = 0xffffffffu;

// the storage after a growth: extents, offsets (the running sum) and the cell count
struct StoragePlan { std::vector<int64_t> ext, off; int64_t total = 0; bool grows = false; };
// the contigs an export looks at, in sorted() order of their names (code points: the bytes of UTF-8 sort alike)
struct ExportSlots { std::vector<int32_t> ids; std::vector<SlotCells> cells; };
// the contigs an export writes: their ranges and the sentinel behind them (none: nothing is written), the name bytes
struct ExportRanges { std::vector<ExRange> ranges; std::vector<uint8_t> names; int64_t cells = 0; };
// nonzero(): the slots that hold cells, in the order of their cells; at: their first cells, then ncells; begin / cnt per
// internal slot: its share of the selected indices
struct NzShares { std::vector<int> live; std::vector<int64_t> at, begin, cnt; };

// The words of a caller's segment checks (check_segments).
struct SegWords { const char *who, *step_name, *outside; };
constexpr SegWords kGatherWords{"pc_track_gather", "out_step", "writes outside the output"};
constexpr SegWords kSetWords{"pc_track_set", "val_step", "reads outside the vector"};

// Segments [start, end) whose position i goes with element off + step * i of a vector of `elems`: the first defect as the
// caller words it, empty: none.  coords: the segments must lie in [0, 2^40] (writes).  off null: no vector (a scalar).
inline std::string check_segments(const SegWords &w, int64_t nseg, const int64_t *start, const int64_t *end, const int64_t *off, const int8_t *step,
                                  int64_t elems, bool coords) {
    char msg[160];
    msg[0] = 0;
    for (int64_t s = 0; s < nseg && !msg[0]; ++s) {
        const int64_t len = end[s] - start[s];
        if (coords && (start[s] < 0 || len < 0 || end[s] > kMaxCoord)) snprintf(msg, sizeof(msg), "%s: segment %lld lies outside [0, 2^40]", w.who, (long long)s);
        if (msg[0] || !off || len <= 0) continue;
        if (step[s] != 1 && step[s] != -1) { snprintf(msg, sizeof(msg), "%s: %s of segment %lld is not +1 / -1", w.who, w.step_name, (long long)s); continue; }
        const int64_t a = off[s], b = off[s] + (int64_t)step[s] * (len - 1);
        if (a < 0 || a >= elems || b < 0 || b >= elems) snprintf(msg, sizeof(msg), "%s: segment %lld %s", w.who, (long long)s, w.outside);
    }
    return msg;
}

// the last k of [0, n) with key(k) <= x, -1: none (the keys ascend; equal keys: the last of them)
template <typename Key> PC_TRK_HD inline int last_at_or_below(int n, int64_t x, Key key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key(mid) <= x) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}
// the written contig (ExRange) of export cell e
PC_TRK_HD inline int ex_range_of(const ExRange *r, int K, int64_t e) {
    return last_at_or_below(K, e, [r](int k) { return r[k].e0; });
}
// the contig of line L of a text with one header line per contig: the last k with run_base[k] + k <= L
PC_TRK_HD inline int ex_range_of_line(const ExRange *r, int K, int64_t L) {
    return last_at_or_below(K, L, [r](int k) { return r[k].run_base + k; });
}

// ---------------------------------------------------------------- export of a counted plan (pc_counts_export, revision 17)
// The contigs of one export, in the sorted order of their names, are counted in BATCHES of at most `budget` output
// elements; a contig longer than the budget gets a batch alone.  The run table holds export elements in 32 bits.
constexpr int64_t kCountBudget = (int64_t)1 << 27;            // 1 GiB of 8-byte counts: the cap of one int64 block (dense_host.h)
constexpr int64_t kCountBatchMax = ((int64_t)1 << 32) - 1;

// batch_of[k]: the batch of contig k (ascending from 0); returns the number of batches.  Empty message: fine.
inline int count_batches(int64_t n, const int64_t *len, int64_t budget, int32_t *batch_of, std::string &msg) {
    msg.clear();
    if (budget < 1) { msg = "the batch budget must be at least one element"; return 0; }
    int nb = 0;
    int64_t used = 0;
    bool open = false;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t x = len[k] > 0 ? len[k] : 0;
        if (x > kCountBatchMax) { msg = "contig " + std::to_string((long long)k) + " has more than 2^32 - 1 positions: export elements are indexed with 32 bits"; return 0; }
        if (open && used + x > budget) { ++nb; used = 0; open = false; }
        batch_of[k] = nb;
        used += x; open = true;
    }
    return open ? nb + 1 : nb;
}

// The range table of one batch: range r is len[r] consecutive output elements of the plan from elem_off[r], position j
// of contig names[r] at element j.  In ExRange terms: cell0 the first output element, pos0 0; the sentinel behind them.
inline ExportRanges count_ranges(int nrange, const char *const *names, const int64_t *elem_off, const int64_t *len, int64_t out_elems, std::string &msg) {
    ExportRanges out;
    msg.clear();
    for (int r = 0; r < nrange; ++r) {
        const int64_t n = len[r] > 0 ? len[r] : 0;
        if (!names[r]) { msg = "range " + std::to_string(r) + " has no name"; return ExportRanges(); }
        if (n > 0 && (elem_off[r] < 0 || elem_off[r] > out_elems || n > out_elems - elem_off[r])) {
            msg = "range " + std::to_string(r) + " lies outside the plan's output";
            return ExportRanges();
        }
        const size_t nl = strlen(names[r]);
        if (out.names.size() + nl >= (size_t)0x7fffffff) { msg = "more than 2^31 bytes of contig names"; return ExportRanges(); }
        ExRange x;
        x.e0 = out.cells; x.n = n; x.cell0 = n > 0 ? elem_off[r] : 0; x.pos0 = 0; x.run_base = 0;
        x.name_off = (int32_t)out.names.size(); x.name_len = (int32_t)nl;
        out.names.insert(out.names.end(), names[r], names[r] + nl);
        out.cells += n;
        if (out.cells > kCountBatchMax) { msg = "a batch of more than 2^32 - 1 elements: export elements are indexed with 32 bits"; return ExportRanges(); }
        out.ranges.push_back(x);
    }
    out.ranges.push_back(ExRange{out.cells, 0, 0, 0, 0, 0, 0});
    return out;
}

// The two predicates of the text (k_counts_flags, k_counts_keep and the host's replay run these).  cells: element 0 of
// the range.  bedGraph (kind 0): element j heads a run when it is the range's first, differs (!=) from the element in
// front of it, or stands on a window border -- period32: the window, 0: no border below 2^32 (no element index reaches
// it); variableStep (kind 1): when it is non-zero.  A run is a bedGraph line when its value is > 0.
template <typename T> PC_TRK_HD inline bool count_is_head(int kind, uint32_t period32, const T *cells, int64_t j) {
    if (kind != 0) return cells[j] != (T)0;
    return j == 0 || cells[j] != cells[j - 1] || (period32 != 0u && (uint32_t)j % period32 == 0u);
}
PC_TRK_HD inline uint32_t count_period32(int kind, int64_t period) { return kind == 0 && period <= (int64_t)0xffffffff ? (uint32_t)period : 0u; }
template <typename T> PC_TRK_HD inline bool count_is_line(T v) { return v > (T)0; }

// Line L of the text of a batch -> its run -> its range.  ranges[k].run_base: runs in front of range k (entry K: all).
// bedGraph (kind 0): run_e holds the head of every run of any value, line_run[L] the run of line L (the runs whose
// value is > 0); the line ends where the next run of its range begins, or with the range (the windows are run borders).
// variableStep (kind 1): run_e holds the non-zero elements; range k has its header at line run_base[k] + k.
// value_at: the place of the line's value among the classified values (bedGraph: the line, variableStep: the run).
struct CountLine { int k; bool header; int64_t run, j, end, value_at; };
PC_TRK_HD inline CountLine count_line_of(int kind, const ExRange *ranges, int K, const uint32_t *run_e, const uint32_t *line_run, int64_t L) {
    CountLine c;
    c.header = false; c.run = 0; c.j = 0; c.end = 0; c.value_at = 0;
    if (kind == 0) {
        c.run = (int64_t)line_run[L];
        const int64_t e = (int64_t)run_e[c.run];
        c.k = ex_range_of(ranges, K, e);
        c.j = e - ranges[c.k].e0;
        c.end = c.run + 1 < ranges[c.k + 1].run_base ? (int64_t)run_e[c.run + 1] - ranges[c.k].e0 : ranges[c.k].n;
        c.value_at = L;
        return c;
    }
    c.k = ex_range_of_line(ranges, K, L);
    if (L == ranges[c.k].run_base + c.k) { c.header = true; return c; }
    c.run = L - c.k - 1;
    c.j = (int64_t)run_e[c.run] - ranges[c.k].e0;
    c.end = c.j + 1;
    c.value_at = c.run;
    return c;
}

struct ContigTable {
    int nstrands = 2;
    int64_t min_chr_size = 10000000;
    std::vector<std::string> names;         // by internal id, in order of first mention
    std::vector<int64_t> length;
    std::vector<uint8_t> born;
    std::map<std::string, int32_t> ids;
    std::vector<int32_t> order, rank;       // the public order; rank[id]: the contig's place in it, -1: not born
    std::vector<int64_t> ext, cell_off;     // per slot: cells [cell_off, cell_off + ext)
    int64_t ncells = 0;

    size_t slot(int32_t id, int strand) const { return (size_t)id * (size_t)nstrands + (size_t)strand; }
    int num_public() const { return (int)order.size(); }
    // the id of public contig i and its slot on strand s, -1: the track has none
    int32_t public_id(int i) const { return i >= 0 && i < num_public() ? order[(size_t)i] : -1; }
    int64_t public_slot(int i, int s) const { return public_id(i) >= 0 && s >= 0 && s < nstrands ? (int64_t)slot(public_id(i), s) : -1; }

    // resolves a name; a new one is an unborn contig
    int32_t id_of(const std::string &name) {
        auto it = ids.find(name);
        if (it != ids.end()) return it->second;
        const int32_t id = (int32_t)names.size();
        names.push_back(name); length.push_back(min_chr_size); born.push_back(0); rank.push_back(-1);
        ids.emplace(name, id);
        ext.resize(names.size() * (size_t)nstrands, 0);
        cell_off.resize(names.size() * (size_t)nstrands, 0);
        return id;
    }
    // an undeclared contig is born at min_chr_size, behind the contigs the array holds already (import and writes)
    void bear(int32_t id) {
        if (born[(size_t)id]) return;
        born[(size_t)id] = 1; length[(size_t)id] = min_chr_size;
        rank[(size_t)id] = (int32_t)order.size();
        order.push_back(id);
    }
    // false: the name is known already
    bool declare(const std::string &name, int64_t len) {
        if (ids.count(name)) return false;
        const int32_t id = id_of(name);
        bear(id);
        length[(size_t)id] = len;
        return true;
    }
    int public_index(const std::string &name) const {
        auto it = ids.find(name);
        return it == ids.end() ? -1 : rank[(size_t)it->second];
    }

    // ---- import: births, growth, storage
    // the length every contig has before a call (what a line must reach to be a growth line)
    std::vector<int64_t> lengths_before() const {
        std::vector<int64_t> len0(names.size());
        for (size_t c = 0; c < names.size(); ++c) len0[c] = born[c] ? length[c] : min_chr_size;
        return len0;
    }
    // the ids to bear, in order of their first yielding line (kNoLine: none)
    std::vector<int32_t> births(const std::vector<uint32_t> &first_line) const {
        std::vector<std::pair<uint32_t, int32_t>> at;
        for (size_t c = 0; c < names.size() && c < first_line.size(); ++c)
            if (!born[c] && first_line[c] != kNoLine) at.emplace_back(first_line[c], (int32_t)c);
        std::sort(at.begin(), at.end());
        std::vector<int32_t> out;
        for (auto &b : at) out.push_back(b.second);
        return out;
    }
    // the reference's rule (genome_array.py:1593-1602), folded in file order over the lines that can matter
    void fold_growth(std::vector<GrowthLine> &lines) {
        std::sort(lines.begin(), lines.end(), [](const GrowthLine &a, const GrowthLine &b) { return a.line < b.line; });
        for (const GrowthLine &x : lines) length[(size_t)x.contig] = grown_length(length[(size_t)x.contig], x.stop);
    }
    // birth and growth of a write, segment by segment as the reference's loop meets them (genome_array.py:1593-1608)
    // returns the furthest end of a segment that writes cells (0: none does)
    int64_t grow_for_set(int32_t id, const int64_t *start, const int64_t *end, int64_t nseg) {
        bear(id);
        int64_t furthest = 0;
        for (int64_t s = 0; s < nseg; ++s) {
            length[(size_t)id] = grown_length(length[(size_t)id], end[s]);
            if (end[s] > start[s]) furthest = std::max(furthest, end[s]);
        }
        return furthest;
    }
    // every slot keeps its cells, slot (c, strand) reaches at least furthest[c]
    StoragePlan plan_storage(int strand, const std::vector<unsigned long long> &furthest) const {
        StoragePlan p;
        const size_t nslot = names.size() * (size_t)nstrands;
        p.ext = ext; p.ext.resize(nslot, 0); p.off.assign(nslot, 0);
        for (size_t c = 0; c < furthest.size() && c < names.size(); ++c) {
            int64_t &x = p.ext[slot((int32_t)c, strand)];
            if ((int64_t)furthest[c] > x) { x = (int64_t)furthest[c]; p.grows = true; }
        }
        for (size_t s = 0; s < nslot; ++s) { p.off[s] = p.total; p.total += p.ext[s]; }
        return p;
    }
    StoragePlan plan_storage(int32_t id, int strand, int64_t furthest) const {
        std::vector<unsigned long long> far((size_t)id + 1, 0ull);
        far[(size_t)id] = (unsigned long long)furthest;
        return plan_storage(strand, far);
    }
    void commit(const StoragePlan &p) { ext = p.ext; cell_off = p.off; ncells = p.total; }
    // first cell of every contig on one strand
    std::vector<int64_t> strand_offsets(int strand) const {
        std::vector<int64_t> off(names.size());
        for (size_t c = 0; c < names.size(); ++c) off[c] = cell_off[slot((int32_t)c, strand)];
        return off;
    }

    // ---- gather and set: the items, cut by the function the dense vector's item kernel runs (dense_host.h).
    // slot_of(s): the slot segment s reads or writes, -1: unknown (all zero).  off null: element 0, step +1.
    template <typename SlotOf>
    void cut_items(int64_t nseg, const int64_t *start, const int64_t *end, const int64_t *off, const int8_t *step, SlotOf slot_of,
                   std::vector<pcdense::Item> &items) const {
        for (int64_t s = 0; s < nseg; ++s) {
            pcdense::SegIn in;
            in.len = end[s] - start[s];
            if (in.len <= 0) continue;
            in.out_off = off ? off[s] : 0; in.step = off ? step[s] : 1;
            in.clip_lo = 0; in.clip_hi = in.len; in.start = start[s];
            const int64_t at = slot_of(s);
            in.known = at >= 0;
            if (in.known) { in.cell_base = cell_off[(size_t)at]; in.ext = ext[(size_t)at]; }
            const int64_t k_end = pcdense::items_of(in.len);
            for (int64_t k = 0; k < k_end; ++k) items.push_back(pcdense::cut_item(in, k));
        }
    }

    // ---- arithmetic and equality
    // cells of public contig i (-1: none) on strand slot s (-1: none): first cell and count, -1 / 0 where the track has none
    void slot_cells(int i, int s, int64_t &c0, int64_t &n) const {
        const int64_t at = public_slot(i, s);
        c0 = at < 0 ? -1 : cell_off[(size_t)at]; n = at < 0 ? 0 : ext[(size_t)at];
    }
    // npair slots to compare: public contig and strand slot in a and in b; returns the cells of the walk
    static int64_t equal_layout(const ContigTable &a, const ContigTable &b, int64_t npair, const int32_t *contig_a, const int32_t *slot_a,
                                const int32_t *contig_b, const int32_t *slot_b, std::vector<OpSlot> &slots) {
        int64_t total = 0;
        for (int64_t k = 0; k < npair; ++k) {
            OpSlot o;
            a.slot_cells(contig_a[k], slot_a[k], o.a0, o.an);
            b.slot_cells(contig_b[k], slot_b[k], o.b0, o.bn);
            o.n = std::max(o.an, o.bn); o.out0 = total;
            total += o.n;
            slots.push_back(o);
        }
        return total;
    }
    // The result of a op b (b null: a op scalar) into the fresh table r: a's contigs in a's order, then (mode all) b's
    // remaining ones at the longer length; truncate: the common ones at the shorter; every length + length_pad.  Strand
    // s of the result takes slot_a[s] of a and slot_b[s] of b.  Returns the cells of the result.
    static int64_t combine_layout(const ContigTable &a, const ContigTable *b, bool mode_all, int64_t length_pad, const int32_t *slot_a,
                                  const int32_t *slot_b, ContigTable &r, std::vector<OpSlot> &slots) {
        struct Pick { int32_t id; int ia, ib; int64_t length; };
        std::vector<Pick> picks;
        for (int i = 0; i < a.num_public(); ++i) {
            const size_t c = (size_t)a.order[(size_t)i];
            const int ib = b ? b->public_index(a.names[c]) : -1;
            if (b && ib < 0 && !mode_all) continue;
            int64_t len = a.length[c];
            if (ib >= 0) { const int64_t lb = b->length[(size_t)b->order[(size_t)ib]]; len = mode_all ? std::max(len, lb) : std::min(len, lb); }
            r.declare(a.names[c], len + length_pad);
            picks.push_back({r.id_of(a.names[c]), i, ib, len});
        }
        for (int i = 0; b && mode_all && i < b->num_public(); ++i) {
            const size_t c = (size_t)b->order[(size_t)i];
            if (a.public_index(b->names[c]) >= 0) continue;
            r.declare(b->names[c], b->length[c] + length_pad);
            picks.push_back({r.id_of(b->names[c]), -1, i, b->length[c]});
        }
        int64_t total = 0;
        for (const Pick &p : picks)
            for (int s = 0; s < r.nstrands; ++s) {
                OpSlot o;
                a.slot_cells(p.ia, slot_a[s], o.a0, o.an);
                if (b) b->slot_cells(p.ib, slot_b[s], o.b0, o.bn); else { o.b0 = -1; o.bn = 0; }
                // a scalar acts on every cell up to the length; arrays: up to the furthest cell either side stores
                o.n = b ? std::min(std::max(o.an, o.bn), p.length) : p.length;
                o.out0 = total;
                r.ext[r.slot(p.id, s)] = o.n; r.cell_off[r.slot(p.id, s)] = total;
                total += o.n;
                slots.push_back(o);
            }
        r.ncells = total;
        return total;
    }

    // ---- export
    ExportSlots export_slots(int strand) const {
        ExportSlots x;
        x.ids = order;
        std::sort(x.ids.begin(), x.ids.end(), [this](int32_t a, int32_t b) { return names[(size_t)a] < names[(size_t)b]; });
        for (int32_t id : x.ids) x.cells.push_back({cell_off[slot(id, strand)], ext[slot(id, strand)]});
        return x;
    }
    // kind 0 (bedGraph) writes a contig whose sum is > 0 and that holds a non-zero cell, from the first to the last of them;
    // kind 1 (variableStep) every contig, all its cells
    ExportRanges export_ranges(int kind, const ExportSlots &x, const std::vector<SlotStat> &stat) const {
        ExportRanges out;
        for (size_t k = 0; k < x.ids.size(); ++k) {
            const SlotStat &s = stat[k];
            if (kind == 0 && !(s.sum > 0.0 && s.first != ~0ull)) continue;
            const std::string &nm = names[(size_t)x.ids[k]];
            ExRange r;
            r.e0 = out.cells; r.run_base = 0;
            r.pos0 = kind == 0 ? (int64_t)s.first : 0;
            r.n = kind == 0 ? (int64_t)(s.last1 - s.first) : x.cells[k].n;
            r.cell0 = x.cells[k].cell0 + r.pos0;
            r.name_off = (int32_t)out.names.size(); r.name_len = (int32_t)nm.size();
            out.names.insert(out.names.end(), nm.begin(), nm.end());
            out.cells += r.n;
            out.ranges.push_back(r);
        }
        if (!out.ranges.empty()) out.ranges.push_back(ExRange{out.cells, 0, 0, 0, 0, 0, 0});
        return out;
    }

    // ---- nonzero
    NzShares nonzero_slots() const {
        NzShares z;
        for (size_t k = 0; k < ext.size(); ++k)
            if (ext[k] > 0) { z.live.push_back((int)k); z.at.push_back(cell_off[k]); }
        z.at.push_back(ncells);
        return z;
    }
    // picked[j]: non-zero cells in front of at[j].  counts[i * nstrands + s]: those of public contig i on strand slot s
    void nonzero_counts(NzShares &z, const std::vector<int64_t> &picked, int64_t *counts) const {
        z.begin.assign(ext.size(), 0); z.cnt.assign(ext.size(), 0);
        for (size_t j = 0; j < z.live.size(); ++j) { z.begin[(size_t)z.live[j]] = picked[j]; z.cnt[(size_t)z.live[j]] = picked[j + 1] - picked[j]; }
        for (int i = 0; i < num_public(); ++i)
            for (int s = 0; s < nstrands; ++s) counts[(size_t)i * (size_t)nstrands + (size_t)s] = z.cnt[slot(order[(size_t)i], s)];
    }
    // the indices in the order of the cells (internal ids) -> slot after slot in public order
    void nonzero_regroup(const NzShares &z, const int64_t *all, int64_t *out) const {
        int64_t w = 0;
        for (int i = 0; i < num_public(); ++i)
            for (int s = 0; s < nstrands; ++s) {
                const size_t k = slot(order[(size_t)i], s);
                if (z.cnt[k]) memcpy(out + w, all + z.begin[k], (size_t)z.cnt[k] * 8);
                w += z.cnt[k];
            }
    }
};

} // namespace pctrack
