// plan_host.h -- the host builder of a plan's tables: one serial pass per table, every table made at once.  Small plans
// and PC_PLAN_BUILD=host take it (pc_plan_create in plastid_counts.hip), and it is the reference the GPU builder's
// tables are compared with (tests/test_gpu_plan.py); a large annotation is built by the kernels of plan_kernels.hip.h.
// Beside it, what the two builders share that needs no HIP: the defect messages and the window choice.
// Plain C++17, no HIP, no threads: tests/plan_host_test.cpp compiles it with the host compiler.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "host_util.h"
#include "plan_tables.h"

namespace pc {

// The caller's segment arrays (pc_plan_create).
struct PlanSegments {
    int64_t n;
    const int32_t *tid;
    const int64_t *start, *end;
    const uint8_t *strand;
    const int64_t *out_off;
    const int8_t *out_step;
    const int64_t *row_stride;
};

struct HostPlan {
    PodVec<Tile> tiles;
    PodVec<Piece> pieces;
    PodVec<OutPiece> opieces;
    std::vector<CenterChunk> cchunks;
    std::vector<GatherSeg> gsegs;
    std::vector<GatherChunk> gchunks;
    int G = 4096;
    uint32_t modes = 0;
    int max_slots = 1;
    int64_t npos = 0;            // island positions (hist row length)
    int64_t covered = 0;
    bool has_sums = false;       // some slices are summed (out_step 0): the output is an accumulator
    bool out_needs_zero = false; // some queried positions lie outside every tile (unknown contig, clipped)
};

// Why a plan was refused.  kind 1: end < start; 2: out_step; 3: the output slice [lo, hi] of segment `seg` leaves the
// buffer; 4: too many rows (`lo`) for the LDS window.
struct PlanDefect { int kind; int64_t seg, lo, hi; };
constexpr int kDefectEnd = 1, kDefectStep = 2, kDefectSlice = 3, kDefectRows = 4;

inline std::string plan_defect_message(const PlanDefect &d, int64_t out_elems) {
    char buf[256];
    const long long b = (long long)d.seg;
    if (d.kind == kDefectEnd) snprintf(buf, sizeof(buf), "segment %lld: end < start", b);
    else if (d.kind == kDefectStep) snprintf(buf, sizeof(buf), "segment %lld: out_step must be +1, -1 or 0 (sum)", b);
    else if (d.kind == kDefectSlice)
        snprintf(buf, sizeof(buf), "segment %lld: output slice [%lld,%lld] outside buffer of %lld elements", b, (long long)d.lo, (long long)d.hi, (long long)out_elems);
    else snprintf(buf, sizeof(buf), "pc_plan_create: too many rows (%d) for the LDS window", (int)d.lo);
    return buf;
}

// The output elements [lo, hi] that segment s (of positive length) writes.
inline void plan_slice_bounds(const PlanSegments &in, int64_t s, int rows, int64_t *lo, int64_t *hi) {
    const int64_t len = in.end[s] - in.start[s];
    const int64_t first = in.out_off[s], last = in.out_off[s] + (int64_t)in.out_step[s] * (len - 1);
    *lo = std::min(first, last);
    *hi = std::max(first, last) + (int64_t)(rows - 1) * in.row_stride[s];
}

// Window size of a plan from the strand modes present and the clipped intervals (their number and total length);
// false: too many rows for the LDS window (the per-call hard limit of LDS is checked in pc_count).
inline bool plan_window(int rows, uint32_t modes, unsigned long long n_iv, unsigned long long iv_len, int knob, int *G) {
    int nmodes = 0;
    for (int m = 0; m < kModes; ++m) nmodes += (modes >> m) & 1;
    if (nmodes == 0) nmodes = 1;
    int64_t budget = 0;
    *G = choose_window(rows, nmodes, n_iv, iv_len, knob, &budget);
    return (rows > 1 ? 2 : 4) * (int64_t)nmodes * rows * *G <= 150 * 1024;
}

namespace planhost {

struct Interval { int32_t tid, mode; int64_t s, e; };
struct Island { int32_t tid, mode; int64_t s, e, off; };

// ---- segments: validation, the per-segment gather records, the clipped intervals.  false: the defect of the lowest
// segment index
static bool scan_segments(const PlanSegments &in, int ntid, int rows, int64_t out_elems, HostPlan &hp, std::vector<Interval> &ivs, PlanDefect &bad) {
    const int64_t kMaxPos = 0x7fffffffLL;
    hp.gsegs.resize((size_t)in.n);
    ivs.reserve((size_t)in.n);
    for (int64_t s = 0; s < in.n; ++s) {
        const int64_t len = in.end[s] - in.start[s];
        const int8_t step = in.out_step[s];
        if (len < 0) { bad = {kDefectEnd, s, 0, 0}; return false; }
        if (step != 1 && step != -1 && step != 0) { bad = {kDefectStep, s, 0, 0}; return false; }
        if (step == 0) hp.has_sums = true;
        if (len > 0) {   // output bounds
            int64_t lo, hi;
            plan_slice_bounds(in, s, rows, &lo, &hi);
            if (lo < 0 || hi >= out_elems || in.row_stride[s] < 0) { bad = {kDefectSlice, s, lo, hi}; return false; }
        }
        GatherSeg &g = hp.gsegs[(size_t)s];
        g.out_off = in.out_off[s]; g.row_stride = in.row_stride[s]; g.len = len; g.step = step; g.pad = 0;
        g.hist_off = -1; g.clip_lo = 0; g.clip_hi = 0; g.start = in.start[s];
        hp.covered += (step == 0 ? (len > 0 ? 1 : 0) : len) * rows;
        if (in.tid[s] < 0 || in.tid[s] >= ntid || len == 0) continue; // unknown chromosome: zeros (genome_array.py:795-798)
        const int64_t cs = std::max<int64_t>(in.start[s], 0), ce = std::min<int64_t>(in.end[s], kMaxPos);
        if (ce <= cs) continue;
        g.clip_lo = cs - in.start[s];
        g.clip_hi = ce - in.start[s];
        const int m = mode_of(in.strand[s]);
        hp.modes |= 1u << m;
        ivs.push_back({in.tid[s], m, cs, ce});
    }
    return true;
}

// ---- islands: union of the queried intervals per (contig, mode), with consecutive offsets into the compact histogram
static std::vector<Island> merge_islands(std::vector<Interval> &ivs, HostPlan &hp) {
    std::sort(ivs.begin(), ivs.end(), [](const Interval &a, const Interval &b) {
        if (a.tid != b.tid) return a.tid < b.tid;
        if (a.mode != b.mode) return a.mode < b.mode;
        if (a.s != b.s) return a.s < b.s;
        return a.e < b.e;
    });
    std::vector<Island> islands;
    for (const Interval &iv : ivs) {
        if (!islands.empty() && islands.back().tid == iv.tid && islands.back().mode == iv.mode && iv.s <= islands.back().e)
            islands.back().e = std::max(islands.back().e, iv.e);
        else
            islands.push_back({iv.tid, iv.mode, iv.s, iv.e, 0});
    }
    for (Island &is : islands) { is.off = hp.npos; hp.npos += is.e - is.s; }
    return islands;
}

// ---- every segment -> its island: where its first clipped position sits in the compact histogram
static void segments_to_islands(const PlanSegments &in, const std::vector<Island> &islands, HostPlan &hp) {
    size_t hint = 0;   // (the exons of a chain follow each other in the caller's arrays: the search starts where the last one ended)
    for (int64_t s = 0; s < in.n; ++s) {
        GatherSeg &g = hp.gsegs[(size_t)s];
        if (g.clip_hi <= g.clip_lo) continue;
        const int64_t cs = in.start[s] + g.clip_lo;
        const int m = mode_of(in.strand[s]);
        const int32_t ts = in.tid[s];
        // first island after the last one with (tid, mode, s) <= (tid, m, cs)
        const size_t lo = gallop_lower_bound(islands.size(), hint, [&](size_t k) {
            const Island &is = islands[k];
            return is.tid < ts || (is.tid == ts && (is.mode < m || (is.mode == m && is.s <= cs)));
        });
        hint = lo;
        const Island &is = islands[lo - 1];
        g.hist_off = is.off + (cs - is.s);
    }
}

// ---- pieces: islands cut at the fixed genome grid of G positions, sorted by (contig, window, mode, start); tiles: the
// grid windows that hold pieces.
// A multi-row plan (stratified rule: rows x G bins per strand mode) gives every strand mode of a window a tile of its
// own: the LDS window of the launch is then sized for ONE mode -- C5: 14 KB instead of 25, seven workgroups per CU
// instead of six -- and the two windows in a hundred that query both strands are scanned twice.  Single-row plans keep
// all modes of a window in one tile: one pass over the records serves both strands.
static void cut_pieces_and_tiles(const std::vector<Island> &islands, bool split_modes, HostPlan &hp) {
    const int G = hp.G;
    struct RawPiece { int32_t tid; int64_t win; Piece pc_; };
    std::vector<RawPiece> raw;
    for (const Island &is : islands)
        for (int64_t a = is.s; a < is.e;) {
            const int64_t win = (a / G) * G;
            const int64_t b = std::min<int64_t>(is.e, win + G);
            Piece pc_;
            pc_.hist_off = is.off + (a - is.s); pc_.start = (int32_t)a; pc_.len = (int32_t)(b - a); pc_.mode = is.mode; pc_.pad = 0;
            raw.push_back({is.tid, win, pc_});
            a = b;
        }
    std::sort(raw.begin(), raw.end(), [](const RawPiece &a, const RawPiece &b) {
        if (a.tid != b.tid) return a.tid < b.tid;
        if (a.win != b.win) return a.win < b.win;
        if (a.pc_.mode != b.pc_.mode) return a.pc_.mode < b.pc_.mode;
        return a.pc_.start < b.pc_.start;
    });
    hp.pieces.reserve(raw.size());
    for (size_t i = 0; i < raw.size();) {
        size_t j = i + 1;
        while (j < raw.size() && raw[j].tid == raw[i].tid && raw[j].win == raw[i].win && (!split_modes || raw[j].pc_.mode == raw[i].pc_.mode)) ++j;
        Tile t;
        t.tid = raw[i].tid; t.win_start = (int32_t)raw[i].win; t.piece_begin = (uint32_t)i; t.piece_end = (uint32_t)j;
        t.mode_mask = 0; t.op_begin = t.op_end = 0; t.span_lo = 0xffff; t.span_hi = 0;
        for (; i < j; ++i) {
            const Piece &pc_ = raw[i].pc_;
            t.mode_mask |= 1u << pc_.mode;
            t.span_lo = std::min<uint16_t>(t.span_lo, (uint16_t)(pc_.start - t.win_start));
            t.span_hi = std::max<uint16_t>(t.span_hi, (uint16_t)(pc_.start - t.win_start + pc_.len));
            hp.pieces.push_back(pc_);
        }
        hp.max_slots = std::max(hp.max_slots, __builtin_popcount(t.mode_mask));
        hp.tiles.push_back(t);
    }
}

// ---- output pieces: every queried segment cut at the tile grid, in the caller's layout -- appended in segment order,
// then one stable counting sort by tile
static void cut_output_pieces(const PlanSegments &in, bool split_modes, HostPlan &hp) {
    const int G = hp.G;
    struct RawOut { uint32_t tile; OutPiece o; };
    std::vector<RawOut> raw;
    raw.reserve((size_t)in.n + (size_t)in.n / 2);
    size_t seg_hint = 0;   // tile of the previous segment's last window: the next exon of the chain is close by
    for (int64_t s = 0; s < in.n; ++s) {
        const GatherSeg &g = hp.gsegs[(size_t)s];
        if (g.len > 0 && (g.hist_off < 0 || g.clip_lo > 0 || g.clip_hi < g.len)) hp.out_needs_zero = true;
        if (g.hist_off < 0 || g.clip_hi <= g.clip_lo) continue;
        const int m = mode_of(in.strand[s]);
        const int32_t ts = in.tid[s];
        const uint32_t want_mask = 1u << m;
        const int64_t cs = in.start[s] + g.clip_lo, ce = in.start[s] + g.clip_hi;
        size_t prev = (size_t)-1;   // tile of the segment's previous window: the next window's tile follows it
        for (int64_t a = cs; a < ce;) {
            const int64_t win = (a / G) * G;
            const int64_t b = std::min<int64_t>(ce, win + G);
            // tile of (tid, win)
            // (tiles are sorted by contig, window and -- when every mode has its own tile -- mode: a one-mode
            // tile's mask, 1 << mode, orders like the mode)
            size_t lo = prev + 1;
            if (prev == (size_t)-1 || lo >= hp.tiles.size() || hp.tiles[lo].tid != ts || (int64_t)hp.tiles[lo].win_start != win ||
                (split_modes && hp.tiles[lo].mode_mask != want_mask))
                lo = gallop_lower_bound(hp.tiles.size(), seg_hint, [&](size_t k) {
                    const Tile &t = hp.tiles[k];
                    if (t.tid != ts) return t.tid < ts;
                    if ((int64_t)t.win_start != win) return (int64_t)t.win_start < win;
                    return split_modes && t.mode_mask < want_mask;
                });
            prev = lo;
            seg_hint = lo;
            OutPiece o;
            o.out_off = g.out_off + (int64_t)g.step * (a - in.start[s]);
            o.row_stride = g.row_stride;
            o.hist_off = g.hist_off + (a - cs);
            o.start = (int32_t)a; o.len = (int32_t)(b - a); o.mode = m; o.step = g.step;
            raw.push_back({(uint32_t)lo, o});
            a = b;
        }
    }
    std::vector<uint32_t> at(hp.tiles.size() + 1, 0);   // at[t + 1]: records of tile t, then the cursor of tile t
    for (const RawOut &r : raw) at[(size_t)r.tile + 1] += 1;
    uint32_t run = 0;
    for (size_t t = 0; t < hp.tiles.size(); ++t) {
        const uint32_t c = at[t + 1];
        hp.tiles[t].op_begin = run;
        at[t + 1] = run;
        run += c;
        hp.tiles[t].op_end = run;
    }
    hp.opieces.resize(raw.size());
    for (const RawOut &r : raw) hp.opieces[at[(size_t)r.tile + 1]++] = r.o;
}

// ---- center chunks: the pieces in tile / piece order, cut into 64 positions (one wave of the ordered center replay
// each), every chunk with the output pieces of its tile
static void cut_center_chunks(HostPlan &hp) {
    hp.cchunks.reserve((size_t)(hp.npos / kWave) + hp.pieces.size());
    for (const Tile &t : hp.tiles)
        for (uint32_t i = t.piece_begin; i < t.piece_end; ++i) {
            const Piece &pc_ = hp.pieces[i];
            for (int32_t a = 0; a < pc_.len; a += kWave) {
                CenterChunk c;
                c.hist_off = pc_.hist_off + a; c.tid = t.tid; c.start = pc_.start + a;
                c.len = std::min<int32_t>(kWave, pc_.len - a); c.mode = pc_.mode;
                c.op_begin = t.op_begin; c.op_end = t.op_end;
                hp.cchunks.push_back(c);
            }
        }
}

// ---- gather list (center rule, coordinate export): the segments in chunks of kGatherChunk positions
static void list_gather_chunks(HostPlan &hp) {
    for (size_t s = 0; s < hp.gsegs.size(); ++s)
        for (int64_t c = 0; c * kGatherChunk < hp.gsegs[s].len; ++c) hp.gchunks.push_back({(uint32_t)s, (uint32_t)c});
}

} // namespace planhost

// All tables and scalars of the plan of `in` into `hp` (which arrives empty).  `ntid`: contigs of the engine; `rows`:
// rows of the mapping rule; `tile_g_knob`: PC_TILE_G (0: none).  false: no plan, and `bad` says why -- a defective
// segment (the lowest index first), then the rows.
inline bool build_plan_host(const PlanSegments &in, int ntid, int rows, int64_t out_elems, int tile_g_knob, HostPlan &hp, PlanDefect &bad) {
    using namespace planhost;
    StageClock clk;
    std::vector<Interval> ivs;
    if (!scan_segments(in, ntid, rows, out_elems, hp, ivs, bad)) return false;
    unsigned long long iv_len = 0;
    for (const Interval &iv : ivs) iv_len += (unsigned long long)(iv.e - iv.s);
    if (!plan_window(rows, hp.modes, (unsigned long long)ivs.size(), iv_len, tile_g_knob, &hp.G)) { bad = {kDefectRows, 0, rows, 0}; return false; }
    clk.lap("plan: segments");
    const std::vector<Island> islands = merge_islands(ivs, hp);
    clk.lap("plan: islands");
    segments_to_islands(in, islands, hp);
    clk.lap("plan: segment->island");
    const bool split_modes = rows > 1;
    cut_pieces_and_tiles(islands, split_modes, hp);
    clk.lap("plan: pieces+tiles");
    cut_output_pieces(in, split_modes, hp);
    clk.lap("plan: output pieces");
    cut_center_chunks(hp);
    clk.lap("plan: center chunks");
    list_gather_chunks(hp);
    clk.lap("plan: gather list");
    return true;
}

} // namespace pc
