// CPU test of plastid_amd/csrc/plan_host.h, the host builder of a plan's tables (compiled and run by
// tests/test_host_logic.py; test infrastructure).  Part one: cases whose tables are written out by hand.  Part two: random
// small inputs against a model that expands every queried position -- it shares no code with the builder.
#include <cstdio>
#include <map>
#include <random>
#include <string>
#include "plan_host.h"

using namespace pc;

namespace {

long bad = 0;
#define CHECK(cond) do { if (!(cond)) { ++bad; printf("line %d: %s\n", __LINE__, #cond); } } while (0)

// A plan's input in the layout the callers use: every segment gets `rows` rows of its own, one after the other; a
// reversed segment (step -1) starts at the end of its first row, a summed one (step 0) has one element per row.
struct Input {
    std::vector<int32_t> tid;
    std::vector<int64_t> start, end, out_off, row_stride, block;   // block: first element of the segment's rows
    std::vector<uint8_t> strand;
    std::vector<int8_t> step;
    int64_t out_elems = 0;
    int rows = 1;
    void add(int32_t t, int64_t s, int64_t e, uint8_t str, int8_t st) {
        const int64_t len = e - s, size = st == 0 ? (len > 0 ? 1 : 0) : len;
        tid.push_back(t); start.push_back(s); end.push_back(e); strand.push_back(str); step.push_back(st);
        block.push_back(out_elems);
        out_off.push_back(st == -1 ? out_elems + len - 1 : out_elems);
        row_stride.push_back(size);
        out_elems += size * rows;
    }
    PlanSegments seg() const { return {(int64_t)tid.size(), tid.data(), start.data(), end.data(), strand.data(), out_off.data(), step.data(), row_stride.data()}; }
};

bool build(const Input &in, int ntid, HostPlan &hp, PlanDefect &d) { return build_plan_host(in.seg(), ntid, in.rows, in.out_elems, 256, hp, d); }

bool same(const Tile &t, int32_t tid, int32_t win, uint32_t pb, uint32_t pe, uint32_t mask, uint32_t ob, uint32_t oe, int lo, int hi) {
    return t.tid == tid && t.win_start == win && t.piece_begin == pb && t.piece_end == pe && t.mode_mask == mask && t.op_begin == ob && t.op_end == oe &&
           t.span_lo == lo && t.span_hi == hi;
}
bool same(const Piece &p, int64_t hist, int32_t start, int32_t len, int32_t mode) {
    return p.hist_off == hist && p.start == start && p.len == len && p.mode == mode && p.pad == 0;
}
bool same(const OutPiece &o, int64_t out, int64_t stride, int64_t hist, int32_t start, int32_t len, int32_t mode, int32_t step) {
    return o.out_off == out && o.row_stride == stride && o.hist_off == hist && o.start == start && o.len == len && o.mode == mode && o.step == step;
}
bool same(const CenterChunk &c, int64_t hist, int32_t tid, int32_t start, int32_t len, int32_t mode, uint32_t ob, uint32_t oe) {
    return c.hist_off == hist && c.tid == tid && c.start == start && c.len == len && c.mode == mode && c.op_begin == ob && c.op_end == oe;
}
bool same(const GatherSeg &g, int64_t out, int64_t stride, int64_t hist, int64_t len, int64_t clo, int64_t chi, int64_t start, int32_t step) {
    return g.out_off == out && g.row_stride == stride && g.hist_off == hist && g.len == len && g.clip_lo == clo && g.clip_hi == chi && g.start == start &&
           g.step == step && g.pad == 0;
}

const uint8_t FWD = PC_STRAND_FWD, REV = PC_STRAND_REV, UNS = PC_STRAND_UNS;

Input starting_case(int rows) {
    Input in;
    in.rows = rows;
    in.add(0, 100, 300, FWD, 1);    // s0
    in.add(0, 250, 600, FWD, -1);   // s1: overlaps s0, reversed output
    in.add(0, 250, 260, REV, 0);    // s2: the other strand, summed
    in.add(7, 0, 10, UNS, 1);       // s3: unknown contig
    in.add(1, -5, 20, UNS, 1);      // s4: clipped at 0
    return in;
}

void hand_worked() {
    {   // ---- the starting case, one row.  Output: s0 at 0 .. 199, s1 at 200 .. 549 (written from 549 down), s2 at 550, s3 at
        // 551 .. 560, s4 at 561 .. 585.  Intervals: contig 0 '+' [100, 300) and [250, 600) merge into [100, 600) (offset 0);
        // contig 0 '-' [250, 260) (offset 500); contig 1 '.' [0, 20) (offset 510): 530 positions.
        const Input in = starting_case(1);
        HostPlan hp;
        PlanDefect d;
        CHECK(in.out_elems == 586);
        CHECK(build(in, 2, hp, d));
        CHECK(hp.G == 256 && hp.modes == 7u && hp.max_slots == 2 && hp.npos == 530 && hp.covered == 586 && hp.has_sums && hp.out_needs_zero);
        CHECK(hp.gsegs.size() == 5);
        if (hp.gsegs.size() == 5) {
            CHECK(same(hp.gsegs[0], 0, 200, 0, 200, 0, 200, 100, 1));
            CHECK(same(hp.gsegs[1], 549, 350, 150, 350, 0, 350, 250, -1));   // position 250 is 150 into the island
            CHECK(same(hp.gsegs[2], 550, 1, 500, 10, 0, 10, 250, 0));
            CHECK(same(hp.gsegs[3], 551, 10, -1, 10, 0, 0, 0, 1));
            CHECK(same(hp.gsegs[4], 561, 25, 510, 25, 5, 25, -5, 1));        // clip_lo 5: positions -5 .. -1 do not exist
        }
        // pieces by (contig, window, mode, start)
        CHECK(hp.pieces.size() == 6);
        if (hp.pieces.size() == 6) {
            CHECK(same(hp.pieces[0], 0, 100, 156, 0));
            CHECK(same(hp.pieces[1], 500, 250, 6, 1));
            CHECK(same(hp.pieces[2], 156, 256, 256, 0));
            CHECK(same(hp.pieces[3], 506, 256, 4, 1));
            CHECK(same(hp.pieces[4], 412, 512, 88, 0));
            CHECK(same(hp.pieces[5], 510, 0, 20, 2));
        }
        CHECK(hp.tiles.size() == 4);
        if (hp.tiles.size() == 4) {
            CHECK(same(hp.tiles[0], 0, 0, 0, 2, 3, 0, 3, 100, 256));
            CHECK(same(hp.tiles[1], 0, 256, 2, 4, 3, 3, 6, 0, 256));
            CHECK(same(hp.tiles[2], 0, 512, 4, 5, 1, 6, 7, 0, 88));
            CHECK(same(hp.tiles[3], 1, 0, 5, 6, 4, 7, 8, 0, 20));
        }
        // output pieces: by tile, in segment order inside a tile
        CHECK(hp.opieces.size() == 8);
        if (hp.opieces.size() == 8) {
            CHECK(same(hp.opieces[0], 0, 200, 0, 100, 156, 0, 1));       // s0, window 0
            CHECK(same(hp.opieces[1], 549, 350, 150, 250, 6, 0, -1));    // s1, window 0
            CHECK(same(hp.opieces[2], 550, 1, 500, 250, 6, 1, 0));       // s2, window 0
            CHECK(same(hp.opieces[3], 156, 200, 156, 256, 44, 0, 1));    // s0, window 256
            CHECK(same(hp.opieces[4], 543, 350, 156, 256, 256, 0, -1));  // s1, window 256: six positions further, six elements lower
            CHECK(same(hp.opieces[5], 550, 1, 506, 256, 4, 1, 0));       // s2, window 256: the same sum
            CHECK(same(hp.opieces[6], 287, 350, 412, 512, 88, 0, -1));   // s1, window 512: 549 - 262
            CHECK(same(hp.opieces[7], 566, 25, 510, 0, 20, 2, 1));       // s4 from position 0: five elements into its row
        }
        CHECK(hp.cchunks.size() == 12);
        if (hp.cchunks.size() == 12) {
            CHECK(same(hp.cchunks[0], 0, 0, 100, 64, 0, 0, 3));
            CHECK(same(hp.cchunks[1], 64, 0, 164, 64, 0, 0, 3));
            CHECK(same(hp.cchunks[2], 128, 0, 228, 28, 0, 0, 3));
            CHECK(same(hp.cchunks[3], 500, 0, 250, 6, 1, 0, 3));
            CHECK(same(hp.cchunks[4], 156, 0, 256, 64, 0, 3, 6));
            CHECK(same(hp.cchunks[5], 220, 0, 320, 64, 0, 3, 6));
            CHECK(same(hp.cchunks[6], 284, 0, 384, 64, 0, 3, 6));
            CHECK(same(hp.cchunks[7], 348, 0, 448, 64, 0, 3, 6));
            CHECK(same(hp.cchunks[8], 506, 0, 256, 4, 1, 3, 6));
            CHECK(same(hp.cchunks[9], 412, 0, 512, 64, 0, 6, 7));
            CHECK(same(hp.cchunks[10], 476, 0, 576, 24, 0, 6, 7));
            CHECK(same(hp.cchunks[11], 510, 1, 0, 20, 2, 7, 8));
        }
        CHECK(hp.gchunks.size() == 5);   // every segment is shorter than a gather chunk, none is empty
        for (size_t s = 0; s < hp.gchunks.size(); ++s) CHECK(hp.gchunks[s].seg == s && hp.gchunks[s].chunk == 0);
    }
    {   // ---- the same segments, two rows: every strand mode of a window has a tile of its own.  Output blocks: s0 at 0, s1 at
        // 400 (from 749 down), s2 at 1100, s3 at 1102, s4 at 1122; 1172 elements.
        const Input in = starting_case(2);
        HostPlan hp;
        PlanDefect d;
        CHECK(in.out_elems == 1172);
        CHECK(build(in, 2, hp, d));
        CHECK(hp.G == 256 && hp.modes == 7u && hp.max_slots == 1 && hp.npos == 530 && hp.covered == 1172 && hp.has_sums && hp.out_needs_zero);
        CHECK(hp.pieces.size() == 6 && hp.tiles.size() == 6 && hp.opieces.size() == 8);
        if (hp.pieces.size() == 6 && hp.tiles.size() == 6 && hp.opieces.size() == 8) {
            CHECK(same(hp.pieces[1], 500, 250, 6, 1) && same(hp.pieces[4], 412, 512, 88, 0));   // the pieces do not move
            CHECK(same(hp.tiles[0], 0, 0, 0, 1, 1, 0, 2, 100, 256));
            CHECK(same(hp.tiles[1], 0, 0, 1, 2, 2, 2, 3, 250, 256));
            CHECK(same(hp.tiles[2], 0, 256, 2, 3, 1, 3, 5, 0, 256));
            CHECK(same(hp.tiles[3], 0, 256, 3, 4, 2, 5, 6, 0, 4));
            CHECK(same(hp.tiles[4], 0, 512, 4, 5, 1, 6, 7, 0, 88));
            CHECK(same(hp.tiles[5], 1, 0, 5, 6, 4, 7, 8, 0, 20));
            CHECK(same(hp.opieces[0], 0, 200, 0, 100, 156, 0, 1));
            CHECK(same(hp.opieces[1], 749, 350, 150, 250, 6, 0, -1));
            CHECK(same(hp.opieces[2], 1100, 1, 500, 250, 6, 1, 0));
            CHECK(same(hp.opieces[3], 156, 200, 156, 256, 44, 0, 1));
            CHECK(same(hp.opieces[4], 743, 350, 156, 256, 256, 0, -1));
            CHECK(same(hp.opieces[5], 1100, 1, 506, 256, 4, 1, 0));
            CHECK(same(hp.opieces[6], 487, 350, 412, 512, 88, 0, -1));
            CHECK(same(hp.opieces[7], 1127, 25, 510, 0, 20, 2, 1));
        }
    }
    {   // ---- a segment that ends exactly on a window border, and one that starts on it: no piece of length 0, no third window
        Input in;
        in.add(0, 200, 512, FWD, 1);
        in.add(1, 256, 300, FWD, 1);
        HostPlan hp;
        PlanDefect d;
        CHECK(build(in, 2, hp, d));
        CHECK(hp.npos == 356 && !hp.out_needs_zero && !hp.has_sums && hp.modes == 1u && hp.max_slots == 1 && hp.covered == 356);
        CHECK(hp.pieces.size() == 3 && hp.tiles.size() == 3 && hp.opieces.size() == 3 && hp.cchunks.size() == 1 + 4 + 1);
        if (hp.pieces.size() == 3 && hp.tiles.size() == 3 && hp.opieces.size() == 3) {
            CHECK(same(hp.pieces[0], 0, 200, 56, 0) && same(hp.pieces[1], 56, 256, 256, 0) && same(hp.pieces[2], 312, 256, 44, 0));
            CHECK(same(hp.tiles[0], 0, 0, 0, 1, 1, 0, 1, 200, 256) && same(hp.tiles[1], 0, 256, 1, 2, 1, 1, 2, 0, 256) && same(hp.tiles[2], 1, 256, 2, 3, 1, 2, 3, 0, 44));
            CHECK(same(hp.opieces[1], 56, 312, 56, 256, 256, 0, 1) && same(hp.opieces[2], 312, 44, 312, 256, 44, 0, 1));
        }
    }
    {   // ---- an empty segment: a record, no interval, nothing to zero; alone it makes a plan without tiles
        Input in;
        in.add(0, 50, 50, FWD, 1);
        HostPlan hp;
        PlanDefect d;
        CHECK(build(in, 2, hp, d));
        CHECK(hp.G == 256 && hp.modes == 0u && hp.npos == 0 && hp.covered == 0 && !hp.out_needs_zero && hp.max_slots == 1);
        CHECK(hp.tiles.empty() && hp.pieces.empty() && hp.opieces.empty() && hp.cchunks.empty() && hp.gchunks.empty());
        CHECK(hp.gsegs.size() == 1 && same(hp.gsegs[0], 0, 0, -1, 0, 0, 0, 50, 1));
        // between two others it changes nothing but the segment numbering of the gather list
        Input in2;
        in2.add(0, 10, 20, FWD, 1);
        in2.add(0, 15, 15, REV, 1);
        in2.add(0, 30, 40, FWD, 1);
        HostPlan h2;
        CHECK(build(in2, 2, h2, d));
        CHECK(h2.modes == 1u && h2.npos == 20 && h2.pieces.size() == 2 && h2.tiles.size() == 1 && h2.opieces.size() == 2 && h2.gchunks.size() == 2);
        if (h2.gchunks.size() == 2) CHECK(h2.gchunks[0].seg == 0 && h2.gchunks[1].seg == 2);
    }
    {   // ---- a segment beyond the last position a record can have (2^31 - 2): clipped at 2^31 - 1
        Input in;
        in.add(0, 2147483638LL, 2147483653LL, FWD, 1);
        HostPlan hp;
        PlanDefect d;
        CHECK(build(in, 1, hp, d));
        CHECK(hp.gsegs.size() == 1 && same(hp.gsegs[0], 0, 15, 0, 15, 0, 9, 2147483638LL, 1) && hp.npos == 9 && hp.out_needs_zero);
    }
    {   // ---- defects: one of each kind, each with another defect at a higher index that must not win
        HostPlan hp;
        PlanDefect d;
        Input a;
        a.add(0, 10, 20, FWD, 1); a.add(0, 30, 40, FWD, 1); a.add(0, 50, 60, FWD, 1); a.add(0, 70, 80, FWD, 1);
        Input e1 = a;
        e1.end[1] = 29; e1.step[3] = 2;
        CHECK(!build(e1, 2, hp, d) && d.kind == kDefectEnd && d.seg == 1);
        CHECK(plan_defect_message(d, e1.out_elems) == "segment 1: end < start");
        Input e2 = a;
        e2.step[0] = 2; e2.end[2] = 49;
        hp = HostPlan();
        CHECK(!build(e2, 2, hp, d) && d.kind == kDefectStep && d.seg == 0);
        CHECK(plan_defect_message(d, e2.out_elems) == "segment 0: out_step must be +1, -1 or 0 (sum)");
        Input e3 = a;   // 40 elements; segment 2 moved to 35 .. 44
        e3.out_off[2] = 35; e3.end[3] = 69;
        hp = HostPlan();
        CHECK(!build(e3, 2, hp, d) && d.kind == kDefectSlice && d.seg == 2 && d.lo == 35 && d.hi == 44);
        CHECK(plan_defect_message(d, e3.out_elems) == "segment 2: output slice [35,44] outside buffer of 40 elements");
        Input e4 = a;   // a reversed slice that starts below its length, and a negative row stride
        e4.step[1] = -1; e4.out_off[1] = 3;
        hp = HostPlan();
        CHECK(!build(e4, 2, hp, d) && d.kind == kDefectSlice && d.seg == 1 && d.lo == -6 && d.hi == 3);
        Input e5 = a;
        e5.row_stride[3] = -1;
        hp = HostPlan();
        CHECK(!build(e5, 2, hp, d) && d.kind == kDefectSlice && d.seg == 3);
    }
    {   // ---- rows: 16-bit bins, one mode, the smallest window (256): 2 x rows x 256 bytes against 150 KiB -- 300 rows fit, 301 do not
        HostPlan hp;
        PlanDefect d;
        Input in;
        in.rows = 300;
        in.add(0, 10, 20, FWD, 1);
        CHECK(build(in, 2, hp, d) && hp.G == 256);
        Input big;
        big.rows = 301;
        big.add(0, 10, 20, FWD, 1);
        hp = HostPlan();
        CHECK(!build(big, 2, hp, d) && d.kind == kDefectRows);
        CHECK(plan_defect_message(d, big.out_elems) == "pc_plan_create: too many rows (301) for the LDS window");
        big.add(0, 30, 29, FWD, 1);   // a defective segment is reported before the rows
        big.out_elems = 3010;         // (the buffer of the first segment)
        hp = HostPlan();
        CHECK(!build(big, 2, hp, d) && d.kind == kDefectEnd && d.seg == 1);
    }
}

// ---- the model: every position of contig t in mode m that some segment queries, and its rank among them in (contig,
// mode, position) order -- which is its offset in the compact histogram, islands being maximal runs of such positions
const int kContigs = 3, kMaxPos = 3000, G = 256;

void model(uint64_t seed, int rows) {
    std::mt19937_64 rng(seed);
    auto pick = [&](std::initializer_list<int> v) { return v.begin()[rng() % v.size()]; };
    Input in;
    in.rows = rows;
    const int n = 1 + (int)(rng() % 200);
    for (int s = 0; s < n; ++s) {
        const int len = pick({0, 1, 2, 30, 30, 30, 64, 65, 255, 256, 257, 600, 2500});
        int64_t start = (int64_t)(rng() % 700) - 20;                     // some start below 0
        if (rng() % 5 == 0) start = start / G * G;                       // window-aligned
        if (s > 0 && rng() % 6 == 0) start = in.end[(size_t)s - 1];      // touching the previous segment
        if (s > 0 && rng() % 8 == 0) start = in.start[(size_t)s - 1];    // the same start
        if (start >= 480) start %= 480;                                  // (every coordinate stays below 3 000)
        in.add((int32_t)(rng() % 5) - 1, start, start + len, (uint8_t)pick({0, 1, 2, 3, 0x11, 0x12}), (int8_t)pick({1, 1, -1, 0}));   // contigs -1 and 3: unknown
    }
    HostPlan hp;
    PlanDefect d;
    if (!build(in, kContigs, hp, d)) { ++bad; printf("model %llu: refused\n", (unsigned long long)seed); return; }
    const long bad_before = bad;
    static int64_t off[kContigs][kModes][kMaxPos];
    static int hits[kContigs][kModes][kMaxPos];
    for (auto &a : off) for (auto &b : a) for (auto &c : b) c = -1;
    for (auto &a : hits) for (auto &b : a) for (auto &c : b) c = 0;
    uint32_t modes = 0;
    int64_t covered = 0, queried = 0;
    bool sums = false, zero = false;
    std::vector<int64_t> owner((size_t)in.out_elems, -1);   // segment of an output element
    for (int s = 0; s < n; ++s) {
        const int64_t len = in.end[(size_t)s] - in.start[(size_t)s];
        const int t = in.tid[(size_t)s], m = mode_of(in.strand[(size_t)s]), st = in.step[(size_t)s];
        covered += (st == 0 ? (len > 0 ? 1 : 0) : len) * rows;
        sums |= st == 0;
        for (int64_t k = 0; k < in.row_stride[(size_t)s] * rows; ++k) owner[(size_t)(in.block[(size_t)s] + k)] = s;
        if (len > 0 && (t < 0 || t >= kContigs || in.start[(size_t)s] < 0)) zero = true;
        if (t < 0 || t >= kContigs) continue;
        for (int64_t pos = std::max<int64_t>(in.start[(size_t)s], 0); pos < in.end[(size_t)s]; ++pos) { off[t][m][pos] = 0; modes |= 1u << m; ++queried; }
    }
    int64_t npos = 0;
    for (auto &a : off) for (auto &b : a) for (auto &c : b) if (c == 0) c = npos++;
    CHECK(hp.G == G && hp.npos == npos && hp.modes == modes && hp.covered == covered && hp.has_sums == sums && hp.out_needs_zero == zero);
    // tiles: strictly ascending in (contig, window[, mode]); their piece and output ranges partition the two lists
    int max_slots = 1;
    uint32_t pe = 0, oe = 0;
    for (size_t k = 0; k < hp.tiles.size(); ++k) {
        const Tile &t = hp.tiles[k];
        CHECK(t.tid >= 0 && t.tid < kContigs && t.win_start >= 0 && t.win_start % G == 0);
        CHECK(t.piece_begin == pe && t.piece_end > t.piece_begin && t.op_begin == oe && t.op_end > t.op_begin);   // (a tile exists for queried positions: it has both)
        pe = t.piece_end; oe = t.op_end;
        CHECK(pe <= hp.pieces.size() && oe <= hp.opieces.size());
        if (pe > hp.pieces.size() || oe > hp.opieces.size()) return;
        if (rows > 1) CHECK(__builtin_popcount(t.mode_mask) == 1);
        max_slots = std::max(max_slots, __builtin_popcount(t.mode_mask));
        if (k > 0) {
            const Tile &u = hp.tiles[k - 1];
            CHECK(u.tid < t.tid || (u.tid == t.tid && (u.win_start < t.win_start || (rows > 1 && u.win_start == t.win_start && u.mode_mask < t.mode_mask))));
        }
        // its pieces: maximal runs of queried positions inside the window, by (mode, start), with the positions' offsets
        uint32_t mask = 0;
        int lo = G, hi = 0;
        for (uint32_t i = t.piece_begin; i < t.piece_end; ++i) {
            const Piece &p = hp.pieces[i];
            CHECK(p.len > 0 && p.mode >= 0 && p.mode < kModes && p.start >= t.win_start && p.start + p.len <= t.win_start + G && p.pad == 0);
            if (i > t.piece_begin) CHECK(hp.pieces[i - 1].mode < p.mode || (hp.pieces[i - 1].mode == p.mode && hp.pieces[i - 1].start < p.start));
            mask |= 1u << p.mode;
            lo = std::min(lo, p.start - t.win_start); hi = std::max(hi, p.start - t.win_start + p.len);
            for (int j = 0; j < p.len; ++j) { CHECK(off[t.tid][p.mode][p.start + j] == p.hist_off + j); hits[t.tid][p.mode][p.start + j] += 1; }
            CHECK(p.start == t.win_start || off[t.tid][p.mode][p.start - 1] < 0);
            CHECK(p.start + p.len == t.win_start + G || off[t.tid][p.mode][p.start + p.len] < 0);
        }
        CHECK(mask == t.mode_mask && t.span_lo == lo && t.span_hi == hi);
    }
    CHECK(pe == hp.pieces.size() && oe == hp.opieces.size() && hp.max_slots == max_slots);
    for (int t = 0; t < kContigs; ++t) for (int m = 0; m < kModes; ++m) for (int p = 0; p < kMaxPos; ++p) CHECK(hits[t][m][p] == (off[t][m][p] >= 0 ? 1 : 0));
    // output pieces: (output element, position) -> the piece that holds it; in a tile, pieces follow the segment order
    std::map<std::pair<int64_t, int64_t>, std::pair<uint32_t, uint32_t>> where;   // -> (tile, output piece)
    int64_t placed = 0;
    for (size_t k = 0; k < hp.tiles.size(); ++k) {
        int64_t last_owner = -1;
        for (uint32_t i = hp.tiles[k].op_begin; i < hp.tiles[k].op_end; ++i) {
            const OutPiece &o = hp.opieces[i];
            CHECK(o.len > 0 && o.out_off >= 0 && o.out_off < in.out_elems);
            if (o.len <= 0 || o.out_off < 0 || o.out_off >= in.out_elems) return;
            CHECK(owner[(size_t)o.out_off] > last_owner);
            last_owner = owner[(size_t)o.out_off];
            for (int j = 0; j < o.len; ++j) CHECK(where.insert({{o.out_off + (int64_t)o.step * j, o.start + j}, {(uint32_t)k, i}}).second);
            placed += o.len;
        }
    }
    CHECK(placed == queried);
    for (int s = 0; s < n; ++s) {
        const int t = in.tid[(size_t)s], m = mode_of(in.strand[(size_t)s]), st = in.step[(size_t)s];
        const int64_t start = in.start[(size_t)s], len = in.end[(size_t)s] - start, cs = std::max<int64_t>(start, 0);
        const bool known = t >= 0 && t < kContigs && in.end[(size_t)s] > cs;
        CHECK(same(hp.gsegs[(size_t)s], in.out_off[(size_t)s], in.row_stride[(size_t)s], known ? off[t][m][cs] : -1, len, known ? cs - start : 0, known ? len : 0, start, st));
        for (int64_t pos = cs; known && pos < in.end[(size_t)s]; ++pos) {
            const auto it = where.find({in.out_off[(size_t)s] + (int64_t)st * (pos - start), pos});
            CHECK(it != where.end());
            if (it == where.end()) break;
            const Tile &tl = hp.tiles[it->second.first];
            const OutPiece &o = hp.opieces[it->second.second];
            CHECK(tl.tid == t && tl.win_start == pos / G * G && (rows > 1 ? tl.mode_mask == 1u << m : (tl.mode_mask >> m) & 1u));
            CHECK(o.mode == m && o.step == st && o.row_stride == in.row_stride[(size_t)s] && o.hist_off + (pos - o.start) == off[t][m][pos]);
        }
    }
    // center chunks: the pieces in tile / piece order, cut every 64 positions, with the output range of their tile
    size_t c = 0;
    for (const Tile &t : hp.tiles)
        for (uint32_t i = t.piece_begin; i < t.piece_end; ++i)
            for (int a = 0; a < hp.pieces[i].len; a += 64, ++c) {
                CHECK(c < hp.cchunks.size());
                if (c >= hp.cchunks.size()) return;
                CHECK(same(hp.cchunks[c], hp.pieces[i].hist_off + a, t.tid, hp.pieces[i].start + a, std::min(64, hp.pieces[i].len - a), hp.pieces[i].mode, t.op_begin, t.op_end));
            }
    CHECK(c == hp.cchunks.size());
    // gather list: every segment in chunks of 1 024 positions
    size_t g = 0;
    for (int s = 0; s < n; ++s)
        for (int64_t k = 0; k * 1024 < in.end[(size_t)s] - in.start[(size_t)s]; ++k, ++g) {
            CHECK(g < hp.gchunks.size());
            if (g >= hp.gchunks.size()) return;
            CHECK(hp.gchunks[g].seg == (uint32_t)s && hp.gchunks[g].chunk == (uint32_t)k);
        }
    CHECK(g == hp.gchunks.size());
    if (bad != bad_before) printf("model: seed %llu, rows %d, %d segments\n", (unsigned long long)seed, rows, n);
}

} // namespace

int main() {
    hand_worked();
    printf("hand-worked cases: bad %ld\n", bad);
    for (uint64_t seed = 1; seed <= 150; ++seed) model(seed, seed % 2 ? 1 : 2);
    printf("model by expansion: bad %ld\n", bad);
    printf("plan_host: %s\n", bad ? "FAILED" : "ok");
    return bad != 0;
}
