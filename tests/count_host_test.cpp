// count_host_test.cpp -- plastid_amd/csrc/count_host.h on a machine without a GPU (tests/test_count_host.py compiles it
// under the address and undefined-behaviour sanitizers and runs it).  Every expected value is a literal worked by hand
// from the formulas of pc_count as they stood before the header existed; none is produced by calling the header.
// Prints "count_host: ok".
#include "count_host.h"

#include <cstdio>
#include <map>
#include <string>

using namespace pccount;

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)
#define CHECK_EQ(got, want)                                                          \
    do {                                                                             \
        const long long g__ = (long long)(got), w__ = (long long)(want);             \
        if (g__ != w__) { fprintf(stderr, "%s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #got, g__, w__); ++failures; } \
    } while (0)

static void check_shape(const HistLds &s, int tab_lo, int tab_n, int fast_lo, int fast_hi, size_t table_words) {
    CHECK_EQ(s.tab_lo, tab_lo); CHECK_EQ(s.tab_n, tab_n); CHECK_EQ(s.fast_lo, fast_lo); CHECK_EQ(s.fast_hi, fast_hi);
    CHECK_EQ(s.table_words, table_words);
}

static void test_lds() {
    static_assert(pc::kOpStage == 32 && sizeof(pc::OutPiece) == 40 && pc::kModes == 4 && pc::kStreamMaxLen == 255, "the literals below assume these");
    // the output pieces parked in LDS: 32 x 40 bytes = 320 words; the dump words: 64
    const LenRange ribo{25, 35, 25, 35};
    // variable rule: lengths 25 .. 35 -> 11 table entries, rounded to 12 words; entry table (35 + 1) x 4 modes = 144
    const HistLds v = hist_lds_shape(PC_MAP_VAR5, 100, &ribo, 1);
    check_shape(v, 25, 11, 25, 35, 12 + 320 + 144 + 64);
    CHECK_EQ(v.table_words, 540);
    CHECK_EQ(hist_lds_bytes(v, 1, 4096, false), 18544);   // (4 096 + 540) x 4
    CHECK_EQ(hist_lds_bytes(v, 1, 4096, true), 10352);    // (2 048 + 540) x 4: 16-bit bins, two positions per word
    CHECK_EQ(hist_lds_bytes(v, 3, 4096, false), 51312);   // three bin words per position: (12 288 + 540) x 4
    CHECK_EQ(hist_lds_bytes(v, 3, 512, true), 5232);      // (768 + 540) x 4
    CHECK_EQ(hist_lds_bytes(v, 1, 0, false), 2160);       // no sparse class: the tables alone
    // the stratified rule keeps the same offset table
    check_shape(hist_lds_shape(PC_MAP_STRAT5, 100, &ribo, 1), 25, 11, 25, 35, 540);
    // fiveprime, threeprime, center: no offset table
    check_shape(hist_lds_shape(PC_MAP_FIVE, 100, &ribo, 1), 0, 0, 25, 35, 0 + 320 + 144 + 64);
    check_shape(hist_lds_shape(PC_MAP_THREE, 0, &ribo, 1), 0, 0, 25, 35, 528);
    check_shape(hist_lds_shape(PC_MAP_CENTER, 100, &ribo, 1), 0, 0, 25, 35, 528);
    // the engine's tables end before the longest read: lengths 25 .. 29 -> 5 entries in 8 words; ... before the shortest: none
    check_shape(hist_lds_shape(PC_MAP_VAR5, 30, &ribo, 1), 25, 5, 25, 35, 8 + 320 + 144 + 64);
    check_shape(hist_lds_shape(PC_MAP_VAR5, 25, &ribo, 1), 25, 0, 25, 35, 528);
    check_shape(hist_lds_shape(PC_MAP_VAR5, 26, &ribo, 1), 25, 1, 25, 35, 4 + 320 + 144 + 64);
    // a length range wider than the cap of 1 024 entries; the streams carry 10 .. 255: entry table 256 x 4
    const LenRange wide{10, 3000, 10, 255};
    check_shape(hist_lds_shape(PC_MAP_VAR5, 10000, &wide, 1), 10, 1024, 10, 255, 1024 + 320 + 1024 + 64);
    const LenRange at_cap{10, 1033, 10, 255}, below_cap{10, 1032, 10, 255};
    CHECK_EQ(hist_lds_shape(PC_MAP_VAR5, 10000, &at_cap, 1).tab_n, 1024);
    CHECK_EQ(hist_lds_shape(PC_MAP_VAR5, 10000, &below_cap, 1).tab_n, 1023);
    // two files whose ranges differ: the union of both -- 20 .. 40, 21 entries in 24 words, entry table 41 x 4 = 164
    const LenRange two[2] = {{20, 30, 20, 30}, {28, 40, 28, 40}};
    check_shape(hist_lds_shape(PC_MAP_STRAT5, 100, two, 2), 20, 21, 20, 40, 24 + 320 + 164 + 64);
    // ... one of which has no read in its streams (its stream range is 0, 0): the entry table starts at 0
    const LenRange two0[2] = {{20, 30, 20, 30}, {300, 400, 0, 0}};
    check_shape(hist_lds_shape(PC_MAP_FIVE, 0, two0, 2), 0, 0, 0, 30, 0 + 320 + 124 + 64);
    // no reads at all (len_max < len_min), no file at all: no offset table, an entry table of length 0 alone
    const LenRange none{65536, -1, 0, 0};
    check_shape(hist_lds_shape(PC_MAP_VAR5, 100, &none, 1), 0, 0, 0, 0, 0 + 320 + 4 + 64);
    check_shape(hist_lds_shape(PC_MAP_VAR5, 100, nullptr, 0), 0, 0, 0, 0, 388);
}

static WorkIn base_work() {   // ten windows of 4 096 over one file of a million reads of 35 nt
    WorkIn in;
    in.ntiles = 10; in.nfiles = 1; in.G = 4096; in.rows = 1; in.modes = 1u; in.npos = 40960;
    in.nrec = 1000000; in.W = 35; in.Ws = 35; in.Wg = 1; in.Wr = 1;
    return in;
}

static void check_sizes(const WorkSizes &w, int64_t cap, int64_t cap_small, int small_g, int64_t pile, bool too_large) {
    CHECK_EQ(w.cap, cap); CHECK_EQ(w.cap_small, cap_small); CHECK_EQ(w.small_g, small_g); CHECK_EQ(w.pile, pile); CHECK_EQ(w.too_large, too_large);
}

// The capacities marked (GPU) were printed by the library before this header existed, under PC_DEBUG_WORK=1 on an
// MI355X, for an engine in exactly the state of the case (docs/history.md has the lines).
static void test_capacity() {
    // windows per record 1 + (35 + 127) / 4096 = 1.03955078125; 2 x that x 10^6 / 49 152 = 42.29 -> 42
    // cap = 10 x 1 + 42 + 1 + 64 = 117 (GPU); every window is queried in full: not sparse
    check_sizes(work_list_sizes(base_work()), 117, 0, 0, 12 * 49152, false);
    {   // the halo is the largest of the four
        WorkIn in = base_work(); in.W = 1; in.Ws = 1; in.Wg = 1; in.Wr = 35;
        CHECK_EQ(work_list_sizes(in).cap, 117);
        in.Wr = 1; in.Wg = 35; CHECK_EQ(work_list_sizes(in).cap, 117);
        in.Wg = 1; CHECK_EQ(work_list_sizes(in).cap, 10 + 41 + 1 + 64);   // 2 x (1 + 128 / 4096) x 10^6 / 49 152 = 41.96
    }
    {   // the sparse-plan boundary npos = 0.25 x 10 x 4096 = 10 240: strictly below it the single-wave class exists (GPU: 117 both,
        // ten small items below, none at the boundary)
        WorkIn in = base_work(); in.small_g = 1024;
        in.npos = 10239; check_sizes(work_list_sizes(in), 117, 10, 1024, 589824, false);
        in.npos = 10240; check_sizes(work_list_sizes(in), 117, 0, 0, 589824, false);
        in.npos = 10239; in.no_small = 1; check_sizes(work_list_sizes(in), 117, 0, 0, 589824, false);   // PC_NO_SMALL (GPU: 117, no small item)
        in.no_small = 0; in.pile = 70000; CHECK_EQ(work_list_sizes(in).pile, 70000);                      // PC_PILE
    }
    {   // small_g > G: PC_TILE_G=256, PC_SMALL_G=512 -- 2 x (1 + 162 / 256) x 10^6 / 49 152 = 66.44 -> 66; cap = 10 + 66 + 1 + 64 = 141 (GPU)
        WorkIn in = base_work(); in.G = 256; in.small_g = 512; in.npos = 600;   // 600 < 0.25 x 10 x 256 = 640
        check_sizes(work_list_sizes(in), 141, 10, 256, 589824, false);
        in.npos = 640; check_sizes(work_list_sizes(in), 141, 0, 0, 589824, false);
    }
    {   // two files of a million each: 10 x 2 + 84 (84.60) + 2 + 64 = 170 (GPU); the sparse list has a slot per window and file
        WorkIn in = base_work(); in.nfiles = 2; in.nrec = 2000000;
        check_sizes(work_list_sizes(in), 170, 0, 0, 589824, false);
        in.npos = 100; check_sizes(work_list_sizes(in), 170, 20, 512, 589824, false);
    }
    {   // stratified, three rows, windows in '+', '-' and '.' (a tile per mode: 5 windows -> 15 tiles), R = 1 024, 104 096 reads
        // of which 2 048 gapped records (300 nt: the halo) and 2 048 long-span reads outside the run stream:
        //   windows per record (1 + 427 / 4096) x 3 = 3.312744140625
        //   15 + int(2 x 3.3127 x 104 096 / 1 024 = 673.52) + 1 + 64                          =  753
        //   + int(6 x 3.3127 x (104 096 + 0 + 2 048) / 1 024 = 2 060.32) + 15 x (4 + 2 x 2)   = 2 180      cap = 2 933 (GPU)
        WorkIn in;
        in.ntiles = 15; in.nfiles = 1; in.G = 4096; in.rows = 3; in.modes = 7u; in.npos = 61440;
        in.nrec = 104096; in.nextra = 0; in.nxlong = 2048; in.ngap = 2048;
        in.W = 300; in.Ws = 30; in.Wg = 300; in.Wr = 1; in.R = 1024; in.stratified = true;
        check_sizes(work_list_sizes(in), 2933, 0, 0, 12288, false);
        in.nextra = 500; CHECK_EQ(work_list_sizes(in).cap, 753 + 2070 + 120);   // 6 x 3.3127 x 106 644 / 1 024 = 2 070.03
        in.nextra = 0; in.nxlong = 2047; CHECK_EQ(work_list_sizes(in).cap, 753 + 2060 + 15 * (4 + 2 * 1));
        in.nxlong = 2048;
        // the same plan under a rule without 16-bit bins (rows > 1 still gives every mode its tile)
        in.stratified = false; CHECK_EQ(work_list_sizes(in).cap, 753);
        // one row: one tile per window whatever the modes -- int(2 x 1.104248046875 x 104 096 / 1 024 = 224.51)
        in.rows = 1; CHECK_EQ(work_list_sizes(in).cap, 15 + 224 + 1 + 64);
        // sparse plans of several rows have no single-wave class unless PC_SMALL_ROWS says so (GPU: 2 933 with it, too)
        in.rows = 3; in.stratified = true; in.npos = 7680;
        check_sizes(work_list_sizes(in), 2933, 0, 0, 12288, false);
        in.small_rows = 1; in.small_g = 1024; check_sizes(work_list_sizes(in), 2933, 15, 1024, 12288, false);
    }
    {   // too large for the 32-bit slots: 2 M tiles x 2 files x (4 + 2 x 600) = 4 816 000 000 alone
        //   4 000 000 + int(2 x 3.3127 x 10^9 / 1 024 = 6 470 203.4) + 2 + 64 + int(6 x 3.3127 x 10^9 / 1 024 = 19 410 610.2) + 4 816 000 000
        WorkIn in;
        in.ntiles = 2000000; in.nfiles = 2; in.G = 4096; in.rows = 3; in.modes = 7u; in.npos = 1;
        in.nrec = 1000000000; in.nxlong = 1024 * 600; in.W = 300; in.R = 1024; in.stratified = true;
        const WorkSizes w = work_list_sizes(in);
        CHECK_EQ(w.cap, 4845880879LL);
        CHECK(w.too_large);
        // ... and the smallest list there is: one window, no record -- 1 + 0 + 1 + 64
        WorkIn fit; fit.ntiles = 1; fit.nfiles = 1; fit.G = 4096; fit.nrec = 0; fit.npos = 4096;
        CHECK_EQ(work_list_sizes(fit).cap, 66);
        CHECK(!work_list_sizes(fit).too_large);
    }
}

static void check_grids(const Grids &g, unsigned grid, unsigned front, unsigned small, uint32_t l0, uint32_t l1, uint32_t l2, bool exact) {
    CHECK_EQ(g.grid, grid); CHECK_EQ(g.grid_front, front); CHECK_EQ(g.grid_small, small);
    CHECK_EQ(g.launched[0], l0); CHECK_EQ(g.launched[1], l1); CHECK_EQ(g.launched[2], l2); CHECK_EQ(g.exact, exact);
}

static void test_grids() {
    const uint32_t none = 0xffffffffu;
    const uint32_t fits[3] = {100, 2000, 300};
    // counts unknown, wrong generation, a small plan: the whole capacity
    check_grids(choose_grids(5000, true, false, nullptr, 9000, 5000, false), 9000, 9000, 5000, none, none, none, false);
    check_grids(choose_grids(5000, false, true, fits, 9000, 5000, false), 9000, 9000, 5000, none, none, none, false);
    check_grids(choose_grids(4095, true, true, fits, 9000, 5000, false), 9000, 9000, 5000, none, none, none, false);
    // counts that fit: heavy items in front, heavy + light workgroups, the small class its own
    check_grids(choose_grids(4096, true, true, fits, 9000, 5000, false), 2100, 100, 300, 100, 2000, 300, true);
    const uint32_t zero[3] = {0, 0, 0};
    check_grids(choose_grids(4096, true, true, zero, 9000, 0, false), 1, 0, 0, 0, 0, 0, true);   // (a grid of at least one workgroup)
    const uint32_t full[3] = {1000, 8000, 5000}, over[3] = {1001, 8000, 5000}, over_small[3] = {1000, 8000, 5001};
    check_grids(choose_grids(5000, true, true, full, 9000, 5000, false), 9000, 1000, 5000, 1000, 8000, 5000, true);
    check_grids(choose_grids(5000, true, true, over, 9000, 5000, false), 9000, 9000, 5000, none, none, none, false);
    check_grids(choose_grids(5000, true, true, over_small, 9000, 5000, false), 9000, 9000, 5000, none, none, none, false);
    // PC_TEST_STALE_COUNTS: one light item short, where there is one
    const uint32_t nolight[3] = {5, 0, 7}, light[3] = {5, 10, 7};
    check_grids(choose_grids(5000, true, true, nolight, 9000, 5000, true), 5, 5, 7, 5, 0, 7, true);
    check_grids(choose_grids(5000, true, true, light, 9000, 5000, true), 14, 5, 7, 5, 9, 7, true);
    check_grids(choose_grids(5000, true, true, light, 9000, 5000, false), 15, 5, 7, 5, 10, 7, true);
    // k_center2: heavy entries a wave each, the light ones in eight parts
    CHECK_EQ(center_grid(true, 3, 0, 100, 1), 3);
    CHECK_EQ(center_grid(true, 3, 1, 100, 1), 11);
    CHECK_EQ(center_grid(true, 3, 8, 100, 1), 11);
    CHECK_EQ(center_grid(true, 3, 9, 100, 1), 19);
    CHECK_EQ(center_grid(true, 0, 0, 100, 1), 1);
    CHECK_EQ(center_grid(true, 3, 9, 100, 4), 11);     // 2 per part, 4 per wave: one wave per part
    CHECK_EQ(center_grid(true, 3, 40, 100, 4), 19);    // 5 per part: two waves per part
    CHECK_EQ(center_grid(false, 3, 9, 100, 1), 208);   // not known: 2 x chunks + 8
    CHECK_EQ(center_grid(false, 0, 0, 0, 1), 8);
    CHECK_EQ(center_grid(true, 0xffffffffu, 0xffffffffu, 0, 1), 0xffffffffULL + 8 * 0x20000000ULL);   // (64-bit arithmetic)
    CHECK(!center_general(255, 0) && center_general(256, 0));
    CHECK(!center_general(30, ((int64_t)1 << 28) - 1) && center_general(30, (int64_t)1 << 28));
}

static void test_conditions() {
    // "a plan over ONE file, under a point rule without rows (fiveprime, threeprime, variable), whose windows are '+' and
    // '-' only": modes 1 ('+'), 2 ('-') and 3 (both) of the sixteen masks; kinds 0, 1 and 3 of the five
    const bool kind_ok[5] = {true, true, false, true, false};
    int n_true = 0;
    for (int nfiles = 1; nfiles <= 2; ++nfiles)
        for (int kind = 0; kind < 5; ++kind)
            for (int rows = 1; rows <= 2; ++rows)
                for (uint32_t modes = 0; modes < 16; ++modes) {
                    const bool want = nfiles == 1 && kind_ok[kind] && rows == 1 && (modes == 1 || modes == 2 || modes == 3);
                    const bool got = stream_plan_conditions(nfiles, kind, rows, modes);
                    if (got != want) { fprintf(stderr, "stream_plan_conditions(%d, %d, %d, %u) = %d, expected %d\n", nfiles, kind, rows, modes, got, want); ++failures; }
                    n_true += got;
                }
    CHECK_EQ(n_true, 9);   // three rules x three masks
    CHECK(!stream_plan_conditions(0, PC_MAP_FIVE, 1, 1u) && !stream_plan_conditions(1, PC_MAP_FIVE, 0, 1u) && !stream_plan_conditions(1, PC_MAP_FIVE, 1, 16u));
    CHECK(point_rule(PC_MAP_FIVE) && point_rule(PC_MAP_THREE) && point_rule(PC_MAP_VAR5) && !point_rule(PC_MAP_CENTER) && !point_rule(PC_MAP_STRAT5) && !point_rule(-1));
    // one window over one file, no diagnostics, not forbidden, not stratified: 4 of the 120 combinations
    n_true = 0;
    for (int ntiles = 0; ntiles <= 2; ++ntiles)
        for (int nfiles = 1; nfiles <= 2; ++nfiles)
            for (int kind = 0; kind < 5; ++kind)
                for (int dbg = 0; dbg <= 1; ++dbg)
                    for (int no = 0; no <= 1; ++no) n_true += single_window(ntiles, nfiles, kind, dbg, no);
    CHECK_EQ(n_true, 4);
    CHECK(single_window(1, 1, PC_MAP_FIVE, 0, 0) && single_window(1, 1, PC_MAP_THREE, 0, 0) && single_window(1, 1, PC_MAP_CENTER, 0, 0) && single_window(1, 1, PC_MAP_VAR5, 0, 0));
    CHECK(!single_window(1, 1, PC_MAP_STRAT5, 0, 0) && !single_window(1, 1, PC_MAP_FIVE, 1, 0) && !single_window(1, 1, PC_MAP_FIVE, 0, 1));
    // the output memset: items -- gaps only; chunks -- never; window kernels -- gaps, positions outside every tile, accumulators
    CHECK(!out_needs_memset(kOutItems, false, false, 100, 100) && out_needs_memset(kOutItems, false, false, 99, 100));
    CHECK(!out_needs_memset(kOutItems, true, true, 100, 100));          // (what only the window kernels leave unwritten)
    CHECK(!out_needs_memset(kOutItems, false, false, 0, 0));
    CHECK(!out_needs_memset(kOutChunks, false, false, 99, 100) && !out_needs_memset(kOutChunks, true, true, 99, 100));
    CHECK(!out_needs_memset(kOutWindows, false, false, 100, 100));
    CHECK(out_needs_memset(kOutWindows, true, false, 100, 100) && out_needs_memset(kOutWindows, false, true, 100, 100) && out_needs_memset(kOutWindows, false, false, 99, 100));
    CHECK(!out_needs_memset(kOutWindows, true, true, 0, 0));            // nothing to clear
    // the lazy histogram: from hist_lazy_bytes on, not for the center rule, not under PC_HIST_MEMSET
    CHECK(hist_lazy(false, 64 << 20, 64 << 20, 0) && !hist_lazy(false, (64 << 20) - 1, 64 << 20, 0));
    CHECK(!hist_lazy(true, 64 << 20, 64 << 20, 0) && !hist_lazy(false, 64 << 20, 64 << 20, 1));
    CHECK(hist_lazy(false, 1, 1, 0) && !hist_lazy(false, 0, 1, 0));
    // the chunk gather: a chunk table for this vector, not PC_DENSE_ITEMS, a line-aligned output block
    CHECK(dense_by_chunks(true, true, 0, 0x1000) && dense_by_chunks(true, true, 0, 0x1080));
    CHECK(!dense_by_chunks(false, true, 0, 0x1000) && !dense_by_chunks(true, false, 0, 0x1000) && !dense_by_chunks(true, true, 1, 0x1000));
    CHECK(!dense_by_chunks(true, true, 0, 0x1040) && !dense_by_chunks(true, true, 0, 0x1001) && !dense_by_chunks(true, true, 0, 0x107f));
}

struct SigIn {   // what an engine and a file hand to the signatures
    int kind = PC_MAP_VAR5, param = 12, filt_on = 1, filt_min = 26, filt_max = 32;
    uint64_t words_gen = 7;
    std::vector<int32_t> fw{-1, 12, 13}, rc{-1, 13, 12};
    int fast_lo = 25, fast_hi = 35, Ws = 35;
    FilterState applied;
};
static CanonSig canon_of(const SigIn &e) {
    CanonSig s;
    s.rule = rule_sig(e.kind, e.param, e.filt_on, e.filt_min, e.filt_max, e.words_gen, e.fw, e.rc);
    s.fast_lo = e.fast_lo; s.fast_hi = e.fast_hi; s.Ws = e.Ws;
    return s;
}
static DenseSig dense_of(const SigIn &e) {
    DenseSig s;
    s.rule = rule_sig(e.kind, e.param, e.filt_on, e.filt_min, e.filt_max, e.words_gen, e.fw, e.rc);
    s.applied = e.applied;
    return s;
}

static void test_signatures() {
    const SigIn a;
    CHECK(canon_of(a) == canon_of(a) && dense_of(a) == dense_of(a));
    // one field at a time; `canon` / `dense`: the signature must see the change (the rule's fields: both)
    auto differs = [&](const char *what, const SigIn &b, bool canon, bool dense) {
        if ((canon_of(a) == canon_of(b)) == canon) { fprintf(stderr, "CanonSig: a change of %s %s\n", what, canon ? "goes unseen" : "is seen"); ++failures; }
        if ((dense_of(a) == dense_of(b)) == dense) { fprintf(stderr, "DenseSig: a change of %s %s\n", what, dense ? "goes unseen" : "is seen"); ++failures; }
    };
    { SigIn b = a; b.kind = PC_MAP_FIVE; differs("kind", b, true, true); }
    { SigIn b = a; b.filt_on = 0; differs("filt_on", b, true, true); }
    { SigIn b = a; b.filt_min = 27; differs("filt_min", b, true, true); }
    { SigIn b = a; b.filt_max = -1; differs("filt_max", b, true, true); }
    { SigIn b = a; b.words_gen = 8; differs("words_gen", b, true, true); }
    { SigIn b = a; b.fw[1] = 11; differs("fw", b, true, true); }
    { SigIn b = a; b.rc.push_back(3); differs("rc", b, true, true); }
    { SigIn b = a; b.fast_lo = 24; differs("fast_lo", b, true, false); }
    { SigIn b = a; b.fast_hi = 36; differs("fast_hi", b, true, false); }
    { SigIn b = a; b.Ws = 36; differs("Ws", b, true, false); }
    { SigIn b = a; b.applied.ff_on = true; differs("applied.ff_on", b, false, true); }
    { SigIn b = a; b.applied.require = 2; differs("applied.require", b, false, true); }
    { SigIn b = a; b.applied.exclude = 0x400; differs("applied.exclude", b, false, true); }
    { SigIn b = a; b.applied.min_mapq = 10; differs("applied.min_mapq", b, false, true); }
    { SigIn b = a; b.applied.max_nh = 1; differs("applied.max_nh", b, false, true); }
    // the variable rule has no parameter: whatever the engine holds compares equal; its tables are compared
    { SigIn b = a; b.param = 0; differs("param (variable rule)", b, false, false); }
    CHECK_EQ(canon_of(a).rule.param, 0);
    CHECK(canon_of(a).rule.fw == a.fw && canon_of(a).rule.rc == a.rc);
    // fiveprime / threeprime: the parameter counts, the tables (left over from an earlier rule) do not
    SigIn five = a; five.kind = PC_MAP_FIVE;
    { SigIn b = five; b.param = 13; CHECK(!(canon_of(five) == canon_of(b)) && !(dense_of(five) == dense_of(b))); }
    { SigIn b = five; b.fw.clear(); b.rc[0] = 5; CHECK(canon_of(five) == canon_of(b) && dense_of(five) == dense_of(b)); }
    CHECK_EQ(canon_of(five).rule.param, 12);
    CHECK(canon_of(five).rule.fw.empty() && canon_of(five).rule.rc.empty());
    { SigIn b = five; b.kind = PC_MAP_THREE; CHECK(!(canon_of(five) == canon_of(b))); }
    // a size filter that is off: 0, 0, -1 whatever bounds it was left with
    SigIn off = a; off.filt_on = 0;
    { SigIn b = off; b.filt_min = 1; b.filt_max = 99; CHECK(canon_of(off) == canon_of(b) && dense_of(off) == dense_of(b)); }
    CHECK_EQ(canon_of(off).rule.filt_on, 0); CHECK_EQ(canon_of(off).rule.filt_min, 0); CHECK_EQ(canon_of(off).rule.filt_max, -1);
    CHECK_EQ(canon_of(a).rule.filt_min, 26); CHECK_EQ(canon_of(a).rule.filt_max, 32);
    // a fresh signature (nothing built yet) equals none that rule_sig makes: kind -1
    CHECK(!(CanonSig() == canon_of(a)) && !(DenseSig() == dense_of(five)));
    // the rule as canon_host.h takes it: kinds 0 / 1 / 3, tables no longer than the engine's table_len
    const pccanon::RuleIn r = canon_rule_in(canon_of(a), 2);
    CHECK_EQ(r.kind, 3); CHECK_EQ(r.table_len, 2); CHECK_EQ(r.filt_on, 1); CHECK_EQ(r.filt_min, 26); CHECK_EQ(r.filt_max, 32);
    CHECK_EQ(r.fast_lo, 25); CHECK_EQ(r.fast_hi, 35);
    CHECK_EQ(canon_rule_in(canon_of(a), 100).table_len, 3);
    const pccanon::RuleIn r5 = canon_rule_in(canon_of(five), 100);
    CHECK_EQ(r5.kind, 0); CHECK_EQ(r5.param, 12); CHECK_EQ(r5.table_len, 0);
    { SigIn b = five; b.kind = PC_MAP_THREE; CHECK_EQ(canon_rule_in(canon_of(b), 100).kind, 1); }
}

static std::map<std::string, std::string> g_env;
static const char *fake_env(const char *name) {
    const auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}
static Knobs knobs_with(const char *name, const char *value) {
    g_env.clear();
    g_env[name] = value;
    Knobs k;
    k.load(fake_env);
    return k;
}

static void test_knobs() {
    g_env.clear();
    Knobs d;
    d.tile_g = 999; d.no_small = 1; d.compact_keep = 0.1;
    d.load(fake_env);   // an empty environment: the defaults, whatever the object held
    CHECK_EQ(d.tile_g, 0); CHECK_EQ(d.work_r, 49152); CHECK_EQ(d.pile, 0); CHECK_EQ(d.no_small, 0); CHECK_EQ(d.small_rows, 0);
    CHECK_EQ(d.ranges_cg16_max, 524288); CHECK_EQ(d.ranges_cg1, 0); CHECK_EQ(d.first_sync_spare, 65536); CHECK_EQ(d.hist_memset, 0);
    CHECK_EQ(d.hist_lazy_bytes, 67108864); CHECK_EQ(d.no_stream_probe, 0); CHECK_EQ(d.no_compact, 0); CHECK(d.compact_keep == 0.9);
    CHECK_EQ(d.no_canon, 0); CHECK_EQ(d.no_dense, 0); CHECK_EQ(d.dense_items, 0); CHECK_EQ(d.dense_debug, 0); CHECK_EQ(d.no_single, 0);
    CHECK_EQ(d.plan_build, 0); CHECK_EQ(d.small_g, 512); CHECK_EQ(d.small_n, 8192); CHECK_EQ(d.debug_work, 0); CHECK_EQ(d.test_stale_counts, 0);
    CHECK_EQ(d.center_t1, 8); CHECK_EQ(d.center_t2, 4); CHECK_EQ(d.center_floor, 32768); CHECK_EQ(d.center_lds, 0); CHECK_EQ(d.center_debug, 0);
    // multiples of 256, at least 256
    CHECK_EQ(knobs_with("PC_TILE_G", "300").tile_g, 256); CHECK_EQ(knobs_with("PC_TILE_G", "255").tile_g, 256);
    CHECK_EQ(knobs_with("PC_TILE_G", "256").tile_g, 256); CHECK_EQ(knobs_with("PC_TILE_G", "511").tile_g, 256);
    CHECK_EQ(knobs_with("PC_TILE_G", "512").tile_g, 512); CHECK_EQ(knobs_with("PC_TILE_G", "1000").tile_g, 768);
    CHECK_EQ(knobs_with("PC_TILE_G", "0").tile_g, 256); CHECK_EQ(knobs_with("PC_TILE_G", "4096").tile_g, 4096);
    // multiples of 64, at least 64
    CHECK_EQ(knobs_with("PC_SMALL_G", "100").small_g, 64); CHECK_EQ(knobs_with("PC_SMALL_G", "63").small_g, 64);
    CHECK_EQ(knobs_with("PC_SMALL_G", "64").small_g, 64); CHECK_EQ(knobs_with("PC_SMALL_G", "127").small_g, 64);
    CHECK_EQ(knobs_with("PC_SMALL_G", "128").small_g, 128); CHECK_EQ(knobs_with("PC_SMALL_G", "1024").small_g, 1024);
    // floors
    CHECK_EQ(knobs_with("PC_WORK_R", "1").work_r, 1024); CHECK_EQ(knobs_with("PC_WORK_R", "1023").work_r, 1024);
    CHECK_EQ(knobs_with("PC_WORK_R", "1024").work_r, 1024); CHECK_EQ(knobs_with("PC_WORK_R", "1025").work_r, 1025);
    CHECK_EQ(knobs_with("PC_SMALL_N", "1").small_n, 64); CHECK_EQ(knobs_with("PC_SMALL_N", "64").small_n, 64); CHECK_EQ(knobs_with("PC_SMALL_N", "65").small_n, 65);
    CHECK_EQ(knobs_with("PC_CENTER_T1", "7").center_t1, 8); CHECK_EQ(knobs_with("PC_CENTER_T1", "8").center_t1, 8); CHECK_EQ(knobs_with("PC_CENTER_T1", "9").center_t1, 9);
    CHECK_EQ(knobs_with("PC_CENTER_T2", "0").center_t2, 1); CHECK_EQ(knobs_with("PC_CENTER_T2", "1").center_t2, 1); CHECK_EQ(knobs_with("PC_CENTER_T2", "2").center_t2, 2);
    CHECK_EQ(knobs_with("PC_CENTER_FLOOR", "63").center_floor, 64); CHECK_EQ(knobs_with("PC_CENTER_FLOOR", "64").center_floor, 64);
    CHECK_EQ(knobs_with("PC_CENTER_FLOOR", "65").center_floor, 65);
    CHECK_EQ(knobs_with("PC_CENTER_LDS", "-1").center_lds, 0); CHECK_EQ(knobs_with("PC_CENTER_LDS", "0").center_lds, 0); CHECK_EQ(knobs_with("PC_CENTER_LDS", "1").center_lds, 1);
    CHECK_EQ(knobs_with("PC_HIST_LAZY_BYTES", "0").hist_lazy_bytes, 1); CHECK_EQ(knobs_with("PC_HIST_LAZY_BYTES", "-5").hist_lazy_bytes, 1);
    CHECK_EQ(knobs_with("PC_HIST_LAZY_BYTES", "1").hist_lazy_bytes, 1); CHECK_EQ(knobs_with("PC_HIST_LAZY_BYTES", "2").hist_lazy_bytes, 2);
    CHECK_EQ(knobs_with("PC_HIST_LAZY_BYTES", "8589934592").hist_lazy_bytes, 8589934592LL);   // (64-bit)
    // the pile is at least one work item -- of the work-item size of the same environment
    CHECK_EQ(knobs_with("PC_PILE", "100").pile, 49152); CHECK_EQ(knobs_with("PC_PILE", "49152").pile, 49152); CHECK_EQ(knobs_with("PC_PILE", "49153").pile, 49153);
    {
        g_env.clear(); g_env["PC_PILE"] = "100"; g_env["PC_WORK_R"] = "2048";
        Knobs k; k.load(fake_env);
        CHECK_EQ(k.work_r, 2048); CHECK_EQ(k.pile, 2048);
        g_env["PC_PILE"] = "2049"; k.load(fake_env); CHECK_EQ(k.pile, 2049);
    }
    // a share between 0 and 1
    CHECK(knobs_with("PC_COMPACT_KEEP", "-1").compact_keep == 0.0 && knobs_with("PC_COMPACT_KEEP", "0").compact_keep == 0.0);
    CHECK(knobs_with("PC_COMPACT_KEEP", "0.5").compact_keep == 0.5);
    CHECK(knobs_with("PC_COMPACT_KEEP", "1").compact_keep == 1.0 && knobs_with("PC_COMPACT_KEEP", "2").compact_keep == 1.0);
    // host | gpu | anything else: the default
    CHECK_EQ(knobs_with("PC_PLAN_BUILD", "host").plan_build, 1); CHECK_EQ(knobs_with("PC_PLAN_BUILD", "gpu").plan_build, 2);
    CHECK_EQ(knobs_with("PC_PLAN_BUILD", "cpu").plan_build, 0); CHECK_EQ(knobs_with("PC_PLAN_BUILD", "").plan_build, 0);
    // plain numbers
    CHECK_EQ(knobs_with("PC_SMALL_ROWS", "1").small_rows, 1); CHECK_EQ(knobs_with("PC_SMALL_ROWS", "0").small_rows, 0);
    CHECK_EQ(knobs_with("PC_RANGES_CG16_MAX", "123").ranges_cg16_max, 123); CHECK_EQ(knobs_with("PC_RANGES_CG16_MAX", "0").ranges_cg16_max, 0);
    CHECK_EQ(knobs_with("PC_FIRST_SYNC_SPARE", "0").first_sync_spare, 0); CHECK_EQ(knobs_with("PC_FIRST_SYNC_SPARE", "99999999999").first_sync_spare, 99999999999LL);
    // switches: set is on, whatever the value
    CHECK_EQ(knobs_with("PC_NO_SMALL", "0").no_small, 1); CHECK_EQ(knobs_with("PC_NO_SMALL", "").no_small, 1);
    CHECK_EQ(knobs_with("PC_NO_SINGLE", "1").no_single, 1); CHECK_EQ(knobs_with("PC_NO_COMPACT", "1").no_compact, 1);
    CHECK_EQ(knobs_with("PC_NO_CANON", "1").no_canon, 1); CHECK_EQ(knobs_with("PC_NO_DENSE", "1").no_dense, 1);
    CHECK_EQ(knobs_with("PC_DENSE_ITEMS", "1").dense_items, 1); CHECK_EQ(knobs_with("PC_DENSE_DEBUG", "1").dense_debug, 1);
    CHECK_EQ(knobs_with("PC_NO_STREAM_PROBE", "1").no_stream_probe, 1); CHECK_EQ(knobs_with("PC_HIST_MEMSET", "1").hist_memset, 1);
    CHECK_EQ(knobs_with("PC_RANGES_CG1", "1").ranges_cg1, 1); CHECK_EQ(knobs_with("PC_DEBUG_WORK", "1").debug_work, 1);
    CHECK_EQ(knobs_with("PC_TEST_STALE_COUNTS", "1").test_stale_counts, 1); CHECK_EQ(knobs_with("PC_CENTER_DEBUG", "1").center_debug, 1);
    CHECK_EQ(knobs_with("PC_NO_SMALL", "1").no_single, 0);   // (and no other)
    // load() twice: the second environment alone
    Knobs k = knobs_with("PC_TILE_G", "1024");
    CHECK_EQ(k.tile_g, 1024);
    g_env.clear(); g_env["PC_WORK_R"] = "4096";
    k.load(fake_env);
    CHECK_EQ(k.tile_g, 0); CHECK_EQ(k.work_r, 4096);
    g_env.clear();
    k.load(fake_env);
    CHECK_EQ(k.work_r, 49152);
}

int main() {
    test_lds();
    test_capacity();
    test_grids();
    test_conditions();
    test_signatures();
    test_knobs();
    if (failures) { fprintf(stderr, "count_host: %d failure(s)\n", failures); return 1; }
    printf("count_host: ok\n");
    return 0;
}
