// count_host.h -- the host decisions of pc_count and pc_query_segment (plastid_counts.hip): which plans the canonical
// stream and the dense vector serve, what a stream or a vector was built from, the dynamic LDS of k_hist_point, the
// capacity of the work lists, the grids, the one-window path, what is cleared in front of a count, and the knobs.
// Nothing here allocates device memory, launches or reads the environment: numbers in, numbers out.
// Plain C++17 (no HIP): tests/count_host_test.cpp compiles it on a machine without a GPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "canon_host.h"
#include "plan_tables.h"   // OutPiece, kModes, kStreamMaxLen, kOpStage, PC_MAP_*

namespace pccount {

// ---- the rules that bin a read at ONE position whatever its length row: fiveprime, threeprime, variable
inline bool point_rule(int kind) { return kind == PC_MAP_FIVE || kind == PC_MAP_THREE || kind == PC_MAP_VAR5; }

// The plans the canonical stream serves (and the dense vector, which adds conditions of its own): over ONE file, under a
// point rule without rows, whose windows are '+' and '-' only -- a '.' window bins both strands by the forward rule:
// another grouping -- and at least one of them.
inline bool stream_plan_conditions(int nfiles, int kind, int rows, uint32_t modes) {
    return nfiles == 1 && point_rule(kind) && rows == 1 && (modes & ~3u) == 0u && modes != 0u;
}

// ---- signatures: what a stream or a vector of a staged file was built from
// The FLAG / MAPQ / NH filter as the setters leave it (pc_set_flag_filter, pc_set_nh_filter); all zero: no filter.
struct FilterState {
    bool ff_on = false;
    uint32_t require = 0, exclude = 0, min_mapq = 0, max_nh = 0;
    bool operator==(const FilterState &o) const {
        return ff_on == o.ff_on && require == o.require && exclude == o.exclude && min_mapq == o.min_mapq && max_nh == o.max_nh;
    }
};

// The rule, the size filter and the stream words (by their generation).  rule_sig fills it: the variable rule has no
// parameter but its tables, and a size filter that is off compares equal whatever bounds it was left with.
struct RuleSig {
    int kind = -1, param = 0, filt_on = 0, filt_min = 0, filt_max = -1;
    uint64_t words_gen = 0;
    std::vector<int32_t> fw, rc;   // the offset tables (variable rule only)
    bool operator==(const RuleSig &o) const {
        return kind == o.kind && param == o.param && filt_on == o.filt_on && filt_min == o.filt_min && filt_max == o.filt_max &&
               words_gen == o.words_gen && fw == o.fw && rc == o.rc;
    }
};

inline RuleSig rule_sig(int kind, int param, int filt_on, int filt_min, int filt_max, uint64_t words_gen, const std::vector<int32_t> &fw,
                        const std::vector<int32_t> &rc) {
    RuleSig s;
    s.kind = kind; s.param = kind == PC_MAP_VAR5 ? 0 : param;
    s.filt_on = filt_on; s.filt_min = filt_on ? filt_min : 0; s.filt_max = filt_on ? filt_max : -1;
    s.words_gen = words_gen;
    if (kind == PC_MAP_VAR5) { s.fw = fw; s.rc = rc; }
    return s;
}

// A canonical stream (build_canonical_stream): the rule, the range of the entry table and the halo it was weighed against.
struct CanonSig {
    RuleSig rule;
    int fast_lo = 0, fast_hi = 0, Ws = 0;
    bool operator==(const CanonSig &o) const { return rule == o.rule && fast_lo == o.fast_lo && fast_hi == o.fast_hi && Ws == o.Ws; }
};

// A dense vector (build_dense_vector): the rule and the FLAG / MAPQ / NH filter whose verdicts the records held.
struct DenseSig {
    RuleSig rule;
    FilterState applied;
    bool operator==(const DenseSig &o) const { return rule == o.rule && applied == o.applied; }
};

// the rule of a canonical stream as canon_host.h takes it (a point rule); `table_len`: entries of the engine's tables
inline pccanon::RuleIn canon_rule_in(const CanonSig &s, int table_len) {
    pccanon::RuleIn r;
    const RuleSig &u = s.rule;
    r.kind = u.kind == PC_MAP_FIVE ? 0 : (u.kind == PC_MAP_THREE ? 1 : 3);
    r.param = u.param;
    r.table_len = (int)std::min<size_t>((size_t)table_len, std::min(u.fw.size(), u.rc.size()));
    r.fw = u.fw.data(); r.rc = u.rc.data();
    r.filt_on = u.filt_on; r.filt_min = u.filt_min; r.filt_max = u.filt_max;
    r.fast_lo = s.fast_lo; r.fast_hi = s.fast_hi;
    return r;
}

// ---- the dynamic LDS of k_hist_point behind its bins: the offset table of the aligned lengths that occur in the data
// (the variable rules; longer reads look the tables up in HBM), the output pieces parked in LDS, the entry table of the
// record stream (the aligned lengths the stream carries) and one dump word per lane.
struct LenRange {   // of one staged file: the aligned lengths present, and those the streams carry (StagedFile)
    int len_min = 65536, len_max = -1, tlen_min = 0, tlen_max = 0;
};
struct HistLds {
    int tab_lo = 0, tab_n = 0, fast_lo = 0, fast_hi = 0;
    size_t table_words = 0;
};

inline HistLds hist_lds_shape(int kind, int table_len, const LenRange *files, int nfiles) {
    HistLds s;
    int lmin = 65536, lmax = -1;
    s.fast_lo = pc::kStreamMaxLen;
    for (int f = 0; f < nfiles; ++f) {
        lmin = std::min(lmin, files[f].len_min); lmax = std::max(lmax, files[f].len_max);
        s.fast_lo = std::min(s.fast_lo, files[f].tlen_min); s.fast_hi = std::max(s.fast_hi, files[f].tlen_max);
    }
    if ((kind == PC_MAP_VAR5 || kind == PC_MAP_STRAT5) && lmax >= lmin) {
        s.tab_lo = lmin;
        s.tab_n = std::max(0, std::min(std::min(lmax, table_len - 1) - lmin + 1, 1024));
    }
    s.fast_lo = std::min(s.fast_lo, s.fast_hi);
    const size_t stage_words = (size_t)pc::kOpStage * sizeof(pc::OutPiece) / sizeof(uint32_t);
    s.table_words = (size_t)((s.tab_n + 3) & ~3) + stage_words + (size_t)(s.fast_hi + 1) * pc::kModes + 64;
    return s;
}

// ... and the bytes with the bins in front: `slot_words` bin words (max_slots x rows) per position of the window, per two
// positions with 16-bit bins (the stratified rule of the work lists)
inline size_t hist_lds_bytes(const HistLds &s, size_t slot_words, int window, bool b16) {
    return (((slot_words * (size_t)window) >> (b16 ? 1 : 0)) + s.table_words) * sizeof(uint32_t);
}

// ---- the work lists of a point-rule count
struct WorkIn {
    int ntiles = 0, nfiles = 0, G = 0, rows = 1;
    uint32_t modes = 0;
    int64_t npos = 0;                 // island positions of the plan
    int64_t nrec = 0, nextra = 0;     // records and extra runs of all files
    int64_t nxlong = 0, ngap = 0;     // ... their long-span reads outside the run stream, their gapped records
    int W = 1, Ws = 1, Wg = 1, Wr = 1;   // the four halos
    int64_t R = 49152, pile = 0;      // PC_WORK_R, PC_PILE (0: 12 R)
    int no_small = 0, small_rows = 0, small_g = 512;   // PC_NO_SMALL, PC_SMALL_ROWS, PC_SMALL_G
    bool stratified = false;          // 16-bit bins, two positions per word (k_hist_point)
};
struct WorkSizes {
    int64_t cap = 0, cap_small = 0;   // capacity of the list of the dense windows, of the sparse ones
    int small_g = 0;                  // window of the sparse class (0: no such class)
    int64_t pile = 0;                 // a 128-nt sub-window with more records than this is merged through the histogram
    bool too_large = false;           // the capacity does not fit the 32-bit slots of the lists
};

inline WorkSizes work_list_sizes(const WorkIn &in) {
    WorkSizes w;
    const int nfiles = in.nfiles, G = in.G;
    const int64_t R = in.R;
    w.pile = in.pile ? in.pile : 12 * R;
    // work-list capacity (an upper bound): a window scanning n records yields at most
    // max(1, 2n/R) items, and every record is scanned by at most 1 + (W+127)/G windows
    const int halo = std::max(std::max(in.W, in.Ws), std::max(in.Wg, in.Wr));
    // (a multi-row plan gives every strand mode of a window a tile of its own -- pc_plan_create, split_modes --
    // so a record is scanned by up to popcount(modes) tiles per window)
    const int tiles_per_window = in.rows > 1 ? std::max(1, __builtin_popcount(in.modes)) : 1;
    const double windows_per_record = (1.0 + (double)(halo + 127) / (double)G) * (double)tiles_per_window;
    w.cap = (int64_t)in.ntiles * nfiles + (int64_t)(2.0 * windows_per_record * (double)in.nrec / (double)R) + nfiles + 64;
    if (in.stratified) {
        // a window that scans more than 65 535 records, runs and list entries is merged, in slices of ONE
        // kind of range each (k_tile_ranges): at most adds / R + 4 items per such window, and fewer than adds / 65 535 of them
        w.cap += (int64_t)(6.0 * windows_per_record * (double)(in.nrec + in.nextra + in.ngap) / (double)R) +
                 (int64_t)in.ntiles * nfiles * (4 + 2 * (in.nxlong / R));
    }
    w.too_large = w.cap >= (int64_t)0xffffffffu;
    // sparse windows: single-wave workgroups with a small LDS window (rows == 1 only)
    // (skipped for dense annotations, where queried positions fill most of every window)
    const bool sparse_plan = (double)in.npos < 0.25 * (double)in.ntiles * (double)G;
    w.small_g = ((in.rows == 1 || in.small_rows) && sparse_plan && !in.no_small) ? std::min(in.small_g, G) : 0;
    w.cap_small = w.small_g ? (int64_t)in.ntiles * nfiles : 0;
    return w;
}

// ---- grids of the two window classes: the whole list capacity, or -- once a count of this plan has shown how many items
// each class queues (same alignments, same knobs: `generation_match`, `known`, counts = heavy, light, small) -- exactly
// those: a sparse annotation leaves most of the capacity empty, and an empty workgroup still costs a dispatch slot.
// Small plans do not track their counts.  `stale_knob` (PC_TEST_STALE_COUNTS) pretends the counts are one light item short.
struct Grids {
    unsigned grid = 0, grid_front = 0, grid_small = 0;
    uint32_t launched[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};   // exact grids: what k_gather_split checks the queued counts against
    bool exact = false;
};

inline Grids choose_grids(int ntiles, bool generation_match, bool known, const uint32_t counts[3], int64_t cap, int64_t cap_small, bool stale_knob) {
    Grids g;
    g.grid = g.grid_front = (unsigned)cap;
    g.grid_small = (unsigned)cap_small;
    if (ntiles < 4096 || !generation_match || !known) return g;
    const uint32_t nh = counts[0], nl = counts[1] - ((stale_knob && counts[1]) ? 1u : 0u), ns = counts[2];
    if ((uint64_t)nh + nl <= (uint64_t)cap && (int64_t)ns <= cap_small) {
        g.grid_front = nh;
        g.grid = std::max(1u, nh + nl);
        g.grid_small = ns;
        g.launched[0] = nh; g.launched[1] = nl; g.launched[2] = ns;
        g.exact = true;
    }
    return g;
}

// waves of k_center2: heavy entries one wave each, `per_wave` light entries per wave (an eighth of the list per XCD);
// counts not read back yet: room for every entry the `nchunks` chunks can make
inline uint64_t center_grid(bool known, uint32_t heavy, uint32_t light, uint64_t nchunks, uint32_t per_wave) {
    uint64_t g2;
    if (known) {
        const uint64_t n8 = ((uint64_t)light + 7) >> 3;
        g2 = (uint64_t)heavy + 8 * ((n8 + per_wave - 1) / per_wave);
    } else g2 = 2 * nchunks + 8;
    return std::max<uint64_t>(g2, 1);
}

// a file with reads beyond a stream entry's 8-bit fields, or with a stream too long for 32-bit byte offsets (`entries`:
// records and runs), takes the instantiation of k_center2 that tests every batch for them
inline bool center_general(int len_max, int64_t entries) { return len_max > 255 || entries >= ((int64_t)1 << 28); }

// ---- a plan of ONE window over one file is one launch -- not under the stratified rule: its 16-bit bins rely on the
// work lists, which cut or merge a window that scans more than 65 535 records
inline bool single_window(int ntiles, int nfiles, int kind, int debug_work, int no_single) {
    return ntiles == 1 && nfiles == 1 && !debug_work && !no_single && kind != PC_MAP_STRAT5;
}

// ---- what is cleared in front of a count.  The output: k_dense_gather (items) writes every position of every segment,
// zeros included: only gaps between slices are cleared.  k_dense_gather_chunks writes every element of the output, the
// gaps too: nothing is.  The window kernels write their outputs exactly once: only positions that belong to no tile
// (unknown contig, clipped coordinates), gaps the caller left between slices and accumulators need a zero fill.
enum OutPath { kOutItems, kOutChunks, kOutWindows };
inline bool out_needs_memset(OutPath path, bool has_sums, bool out_needs_zero, int64_t covered, int64_t out_elems) {
    if (path == kOutChunks || !out_elems) return false;
    if (path == kOutItems) return covered != out_elems;
    return has_sums || out_needs_zero || covered != out_elems;
}
// a large compact histogram is not cleared as a whole: k_clear_split zeroes the slices of the merged windows behind every
// k_tile_ranges, which is all that is ever read of it
inline bool hist_lazy(bool center, int64_t hist_bytes, int64_t lazy_bytes, int hist_memset) {
    return !center && hist_bytes >= lazy_bytes && !hist_memset;
}
// a count from the dense vector goes by chunks where the plan has a chunk table for this vector (no overlapping output
// ranges) and the output block is line aligned -- the chunk kernel's stores are whole lines -- else by items
inline bool dense_by_chunks(bool chunks_ok, bool ids_match, int dense_items, uintptr_t out_addr) {
    return chunks_ok && ids_match && !dense_items && (out_addr & 127u) == 0;
}

// ---- tuning and diagnostic knobs.  The engine reads them from the environment ONCE, at pc_create -- the query path is
// advertised at tens of microseconds per call and does not look at the environment; pc_reload_knobs() re-reads them
// (tests and experiments drive the scheduling paths with them).  `lookup`: getenv, or a test's table.
struct Knobs {
    int tile_g = 0;            // PC_TILE_G: window size (0: chosen from the LDS budget)
    int64_t work_r = 49152;    // PC_WORK_R: records per work item (192 KiB of the 4-byte stream)
    int64_t pile = 0;          // PC_PILE: records of a 128-nt sub-window beyond which it is merged through the histogram (0: 12 R)
    int no_small = 0;          // PC_NO_SMALL: no single-wave class for sparse windows
    int small_rows = 0;        // PC_SMALL_ROWS: 1 = multi-row plans (stratified rule) may use the single-wave class too
    int64_t ranges_cg16_max = (int64_t)1 << 19;   // PC_RANGES_CG16_MAX: k_tile_ranges gives a window sixteen lanes while windows x 16 stays within this many threads
    int ranges_cg1 = 0;        // PC_RANGES_CG1: one thread per window in k_tile_ranges whatever the plan's size (tests compare the two forms)
    int64_t first_sync_spare = 65536;   // PC_FIRST_SYNC_SPARE: spare work-list slots from which the first count of a plan reads its item counts back before it launches
    int hist_memset = 0;       // PC_HIST_MEMSET: the compact histogram of a large plan is cleared as a whole before its first count (round 5) instead of slice by slice
    int64_t hist_lazy_bytes = (int64_t)64 << 20;   // PC_HIST_LAZY_BYTES: size from which it is cleared slice by slice (tests: 1)
    int no_stream_probe = 0;   // PC_NO_STREAM_PROBE: keep the engine's streams as created (see settle_streams)
    int no_compact = 0;        // PC_NO_COMPACT: no compact stream -- files staged (or re-filtered) from then on are counted record by record (tests compare the two)
    double compact_keep = 0.9; // PC_COMPACT_KEEP: a file that keeps more than this share of its records as entries gets no compact stream (build_compact_stream)
    int no_canon = 0;          // PC_NO_CANON: no canonical stream -- eligible plans stream what the others do (A/B runs in one build; tests compare the two)
    int no_dense = 0;          // PC_NO_DENSE: no dense vector -- eligible plans go through the window kernels (A/B runs in one build; tests compare the two)
    int dense_items = 0;       // PC_DENSE_ITEMS: the dense vector serves every plan by items (k_dense_gather), none by chunks (A/B runs in one build; tests compare the two)
    int dense_debug = 0;       // PC_DENSE_DEBUG: print what dense_for_plan decided and from which figures (stderr)
    int no_single = 0;         // PC_NO_SINGLE: one-window plans go through the work lists like any other (tests compare the two paths)
    int plan_build = 0;        // PC_PLAN_BUILD=host|gpu: where pc_plan_create builds the tables (default: on the GPU from 8 192 segments)
    int small_g = 512;         // PC_SMALL_G: queried span a single-wave window may have
    int64_t small_n = 8192;    // PC_SMALL_N: records a single-wave window may scan (C4: 1.25 ms at 2048, 1.22 at 8192, 1.21 at 32768)
    int debug_work = 0;        // PC_DEBUG_WORK: print the queued work items per class (stderr; synchronises)
    int test_stale_counts = 0; // PC_TEST_STALE_COUNTS: pretend the cached work counts are one light item short (exercises the exact-grid guard)
    int center_t1 = 8;         // PC_CENTER_T1 / PC_CENTER_T2: center chunks with more than T1 x (T1*T2 x) the mean candidate
    int center_t2 = 4;         //   count are cut into 4 (8) sub-chunks
    int64_t center_floor = 32768; // PC_CENTER_FLOOR: stream entries below which a chunk is never cut (a wave alone replays ~50 k per ms)
    int center_lds = 0;        // PC_CENTER_LDS: bytes of (unused) LDS per k_center2 workgroup -- an occupancy throttle for experiments
    int center_per_wave = 0;   // (reserved)
    int center_debug = 0;      // PC_CENTER_DEBUG: wall-clock span of every dispatched wave of k_center2, printed after the launch (synchronises)
    void load(const char *(*lookup)(const char *)) {
        *this = Knobs();
        if (const char *env = lookup("PC_TILE_G")) tile_g = std::max(256, atoi(env) / 256 * 256);
        if (const char *env = lookup("PC_WORK_R")) work_r = std::max(1024, atoi(env));
        if (const char *env = lookup("PC_PILE")) pile = std::max<int64_t>(work_r, atoll(env));
        no_small = lookup("PC_NO_SMALL") ? 1 : 0;
        if (const char *env = lookup("PC_SMALL_ROWS")) small_rows = atoi(env);
        no_single = lookup("PC_NO_SINGLE") ? 1 : 0;
        no_compact = lookup("PC_NO_COMPACT") ? 1 : 0;
        no_canon = lookup("PC_NO_CANON") ? 1 : 0;
        no_dense = lookup("PC_NO_DENSE") ? 1 : 0;
        dense_items = lookup("PC_DENSE_ITEMS") ? 1 : 0;
        dense_debug = lookup("PC_DENSE_DEBUG") ? 1 : 0;
        if (const char *env = lookup("PC_COMPACT_KEEP")) compact_keep = std::min(1.0, std::max(0.0, atof(env)));
        no_stream_probe = lookup("PC_NO_STREAM_PROBE") ? 1 : 0;
        hist_memset = lookup("PC_HIST_MEMSET") ? 1 : 0;
        if (const char *env = lookup("PC_HIST_LAZY_BYTES")) hist_lazy_bytes = std::max<int64_t>(1, atoll(env));
        ranges_cg1 = lookup("PC_RANGES_CG1") ? 1 : 0;
        if (const char *env = lookup("PC_RANGES_CG16_MAX")) ranges_cg16_max = atoll(env);
        if (const char *env = lookup("PC_FIRST_SYNC_SPARE")) first_sync_spare = atoll(env);
        if (const char *env = lookup("PC_PLAN_BUILD")) plan_build = std::strcmp(env, "host") == 0 ? 1 : (std::strcmp(env, "gpu") == 0 ? 2 : 0);
        if (const char *env = lookup("PC_SMALL_G")) small_g = std::max(64, atoi(env) / 64 * 64);
        if (const char *env = lookup("PC_SMALL_N")) small_n = std::max(64, atoi(env));
        debug_work = lookup("PC_DEBUG_WORK") ? 1 : 0;
        test_stale_counts = lookup("PC_TEST_STALE_COUNTS") ? 1 : 0;
        if (const char *env = lookup("PC_CENTER_T1")) center_t1 = std::max(8, atoi(env));
        if (const char *env = lookup("PC_CENTER_T2")) center_t2 = std::max(1, atoi(env));
        if (const char *env = lookup("PC_CENTER_FLOOR")) center_floor = std::max(64, atoi(env));
        center_debug = lookup("PC_CENTER_DEBUG") ? 1 : 0;
        if (const char *env = lookup("PC_CENTER_LDS")) center_lds = std::max(0, atoi(env));
    }
};

} // namespace pccount
