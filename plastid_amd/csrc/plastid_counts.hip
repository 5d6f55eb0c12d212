// plastid_counts.hip -- host side of the C ABI declared in include/plastid_counts.h.
//
// Owns device memory, builds the interval plan (islands -> genome tiles ->
// pieces), launches the kernels of pc_kernels.hip.h on the engine's stream and
// times them with HIP events.  There is no CPU counting path in this file: every
// count comes out of a HIP kernel.
//
// Host-side structure, in file order:
//   device_util.hip.h (included)   the plumbing of this file and of every driver included at its end: fail / HIP_TRY,
//                                  DevPool / DevBuf / PinnedBuf (device blocks recycled per engine, one page-locked
//                                  buffer: a plan of one short segment costs API calls, not bytes; the policy is
//                                  pool_host.h), TransferRing (the caller's columns cross PCIe through a ring of
//                                  page-locked pieces), room, DrainOnExit / finish_phase, the hipcub seam
//   StagedFile / pc_engine / pc_plan   what the entry points keep in HBM
//   plan_build_gpu                 the tables of a large plan as kernels, sorts and scans (plan_kernels.hip.h), phase
//                                  by phase: upload, segments, islands, pieces + tiles, output pieces, the block;
//                                  plan_upload for a host-built plan; the center and gather tables on first use
//   pc_create / pc_destroy         streams, events, the engine's pool
//   pc_add_alignment_file          staging, phase by phase (stage_file): columns to HBM while the contig column stays on
//                                  the host and becomes ntid + 1 record bounds (scan_contigs), then kernels only
//                                  (stage_kernels.hip.h: validation, 8-byte records, run stream, statistics;
//                                  pc_kernels.hip.h: record stream, side lists, linear-index tables)
//   pc_plan_create                 segments -> islands -> windows -> output pieces, all tables of a
//                                  plan in one device block (host builder: plan_host.h; GPU: plan_build_gpu)
//   pc_count                       k_tile_ranges -> k_hist_point (two classes, two streams) ->
//                                  k_gather_split, or the three center kernels + k_gather, or -- a '+' / '-' plan
//                                  under a point rule over a file with a dense vector -- k_dense_gather alone
//   pc_rle / pc_total / pc_mapped_reads / pc_warn_flags   consumers of a finished count
//                                  (pc_counts_export and pc_track_set_counts, revision 17: track_decoder.hip.h)
#include "pc_kernels.hip.h"
#include "plan_kernels.hip.h"
#include "stage_kernels.hip.h"
#include "dense_kernels.hip.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <chrono>
#include <future>
#include <functional>
#include <condition_variable>
#include <map>
#include <mutex>
#include <unistd.h>
#include <mutex>
#include <sched.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <fcntl.h>
#include <cerrno>
#include <thread>
#include <vector>

#include "plastid_counts.h"
#include "host_util.h"
#include "plan_host.h"
#include "canon_host.h"
#include "count_host.h"
#include "dense_host.h"
#include "device_util.hip.h"

using namespace pc;

namespace {

static int stage_threads(int64_t n) {
    int t = std::min(usable_cpus(), 32);
    if (const char *env = getenv("PC_STAGE_THREADS")) t = std::max(1, atoi(env));
    return (int)std::max<int64_t>(1, std::min<int64_t>(t, n / (1 << 20) + 1)); // a thread is not worth < 1 M records
}

// what a canonical stream / a dense vector of a staged file was built from, and the filter state in the latter (count_host.h)
using pccount::CanonSig;
using pccount::DenseSig;
using pccount::FilterState;

struct StagedFile {
    int64_t n = 0, nrun = 0, nlong = 0;
    int W = 1;               // max reference span of the records scanned by the window kernels
    int64_t max_span = 1;    // over all records (long ones too)
    DevBuf<uint2> rec;
    DevBuf<uint32_t> blk_off;
    DevBuf<int2> blk;
    DevBuf<int64_t> tid_bounds;
    DevBuf<uint32_t> long_idx;
    DevBuf<int32_t> long_tid;
    DevBuf<int32_t> long_pmax;
    DevBuf<int64_t> long_tid_bounds;
    DevBuf<uint4> long_rec;
    int64_t ngap = 0;
    DevBuf<uint4> gap_rec;
    DevBuf<int4> gap_runs, long_runs; // first two aligned runs of every side-list record
    DevBuf<int64_t> gap_tid_bounds;
    DevBuf<uint32_t> lin_tab, glin_tab, llin_tab, plin_tab;
    DevBuf<int64_t> lin_off;
    std::vector<int64_t> len_hist; // records per aligned length (host), for cheap warn pre-checks
    int len_min = 65536, len_max = -1; // aligned lengths present
    int slen_min = 0, slen_max = 0;    // ... among the records the 4-byte stream carries
    int tlen_min = 0, tlen_max = 0;    // ... among those and the reads of the run stream (range of the LDS entry table)
    DevBuf<uint32_t> stream;           // 4-byte record stream (pc::stream_word), padded with skip words
    // compact stream (build_compact_stream): duplicate reads as one entry with a multiplicity, and its linear index;
    // rebuilt whenever the stream words are rewritten.  cn = its entries, -1: none (nothing worth merging: the point
    // rules stream the records)
    DevBuf<uint32_t> cstream, clin_tab;
    int64_t cn = -1;
    uint64_t words_gen = 0;            // counts the rewrites of the stream words (build_compact_stream runs behind every one)
    // canonical stream (build_canonical_stream): one entry per (strand, mapped position) under ONE rule and size filter,
    // built at the first count of an eligible plan and kept until `ksig` no longer holds.  kn = its entries, -1: none
    // (not built, or not worth it under this signature); kid: changes with every build (pc_plan::WorkKey)
    DevBuf<uint32_t> kstream, klin_tab;
    DevBuf<int16_t> kshift;
    int64_t kn = -1;
    bool ksig_valid = false;
    CanonSig ksig;
    uint64_t kid = 0;
    // dense vector (build_dense_vector, dense_host.h): one 16-bit cell per (contig, strand, position of the extent) with
    // the count of that position under ONE rule, size filter and filter state; cells that hold 65 535 or more escape to
    // the sorted overflow list.  Built at the first count of an eligible plan, kept until `dsig` no longer holds, dropped
    // with the file.  The layout (extents, cell offsets) depends on the staged reads alone.
    std::vector<int64_t> tid_end;      // furthest aligned end per contig (0: no read)
    std::vector<int64_t> dext, dcell_off;   // extents [ntid], first cell of (contig, strand) [2 ntid + 1]; empty: not laid out yet
    int64_t dcells = -1;               // cells of the layout
    DevBuf<int64_t> d_dext, d_dcell_off;
    DevBuf<uint16_t> dense;
    DevBuf<uint32_t> dovf_key, dovf_val;
    uint32_t dn_ovf = 0;
    bool dsig_valid = false;
    DenseSig dsig;
    uint64_t did = 0;                  // changes with every build, unique in the process (pc_plan::ditems_id)
    size_t nlin = 0;                   // entries of every linear-index table
    // run stream (aligned runs of multi-run reads with L <= kStreamMaxLen, sorted by contig and run start)
    int64_t nrunrec = 0;
    int Wr = 1;                        // longest run it carries
    DevBuf<uint2> run_rec;
    DevBuf<uint32_t> run_recidx;       // record of every run (for pc_update_flags)
    DevBuf<uint32_t> rlin_tab;
    // long-span reads outside the run stream: the point rules' own long list
    int64_t nxlong = 0;
    int Wg = 1;                        // longest span in the gapped-record list
    DevBuf<uint4> xlong_rec;
    DevBuf<int4> xlong_runs;
    DevBuf<uint32_t> xllin_tab, xplin_tab;
    // wide records (aligned length > 65 535 or > 255 aligned runs): their true {length, run count} next to every
    // long-list entry, and by record index (ascending) for the kernels that start from a record
    int64_t nwide = 0;
    DevBuf<uint2> long_wide, xlong_wide, wide_val;
    DevBuf<uint32_t> wide_rec;
    // SAM FLAG word and MAPQ of every record (pc_set_alignment_sam, or straight from the device decoder): what the
    // vectorised FLAG / MAPQ filter reads
    DevBuf<uint16_t> sam_flag;
    DevBuf<uint8_t> sam_mapq;
    bool have_sam = false;
    DevBuf<uint16_t> sam_nh;           // the NH:i tag of every record (0: none): pc_set_alignment_nh, or straight from the device decoder
    bool have_nh = false;
    // the filter whose verdicts the exclusion bits of the staged records hold right now (none: the caller's bits alone);
    // `applied_valid` false: the columns those verdicts were read from have been replaced since
    FilterState applied;
    bool applied_valid = true;
    // center streams (built at the first center-rule count that needs them; dropped when the host-side filters change)
    DevBuf<uint2> cs_ent[3];
    DevBuf<uint32_t> cs_soff[3];
    int64_t cs_n[3] = {-1, -1, -1};    // entries, -1: not built
    int cs_nib[3] = {-1, -1, -1};      // the nibble the entries were trimmed with
    FileView view() const {
        FileView v;
        v.rec = rec.p; v.blk_off = blk_off.p; v.blk = blk.p; v.tid_bounds = tid_bounds.p;
        v.stream = stream.p;
        v.cstream = cn >= 0 ? cstream.p : nullptr; v.clin_tab = cn >= 0 ? clin_tab.p : nullptr;
        v.long_idx = long_idx.p; v.long_tid = long_tid.p; v.long_pmax = long_pmax.p;
        v.long_tid_bounds = long_tid_bounds.p; v.long_rec = long_rec.p; v.n = n; v.nlong = nlong;
        v.gap_rec = gap_rec.p; v.gap_tid_bounds = gap_tid_bounds.p; v.ngap = ngap;
        v.gap_runs = gap_runs.p; v.long_runs = long_runs.p;
        v.lin_tab = lin_tab.p; v.glin_tab = glin_tab.p; v.llin_tab = llin_tab.p; v.plin_tab = plin_tab.p; v.lin_off = lin_off.p;
        v.run_rec = run_rec.p; v.rlin_tab = rlin_tab.p; v.nrunrec = nrunrec;
        v.xlong_rec = xlong_rec.p; v.xlong_runs = xlong_runs.p; v.xllin_tab = xllin_tab.p; v.xplin_tab = xplin_tab.p; v.nxlong = nxlong;
        for (int k = 0; k < 3; ++k) {
            v.cs_ent[k] = cs_n[k] >= 0 ? cs_ent[k].p : nullptr; v.cs_soff[k] = cs_n[k] >= 0 ? cs_soff[k].p : nullptr;
            v.cs_total[k] = cs_n[k] >= 0 ? (uint32_t)cs_n[k] : 0u;
            v.cs_indirect[k] = len_max > 255 ? 1u : 0u;   // (reads beyond the 8-bit fields of a stream entry)
        }
        v.long_wide = nwide ? long_wide.p : nullptr; v.xlong_wide = nwide ? xlong_wide.p : nullptr;
        v.wide_rec = wide_rec.p; v.wide_val = wide_val.p; v.nwide = nwide;
        return v;
    }
};

// Counts a kernel queued on the GPU, read back without a wait: page-locked words, the event behind the copy into them,
// whether that copy has arrived (`known`: host[] holds the counts) and the engine work_generation they belong to
// (0: none in flight).
struct QueuedCounts {
    uint32_t *host = nullptr;
    size_t words = 0;
    hipEvent_t ev = nullptr;
    bool known = false;
    uint64_t generation = 0;
    QueuedCounts() = default;
    QueuedCounts(const QueuedCounts &) = delete;
    QueuedCounts &operator=(const QueuedCounts &) = delete;
    ~QueuedCounts() {
        if (ev) (void)hipEventDestroy(ev);
        if (host) (void)hipHostFree(host);
    }
    int ensure(size_t n) {
        if (host) return PC_OK;
        HIP_TRY(hipHostMalloc((void **)&host, n * sizeof(uint32_t), hipHostMallocDefault));
        words = n;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        return PC_OK;
    }
    int request(hipStream_t st, const uint32_t *src) {   // (behind ensure)
        known = false;
        HIP_TRY(hipMemcpyAsync(host, src, words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(ev, st));
        return PC_OK;
    }
    // has the read-back arrived?  Deterministic for its plan while the generation stands: no further read-backs
    bool poll() {
        if (host && !known && hipEventQuery(ev) == hipSuccess) known = true;
        return known;
    }
};

} // namespace

using pccount::Knobs;   // tuning and diagnostic knobs (count_host.h), read from the environment at pc_create and by pc_reload_knobs
static const char *env_lookup(const char *name) { return getenv(name); }

static void destroy_tracks_of(pc_engine *e);   // (track_decoder.hip.h)
static void destroy_summaries_of(pc_engine *e);   // (bigwig_summary.hip.h)

struct pc_engine {
    DevPool pool;   // first member: outlives every buffer of the engine
    DevBuf<uint8_t> plan_scratch[3];   // working arrays of the GPU plan builder (per segment, per piece, per output piece): grown, never shrunk
    Knobs knobs;
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t side_stream = nullptr;   // the single-wave kernel of sparse windows runs beside the main one
    static constexpr int kAux = 3;
    hipStream_t aux_stream[kAux] = {nullptr, nullptr, nullptr};   // the upload pieces of the BAM decoder are inflated on these and the main stream in turn, so that one launch fills the tail of the launches before it
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::vector<hipStream_t> parked_streams;   // streams settle_streams traded away (they shared a hardware queue with the main one)
    hipEvent_t ev_pinned = nullptr;      // end of the last copy out of `pinned`
    hipEvent_t ev[8] = {};
    std::vector<StagedFile *> files;
    std::vector<pc_track *> tracks;   // the count tracks made on this engine (track_decoder.hip.h): they go with it
    std::vector<pc_bigwig_summary *> summaries;   // the summary readers opened on this engine (bigwig_summary.hip.h): their tables come from its pool
    DevBuf<uint8_t> cx_text;          // the last pc_counts_export (track_decoder.hip.h): its text waits in HBM for pc_counts_export_read
    int64_t cx_bytes = -1;
    int64_t cx_stats[4] = {0, 0, 0, 0};      // lines, runs / non-zero cells, values listed for the host, bytes
    double cx_ms[6] = {0, 0, 0, 0, 0, 0};    // run heads | sums + selects | listed values | lengths + offsets | format | read-back
    int ntid = 0;
    DevBuf<FileView> d_files;
    bool files_dirty = true;
    // mapping
    bool have_map = false;
    int kind = PC_MAP_CENTER, param = 0, min_len = 25, max_len = 35, rows = 1, table_len = 0;
    std::vector<int32_t> h_fw, h_rc;
    DevBuf<int32_t> d_fw, d_rc;
    int filt_on = 0, filt_min = 0, filt_max = -1;
    int norm_on = 0;
    double norm_sum = 1.0;
    DevBuf<double> d_inv; // 1.0/m, m = 0..65535 (host-computed IEEE quotients)
    DevBuf<double> d_invh; // the same halved (exact): what the center kernel's fma doubles again
    DevBuf<double> d_cvalh; // [256] half the value of a read by aligned length under the current rule and size filter (k_center_vals)
    // scratch for counting
    DevBuf<uint32_t> d_counters; // [1] unmappable count, [7] sink of the stream probe, [12] exact-grid guard (work counts: pc_plan::d_wcounters)
    DevBuf<uint8_t> d_flags;     // staging buffer of pc_update_flags
    uint8_t *q_host = nullptr;   // pc_query_segment: page-locked buffer the kernel writes the counts of one window into (+ the flag word behind them)
    void *q_dev = nullptr;       //   ... and its address on the device
    uint32_t q_seq = 0;
    bool ff_on = false;          // pc_set_flag_filter: keep (flag & require) == require && (flag & exclude) == 0 && mapq >= min_mapq
    uint32_t ff_require = 0, ff_exclude = 0, ff_min_mapq = 0;
    uint32_t ff_max_nh = 0;      // pc_set_nh_filter: keep only reads with an NH:i tag of at most this many reported alignments (0: no such test)
    bool filter_on() const { return ff_on || ff_max_nh != 0u; }
    FilterState filter_state() const {
        FilterState s;
        s.ff_on = ff_on; s.require = ff_require; s.exclude = ff_exclude; s.min_mapq = ff_min_mapq; s.max_nh = ff_max_nh;
        return s;
    }
    bool pinned_busy = false;
    PinnedBuf pinned;            // host side of the plan-table upload (reused: ev_pinned is waited for before it is rewritten)
    PinnedBuf bam_ring[2];       // page-locked halves the image of a large BAM file crosses PCIe through (filled by all host threads)
    hipEvent_t ev_ring[2] = {nullptr, nullptr};
    uint64_t work_generation = 1; // bumped by whatever changes the work list of a plan (alignment files, knobs)
    size_t max_lds = 64 * 1024; // LDS a workgroup may use (160 KiB on gfx950)
    DevBuf<double> d_partial;
    DevBuf<Unmappable> d_unmap;
    double last_ms[6] = {0, 0, 0, 0, 0, 0};
    bool timing_valid = false;
    int prof_level = 0;      // pc_set_profiling: 0 no events, 1 whole call + histogram/center kernel, 2 every phase
    int timed_level = 0;     // level the last pc_count was recorded with
    int64_t last_alg_bytes = 0;
    bool last_count_dense = false;       // the last pc_count was served from the dense vector of file 0 (pc_dense_cells)
    int last_dense_path = PC_DENSE_PATH_NONE;   // ... and by which kernel (pc_dense_path)
    bool want_center_steps = false;      // pc_center_replay_steps: the next center count reports the replay steps it executed
    int64_t center_steps = 0, center_waves = 0;

    MapParams params() const {
        MapParams mp;
        mp.kind = kind; mp.param = param; mp.min_len = min_len; mp.max_len = max_len; mp.rows = rows;
        mp.filt_on = filt_on; mp.filt_min = filt_min; mp.filt_max = filt_max;
        mp.table_len = table_len; mp.fw = d_fw.p; mp.rc = d_rc.p;
        return mp;
    }
    int max_over_files(int StagedFile::*field) const {
        int w = 1;
        for (auto *f : files) w = std::max(w, f->*field);
        return w;
    }
    int W() const { return max_over_files(&StagedFile::W); }
    int Wg() const { return max_over_files(&StagedFile::Wg); }        // halo of the gapped-record list
    int Wr() const { return max_over_files(&StagedFile::Wr); }        // halo of the run stream: its longest run
    int Ws() const { return max_over_files(&StagedFile::slen_max); }  // halo of the 4-byte record stream: the longest aligned length it carries
};

struct pc_plan {
    pc_engine *e = nullptr;
    int64_t nseg = 0, out_elems = 0, covered = 0;
    int rows = 1, G = 4096;
    uint32_t modes = 0;
    int max_slots = 1;
    int64_t npos = 0; // island positions (hist row length)
    HostPlan host;               // the tables as the host builder made them (empty for a GPU-built plan): the uploads read them, pc_plan_table its gsegs
    size_t n_tiles = 0, n_pieces = 0, n_opieces = 0;   // table sizes (a GPU-built plan keeps its tables in HBM only)
    size_t n_cchunks = 0, n_gchunks = 0;               // ... of the center chunk list and of the gather list, once built
    bool gpu_built = false;      // pc_plan_create built the tables on the GPU (large annotations): they live in HBM only
    bool host_inputs = true;
    DevBuf<uint8_t> d_inputs;    // the caller's segment arrays as uploaded (GPU-built plans)
    DevBuf<GatherSeg> d_gsegs_own;
    bool has_sums = false;       // some slices are summed (out_step 0): the output is an accumulator
    bool out_needs_zero = false; // some queried positions lie outside every tile (unknown contig, clipped)
    // Gather items of the dense vector (dense_host.h): the plan's segments cut into at most 2 048 positions each, with
    // the cells they read.  They depend on the plan and the layout of the file's vector only: built by a kernel at the
    // first count served from a vector, kept while that vector stands (StagedFile::did).
    bool no_dense = false;       // the plan a dense vector is built with: counted by the window kernels
    DevBuf<pcdense::Item> d_ditems;
    uint32_t n_ditems = 0;
    uint64_t ditems_id = 0;      // (0: none)
    // ... and the chunk table beside them (dense_host.h): one descriptor per 1 024 elements of the output, the spans of
    // all chunks in output order.  chunks_ok false: the plan's output ranges overlap, or it has too many spans -- items only
    DevBuf<pcdense::ChunkDesc> d_dchunks;
    DevBuf<pcdense::Span> d_dspans;
    bool chunks_ok = false;
    uint64_t dchunks_id = 0;     // the vector the table was made for (0: none, or not asked for yet: PC_DENSE_ITEMS)
    bool hist_clean = false;     // the WHOLE compact histogram is known to be zero (a lazy count does not need that: it clears the slices it merges)
    bool hist_lazy = false;      // the histogram is large: never cleared as a whole, k_clear_split runs behind every k_tile_ranges
    // GPU-built plans: the center chunks and the gather list wait for the first center count or coordinate export
    bool center_ready = false, gather_ready = false;
    DevBuf<uint8_t> d_tables2, d_tables3;   // ... and live in these blocks (chunks; gather list)
    // host copies for warn evaluation
    std::vector<int32_t> h_tid;
    std::vector<int64_t> h_start, h_end;
    std::vector<uint8_t> h_strand;
    DevBuf<uint8_t> d_tables;   // one block: tiles, pieces, output pieces, chunks, segments, per-tile counters, total
    DevView<Tile> d_tiles;
    DevView<Piece> d_pieces;
    DevView<OutPiece> d_opieces;
    DevView<CenterChunk> d_cchunks;
    DevBuf<uint32_t> d_corder;
    DevBuf<uint32_t> d_ccand;   // candidate records per center chunk
    DevBuf<uint32_t> d_rle_cnt; // run-length encoding of the output: heads per workgroup, their scan,
    DevBuf<int64_t> d_rle_base; // [nwg] bases + [1] total
    DevBuf<int64_t> d_rle_starts;
    DevBuf<unsigned long long> d_rle_values;
    int64_t rle_runs = -1;
    DevBuf<u32x4> d_cranges;    // per (chunk, file): entry range of the near window and candidate range of the long-span list
    DevBuf<u32x2> d_crec;       // per (chunk, file): the near window as a record range (sub-chunks narrow it)
    DevBuf<uint32_t> d_crows;   // per (chunk, file): entry ranges of the chunk's four rows of 16 positions (4 x lo, 4 x hi)
    DevBuf<uint32_t> d_ccounts; // [0] heavy, [1] light entries of the dispatch list, [2..3] sum of the candidate counts, [4..5] entries of all rows, [6..7] 4 x replay steps (row fill)
    DevBuf<CenterSlot> d_cslots; // one descriptor per dispatch entry (plans over one alignment file: k_center2)
    // the center pre-passes (ranges, candidate counts, dispatch order) depend on the plan, the staged files and the
    // knobs only -- not on the mapping rule: kept from count to count while the engine's work generation stands
    uint64_t center_generation = 0;        // (0: no dispatch list yet -- the engine's work_generation starts at 1)
    int center_W = -1;
    int center_nfiles = 0;                 // alignment files the dispatch list was resolved into descriptors for (d_cslots: one per entry and file)
    QueuedCounts center_counts;            // [2]: heavy, light entries of the list (sizes the grids of later counts)
    DevView<GatherSeg> d_gsegs;
    DevView<GatherChunk> d_gchunks;
    DevView<uint32_t> d_tile_items;
    bool tile_items_zero = false;
    // Work lists of the point rules.  They depend on the plan's windows, the staged alignments and the halo of the
    // mapping rule only -- not on the counts -- so they belong to the plan and k_tile_ranges runs once per
    // (plan, WorkKey): a repeated count goes straight to the histogram kernels.
    struct WorkKey {
        uint64_t generation = 0;   // engine work_generation (alignments, host-side filters, knobs)
        int nfiles = 0, G = 0, Wg = 0, Ws = 0, Wr = 0, small_g = 0;
        int64_t R = 0, pile = 0, small_n = 0, cap = 0;
        uint64_t canon = 0;        // StagedFile::kid of the canonical stream the lists index (0: none) -- a rule or filter change rebuilds them
        bool operator==(const WorkKey &o) const {
            return canon == o.canon && generation == o.generation && nfiles == o.nfiles && G == o.G && Wg == o.Wg && Ws == o.Ws && Wr == o.Wr &&
                   small_g == o.small_g && R == o.R && pile == o.pile && small_n == o.small_n && cap == o.cap;
        }
    };
    WorkKey work_key;
    bool work_valid = false;
    DevBuf<WorkItem> d_work, d_work_small;
    DevBuf<FileRange> d_chain, d_chain_small;   // several files: the ranges of files >= 1 of every (joint) work item
    DevView<uint32_t> d_wcounters;              // [0..3] queued heavy, light, small items, long-span candidates
    bool wcounters_zero = false;
    DevView<uint8_t> d_hist; // uint32 or double; inside d_tables when short, else d_hist_own
    DevBuf<uint8_t> d_hist_own;
    DevBuf<uint8_t> d_out;  // int64 or double
    DevBuf<unsigned long long> d_mr_off;   // pc_mapped_reads_batch: mapped reads before every (segment, file) pair
    DevBuf<uint32_t> d_mr_rec;             // ... and their record indices
    int64_t mr_total = -1;
    DevView<uint8_t> d_total;
    int last_dtype = -1;
    bool counted = false;
    // queued work items per class as the last count of this plan left them (a large plan launches exactly
    // that many workgroups next time instead of the whole list capacity)
    QueuedCounts work_counts;            // [8]: heavy, light, small, (diagnostics), [4] windows of the lists that are merged through the compact histogram (what k_gather_split lays out)
    bool exact_grid_used = false;        // some count of this plan launched exact grids: its results are read back with the guard word
    bool guard_pending = false;          // the work lists were rebuilt since the guard word was last read (capacity check)

    explicit pc_plan(pc_engine *eng) : e(eng) {
        DevPool *pl = &eng->pool;
        d_tables.pool = pl; d_corder.pool = pl;
        d_ccand.pool = pl; d_rle_cnt.pool = pl; d_rle_base.pool = pl; d_rle_starts.pool = pl; d_rle_values.pool = pl;
        d_cranges.pool = pl; d_crec.pool = pl; d_crows.pool = pl; d_ccounts.pool = pl; d_cslots.pool = pl; d_hist_own.pool = pl; d_out.pool = pl; d_tables2.pool = pl; d_tables3.pool = pl;
        d_work.pool = pl; d_work_small.pool = pl; d_chain.pool = pl; d_chain_small.pool = pl;
        d_inputs.pool = pl; d_gsegs_own.pool = pl; d_ditems.pool = pl; d_dchunks.pool = pl; d_dspans.pool = pl;
    }
};

namespace {

int refresh_file_views(pc_engine *e) {
    if (!e->files_dirty) return PC_OK;
    std::vector<FileView> v;
    for (auto *f : e->files) v.push_back(f->view());
    PC_TRY(e->d_files.upload(v, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->files_dirty = false;
    return PC_OK;
}

// ---- plans built on the GPU (plan_kernels.hip.h): the host copies of the caller's segment arrays, when a host pass needs them
struct PlanInputLayout {   // the caller's seven segment arrays in one block
    size_t at_tid, at_start, at_end, at_strand, at_off, at_step, at_stride, bytes;
    explicit PlanInputLayout(size_t n) {
        size_t b = 0;
        auto place = [&b](size_t k) { const size_t at = b; b += (k + 255) & ~(size_t)255; return at; };
        at_tid = place(n * 4); at_start = place(n * 8); at_end = place(n * 8); at_strand = place(n);
        at_off = place(n * 8); at_step = place(n); at_stride = place(n * 8);
        bytes = b;
    }
};

int fetch_host_inputs(pc_plan *p) {
    if (p->host_inputs) return PC_OK;
    const size_t n = (size_t)p->nseg;
    const PlanInputLayout L(n);
    HIP_TRY(hipStreamSynchronize(p->e->stream));
    p->h_tid.resize(n); p->h_start.resize(n); p->h_end.resize(n); p->h_strand.resize(n);
    if (n) {
        HIP_TRY(hipMemcpy(p->h_tid.data(), p->d_inputs.p + L.at_tid, n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(p->h_start.data(), p->d_inputs.p + L.at_start, n * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(p->h_end.data(), p->d_inputs.p + L.at_end, n * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(p->h_strand.data(), p->d_inputs.p + L.at_strand, n, hipMemcpyDeviceToHost));
    }
    p->host_inputs = true;
    return PC_OK;
}

struct Bump {   // carves the working arrays of one stage out of one block
    uint8_t *base = nullptr;
    size_t used = 0;
    template <typename T> T *take(size_t n) {
        used = (used + 255) & ~(size_t)255;
        T *q = base ? (T *)(base + used) : nullptr;
        used += n * sizeof(T);
        return q;
    }
};

inline int bits_for(uint64_t v) { int b = 0; while (b < 64 && (v >> b)) ++b; return std::max(b, 1); }

// The plan's block in HBM, as both builders lay it out: tiles, island pieces, output pieces, center chunks, gather
// records, gather list (the last three empty in a GPU-built plan, which makes them on first use), then what arrives
// zeroed -- the per-tile item counters, the work counters, the total and, when it is short, the compact histogram (one
// memset less on the first count).
struct PlanBlockLayout {
    size_t at_tiles, at_pieces, at_opieces, at_cchunks, at_gsegs, at_gchunks, at_items, at_wcounters, at_total, at_hist = 0, bytes = 0;
    bool hist_here;
    PlanBlockLayout(size_t n_tiles, size_t n_pieces, size_t n_opieces, size_t n_cchunks, size_t n_gsegs, size_t n_gchunks, int64_t npos, int rows) {
        auto place = [this](size_t n) { const size_t at = bytes; bytes += (n + 255) & ~(size_t)255; return at; };
        at_tiles = place(n_tiles * sizeof(Tile)); at_pieces = place(n_pieces * sizeof(Piece)); at_opieces = place(n_opieces * sizeof(OutPiece));
        at_cchunks = place(n_cchunks * sizeof(CenterChunk)); at_gsegs = place(n_gsegs * sizeof(GatherSeg)); at_gchunks = place(n_gchunks * sizeof(GatherChunk));
        at_items = place((n_tiles + 1) * sizeof(uint32_t)); at_wcounters = place(64); at_total = place(64);
        const size_t hist_full = (size_t)npos * (size_t)rows * sizeof(double);
        hist_here = hist_full > 0 && hist_full <= 64 * 1024;
        if (hist_here) at_hist = place(hist_full);
    }
    size_t zeroed_bytes() const { return bytes - at_items; }   // from at_items to the end
    void bind(pc_plan *p) const {   // the views of `p` into its block (which is, or is about to be, zeroed from at_items on)
        uint8_t *d = p->d_tables.p;
        p->d_tiles.p = (Tile *)(d + at_tiles); p->d_pieces.p = (Piece *)(d + at_pieces);
        p->d_opieces.p = (OutPiece *)(d + at_opieces); p->d_cchunks.p = (CenterChunk *)(d + at_cchunks);
        p->d_gsegs.p = (GatherSeg *)(d + at_gsegs); p->d_gchunks.p = (GatherChunk *)(d + at_gchunks);
        p->d_tile_items.p = (uint32_t *)(d + at_items); p->d_total.p = d + at_total;
        p->d_wcounters.p = (uint32_t *)(d + at_wcounters);
        p->tile_items_zero = true;
        p->wcounters_zero = true;
        if (hist_here) { p->d_hist.p = d + at_hist; p->hist_clean = true; }
    }
};

// ---- the tables of a plan, built on the GPU, phase by phase.  What the phases share beside the engine and the plan:
// the caller's arrays in HBM, the counters block and its host copy, the working arrays of the three stages -- A per
// segment, B per piece, C per output piece, each carved from one scratch block of the engine with the temporary of
// its scans and sorts at the end -- and the counts the read-backs bring.
struct PlanBuild {
    typedef unsigned long long u64;
    pc_engine *e;
    pc_plan *p;
    const PlanSegments &segs;   // the caller's host arrays
    int64_t out_elems;
    int rows;
    hipStream_t st;
    int ntid;
    size_t n;
    unsigned gseg;              // blocks of a per-segment kernel
    StageClock pclk;
    pcplan::SegIn in;
    pcplan::Misc h, *misc = nullptr;
    Bump A, B, C;
    size_t cub_a = 0, cub_b = 0, cub_c = 0;
    uint8_t *cub_tmp = nullptr, *cub_tmp_b = nullptr, *cub_tmp_c = nullptr;
    u64 *keys = nullptr, *keys2 = nullptr, *ge = nullptr, *pm = nullptr, *island_keys = nullptr;
    uint32_t *ends = nullptr, *ends2 = nullptr, *flags = nullptr, *before = nullptr, *npieces = nullptr, *piece_at = nullptr, *nout = nullptr, *out_at = nullptr;
    pcplan::Island *islands = nullptr;
    int64_t *lens = nullptr, *offs = nullptr;
    u64 *pkeys = nullptr, *pkeys2 = nullptr, *tile_keys = nullptr;
    uint32_t *pidx = nullptr, *pidx2 = nullptr, *new_tile = nullptr, *tbefore = nullptr, *otile = nullptr, *otile2 = nullptr, *oidx = nullptr, *oidx2 = nullptr;
    Piece *praw = nullptr, *psorted = nullptr;
    Tile *tiles_tmp = nullptr;
    OutPiece *oraw = nullptr;
    int G = 0, split_modes = 0;
    size_t n_iv = 0, n_pieces = 0, n_op = 0, n_tiles = 0;
    PlanBuild(pc_engine *eng, pc_plan *plan, const PlanSegments &s, int64_t oe, int r)
        : e(eng), p(plan), segs(s), out_elems(oe), rows(r), st(eng->stream), ntid(eng->ntid), n((size_t)s.n), gseg((unsigned)(((size_t)s.n + 255) / 256)) {}
    // The scans and sorts as `call(tmp, bytes)` (cub_need / cub_run_sized).  A stage asks at an upper bound before its
    // arrays are carved (the pointers are read when the call runs) and runs at the count a read-back brought.
    auto sort_segs(int end_bit) { return [this, end_bit](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, keys, keys2, ends, ends2, (int)n, 0, end_bit, st); }; }
    auto max_ends(size_t cnt) { return [this, cnt](void *t, size_t &b) { return hipcub::DeviceScan::InclusiveScan(t, b, ge, pm, pcplan::GroupMax(), (int)cnt, st); }; }
    template <typename T> auto sum(T *PlanBuild::*from, T *PlanBuild::*to, size_t cnt) {
        return [this, from, to, cnt](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, this->*from, this->*to, (int)cnt, st); };
    }
    auto sort_pieces(int end_bit) { return [this, end_bit](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, pkeys, pkeys2, pidx, pidx2, (int)n_pieces, 0, end_bit, st); }; }
    auto sort_out(int end_bit) { return [this, end_bit](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, otile, otile2, oidx, oidx2, (int)n_op, 0, end_bit, st); }; }
    int read_misc() {   // what the phase queued so far, then the counters
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&h, misc, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return PC_OK;
    }
};

int plan_upload_inputs(PlanBuild &x) {
    pc_plan *p = x.p;
    hipStream_t st = x.st;
    const size_t n = x.n;
    const PlanInputLayout L(n);
    int rc = p->d_inputs.reserve(std::max<size_t>(L.bytes, 256));
    room(rc, p->d_gsegs_own, std::max<size_t>(n, 1));
    if (rc != PC_OK) return rc;
    uint8_t *di = p->d_inputs.p;
    HIP_TRY(hipMemcpyAsync(di + L.at_tid, x.segs.tid, n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(di + L.at_start, x.segs.start, n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(di + L.at_end, x.segs.end, n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(di + L.at_strand, x.segs.strand, n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(di + L.at_off, x.segs.out_off, n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(di + L.at_step, x.segs.out_step, n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(di + L.at_stride, x.segs.row_stride, n * 8, hipMemcpyHostToDevice, st));
    pcplan::SegIn &in = x.in;
    in.tid = (const int32_t *)(di + L.at_tid); in.start = (const int64_t *)(di + L.at_start); in.end = (const int64_t *)(di + L.at_end);
    in.strand = di + L.at_strand; in.out_off = (const int64_t *)(di + L.at_off); in.out_step = (const int8_t *)(di + L.at_step);
    in.row_stride = (const int64_t *)(di + L.at_stride);
    x.pclk.lap("plan(gpu): upload");
    return PC_OK;
}

// stage A: its arrays, then the per-segment records, the sort keys and the first defect
int plan_segments(PlanBuild &x) {
    using namespace pcplan;
    typedef PlanBuild::u64 u64;
    pc_engine *e = x.e;
    pc_plan *p = x.p;
    const size_t n = x.n;
    size_t b = 0;   // (the three 32-bit sums are one instantiation: one of them asks for all)
    PC_TRY(cub_need(x.cub_a, b, x.sort_segs(64)));
    PC_TRY(cub_need(x.cub_a, b, x.max_ends(n)));
    PC_TRY(cub_need(x.cub_a, b, x.sum(&PlanBuild::lens, &PlanBuild::offs, n + 1)));
    PC_TRY(cub_need(x.cub_a, b, x.sum(&PlanBuild::flags, &PlanBuild::before, n + 1)));
    Bump &A = x.A;
    for (int pass = 0; pass < 2; ++pass) {   // (first pass: sizes)
        A.used = 0;
        x.misc = A.take<Misc>(1);
        x.keys = A.take<u64>(n); x.keys2 = A.take<u64>(n); x.ends = A.take<uint32_t>(n); x.ends2 = A.take<uint32_t>(n);
        x.ge = A.take<u64>(n); x.pm = A.take<u64>(n); x.flags = A.take<uint32_t>(n + 1); x.before = A.take<uint32_t>(n + 1);
        x.islands = A.take<Island>(n); x.island_keys = A.take<u64>(n); x.lens = A.take<int64_t>(n + 1); x.offs = A.take<int64_t>(n + 1);
        x.npieces = A.take<uint32_t>(n + 1); x.piece_at = A.take<uint32_t>(n + 1); x.nout = A.take<uint32_t>(n + 1); x.out_at = A.take<uint32_t>(n + 1);
        x.cub_tmp = A.take<uint8_t>(x.cub_a + 256);
        if (pass == 0) {
            PC_TRY(e->plan_scratch[0].reserve(A.used + 256));
            A.base = e->plan_scratch[0].p;
        }
    }
    Misc &h = x.h;
    std::memset(&h, 0, sizeof(h));
    h.first_bad = ~0ull;
    h.max_slots = 1;
    HIP_TRY(hipMemcpyAsync(x.misc, &h, sizeof(h), hipMemcpyHostToDevice, x.st));
    hipLaunchKernelGGL(k_plan_segs, dim3(x.gseg), dim3(256), 0, x.st, x.in, x.segs.n, x.ntid, x.rows, x.out_elems, p->d_gsegs_own.p, x.keys, x.ends, x.misc);
    PC_TRY(x.read_misc());
    if (h.first_bad != ~0ull) {   // the defect of the lowest segment index, as a serial pass reports it
        PlanDefect bad = {(int)(h.first_bad & 0xffu), (int64_t)(h.first_bad >> 8), 0, 0};
        if (bad.kind == kDefectSlice) plan_slice_bounds(x.segs, bad.seg, x.rows, &bad.lo, &bad.hi);
        return fail(PC_ERR_ARG, "%s", plan_defect_message(bad, x.out_elems).c_str());
    }
    p->modes = h.modes;
    p->covered = (int64_t)h.covered;
    p->has_sums = h.has_sums != 0;
    if (!plan_window(x.rows, h.modes, h.n_iv, h.iv_len, e->knobs.tile_g, &p->G))
        return fail(PC_ERR_ARG, "%s", plan_defect_message({kDefectRows, 0, x.rows, 0}, x.out_elems).c_str());
    x.G = p->G;
    x.split_modes = x.rows > 1 ? 1 : 0;
    x.n_iv = (size_t)h.n_iv;
    x.pclk.lap("plan(gpu): segments");
    return PC_OK;
}

// intervals by (contig, mode, start) -> islands, their lengths and pieces; every segment finds its island
int plan_islands(PlanBuild &x) {
    using namespace pcplan;
    pc_plan *p = x.p;
    hipStream_t st = x.st;
    const size_t n = x.n, n_iv = x.n_iv;
    const int G = x.G;
    if (n_iv) {
        const unsigned giv = (unsigned)((n_iv + 255) / 256);
        PC_TRY(cub_run_sized(x.cub_tmp, x.cub_a, x.sort_segs(std::min(64, 33 + bits_for((uint64_t)x.ntid)))));
        hipLaunchKernelGGL(k_group_ends, dim3(giv), dim3(256), 0, st, x.keys2, x.ends2, x.misc, x.ge);
        PC_TRY(cub_run_sized(x.cub_tmp, x.cub_a, x.max_ends(n_iv)));
        hipLaunchKernelGGL(k_island_flags, dim3(giv), dim3(256), 0, st, x.keys2, x.pm, x.misc, x.flags, (int64_t)n_iv);
        PC_TRY(cub_run_sized(x.cub_tmp, x.cub_a, x.sum(&PlanBuild::flags, &PlanBuild::before, n_iv)));
        hipLaunchKernelGGL(k_island_fill, dim3(giv), dim3(256), 0, st, x.keys2, x.pm, x.flags, x.before, x.misc, x.islands, x.island_keys);
        hipLaunchKernelGGL(k_island_lens, dim3(giv), dim3(256), 0, st, x.misc, x.islands, x.lens, x.npieces, G, (int64_t)n_iv);
        PC_TRY(cub_run_sized(x.cub_tmp, x.cub_a, x.sum(&PlanBuild::lens, &PlanBuild::offs, n_iv)));
        PC_TRY(cub_run_sized(x.cub_tmp, x.cub_a, x.sum(&PlanBuild::npieces, &PlanBuild::piece_at, n_iv)));
        hipLaunchKernelGGL(k_island_offsets, dim3(giv), dim3(256), 0, st, x.misc, x.islands, x.offs, x.lens, x.piece_at, x.npieces);
    }
    if (n) {
        hipLaunchKernelGGL(k_seg_island, dim3(x.gseg), dim3(256), 0, st, x.in, x.segs.n, p->d_gsegs_own.p, x.misc, x.islands, x.island_keys, x.nout, G);
        PC_TRY(cub_run_sized(x.cub_tmp, x.cub_a, x.sum(&PlanBuild::nout, &PlanBuild::out_at, n)));
        hipLaunchKernelGGL(k_out_total, dim3(1), dim3(64), 0, st, x.misc, x.out_at, x.nout, x.segs.n);
    }
    PC_TRY(x.read_misc());
    p->npos = (int64_t)x.h.npos;
    p->out_needs_zero = x.h.needs_zero != 0;
    x.n_pieces = x.h.n_pieces; x.n_op = x.h.n_opieces;
    if (x.n_pieces >= 0x7fffffffu || x.n_op >= 0x7fffffffu) return fail(PC_ERR_ARG, "pc_plan_create: too many window pieces");
    x.pclk.lap("plan(gpu): islands");
    return PC_OK;
}

// stage B: the pieces by (contig, window, mode, offset), a tile where the window changes
int plan_pieces_tiles(PlanBuild &x) {
    using namespace pcplan;
    typedef PlanBuild::u64 u64;
    pc_engine *e = x.e;
    hipStream_t st = x.st;
    const size_t n_pieces = x.n_pieces, n_op = x.n_op;
    size_t b = 0;
    PC_TRY(cub_need(x.cub_b, b, x.sort_pieces(64)));
    PC_TRY(cub_need(x.cub_b, b, x.sum(&PlanBuild::new_tile, &PlanBuild::tbefore, n_pieces + 1)));
    PC_TRY(cub_need(x.cub_c, b, x.sort_out(32)));
    Bump &B = x.B, &C = x.C;
    for (int pass = 0; pass < 2; ++pass) {   // (the arrays of stage C beside them: both blocks are had before anything runs)
        B.used = 0; C.used = 0;
        x.pkeys = B.take<u64>(n_pieces); x.pkeys2 = B.take<u64>(n_pieces); x.pidx = B.take<uint32_t>(n_pieces); x.pidx2 = B.take<uint32_t>(n_pieces);
        x.praw = B.take<Piece>(n_pieces); x.psorted = B.take<Piece>(n_pieces); x.new_tile = B.take<uint32_t>(n_pieces + 1); x.tbefore = B.take<uint32_t>(n_pieces + 1);
        x.tiles_tmp = B.take<Tile>(n_pieces); x.tile_keys = B.take<u64>(n_pieces); x.cub_tmp_b = B.take<uint8_t>(x.cub_b + 256);
        x.oraw = C.take<OutPiece>(n_op); x.otile = C.take<uint32_t>(n_op); x.otile2 = C.take<uint32_t>(n_op); x.oidx = C.take<uint32_t>(n_op); x.oidx2 = C.take<uint32_t>(n_op);
        x.cub_tmp_c = C.take<uint8_t>(x.cub_c + 256);
        if (pass == 0) {
            int rc = e->plan_scratch[1].reserve(B.used + 256);
            room(rc, e->plan_scratch[2], C.used + 256);
            if (rc != PC_OK) return rc;
            B.base = e->plan_scratch[1].p; C.base = e->plan_scratch[2].p;
        }
    }
    if (n_pieces) {
        const unsigned gp = (unsigned)((n_pieces + 255) / 256);
        hipLaunchKernelGGL(k_pieces_raw, dim3(gp), dim3(256), 0, st, x.misc, x.islands, x.piece_at, x.G, x.pkeys, x.pidx, x.praw);
        PC_TRY(cub_run_sized(x.cub_tmp_b, x.cub_b, x.sort_pieces(std::min(64, 37 + bits_for((uint64_t)x.ntid)))));
        hipLaunchKernelGGL(k_pieces_sorted, dim3(gp), dim3(256), 0, st, x.misc, x.pkeys2, x.pidx2, x.praw, x.psorted, x.new_tile, x.split_modes, (int64_t)n_pieces);
        PC_TRY(cub_run_sized(x.cub_tmp_b, x.cub_b, x.sum(&PlanBuild::new_tile, &PlanBuild::tbefore, n_pieces)));
        hipLaunchKernelGGL(k_tile_fill, dim3(gp), dim3(256), 0, st, x.misc, x.pkeys2, x.psorted, x.new_tile, x.tbefore, x.G, x.split_modes, x.tiles_tmp, x.tile_keys);
    }
    return PC_OK;
}

// stage C: the output pieces of every segment, by tile
int plan_out_pieces(PlanBuild &x) {
    using namespace pcplan;
    pc_plan *p = x.p;
    if (x.n_op) {
        hipLaunchKernelGGL(k_out_raw, dim3(x.gseg), dim3(256), 0, x.st, x.in, x.segs.n, p->d_gsegs_own.p, x.misc, x.tile_keys, x.out_at, x.nout, x.G, x.split_modes, x.oraw, x.otile, x.oidx);
        PC_TRY(cub_run_sized(x.cub_tmp_c, x.cub_c, x.sort_out(std::min(32, bits_for((uint64_t)x.n_pieces)))));
    }
    PC_TRY(x.read_misc());
    x.n_tiles = x.h.n_tiles;
    p->max_slots = (int)x.h.max_slots;
    p->n_tiles = x.n_tiles; p->n_pieces = x.n_pieces; p->n_opieces = x.n_op;
    x.pclk.lap("plan(gpu): pieces + tiles + output pieces");
    return PC_OK;
}

// the plan's block
int plan_block(PlanBuild &x) {
    using namespace pcplan;
    pc_plan *p = x.p;
    hipStream_t st = x.st;
    const size_t n_tiles = x.n_tiles, n_pieces = x.n_pieces, n_op = x.n_op;
    const PlanBlockLayout blk(n_tiles, n_pieces, n_op, 0, 0, 0, p->npos, p->rows);
    PC_TRY(p->d_tables.reserve(blk.bytes));
    uint8_t *d = p->d_tables.p;
    if (n_tiles) HIP_TRY(hipMemcpyAsync(d + blk.at_tiles, x.tiles_tmp, n_tiles * sizeof(Tile), hipMemcpyDeviceToDevice, st));
    if (n_pieces) HIP_TRY(hipMemcpyAsync(d + blk.at_pieces, x.psorted, n_pieces * sizeof(Piece), hipMemcpyDeviceToDevice, st));
    if (n_op) hipLaunchKernelGGL(k_out_sorted, dim3((unsigned)((n_op + 255) / 256)), dim3(256), 0, st, x.misc, x.otile2, x.oidx2, x.oraw, (OutPiece *)(d + blk.at_opieces), (Tile *)(d + blk.at_tiles));
    HIP_TRY(hipMemsetAsync(d + blk.at_items, 0, blk.zeroed_bytes(), st));
    HIP_TRY(hipGetLastError());
    blk.bind(p);
    p->gpu_built = true;
    p->host_inputs = false;
    x.pclk.lap("plan(gpu): tables");
    return PC_OK;
}

// The tables of a plan, built on the GPU.  `p` arrives with nseg / out_elems / rows set; on PC_OK it has its tables in
// HBM (d_tables and the views into it), the sizes and flags the host builder sets, and no host copies.
int plan_build_gpu(pc_engine *e, pc_plan *p, const PlanSegments &segs, int64_t out_elems, int rows) {
    PlanBuild x(e, p, segs, out_elems, rows);
    PC_TRY(plan_upload_inputs(x));
    PC_TRY(plan_segments(x));
    PC_TRY(plan_islands(x));
    PC_TRY(plan_pieces_tiles(x));
    PC_TRY(plan_out_pieces(x));
    return plan_block(x);
}

// The tables of a host-built plan (p->host) into one device block with one upload (a plan of one short segment is
// otherwise dominated by the per-copy cost); the per-tile item counters arrive zeroed with it.  On an error the caller
// waits for the stream before it deletes the plan: copies out of the plan's vectors may be in flight.
int plan_upload(pc_engine *e, pc_plan *p) {
    StageClock pclk;
    const HostPlan &hp = p->host;
    const PlanBlockLayout blk(hp.tiles.size(), hp.pieces.size(), hp.opieces.size(), hp.cchunks.size(), hp.gsegs.size(), hp.gchunks.size(), p->npos, p->rows);
    // (a large annotation's tables -- tens of MB -- go up table by table from where they are: a
    // page-locked buffer of that size costs more to create than it saves)
    const bool through_pinned = blk.bytes <= ((size_t)4 << 20);
    PC_TRY(p->d_tables.reserve(blk.bytes));
    if (through_pinned && e->pinned_busy && hipEventSynchronize(e->ev_pinned) != hipSuccess) return fail(PC_ERR_HIP, "pc_plan_create: wait failed");
    if (through_pinned) PC_TRY(e->pinned.reserve(blk.bytes));
    uint8_t *h = through_pinned ? e->pinned.p : nullptr, *d = p->d_tables.p;
    bool copy_failed = false;
    auto put = [&](size_t at, const void *src, size_t n) {
        if (!n) return;
        if (through_pinned) memcpy(h + at, src, n);
        else if (hipMemcpyAsync(d + at, src, n, hipMemcpyHostToDevice, e->stream) != hipSuccess) copy_failed = true;
    };
    put(blk.at_tiles, hp.tiles.data(), hp.tiles.size() * sizeof(Tile));
    put(blk.at_pieces, hp.pieces.data(), hp.pieces.size() * sizeof(Piece));
    put(blk.at_opieces, hp.opieces.data(), hp.opieces.size() * sizeof(OutPiece));
    put(blk.at_cchunks, hp.cchunks.data(), hp.cchunks.size() * sizeof(CenterChunk));
    put(blk.at_gsegs, hp.gsegs.data(), hp.gsegs.size() * sizeof(GatherSeg));
    put(blk.at_gchunks, hp.gchunks.data(), hp.gchunks.size() * sizeof(GatherChunk));
    if (through_pinned) memset(h + blk.at_items, 0, blk.zeroed_bytes());
    else if (hipMemsetAsync(d + blk.at_items, 0, blk.zeroed_bytes(), e->stream) != hipSuccess) copy_failed = true;
    blk.bind(p);
    p->n_tiles = hp.tiles.size(); p->n_pieces = hp.pieces.size(); p->n_opieces = hp.opieces.size();
    p->n_cchunks = hp.cchunks.size(); p->n_gchunks = hp.gchunks.size();
    if (!through_pinned) {   // the copies read the plan's own vectors, which live as long as the plan
        if (copy_failed) return fail(PC_ERR_HIP, "pc_plan_create: upload failed");
    } else {
        if (hipMemcpyAsync(d, h, blk.bytes, hipMemcpyHostToDevice, e->stream) != hipSuccess) return fail(PC_ERR_HIP, "pc_plan_create: upload failed");
        if (hipEventRecord(e->ev_pinned, e->stream) != hipSuccess) return fail(PC_ERR_HIP, "pc_plan_create: event failed");
        e->pinned_busy = true;
    }
    pclk.lap("plan: upload");
    return PC_OK;
}

// The tables of a GPU-built plan that only the center rule (64-position chunks) or only the coordinate export (the
// per-segment gather list) reads are built when first asked for, each on its own, from the tables in HBM: a point-rule
// plan of 479 k exons otherwise pays for 1.4 M chunk descriptors it never uses.  (A host-built plan has everything in
// its one upload.)
int ensure_center_tables(pc_engine *e, pc_plan *p) {
    if (!p->gpu_built || p->center_ready) return PC_OK;
    // chunks per tile, exclusive sum, fill
    using namespace pcplan;
    hipStream_t st = e->stream;
    const size_t ntl = p->n_tiles;
    Bump A;
    uint32_t *cnt = nullptr, *at = nullptr;
    uint8_t *tmp = nullptr;
    auto scan = [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, cnt, at, (int)ntl + 1, st); };   // (the pointers as they are when it runs)
    size_t tb = 0, asked = 0;
    PC_TRY(cub_need(tb, asked, scan));
    for (int pass = 0; pass < 2; ++pass) {
        A.used = 0;
        cnt = A.take<uint32_t>(ntl + 1); at = A.take<uint32_t>(ntl + 1); tmp = A.take<uint8_t>(tb + 256);
        if (pass == 0) {
            PC_TRY(e->plan_scratch[0].reserve(A.used + 256));
            A.base = e->plan_scratch[0].p;
        }
    }
    uint32_t total = 0;
    if (ntl) {
        const unsigned g = (unsigned)((ntl + 255) / 256);
        HIP_TRY(hipMemsetAsync(cnt + ntl, 0, 4, st));
        hipLaunchKernelGGL(k_cchunk_count, dim3(g), dim3(256), 0, st, p->d_tiles.p, p->d_pieces.p, (uint32_t)ntl, cnt);
        PC_TRY(cub_run_sized(tmp, tb, scan));
        HIP_TRY(hipMemcpyAsync(&total, at + ntl, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        PC_TRY(p->d_tables2.reserve(std::max<size_t>((size_t)total * sizeof(CenterChunk), 256)));
        if (total) hipLaunchKernelGGL(k_cchunk_fill, dim3(g), dim3(256), 0, st, p->d_tiles.p, p->d_pieces.p, (uint32_t)ntl, at, (CenterChunk *)p->d_tables2.p);
        HIP_TRY(hipGetLastError());
    } else {
        PC_TRY(p->d_tables2.reserve(256));
    }
    p->d_cchunks.p = (CenterChunk *)p->d_tables2.p;
    p->n_cchunks = total;
    p->center_ready = true;
    return PC_OK;
}

int ensure_gather_tables(pc_engine *e, pc_plan *p) {
    if (!p->gpu_built || p->gather_ready) return PC_OK;
    // the per-segment records are in HBM already: (segment, chunk) pairs by count, exclusive sum, fill
    using namespace pcplan;
    hipStream_t st = e->stream;
    const size_t n = (size_t)p->nseg;
    Bump A;
    uint32_t *cnt = nullptr, *at = nullptr;
    uint8_t *tmp = nullptr;
    auto scan = [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, cnt, at, (int)n + 1, st); };   // (the pointers as they are when it runs)
    size_t tb = 0, asked = 0;
    PC_TRY(cub_need(tb, asked, scan));
    for (int pass = 0; pass < 2; ++pass) {
        A.used = 0;
        cnt = A.take<uint32_t>(n + 1); at = A.take<uint32_t>(n + 1); tmp = A.take<uint8_t>(tb + 256);
        if (pass == 0) {
            PC_TRY(e->plan_scratch[0].reserve(A.used + 256));
            A.base = e->plan_scratch[0].p;
        }
    }
    uint32_t total = 0;
    const unsigned g = (unsigned)((n + 255) / 256);
    HIP_TRY(hipMemsetAsync(cnt + n, 0, 4, st));
    if (n) hipLaunchKernelGGL(k_gchunk_count, dim3(g), dim3(256), 0, st, p->d_gsegs_own.p, p->nseg, cnt);
    PC_TRY(cub_run_sized(tmp, tb, scan));
    HIP_TRY(hipMemcpyAsync(&total, at + n, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    PC_TRY(p->d_tables3.reserve(std::max<size_t>((size_t)total * sizeof(GatherChunk), 256)));
    if (total) hipLaunchKernelGGL(k_gchunk_fill, dim3(g), dim3(256), 0, st, p->nseg, cnt, at, (GatherChunk *)p->d_tables3.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // (the scratch block may be reused by the next builder call)
    p->d_gsegs.p = p->d_gsegs_own.p;
    p->d_gchunks.p = (GatherChunk *)p->d_tables3.p;
    p->n_gchunks = total;
    p->gather_ready = true;
    return PC_OK;
}

// Center stream `sel` (0 forward reads, 1 reverse reads, 2 all reads) of one staged file: entries per record,
// exclusive sum, scatter -- three passes over the 8-byte records in HBM (see k_center in pc_kernels.hip.h).
int build_center_stream(pc_engine *e, StagedFile *sf, int sel, int nib) {
    hipStream_t st = e->stream;
    const int64_t n = sf->n;
    if (sf->cs_n[sel] >= 0 && sf->cs_nib[sel] == nib) return PC_OK;
    // (one entry per aligned run, counted and scanned in 32 bits: n records + the extra runs of the multi-run ones bounds them)
    if (n + sf->nrun >= (int64_t)0xffffffffu)
        return fail(PC_ERR_ARG, "pc_count: the center rule takes at most 2^32-2 aligned runs per file (%lld records, %lld runs of multi-run reads); split the file",
                    (long long)n, (long long)sf->nrun);
    if (sf->cs_n[sel] < 0) {   // entries per record and their exclusive sum: independent of the nibble
        PC_TRY(sf->cs_soff[sel].reserve((size_t)n + 1));
        hipLaunchKernelGGL(k_cs_count, dim3((unsigned)((n + 1 + kWG - 1) / kWG)), dim3(kWG), 0, st, sf->rec.p, n, sel, sf->cs_soff[sel].p);
        {
            DevBuf<uint8_t> d_tmp;
            uint32_t *soff = sf->cs_soff[sel].p;
            PC_TRY(cub_run(d_tmp, [=](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, soff, soff, (int)(n + 1), st); }));
            HIP_TRY(hipStreamSynchronize(st));   // d_tmp goes out of scope
        }
        uint32_t total = 0;
        HIP_TRY(hipMemcpy(&total, sf->cs_soff[sel].p + n, sizeof(total), hipMemcpyDeviceToHost));
        PC_TRY(sf->cs_ent[sel].reserve((size_t)total + 64));
        sf->cs_n[sel] = (int64_t)total;
        e->files_dirty = true;
    }
    hipLaunchKernelGGL(k_cs_scatter, dim3((unsigned)((n + 64 + kWG - 1) / kWG)), dim3(kWG), 0, st, sf->rec.p, sf->blk_off.p, sf->blk.p, n,
                       sel, nib, sf->cs_soff[sel].p, sf->cs_ent[sel].p);
    HIP_TRY(hipGetLastError());
    sf->cs_nib[sel] = nib;
    return PC_OK;
}

// ------------------------------------------------------------------ counting

} // namespace

// ---- which of the engine's streams really run beside the main one
// The runtime multiplexes a process's streams onto a few hardware queues (four by default), and two streams that share
// one run their kernels one after the other.  Two places of the engine count on kernels running side by side -- the
// sparse-window class of a point-rule count (`side_stream`) and the inflate launches of the BAM decoder, which alternate
// between the main stream and `aux_stream[0]` so that one launch fills the tail of the other -- and which queue a new
// stream lands on depends on every stream the process already holds (other engines, torch, RCCL).  Measured in
// bench.py's process, where the headline engine is alive beside the one that decodes the BAM: the two inflate streams
// shared a queue, 139 ms for the 2.9 GB file against 94.5 ms in a process of its own (and 94.5 with GPU_MAX_HW_QUEUES=8).
// So the engine asks: a kernel that waits (at most half a millisecond) for a flag on the main stream, a kernel that sets
// it on the candidate -- seen means the two ran at once.  Candidates that did not are replaced by new streams (the
// runtime hands those to its least-used queue) a few times over; what cannot be had stays as it is: correct, serial.
namespace {
__global__ void k_stream_probe_wait(uint32_t *flag, unsigned long long budget) {
    const unsigned long long t0 = wall_clock64();
    uint32_t seen = 0;
    while ((seen = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0u && wall_clock64() - t0 < budget)
        __builtin_amdgcn_s_sleep(16);
    flag[1] = seen;
}
__global__ void k_stream_probe_set(uint32_t *flag) { __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// 1: a kernel on `b` ran while one on `a` was running; 0: it did not; < 0: error
int streams_run_side_by_side(pc_engine *e, hipStream_t a, hipStream_t b, uint32_t *flag) {
    HIP_TRY(hipMemsetAsync(flag, 0, 2 * sizeof(uint32_t), a));
    HIP_TRY(hipEventRecord(e->ev_fork, a));
    HIP_TRY(hipStreamWaitEvent(b, e->ev_fork, 0));
    hipLaunchKernelGGL(k_stream_probe_wait, dim3(1), dim3(1), 0, a, flag, 50000ull);   // wall_clock64 ticks at 100 MHz: 0.5 ms
    hipLaunchKernelGGL(k_stream_probe_set, dim3(1), dim3(1), 0, b, flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(a));
    HIP_TRY(hipStreamSynchronize(b));
    uint32_t seen[2] = {0, 0};
    HIP_TRY(hipMemcpy(seen, flag, sizeof(seen), hipMemcpyDeviceToHost));
    return seen[1] ? 1 : 0;
}

// `side_stream` is made a stream that runs beside `stream`, and `aux_stream[0]` one that runs beside both (the BAM
// decoder uploads on the side stream while the main and the auxiliary one inflate), if the process can have such
int settle_streams(pc_engine *e) {
    if (e->knobs.no_stream_probe) return PC_OK;
    DevBuf<uint32_t> flag;
    flag.pool = &e->pool;
    PC_TRY(flag.reserve(2));
    auto settle = [&](hipStream_t &cand, std::initializer_list<hipStream_t> beside) -> int {
        for (int attempt = 0;; ++attempt) {
            int ok = 1;
            for (hipStream_t other : beside) {
                ok = streams_run_side_by_side(e, other, cand, flag.p);
                if (ok <= 0) break;
            }
            if (ok < 0) return ok;
            if (ok || attempt == 7) return PC_OK;          // (attempt 7: stays as it is -- correct, serial)
            hipStream_t fresh = nullptr;
            HIP_TRY(hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking));
            e->parked_streams.push_back(cand);             // (destroyed with the engine: destroying it now would hand its queue slot straight back)
            cand = fresh;
        }
    };
    int rc = settle(e->side_stream, {e->stream});
    if (rc == PC_OK) rc = settle(e->aux_stream[0], {e->stream, e->side_stream});
    return rc;
}
} // namespace

extern "C" {

const char *pc_last_error(void) { return g_err.c_str(); }
int pc_abi_version(void) { return PC_ABI_VERSION; }

int pc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int pc_create(int device, pc_engine **out) {
    if (!out) return fail(PC_ERR_ARG, "pc_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t err = hipGetDeviceCount(&ndev);
    if (err != hipSuccess || ndev <= 0)
        return fail(PC_ERR_HIP, "pc_create: no HIP device available (%s); this engine has no CPU fallback",
                    err == hipSuccess ? "device count is 0" : hipGetErrorString(err));
    if (device < 0 || device >= ndev) return fail(PC_ERR_ARG, "pc_create: device %d out of range [0,%d)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    pc_engine *e = new pc_engine();
    e->device = device;
    e->pool.device = device;
    e->knobs.load(env_lookup);
    BigReservoir::get().engine_created(device);
    HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&e->side_stream, hipStreamNonBlocking));
    for (auto &a : e->aux_stream) HIP_TRY(hipStreamCreateWithFlags(&a, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&e->ev_pinned, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
    {
        int lds_attr = 0;
        if (hipDeviceGetAttribute(&lds_attr, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && lds_attr > 0)
            e->max_lds = (size_t)lds_attr;
    }
    for (auto &ev : e->ev) HIP_TRY(hipEventCreate(&ev));
    std::vector<double> inv(65536);
    inv[0] = 0.0;
    for (int m = 1; m < 65536; ++m) inv[m] = 1.0 / (double)m; // the reference's `1.0 / map_length`
    int rc = e->d_inv.upload(inv, e->stream);
    std::vector<double> invh(65536);
    for (int m = 0; m < 65536; ++m) invh[m] = inv[m] * 0.5;   // exact: a power-of-two scaling of a normal number
    if (rc == PC_OK) rc = e->d_invh.upload(invh, e->stream);
    room(rc, e->d_counters, 16);
    if (rc == PC_OK && hipMemsetAsync(e->d_counters.p, 0, 16 * sizeof(uint32_t), e->stream) != hipSuccess) rc = fail(PC_ERR_HIP, "pc_create: memset failed");
    if (rc == PC_OK && hipStreamSynchronize(e->stream) != hipSuccess) rc = fail(PC_ERR_HIP, "pc_create: sync failed");
    if (rc == PC_OK) rc = settle_streams(e);
    if (rc != PC_OK) {
        pc_destroy(e);
        return rc;
    }
    *out = e;
    return PC_OK;
}

int pc_destroy(pc_engine *e) {
    if (!e) return PC_OK;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    destroy_tracks_of(e);
    destroy_summaries_of(e);
    for (auto *f : e->files) delete f;
    e->files.clear();
    for (auto &ev : e->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (e->side_stream) { (void)hipStreamSynchronize(e->side_stream); (void)hipStreamDestroy(e->side_stream); }
    for (auto &a : e->aux_stream) if (a) { (void)hipStreamSynchronize(a); (void)hipStreamDestroy(a); }
    for (auto a : e->parked_streams) if (a) (void)hipStreamDestroy(a);
    if (e->q_host) (void)hipHostFree(e->q_host);
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_pinned) (void)hipEventDestroy(e->ev_pinned);
    for (auto &x : e->ev_ring) if (x) (void)hipEventDestroy(x);
    if (e->ev_join) (void)hipEventDestroy(e->ev_join);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    const int device = e->device;
    delete e;                                          // (its pool hands its idle blocks to the reservoir)
    BigReservoir::get().engine_destroyed(device);      // the last engine of the device: the reservoir shrinks to its default size
    return PC_OK;
}

int pc_release_cached_memory(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(PC_ERR_ARG, "pc_release_cached_memory: device %d out of range", device);
    HIP_TRY(hipSetDevice(device));
    BigReservoir::get().free_all(device);
    return PC_OK;
}

int pc_host_alloc(pc_engine *e, uint64_t bytes, void **out) {
    if (!e || !out) return fail(PC_ERR_ARG, "pc_host_alloc: engine / out is NULL");
    *out = nullptr;
    HIP_TRY(hipSetDevice(e->device));
    void *p = nullptr;
    HIP_TRY(hipHostMalloc(&p, std::max<uint64_t>(bytes, 8), hipHostMallocDefault));
    *out = p;
    return PC_OK;
}

int pc_host_free(pc_engine *e, void *p) {
    if (!e) return fail(PC_ERR_ARG, "pc_host_free: engine is NULL");
    if (!p) return PC_OK;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));   // (a read-back into it may still be in flight)
    HIP_TRY(hipHostFree(p));
    return PC_OK;
}

int pc_reload_knobs(pc_engine *e) {
    if (!e) return fail(PC_ERR_ARG, "engine is NULL");
    e->knobs.load(env_lookup);
    e->work_generation += 1;
    return PC_OK;
}

int pc_clear_alignments(pc_engine *e) {
    if (!e) return fail(PC_ERR_ARG, "engine is NULL");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (auto *f : e->files) delete f;
    e->files.clear();
    e->ntid = 0;
    e->files_dirty = true;
    e->work_generation += 1;
    return PC_OK;
}

int pc_num_files(pc_engine *e) { return e ? (int)e->files.size() : 0; }
int64_t pc_num_records(pc_engine *e, int file) {
    if (!e || file < 0 || file >= (int)e->files.size()) return -1;
    return e->files[file]->n;
}
int64_t pc_stream_entries(pc_engine *e, int file) {
    if (!e || file < 0 || file >= (int)e->files.size()) return -1;
    const StagedFile *sf = e->files[file];
    return sf->cn >= 0 ? sf->cn : sf->n;
}
int64_t pc_canonical_entries(pc_engine *e, int file) {
    if (!e || file < 0 || file >= (int)e->files.size()) return -1;
    const StagedFile *sf = e->files[file];
    if (e->files.size() != 1) return -1;   // (only a plan over ONE file streams it: what an earlier count of file 0 alone built is kept, and not served)
    return (!e->knobs.no_canon && sf->ksig_valid && sf->ksig.rule.words_gen == sf->words_gen) ? sf->kn : -1;
}

namespace {
// PC_STAGE_TIMING=1: print where pc_add_alignment_file spends its time (stderr)
} // namespace

int pc_read_records(pc_engine *e, int file, int64_t n, const int64_t *idx, int32_t *tid, int32_t *pos, int32_t *alen, uint8_t *reverse,
                    int32_t *nblk, uint16_t *flag16, uint8_t *mapq) {
    if (!e || file < 0 || file >= (int)e->files.size()) return fail(PC_ERR_ARG, "pc_read_records: bad file index");
    if (n < 0 || (n > 0 && (!idx || !tid || !pos || !alen || !reverse || !nblk))) return fail(PC_ERR_ARG, "pc_read_records: bad arguments");
    if (n == 0) return PC_OK;
    StagedFile *sf = e->files[file];
    for (int64_t k = 0; k < n; ++k)
        if (idx[k] < 0 || idx[k] >= sf->n) return fail(PC_ERR_ARG, "pc_read_records: record index %lld out of range", (long long)idx[k]);
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    DevBuf<int64_t> d_idx;
    DevBuf<uint8_t> d_out;   // tid, pos, alen, nblk (int32 each), flag16 (u16), reverse, mapq (u8): 20 bytes per record
    int rc = d_idx.upload(idx, (size_t)n, st);
    room(rc, d_out, (size_t)n * 20 + 64);
    if (rc != PC_OK) return rc;
    int32_t *o_tid = (int32_t *)d_out.p, *o_pos = o_tid + n, *o_alen = o_pos + n, *o_nblk = o_alen + n;
    uint16_t *o_f16 = (uint16_t *)(o_nblk + n);
    uint8_t *o_rev = (uint8_t *)(o_f16 + n), *o_mq = o_rev + n;
    hipLaunchKernelGGL(k_gather_records, dim3((unsigned)((n + kWG - 1) / kWG)), dim3(kWG), 0, st, sf->view(), e->ntid, d_idx.p, n,
                       sf->have_sam ? sf->sam_flag.p : nullptr, sf->have_sam ? sf->sam_mapq.p : nullptr, o_tid, o_pos, o_alen, o_rev, o_nblk, o_f16, o_mq);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(tid, o_tid, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(pos, o_pos, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(alen, o_alen, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(nblk, o_nblk, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(reverse, o_rev, (size_t)n, hipMemcpyDeviceToHost, st));
    if (flag16) HIP_TRY(hipMemcpyAsync(flag16, o_f16, (size_t)n * 2, hipMemcpyDeviceToHost, st));
    if (mapq) HIP_TRY(hipMemcpyAsync(mapq, o_mq, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PC_OK;
}

int pc_read_record_runs(pc_engine *e, int file, int64_t n, const int64_t *idx, const int64_t *run_at, int64_t nruns, int32_t *start, int32_t *len) {
    if (!e || file < 0 || file >= (int)e->files.size()) return fail(PC_ERR_ARG, "pc_read_record_runs: bad file index");
    if (n < 0 || nruns < 0 || (n > 0 && (!idx || !run_at)) || (nruns > 0 && (!start || !len))) return fail(PC_ERR_ARG, "pc_read_record_runs: bad arguments");
    if (n == 0 || nruns == 0) return PC_OK;
    StagedFile *sf = e->files[file];
    for (int64_t k = 0; k < n; ++k) {
        if (idx[k] < 0 || idx[k] >= sf->n) return fail(PC_ERR_ARG, "pc_read_record_runs: record index %lld out of range", (long long)idx[k]);
        if (run_at[k] < 0 || run_at[k] > nruns || (k > 0 && run_at[k] < run_at[k - 1])) return fail(PC_ERR_ARG, "pc_read_record_runs: run offsets must ascend within [0, nruns]");
    }
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    DevBuf<int64_t> d_idx, d_at;
    DevBuf<int32_t> d_runs;
    int rc = d_idx.upload(idx, (size_t)n, st);
    if (rc == PC_OK) rc = d_at.upload(run_at, (size_t)n, st);
    room(rc, d_runs, (size_t)nruns * 2);
    if (rc != PC_OK) return rc;
    // (the caller sized the run arrays from the run counts pc_read_records gave it: a slot beyond them would be a bug there)
    hipLaunchKernelGGL(k_gather_runs, dim3((unsigned)((n + kWG - 1) / kWG)), dim3(kWG), 0, st, sf->view(), d_idx.p, n, d_at.p, d_runs.p, d_runs.p + nruns);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(start, d_runs.p, (size_t)nruns * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(len, d_runs.p + nruns, (size_t)nruns * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PC_OK;
}

int pc_add_alignment_file(pc_engine *e, int64_t n, int32_t ntid, const int32_t *tid, const int32_t *pos,
                          const uint16_t *alen, const uint8_t *flags, const uint8_t *nblk, int64_t nrun,
                          const int32_t *blk_start, const int32_t *blk_len) {
    return pc_add_alignment_file_wide(e, n, ntid, tid, pos, alen, flags, nblk, nrun, blk_start, blk_len, 0, nullptr, nullptr, nullptr);
}

static int build_compact_stream(pc_engine *e, StagedFile *sf, int ntid);

} // extern "C"

namespace {

// ---- staging, phase by phase: every alignment file becomes a StagedFile here -- caller-owned columns
// (pc_add_alignment_file[_wide]), the columns the GPU BAM decoder left in HBM (add_alignment_bam_impl), the same columns
// read back (PC_BAM_STAGE_HOST=1).  The phases enqueue on e->stream in the order they are called.  A phase owns its
// temporaries and waits for the stream before they go back to the pool, on the error paths too: PC_TRY / HIP_TRY stand
// where nothing is in flight, and behind the first launch or copy of a phase its errors are collected and reported behind
// the wait (finish_phase).
struct StageInput {   // one file, as its caller has it
    int64_t n = 0;                // records
    int32_t ntid = 0;             // contigs of the reference list
    const int32_t *tid = nullptr, *pos = nullptr;   // host columns (NULL with `dev`)
    const uint16_t *alen = nullptr;
    const uint8_t *flags = nullptr, *nblk = nullptr;
    int64_t nrun = 0;             // aligned runs of the multi-run records
    const int32_t *blk_start = nullptr, *blk_len = nullptr;
    int64_t n_wide = 0;           // wide records: always from the host
    const int64_t *wide_idx = nullptr;
    const int32_t *wide_alen = nullptr, *wide_nblk = nullptr;
    // set: the columns are in HBM already (a BAM file decoded on the GPU) -- nothing is uploaded or validated (the decoder
    // did that); its wide_rec / wide_val / n_wide are filled in here
    const pcstage::DevCols *dev = nullptr;
};

struct FileStats {   // the statistics block of k_cols_pack, back on the host
    std::vector<int64_t> span_hist, gap_span_hist, wide_span_hist, len_hist, len1_hist, tid_end;
    std::vector<int32_t> last_pos;   // start of the last record of every contig
    int Wr = 1, rmin = 65536, rmax = -1;
    int64_t max_span = 1;
    explicit FileStats(int ntid)
        : span_hist(pcstage::kSpanBins, 0), gap_span_hist(pcstage::kSpanBins, 0), wide_span_hist(pcstage::kSpanBins, 0), len_hist(pcstage::kLenBins, 0),
          len1_hist(pcstage::kLen1Bins, 0), tid_end((size_t)ntid, 0), last_pos((size_t)ntid, -1) {}
};

struct StageCall {   // what the phases of one call share beside the engine and the file under construction
    const StageInput &in;
    StageClock clk;
    // caller-owned columns in HBM as they are (stage_upload); read up to k_zip_runs
    DevBuf<int32_t> d_pos, d_bs, d_bl;
    DevBuf<uint16_t> d_alen;
    DevBuf<uint8_t> d_flags8, d_nblk8;
    pcstage::DevCols cols;              // the columns every kernel reads: those, or the decoder's
    std::vector<int64_t> tid_bounds;    // first record of every contig
    int64_t n_ok;                       // records before the first defect of the contig column
    DevBuf<uint32_t> d_run_at;          // where the runs of every record go in the run stream (stage_run_layout -> stage_pack)
    int64_t nrunrec = 0;                // entries of the run stream
    // run-stream records {run start, len | cum << 8 | L << 16 | flags << 24} and the record of every run, in record order
    // (stage_pack -> stage_run_stream)
    DevBuf<uint2> d_val_in;
    DevBuf<uint32_t> d_idx_in;
    FileStats stats;
    int wcap = 64;                      // the window halo
    uint32_t nwg = 0;                   // workgroups of k_classify
    DevBuf<uint32_t> d_side_at;         // [3 * nwg + 1]: members of the three side lists per workgroup, then their exclusive sum
    size_t side_total[3] = {0, 0, 0};   // long, gapped, extra-long
    std::vector<int64_t> lin_off;       // first linear-index entry of every contig
    explicit StageCall(const StageInput &i) : in(i), cols(), tid_bounds((size_t)i.ntid + 1, 0), n_ok(i.n), stats(i.ntid) {}
};

int stage_check(const pc_engine *e, const StageInput &in) {   // (no HIP call)
    const int64_t n = in.n, nrun = in.nrun, n_wide = in.n_wide;
    if (!e) return fail(PC_ERR_ARG, "engine is NULL");
    if (n < 0 || in.ntid <= 0 || nrun < 0) return fail(PC_ERR_ARG, "pc_add_alignment_file: bad sizes");
    if (!in.dev && n > 0 && (!in.tid || !in.pos || !in.alen || !in.flags || !in.nblk)) return fail(PC_ERR_ARG, "pc_add_alignment_file: NULL array");
    if (!in.dev && nrun > 0 && (!in.blk_start || !in.blk_len)) return fail(PC_ERR_ARG, "pc_add_alignment_file: NULL run array");
    if (n_wide < 0 || (n_wide > 0 && (!in.wide_idx || !in.wide_alen || !in.wide_nblk))) return fail(PC_ERR_ARG, "pc_add_alignment_file: bad wide-record arrays");
    for (int64_t k = 0; k < n_wide && !in.dev; ++k) {
        const int64_t i = in.wide_idx[k];
        if (i < 0 || i >= n || (k > 0 && i <= in.wide_idx[k - 1])) return fail(PC_ERR_ARG, "pc_add_alignment_file: wide_idx must be ascending record indices");
        if (in.alen[i] != 0xffffu || in.nblk[i] != 0xffu) return fail(PC_ERR_ARG, "pc_add_alignment_file: record %lld is listed as wide but its alen / nblk are not 65535 / 255", (long long)i);
        if (in.wide_alen[k] < 0 || in.wide_nblk[k] < 0 || (in.wide_nblk[k] == 0) != (in.wide_alen[k] == 0) || in.wide_nblk[k] > in.wide_alen[k])
            return fail(PC_ERR_ARG, "pc_add_alignment_file: record %lld: bad wide alen / nblk", (long long)i);
    }
    if (n >= (int64_t)0x7fffffff || nrun >= (int64_t)0xffffffffu)
        return fail(PC_ERR_ARG, "pc_add_alignment_file: more than 2^31-2 records per file are not supported");
    if (!e->files.empty() && in.ntid != e->ntid)
        return fail(PC_ERR_ARG, "pc_add_alignment_file: all files must use the same reference list (ntid %d vs %d)", in.ntid, e->ntid);
    return PC_OK;
}

// The wide records by record index, {uint32 record, uint2 {aligned length, run count}}: what the per-record kernels look
// up, from k_cols_runs on.  They go up once, straight into the arrays the file keeps.
int upload_wide_records(pc_engine *e, StagedFile *sf, StageCall &c) {
    const StageInput &in = c.in;
    if (in.n_wide > 0) {
        std::vector<uint32_t> wr((size_t)in.n_wide);
        std::vector<uint2> wv((size_t)in.n_wide);
        for (int64_t k = 0; k < in.n_wide; ++k) { wr[(size_t)k] = (uint32_t)in.wide_idx[k]; wv[(size_t)k] = make_uint2((uint32_t)in.wide_alen[k], (uint32_t)in.wide_nblk[k]); }
        int rc = sf->wide_rec.upload(wr, e->stream);
        if (rc == PC_OK) rc = sf->wide_val.upload(wv, e->stream);
        if (hipStreamSynchronize(e->stream) != hipSuccess && rc == PC_OK) rc = fail(PC_ERR_HIP, "stage: uploading the wide records failed");   // (the host vectors go out of scope)
        if (rc != PC_OK) return rc;
        sf->nwide = in.n_wide;
    }
    c.cols.wide_rec = sf->wide_rec.p; c.cols.wide_val = sf->wide_val.p; c.cols.n_wide = in.n_wide;
    return PC_OK;
}

// the arrays of the staged file whose sizes follow from the record count alone
int reserve_record_arrays(StagedFile *sf, StageCall &c) {
    const size_t n = (size_t)c.in.n;
    PC_TRY(sf->blk_off.reserve(n + 1));
    PC_TRY(c.d_run_at.reserve(n + 1));
    PC_TRY(sf->rec.reserve(n + 2));
    return sf->stream.reserve(n + 8);
}

// ---- caller-owned columns: up to HBM as they are.  The host moves bytes and looks at ONE column, the contigs: sorted,
// that column is ntid + 1 record bounds, so it does not travel -- a streaming comparison finds the bounds (and the first
// record out of order or out of range) on the worker threads while the other columns cross PCIe through the ring.
int stage_upload(pc_engine *e, StagedFile *sf, StageCall &c) {
    const StageInput &in = c.in;
    const size_t n = (size_t)in.n, nrun = (size_t)in.nrun;
    int rc = PC_OK;
    room(rc, c.d_pos, n + 1); room(rc, c.d_alen, n + 1); room(rc, c.d_flags8, n + 1); room(rc, c.d_nblk8, n + 1);
    room(rc, c.d_bs, nrun + 1); room(rc, c.d_bl, nrun + 1);
    PC_TRY(rc);
    // (the ring fills these blocks on ITS stream: a block the pool recycled may still be read or written by work
    // queued on the engine's stream -- a plan buffer that grew inside an asynchronous pc_count -- and every other user of
    // the pool is ordered on that stream; the ring is the exception, so it starts behind everything queued there)
    HIP_TRY(hipStreamSynchronize(e->stream));
    size_t piece = TransferRing::kPiece;
    if (const char *env = getenv("PC_STAGE_SLICE")) piece = (size_t)std::max<int64_t>(1, std::min<int64_t>(atoll(env), (int64_t)(TransferRing::kPiece / 4))) * 4; // test knob: tiny pieces
    std::vector<TransferJob> jobs;   // (what the first kernel reads goes first)
    jobs.push_back({c.d_nblk8.p, in.nblk, n});
    jobs.push_back({c.d_alen.p, in.alen, n * 2});
    jobs.push_back({c.d_pos.p, in.pos, n * 4});
    jobs.push_back({c.d_flags8.p, in.flags, n});
    jobs.push_back({c.d_bs.p, in.blk_start, nrun * 4});
    jobs.push_back({c.d_bl.p, in.blk_len, nrun * 4});
    struct Joined { std::future<int> f; ~Joined() { if (f.valid()) f.wait(); } } up;   // (joined on every way out, before the buffers go)
    c.clk.lap("column buffers");
    const int devno = e->device;
    up.f = std::async(std::launch::async, [devno, &jobs, piece]() -> int {
        StageClock uclk;
        const int r = TransferRing::of(devno).run(devno, jobs, piece, getenv("PC_STAGE_SLICE") != nullptr);
        uclk.lap("  (upload thread: ring)");
        return r;
    });
    c.n_ok = scan_contigs(in.tid, in.n, in.ntid, stage_threads(in.n), c.tid_bounds);
    c.clk.lap("contig bounds");
    rc = upload_wide_records(e, sf, c);
    // while the columns cross PCIe: the arrays of the staged file whose sizes follow from the record count alone (a
    // billion records: 20 GB of hipMalloc, 0.12 s when the pool has no such blocks -- a third of the call)
    if (rc == PC_OK) rc = reserve_record_arrays(sf, c);
    c.clk.lap("arrays of the file (beside the upload)");
    const int urc = up.f.get();
    if (rc != PC_OK) return rc;
    if (urc != PC_OK) return fail(urc, "pc_add_alignment_file: uploading the columns failed");
    c.cols.tid = nullptr; c.cols.pos = c.d_pos.p; c.cols.alen = c.d_alen.p; c.cols.flags = c.d_flags8.p; c.cols.nblk = c.d_nblk8.p;
    c.cols.blk_start = c.d_bs.p; c.cols.blk_len = c.d_bl.p;
    c.clk.lap("columns to HBM");
    return PC_OK;
}

// ---- where the runs of every record sit in the run arrays (blk_off, kept with the file) / go in the run stream: two
// exclusive sums
int stage_run_layout(pc_engine *e, StagedFile *sf, StageCall &c) {
    using namespace pcstage;
    hipStream_t st = e->stream;
    const int64_t n = c.in.n, nrun = c.in.nrun;
    DevBuf<uint8_t> d_tmp;
    DevBuf<unsigned long long> d_tot;
    PC_TRY(d_tot.reserve(2));
    auto sum_in_place = [=](uint32_t *v) { return [=](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, v, v, (int)n + 1, st); }; };
    size_t most = 16, tb = 0;
    PC_TRY(cub_need(most, tb, sum_in_place(c.d_run_at.p)));
    PC_TRY(d_tmp.reserve(most));
    unsigned long long tot[2] = {0, 0};
    hipError_t he = hipMemsetAsync(d_tot.p, 0, 16, st);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(k_cols_runs, dim3((unsigned)std::min<int64_t>((n + 256) / 256, 4096)), dim3(256), 0, st, c.cols, n, sf->blk_off.p, c.d_run_at.p, d_tot.p);
        he = cub_enqueue(d_tmp.p, tb, sum_in_place(sf->blk_off.p));
    }
    if (he == hipSuccess) he = cub_enqueue(d_tmp.p, tb, sum_in_place(c.d_run_at.p));
    if (he == hipSuccess) he = hipMemcpyAsync(tot, d_tot.p, 16, hipMemcpyDeviceToHost, st);
    PC_TRY(finish_phase(st, he, "stage: laying out the runs failed: %s"));
    if ((int64_t)tot[0] != nrun)
        return fail(PC_ERR_ARG, (int64_t)tot[0] > nrun ? "run arrays shorter than sum of nblk" : "run arrays longer than sum of nblk (%lld vs %lld)",
                    (long long)tot[0], (long long)nrun);
    if (tot[1] >= 0x7fffffffull) return fail(PC_ERR_ARG, "pc_add_alignment_file: more than 2^31-2 aligned runs of multi-run reads per file are not supported");
    c.nrunrec = (int64_t)tot[1];
    return PC_OK;
}

// the verdict of k_cols_pack<true>: defect code in the low byte, the record above it
int column_defect(unsigned long long verdict) {
    using namespace pcstage;
    const long long i = (long long)(verdict >> 8);
    switch ((int)(verdict & 0xffu)) {
    case kBadNegPos: return fail(PC_ERR_ARG, "record %lld: negative position", i);
    case kBadOrder: return fail(PC_ERR_UNSORTED, "records are not sorted by (tid, pos) at record %lld; alignment files must be coordinate sorted", i);
    case kBadRuns: return fail(PC_ERR_ARG, "record %lld: aligned runs must be non-empty, ascending and non-adjacent", i);
    case kBadFirstRun: return fail(PC_ERR_ARG, "record %lld: first run must start at pos", i);
    case kBadRunSum: return fail(PC_ERR_ARG, "record %lld: run lengths do not sum to alen", i);
    case kBadLenRuns: return fail(PC_ERR_ARG, "record %lld: nblk/alen mismatch", i);
    default: return fail(PC_ERR_ARG, "record %lld: alignment end beyond 2^31-1", i);
    }
}

// the first defect of the contig column, as the message the caller sees (unless a record before it has one of its own)
int contig_defect(const StageInput &in, int64_t i) {
    if (in.tid[i] < 0 || in.tid[i] >= in.ntid) return fail(PC_ERR_ARG, "record %lld: tid %lld out of range", (long long)i, (long long)in.tid[i]);
    if (in.pos[i] < 0) return fail(PC_ERR_ARG, "record %lld: negative position", (long long)i);
    return fail(PC_ERR_UNSORTED, "records are not sorted by (tid, pos) at record %lld; alignment files must be coordinate sorted", (long long)i);
}

void take_stats(const std::vector<unsigned long long> &hstats, const std::vector<int32_t> &htid_end, StageCall &c) {
    using namespace pcstage;
    FileStats &s = c.stats;
    for (size_t t = 0; t < s.tid_end.size(); ++t) s.tid_end[t] = c.tid_bounds[t + 1] > c.tid_bounds[t] ? (int64_t)htid_end[t] : 0;
    for (int k = 0; k < kSpanBins; ++k) {
        s.span_hist[(size_t)k] = (int64_t)hstats[(size_t)(kAtSpan + k)];
        s.gap_span_hist[(size_t)k] = (int64_t)hstats[(size_t)(kAtGap + k)];
        s.wide_span_hist[(size_t)k] = (int64_t)hstats[(size_t)(kAtWide + k)];
    }
    for (int k = 0; k < kLenBins; ++k) s.len_hist[(size_t)k] = (int64_t)hstats[(size_t)(kAtLen + k)];
    for (int k = 0; k < kLen1Bins; ++k) s.len1_hist[(size_t)k] = (int64_t)hstats[(size_t)(kAtLen1 + k)];
    s.Wr = std::max(1, (int)hstats[(size_t)kAtMisc + 0]);
    s.rmin = (int)hstats[(size_t)kAtMisc + 1];
    s.rmax = s.rmin >= 65536 ? -1 : (int)hstats[(size_t)kAtMisc + 2];
    s.max_span = std::max<int64_t>(1, (int64_t)hstats[(size_t)kAtMisc + 3]);
}

// ---- one pass over the columns: validation (caller-owned columns), the 8-byte records, the run-stream records, the
// ends, the statistics of the file (span and length histograms, per-contig bounds) -- stage_kernels.hip.h.  What
// depends on the statistics of the WHOLE file -- the window halo `wcap` (a span quantile) and with it the long-span
// class of a record and its stream word -- is derived afterwards (k_classify).
int stage_pack(pc_engine *e, StagedFile *sf, StageCall &c) {
    using namespace pcstage;
    const StageInput &in = c.in;
    const int64_t n = in.n;
    const int ntid = in.ntid;
    const bool host_cols = in.dev == nullptr;
    if (n == 0) return PC_OK;
    hipStream_t st = e->stream;
    DevBuf<unsigned long long> d_stats;   // the statistics block, then the error word of the validation
    DevBuf<int32_t> d_last_pos, d_tid_end;
    DevBuf<int64_t> d_bounds;
    int rc = d_stats.reserve(kStatWords + 1);
    room(rc, d_last_pos, (size_t)ntid); room(rc, d_tid_end, (size_t)ntid); room(rc, d_bounds, (size_t)ntid + 1);
    PC_TRY(rc);
    std::vector<unsigned long long> hstats((size_t)kStatWords + 1, 0ull);
    hstats[(size_t)kAtMisc + 1] = 65536ull;   // rmin
    hstats[(size_t)kStatWords] = ~0ull;       // no defect
    std::vector<int32_t> htid_end((size_t)ntid);
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 2048);
    hipError_t he = hipMemcpyAsync(d_stats.p, hstats.data(), hstats.size() * 8, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemsetAsync(d_tid_end.p, 0, (size_t)ntid * 4, st);
    if (he == hipSuccess && host_cols) {
        he = hipMemcpyAsync(d_bounds.p, c.tid_bounds.data(), ((size_t)ntid + 1) * 8, hipMemcpyHostToDevice, st);
        if (he == hipSuccess)
            hipLaunchKernelGGL((k_cols_pack<true>), dim3(grid), dim3(256), 0, st, c.cols, c.n_ok, sf->blk_off.p, c.d_run_at.p, sf->rec.p, c.d_val_in.p, c.d_idx_in.p,
                               d_tid_end.p, d_stats.p, d_bounds.p, ntid, d_stats.p + kStatWords);
        // the verdict before anything is derived from the records
        unsigned long long verdict = ~0ull;
        if (he == hipSuccess) he = hipMemcpyAsync(&verdict, d_stats.p + kStatWords, 8, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he == hipSuccess && verdict != ~0ull) return column_defect(verdict);
        if (he == hipSuccess && c.n_ok < n) return contig_defect(in, c.n_ok);
        for (int t = 0; t < ntid; ++t)
            if (c.tid_bounds[(size_t)t + 1] > c.tid_bounds[(size_t)t]) c.stats.last_pos[(size_t)t] = in.pos[c.tid_bounds[(size_t)t + 1] - 1];
    } else if (he == hipSuccess) {
        hipLaunchKernelGGL(k_cols_bounds, dim3((unsigned)((ntid + 256) / 256)), dim3(256), 0, st, c.cols.tid, c.cols.pos, n, ntid, d_bounds.p, d_last_pos.p);
        hipLaunchKernelGGL((k_cols_pack<false>), dim3(grid), dim3(256), 0, st, c.cols, n, sf->blk_off.p, c.d_run_at.p, sf->rec.p, c.d_val_in.p, c.d_idx_in.p,
                           d_tid_end.p, d_stats.p, d_bounds.p, ntid, (unsigned long long *)nullptr);
    }
    if (he == hipSuccess) he = hipMemcpyAsync(hstats.data(), d_stats.p, (size_t)kStatWords * 8, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && !host_cols) he = hipMemcpyAsync(c.tid_bounds.data(), d_bounds.p, ((size_t)ntid + 1) * 8, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipMemcpyAsync(htid_end.data(), d_tid_end.p, (size_t)ntid * 4, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && !host_cols) he = hipMemcpyAsync(c.stats.last_pos.data(), d_last_pos.p, (size_t)ntid * 4, hipMemcpyDeviceToHost, st);
    PC_TRY(finish_phase(st, he, "stage: packing the columns failed: %s"));
    take_stats(hstats, htid_end, c);
    return PC_OK;
}

// ---- what every later kernel sees of the file: the window halo and the length ranges of the LDS entry table
// (choose_halo), the aligned lengths present, the layout of the linear-index tables (lin_layout) -- host arithmetic
void stage_halo(StagedFile *sf, StageCall &c) {
    FileStats &s = c.stats;
    const StageHalo h = choose_halo(s.span_hist, s.gap_span_hist, s.wide_span_hist, s.len1_hist, s.rmin, s.rmax, c.in.n, kStreamMaxLen);
    c.wcap = h.wcap;
    sf->slen_min = h.slen_min; sf->slen_max = h.slen_max; sf->tlen_min = h.tlen_min; sf->tlen_max = h.tlen_max;
    sf->W = h.W; sf->Wg = h.Wg; sf->Wr = s.Wr; sf->max_span = s.max_span;
    sf->len_hist.swap(s.len_hist);
    for (int L = 0; L < 65536; ++L)
        if (sf->len_hist[(size_t)L]) { sf->len_min = std::min(sf->len_min, L); sf->len_max = std::max(sf->len_max, L); }
    sf->nrunrec = c.nrunrec;
    sf->tid_end = s.tid_end;
    sf->nlin = lin_layout(c.tid_bounds, s.last_pos, s.tid_end, kLinShift, c.lin_off);
}

// ---- sentinels behind the last record, the aligned runs as {start, length} pairs, then the class and the 4-byte stream
// word of every record; per workgroup, the members of the three side lists
int stage_classify(pc_engine *e, StagedFile *sf, StageCall &c) {
    hipStream_t st = e->stream;
    const int64_t n = c.in.n, nrun = c.in.nrun;
    c.nwg = (uint32_t)((n + 255) / 256);
    const int nside = 3 * (int)c.nwg + 1;
    DevBuf<uint8_t> d_tmp;
    size_t most = 16, tb = 0;
    auto sum_sides = [&c, nside, st](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, c.d_side_at.p, c.d_side_at.p, nside, st); };
    if (nrun > 0) PC_TRY(sf->blk.reserve((size_t)nrun));
    if (nrun == 0) sf->blk_off.release();   // (all zero: no record keeps runs in the run arrays)
    if (n > 0) {
        PC_TRY(c.d_side_at.reserve((size_t)nside));
        PC_TRY(cub_need(most, tb, sum_sides));
        PC_TRY(d_tmp.reserve(most));
    }
    {   // two excluded headers, eight skip words (whole quads can always be loaded)
        const uint2 tail_rec[2] = {make_uint2(0u, (uint32_t)PC_FLAG_EXCLUDED << 16), make_uint2(0u, (uint32_t)PC_FLAG_EXCLUDED << 16)};
        uint32_t tail_stream[8];
        for (int k = 0; k < 8; ++k) tail_stream[k] = kStreamSkip;
        if (hipMemcpyAsync(sf->rec.p + n, tail_rec, sizeof(tail_rec), hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(sf->stream.p + n, tail_stream, sizeof(tail_stream), hipMemcpyHostToDevice, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fail(PC_ERR_HIP, "pc_add_alignment_file: staging the sentinels failed");
    }
    if (nrun > 0)
        hipLaunchKernelGGL(k_zip_runs, dim3((unsigned)((nrun + kWG - 1) / kWG)), dim3(kWG), 0, st, c.cols.blk_start, c.cols.blk_len, nrun, sf->blk.p);
    if (n == 0) return PC_OK;
    uint32_t at[4] = {0, 0, 0, 0};
    hipError_t he = hipMemsetAsync(c.d_side_at.p + 3 * (size_t)c.nwg, 0, 4, st);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(pcstage::k_classify, dim3(c.nwg), dim3(256), 0, st, sf->rec.p, n, sf->blk_off.p, sf->blk.p, c.wcap, sf->stream.p, c.d_side_at.p);
        he = cub_enqueue(d_tmp.p, tb, sum_sides);
    }
    for (int k = 1; k <= 3 && he == hipSuccess; ++k) he = hipMemcpyAsync(&at[k], c.d_side_at.p + (size_t)k * c.nwg, 4, hipMemcpyDeviceToHost, st);
    PC_TRY(finish_phase(st, he, "pc_add_alignment_file: deriving the record stream failed: %s"));
    for (int k = 0; k < 3; ++k) c.side_total[k] = at[k + 1] - at[k];
    return PC_OK;
}

// ---- side lists and linear-index tables, on the GPU (pc_kernels.hip.h, "side lists"): the records are there
// already; from the host come only the two small per-contig tables
struct SideList {   // one of the three lists: its members in record order, and where its entries go
    const uint32_t *idx;
    size_t m;
    uint4 *rec;
    int4 *runs;
    int32_t *tid;       // contig of every entry (the long list only)
    uint2 *wide;        // true {length, run count} of every entry (files with wide records; not the gapped list)
    int32_t *pmax;      // running maximum of the ends (NULL: the list has none)
    int64_t *bounds;    // per-contig ranges
};

struct SideScratch {   // the working arrays of the running maxima
    DevBuf<unsigned long long> d_key, d_key_scanned;
    DevBuf<uint8_t> d_tmp;
};

dim3 grid_of(size_t m) { return dim3((unsigned)((m + kWG - 1) / kWG)); }

// the running maximum over the first `cnt` packed ends, as `call(tmp, bytes)`: asked at the longer list, run per list
auto side_max_scan(SideScratch &w, size_t cnt, hipStream_t st) {
    return [&w, cnt, st](void *t, size_t &b) { return hipcub::DeviceScan::InclusiveScan(t, b, w.d_key.p, w.d_key_scanned.p, hipcub::Max(), (int)cnt, st); };
}

// the entries of one list, and the running maximum of their ends if the list has one
hipError_t fill_side_list(pc_engine *e, const StagedFile *sf, const StageCall &c, const SideList &l, SideScratch &w) {
    if (!l.m) return hipSuccess;
    hipStream_t st = e->stream;
    hipLaunchKernelGGL(k_side_fill, grid_of(l.m), dim3(kWG), 0, st, l.idx, (int64_t)l.m, sf->rec.p, sf->blk_off.p, sf->blk.p, sf->tid_bounds.p, c.in.ntid,
                       sf->wide_rec.p, sf->wide_val.p, c.in.n_wide, l.rec, l.runs, l.tid, l.pmax ? w.d_key.p : nullptr, l.wide);
    if (!l.pmax) return hipSuccess;
    const hipError_t he = cub_enqueue(w.d_tmp.p, w.d_tmp.cap, side_max_scan(w, l.m, st));
    if (he == hipSuccess) hipLaunchKernelGGL(k_unpack_pmax, grid_of(l.m), dim3(kWG), 0, st, w.d_key_scanned.p, (int64_t)l.m, l.pmax);
    return he;
}

int reserve_side_lists(StagedFile *sf, const StageCall &c, size_t nlong, size_t ngap, size_t nxlong) {
    const size_t ntid1 = (size_t)c.in.ntid + 1, nlin = sf->nlin;
    const bool wide = c.in.n_wide != 0;
    int rc = PC_OK;
    room(rc, sf->tid_bounds, ntid1); room(rc, sf->lin_off, ntid1); room(rc, sf->long_tid_bounds, ntid1); room(rc, sf->gap_tid_bounds, ntid1);
    room(rc, sf->long_idx, nlong); room(rc, sf->long_rec, nlong); room(rc, sf->long_runs, nlong); room(rc, sf->long_tid, nlong); room(rc, sf->long_pmax, nlong);
    room(rc, sf->gap_rec, ngap); room(rc, sf->gap_runs, ngap);
    room(rc, sf->xlong_rec, nxlong); room(rc, sf->xlong_runs, nxlong);
    if (wide) { room(rc, sf->long_wide, nlong); room(rc, sf->xlong_wide, nxlong); }
    room(rc, sf->lin_tab, nlin); room(rc, sf->glin_tab, nlin); room(rc, sf->llin_tab, nlin); room(rc, sf->plin_tab, nlin);
    if (nxlong) { room(rc, sf->xllin_tab, nlin); room(rc, sf->xplin_tab, nlin); }
    return rc;
}

int stage_side_lists(pc_engine *e, StagedFile *sf, StageCall &c) {
    hipStream_t st = e->stream;
    const int64_t n = c.in.n;
    const int ntid = c.in.ntid;
    const size_t nlong = c.side_total[0], ngap = c.side_total[1], nxlong = c.side_total[2], nlin = sf->nlin;
    sf->nlong = (int64_t)nlong;
    sf->ngap = (int64_t)ngap;
    sf->nxlong = (int64_t)nxlong;
    DevBuf<uint32_t> d_gap_idx, d_xlong_idx;   // the gapped and the extra-long list keep no member array
    DevBuf<int64_t> d_xlong_bounds;
    DevBuf<int32_t> d_xlong_pmax;
    SideScratch w;
    int rc = reserve_side_lists(sf, c, nlong, ngap, nxlong);
    room(rc, d_gap_idx, ngap);
    room(rc, d_xlong_idx, nxlong); room(rc, d_xlong_pmax, nxlong);
    room(rc, d_xlong_bounds, (size_t)ntid + 1);
    room(rc, w.d_key, std::max(nlong, nxlong)); room(rc, w.d_key_scanned, std::max(nlong, nxlong));
    PC_TRY(rc);
    size_t most = 16, need = 0;
    PC_TRY(cub_need(most, need, side_max_scan(w, std::max(nlong, nxlong), st)));
    PC_TRY(w.d_tmp.reserve(most));
    const SideList lists[3] = {
        {sf->long_idx.p, nlong, sf->long_rec.p, sf->long_runs.p, sf->long_tid.p, c.in.n_wide ? sf->long_wide.p : nullptr, sf->long_pmax.p, sf->long_tid_bounds.p},
        {d_gap_idx.p, ngap, sf->gap_rec.p, sf->gap_runs.p, nullptr, nullptr, nullptr, sf->gap_tid_bounds.p},
        {d_xlong_idx.p, nxlong, sf->xlong_rec.p, sf->xlong_runs.p, nullptr, c.in.n_wide ? sf->xlong_wide.p : nullptr, d_xlong_pmax.p, d_xlong_bounds.p}};
    hipError_t he = hipMemcpyAsync(sf->tid_bounds.p, c.tid_bounds.data(), ((size_t)ntid + 1) * 8, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(sf->lin_off.p, c.lin_off.data(), ((size_t)ntid + 1) * 8, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && n > 0 && nlong + ngap + nxlong > 0)   // members of the three lists, in record order
        hipLaunchKernelGGL(pcstage::k_side_select, dim3(c.nwg), dim3(256), 0, st, sf->rec.p, n, c.d_side_at.p, c.nwg, sf->long_idx.p, d_gap_idx.p, d_xlong_idx.p);
    // entries and running maxima of the ends, list by list; then the per-contig ranges of every list
    for (int k = 0; k < 3 && he == hipSuccess; ++k) he = fill_side_list(e, sf, c, lists[k], w);
    for (int k = 0; k < 3 && he == hipSuccess; ++k)
        hipLaunchKernelGGL(k_list_bounds, grid_of((size_t)ntid + 1), dim3(kWG), 0, st, lists[k].idx, (int64_t)lists[k].m, sf->tid_bounds.p, ntid, lists[k].bounds);
    // the linear-index tables: one bisection per table entry
    if (he == hipSuccess && nlin) {
        const dim3 gl = grid_of(nlin);
        hipLaunchKernelGGL((k_lin_table<0>), gl, dim3(kWG), 0, st, (const void *)sf->rec.p, sf->tid_bounds.p, sf->lin_off.p, ntid, (int64_t)nlin, sf->lin_tab.p);
        hipLaunchKernelGGL((k_lin_table<1>), gl, dim3(kWG), 0, st, (const void *)sf->gap_rec.p, sf->gap_tid_bounds.p, sf->lin_off.p, ntid, (int64_t)nlin, sf->glin_tab.p);
        hipLaunchKernelGGL((k_lin_table<1>), gl, dim3(kWG), 0, st, (const void *)sf->long_rec.p, sf->long_tid_bounds.p, sf->lin_off.p, ntid, (int64_t)nlin, sf->llin_tab.p);
        hipLaunchKernelGGL((k_lin_table<2>), gl, dim3(kWG), 0, st, (const void *)sf->long_pmax.p, sf->long_tid_bounds.p, sf->lin_off.p, ntid, (int64_t)nlin, sf->plin_tab.p);
        if (nxlong) {
            hipLaunchKernelGGL((k_lin_table<1>), gl, dim3(kWG), 0, st, (const void *)sf->xlong_rec.p, d_xlong_bounds.p, sf->lin_off.p, ntid, (int64_t)nlin, sf->xllin_tab.p);
            hipLaunchKernelGGL((k_lin_table<2>), gl, dim3(kWG), 0, st, (const void *)d_xlong_pmax.p, d_xlong_bounds.p, sf->lin_off.p, ntid, (int64_t)nlin, sf->xplin_tab.p);
        }
    }
    return finish_phase(st, he, "stage: building the side lists failed: %s");
}

// ---- run stream: sorted by (contig, run start) on the GPU (radix sort of the 64-bit keys, the 8-byte
// records and their record indices permuted along), then its linear index by one bisection per bucket
int stage_run_stream(pc_engine *e, StagedFile *sf, StageCall &c) {
    const size_t nrunrec = (size_t)c.nrunrec, nlin = sf->nlin;
    if (!nrunrec) return PC_OK;
    hipStream_t st = e->stream;
    const int ntid = c.in.ntid;
    DevBuf<unsigned long long> d_key, d_key_sorted;
    DevBuf<uint32_t> d_ord, d_ord_sorted;
    DevBuf<uint8_t> d_tmp;
    int rc = PC_OK;
    room(rc, d_key, nrunrec); room(rc, d_ord, nrunrec); room(rc, d_key_sorted, nrunrec); room(rc, d_ord_sorted, nrunrec); room(rc, sf->run_recidx, nrunrec);
    room(rc, sf->run_rec, nrunrec + 1);
    room(rc, sf->rlin_tab, nlin);
    PC_TRY(rc);
    const int end_bit = 32 + (ntid > 1 ? 32 - __builtin_clz((unsigned)(ntid - 1)) : 1);
    auto sort_runs = [&, end_bit](void *t, size_t &b) {   // stable: equal starts keep record order
        return hipcub::DeviceRadixSort::SortPairs(t, b, d_key.p, d_key_sorted.p, d_ord.p, d_ord_sorted.p, (int)nrunrec, 0, end_bit, st);
    };
    size_t most = 16, tmp_bytes = 0;
    PC_TRY(cub_need(most, tmp_bytes, sort_runs));
    PC_TRY(d_tmp.reserve(most));
    const dim3 grid = grid_of(nrunrec);
    // sort keys (contig << 32 | run start) and the identity permutation, made on the GPU
    hipLaunchKernelGGL(k_run_keys, grid, dim3(kWG), 0, st, c.d_val_in.p, c.d_idx_in.p, (int64_t)nrunrec, sf->tid_bounds.p, ntid, d_key.p, d_ord.p);
    hipError_t he = cub_enqueue(d_tmp.p, tmp_bytes, sort_runs);
    if (he != hipSuccess) return finish_phase(st, he, "stage: sorting the run stream failed: %s");
    hipLaunchKernelGGL(k_run_gather, grid, dim3(kWG), 0, st, d_ord_sorted.p, c.d_val_in.p, c.d_idx_in.p, (int64_t)nrunrec, sf->run_rec.p, sf->run_recidx.p);
    hipLaunchKernelGGL(k_run_lin, grid_of(nlin), dim3(kWG), 0, st, d_key_sorted.p, (int64_t)nrunrec, sf->lin_off.p, ntid, (int64_t)nlin, sf->rlin_tab.p);
    const uint2 tail_run = make_uint2(0u, (uint32_t)PC_FLAG_EXCLUDED << 24);
    he = hipMemcpyAsync(sf->run_rec.p + nrunrec, &tail_run, sizeof(tail_run), hipMemcpyHostToDevice, st);
    return finish_phase(st, he, "stage: building the run stream failed");
}

int stage_file(pc_engine *e, const StageInput &in) {
    PC_TRY(stage_check(e, in));
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);   // the file's arrays and the temporaries of staging are recycled through the engine's pool
    StageCall c(in);
    StagedFile *sf = new StagedFile();
    struct Owner { StagedFile *p; ~Owner() { delete p; } } owner{sf};   // (until the file is the engine's)
    sf->n = in.n;
    sf->nrun = in.nrun;
    if (in.dev) {   // the decoder's columns: only the wide records and the per-record arrays are missing
        c.cols = *in.dev;
        PC_TRY(upload_wide_records(e, sf, c));
        PC_TRY(reserve_record_arrays(sf, c));
    } else PC_TRY(stage_upload(e, sf, c));   // (laps: column buffers, contig bounds, arrays of the file, columns to HBM)
    PC_TRY(stage_run_layout(e, sf, c));
    c.clk.lap("run layout (GPU)");
    int rc = PC_OK;
    room(rc, c.d_val_in, (size_t)c.nrunrec); room(rc, c.d_idx_in, (size_t)c.nrunrec);
    PC_TRY(rc);
    c.clk.lap("allocations");
    PC_TRY(stage_pack(e, sf, c));
    c.clk.lap("validate + pack (GPU)");
    stage_halo(sf, c);
    PC_TRY(stage_classify(e, sf, c));
    c.clk.lap("record stream (GPU)");
    PC_TRY(stage_side_lists(e, sf, c));
    c.clk.lap("side lists + linear index (GPU)");
    PC_TRY(stage_run_stream(e, sf, c));
    c.clk.lap("run stream (GPU sort)");
    PC_TRY(build_compact_stream(e, sf, in.ntid));
    c.clk.lap("compact stream (GPU)");
    owner.p = nullptr;
    e->files.push_back(sf);
    e->ntid = in.ntid;
    e->files_dirty = true;
    e->work_generation += 1;
    return PC_OK;
}

} // namespace

extern "C" {

int pc_add_alignment_file_wide(pc_engine *e, int64_t n, int32_t ntid, const int32_t *tid, const int32_t *pos,
                               const uint16_t *alen, const uint8_t *flags, const uint8_t *nblk, int64_t nrun,
                               const int32_t *blk_start, const int32_t *blk_len, int64_t n_wide, const int64_t *wide_idx,
                               const int32_t *wide_alen, const int32_t *wide_nblk) {
    StageInput in;
    in.n = n; in.ntid = ntid; in.tid = tid; in.pos = pos; in.alen = alen; in.flags = flags; in.nblk = nblk;
    in.nrun = nrun; in.blk_start = blk_start; in.blk_len = blk_len;
    in.n_wide = n_wide; in.wide_idx = wide_idx; in.wide_alen = wide_alen; in.wide_nblk = wide_nblk;
    return stage_file(e, in);
}

static int propagate_record_flags(pc_engine *e, StagedFile *sf);

// The compact stream of a staged file and its linear index, from the stream words as they stand (stage_kernels.hip.h):
// at staging, and again whenever the words are rewritten (pc_update_flags, the FLAG / MAPQ / NH filter).  One pass
// over 4 bytes per record and an LDS sort per tile; the working arrays are the pool's and go back to it.
// A file that keeps more than `compact_keep` (PC_COMPACT_KEEP, 0.9) of its records as entries gets none: its block
// returns to the pool and the point rules stream the records, at no extra HBM.  (Every item pays the multiplicity
// field's two instructions per word either way, so fewer entries are never slower to bin; what the bound weighs is 4
// bytes of HBM per entry and a rebuild on every filter change against the stream bytes a count no longer reads, at most
// a tenth of them at the bound.  The bound is reasoned, not measured: profiles/compact_stream/NOTES.md says how the
// knob is to settle it.)
static int build_compact_stream(pc_engine *e, StagedFile *sf, int ntid) {
    using namespace pcstage;
    sf->cn = -1;
    sf->words_gen += 1;   // (whatever was derived from the words under one rule -- the canonical stream -- is stale)
    const int64_t n = sf->n;
    if (n <= 0 || !sf->nlin || e->knobs.no_compact) { sf->cstream.release(); sf->clin_tab.release(); return PC_OK; }
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    const uint32_t ntiles = (uint32_t)((n + kCompactTile - 1) / kCompactTile);
    DevBuf<uint32_t> d_words, d_cnt, d_off, d_base;
    DevBuf<uint8_t> d_scan;
    int rc = d_words.reserve((size_t)n);
    room(rc, d_cnt, (size_t)ntiles + 1); room(rc, d_off, (size_t)ntiles + 1); room(rc, d_base, (size_t)ntiles);
    if (rc != PC_OK) return rc;
    auto sum_tiles = [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, d_cnt.p, d_off.p, (int)ntiles + 1, st); };
    size_t most = 16, tb = 0;
    PC_TRY(cub_need(most, tb, sum_tiles));
    PC_TRY(d_scan.reserve(most));
    HIP_TRY(hipMemsetAsync(d_cnt.p + ntiles, 0, 4, st));
    hipLaunchKernelGGL(k_compact_tiles, dim3(ntiles), dim3(256), 0, st, sf->rec.p, sf->stream.p, n, sf->tid_bounds.p, ntid, d_words.p, d_cnt.p, d_base.p);
    hipError_t he = cub_enqueue(d_scan.p, tb, sum_tiles);
    uint32_t total = 0;
    if (he == hipSuccess) he = hipMemcpyAsync(&total, d_off.p + ntiles, 4, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipGetLastError();
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) return fail(PC_ERR_HIP, "building the compact stream failed: %s", hipGetErrorString(he));
    if ((double)total > e->knobs.compact_keep * (double)n) { sf->cstream.release(); sf->clin_tab.release(); return PC_OK; }
    rc = sf->cstream.reserve((size_t)total + 8);
    room(rc, sf->clin_tab, sf->nlin);
    if (rc != PC_OK) return rc;
    hipLaunchKernelGGL(k_compact_gather, dim3(ntiles), dim3(256), 0, st, d_words.p, d_off.p, ntiles, sf->cstream.p);
    hipLaunchKernelGGL(k_compact_lin, dim3((unsigned)((sf->nlin + 255) / 256)), dim3(256), 0, st, sf->lin_tab.p, (int64_t)sf->nlin, sf->rec.p, n,
                       d_off.p, d_base.p, sf->cstream.p, sf->clin_tab.p);
    he = hipGetLastError();
    if (he == hipSuccess) he = hipStreamSynchronize(st);   // (the working arrays go out of scope)
    if (he != hipSuccess) return fail(PC_ERR_HIP, "building the compact stream failed: %s", hipGetErrorString(he));
    sf->cn = (int64_t)total;
    return PC_OK;
}

// The columns the engine's filter reads are there for this file: the ONE test of every setter, of pc_update_flags and
// of the entry points that read the exclusion bits (check_filter_columns).
static bool columns_present(const pc_engine *e, const StagedFile *sf) {
    return (!e->ff_on || sf->have_sam) && (!e->ff_max_nh || sf->have_nh);
}

// Every entry point that reads the exclusion bit of staged records refuses while a filter is set and a file with
// records lacks the columns the filter reads: that file's verdicts cannot have been applied.
static int check_filter_columns(const pc_engine *e, const char *who) {
    for (size_t f = 0; f < e->files.size(); ++f) {
        const StagedFile *sf = e->files[f];
        if (sf->n == 0) continue;
        if (e->ff_max_nh && !sf->have_nh)
            return fail(PC_ERR_STATE, "%s: an NH filter is set but alignment file %d has no NH column (pc_set_alignment_nh)", who, (int)f);
        if (e->ff_on && !sf->have_sam)   // a file staged after pc_set_flag_filter gets its verdicts when its columns arrive: not counted without them
            return fail(PC_ERR_STATE, "%s: a FLAG / MAPQ filter is set but alignment file %d has no FLAG / MAPQ columns (pc_set_alignment_sam)", who, (int)f);
    }
    return PC_OK;
}

// the verdicts of the engine's FLAG / MAPQ / NH filter into the exclusion bits of one staged file (`on` 0: taken out again)
static void launch_flag_filter(pc_engine *e, StagedFile *sf, uint32_t on) {
    hipLaunchKernelGGL(k_flag_filter, dim3((unsigned)((sf->n + kWG - 1) / kWG)), dim3(kWG), 0, e->stream, sf->rec.p, sf->stream.p,
                       sf->have_sam ? sf->sam_flag.p : nullptr, sf->have_sam ? sf->sam_mapq.p : nullptr, sf->n, on,
                       e->ff_on ? e->ff_require : 0u, e->ff_on ? e->ff_exclude : 0u, e->ff_on ? e->ff_min_mapq : 0u,
                       sf->have_nh ? sf->sam_nh.p : nullptr, e->ff_max_nh);
}

int pc_update_flags(pc_engine *e, int file, int64_t n, const uint8_t *flags) {
    if (!e || file < 0 || file >= (int)e->files.size()) return fail(PC_ERR_ARG, "pc_update_flags: bad file index");
    StagedFile *sf = e->files[file];
    if (n != sf->n || (n > 0 && !flags)) return fail(PC_ERR_ARG, "pc_update_flags: wrong record count");
    HIP_TRY(hipSetDevice(e->device));
    if (n == 0) return PC_OK;
    // the flags go up (1 byte per record); every staged copy of the headers is patched in HBM
    PC_TRY(e->d_flags.reserve((size_t)n));
    hipStream_t st = e->stream;
    HIP_TRY(hipMemcpyAsync(e->d_flags.p, flags, (size_t)n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_update_flags, dim3((unsigned)((n + kWG - 1) / kWG)), dim3(kWG), 0, st, sf->rec.p, sf->stream.p,
                       e->d_flags.p, n);
    // (k_update_flags has left the caller's verdicts alone in the exclusion bits)
    sf->applied = FilterState();
    sf->applied_valid = true;
    if (e->filter_on() && columns_present(e, sf)) {   // the FLAG / MAPQ / NH filter's verdicts on top of the caller's
        launch_flag_filter(e, sf, 1u);
        sf->applied = e->filter_state();
    }
    const int prc = propagate_record_flags(e, sf);
    if (prc != PC_OK) return prc;
    HIP_TRY(hipStreamSynchronize(st)); // the caller's flag buffer may go away
    return PC_OK;
}

// The strand / excluded bits of the packed records have changed: copy them into every other staged form of the
// headers (side lists, run stream), rebuild the compact stream, drop what was derived from them (center streams, work
// lists).  Waits for the engine's stream (build_compact_stream reads the entry count back).
static int propagate_record_flags(pc_engine *e, StagedFile *sf) {
    hipStream_t st = e->stream;
    const struct { uint4 *rec; int64_t m; } side[3] = {{sf->long_rec.p, sf->nlong}, {sf->gap_rec.p, sf->ngap}, {sf->xlong_rec.p, sf->nxlong}};
    for (const auto &l : side)
        if (l.m) hipLaunchKernelGGL(k_update_side_flags, dim3((unsigned)((l.m + kWG - 1) / kWG)), dim3(kWG), 0, st, l.rec, l.m, sf->rec.p);
    if (sf->nrunrec)
        hipLaunchKernelGGL(k_update_run_flags, dim3((unsigned)((sf->nrunrec + kWG - 1) / kWG)), dim3(kWG), 0, st, sf->run_rec.p,
                           sf->run_recidx.p, sf->nrunrec, sf->rec.p);
    HIP_TRY(hipGetLastError());
    PC_TRY(build_compact_stream(e, sf, e->ntid));   // (the stream words have been rewritten)
    for (int k = 0; k < 3; ++k) sf->cs_n[k] = -1;   // the center streams leave excluded reads out: rebuilt at the next center count
    e->files_dirty = true;
    e->work_generation += 1;
    return PC_OK;
}

// (re-)apply the engine's FLAG / MAPQ filter to one staged file
static int apply_flag_filter(pc_engine *e, StagedFile *sf) {
    if (sf->n == 0) return PC_OK;
    if (e->ff_on && !sf->have_sam)
        return fail(PC_ERR_STATE, "a FLAG / MAPQ filter is set but an alignment file was staged without its FLAG / MAPQ columns (pc_set_alignment_sam)");
    if (e->ff_max_nh && !sf->have_nh)
        return fail(PC_ERR_STATE, "an NH filter is set but an alignment file was staged without its NH column (pc_set_alignment_nh)");
    if (!sf->have_sam && !sf->have_nh && !e->filter_on()) {
        // nothing to read the verdicts from, and nothing to undo: a file without the columns never had the filter applied
        return PC_OK;
    }
    launch_flag_filter(e, sf, e->filter_on() ? 1u : 0u);
    sf->applied = e->filter_state();
    sf->applied_valid = true;
    return propagate_record_flags(e, sf);
}

// After any change of the filter or of a file's columns: bring the verdicts of every file up to date whose columns
// allow it (the others are refused by check_filter_columns until theirs arrive).  A file whose exclusion bits already
// hold the verdicts of the current filter costs nothing.
static int sync_flag_filter(pc_engine *e) {
    const FilterState want = e->filter_state();
    for (StagedFile *sf : e->files) {
        if (sf->n == 0 || !columns_present(e, sf)) continue;
        if (sf->applied_valid && sf->applied == want) continue;
        PC_TRY(apply_flag_filter(e, sf));
    }
    return PC_OK;
}

int pc_set_alignment_sam(pc_engine *e, int file, int64_t n, const uint16_t *flag, const uint8_t *mapq) {
    if (!e || file < 0 || file >= (int)e->files.size()) return fail(PC_ERR_ARG, "pc_set_alignment_sam: bad file index");
    StagedFile *sf = e->files[file];
    if (n != sf->n || (n > 0 && (!flag || !mapq))) return fail(PC_ERR_ARG, "pc_set_alignment_sam: wrong record count");
    HIP_TRY(hipSetDevice(e->device));
    if (n > 0) {
        PoolScope pool_scope(&e->pool);
        int rc = sf->sam_flag.reserve((size_t)n);
        room(rc, sf->sam_mapq, (size_t)n);
        if (rc != PC_OK) return rc;
        HIP_TRY(hipMemcpyAsync(sf->sam_flag.p, flag, (size_t)n * 2, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(sf->sam_mapq.p, mapq, (size_t)n, hipMemcpyHostToDevice, e->stream));
    }
    sf->have_sam = true;
    if (e->ff_on || sf->applied.ff_on) sf->applied_valid = false;   // verdicts read from the columns just replaced, if any
    const int rc = sync_flag_filter(e);
    HIP_TRY(hipStreamSynchronize(e->stream));   // the caller's arrays may go away
    return rc;
}

int pc_set_alignment_nh(pc_engine *e, int file, int64_t n, const uint16_t *nh) {
    if (!e || file < 0 || file >= (int)e->files.size()) return fail(PC_ERR_ARG, "pc_set_alignment_nh: bad file index");
    StagedFile *sf = e->files[file];
    if (n != sf->n || (n > 0 && !nh)) return fail(PC_ERR_ARG, "pc_set_alignment_nh: wrong record count");
    HIP_TRY(hipSetDevice(e->device));
    if (n > 0) {
        PoolScope pool_scope(&e->pool);
        PC_TRY(sf->sam_nh.reserve((size_t)n));
        HIP_TRY(hipMemcpyAsync(sf->sam_nh.p, nh, (size_t)n * 2, hipMemcpyHostToDevice, e->stream));
    }
    sf->have_nh = true;
    if (e->ff_max_nh || sf->applied.max_nh) sf->applied_valid = false;
    const int rc = sync_flag_filter(e);
    HIP_TRY(hipStreamSynchronize(e->stream));   // the caller's array may go away
    return rc;
}

int pc_set_nh_filter(pc_engine *e, int max_nh) {
    if (!e) return fail(PC_ERR_ARG, "engine is NULL");
    if (max_nh < 0 || max_nh > 65535) return fail(PC_ERR_ARG, "pc_set_nh_filter: max_nh is 0 (off) .. 65535");
    if (max_nh)
        for (size_t f = 0; f < e->files.size(); ++f)
            if (e->files[f]->n > 0 && !e->files[f]->have_nh)
                return fail(PC_ERR_STATE, "pc_set_nh_filter: alignment file %d was staged without its NH column (pc_set_alignment_nh)", (int)f);
    HIP_TRY(hipSetDevice(e->device));
    if (e->ff_max_nh == (uint32_t)max_nh) return PC_OK;
    e->ff_max_nh = (uint32_t)max_nh;
    return sync_flag_filter(e);
}

int pc_set_flag_filter(pc_engine *e, int enabled, uint32_t require, uint32_t exclude, int min_mapq) {
    if (!e) return fail(PC_ERR_ARG, "engine is NULL");
    if (enabled && (require > 0xffffu || exclude > 0xffffu || min_mapq < 0 || min_mapq > 255))
        return fail(PC_ERR_ARG, "pc_set_flag_filter: FLAG masks are 16-bit, MAPQ is 0 .. 255");
    if (enabled)
        for (size_t f = 0; f < e->files.size(); ++f)
            if (e->files[f]->n > 0 && !e->files[f]->have_sam)
                return fail(PC_ERR_STATE, "pc_set_flag_filter: alignment file %d was staged without its FLAG / MAPQ columns (pc_set_alignment_sam)", (int)f);
    HIP_TRY(hipSetDevice(e->device));
    const bool was_on = e->ff_on;
    const bool same = was_on == (enabled != 0) && (!enabled || (e->ff_require == require && e->ff_exclude == exclude && e->ff_min_mapq == (uint32_t)min_mapq));
    if (same) return PC_OK;
    e->ff_on = enabled != 0;
    e->ff_require = enabled ? require : 0u; e->ff_exclude = enabled ? exclude : 0u; e->ff_min_mapq = enabled ? (uint32_t)min_mapq : 0u;
    return sync_flag_filter(e);
}

int pc_set_mapping(pc_engine *e, int kind, int param, const int32_t *fw, const int32_t *rc, int table_len,
                   int min_len, int max_len) {
    if (!e) return fail(PC_ERR_ARG, "engine is NULL");
    if (kind < PC_MAP_FIVE || kind > PC_MAP_STRAT5) return fail(PC_ERR_ARG, "pc_set_mapping: unknown kind %d", kind);
    if ((kind == PC_MAP_FIVE || kind == PC_MAP_THREE || kind == PC_MAP_CENTER) && param < 0)
        return fail(PC_ERR_ARG, "pc_set_mapping: offset/nibble must be >= 0, got %d", param);
    int rows = 1;
    if (kind == PC_MAP_VAR5 || kind == PC_MAP_STRAT5) {
        if (!fw || !rc || table_len <= 0 || table_len > 65536) return fail(PC_ERR_ARG, "pc_set_mapping: offset tables required");
        for (int L = 0; L < table_len; ++L) {
            if (fw[L] < -1 || rc[L] < -1 || (fw[L] >= 0 && fw[L] >= std::max(L, 1)) || (rc[L] >= 0 && rc[L] >= std::max(L, 1)))
                return fail(PC_ERR_ARG, "pc_set_mapping: table entry for length %d out of range (the reference would index read.positions out of bounds)", L);
            if ((fw[L] < 0) != (rc[L] < 0)) return fail(PC_ERR_ARG, "pc_set_mapping: forward/reverse tables disagree on length %d", L);
        }
    }
    if (kind == PC_MAP_STRAT5) {
        if (max_len <= min_len) return fail(PC_ERR_ARG, "pc_set_mapping: max length must be > min length"); // :716-717
        if (max_len >= table_len) return fail(PC_ERR_ARG, "pc_set_mapping: max length beyond offset table");
        rows = max_len - min_len + 1;
    }
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->kind = kind; e->param = param; e->min_len = min_len; e->max_len = max_len; e->rows = rows;
    e->table_len = 0;
    e->h_fw.clear(); e->h_rc.clear();
    if (kind == PC_MAP_VAR5 || kind == PC_MAP_STRAT5) {
        e->h_fw.assign(fw, fw + table_len);
        e->h_rc.assign(rc, rc + table_len);
        int r = e->d_fw.upload(e->h_fw, e->stream);
        if (r == PC_OK) r = e->d_rc.upload(e->h_rc, e->stream);
        if (r != PC_OK) return r;
        HIP_TRY(hipStreamSynchronize(e->stream));
        e->table_len = table_len;
    }
    e->have_map = true;
    return PC_OK;
}

int pc_set_size_filter(pc_engine *e, int enabled, int min_len, int max_len) {
    if (!e) return fail(PC_ERR_ARG, "engine is NULL");
    if (enabled) {
        if (max_len != -1 && max_len < min_len) return fail(PC_ERR_ARG, "Alignment size filter: max read length must be >= min read length");
        if (min_len < 1) return fail(PC_ERR_ARG, "Alignment size filter: min read length must be >= 1. Got %d", min_len);
    }
    e->filt_on = enabled ? 1 : 0;
    e->filt_min = min_len;
    e->filt_max = max_len;
    return PC_OK;
}

int pc_set_normalize(pc_engine *e, int enabled, double sum) {
    if (!e) return fail(PC_ERR_ARG, "engine is NULL");
    e->norm_on = enabled ? 1 : 0;
    e->norm_sum = sum;
    return PC_OK;
}

int pc_mapping_rows(pc_engine *e) { return e ? e->rows : 0; }

// ------------------------------------------------------------------ plan
int pc_plan_create(pc_engine *e, int64_t nseg, const int32_t *tid, const int64_t *start, const int64_t *end,
                   const uint8_t *strand, const int64_t *out_off, const int8_t *out_step,
                   const int64_t *row_stride, int64_t out_elems, int rows, pc_plan **out) {
    if (!e || !out) return fail(PC_ERR_ARG, "pc_plan_create: NULL argument");
    *out = nullptr;
    if (nseg < 0 || out_elems < 0 || rows < 1) return fail(PC_ERR_ARG, "pc_plan_create: bad sizes");
    if (nseg > 0 && (!tid || !start || !end || !strand || !out_off || !out_step || !row_stride))
        return fail(PC_ERR_ARG, "pc_plan_create: NULL array");
    if (nseg >= (int64_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_plan_create: too many segments");
    HIP_TRY(hipSetDevice(e->device));

    // large annotations: every pass of the builder as a kernel, a radix sort or a scan (plan_kernels.hip.h); small plans
    // -- and PC_PLAN_BUILD=host -- take the serial host builder (plan_host.h), which the GPU tables are tested against
    const bool on_gpu = nseg > 0 && (int64_t)e->ntid < ((int64_t)1 << pcplan::kTidBits) &&
                        (e->knobs.plan_build == 2 || (e->knobs.plan_build == 0 && nseg >= (1 << 13)));
    HostPlan hp;
    if (!on_gpu) {
        PlanDefect bad;
        if (!build_plan_host({nseg, tid, start, end, strand, out_off, out_step, row_stride}, e->ntid, rows, out_elems, e->knobs.tile_g, hp, bad))
            return fail(PC_ERR_ARG, "%s", plan_defect_message(bad, out_elems).c_str());
    }
    pc_plan *p = new pc_plan(e);
    p->nseg = nseg;
    p->out_elems = out_elems;
    p->rows = rows;
    int rc;
    if (on_gpu) rc = plan_build_gpu(e, p, {nseg, tid, start, end, strand, out_off, out_step, row_stride}, out_elems, rows);
    else {
        p->G = hp.G; p->modes = hp.modes; p->max_slots = hp.max_slots; p->npos = hp.npos;
        p->covered = hp.covered; p->has_sums = hp.has_sums; p->out_needs_zero = hp.out_needs_zero;
        p->host = std::move(hp);
        p->h_tid.assign(tid, tid + nseg);
        p->h_start.assign(start, start + nseg);
        p->h_end.assign(end, end + nseg);
        p->h_strand.assign(strand, strand + nseg);
        rc = plan_upload(e, p);
    }
    if (rc != PC_OK) {
        (void)hipStreamSynchronize(e->stream);   // copies out of the plan's vectors may be in flight
        delete p;
        return rc;
    }
    *out = p;
    return PC_OK;
}

int pc_plan_destroy(pc_plan *p) {
    if (!p) return PC_OK;
    if (p->e) {
        (void)hipSetDevice(p->e->device);
        (void)hipStreamSynchronize(p->e->stream);
    }
    delete p;
    return PC_OK;
}

int64_t pc_plan_positions(pc_plan *p) { return p ? p->npos : -1; }
int64_t pc_plan_tiles(pc_plan *p) { return p ? (int64_t)p->n_tiles : -1; }

int pc_plan_table(pc_plan *p, int which, void *buf, int64_t cap_bytes, int64_t *bytes) {
    if (!p || !bytes || which < 0 || which > 4 || cap_bytes < 0 || (cap_bytes > 0 && !buf)) return fail(PC_ERR_ARG, "pc_plan_table: bad arguments");
    HIP_TRY(hipSetDevice(p->e->device));
    HIP_TRY(hipStreamSynchronize(p->e->stream));
    if (which == 4) {
        const int64_t v[12] = {p->G, (int64_t)p->modes, p->max_slots, p->npos, p->covered, p->has_sums ? 1 : 0, p->out_needs_zero ? 1 : 0,
                               (int64_t)p->n_tiles, (int64_t)p->n_pieces, (int64_t)p->n_opieces, p->gpu_built ? 1 : 0, p->nseg};
        *bytes = (int64_t)sizeof(v);
        std::memcpy(buf, v, (size_t)std::min<int64_t>(cap_bytes, *bytes));
        return PC_OK;
    }
    const void *src = nullptr;
    size_t n = 0;
    bool on_host = false;
    if (which == 0) { src = p->d_tiles.p; n = p->n_tiles * sizeof(Tile); }
    else if (which == 1) { src = p->d_pieces.p; n = p->n_pieces * sizeof(Piece); }
    else if (which == 2) { src = p->d_opieces.p; n = p->n_opieces * sizeof(OutPiece); }
    else if (p->gpu_built) { src = p->d_gsegs_own.p; n = (size_t)p->nseg * sizeof(GatherSeg); }
    else { src = p->host.gsegs.data(); n = p->host.gsegs.size() * sizeof(GatherSeg); on_host = true; }
    *bytes = (int64_t)n;
    const size_t take = (size_t)std::min<int64_t>(cap_bytes, (int64_t)n);
    if (take) {
        if (on_host) std::memcpy(buf, src, take);
        else HIP_TRY(hipMemcpy(buf, src, take, hipMemcpyDeviceToHost));
    }
    return PC_OK;
}

} // extern "C"

namespace {

// ---- run-time values turned into template arguments: `launch` is a generic lambda; it receives the std::integral_constant
// of the one of Vs that equals v and launches the instantiation it names
template <int... Vs, class F>
void dispatch_int(int v, F &&launch) {
    (void)((v == Vs ? (launch(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// (mapping rule, output mode: 0 int64, 1 float64, 2 normalised float64) -> (KIND, OUTMODE) of k_hist_point.  The one-window
// callers (a plan of one window, pc_query_segment) never run under the stratified rule: they pass STRAT = false and its
// kernels are not instantiated.
template <bool STRAT, class F>
void dispatch_hist(int kind, int outmode, F &&launch) {
    const int k = kind == PC_MAP_FIVE ? 0 : kind == PC_MAP_THREE ? 1 : (STRAT && kind == PC_MAP_STRAT5) ? 4 : 3;
    dispatch_int<0, 1, 2>(outmode, [&](auto O) {
        if constexpr (STRAT) dispatch_int<0, 1, 3, 4>(k, [&](auto K) { launch(K, O); });
        else dispatch_int<0, 1, 3>(k, [&](auto K) { launch(K, O); });
    });
}

// ---- the dynamic LDS of k_hist_point behind its bins (count_host.h) for the engine's rule and files; hist_lds_bytes
// puts the bins of a window in front
using pccount::HistLds;

HistLds hist_lds_shape(const pc_engine *e) {
    std::vector<pccount::LenRange> r;
    r.reserve(e->files.size());
    for (auto *f : e->files) r.push_back({f->len_min, f->len_max, f->tlen_min, f->tlen_max});
    return pccount::hist_lds_shape(e->kind, e->table_len, r.data(), (int)r.size());
}

// ---- pc_count, phase by phase.  The phases enqueue on e->stream (the sparse-window class on e->side_stream) in the
// order they are called and record the events pc_last_timing reads: ev[0] in front of the output memset, ev[1] behind
// the memsets, ev[2] in front of the first k_hist_point (behind the work lists) or of the center kernels, ev[3] and
// ev[4] behind the join, ev[5] behind k_gather_split.  A plan without windows records all of them as well.
struct CountCall {   // what the phases of one call share beside the engine and the plan
    int out_dtype;
    int outmode;           // OUTMODE of the kernels that write the output
    int nfiles, ntiles;
    int64_t nrec, nextra;  // records and extra runs of all files
    size_t hist_bytes;     // the compact histogram (uint32 per island position and row): what merged windows of the point rules go through; the center rule does not use it
    MapParams mp;
};

int mark(pc_engine *e, int k) {   // ev[1] and ev[4] from profiling level 2, the others from level 1
    if (e->prof_level >= ((k == 1 || k == 4) ? 2 : 1)) HIP_TRY(hipEventRecord(e->ev[k], e->stream));
    return PC_OK;
}

int count_validate(pc_engine *e, pc_plan *p, int out_dtype) {   // (no HIP call)
    if (!e || !p || p->e != e) return fail(PC_ERR_ARG, "pc_count: bad engine/plan");
    if (!e->have_map) return fail(PC_ERR_STATE, "pc_count: no mapping rule set (pc_set_mapping)");
    if (e->files.empty()) return fail(PC_ERR_STATE, "pc_count: no alignments staged (pc_add_alignment_file)");
    if (out_dtype != PC_OUT_INT64 && out_dtype != PC_OUT_FLOAT64) return fail(PC_ERR_ARG, "pc_count: bad out_dtype");
    if (p->rows != e->rows) return fail(PC_ERR_ARG, "pc_count: plan built for %d rows, mapping rule has %d", p->rows, e->rows);
    PC_TRY(check_filter_columns(e, "pc_count"));
    const bool float_only = e->kind == PC_MAP_CENTER || e->norm_on;
    if (float_only && out_dtype != PC_OUT_FLOAT64)
        return fail(PC_ERR_ARG, "pc_count: center mapping / normalisation produce float64 (map_factories.pyx:230, genome_array.py:826-827)");
    if (p->has_sums && float_only)
        return fail(PC_ERR_ARG, "pc_count: summed slices (out_step 0) need an integer mapping rule without normalisation");
    return PC_OK;
}

int count_prepare(pc_engine *e, pc_plan *p, bool dense) {   // dense: served from a dense vector -- no compact histogram
    const bool center = e->kind == PC_MAP_CENTER;
    if (center) {   // the center-only tables of a large plan; the center streams of the strand selections it queries
        PC_TRY(ensure_center_tables(e, p));
        const bool need[3] = {(p->modes & 1u) != 0, (p->modes & 2u) != 0, (p->modes & 12u) != 0};
        for (auto *f : e->files)
            for (int k = 0; k < 3; ++k)
                if (need[k]) PC_TRY(build_center_stream(e, f, k, e->param));   // (no-op when built for this nibble)
    }
    PC_TRY(refresh_file_views(e));
    if (!center && !dense && !p->d_hist.p) {
        const int rc = p->d_hist_own.reserve(std::max<size_t>((size_t)p->npos * p->rows * sizeof(uint32_t), 8));
        p->d_hist.p = p->d_hist_own.p;
        PC_TRY(rc);
    }
    return p->d_out.reserve(std::max<size_t>((size_t)p->out_elems * 8, 8));
}

int ensure_dense_tables(pc_engine *e, pc_plan *p, const StagedFile *sf);   // (below, with the dense vector)

// `dense`: the file whose vector serves this count (dense_for_plan), else nullptr; *path: which gather will (pc_dense_path)
int count_clear(pc_engine *e, pc_plan *p, const CountCall &c, const StagedFile *dense, int *path) {
    const bool center = e->kind == PC_MAP_CENTER;
    PC_TRY(mark(e, 0));
    // A count served from a dense vector: the plan's one-time tables are made here, behind mark 0, so that last_timing()
    // of a first count holds them.  By chunks or by items: dense_by_chunks (count_host.h)
    int dense_path = PC_DENSE_PATH_NONE;
    if (dense) {
        PC_TRY(ensure_dense_tables(e, p, dense));
        const bool chunks = pccount::dense_by_chunks(p->chunks_ok, p->dchunks_id == dense->did, e->knobs.dense_items, (uintptr_t)p->d_out.p);
        dense_path = chunks ? PC_DENSE_PATH_CHUNKS : PC_DENSE_PATH_ITEMS;
    }
    *path = dense_path;
    // what the kernels of the path leave unwritten is cleared (out_needs_memset); the compact histogram of the point
    // rules is kept all-zero between calls
    const pccount::OutPath out_path = dense_path == PC_DENSE_PATH_CHUNKS ? pccount::kOutChunks : (dense_path == PC_DENSE_PATH_ITEMS ? pccount::kOutItems : pccount::kOutWindows);
    if (pccount::out_needs_memset(out_path, p->has_sums, p->out_needs_zero, p->covered, p->out_elems))
        HIP_TRY(hipMemsetAsync(p->d_out.p, 0, (size_t)p->out_elems * 8, e->stream));
    if (dense_path != PC_DENSE_PATH_NONE) return mark(e, 1);
    // `hist_clean` says that the WHOLE histogram is zero: true once it has been cleared as a whole, and kept by every
    // count (k_clear_split only zeroes, k_gather_split zeroes what it merged).  Lazy counts never make it true, so the
    // first count after the knobs turn lazy off (pc_reload_knobs) clears what the lazy ones left alone.
    p->hist_lazy = pccount::hist_lazy(center, (int64_t)c.hist_bytes, e->knobs.hist_lazy_bytes, e->knobs.hist_memset);
    if (!center && c.hist_bytes && !p->hist_clean && !p->hist_lazy) {
        HIP_TRY(hipMemsetAsync(p->d_hist.p, 0, c.hist_bytes, e->stream));
        p->hist_clean = true;
    }
    return mark(e, 1);
}

// ---- a plan of ONE window over one file (`ga[segment]`): the whole count is one launch -- the workgroup looks its
// record ranges up itself; no work list, no second window class, no merge pass, no events
int count_single(pc_engine *e, pc_plan *p, const CountCall &c) {
    const HistLds s = hist_lds_shape(e);
    const size_t lds = pccount::hist_lds_bytes(s, (size_t)p->max_slots * p->rows, p->G, false);
    if (lds > e->max_lds)
        return fail(PC_ERR_ARG, "pc_count: the window needs %zu bytes of LDS, the device offers %zu per workgroup (too many rows)", lds, e->max_lds);
    const FileView fv0 = e->files[0]->view();
    PC_TRY(mark(e, 2));
    dispatch_hist<false>(e->kind, c.outmode, [&](auto K, auto O) {
        constexpr int k = decltype(K)::value, o = decltype(O)::value;
        hipLaunchKernelGGL((k_hist_point<k, o, kHistWG, false, false, true>), dim3(1), dim3(kHistWG), lds, e->stream, p->d_pieces.p, p->d_opieces.p,
                           fv0, fv0, e->d_files.p, (const WorkItem *)p->d_tiles.p, p->d_wcounters.p, p->d_tile_items.p, c.mp, p->G, p->max_slots,
                           s.tab_lo, s.tab_n, s.fast_lo, s.fast_hi, (uint32_t *)p->d_hist.p, (int64_t)e->Ws(), (typename OutT_<o>::type *)p->d_out.p,
                           e->norm_sum, (uint32_t)e->Wg(), (uint32_t)e->Wr(), (const FileRange *)nullptr, c.nfiles, Tile{}, OutPiece{}, (uint32_t *)nullptr, 0u);
    });
    PC_TRY(mark(e, 3));
    return mark(e, 4);
}

// ---- the work lists of a point-rule count
struct WorkLists {
    int64_t cap = 0, cap_small = 0;   // capacity of the list of the dense windows, of the sparse ones
    int small_g = 0;                  // window of the sparse class (0: no such class)
    pc_plan::WorkKey key;
    HistLds shape;                    // dynamic LDS of k_hist_point: what both classes share, and the bytes of either
    size_t lds = 0, lds_small = 0;
    pccount::Grids grids;             // of both classes: the whole capacity, or exactly the queued items (choose_grids)
};

int size_work_lists(pc_engine *e, pc_plan *p, const CountCall &c, WorkLists &w) {
    const int nfiles = c.nfiles, G = p->G;
    const bool b16 = e->kind == PC_MAP_STRAT5;   // 16-bit bins, two positions per word (k_hist_point)
    pccount::WorkIn in;
    in.ntiles = c.ntiles; in.nfiles = nfiles; in.G = G; in.rows = p->rows; in.modes = p->modes; in.npos = p->npos;
    in.nrec = c.nrec; in.nextra = c.nextra;
    for (auto *f : e->files) { in.nxlong += f->nxlong; in.ngap += f->ngap; }
    in.W = e->W(); in.Ws = e->Ws(); in.Wg = e->Wg(); in.Wr = e->Wr();
    in.R = e->knobs.work_r; in.pile = e->knobs.pile;
    in.no_small = e->knobs.no_small; in.small_rows = e->knobs.small_rows; in.small_g = e->knobs.small_g;
    in.stratified = b16;
    const pccount::WorkSizes ws = pccount::work_list_sizes(in);   // the capacities: upper bounds (count_host.h)
    if (ws.too_large) return fail(PC_ERR_ARG, "pc_count: work list too large");
    const int64_t R = in.R, pile = ws.pile;
    w.cap = ws.cap; w.small_g = ws.small_g; w.cap_small = ws.cap_small;
    PC_TRY(p->d_work.reserve((size_t)w.cap));
    PC_TRY(p->d_work_small.reserve((size_t)std::max<int64_t>(w.cap_small, 1)));
    if (nfiles > 1) {
        PC_TRY(p->d_chain.reserve((size_t)w.cap * (size_t)(nfiles - 1)));
        PC_TRY(p->d_chain_small.reserve((size_t)std::max<int64_t>(w.cap_small, 1) * (size_t)(nfiles - 1)));
    }
    pc_plan::WorkKey &key = w.key;
    key.generation = e->work_generation; key.nfiles = nfiles; key.G = G; key.Wg = e->Wg(); key.Ws = e->Ws(); key.Wr = e->Wr();
    key.small_g = w.small_g; key.R = R; key.pile = pile; key.small_n = e->knobs.small_n; key.cap = w.cap;
    w.shape = hist_lds_shape(e);
    const size_t slot_words = (size_t)p->max_slots * p->rows;   // bin words per window position (per two, with 16-bit bins)
    w.lds = pccount::hist_lds_bytes(w.shape, slot_words, G, b16);
    w.lds_small = pccount::hist_lds_bytes(w.shape, slot_words, w.small_g, b16);
    return PC_OK;
}

// the engine's rule and size filter over the file's stream words: what its canonical stream and its dense vector hang on
pccount::RuleSig rule_sig(const pc_engine *e, const StagedFile *sf) {
    return pccount::rule_sig(e->kind, e->param, e->filt_on, e->filt_min, e->filt_max, sf->words_gen, e->h_fw, e->h_rc);
}

// ---- the canonical stream of the plan's file under the engine's rule and size filter (stage_kernels.hip.h,
// canon_host.h).  Used by the plans of stream_plan_conditions (count_host.h: ONE file, a point rule without rows,
// windows '+' and '-' only), and only when
// it has at most `compact_keep` of the entries of the stream it replaces (the compact stream's own rule).  Built at the
// first count that wants it and kept on the file under its signature: rule, filter, entry-table range, halo and the
// generation of the stream words.  A steady-state count compares the signature and goes on; a build allocates from the
// engine's pool and reads the entry total back once.  `canon`: the file's stream when it is to be used, else nullptr.
int canonical_for_plan(pc_engine *e, pc_plan *p, const CountCall &c, const HistLds &shape, StagedFile **canon) {
    using namespace pcstage;
    *canon = nullptr;
    if (e->knobs.no_canon || !pccount::stream_plan_conditions(c.nfiles, e->kind, p->rows, p->modes)) return PC_OK;
    StagedFile *sf = e->files[0];
    if (sf->n <= 0 || !sf->nlin) return PC_OK;
    CanonSig sig;
    sig.rule = rule_sig(e, sf);
    sig.fast_lo = shape.fast_lo; sig.fast_hi = shape.fast_hi; sig.Ws = e->Ws();
    if (!(sf->ksig_valid && sf->ksig == sig)) {
        sf->ksig_valid = false;
        sf->kn = -1;
        const pccanon::CanonRule cr = pccanon::canon_rule(pccount::canon_rule_in(sig, e->table_len));
        if (cr.usable && pccanon::canon_fits_halo(cr, sig.Ws)) {
            PoolScope pool_scope(&e->pool);
            hipStream_t st = e->stream;
            const int64_t nlin = (int64_t)sf->nlin;
            PC_TRY(sf->klin_tab.reserve((size_t)nlin + 1));
            PC_TRY(sf->kshift.reserve(2 * pccanon::kLenSlots));
            DevBuf<uint8_t> d_scan;
            auto sum_buckets = [=](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, sf->klin_tab.p, sf->klin_tab.p, (int)nlin + 1, st); };
            size_t most = 16, tb = 0;
            PC_TRY(cub_need(most, tb, sum_buckets));
            PC_TRY(d_scan.reserve(most));
            HIP_TRY(hipMemcpyAsync(sf->kshift.p, cr.shift, sizeof(cr.shift), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemsetAsync(sf->klin_tab.p + nlin, 0, 4, st));
            const int back = pccanon::canon_buckets_back(cr, kLinShift);
            const uint32_t lc0 = (uint32_t)cr.Lc[0] << 4, lc1 = ((uint32_t)cr.Lc[1] << 4) | 4u;
            hipLaunchKernelGGL((k_canon_buckets<false>), dim3((unsigned)std::min<int64_t>(nlin, kCanonMaxGrid)), dim3(256), 0, st, sf->stream.p, sf->lin_tab.p, sf->lin_off.p, e->ntid, nlin,
                               sf->kshift.p, back, lc0, lc1, sf->klin_tab.p, (uint32_t *)nullptr);
            hipError_t he = cub_enqueue(d_scan.p, tb, sum_buckets);
            uint32_t total = 0;
            if (he == hipSuccess) he = hipMemcpyAsync(&total, sf->klin_tab.p + nlin, 4, hipMemcpyDeviceToHost, st);
            if (he == hipSuccess) he = hipGetLastError();
            if (he == hipSuccess) he = hipStreamSynchronize(st);   // (the shift table on the host and the scan's scratch go out of scope)
            if (he != hipSuccess) return fail(PC_ERR_HIP, "building the canonical stream failed: %s", hipGetErrorString(he));
            const int64_t replaces = sf->cn >= 0 ? sf->cn : sf->n;
            if ((double)total <= e->knobs.compact_keep * (double)replaces) {
                PC_TRY(sf->kstream.reserve((size_t)total + 8));
                hipLaunchKernelGGL((k_canon_buckets<true>), dim3((unsigned)std::min<int64_t>(nlin, kCanonMaxGrid)), dim3(256), 0, st, sf->stream.p, sf->lin_tab.p, sf->lin_off.p, e->ntid, nlin,
                                   sf->kshift.p, back, lc0, lc1, sf->klin_tab.p, sf->kstream.p);
                hipLaunchKernelGGL(k_canon_pad, dim3(1), dim3(64), 0, st, sf->klin_tab.p, nlin, sf->kstream.p);
                HIP_TRY(hipGetLastError());
                sf->kn = (int64_t)total;
            }
        }
        if (sf->kn < 0) { sf->kstream.release(); sf->klin_tab.release(); }
        sf->ksig = sig;
        sf->ksig_valid = true;
        sf->kid += 1;
    }
    if (sf->kn >= 0) *canon = sf;
    return PC_OK;
}

// the view the window kernels get of the plan's first file: its canonical stream in the compact stream's place
FileView hist_view(pc_engine *e, const StagedFile *canon) {
    FileView v = e->files[0]->view();
    if (canon) { v.cstream = canon->kstream.p; v.clin_tab = canon->klin_tab.p; }
    return v;
}

int build_work_lists(pc_engine *e, pc_plan *p, const CountCall &c, const WorkLists &w, const StagedFile *canon) {
    hipStream_t st = e->stream;
    const int ntiles = c.ntiles;
    // the lists of this plan are (re)built: counters and per-tile item counts start from zero (they arrive
    // zeroed with the plan's tables, so the first count of a plan needs no memset)
    if (!p->wcounters_zero) HIP_TRY(hipMemsetAsync(p->d_wcounters.p, 0, 8 * sizeof(uint32_t), st));
    if (!p->tile_items_zero) HIP_TRY(hipMemsetAsync(p->d_tile_items.p, 0, ((size_t)ntiles + 1) * sizeof(uint32_t), st));
    p->wcounters_zero = false;
    p->tile_items_zero = false;
    // one thread per window (several files: joint windows), or sixteen lanes per window while that still fits the chip at
    // once: the exact record bounds of a window are then searched by the group (three rounds of sixteen probes instead of a
    // dozen dependent loads each) -- a plan of a few thousand windows (C2: 6 144) otherwise runs on two dozen CUs at the
    // pace of one thread's load chain
    const int64_t nwin = ntiles;
    const int lanes = (nwin * 16 <= e->knobs.ranges_cg16_max && !e->knobs.ranges_cg1) ? 16 : 1;
    dispatch_int<16, 1>(lanes, [&](auto CG) {
        hipLaunchKernelGGL((k_tile_ranges<decltype(CG)::value>), dim3((unsigned)((nwin * lanes + kRangesWG - 1) / kRangesWG)), dim3(kRangesWG), 0, st, p->d_tiles.p, ntiles,
                           hist_view(e, canon), e->d_files.p, c.nfiles, p->G, e->Wg(), e->Ws(), e->Wr(), w.key.R, w.key.pile, p->d_work.p, p->d_wcounters.p, p->d_tile_items.p, (uint32_t)w.cap,
                           p->d_work_small.p, w.small_g, w.key.small_n, e->knobs.debug_work, p->d_chain.p, p->d_chain_small.p, e->kind == PC_MAP_STRAT5 ? 1 : 0);
    });
    if (p->hist_lazy)
        hipLaunchKernelGGL(k_clear_split, dim3((unsigned)((ntiles + kClearPerWG - 1) / kClearPerWG)), dim3(kWG), 0, st, p->d_tiles.p, ntiles,
                           p->d_pieces.p, p->d_tile_items.p, p->d_wcounters.p, p->rows, (uint32_t *)p->d_hist.p, (int64_t)p->npos);
    p->work_key = w.key;
    p->work_valid = true;
    p->work_counts.known = false;      // the counts of the lists just replaced size no grid
    p->guard_pending = true;           // k_gather_split checks the new lists against the capacity: read with the results
    p->work_counts.generation = 0;
    // The first count of a plan does not know how many items its lists hold, and used to launch the whole
    // capacity: for a sparse annotation under a multi-row rule that is 3.6 M workgroups for 0.53 M items (C5:
    // 3.88 ms against 3.24, and the merge pass on top).  Where the capacity is far above the window count, the
    // queued counts are read back NOW -- one small copy and a stream synchronisation, ~20 us of idle GPU -- and
    // this count already launches exact grids.
    const int64_t spare = w.cap + w.cap_small - nwin;
    if (ntiles >= 4096 && spare >= e->knobs.first_sync_spare && !e->knobs.test_stale_counts && !e->knobs.debug_work) {
        QueuedCounts &q = p->work_counts;   // (read in place: a copy and a wait, no event)
        PC_TRY(q.ensure(8));
        HIP_TRY(hipMemcpyAsync(q.host, p->d_wcounters.p, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        q.known = true;
        q.generation = e->work_generation;
    }
    return PC_OK;
}

// the whole list capacity, or what the read-back of an earlier count of these lists says they hold (count_host.h)
void choose_grids(pc_engine *e, pc_plan *p, const CountCall &c, WorkLists &w) {
    QueuedCounts &q = p->work_counts;
    const bool tracked = c.ntiles >= 4096 && q.generation == e->work_generation;   // (small plans do not track their counts)
    const bool known = tracked && q.poll();
    w.grids = pccount::choose_grids(c.ntiles, tracked, known, q.host, w.cap, w.cap_small, e->knobs.test_stale_counts != 0);
    if (w.grids.exact) p->exact_grid_used = true;
}

// sparse windows (single-wave workgroups) and dense ones are two independent launches over
// disjoint windows: they run side by side on two streams, forked after the work lists exist
// and joined before the last kernel of the call
int launch_hist(pc_engine *e, pc_plan *p, const CountCall &c, const WorkLists &w, const StagedFile *canon) {
    const HistLds &s = w.shape;
    const int nfiles = c.nfiles;
    const FileView fv0 = hist_view(e, canon);
    const FileView fv1 = nfiles > 1 ? e->files[1]->view() : fv0;
    hipStream_t st = e->stream, st_small = e->side_stream;
    if (w.cap_small) {
        HIP_TRY(hipEventRecord(e->ev_fork, st));
        HIP_TRY(hipStreamWaitEvent(st_small, e->ev_fork, 0));
    }
    dispatch_hist<true>(e->kind, c.outmode, [&](auto K, auto O) {
        dispatch_int<0, 1>(nfiles > 1, [&](auto M) {
            constexpr int k = decltype(K)::value, o = decltype(O)::value;
            constexpr bool m = decltype(M)::value != 0;
            typename OutT_<o>::type *out = (typename OutT_<o>::type *)p->d_out.p;
            hipLaunchKernelGGL((k_hist_point<k, o, kHistWG, false, m>), dim3(w.grids.grid), dim3(kHistWG), w.lds, st, p->d_pieces.p,
                               p->d_opieces.p, fv0, fv1, e->d_files.p, p->d_work.p, p->d_wcounters.p, p->d_tile_items.p, c.mp,
                               p->G, p->max_slots, s.tab_lo, s.tab_n, s.fast_lo, s.fast_hi, (uint32_t *)p->d_hist.p, p->npos, out,
                               e->norm_sum, (uint32_t)w.cap, w.grids.grid_front, p->d_chain.p, nfiles, Tile{}, OutPiece{}, (uint32_t *)nullptr, 0u);
            if (w.cap_small && w.grids.grid_small)
                hipLaunchKernelGGL((k_hist_point<k, o, 64, true, m>), dim3(w.grids.grid_small), dim3(64), w.lds_small, st_small,
                                   p->d_pieces.p, p->d_opieces.p, fv0, fv1, e->d_files.p, p->d_work_small.p,
                                   p->d_wcounters.p, p->d_tile_items.p, c.mp, w.small_g, p->max_slots, s.tab_lo, s.tab_n, s.fast_lo, s.fast_hi,
                                   (uint32_t *)p->d_hist.p, p->npos, out, e->norm_sum, (uint32_t)w.cap_small, w.grids.grid_small,
                                   p->d_chain_small.p, nfiles, Tile{}, OutPiece{}, (uint32_t *)nullptr, 0u);
        });
    });
    if (w.cap_small) {
        HIP_TRY(hipEventRecord(e->ev_join, st_small));
        HIP_TRY(hipStreamWaitEvent(st, e->ev_join, 0));
    }
    return PC_OK;
}

// tiles that were split into several work items: lay out from the merged histogram
// (k_gather_split clears what the split tiles merged: a histogram that was all zero stays so)
void merge_windows(pc_engine *e, pc_plan *p, const CountCall &c, const WorkLists &w) {
    // (skipped once the plan's lists are known to hold no merged window: the lists are the plan's own and do not
    // change from count to count, so neither does that -- and the exact grids it would check were read from them)
    if (w.grids.exact && p->work_counts.host[4] == 0 && !e->knobs.test_stale_counts) return;
    const int split_per_wg = kWG; // merged windows are the exception (pile-ups), with several files too (joint windows)
    dispatch_int<0, 1, 2>(c.outmode, [&](auto O) {
        constexpr int o = decltype(O)::value;
        hipLaunchKernelGGL((k_gather_split<o>), dim3((unsigned)((c.ntiles + split_per_wg - 1) / split_per_wg)), dim3(kWG), 0, e->stream,
                           p->d_tiles.p, c.ntiles, split_per_wg, p->d_pieces.p,
                           p->d_opieces.p, p->d_tile_items.p, p->d_wcounters.p, p->rows, (uint32_t *)p->d_hist.p, p->npos,
                           (typename OutT_<o>::type *)p->d_out.p, e->norm_sum, w.grids.launched[0], w.grids.launched[1], w.grids.launched[2], (uint32_t)w.cap, e->d_counters.p + 12);
    });
}

// how many items each class queued (k_gather_split keeps a copy): sizes the next launch of a large plan
int read_work_counts(pc_engine *e, pc_plan *p, const CountCall &c, const WorkLists &w) {
    hipStream_t st = e->stream;
    if (c.ntiles >= 4096) {
        QueuedCounts &q = p->work_counts;
        PC_TRY(q.ensure(8));
        if (q.generation != e->work_generation) {   // one read-back per (plan, generation)
            PC_TRY(q.request(st, p->d_wcounters.p));
            q.generation = e->work_generation;
        }
    }
    if (e->knobs.debug_work) { // diagnostics: how many work items of each class this call queued
        uint32_t c4[4] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpyAsync(c4, p->d_wcounters.p, sizeof(c4), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        fprintf(stderr, "[work] tiles %d: heavy %u light %u small %u, long-span candidates %u (capacity %lld, G %d, R %lld)\n", c.ntiles,
                c4[0], c4[1], c4[2], c4[3], (long long)w.cap, p->G, (long long)w.key.R);
    }
    return PC_OK;
}

int count_lists(pc_engine *e, pc_plan *p, const CountCall &c) {
    WorkLists w;
    PC_TRY(size_work_lists(e, p, c, w));
    StagedFile *canon = nullptr;
    PC_TRY(canonical_for_plan(e, p, c, w.shape, &canon));
    w.key.canon = canon ? canon->kid : 0;
    if (!(p->work_valid && p->work_key == w.key) || e->knobs.debug_work) PC_TRY(build_work_lists(e, p, c, w, canon));
    PC_TRY(mark(e, 2));
    if (w.lds > e->max_lds)
        return fail(PC_ERR_ARG, "pc_count: the window needs %zu bytes of LDS, the device offers %zu per workgroup (too many rows)", w.lds, e->max_lds);
    choose_grids(e, p, c, w);
    PC_TRY(launch_hist(e, p, c, w, canon));
    PC_TRY(mark(e, 3));
    PC_TRY(mark(e, 4));
    merge_windows(e, p, c, w);
    return read_work_counts(e, p, c, w);
}

// ---- the dense vector of the plan's file under the engine's rule and filters (dense_host.h, dense_kernels.hip.h).
// Under a point rule the count at a position is the same whatever the query, so a file whose genome is small beside its
// reads keeps one 16-bit cell per (contig, strand, position) and a count of a '+' / '-' plan is a copy with widening:
// no work lists, no windows, no LDS, no merge pass.
DenseSig dense_sig(const pc_engine *e, const StagedFile *sf) {
    DenseSig sig;
    sig.rule = rule_sig(e, sf);
    sig.applied = sf->applied;
    return sig;
}

std::atomic<uint64_t> g_dense_id{0};

// The build adds no second implementation of the rules and filters: an internal plan of one segment per contig and
// strand over the whole extent is counted by the window kernels (the dense vector forbidden for that plan) into the
// int64 block of that plan -- 8 bytes per cell from the engine's pool, at most pcdense::kBuildBlockCap, returned behind
// the build -- and one kernel narrows it.  Waits for the engine's stream.
int build_dense_vector(pc_engine *e, StagedFile *sf, const DenseSig &sig) {
    using namespace pcdense;
    sf->dsig_valid = false;
    const int ntid = e->ntid;
    const int64_t cells = sf->dcells;
    std::vector<int32_t> tid;
    std::vector<int64_t> start, end, off, stride;
    std::vector<uint8_t> strand;
    std::vector<int8_t> step;
    for (int t = 0; t < ntid; ++t)
        for (int s = 0; s < 2 && sf->dext[(size_t)t] > 0; ++s) {
            tid.push_back(t); start.push_back(0); end.push_back(sf->dext[(size_t)t]); strand.push_back(s ? PC_STRAND_REV : PC_STRAND_FWD);
            off.push_back(sf->dcell_off[(size_t)(2 * t + s)]); step.push_back(1); stride.push_back(0);
        }
    pc_plan *ip = nullptr;
    PC_TRY(pc_plan_create(e, (int64_t)tid.size(), tid.data(), start.data(), end.data(), strand.data(), off.data(), step.data(), stride.data(), cells, 1, &ip));
    ip->no_dense = true;
    // (raw counts, whatever the engine's output mode; the events of the count that asked for the vector stay its own)
    const int norm_on = e->norm_on, prof_level = e->prof_level;
    e->norm_on = 0; e->prof_level = 0;
    int rc = pc_count(e, ip, PC_OUT_INT64);
    e->norm_on = norm_on; e->prof_level = prof_level;
    auto narrow = [&]() -> int {
        PoolScope pool_scope(&e->pool);
        hipStream_t st = e->stream;
        DevBuf<uint32_t> d_n, d_key, d_val;
        DevBuf<uint8_t> d_tmp;
        PC_TRY(sf->dense.reserve((size_t)cells + 8));
        PC_TRY(sf->d_dext.upload(sf->dext, st));
        PC_TRY(sf->d_dcell_off.upload(sf->dcell_off, st));
        PC_TRY(d_n.reserve(2));
        HIP_TRY(hipMemsetAsync(d_n.p, 0, 8, st));
        const unsigned grid = (unsigned)((cells + 255) / 256);
        const int64_t *src = (const int64_t *)ip->d_out.p;
        hipLaunchKernelGGL(k_dense_narrow, dim3(grid), dim3(256), 0, st, src, cells, sf->dense.p, d_n.p);
        uint32_t n_ovf = 0;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&n_ovf, d_n.p, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (n_ovf) {   // the escaped cells, sorted by cell index
            auto sort_cells = [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, d_key.p, sf->dovf_key.p, d_val.p, sf->dovf_val.p, (int)n_ovf, 0, 32, st); };
            size_t most = 16, tb = 0;
            PC_TRY(cub_need(most, tb, sort_cells));
            PC_TRY(d_key.reserve(n_ovf)); PC_TRY(d_val.reserve(n_ovf)); PC_TRY(d_tmp.reserve(most));
            PC_TRY(sf->dovf_key.reserve(n_ovf)); PC_TRY(sf->dovf_val.reserve(n_ovf));
            hipLaunchKernelGGL(k_dense_overflow, dim3(grid), dim3(256), 0, st, src, cells, d_n.p + 1, n_ovf, d_key.p, d_val.p);
            PC_TRY(cub_run_sized(d_tmp, tb, sort_cells));
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(st));   // (the working arrays go out of scope)
        }
        sf->dn_ovf = n_ovf;
        return PC_OK;
    };
    if (rc == PC_OK) rc = narrow();
    (void)pc_plan_destroy(ip);   // (waits for the stream: the int64 block goes back to the pool)
    PC_TRY(rc);
    sf->dsig = sig;
    sf->dsig_valid = true;
    sf->did = ++g_dense_id;
    return PC_OK;
}

// `dense`: the plan's file when this count is to be served from its vector (built or rebuilt here when its signature
// no longer holds), else nullptr.  The plan conditions are those of the canonical stream, and no summed slice; the
// vector must not take more bytes than the stream it replaces -- canonical (weighed, and built, exactly as count_lists
// would), else compact, else the records -- and its build block must fit (dense_host.h).  A one-window plan keeps its
// single launch.
int dense_for_plan(pc_engine *e, pc_plan *p, const CountCall &c, StagedFile **dense) {
    *dense = nullptr;
    pcdense::PlanIn in;
    in.nfiles = c.nfiles;
    in.kind = e->kind;
    in.rows = p->rows; in.modes = p->modes; in.has_sums = p->has_sums;
    in.forbidden = e->knobs.no_dense || p->no_dense;
    if (!pcdense::plan_conditions(in)) return PC_OK;
    StagedFile *sf = e->files[0];
    if (sf->n <= 0 || !sf->nlin || sf->tid_end.size() != (size_t)e->ntid) return PC_OK;
    if (sf->dcells < 0) {   // the layout: once per file
        sf->dext.resize((size_t)e->ntid);
        sf->dcell_off.resize(2 * (size_t)e->ntid + 1);
        for (int t = 0; t < e->ntid; ++t) sf->dext[(size_t)t] = pcdense::extent(0, sf->tid_end[(size_t)t]);   // (the engine is told no declared lengths)
        sf->dcells = pcdense::layout(e->ntid, sf->dext.data(), sf->dcell_off.data());
    }
    in.cells = sf->dcells;
    if (!pcdense::build_fits(in.cells) || in.cells >= (int64_t)0xffffffffu) return PC_OK;
    StagedFile *canon = nullptr;
    PC_TRY(canonical_for_plan(e, p, c, hist_lds_shape(e), &canon));
    in.stream_entries = canon ? canon->kn : (sf->cn >= 0 ? sf->cn : sf->n);
    const bool ok = pcdense::eligible(in);
    if (e->knobs.dense_debug)
        fprintf(stderr, "[dense] cells %lld (%lld bytes) against %lld entries of the %s stream (%lld bytes): %s\n", (long long)in.cells,
                (long long)(in.cells * pcdense::kBytesPerCell), (long long)in.stream_entries, canon ? "canonical" : (sf->cn >= 0 ? "compact" : "record"),
                (long long)(in.stream_entries * 4), ok ? "vector" : "window kernels");
    if (!ok) return PC_OK;
    const DenseSig sig = dense_sig(e, sf);
    if (!(sf->dsig_valid && sf->dsig == sig)) PC_TRY(build_dense_vector(e, sf, sig));
    *dense = sf;
    return PC_OK;
}

// the chunk table of the plan (dense_host.h): the segments sorted by their first output element, their spans counted,
// placed and written, one descriptor per chunk.  p->chunks_ok says whether the plan can be served by chunks
int build_dense_chunks(pc_engine *e, pc_plan *p, const StagedFile *sf, const GatherSeg *gsegs, const int32_t *tid, const uint8_t *strand) {
    using namespace pcdense;
    p->chunks_ok = false;
    const size_t n = (size_t)p->nseg, nchunks = (size_t)chunks_of(p->out_elems);
    if (!n || !nchunks || !spans_fit((int64_t)n, p->covered) || nchunks >= (size_t)0x7fffffffu) return PC_OK;
    hipStream_t st = e->stream;
    DevBuf<uint64_t> d_key, d_key2;
    DevBuf<uint32_t> d_idx, d_idx2, d_cnt, d_at, d_first, d_nof, d_flag;
    DevBuf<uint8_t> d_tmp;
    d_key.pool = d_key2.pool = d_idx.pool = d_idx2.pool = d_cnt.pool = d_at.pool = d_first.pool = d_nof.pool = d_flag.pool = d_tmp.pool = &e->pool;
    size_t most = 16, sort_b = 0, scan_b = 0;
    const uint64_t nokey = (uint64_t)p->out_elems;               // the key of an empty segment: behind every start
    const int key_bits = bits_for(nokey);
    auto sort_starts = [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, d_key.p, d_key2.p, d_idx.p, d_idx2.p, (int)n, 0, key_bits, st); };
    auto sum_spans = [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, d_cnt.p, d_at.p, (int)n + 1, st); };
    PC_TRY(cub_need(most, sort_b, sort_starts));
    PC_TRY(cub_need(most, scan_b, sum_spans));
    PC_TRY(d_key.reserve(n)); PC_TRY(d_key2.reserve(n)); PC_TRY(d_idx.reserve(n)); PC_TRY(d_idx2.reserve(n));
    PC_TRY(d_cnt.reserve(n + 1)); PC_TRY(d_at.reserve(n + 1)); PC_TRY(d_first.reserve(nchunks)); PC_TRY(d_nof.reserve(nchunks)); PC_TRY(d_flag.reserve(2));
    PC_TRY(d_tmp.reserve(most));
    const unsigned g = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_chunk_keys, dim3(g), dim3(256), 0, st, gsegs, (int64_t)n, nokey, d_key.p, d_idx.p);
    PC_TRY(cub_run_sized(d_tmp, sort_b, sort_starts));
    HIP_TRY(hipMemsetAsync(d_cnt.p + n, 0, 4, st));
    HIP_TRY(hipMemsetAsync(d_flag.p, 0, 8, st));
    hipLaunchKernelGGL(k_chunk_count, dim3(g), dim3(256), 0, st, gsegs, d_key2.p, d_idx2.p, (int64_t)n, nokey, d_cnt.p, d_flag.p);
    PC_TRY(cub_run_sized(d_tmp, scan_b, sum_spans));
    // No wait in between: the span array takes the bound that spans_fit checked (every segment: its whole chunks and two
    // ends), and k_chunk_descs leaves the descriptors alone where k_chunk_count found an overlap
    PC_TRY(p->d_dspans.reserve(2 * n + (size_t)(p->covered / kChunk) + 1));
    PC_TRY(p->d_dchunks.reserve(nchunks));
    HIP_TRY(hipMemsetAsync(d_nof.p, 0, nchunks * 4, st));
    HIP_TRY(hipMemsetAsync(d_first.p, 0, nchunks * 4, st));   // (a chunk without spans names none)
    hipLaunchKernelGGL(k_chunk_spans, dim3(g), dim3(256), 0, st, gsegs, tid, strand, d_key2.p, d_idx2.p, (int64_t)n, nokey, e->ntid, sf->d_dcell_off.p, sf->d_dext.p, d_at.p,
                       p->d_dspans.p, d_first.p, d_nof.p);
    hipLaunchKernelGGL(k_chunk_descs, dim3((unsigned)((nchunks + 255) / 256)), dim3(256), 0, st, p->d_dspans.p, d_first.p, d_nof.p, d_flag.p, (int64_t)nchunks, p->d_dchunks.p);
    HIP_TRY(hipGetLastError());
    uint32_t overlap = 0;
    HIP_TRY(hipMemcpyAsync(&overlap, d_flag.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // (the working arrays go out of scope)
    if (overlap) return PC_OK;           // overlapping output ranges: the items serve the plan
    p->chunks_ok = true;
    return PC_OK;
}

// the plan's segments cut into gather items, and its chunk table: each once per plan and vector.  The chunk table waits
// for the first count that may take the chunk path: under PC_DENSE_ITEMS a plan never pays for it
int ensure_dense_tables(pc_engine *e, pc_plan *p, const StagedFile *sf) {
    using namespace pcdense;
    const bool need_items = p->ditems_id != sf->did, need_chunks = !e->knobs.dense_items && p->dchunks_id != sf->did;
    if (!need_items && !need_chunks) return PC_OK;
    hipStream_t st = e->stream;
    const size_t n = (size_t)p->nseg;
    if (need_items) { p->ditems_id = 0; p->n_ditems = 0; }
    if (need_chunks) { p->dchunks_id = 0; p->chunks_ok = false; }
    DevBuf<int32_t> d_tid;
    DevBuf<uint8_t> d_strand, d_tmp;
    DevBuf<uint32_t> d_cnt, d_at;
    d_tid.pool = d_strand.pool = d_tmp.pool = d_cnt.pool = d_at.pool = &e->pool;
    const GatherSeg *gsegs = p->gpu_built ? p->d_gsegs_own.p : p->d_gsegs.p;
    const int32_t *tid = nullptr;
    const uint8_t *strand = nullptr;
    if (p->gpu_built) {   // the caller's arrays are in HBM
        const PlanInputLayout L(n);
        tid = (const int32_t *)(p->d_inputs.p + L.at_tid); strand = p->d_inputs.p + L.at_strand;
    } else {
        PC_TRY(d_tid.upload(p->h_tid, st)); PC_TRY(d_strand.upload(p->h_strand, st));
        tid = d_tid.p; strand = d_strand.p;
    }
    if (need_items) {
        uint32_t total = 0;
        if (n) {
            auto sum_items = [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, d_cnt.p, d_at.p, (int)n + 1, st); };
            size_t most = 16, tb = 0;
            PC_TRY(cub_need(most, tb, sum_items));
            PC_TRY(d_cnt.reserve(n + 1)); PC_TRY(d_at.reserve(n + 1)); PC_TRY(d_tmp.reserve(most));
            const unsigned g = (unsigned)((n + 255) / 256);
            HIP_TRY(hipMemsetAsync(d_cnt.p + n, 0, 4, st));
            hipLaunchKernelGGL(k_dense_seg_items, dim3(g), dim3(256), 0, st, gsegs, (int64_t)n, d_cnt.p);
            PC_TRY(cub_run_sized(d_tmp, tb, sum_items));
            HIP_TRY(hipMemcpyAsync(&total, d_at.p + n, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            PC_TRY(p->d_ditems.reserve(std::max<size_t>(total, 1)));
            if (total) hipLaunchKernelGGL(k_dense_items, dim3(g), dim3(256), 0, st, gsegs, tid, strand, (int64_t)n, e->ntid, sf->d_dcell_off.p, sf->d_dext.p, d_at.p, p->d_ditems.p);
            HIP_TRY(hipGetLastError());
        }
        p->n_ditems = total;
    }
    // (a chunk table that cannot be built -- no memory for it -- is no failure of the count: the items serve the plan)
    if (need_chunks && n && build_dense_chunks(e, p, sf, gsegs, tid, strand) != PC_OK) { p->chunks_ok = false; (void)hipGetLastError(); }
    HIP_TRY(hipStreamSynchronize(st));   // (the working arrays go out of scope; behind the chunk table's own wait the stream is idle)
    if (need_items) p->ditems_id = sf->did;
    if (need_chunks) p->dchunks_id = sf->did;
    return PC_OK;
}

// a count served from the dense vector: one launch, between the marks of the histogram kernels
int count_dense(pc_engine *e, pc_plan *p, const CountCall &c, const StagedFile *sf, int path) {
    PC_TRY(mark(e, 2));
    if (path == PC_DENSE_PATH_CHUNKS)
        dispatch_int<0, 1, 2>(c.outmode, [&](auto O) {
            constexpr int o = decltype(O)::value;
            hipLaunchKernelGGL((pcdense::k_dense_gather_chunks<o>), dim3((unsigned)pcdense::chunks_of(p->out_elems)), dim3(pcdense::kGatherWG), 0, e->stream,
                               p->d_dchunks.p, p->d_dspans.p, sf->dense.p, sf->dovf_key.p, sf->dovf_val.p, sf->dn_ovf, (typename OutT_<o>::type *)p->d_out.p,
                               (int64_t)p->out_elems, e->norm_sum);
        });
    else if (p->n_ditems)
        dispatch_int<0, 1, 2>(c.outmode, [&](auto O) {
            constexpr int o = decltype(O)::value;
            hipLaunchKernelGGL((pcdense::k_dense_gather<o>), dim3((unsigned)pcdense::batches_of(p->n_ditems)), dim3(pcdense::kGatherWG), 0, e->stream, p->d_ditems.p,
                               (uint32_t)p->n_ditems, sf->dense.p, sf->dovf_key.p, sf->dovf_val.p, sf->dn_ovf, (typename OutT_<o>::type *)p->d_out.p, e->norm_sum);
        });
    PC_TRY(mark(e, 3));
    return mark(e, 4);
}

// ---- the center rule: k_center2 writes every queried position of the tiles straight into the output layout; the
// compact histogram is not touched
int reserve_center(pc_engine *e, pc_plan *p) {
    const size_t nchunks = p->n_cchunks, nfiles = e->files.size();
    if (kCenterCap * (int64_t)nchunks >= (int64_t)1 << kSubShift) return fail(PC_ERR_ARG, "pc_count: too many positions for the center rule");
    PC_TRY(p->d_corder.reserve((size_t)kCenterCap * nchunks));   // dispatch list: heavy entries front, light back
    PC_TRY(p->d_ccand.reserve(nchunks));
    PC_TRY(p->d_cranges.reserve(nchunks * nfiles));
    PC_TRY(p->d_crec.reserve(nchunks * nfiles));
    PC_TRY(p->d_crows.reserve(nchunks * nfiles * (size_t)(2 * kCenterRows)));
    PC_TRY(p->d_ccounts.reserve(8));
    PC_TRY(e->d_cvalh.reserve(256));
    // one descriptor per dispatch entry and file; k_center2 takes several entries per wave
    return p->d_cslots.reserve(2 * nchunks * nfiles);   // (heavy entries < chunks, light entries <= chunks)
}

// the dispatch list of the plan's chunks and its descriptors: kept while the work generation, the halo and the file count stand
int build_center_dispatch(pc_engine *e, pc_plan *p, int W) {
    hipStream_t st = e->stream;
    const int nfiles = (int)e->files.size();
    const int64_t nchunks = (int64_t)p->n_cchunks;
    p->center_nfiles = nfiles;
    HIP_TRY(hipMemsetAsync(p->d_ccounts.p, 0, 8 * sizeof(uint32_t), st));
    unsigned long long *total = (unsigned long long *)(p->d_ccounts.p + 2);
    const unsigned wgs = (unsigned)((nchunks + kRangesWG - 1) / kRangesWG);
    hipLaunchKernelGGL(k_center_weigh, dim3(wgs), dim3(kRangesWG), 0, st, p->d_cchunks.p, nchunks, e->d_files.p, nfiles, W,
                       p->d_ccand.p, p->d_cranges.p, p->d_crec.p, p->d_crows.p, total);
    // cut thresholds, in multiples of the mean candidate count
    const int ck1 = e->knobs.center_t1, ck2 = e->knobs.center_t2;
    hipLaunchKernelGGL(k_center_order, dim3(wgs), dim3(kRangesWG), 0, st, p->d_ccand.p, nchunks, total, e->knobs.center_floor,
                       (int64_t)2048, ck1, ck2, p->d_corder.p, p->d_ccounts.p);
    hipLaunchKernelGGL(k_center_slots, dim3((unsigned)((2 * nchunks + kRangesWG - 1) / kRangesWG)), dim3(kRangesWG), 0, st, p->d_cchunks.p, nchunks,
                       e->d_files.p, nfiles, W, p->d_corder.p, p->d_ccounts.p, p->d_cranges.p, p->d_crec.p, p->d_crows.p, p->d_opieces.p,
                       p->d_cslots.p, (unsigned long long *)(p->d_ccounts.p + 4));
    p->center_generation = e->work_generation;
    p->center_W = W;
    // how many entries the list got: sizes the grid of the later counts of this plan (read back once)
    PC_TRY(p->center_counts.ensure(2));
    return p->center_counts.request(st, p->d_ccounts.p);
}

// descriptors: heavy entries one wave each, PC_CENTER_PER_WAVE light entries per wave (an eighth of the list per XCD)
void launch_center2(pc_engine *e, pc_plan *p, const CountCall &c, int W, unsigned long long *dbg, size_t dbg_slots) {
    Center2Ctx c2;
    StagedFile *sf0 = e->files[0];
    c2.slots = p->d_cslots.p;
    c2.indirect = 0u;
    for (int k = 0; k < 3; ++k) {
        c2.ent[k] = sf0->cs_n[k] >= 0 ? sf0->cs_ent[k].p : nullptr;
        if (sf0->len_max > 255) c2.indirect |= 1u << k;
    }
    c2.files = e->d_files.p; c2.nfiles = c.nfiles; c2.file0 = sf0->view(); c2.mp = c.mp; c2.W = W; c2.inv = e->d_inv.p; c2.invh = e->d_invh.p; c2.cvalh = e->d_cvalh.p;
    c2.counters = p->d_ccounts.p;
    const QueuedCounts &q = p->center_counts;   // (heavy, light; the kernel reads its own counters while they are not known)
    const uint32_t n_heavy = q.known ? q.host[0] : 0u, n_light = q.known ? q.host[1] : 0u;
    c2.known = q.known ? 1u : 0u; c2.n_heavy = n_heavy; c2.n_light = n_light;
    c2.opieces = p->d_opieces.p; c2.out = (double *)p->d_out.p; c2.norm_sum = e->norm_sum; c2.norm_on = e->norm_on ? 1 : 0;
    c2.dbg = dbg; c2.dbg_cap = (uint32_t)dbg_slots;
    const dim3 cg2((unsigned)pccount::center_grid(q.known, n_heavy, n_light, (uint64_t)p->n_cchunks, PC_CENTER_PER_WAVE));
    // (files with reads beyond a stream entry's 8-bit fields, or a stream too long for 32-bit byte offsets, take the
    // instantiation that tests every batch for them)
    bool general = false;
    for (auto *f : e->files) general |= pccount::center_general(f->len_max, f->n + f->nrun);
    // (several files: one descriptor per entry and file, replayed into the same sums in file order)
    dispatch_int<0, 1>(dbg != nullptr, [&](auto D) {
        dispatch_int<0, 1>(general, [&](auto G) {
            dispatch_int<0, 1>(c.nfiles > 1, [&](auto M) {
                hipLaunchKernelGGL((k_center2<decltype(D)::value != 0, decltype(G)::value != 0, decltype(M)::value != 0>), cg2, dim3(64), (size_t)e->knobs.center_lds, e->stream, c2);
            });
        });
    });
}

// diagnostic launch: replay steps and dispatched waves, summed on the host; PC_CENTER_DEBUG prints them
int report_center_debug(pc_engine *e, pc_plan *p, int W, const unsigned long long *d_dbg, size_t dbg_slots) {
    std::vector<unsigned long long> h(2 * dbg_slots), h_slots(dbg_slots);
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(h.data(), d_dbg, h.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_slots.data(), d_dbg + h.size(), h_slots.size() * 8, hipMemcpyDeviceToHost));
    e->center_steps = 0; e->center_waves = 0;
    unsigned long long t0 = ~0ull, t1 = 0, sum = 0, steps_heavy = 0, steps_pers = 0, n_heavy_w = 0, n_pers_w = 0;
    const size_t n_front = p->n_cchunks;   // (heavy entries occupy the front of the list: fewer than the chunk count)
    std::vector<std::pair<unsigned long long, size_t>> byd;
    for (size_t i = 0; i < dbg_slots; ++i)
        if (h[2 * i]) {
            e->center_steps += (int64_t)h_slots[i]; e->center_waves += 1;
            const bool pers = i >= n_front;
            (pers ? steps_pers : steps_heavy) += h_slots[i];
            (pers ? n_pers_w : n_heavy_w) += 1;
            t0 = std::min(t0, h[2 * i + 1]); t1 = std::max(t1, h[2 * i + 1] + h[2 * i]);
            sum += h[2 * i];
            byd.emplace_back(h[2 * i], i);
        }
    if (e->knobs.center_debug != 0) {
        fprintf(stderr, "[center] replay steps: %llu in %llu waves of the heavy entries, %llu in %llu waves of the light ones\n", steps_heavy, n_heavy_w,
                steps_pers, n_pers_w);
        fprintf(stderr, "[center] W %d: launch span %llu ticks (100 MHz: %.3f ms), summed wave time %llu ticks = %.1f x the span\n", W, t1 - t0,
                (t1 - t0) / 1e5, sum, (double)sum / (double)std::max<unsigned long long>(t1 - t0, 1));
        const int nb = 20;
        std::vector<double> occ(nb, 0.0);
        const double span = (double)std::max<unsigned long long>(t1 - t0, 1);
        for (size_t i = 0; i < dbg_slots; ++i)
            if (h[2 * i]) {
                const double a = (double)(h[2 * i + 1] - t0) / span * nb, b = (double)(h[2 * i + 1] + h[2 * i] - t0) / span * nb;
                for (int k = std::max(0, (int)a); k < nb && k < b; ++k) occ[(size_t)k] += std::min(b, k + 1.0) - std::max(a, (double)k);
            }
        fprintf(stderr, "[center] resident waves per twentieth of the launch:");
        for (int k = 0; k < nb; ++k) fprintf(stderr, " %.0f", occ[(size_t)k]);
        fprintf(stderr, "\n");
        std::sort(byd.rbegin(), byd.rend());
        for (size_t k = 0; k < std::min<size_t>(byd.size(), 8); ++k) {
            const size_t i = byd[k].second;
            fprintf(stderr, "[center]   slot %zu (%s): %.3f ms, started at %.3f ms, %llu steps\n", i,
                    i >= n_front ? "light" : "heavy", byd[k].first / 1e5, (h[2 * i + 1] - t0) / 1e5, h_slots[i]);
        }
        if (!byd.empty()) {
            const size_t i = byd.back().second;
            fprintf(stderr, "[center]   shortest: slot %zu: %.3f ms, %llu steps\n", i, byd.back().first / 1e5, h_slots[i]);
        }
    }
    return PC_OK;
}

int count_center(pc_engine *e, pc_plan *p, const CountCall &c) {
    PC_TRY(mark(e, 2));
    if (p->n_cchunks > 0) {
        const int W = e->W();
        PC_TRY(reserve_center(e, p));
        hipLaunchKernelGGL(k_center_vals, dim3(1), dim3(256), 0, e->stream, c.mp, e->d_invh.p, e->d_cvalh.p);
        if (p->center_generation != e->work_generation || p->center_W != W || p->center_nfiles != c.nfiles) {
            PC_TRY(build_center_dispatch(e, p, W));
        } else (void)p->center_counts.poll();
        // PC_CENTER_DEBUG: how long every dispatched wave ran (wall clock ticks), printed after the launch
        DevBuf<unsigned long long> d_dbg;
        const bool dbg_on = e->knobs.center_debug != 0 || e->want_center_steps;
        const size_t dbg_slots = (size_t)kCenterCap * p->n_cchunks;   // heavy entries from the front, light ones from the back
        if (dbg_on) {
            PC_TRY(d_dbg.reserve(3 * dbg_slots));
            HIP_TRY(hipMemsetAsync(d_dbg.p, 0, 3 * dbg_slots * 8, e->stream));
        }
        launch_center2(e, p, c, W, d_dbg.p, dbg_slots);
        if (dbg_on) PC_TRY(report_center_debug(e, p, W, d_dbg.p, dbg_slots));
    }
    PC_TRY(mark(e, 3));
    return mark(e, 4);
}

int count_finish(pc_engine *e, pc_plan *p, const CountCall &c) {
    PC_TRY(mark(e, 5));
    HIP_TRY(hipGetLastError());
    p->last_dtype = c.out_dtype;
    p->counted = true;
    p->rle_runs = -1;
    e->timing_valid = e->prof_level > 0;
    e->timed_level = e->prof_level;
    // records once (8 B) + extra runs (8 B) + segments (24 B) + outputs once (8 B)
    e->last_alg_bytes = c.nrec * 8 + (c.nextra > 0 ? c.nextra * 8 : 0) + p->nseg * 24 + p->covered * 8;
    return PC_OK;
}

} // namespace

extern "C" {

int pc_count(pc_engine *e, pc_plan *p, int out_dtype) {
    PC_TRY(count_validate(e, p, out_dtype));
    HIP_TRY(hipSetDevice(e->device));
    const bool center = e->kind == PC_MAP_CENTER;
    CountCall c;
    c.out_dtype = out_dtype;
    c.outmode = e->norm_on ? 2 : (out_dtype == PC_OUT_FLOAT64 ? 1 : 0);
    c.nfiles = (int)e->files.size(); c.ntiles = (int)p->n_tiles;
    c.nrec = c.nextra = 0;
    for (auto *f : e->files) { c.nrec += f->n; c.nextra += f->nrun; }
    c.hist_bytes = center ? 0 : (size_t)p->npos * p->rows * sizeof(uint32_t);
    c.mp = e->params();
    const bool single = pccount::single_window(c.ntiles, c.nfiles, e->kind, e->knobs.debug_work, e->knobs.no_single);
    StagedFile *dense = nullptr;   // (decided first: a build counts a plan of its own on this engine)
    if (!center && !single && c.ntiles > 0) PC_TRY(dense_for_plan(e, p, c, &dense));
    e->last_count_dense = dense != nullptr;
    PC_TRY(count_prepare(e, p, dense != nullptr));
    int dense_path = PC_DENSE_PATH_NONE;
    PC_TRY(count_clear(e, p, c, dense, &dense_path));
    e->last_dense_path = dense_path;
    if (center) PC_TRY(count_center(e, p, c));
    else if (dense) PC_TRY(count_dense(e, p, c, dense, dense_path));
    else if (single) PC_TRY(count_single(e, p, c));
    else if (c.ntiles > 0) PC_TRY(count_lists(e, p, c));
    else for (int k = 2; k <= 4; ++k) PC_TRY(mark(e, k));   // a plan without windows
    return count_finish(e, p, c);
}

int64_t pc_dense_cells(pc_engine *e, int file) {
    if (!e || file < 0 || file >= (int)e->files.size()) return -1;
    const StagedFile *sf = e->files[file];
    if (e->files.size() != 1 || e->knobs.no_dense || !e->last_count_dense) return -1;   // (only a plan over ONE file is served from it)
    return (sf->dsig_valid && sf->dsig == dense_sig(e, sf)) ? sf->dcells : -1;
}

int pc_dense_path(pc_engine *e) { return e && pc_dense_cells(e, 0) >= 0 ? e->last_dense_path : PC_DENSE_PATH_NONE; }   // (NONE wherever pc_dense_cells says -1)

int pc_sync(pc_engine *e) {
    if (!e) return fail(PC_ERR_ARG, "engine is NULL");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return PC_OK;
}


// Exact grids (pc_count) rest on the work counts of a plan being a function of (plan, work generation).  The last
// kernel of a count compares what was queued with what was launched; a mismatch means work items went unserved.
static int check_grid_guard(pc_engine *e, pc_plan *p) {
    if (!p->exact_grid_used && !p->guard_pending) return PC_OK;
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, e->d_counters.p + 12, sizeof(err), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    p->guard_pending = false;
    if (!err) return PC_OK;
    HIP_TRY(hipMemsetAsync(e->d_counters.p + 12, 0, sizeof(uint32_t), e->stream));
    p->work_counts.known = false;
    p->work_counts.generation = 0;
    p->exact_grid_used = false;
    p->work_valid = false;
    if (err & 2u)
        return fail(PC_ERR_STATE, "the work lists of this plan overflowed their capacity (results incomplete): an engine defect -- please report "
                                  "the annotation / alignment shape; PC_WORK_R changes the item size");
    return fail(PC_ERR_STATE, "a count of this plan queued more work items than the cached work counts launched (results incomplete); "
                              "the cache has been dropped -- count again");
}

int pc_read_counts(pc_engine *e, pc_plan *p, void *host_out, int64_t out_elems) {
    if (!e || !p || p->e != e || !p->counted) return fail(PC_ERR_STATE, "pc_read_counts: nothing counted yet");
    if (out_elems != p->out_elems || (out_elems > 0 && !host_out)) return fail(PC_ERR_ARG, "pc_read_counts: buffer size mismatch");
    HIP_TRY(hipSetDevice(e->device));
    PC_TRY(check_grid_guard(e, p));
    const size_t bytes = (size_t)out_elems * 8;
    const char *knob = getenv("PC_STAGE_SLICE");   // (test knob: the ring for every size, in pieces of so many 4 KiB pages)
    const pcmem::Route route = pcmem::read_route(bytes, knob != nullptr);
    if (route == pcmem::Route::ring) {
        // the counts of a whole annotation: through the ring of page-locked pieces (a pageable destination the runtime has
        // not seen before is filled at 25 GB/s; see TransferRing)
        HIP_TRY(hipStreamSynchronize(e->stream));
        const std::vector<TransferJob> job{{host_out, p->d_out.p, bytes}};
        const size_t piece = knob ? (size_t)std::max<int64_t>(1, std::min<int64_t>(atoll(knob), 4096)) * 4096 : TransferRing::kPiece;
        return TransferRing::of(e->device).run(e->device, job, piece, knob != nullptr, true);
    }
    // (growing the buffer frees the old one: not while a plan upload may still be reading from it)
    if (bytes > e->pinned.cap && e->pinned_busy) { HIP_TRY(hipEventSynchronize(e->ev_pinned)); e->pinned_busy = false; }
    if (route == pcmem::Route::pinned && e->pinned.reserve(bytes) == PC_OK) {
        // short vectors come back through the page-locked buffer (stream order keeps it behind any
        // plan upload still reading from it): a pageable destination costs an extra staging hop
        HIP_TRY(hipMemcpyAsync(e->pinned.p, p->d_out.p, bytes, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        e->pinned_busy = false;
        memcpy(host_out, e->pinned.p, bytes);
        return PC_OK;
    }
    if (bytes > 0) HIP_TRY(hipMemcpyAsync(host_out, p->d_out.p, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return PC_OK;
}

int pc_plan_coordinates(pc_engine *e, pc_plan *p, int64_t *host_out, int64_t out_elems) {
    if (!e || !p || p->e != e) return fail(PC_ERR_ARG, "pc_plan_coordinates: bad engine/plan");
    if (out_elems != p->out_elems || (out_elems > 0 && !host_out)) return fail(PC_ERR_ARG, "pc_plan_coordinates: buffer size mismatch");
    HIP_TRY(hipSetDevice(e->device));
    if (out_elems == 0) return PC_OK;
    DevBuf<int64_t> d;
    d.pool = &e->pool;
    int rc = d.reserve((size_t)out_elems);
    if (rc == PC_OK) rc = ensure_gather_tables(e, p);   // the per-segment gather list of a large plan
    if (rc != PC_OK) return rc;
    hipStream_t st = e->stream;
    HIP_TRY(hipMemsetAsync(d.p, 0xff, (size_t)out_elems * 8, st));   // -1: elements no segment covers
    const unsigned grid = (unsigned)p->n_gchunks;
    if (grid) hipLaunchKernelGGL(k_coordinates, dim3(grid), dim3(kWG), 0, st, p->d_gsegs.p, p->d_gchunks.p, p->rows, d.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_out, d.p, (size_t)out_elems * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PC_OK;
}

void *pc_counts_device_ptr(pc_plan *p) { return p ? (void *)p->d_out.p : nullptr; }
void *pc_stream(pc_engine *e) { return e ? (void *)e->stream : nullptr; }
void *pc_total_device_ptr(pc_plan *p) { return p ? (void *)p->d_total.p : nullptr; }

int pc_total(pc_engine *e, pc_plan *p, void *host_out8) {
    if (!e || !p || p->e != e || !p->counted) return fail(PC_ERR_STATE, "pc_total: nothing counted yet");
    HIP_TRY(hipSetDevice(e->device));
    PC_TRY(check_grid_guard(e, p));
    hipStream_t st = e->stream;
    HIP_TRY(hipMemsetAsync(p->d_total.p, 0, 8, st));
    if (p->out_elems > 0) {
        if (p->last_dtype == PC_OUT_INT64) {
            hipLaunchKernelGGL(k_total_i64, dim3(1024), dim3(kWG), 0, st, (const int64_t *)p->d_out.p, p->out_elems, (int64_t *)p->d_total.p);
        } else {
            const int nb = 1024;
            PC_TRY(e->d_partial.reserve(nb));
            hipLaunchKernelGGL(k_total_f64_partial, dim3(nb), dim3(kWG), 0, st, (const double *)p->d_out.p, p->out_elems, e->d_partial.p);
            hipLaunchKernelGGL(k_total_f64_final, dim3(1), dim3(64), 0, st, e->d_partial.p, nb, (double *)p->d_total.p);
        }
    }
    if (host_out8) HIP_TRY(hipMemcpyAsync(host_out8, p->d_total.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PC_OK;
}

// ------------------------------------------------------------------ export: run-length encoding
int pc_rle(pc_engine *e, pc_plan *p, int64_t period, int64_t *n_runs) {
    if (!e || !p || p->e != e || !n_runs) return fail(PC_ERR_ARG, "pc_rle: bad arguments");
    if (!p->counted) return fail(PC_ERR_STATE, "pc_rle: nothing counted yet");
    if (period < 0) return fail(PC_ERR_ARG, "pc_rle: period must be >= 0");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const int64_t n = p->out_elems;
    p->rle_runs = 0;
    *n_runs = 0;
    if (n == 0) return PC_OK;
    const int64_t nwg = (n + kRleChunk - 1) / kRleChunk;
    int rc = p->d_rle_cnt.reserve((size_t)nwg);
    room(rc, p->d_rle_base, (size_t)nwg + 1);
    if (rc != PC_OK) return rc;
    const unsigned long long *v = (const unsigned long long *)p->d_out.p;
    hipLaunchKernelGGL(k_rle_count, dim3((unsigned)nwg), dim3(kWG), 0, st, v, n, period, p->d_rle_cnt.p);
    hipLaunchKernelGGL(k_rle_scan, dim3(1), dim3(kWG), 0, st, p->d_rle_cnt.p, nwg, p->d_rle_base.p, p->d_rle_base.p + nwg);
    int64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, p->d_rle_base.p + nwg, sizeof(total), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    rc = p->d_rle_starts.reserve((size_t)std::max<int64_t>(total, 1));
    room(rc, p->d_rle_values, (size_t)std::max<int64_t>(total, 1));
    if (rc != PC_OK) return rc;
    hipLaunchKernelGGL(k_rle_write, dim3((unsigned)nwg), dim3(kWG), 0, st, v, n, period, p->d_rle_base.p, p->d_rle_starts.p,
                       p->d_rle_values.p);
    HIP_TRY(hipGetLastError());
    p->rle_runs = total;
    *n_runs = total;
    return PC_OK;
}

int pc_read_rle(pc_engine *e, pc_plan *p, int64_t *starts, void *values, int64_t n_runs) {
    if (!e || !p || p->e != e) return fail(PC_ERR_ARG, "pc_read_rle: bad arguments");
    if (p->rle_runs < 0) return fail(PC_ERR_STATE, "pc_read_rle: pc_rle has not run");
    if (n_runs != p->rle_runs || (n_runs > 0 && (!starts || !values))) return fail(PC_ERR_ARG, "pc_read_rle: expected %lld runs", (long long)p->rle_runs);
    HIP_TRY(hipSetDevice(e->device));
    if (n_runs > 0) {
        HIP_TRY(hipMemcpyAsync(starts, p->d_rle_starts.p, (size_t)n_runs * 8, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemcpyAsync(values, p->d_rle_values.p, (size_t)n_runs * 8, hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return PC_OK;
}

int pc_set_profiling(pc_engine *e, int level) {
    if (!e) return fail(PC_ERR_ARG, "engine is NULL");
    if (level < 0 || level > 2) return fail(PC_ERR_ARG, "pc_set_profiling: level must be 0, 1 or 2");
    e->prof_level = level;
    e->timing_valid = false;
    return PC_OK;
}

int pc_last_timing(pc_engine *e, double *ms, int n) {
    if (!e || !ms || n <= 0) return fail(PC_ERR_ARG, "pc_last_timing: bad arguments");
    if (!e->timing_valid) return fail(PC_ERR_STATE, "pc_last_timing: no timed pc_count yet (see pc_set_profiling)");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipEventSynchronize(e->ev[5]));
    float t;
    for (double &v : e->last_ms) v = 0.0;
    HIP_TRY(hipEventElapsedTime(&t, e->ev[0], e->ev[5])); e->last_ms[0] = t;
    HIP_TRY(hipEventElapsedTime(&t, e->ev[2], e->ev[3])); e->last_ms[2] = t;
    if (e->timed_level >= 2) {
        HIP_TRY(hipEventElapsedTime(&t, e->ev[1], e->ev[2])); e->last_ms[1] = t;
        HIP_TRY(hipEventElapsedTime(&t, e->ev[3], e->ev[4])); e->last_ms[3] = t;
        HIP_TRY(hipEventElapsedTime(&t, e->ev[4], e->ev[5])); e->last_ms[4] = t;
        HIP_TRY(hipEventElapsedTime(&t, e->ev[0], e->ev[1])); e->last_ms[5] = t;
    }
    const int k = std::min(n, 6);
    for (int i = 0; i < k; ++i) ms[i] = e->last_ms[i];
    return k;
}

int64_t pc_last_algorithmic_bytes(pc_engine *e) { return e ? e->last_alg_bytes : -1; }

int pc_center_replay_steps(pc_engine *e, pc_plan *p, int64_t *steps, int64_t *waves) {
    if (!e || !p || p->e != e || !steps || !waves) return fail(PC_ERR_ARG, "pc_center_replay_steps: bad arguments");
    if (e->kind != PC_MAP_CENTER) return fail(PC_ERR_STATE, "pc_center_replay_steps: the mapping rule is not the center rule");
    e->want_center_steps = true;
    const int rc = pc_count(e, p, PC_OUT_FLOAT64);
    e->want_center_steps = false;
    if (rc != PC_OK) return rc;
    *steps = e->center_steps;
    *waves = e->center_waves;
    return PC_OK;
}

// ---- one segment in one call
// `ga[segment]` / `ga.get(segment)` (genome_array.py:861-928; the reference's scripts ask region by region, bin/psite.py:181-192):
// no plan object, no table upload, no read-back copy.  The window and its output piece travel in the kernel's arguments
// (k_hist_point<..., SINGLE> looks its record ranges up itself); the kernel writes the counts into page-locked host memory
// and a flag word behind them, which this call polls.  What a query paid for before was API calls and DMA hops, not
// bytes: plan create + upload + launch + read-back + sync, 59 us through the mirror at the end of round 4.
constexpr int kQueryMax = 4096;   // positions of one argument-borne window: 16 KiB of 32-bit bins

int pc_query_segment(pc_engine *e, int32_t tid, int64_t start, int64_t end, uint8_t strand, int reverse_out, int out_dtype, void *host_out) {
    if (!e || !host_out) return fail(PC_ERR_ARG, "pc_query_segment: bad arguments");
    if (!e->have_map) return fail(PC_ERR_STATE, "pc_query_segment: no mapping rule set (pc_set_mapping)");
    if (e->files.size() != 1) return fail(PC_ERR_STATE, "pc_query_segment: needs exactly one staged alignment file (several: pc_plan_create)");
    if (!pccount::point_rule(e->kind))
        return fail(PC_ERR_STATE, "pc_query_segment: the center and the stratified rule go through pc_plan_create");
    if (out_dtype != PC_OUT_INT64 && out_dtype != PC_OUT_FLOAT64) return fail(PC_ERR_ARG, "pc_query_segment: bad out_dtype");
    if (e->norm_on && out_dtype != PC_OUT_FLOAT64) return fail(PC_ERR_ARG, "pc_query_segment: normalisation produces float64");
    const int64_t len = end - start;
    if (len <= 0 || len > kQueryMax || start < 0 || end > 0x7fffffffLL) return fail(PC_ERR_STATE, "pc_query_segment: the segment does not fit one window (1 .. %d positions)", kQueryMax);
    if (tid < 0 || tid >= e->ntid) return fail(PC_ERR_ARG, "pc_query_segment: reference id out of range");
    StagedFile *sf = e->files[0];
    PC_TRY(check_filter_columns(e, "pc_query_segment"));
    HIP_TRY(hipSetDevice(e->device));
    if (!e->q_host) {
        HIP_TRY(hipHostMalloc((void **)&e->q_host, (size_t)kQueryMax * 8 + 64, hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer(&e->q_dev, e->q_host, 0));
        std::memset(e->q_host, 0, (size_t)kQueryMax * 8 + 64);
    }
    hipStream_t st = e->stream;
    const MapParams mp = e->params();
    const HistLds ls = hist_lds_shape(e);
    const int G = kQueryMax;
    const size_t lds = pccount::hist_lds_bytes(ls, 1, G, false);
    if (lds > e->max_lds) return fail(PC_ERR_STATE, "pc_query_segment: the window needs %zu bytes of LDS", lds);
    const int mode = mode_of(strand);
    Tile tl{};
    tl.tid = tid; tl.win_start = (int32_t)start; tl.piece_begin = tl.piece_end = 0; tl.mode_mask = 1u << mode;
    tl.op_begin = 0; tl.op_end = 1; tl.span_lo = 0; tl.span_hi = (uint16_t)len;
    OutPiece op{};
    op.out_off = reverse_out ? len - 1 : 0; op.row_stride = len; op.hist_off = 0; op.start = (int32_t)start; op.len = (int32_t)len;
    op.mode = mode; op.step = reverse_out ? -1 : 1;
    const uint32_t seq = ++e->q_seq ? e->q_seq : ++e->q_seq;   // (never 0: the flag's resting value)
    volatile uint32_t *flag = (volatile uint32_t *)(e->q_host + (size_t)kQueryMax * 8);
    uint32_t *d_flag = (uint32_t *)((uint8_t *)e->q_dev + (size_t)kQueryMax * 8);
    const FileView fv0 = sf->view();
    const int outmode = e->norm_on ? 2 : (out_dtype == PC_OUT_FLOAT64 ? 1 : 0);
    dispatch_hist<false>(e->kind, outmode, [&](auto K, auto O) {
        constexpr int k = decltype(K)::value, o = decltype(O)::value;
        hipLaunchKernelGGL((k_hist_point<k, o, kHistWG, false, false, true>), dim3(1), dim3(kHistWG), lds, st, (const Piece *)nullptr, (const OutPiece *)nullptr,
                           fv0, fv0, (const FileView *)nullptr, (const WorkItem *)nullptr, (const uint32_t *)nullptr, (const uint32_t *)nullptr, mp, G, 1,
                           ls.tab_lo, ls.tab_n, ls.fast_lo, ls.fast_hi, (uint32_t *)nullptr, (int64_t)e->Ws(), (typename OutT_<o>::type *)e->q_dev,
                           e->norm_sum, (uint32_t)e->Wg(), (uint32_t)e->Wr(), (const FileRange *)nullptr, 1, tl, op, d_flag, seq);
    });
    HIP_TRY(hipGetLastError());
    // poll the flag the kernel writes behind its counts (a stream synchronisation costs more than the kernel runs);
    // fall back to the synchronisation if it does not show up soon
    const auto t0 = std::chrono::steady_clock::now();
    bool seen = false;
    for (uint64_t spin = 0;; ++spin) {
        if (*flag == seq) { seen = true; break; }
        if ((spin & 1023u) == 1023u && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2e-3) break;
    }
    if (!seen) {
        HIP_TRY(hipStreamSynchronize(st));
        if (*flag != seq) return fail(PC_ERR_STATE, "pc_query_segment: the kernel did not report completion");
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    std::memcpy(host_out, e->q_host, (size_t)len * 8);
    return PC_OK;
}

int pc_center_row_fill(pc_engine *e, pc_plan *p, int64_t *row_entries, int64_t *row_slots) {
    if (!e || !p || p->e != e || !row_entries || !row_slots) return fail(PC_ERR_ARG, "pc_center_row_fill: bad arguments");
    if (p->center_generation != e->work_generation || !p->d_ccounts.p)
        return fail(PC_ERR_STATE, "pc_center_row_fill: the plan has no center dispatch list of one alignment file (count it under the center rule first)");
    HIP_TRY(hipSetDevice(e->device));
    unsigned long long v[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(v, p->d_ccounts.p + 4, sizeof(v), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *row_entries = (int64_t)v[0];
    *row_slots = (int64_t)v[1];
    return PC_OK;
}

int pc_stream_probe(pc_engine *e, int64_t bytes, int iters, double *read_gbps, double *write_gbps) {
    if (!e || bytes < (1 << 20) || iters < 1) return fail(PC_ERR_ARG, "pc_stream_probe: bad arguments");
    HIP_TRY(hipSetDevice(e->device));
    DevBuf<uint8_t> buf;
    PC_TRY(buf.reserve((size_t)bytes));
    hipStream_t st = e->stream;
    const int64_t nvec = bytes / 16, n8 = bytes / 8;
    const unsigned grid_r = (unsigned)((nvec + kProbeChunk - 1) / kProbeChunk), grid_w = (unsigned)((n8 + 2 * kProbeChunk - 1) / (2 * kProbeChunk));
    uint32_t *sink = e->d_counters.p + 7;   // a word no kernel of the counting path reads
    float ms = 0.f;
    for (int pass = 0; pass < 2; ++pass) {   // pass 0: stores (also fills the buffer), pass 1: loads
        for (int it = -1; it < iters; ++it) {   // one untimed launch first
            if (it == 0) HIP_TRY(hipEventRecord(e->ev[6], st));
            if (pass == 0) hipLaunchKernelGGL(k_probe_write, dim3(grid_w), dim3(kWG), 0, st, (unsigned long long *)buf.p, n8);
            else hipLaunchKernelGGL(k_probe_read, dim3(grid_r), dim3(kWG), 0, st, (const u32x4 *)buf.p, nvec, sink);
        }
        HIP_TRY(hipEventRecord(e->ev[7], st));
        HIP_TRY(hipEventSynchronize(e->ev[7]));
        HIP_TRY(hipEventElapsedTime(&ms, e->ev[6], e->ev[7]));
        const double gbps = (double)bytes * iters / ((double)ms * 1e-3) / 1e9;
        if (pass == 0 && write_gbps) *write_gbps = gbps;
        if (pass == 1 && read_gbps) *read_gbps = gbps;
    }
    HIP_TRY(hipGetLastError());
    return PC_OK;
}

// ------------------------------------------------------------------ warnings
int pc_warn_flags(pc_engine *e, pc_plan *p, uint8_t *flags) { return pc_warn_details(e, p, flags, nullptr); }

int pc_warn_details(pc_engine *e, pc_plan *p, uint8_t *flags, int32_t *last_len) {
    if (!e || !p || p->e != e || (p->nseg > 0 && !flags)) return fail(PC_ERR_ARG, "pc_warn_flags: bad arguments");
    if (!e->have_map) return fail(PC_ERR_STATE, "pc_warn_flags: no mapping rule set");
    std::memset(flags, 0, (size_t)p->nseg);
    if (last_len) std::fill(last_len, last_len + p->nseg, (int32_t)-1);
    if (e->kind == PC_MAP_STRAT5) return PC_OK; // never warns
    // cheap pre-check on the per-length record histogram (ignores filters: conservative)
    bool any = false;
    for (auto *f : e->files) {
        for (int L = f->len_min; L <= f->len_max && !any; ++L) {   // lengths present in the file
            if (!f->len_hist[(size_t)L]) continue;
            bool bad;
            switch (e->kind) {
            case PC_MAP_FIVE: case PC_MAP_THREE: bad = e->param >= L; break;
            case PC_MAP_CENTER: bad = L - 2 * e->param < 0; break;
            default: bad = L >= e->table_len || e->h_fw[(size_t)L] < 0;
            }
            any |= bad;
        }
    }
    if (!any) return PC_OK;
    HIP_TRY(hipSetDevice(e->device));
    PC_TRY(refresh_file_views(e));
    const MapParams mp = e->params();
    std::vector<Unmappable> all;
    std::vector<uint32_t> file_of;   // staged file of every entry of `all` (parallel array, permuted with it)
    int file_index = -1;
    for (auto *f : e->files) {
        ++file_index;
        if (!f->n) continue;
        uint32_t cap = 1u << 16;
        for (;;) {
            PC_TRY(e->d_unmap.reserve(cap));
            HIP_TRY(hipMemsetAsync(e->d_counters.p + 1, 0, sizeof(uint32_t), e->stream));
            hipLaunchKernelGGL(k_unmappable, dim3((unsigned)((f->n + kWG - 1) / kWG)), dim3(kWG), 0, e->stream, f->view(), mp, e->ntid,
                               e->d_unmap.p, cap, e->d_counters.p + 1);
            uint32_t cnt = 0;
            HIP_TRY(hipMemcpyAsync(&cnt, e->d_counters.p + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            if (cnt <= cap) {
                const size_t base = all.size();
                all.resize(base + cnt);
                if (cnt) HIP_TRY(hipMemcpy(all.data() + base, e->d_unmap.p, (size_t)cnt * sizeof(Unmappable), hipMemcpyDeviceToHost));
                file_of.resize(base + cnt, (uint32_t)file_index);
                break;
            }
            cap = cnt;
        }
    }
    if (all.empty()) return PC_OK;
    // host: does any unmappable record of the right strand overlap the segment (htslib rule)?
    {   // sort by (tid, pos), carrying the file index along
        std::vector<size_t> perm(all.size());
        for (size_t i = 0; i < perm.size(); ++i) perm[i] = i;
        std::sort(perm.begin(), perm.end(), [&](size_t a, size_t b) {
            if (all[a].tid != all[b].tid) return all[a].tid < all[b].tid;
            return all[a].pos < all[b].pos;
        });
        std::vector<Unmappable> a2(all.size());
        std::vector<uint32_t> f2(all.size());
        for (size_t i = 0; i < perm.size(); ++i) { a2[i] = all[perm[i]]; f2[i] = file_of[perm[i]]; }
        all.swap(a2);
        file_of.swap(f2);
    }
    const size_t n = all.size();
    std::vector<int32_t> pmax_f(n), pmax_r(n);
    for (size_t i = 0; i < n; ++i) {
        const bool fresh = i == 0 || all[i].tid != all[i - 1].tid;
        int32_t pf = fresh ? INT32_MIN : pmax_f[i - 1], pr = fresh ? INT32_MIN : pmax_r[i - 1];
        if (all[i].rev) pr = std::max(pr, all[i].end); else pf = std::max(pf, all[i].end);
        pmax_f[i] = pf;
        pmax_r[i] = pr;
    }
    PC_TRY(fetch_host_inputs(p));
    for (int64_t s = 0; s < p->nseg; ++s) {
        const int32_t t = p->h_tid[(size_t)s];
        if (t < 0 || t >= e->ntid) continue;
        const int64_t st = p->h_start[(size_t)s], en = p->h_end[(size_t)s];
        // last record of tid t with pos < en
        size_t lo = 0, hi = n;
        while (lo < hi) {
            size_t mid = (lo + hi) / 2;
            if (all[mid].tid < t || (all[mid].tid == t && (int64_t)all[mid].pos < en)) lo = mid + 1; else hi = mid;
        }
        if (lo == 0 || all[lo - 1].tid != t) continue;
        const int mode = mode_of(p->h_strand[(size_t)s]);
        int64_t best;
        if (mode == 0) best = pmax_f[lo - 1];
        else if (mode == 1) best = pmax_r[lo - 1];
        else best = std::max(pmax_f[lo - 1], pmax_r[lo - 1]);
        if (best > st) flags[s] = 1;
        if (best > st && last_len) {
            // the LAST offending read in fetch order (file-major, then record order) among those fetch
            // returns for the segment: walk back while some earlier read of the strand can still reach it
            uint64_t best_key = 0;
            bool have = false;
            for (size_t i = lo; i-- > 0 && all[i].tid == t;) {
                const int64_t reach = mode == 0 ? pmax_f[i] : (mode == 1 ? pmax_r[i] : std::max(pmax_f[i], pmax_r[i]));
                if (reach <= st) break;
                const bool strand_ok = mode == 0 ? !all[i].rev : (mode == 1 ? all[i].rev != 0 : true);
                if (!strand_ok || (int64_t)all[i].end <= st) continue;
                const uint64_t key = ((uint64_t)file_of[i] << 32) | all[i].rec;
                if (!have || key > best_key) { best_key = key; last_len[s] = all[i].len; have = true; }
            }
        }
    }
    return PC_OK;
}

int pc_mapped_reads(pc_engine *e, int file, int64_t rec_lo, int64_t rec_hi, int32_t tid, int64_t start, int64_t end,
                    uint8_t strand, uint8_t *mask) {
    if (!e || file < 0 || file >= (int)e->files.size()) return fail(PC_ERR_ARG, "pc_mapped_reads: bad file index");
    if (!e->have_map) return fail(PC_ERR_STATE, "pc_mapped_reads: no mapping rule set");
    PC_TRY(check_filter_columns(e, "pc_mapped_reads"));
    StagedFile *f = e->files[file];
    if (rec_lo < 0 || rec_hi > f->n || rec_hi < rec_lo || (rec_hi > rec_lo && !mask)) return fail(PC_ERR_ARG, "pc_mapped_reads: bad record range");
    (void)tid;
    if (rec_hi == rec_lo) return PC_OK;
    HIP_TRY(hipSetDevice(e->device));
    const int64_t n = rec_hi - rec_lo;
    DevBuf<uint8_t> d_mask;
    PC_TRY(d_mask.reserve((size_t)n));
    hipLaunchKernelGGL(k_mapped_reads, dim3((unsigned)((n + kWG - 1) / kWG)), dim3(kWG), 0, e->stream, f->view(), e->params(), rec_lo, rec_hi,
                       start, end, mode_of(strand), !(strand & PC_STRAND_NOFILTER), d_mask.p);
    HIP_TRY(hipMemcpyAsync(mask, d_mask.p, (size_t)n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return PC_OK;
}

int pc_mapped_reads_batch(pc_engine *e, pc_plan *p, int64_t *offsets, int64_t *total) {
    if (!e || !p || p->e != e || !offsets || !total) return fail(PC_ERR_ARG, "pc_mapped_reads_batch: bad arguments");
    if (!e->have_map) return fail(PC_ERR_STATE, "pc_mapped_reads_batch: no mapping rule set");
    if (e->files.empty()) return fail(PC_ERR_STATE, "pc_mapped_reads_batch: no alignments staged");
    PC_TRY(check_filter_columns(e, "pc_mapped_reads_batch"));
    HIP_TRY(hipSetDevice(e->device));
    PC_TRY(refresh_file_views(e));
    const int nfiles = (int)e->files.size();
    const int64_t nseg = p->nseg, npair = nseg * nfiles;
    *total = 0;
    offsets[0] = 0;
    p->mr_total = 0;
    if (npair == 0) return PC_OK;
    if (npair >= (int64_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_mapped_reads_batch: too many (segment, file) pairs");
    PC_TRY(fetch_host_inputs(p));
    std::vector<BatchSeg> segs((size_t)nseg);
    for (int64_t s = 0; s < nseg; ++s) {
        BatchSeg &g = segs[(size_t)s];
        const int32_t t = p->h_tid[(size_t)s];
        g.tid = (t >= 0 && t < e->ntid) ? t : -1;
        g.start = std::max<int64_t>(p->h_start[(size_t)s], 0);
        g.end = std::min<int64_t>(p->h_end[(size_t)s], 0x7fffffffLL);
        g.mode = mode_of(p->h_strand[(size_t)s]) | ((p->h_strand[(size_t)s] & PC_STRAND_NOFILTER) ? 0x100 : 0);
    }
    std::vector<int64_t> spans;
    for (auto *f : e->files) spans.push_back(f->max_span);
    DevBuf<BatchSeg> d_segs;
    DevBuf<int64_t> d_spans;
    d_segs.pool = &e->pool; d_spans.pool = &e->pool; p->d_mr_off.pool = &e->pool; p->d_mr_rec.pool = &e->pool;
    hipStream_t st = e->stream;
    int rc = d_segs.upload(segs, st);
    if (rc == PC_OK) rc = d_spans.upload(spans, st);
    room(rc, p->d_mr_off, (size_t)npair + 1);
    if (rc != PC_OK) return rc;
    const MapParams mp = e->params();
    HIP_TRY(hipMemsetAsync(p->d_mr_off.p + npair, 0, 8, st));
    hipLaunchKernelGGL((k_mapped_reads_batch<false>), dim3((unsigned)npair), dim3(kWG), 0, st, d_segs.p, nseg, e->d_files.p, nfiles, d_spans.p, mp,
                       p->d_mr_off.p, (const unsigned long long *)nullptr, (uint32_t *)nullptr);
    {
        DevBuf<uint8_t> d_tmp;
        d_tmp.pool = &e->pool;
        PC_TRY(cub_run(d_tmp, [=](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, p->d_mr_off.p, p->d_mr_off.p, (int)(npair + 1), st); }));
        static_assert(sizeof(unsigned long long) == sizeof(int64_t), "offsets are copied as they are");
        HIP_TRY(hipMemcpyAsync(offsets, p->d_mr_off.p, (size_t)(npair + 1) * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    const int64_t tot = offsets[npair];
    if (tot >= (int64_t)0xffffffffu) return fail(PC_ERR_ARG, "pc_mapped_reads_batch: more than 2^32-2 mapped reads in one batch; split the segments");
    PC_TRY(p->d_mr_rec.reserve((size_t)std::max<int64_t>(tot, 1)));
    hipLaunchKernelGGL((k_mapped_reads_batch<true>), dim3((unsigned)npair), dim3(kWG), 0, st, d_segs.p, nseg, e->d_files.p, nfiles, d_spans.p, mp,
                       (unsigned long long *)nullptr, p->d_mr_off.p, p->d_mr_rec.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // (the segment table and the spans return to the pool)
    p->mr_total = tot;
    *total = tot;
    return PC_OK;
}

int pc_read_mapped_reads(pc_engine *e, pc_plan *p, uint32_t *rec, int64_t total) {
    if (!e || !p || p->e != e) return fail(PC_ERR_ARG, "pc_read_mapped_reads: bad arguments");
    if (total != p->mr_total || (total > 0 && !rec)) return fail(PC_ERR_ARG, "pc_read_mapped_reads: expected %lld records (pc_mapped_reads_batch)", (long long)p->mr_total);
    HIP_TRY(hipSetDevice(e->device));
    if (total > 0) HIP_TRY(hipMemcpyAsync(rec, p->d_mr_rec.p, (size_t)total * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return PC_OK;
}

} // extern "C"

// ================================================================== compressed BAM on the GPU (bam_decoder.hip.h, bam_kernels.hip.h)
#include "bam_decoder.hip.h"
#include "sam_decoder.hip.h"
#include "track_decoder.hip.h"
#include "bigwig_decoder.hip.h"
#include "deflate_encoder.hip.h"
#include "bigwig_writer.hip.h"
#include "bigwig_summary.hip.h"
