/*
 * plastid_counts.h -- C ABI of the MI355X per-position read-counting engine.
 *
 * This is the drop-in boundary for ONE hot path of plastid (reference paths are
 * relative to the reference checkout):
 *
 *   plastid/genomics/genome_array.py:760-832   BAMGenomeArray.get_reads_and_counts
 *   plastid/genomics/genome_array.py:861-928   BAMGenomeArray.__getitem__ / get
 *   plastid/genomics/map_factories.pyx:167-839 the five BAM mapping functions + SizeFilterFactory
 *   plastid/genomics/roitools.pyx:3221-3315    SegmentChain.get_counts / get_masked_counts
 *
 * The reference has no FFI on this path (it is Cython calling pysam); the entry
 * points below are what a binding for the path would bind.  Each one cites the
 * reference interface it replaces.  INTEGRATION.md shows the reference-side
 * ctypes stub.
 *
 * Conventions
 *   - every function returns 0 on success, a negative PC_ERR_* code on failure;
 *     pc_last_error() returns a message for the calling thread's last failure;
 *   - no exceptions cross the ABI, no torch types, plain pointers and sizes;
 *   - host buffers are caller-owned, C-contiguous; device buffers are
 *     engine-owned behind the opaque handles;
 *   - one engine per GPU; an engine and its plans are not thread-safe;
 *   - there is NO CPU fallback: without a usable HIP device pc_create() fails.
 */
#ifndef PLASTID_COUNTS_H
#define PLASTID_COUNTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever entry points are added or the meaning of an argument changes (6: round 6).  A binding checks it
 * BEFORE it resolves any other symbol: a stale library then fails with a version message, not with a missing symbol. */
#define PC_ABI_VERSION 23

typedef struct pc_engine pc_engine;
typedef struct pc_plan pc_plan;

/* error codes */
#define PC_OK 0
#define PC_ERR_ARG (-1)        /* invalid argument (ValueError in the Python shim)   */
#define PC_ERR_HIP (-2)        /* HIP runtime failure                                */
#define PC_ERR_NOMEM (-3)
#define PC_ERR_UNSORTED (-4)   /* records not coordinate sorted (pysam.fetch raises) */
#define PC_ERR_STATE (-5)      /* e.g. counting before alignments / mapping are set  */

/* mapping rules: plastid/genomics/map_factories.pyx */
#define PC_MAP_FIVE 0    /* FivePrimeMapFactory                    :278-374 */
#define PC_MAP_THREE 1   /* ThreePrimeMapFactory                   :377-474 */
#define PC_MAP_CENTER 2  /* CenterMapFactory                       :167-276 */
#define PC_MAP_VAR5 3    /* VariableFivePrimeMapFactory            :477-650 */
#define PC_MAP_STRAT5 4  /* StratifiedVariableFivePrimeMapFactory  :653-791 */

/* strand codes: plastid/genomics/c_common.pxd:1-6 */
#define PC_STRAND_UNDEF 0
#define PC_STRAND_FWD 1
#define PC_STRAND_REV 2
#define PC_STRAND_UNS 3
/* OR-ed into a segment's strand byte: do not strand-filter reads (semantics of
 * calling a map factory directly on a read list, map_factories.pyx:308, instead
 * of going through BAMGenomeArray, genome_array.py:812-815) */
#define PC_STRAND_NOFILTER 0x10

/* record flag bits (the `flags` array of pc_add_alignment_file) */
#define PC_FLAG_REVERSE 0x01   /* pysam AlignedSegment.is_reverse                       */
#define PC_FLAG_EXCLUDED 0x80  /* dropped by a host-side read filter (genome_array.py:819-820) */

#define PC_OUT_INT64 0
#define PC_OUT_FLOAT64 1

#define PC_OFFSET_TABLE_LEN 10000 /* map_factories.pxd:10-12 */
#define PC_MAX_ALIGNED_LEN 65535 /* of the packed 16-bit field; longer reads: pc_add_alignment_file_wide */

const char *pc_last_error(void);
int pc_abi_version(void);
/* number of HIP devices visible; never initialises more than the runtime needs */
int pc_device_count(void);

/* ---- engine ------------------------------------------------------------- */
int pc_create(int device, pc_engine **out);
/* Every plan of the engine must have been destroyed first (plans return their device blocks to it). */
int pc_destroy(pc_engine *e);
/* A destroyed engine leaves its idle device blocks to the process (up to PC_POOL_RESERVOIR_GB per device, default 4; the
 * last engine of a device to go trims what is kept to that default) for the next engine on the same device --
 * BAMGenomeArray objects come and go, and allocating tens of GB again can take seconds.
 * This returns them to the driver (no reference counterpart; for callers that share the GPU with other libraries). */
int pc_release_cached_memory(int device);
/* Page-locked host memory for count vectors that are read back repeatedly (pc_read_counts into such a buffer is one DMA
 * at the rate of the link, no staging through the transfer ring): `bytes` of it, touched by the calling thread's NUMA
 * policy.  What the reference returns from get_counts is an ordinary numpy array (roitools.pyx:3259-3271); this is an
 * allocator a caller MAY use for the array it hands to pc_read_counts -- no reference counterpart. */
int pc_host_alloc(pc_engine *e, uint64_t bytes, void **out);
int pc_host_free(pc_engine *e, void *p);
/* The PC_* tuning/diagnostic environment knobs are read once, by pc_create;
 * this re-reads them (tests and experiments only -- no reference counterpart). */
int pc_reload_knobs(pc_engine *e);

/* ---- alignments: replaces pysam AlignmentFile.fetch + AlignedSegment.positions /
 * .is_reverse as consumed at genome_array.py:800-815 and map_factories.pyx:243,
 * 349, 448, 629, 769, 838.  One call per BAM file, in the order the files were
 * given to BAMGenomeArray (file-major order matters, genome_array.py:800-809).
 *
 *   n          records, sorted by (tid, pos), ties in file order; at most 2^31 - 2 per file (and
 *              2^31 - 2 runs of multi-run reads): record indices and window bins are 32-bit (PC_ERR_ARG beyond that --
 *              split larger inputs into several files, which are counted as one)
 *   tid,pos    reference index (0 <= tid < ntid) and leftmost aligned coordinate
 *   alen       L = len(read.positions): aligned reference positions (M/=/X)
 *   flags      PC_FLAG_* bits
 *   nblk       number of maximal runs of contiguous aligned positions (0 iff L==0)
 *   nrun,blk_* runs (start,len) of every record with nblk >= 2, record after
 *              record; a record with nblk == 1 is the implicit run [pos, pos+L)
 *
 * The arrays are the caller's (pageable or page-locked host memory) and are only read: they cross PCIe as they are
 * and are validated on the GPU.  A file that breaks the contract is refused (PC_ERR_ARG; PC_ERR_UNSORTED for records
 * out of (tid, pos) order) with the defect of the LOWEST record index in pc_last_error(), and nothing is staged.
 */
int pc_clear_alignments(pc_engine *e);
int pc_add_alignment_file(pc_engine *e, int64_t n, int32_t ntid, const int32_t *tid,
                          const int32_t *pos, const uint16_t *alen, const uint8_t *flags,
                          const uint8_t *nblk, int64_t nrun, const int32_t *blk_start,
                          const int32_t *blk_len);
/* The same with WIDE records: reads whose aligned length exceeds 65 535 or that have more than 255 aligned runs (long
 * reads; the reference has no such limit -- read.positions is a Python list, map_factories.pyx:243, 349).  Such a
 * record carries the markers alen = 65535 AND nblk = 255 in the packed arrays and its true values in the side arrays:
 *   n_wide                 number of wide records
 *   wide_idx               their record indices, ascending
 *   wide_alen, wide_nblk   true L and run count (int32); runs in blk_* as for every record with >= 2 runs */
int pc_add_alignment_file_wide(pc_engine *e, int64_t n, int32_t ntid, const int32_t *tid,
                               const int32_t *pos, const uint16_t *alen, const uint8_t *flags,
                               const uint8_t *nblk, int64_t nrun, const int32_t *blk_start,
                               const int32_t *blk_len, int64_t n_wide, const int64_t *wide_idx,
                               const int32_t *wide_alen, const int32_t *wide_nblk);
/* replace the flags of one staged file (host-side filters changed) */
int pc_update_flags(pc_engine *e, int file, int64_t n, const uint8_t *flags);
int pc_num_files(pc_engine *e);
int64_t pc_num_records(pc_engine *e, int file);
/* Entries the point rules stream for one staged file: duplicate reads -- same contig, position, aligned length and
 * strand -- are staged a second time as one entry with a multiplicity (up to 16 reads per entry; excluded reads and
 * reads binned from the side lists are not carried), and counted once.  Equal to pc_num_records when the file keeps no
 * such stream (too few duplicates to be worth its memory).  -1: bad file index. */
int64_t pc_stream_entries(pc_engine *e, int file);
/* Entries of the file's CANONICAL stream: one entry per contig, strand and MAPPED position under the current point rule
 * and size filter (up to 16 reads per entry) -- what a plan over this one file with '+' / '-' segments only streams
 * under the fiveprime, threeprime and variable rules.  Built at the first count of such a plan, rebuilt when the rule,
 * the filter or the file's flags change; PC_NO_CANON=1 (read at pc_create / pc_reload_knobs) forbids it.  -1: no such
 * stream right now (never wanted, forbidden, stale, more than one file staged, or not at most 0.9 x the entries of the
 * stream it would replace), or a bad file index. */
int64_t pc_canonical_entries(pc_engine *e, int file);
/* Cells of the file's DENSE VECTOR: one 16-bit cell per contig, strand ('+', '-') and position of the contig's extent (the
 * furthest aligned end staged) with the count of that position under the current point rule, size filter and FLAG /
 * MAPQ / NH filters; counts of 65 535 and more sit in a sorted overflow list.  A plan over this one file with '+' / '-'
 * segments only and no summed slice is served from it by one gather kernel when the vector takes no more bytes than the
 * stream it replaces (2 bytes per cell against 4 per entry) and fits the build's cap (2^27 cells).  Built at the first
 * count of such a plan, rebuilt when the rule, a filter or the file's flags change, dropped with the file; PC_NO_DENSE=1
 * (read at pc_create / pc_reload_knobs) forbids it.  -1: the engine's last pc_count was not served from it (plan or file
 * not eligible, forbidden, more than one file staged), the rule or a filter has changed since, or a bad file index. */
int64_t pc_dense_cells(pc_engine *e, int file);
/* Which gather served the engine's last pc_count from the dense vector.  CHUNKS: one workgroup per 1 024 aligned
 * elements of the output, every element written (no zero fill of the gaps between slices).  ITEMS: one workgroup per
 * piece of a segment -- plans whose output ranges overlap, an output block that is not 128-byte aligned, or
 * PC_DENSE_ITEMS=1 (read at pc_create / pc_reload_knobs).  NONE: that count was not served from the vector, or
 * pc_dense_cells(e, 0) is -1 for any of its reasons (the rule or a filter has changed since, ...). */
#define PC_DENSE_PATH_NONE 0
#define PC_DENSE_PATH_ITEMS 1
#define PC_DENSE_PATH_CHUNKS 2
int pc_dense_path(pc_engine *e);
/* Read objects of a staged file back (the reference hands pysam reads to its callers: get_reads / reads_out,
 * genome_array.py:834-859, and to filter functions, :697-722) -- for files whose records never visited the host
 * (pc_add_alignment_bam[_path | _span]).  pc_read_records: per requested record index its reference id, first aligned
 * position, aligned length L = len(read.positions), strand (1: reverse), number of aligned runs, and -- pointers may be
 * NULL -- the SAM FLAG word and MAPQ (from the strand alone / 255 when the file carries none).  pc_read_record_runs: the
 * aligned runs of the same records, record k's from slot run_at[k] on (the caller's exclusive sum of its run counts;
 * nruns = their total): read.positions is their concatenation. */
int pc_read_records(pc_engine *e, int file, int64_t n, const int64_t *idx, int32_t *tid, int32_t *pos, int32_t *alen, uint8_t *reverse,
                    int32_t *nblk, uint16_t *flag16, uint8_t *mapq);
int pc_read_record_runs(pc_engine *e, int file, int64_t n, const int64_t *idx, const int64_t *run_at, int64_t nruns, int32_t *start,
                        int32_t *len);

/* ---- read filters on the SAM FLAG word and MAPQ.  The reference's filter contract is "a function of the
 * pysam.AlignedSegment" (BAMGenomeArray.add_filter, plastid/genomics/genome_array.py:697-722; every filter is called on
 * every fetched read, :819-820).  Filters of the common kind -- `not read.is_secondary`, `not read.is_duplicate`,
 * `read.mapping_quality >= 10`, `read.is_proper_pair` -- depend on two fields of the BAM record only (FLAG: u16 at
 * byte 14, MAPQ: u8 at byte 9 of the record body, kent/src/htslib/sam.c bam_read1; bit names htslib/sam.h:110-132):
 *   pc_set_alignment_sam   hands the engine those two columns of one staged file (3 bytes per record; files staged by
 *                          pc_add_alignment_bam[_path] carry them already);
 *   pc_set_flag_filter     a record is kept iff (flag & require) == require && (flag & exclude) == 0 && mapq >= min_mapq.
 *                          Evaluated on the GPU in one pass per file and folded into the exclusion bit the counting
 *                          kernels honour, on top of the caller's own PC_FLAG_EXCLUDED verdicts; enabled = 0 lifts it.
 *                          PC_ERR_STATE if a staged file has records but no FLAG / MAPQ columns (also from pc_count,
 *                          for a file staged after the filter was set). */
int pc_set_alignment_sam(pc_engine *e, int file, int64_t n, const uint16_t *flag, const uint8_t *mapq);
int pc_set_flag_filter(pc_engine *e, int enabled, uint32_t require, uint32_t exclude, int min_mapq);
/* The same for the NH:i tag (number of reported alignments of the query): `lambda read: read.get_tag("NH") == 1` is the
 * usual unique-mapper filter of the reference's users (genome_array.py:697-722, applied :819-820).
 *   pc_set_alignment_nh    hands the engine the tag's value per record of one staged file (uint16, clamped to 65 535;
 *                          0: the record has no NH tag); files staged by pc_add_alignment_bam* carry it already.
 *   pc_set_nh_filter       max_nh > 0: a record is kept iff it has the tag and its value is <= max_nh; 0 lifts the test.
 *                          Combines with pc_set_flag_filter and the caller's own exclusions (all must keep the read). */
int pc_set_alignment_nh(pc_engine *e, int file, int64_t n, const uint16_t *nh);
int pc_set_nh_filter(pc_engine *e, int max_nh);

/* ---- mapping rule: replaces BAMGenomeArray.set_mapping (genome_array.py:935-963)
 * with one of the five factories.  `param` = offset (FIVE/THREE) or nibble
 * (CENTER).  fw/rc = forward_offsets/reverse_offsets[table_len] built on the
 * host by the restated __cinit__ rules (map_factories.pyx:494-543); entries are
 * -1 (no usable offset) or 0 <= off < L.  min_len/max_len: STRAT5 rows. */
int pc_set_mapping(pc_engine *e, int kind, int param, const int32_t *fw, const int32_t *rc,
                   int table_len, int min_len, int max_len);
/* SizeFilterFactory(min,max) (map_factories.pyx:794-839); max == -1: no maximum */
int pc_set_size_filter(pc_engine *e, int enabled, int min_len, int max_len);
/* set_normalize/set_sum (genome_array.py:482-520): out = count / sum * 1e6 */
int pc_set_normalize(pc_engine *e, int enabled, double sum);
int pc_mapping_rows(pc_engine *e);

/* ---- query plan: a batch of GenomicSegments and where their count vectors go.
 * Replaces the per-segment loop of SegmentChain.get_counts (roitools.pyx:3259-3271)
 * and BAMGenomeArray.get (genome_array.py:891-928).  For segment s, genomic
 * position start[s]+i (0 <= i < end[s]-start[s]), row r is written to
 *     out[out_off[s] + out_step[s]*i + r*row_stride[s]]
 * so a '-' chain is laid out 5'->3' by giving its segments out_step = -1
 * (roitools.pyx:3270-3271, genome_array.py:829-830).  out_step = 0 SUMS the slice instead:
 *     out[out_off[s] + r*row_stride[s]] += sum_i count(start[s]+i, r)
 * (fused region statistics, numpy.nansum(chain.get_masked_counts(ga)) of
 * bin/counts_in_region.py:120; integer rules without normalisation only).  tid < 0 or >= ntid means
 * "chromosome not in the array": the slice is zero (genome_array.py:795-798).
 * A plan depends only on the intervals; it can be reused across alignment sets,
 * mapping rules and normalisation settings with the same number of rows.
 */
int pc_plan_create(pc_engine *e, int64_t nseg, const int32_t *tid, const int64_t *start,
                   const int64_t *end, const uint8_t *strand, const int64_t *out_off,
                   const int8_t *out_step, const int64_t *row_stride, int64_t out_elems, int rows,
                   pc_plan **out);
int pc_plan_destroy(pc_plan *p);
/* SegmentChain.get_position_list / _get_position_hash (roitools.pyx:1450-1484, 2059-2080) for the whole
 * batch: host_out[k] = genomic coordinate of output element k of the plan's layout (-1 where no segment
 * writes; every row of a multi-row layout gets the coordinates; summed slices have none). */
int pc_plan_coordinates(pc_engine *e, pc_plan *p, int64_t *host_out, int64_t out_elems);
int64_t pc_plan_positions(pc_plan *p); /* distinct (strand-mode, position) pairs counted */
int64_t pc_plan_tiles(pc_plan *p);
/* The plan's tables as pc_plan_create built them (tests compare the GPU builder of large annotations with the host
 * builder, table by table).  which: 0 tiles (32-byte records), 1 island pieces (24), 2 output pieces (40), 3 per-segment
 * gather records (64), 4 scalars as int64[12] = {window size, strand-mode mask, modes per window (max), histogram
 * positions, covered output elements, has summed slices, output needs zeroing, tiles, pieces, output pieces, built on
 * the GPU, segments}.  Copies min(cap_bytes, table bytes) to `buf`; *bytes = table bytes. */
int pc_plan_table(pc_plan *p, int which, void *buf, int64_t cap_bytes, int64_t *bytes);

/* ---- counting: map_fn(list(reads), roi) for every segment of the plan
 * (genome_array.py:823), then normalisation/strand layout.  pc_count launches
 * asynchronously on the engine's stream; results stay in HBM until read. */
int pc_count(pc_engine *e, pc_plan *p, int out_dtype);
int pc_sync(pc_engine *e);
/* ONE segment in ONE call: `ga[segment]` / `BAMGenomeArray.get(segment, roi_order)` (genome_array.py:861-928) -- what the
 * reference's scripts do region by region (bin/psite.py:181-192) -- without a plan object: the window travels in the
 * kernel's arguments, the counts come back through page-locked memory the kernel writes itself.  host_out: end - start
 * elements of int64 / float64 (reads per million when normalisation is on), reversed when `reverse_out` (roi_order on
 * a '-' segment, :829-830).  PC_ERR_STATE when the query does not qualify -- several staged files, the center or the
 * stratified rule, a segment longer than 4 096 positions -- and the caller takes pc_plan_create; the DataWarning of the
 * map functions is not reported here (a caller that needs it asks pc_warn_flags through a plan). */
int pc_query_segment(pc_engine *e, int32_t tid, int64_t start, int64_t end, uint8_t strand, int reverse_out, int out_dtype,
                     void *host_out);
int pc_read_counts(pc_engine *e, pc_plan *p, void *host_out, int64_t out_elems);
/* device pointer/stream of the last pc_count output (for zero-copy consumers) */
void *pc_counts_device_ptr(pc_plan *p);
void *pc_stream(pc_engine *e);

/* ---- export: run-length encoding of the last pc_count output on the GPU, so that only the runs
 * cross PCIe (BAMGenomeArray.to_bedgraph / to_variable_step, genome_array.py:990-1111).  A run
 * starts at element 0, wherever the 8-byte value differs from its predecessor, and at every multiple
 * of `period` elements (0: no such cut; the reference cuts its runs at window borders; 1 lists
 * every element).  pc_read_rle returns, for run k, its first element and its value (int64 or
 * float64 as counted); run k ends where run k+1 starts, the last one at out_elems. */
int pc_rle(pc_engine *e, pc_plan *p, int64_t period, int64_t *n_runs);
int pc_read_rle(pc_engine *e, pc_plan *p, int64_t *starts, void *values, int64_t n_runs);

/* per-segment "the reference would emit its DataWarning" flags
 * (map_factories.pyx:258-263, 360-365, 459-464, 643-648) for the last pc_count */
int pc_warn_flags(pc_engine *e, pc_plan *p, uint8_t *flags);
/* the same, plus (last_len, may be NULL) the aligned length of the LAST such read in fetch order per
 * flagged segment, -1 otherwise: the length VariableFivePrimeMapFactory names in its warning
 * (`no_offset_length`, map_factories.pyx:633-648) */
int pc_warn_details(pc_engine *e, pc_plan *p, uint8_t *flags, int32_t *last_len);

/* Sum over all output elements of the last pc_count, left in HBM for an RCCL
 * all-reduce (int64 for PC_OUT_INT64, fixed-order float64 otherwise);
 * host_out8 (8 bytes) may be NULL. */
int pc_total(pc_engine *e, pc_plan *p, void *host_out8);
void *pc_total_device_ptr(pc_plan *p);

/* reads_out of map_fn for ONE segment over records [rec_lo, rec_hi) of `file`
 * (genome_array.py:800-823): mask[i - rec_lo] = 1 iff the record is fetched
 * (htslib overlap), passes strand + filters and is mapped into the segment. */
int pc_mapped_reads(pc_engine *e, int file, int64_t rec_lo, int64_t rec_hi, int32_t tid,
                    int64_t start, int64_t end, uint8_t strand, uint8_t *mask);

/* reads_out for EVERY segment of a plan in one pass: which reads the reference's map function appends for each
 * segment (genome_array.py:800-823 fetch -> strand -> filters -> map_fn; `get_reads` :834-859; bin/psite.py:182 and
 * bin/phase_by_size.py:187 ask per region).  A CSR over (segment, file) pairs, pair index = segment * n_files + file:
 * offsets[n_segments * n_files + 1]; the reads of a pair are listed in file order, so a segment's reads come out in
 * the reference's fetch order (file-major).  pc_mapped_reads_batch computes the lists on the device and returns the
 * offsets and *total = offsets[last]; pc_read_mapped_reads copies the record indices (within their file) out. */
int pc_mapped_reads_batch(pc_engine *e, pc_plan *p, int64_t *offsets, int64_t *total);
int pc_read_mapped_reads(pc_engine *e, pc_plan *p, uint32_t *rec, int64_t total);

/* HIP-event timing of pc_count on the engine's stream.  level 0 (default): no events are
 * recorded; 1: the whole call and the histogram / center kernel; 2: every phase.  Each
 * recorded event costs a few microseconds of stream time, which is why it is opt-in. */
int pc_set_profiling(pc_engine *e, int level);
/* last timed pc_count, milliseconds: [0] total, [1] work-list, [2] histogram/center kernel,
 * [3] long reads, [4] gather, [5] zero-fill ([1],[3],[4],[5] are 0 below level 2).
 * Returns number of entries written. */
int pc_last_timing(pc_engine *e, double *ms, int n);
/* algorithmic bytes of the last pc_count (SURVEY.md section 8d formula) */
int64_t pc_last_algorithmic_bytes(pc_engine *e);
/* Measurement helper for the center rule (CenterMapFactory.__call__, map_factories.pyx:200-265): counts `plan` once
 * more in a diagnostic launch and reports how many replay steps (one step = entry j of each 16-lane row applied to the
 * row: 3 single-rate vector instructions + one v_fmac_f64) and how many waves the launch executed -- the numerator
 * of the kernel's vector-issue bound that bench.py reports beside the HBM fraction.  No reference counterpart. */
int pc_center_replay_steps(pc_engine *e, pc_plan *p, int64_t *steps, int64_t *waves);
/* Row fill of the center kernel's dispatch list (plans over one alignment file, after a center-rule count): the four
 * 16-lane rows of a wave replay in lock-step, one step per entry of the LONGEST row, so a step does useful work for
 * row_entries / row_slots of its four rows -- row_entries = entries of all rows of all dispatch entries, row_slots =
 * 4 x replay steps.  A measurement helper like pc_center_replay_steps; no reference counterpart. */
int pc_center_row_fill(pc_engine *e, pc_plan *p, int64_t *row_entries, int64_t *row_slots);
/* Measured streaming rates of this GPU (GB/s) for the access patterns of the tile kernel: 16-byte
 * contiguous loads per lane and 8-byte contiguous stores per lane over a buffer of `bytes` bytes
 * (>= 1 MiB; use several hundred MB to get past the 256 MiB Infinity Cache).  The second roofline
 * denominator of SURVEY.md 8(d); no reference counterpart. */
int pc_stream_probe(pc_engine *e, int64_t bytes, int iters, double *read_gbps, double *write_gbps);

/* ---- compressed BAM on the GPU (extends SURVEY.md 8(f1)).
 * Replaces, for a whole coordinate-sorted file, what the reference gets from pysam / htslib: `pysam.AlignmentFile(X, "rb")`
 * + `fetch` + `read.positions` / `read.is_reverse` / `.mapped` (plastid/genomics/genome_array.py:660, 669, 690, 800-815),
 * i.e. htslib's BGZF reader (kent/src/htslib/bgzf.c:292-340 block header, :421-530 inflate + CRC check), bam_read1
 * (kent/src/htslib/sam.c) and the CIGAR operation table (kent/src/htslib/htslib/sam.h:64-104).
 * `image` = the bytes of the .bam file (host memory; e.g. an mmap).  The BGZF members are inflated on the GPU (one wave
 * per member), the BAM records found and decoded there; what comes back are the packed columns pc_add_alignment_file
 * takes -- bit-identical to those of the host decoder (plastid_amd/csrc/bam_stager.cpp), same checks, same messages.
 * Errors: PC_ERR_ARG (not a BGZF / BAM file, damaged member, CRC mismatch, corrupt record), PC_ERR_UNSORTED (not
 * coordinate sorted -- pysam raises ValueError at fetch, genome_array.py:784-787). */
typedef struct pc_bam pc_bam;
int pc_bam_open(pc_engine *e, const void *image, int64_t size, const char *name /* for messages; may be NULL */, pc_bam **out);
/* counts[0] staged (placed) records, [1] runs of the multi-run ones, [2] mapped (flag 0x4 unset: pysam's .mapped),
 * [3] all records, [4] wide records, [5] BGZF members, [6] inflated bytes, [7] members whose first-record guess was redone */
int pc_bam_counts(pc_bam *b, int64_t *counts8);
/* milliseconds on the engine's stream: [0] upload of the image, [1] inflate + CRC, [2] record chain, [3] fields + columns */
int pc_bam_timing(pc_bam *b, double *ms4);
int pc_bam_nref(pc_bam *b);
const char *pc_bam_ref_name(pc_bam *b, int i);
int32_t pc_bam_ref_length(pc_bam *b, int i);
/* the columns, to caller-owned arrays of counts[0] / counts[1] / counts[4] elements (see pc_add_alignment_file_wide) */
int pc_bam_read(pc_bam *b, int32_t *tid, int32_t *pos, uint16_t *alen, uint8_t *flags, uint8_t *nblk, int32_t *blk_start,
                int32_t *blk_len, int64_t *wide_idx, int32_t *wide_alen, int32_t *wide_nblk);
/* the SAM FLAG word, MAPQ and l_seq of the same records (pysam: read.flag, .mapping_quality, .query_length -- what a
 * filter function may look at, genome_array.py:697-722); any pointer may be NULL */
int pc_bam_read_sam(pc_bam *b, uint16_t *flag, uint8_t *mapq, int32_t *lseq);
/* ... and their NH:i tags (0: none), what read.get_tag("NH") / read.has_tag("NH") answer from (pysam AlignedSegment; the
 * walk over the auxiliary fields is htslib's bam_aux_get, kent/src/htslib/sam.c). */
int pc_bam_read_nh(pc_bam *b, uint16_t *nh);
int pc_bam_close(pc_bam *b);
/* decode `image` and stage it as one more alignment file of the engine (reference ids = the file's own reference
 * list, which must be that of the files staged before it); *mapped (optional) = the file's mapped-read count */
int pc_add_alignment_bam(pc_engine *e, const void *image, int64_t size, const char *name, int64_t *mapped);
/* The same two calls for a file named by path (what `pysam.AlignmentFile(path, "rb")` takes, genome_array.py:660): the
 * library maps the file itself -- the pages are touched by all host threads at once instead of one soft fault after the
 * other, and the mapping is taken down on a thread of its own after the call has returned. */
int pc_bam_open_path(pc_engine *e, const char *path, pc_bam **out);
int pc_add_alignment_bam_path(pc_engine *e, const char *path, int64_t *mapped);
/* REGION reads: what `AlignmentFile.fetch(reference, start, end)` returns (genome_array.py:800-809; htslib's iterator,
 * kent/src/htslib/hts.c:1924-1960) for a set of regions, decoded on the GPU.  The caller resolves the regions through the
 * file's BAI index (bins + 16 kb linear index: plastid_amd/csrc/bam_stager.cpp pb_resolve_regions) into
 *   voff_begin, voff_end   the span of virtual offsets (file offset of a BGZF member << 16 | offset in its payload) that
 *                          holds every chunk of every region; 0, 0: nothing overlaps (the header alone is read);
 *   nreg, tid, beg, end    the regions themselves by reference id, ascending by (tid, beg), merged (none overlap).
 * Only the members of the span -- and the leading ones that hold the header -- are uploaded and inflated; the record
 * chain starts at the record the index points to; a placed record stays iff pos < end && endpos > beg for one of the
 * regions (htslib's rule, as the host reader applies it).  counts[2] / *mapped = mapped records among those kept (the
 * whole file's count lives in the index).
 * A span is read as the chunk list of ONE chunk [voff_begin, voff_end) (none for 0, 0) by pc_bam_open_chunks below, with
 * that call's checks and errors: every offset has to name a BGZF member of the file and a place inside its payload.  For
 * a span that no valid index holds this is stricter than the span reader of ABI 6 was; among other things, one that does
 * not start at a BGZF member is PC_ERR_ARG "the index does not belong to this BAM file (...)" (not the error of the
 * member walk that ran into it), and one that ends at the file's size with a non-zero offset in the payload -- inside a
 * member that does not exist -- is refused with the same message (it is not read up to the end of the file). */
int pc_bam_open_span(pc_engine *e, const char *path, uint64_t voff_begin, uint64_t voff_end, int nreg, const int32_t *tid,
                     const int64_t *beg, const int64_t *end, pc_bam **out);
int pc_add_alignment_bam_span(pc_engine *e, const char *path, uint64_t voff_begin, uint64_t voff_end, int nreg, const int32_t *tid,
                              const int64_t *beg, const int64_t *end, int64_t *mapped);
/* (ABI 7) The same region reads from the CHUNK LIST of the index instead of its span (plastid_amd/csrc/bam_stager.cpp
 * pb_resolve_chunks: the regions' chunks, clipped by the linear index, sorted and merged -- what htslib's iterator walks
 * chunk by chunk, hts.c:1924-1960):
 *   nchunk, voff_beg, voff_end   [voff_beg[k], voff_end[k]) ascending and disjoint; nchunk = 0: the header alone is read.
 * Only the leading members that hold the header and the members the chunks touch are uploaded and inflated: two far-apart
 * regions cost what they hold, not the file between them.  Chunks that share or touch a member form one RUN (one
 * contiguous upload; one record chain from the run's first chunk start to its last chunk end -- the records between two
 * chunks of a run are decoded and dropped by the overlap rule).  The columns are those pc_bam_open_span gives over the
 * enclosing span, record for record.  One rank of a multi-GPU job stages its genome range of ONE shared file this way
 * (SURVEY 8e).  Errors: as pc_bam_open, plus PC_ERR_ARG, "the index does not belong to this BAM file (...)", for a foreign
 * index: a chunk beyond the end of the file, one that does not start at a member, one that ends inside a record. */
int pc_bam_open_chunks(pc_engine *e, const char *path, int nchunk, const uint64_t *voff_beg, const uint64_t *voff_end, int nreg,
                       const int32_t *tid, const int64_t *beg, const int64_t *end, pc_bam **out);
int pc_add_alignment_bam_chunks(pc_engine *e, const char *path, int nchunk, const uint64_t *voff_beg, const uint64_t *voff_end,
                                int nreg, const int32_t *tid, const int64_t *beg, const int64_t *end, int64_t *mapped);
/* what an open read: [0] compressed bytes of the file uploaded to HBM, [1] runs they came in (1: a whole file), [2] BGZF
 * members inflated, [3] inflated bytes */
int pc_bam_stats(pc_bam *b, int64_t *out4);
/* (ABI 11) COORDINATE SORT AT DECODE: a whole-file read of a BAM file in any record order (an aligner's output, a
 * name-sorted or collated file) -- what `samtools sort` is run for in front of every reader that needs coordinate order.
 * The `_flags` twins of the four whole-file entry points take PC_BAM_SORT in `flags` (flags 0: the call without the
 * suffix, bit for bit; any other bit: PC_ERR_ARG).  With it the staged records come out
 *   placed records first, ordered by (reference id, POS field, reverse-strand bit of FLAG), ties in file order (a stable
 *   sort; placed but unmapped records sort by their coordinates like any other); unplaced records last, not staged --
 * the comparator of a coordinate sort (samtools' bam1_lt as this project knows it: tid, pos, reverse bit; pinned by this
 * project's own tests, not against samtools).  The key is POS, not the first aligned position.  A file that is in order
 * already by the test of pc_bam_open ((tid, POS) non-decreasing, no placed record behind an unplaced one) is not touched:
 * the columns are those of flags 0, whatever the strand order inside its ties.  PC_ERR_UNSORTED cannot occur; a
 * record's own defects are reported as by pc_bam_open, lowest record number first, then an alignment that starts with a
 * deletion and so breaks the order of first aligned positions among its SORTED neighbours, a truncated last record last.
 * (A file that is in order already goes through the checks of pc_bam_open and reports what pc_bam_open reports: of a
 * deletion-order pair and a record's own defect, the one with the lower record number.  The host reader's pb_load_sorted
 * gives a record's own defect precedence in that case too; files with both defects are the only ones where the two differ.)
 * The span and chunk reads take no flag: an index of an unsorted file means nothing. */
#define PC_BAM_SORT 1u
int pc_bam_open_flags(pc_engine *e, const void *image, int64_t size, const char *name, uint32_t flags, pc_bam **out);
int pc_bam_open_path_flags(pc_engine *e, const char *path, uint32_t flags, pc_bam **out);
int pc_add_alignment_bam_flags(pc_engine *e, const void *image, int64_t size, const char *name, uint32_t flags, int64_t *mapped);
int pc_add_alignment_bam_path_flags(pc_engine *e, const char *path, uint32_t flags, int64_t *mapped);
/* out4: [0] 1 if the open asked for PC_BAM_SORT, [1] 1 if the file was in order (nothing was sorted), [2] records whose
 * staged index differs from their rank among the placed records in file order, [3] key bits the radix sort looked at
 * (33 + the bits of the largest reference id; 0: no sort ran); *ms (optional): GPU time of the sort phase -- the key
 * kernel, plus the sort, the ranks and the run offsets when the file was out of order */
int pc_bam_sort_stats(pc_bam *b, int64_t *out4, double *ms);
/* the 0-based record number in the file (all records counted, unplaced ones too) of every staged record, counts[0]
 * elements; PC_ERR_STATE when no record was moved (out4[2] == 0: staged record k is the k-th placed record of the file) */
int pc_bam_read_file_order(pc_bam *b, int64_t *rec_no);

/* ---- (ABI 14) SAM TEXT: an aligner's output as it is written (bowtie, bowtie2, bwa, hisat2, minimap2; STAR's default
 * Aligned.out.sam).  Replaces pysam opening a SAM file with `AlignmentFile(path)` and the `samtools view -b` that every
 * BGZF reader needs in front of it.  The text crosses PCIe once; line starts, fields and CIGAR strings are parsed by
 * kernels (csrc/sam_kernels.hip.h) that run the line parser of the host reader (csrc/sam_host.h), and the records go
 * through the placement of pc_bam_open -- order checks, or the coordinate sort with PC_BAM_SORT in `flags` (any other bit:
 * PC_ERR_ARG).  The result is an ordinary pc_bam: pc_bam_read, pc_bam_read_sam, pc_bam_read_nh, pc_bam_counts,
 * pc_bam_sort_stats and pc_bam_read_file_order give, bit for bit, what they give for the same records in a BAM file;
 * counts[5] (members) and counts[6] (inflated bytes) are 0, pc_bam_stats' out4[0] is the bytes of text uploaded, and
 * pc_bam_timing's four laps are upload, line starts, fields, placement + columns.
 * The header is the leading '@' lines; every @SQ gives a reference (SN, LN in 1 .. 2^31-1, any field order; a repeated SN
 * is refused), every other header line is ignored (@HD SO: too: the records decide).  A line has 11 tab-separated
 * mandatory fields; FLAG, POS and MAPQ are plain decimal; RNAME is '*' or the SN of an @SQ line; CIGAR is '*' or
 * <length 0 .. 2^28-1><one of MIDNSHP=X> repeated; l_seq is the length of SEQ (0 for '*'); NH is the value of the first
 * optional field that begins with "NH:i:", clamped to 0 .. 65 535.  "\r\n" line ends and a last line without '\n' are
 * read.  A malformed line is PC_ERR_ARG with "<path>: SAM line <n>: <what>" (n 1-based, header lines counted), the lowest
 * line first; PC_ERR_UNSORTED and the CIGAR defects the formats share are worded as for BAM.  Compressed SAM (gzip or
 * BGZF magic) is refused.  Limits: 2^31-2 records, and a body that fits HBM.
 * pc_add_alignment_sam_path_flags stages the file without its columns visiting the host, as pc_add_alignment_bam_path
 * does; *mapped (optional): the lines with FLAG bit 0x4 unset. */
int pc_sam_open_path_flags(pc_engine *e, const char *path, uint32_t flags, pc_bam **out);
int pc_sam_open_flags(pc_engine *e, const void *image, int64_t size, const char *name, uint32_t flags, pc_bam **out);
int pc_add_alignment_sam_path_flags(pc_engine *e, const char *path, uint32_t flags, int64_t *mapped);

/* ---- (ABI 8) the BAI index of a coordinate-sorted BAM file, built on the GPU.  Replaces `samtools index` / pysam.index,
 * i.e. htslib's sam_index_build for BAI (kent/src/htslib/sam.c:470-496: every record is pushed with POS, bam_endpos
 * (sam.c:338-344) and the virtual offset bgzf_tell gives (bgzf.c:569-572); hts_idx_push / hts_idx_finish, hts.c:1293-1351
 * and :1193-1291; the file layout of hts_idx_save, hts.c:1395-1457; SAM specification section 5): min_shift 14, 5 levels,
 * the pseudo-bin 37450 with the file range and the mapped / unmapped counts of every reference, n_no_coor.  The index a
 * region read needs (pc_bam_open_chunks) without an outside tool.  The bins are written in ascending order with 37450
 * last (htslib writes them in the order of its hash table); parsed, the two indexes are equal.
 * The build runs the whole-file open up to the record fields (upload, inflate + CRC, record chain, k_bam_fields and the
 * order checks), writes no column, and walks the records once more for their bins, runs, linear windows and counts; the
 * host finishes the index.  Errors: those of pc_bam_open with its messages (a file the decoder refuses has no index), and
 * PC_ERR_ARG "a BAI index cannot hold ..." for a reference longer than 2^29 or an alignment that reaches beyond it. */
typedef struct pc_bam_index pc_bam_index;
int pc_bam_index_build(pc_engine *e, const char *path, pc_bam_index **out);
/* The host half alone -- no engine, no GPU call; the build above ends in it (hts_idx_finish: update_loff's forward fill
 * and compress_binning, hts.c:1193-1275).  Input:
 *   n_runs, run_tid, run_bin, run_beg, run_end   the runs (maximal stretches of consecutive placed records with one
 *       reference id and one bin): [virtual offset of the first record, of the first record behind the run); in file order
 *       or already in (tid, bin) order with file order kept inside a bin;
 *   lin_start (n_ref + 1), linear                the 16 kb windows of reference t are linear[lin_start[t] .. lin_start[t + 1]):
 *       the offset of the first mapped record that covers the window, 0 where none does;
 *   ref_beg, ref_end, ref_mapped, ref_unmapped   per reference: the file range of its records and their counts (all 0:
 *       a reference without records);  n_no_coor: records without a reference. */
int pc_bam_index_finish(int n_ref, int64_t n_runs, const int32_t *run_tid, const uint32_t *run_bin, const uint64_t *run_beg,
                        const uint64_t *run_end, const int64_t *lin_start, const uint64_t *linear, const uint64_t *ref_beg,
                        const uint64_t *ref_end, const int64_t *ref_mapped, const int64_t *ref_unmapped, int64_t n_no_coor,
                        pc_bam_index **out);
/* ---- (ABI 10) the CSI index (SAM specification 5.3; htslib's sam_index_build with min_shift > 0, sam.c:477-485): the
 * index of a file whose references are longer than 2^29, or of any file with another leaf size.  min_shift: 8 .. 30, the
 * leaves hold 2^min_shift positions; the depth n_lvls is the smallest with max(reference length) + 256 <=
 * 2^(min_shift + 3 n_lvls), as htslib takes it from the header (0: one bin).  The same kernels with the shape as a
 * parameter; the windows of 2^min_shift positions never leave the GPU: they are forward-filled there and every bin takes
 * the offset of its first window (loff).  Errors: as pc_bam_index_build, and PC_ERR_ARG for a min_shift out of range, for
 * an alignment that reaches beyond 2^(min_shift + 3 n_lvls) and for a file whose windows, summed over the references,
 * exceed 2^28 (the message asks for a larger min_shift). */
int pc_bam_index_build_csi(pc_engine *e, const char *path, int min_shift, pc_bam_index **out);
/* The host half of a CSI build; no GPU call.  As pc_bam_index_finish, with run_loff -- per run the loff of its bin: the
 * filled window at the bin's first leaf, 0 beyond the reference's windows; the runs of one bin carry one value -- in place
 * of the linear arrays.  A bin >= ((1 << (3 n_lvls + 3)) - 1) / 7 is refused; the pseudo-bin is that number + 1. */
int pc_bam_index_finish_csi(int min_shift, int n_lvls, int n_ref, int64_t n_runs, const int32_t *run_tid, const uint32_t *run_bin,
                            const uint64_t *run_beg, const uint64_t *run_end, const uint64_t *run_loff, const uint64_t *ref_beg,
                            const uint64_t *ref_end, const int64_t *ref_mapped, const int64_t *ref_unmapped, int64_t n_no_coor,
                            pc_bam_index **out);
/* the serialised .bai file: *bytes = its size; copied to buf when cap holds it (call with cap 0 first).  For a CSI these
 * are the bytes of the UNCOMPRESSED payload ("CSI\1" ...): a .csi file is that payload in BGZF members, and this library
 * does not link zlib -- the caller compresses (plastid_amd.bam.build_index does). */
int pc_bam_index_bytes(pc_bam_index *idx, void *buf, int64_t cap, int64_t *bytes);
/* [0] records, [1] placed records, [2] runs before the finish, [3] chunks after it, [4] bins (the pseudo-bin not counted),
 * [5] linear entries (CSI: the windows held on the device), [6] n_no_coor, [7] mapped (what pysam's AlignmentFile.mapped
 * sums from the index) */
int pc_bam_index_stats(pc_bam_index *idx, int64_t *out8);
/* milliseconds: [0] upload, [1] inflate + CRC, [2] record chain (the engine's stream, as pc_bam_timing), [3] fields + order
 * checks, [4] index kernels, [5] read-back, [6] host finish, [7] the whole call (wall clock) */
int pc_bam_index_timing(pc_bam_index *idx, double *ms8);
int pc_bam_index_close(pc_bam_index *idx);

/* ---- COUNT TRACKS: a device-resident GenomeArray read from bedGraph / wiggle text (revision 15)
 * A pc_track is the reference's GenomeArray (plastid/genomics/genome_array.py:1323-1533) as a read-and-count object: one
 * float64 cell per contig, strand slot and position in HBM, filled from track text and read through a gather kernel.
 * pc_track_create (GenomeArray.__init__, :1354-1387): nstrands strand slots (1 .. 8; the binding maps '+', '-' ... to
 * 0, 1 ...); min_chr_size is the length an undeclared contig is born with.  pc_track_declare (the chr_lengths of :1382-1387)
 * names a contig and its length before any text is added; declared contigs come first in the contig order.  A track
 * belongs to its engine: pc_destroy takes the engine's remaining tracks with it, and their handles are dead then. */
typedef struct pc_track pc_track;
int pc_track_create(pc_engine *e, int nstrands, int64_t min_chr_size, pc_track **out);
int pc_track_destroy(pc_track *t);
int pc_track_declare(pc_track *t, const char *name, int64_t length);
/* add_from_wiggle (genome_array.py:1978-1994) over WiggleReader (plastid/readers/wiggle.py:43-174): the text -- bedGraph,
 * variableStep and fixedStep wiggle, mixed freely -- is uploaded as it is and parsed by the kernels of
 * csrc/track_kernels.hip.h; every yielded (contig, start, stop, value) is ADDED to cells [start, stop) of the strand slot,
 * overlapping lines in file order, a second call on top of the first.  The host reads only the lines that change the
 * reader's state (data headers, and bedGraph lines that name another contig than the bedGraph line before), the lines with
 * a token that is not plain (csrc/track_host.h: Python's int / float grammar and strtod) and the lines that reach a
 * contig's length.  Contigs not declared are born in the order of their first yielded line with min_chr_size; a line
 * whose end reaches the current length sets it to end + 10 000 (:1593-1602).  Cells are stored up to the furthest end
 * written per contig and strand slot (the extent), not up to the length.  A malformed line is PC_ERR_ARG with
 * "<path>: track line <n>: <what>" (n 1-based), the lowest line first, and leaves every cell as it was: a negative start,
 * a token Python's int / float refuse, a data line under a header without chrom=, a fixedStep data line of several tokens,
 * coordinates beyond 2^40.  "\r\n" line ends and a last line without '\n' are read.  `name`: what messages call the text. */
int pc_track_add_text(pc_track *t, const void *image, int64_t size, const char *name, int strand_slot);
int pc_track_add_path(pc_track *t, const char *path, int strand_slot);
/* chroms() / lengths() (genome_array.py:1613-1615 and the arrays' sizes): contigs in their order -- declared ones, then the
 * others by first yielded line; the extent is the number of cells stored for one strand slot (positions beyond it are 0).
 * -1 / NULL: bad index. */
int pc_track_num_contigs(pc_track *t);
const char *pc_track_contig_name(pc_track *t, int i);
int64_t pc_track_contig_length(pc_track *t, int i);
int64_t pc_track_contig_extent(pc_track *t, int i, int strand_slot);
/* get (genome_array.py:1477-1533) for a table of segments in one launch: position i of segment s -- genomic start[s] + i
 * on contig[s] (index into the contig order, -1: unknown) and strand_slot[s] -- goes to
 * host_out[out_off[s] + out_step[s] * i], out_step +1 or -1; a chain is its segments at their spliced offsets (reversed
 * for '-': SegmentChain.get_counts, roitools.pyx:3259-3271).  Positions below 0, beyond the extent or on an unknown contig
 * are 0.  normalize: 1e6 * v / sum, the reference's order for this class (:1528).  Elements no segment writes are 0. */
int pc_track_gather(pc_track *t, int64_t nseg, const int32_t *contig, const int32_t *strand_slot, const int64_t *start, const int64_t *end,
                    const int64_t *out_off, const int8_t *out_step, int64_t out_elems, int normalize, double *host_out);
/* sum (genome_array.py:1389-1392): a fixed-tree reduction over every cell, the same bits run to run, cached until the
 * next add.  Equal to the reference's for integer values with a total below 2^53; otherwise a reordering of its sum. */
int pc_track_sum(pc_track *t, double *sum);
/* the last add: [0] lines, [1] yielded lines, [2] escaped lines (a token that is not plain: converted on the host),
 * [3] state records, [4] overlapping lines (members of clusters of several lines, applied in file order), [5] lines that
 * reached a contig's length */
int pc_track_stats(pc_track *t, int64_t *out6);
/* milliseconds of the last add on the engine's stream: [0] upload, [1] line starts, [2] classify + state records,
 * [3] fields (the host's conversion of escaped lines included), [4] growth, sort and apply */
int pc_track_timing(pc_track *t, double *ms5);

/* ---- MUTABLE COUNT TRACKS: set, add, multiply, compare and export (revision 16)
 * The reference's MutableAbstractGenomeArray / GenomeArray (genome_array.py:1323-2104) without add_from_bowtie and plot.
 * pc_track_set (__setitem__, :1535-1611): one launch writes every segment of a chain on one contig and strand slot.
 * Position i of segment s takes values[val_off[s] + val_step[s] * i] (val_step +1 / -1; the binding reverses for '-' as
 * the reference does), or `scalar` when values is NULL.  An undeclared contig is born at min_chr_size; a segment whose
 * end reaches the contig's length sets it to max(length, end) + 10000 -- the rule of pc_track_add_text; the cells grow to
 * the furthest end written; the cached sum is dropped.  Every argument is checked before anything changes. */
int pc_track_set(pc_track *t, const char *contig, int strand_slot, int64_t nseg, const int64_t *start, const int64_t *end, const int64_t *val_off,
                 const int8_t *val_step, const double *values, int64_t nvalues, double scalar);
/* apply_operation (:1697-1835): a NEW track on a's engine, a op b, op 0 add / 1 subtract / 2 multiply; a and b are
 * unchanged.  b NULL: a op scalar on every cell up to each contig's length (the result stores that many cells).
 * Otherwise mode_all != 0: the union of the contigs (a's in a's order, then b's remaining ones) at the longer length, zero
 * for what one side lacks; mode_all == 0 ("truncate"): the common contigs at the shorter length.  length_pad is added to
 * every length of the result (zeros; the reference's "same" mode grows its result as it writes it).  The result has
 * nstrands_out strand slots; slot s reads slot_a[s] of a and slot_b[s] of b (-1: the operand has no such strand: zero).
 * One elementwise kernel over the concatenated cells of the result.  b on another engine: PC_ERR_ARG. */
int pc_track_combine(pc_track *a, pc_track *b, double scalar, int op, int mode_all, int64_t length_pad, int nstrands_out, const int32_t *slot_a,
                     const int32_t *slot_b, pc_track **out);
/* __eq__: over npair (contig, strand) pairs -- public contig index and strand slot in a and in b, -1 where the array lacks
 * it -- *equal = 1 when every position is non-zero in both arrays or in neither, and |a - b| <= tol where it is non-zero.
 * A reduction on the device; no cell crosses to the host. */
int pc_track_equal(pc_track *a, pc_track *b, int64_t npair, const int32_t *contig_a, const int32_t *slot_a, const int32_t *contig_b, const int32_t *slot_b,
                   double tol, int *equal);
/* nonzero (:1679-1695): count, exclusive sum and select over the cells; NaN is non-zero, -0.0 is not.
 * pc_track_nonzero_count fills counts[i * nstrands + s] for public contig i and strand slot s and keeps the indices in HBM;
 * pc_track_nonzero_read copies them out, slot after slot in that order (`total`: the sum of the counts). */
int pc_track_nonzero_count(pc_track *t, int64_t *counts);
int pc_track_nonzero_read(pc_track *t, int64_t *out, int64_t total);
/* to_bedgraph (kind 0) / to_variable_step (kind 1) of one strand slot (:1996-2084), everything behind the track line, byte
 * for byte: contigs in the sorted order of their names; bedGraph writes a contig only when its sum is > 0, the leading
 * "chrom\t0\t<first>\t0" line and the runs of equal value between the first and the last non-zero cell; variableStep
 * writes every contig's header and a line per non-zero cell.  Values print as Python's repr(float): integers below 10^16,
 * nan and +-inf by the format kernel, every other value listed for the host (csrc/track_host.h: float_repr) and copied
 * in.  pc_track_export builds the text in HBM and reports its size; pc_track_export_read copies it out (through the
 * transfer ring when it is large) and frees it. */
int pc_track_export(pc_track *t, int kind, int strand_slot, int64_t *bytes);
int pc_track_export_read(pc_track *t, void *dst, int64_t bytes);
/* the last export: [0] lines, [1] runs (bedGraph) or non-zero cells (variableStep), [2] values listed for the host, [3] bytes */
int pc_track_export_stats(pc_track *t, int64_t *out4);
/* milliseconds of the last export: [0] slot sums, [1] run heads + select, [2] listed values (the host's repr included),
 * [3] line lengths + offsets, [4] format, [5] read-back (host clock) */
int pc_track_export_timing(pc_track *t, double *ms6);
/* [0] cells one workgroup covers in the run-head kernel, [1] lines one workgroup formats */
int pc_track_export_geometry(int *out2);

/* ---- A COUNTED PLAN AS TEXT, AND INTO A TRACK (revision 17)
 * BAMGenomeArray.to_bedgraph / to_variable_step (genome_array.py:990-1111) and to_genome_array (:965-988) without the
 * counts leaving HBM.  The source is a counted plan (pc_count) of ONE row per position without summed slices, at either
 * output dtype; PC_ERR_STATE before pc_count, PC_ERR_ARG for any other plan or a plan of another engine.
 *
 * pc_counts_export_batches: the contigs of one export (lengths in the order of the text) are counted in batches of at
 * most `budget` output elements (<= 0: 2^27, 1 GiB of counts); a contig longer than the budget gets a batch alone;
 * batch_of[k]: the batch of contig k.  The layout indexes export elements with 32 bits; the scans of pc_counts_export
 * count in int, so a contig of 2^31 - 1 positions or more is refused here (PC_ERR_ARG).  The number of contigs in a
 * batch is bounded by the 2^31 bytes of their names only.
 *
 * pc_counts_export: the text of `nrange` ranges, everything behind the track line of this batch.  Range r is len[r]
 * consecutive output elements from elem_off[r]; element j of it is genomic position j of contig names[r].  kind 0
 * (bedGraph): a range of length <= 0 writes nothing; the others are cut into windows of `period` positions (>= 1) and
 * every maximal run of equal value inside a window whose value is > 0 writes "chrom\tstart\tend\tvalue\n" -- no leading
 * line, a run across a window border is two lines.  kind 1 (variableStep): "variableStep chrom=<name> span=1\n" for every
 * range, then "<pos + 1>\tvalue\n" for every non-zero element.  An int64 count prints as its decimal digits, a float64
 * value as Python's repr(float): integers below 10^16 by the format kernel, every other finite value listed for the host
 * (csrc/track_host.h: float_repr) and copied in.  Phases, all on the engine's stream: run-head flags over the 8-byte
 * output (typed by the dtype); exclusive sum, select into the run table and the runs in front of every range; bedGraph: a
 * second flag, sum and select pass keeps the runs whose value is > 0 as the lines; float64: the listed values; a byte
 * length per line and their exclusive sum; the format kernel.  pc_counts_export_read copies the text out (through the
 * transfer ring when it is large) and frees it.  One batch holds fewer than 2^31 elements and lines. */
int pc_counts_export_batches(int64_t n, const int64_t *len, int64_t budget, int32_t *batch_of, int *nbatch);
int pc_counts_export(pc_engine *e, pc_plan *p, int kind, int64_t period, int nrange, const char *const *names, const int64_t *elem_off,
                     const int64_t *len, int64_t *bytes);
int pc_counts_export_read(pc_engine *e, void *dst, int64_t bytes);
/* the last pc_counts_export: [0] lines, [1] runs of any value (bedGraph) or non-zero elements (variableStep), [2] values
 * listed for the host, [3] bytes */
int pc_counts_export_stats(pc_engine *e, int64_t *out4);
/* milliseconds of the last pc_counts_export: [0] run heads, [1] sums and selects (run table, lines), [2] listed values
 * (the host's repr included), [3] line lengths + offsets, [4] format, [5] read-back (host clock) */
int pc_counts_export_timing(pc_engine *e, double *ms6);
/* Cells [start, start + n) of (contig, strand_slot) = (double) of output elements [elem_off, elem_off + n) of a counted
 * plan on the track's engine: the birth, growth, extent and cached-sum rules of pc_track_set for one segment; k_track_set
 * reading HBM instead of an uploaded vector (int64 -> double is exact for every count a file can hold).  Every argument
 * is checked before anything changes. */
int pc_track_set_counts(pc_track *t, const char *contig, int strand_slot, int64_t start, pc_plan *p, int64_t elem_off, int64_t n);

/* ---- bigWig FILES (revision 18)
 * The reference's BigWigReader / BigWigGenomeArray (plastid/readers/bigwig.pyx:109-412, genome_array.py:1114-1320) over
 * Kent's readers (kent/src/lib/bbiRead.c, bwgQuery.c:155-285, bwgValsOnChrom.c:36-214).  The container -- the 64-byte
 * header, the chromosome B+ tree, the unzoomed R-tree -- is walked by the host (csrc/bigwig_host.h); the data blocks,
 * independent zlib streams of a few KiB each (uncompressBufSize > 0) or stored sections, are inflated, checked and
 * decoded in HBM (csrc/bigwig_kernels.hip.h).  Zoom levels, the total summary and byte-swapped files are not read.
 * A file that is refused is PC_ERR_ARG with "<path>: bigWig: <what>" -- the file's structure first, then the lowest
 * (block, item) -- and changes nothing: a wrong magic (bigBed's named), a byte-swapped file, a version below 3, tree
 * nodes or blocks outside the file, a zlib header that is not CM = 8 without FDICT, a block above 2^28 bytes or an
 * uncompressBufSize above 2^30 (the inflate kernel counts bits and bytes in 32 bits), a section of unknown type, a section
 * whose 24 + itemCount x itemsize is not the block's inflated length, an item with end <= start, a chromId outside the
 * tree, an end beyond its contig's size, a failed Adler-32, a DEFLATE error.
 *
 * pc_bigwig_info (host only, no engine): `path`, or `image` / `size` when image is not NULL (path then only names the file in
 * messages).  out5: [0] contigs, [1] data blocks, [2] uncompressBufSize, [3] version, [4] bytes of the names with their
 * NULs.  names / sizes (optional: filled when max_contigs and names_bytes suffice): the contigs in the order of
 * bbiChromList (a depth-first walk of the tree), names NUL-terminated one behind the other.
 * pc_bigwig_blocks: the block table in index order -- file offset and bytes of every block; nblocks must be out5[1]. */
int pc_bigwig_info(const char *path, const void *image, int64_t size, int64_t *out5, int max_contigs, char *names, int64_t names_bytes, int64_t *sizes);
int pc_bigwig_blocks(const char *path, const void *image, int64_t size, int64_t nblocks, int64_t *off, int64_t *bytes);
/* n independent zlib streams (RFC 1950), stream k the len[k] bytes at image + off[k], each inflated by one wave of the
 * zlib instantiation of the BGZF inflate kernel into at most `capacity` bytes and checked against its Adler-32.
 * out: n x capacity bytes, stream k at out + k x capacity; out_len[k]: the bytes it gave (0 with a status); status[k]: 0,
 * or 1 - 9 and 11 a DEFLATE error (csrc/bam_kernels.hip.h: 7 more than `capacity` bytes, 11 the stream does not end in the
 * byte before its trailer), 10 the Adler-32, 12 a header that is not CM = 8 without FDICT.  A refused stream is a status,
 * not an error of the call.  capacity <= 2^30, len[k] <= 2^28. */
int pc_inflate_zlib(pc_engine *e, const void *image, int64_t n, const int64_t *off, const int64_t *len, int64_t capacity, void *out, int64_t *out_len,
                    int32_t *status);
/* The items of a bigWig file ASSIGNED to cells [start, end) of one strand slot, in file order: where items overlap the
 * last one wins, as in both Kent readers (Kent's writer refuses such files; the semantic is the contract all the same).
 * Contigs the track does not hold are declared from the chromosome tree at their sizes, in bbiChromList's order, and do
 * not grow; cells are stored up to the furthest end written.  Meant for a slot that holds zeros (a BigWigReader's track):
 * on a slot that holds values the items overwrite them.  The bytes that hold the blocks cross PCIe once (through the
 * page-locked halves when they are large); the blocks inflate into slots of uncompressBufSize bytes rounded to 16. */
int pc_track_add_bigwig(pc_track *t, const void *image, int64_t size, const char *name, int strand_slot);
int pc_track_add_bigwig_path(pc_track *t, const char *path, int strand_slot);
/* the last pc_track_add_bigwig: [0] blocks, [1] blocks inflated on the GPU, [2] items of bedGraph, [3] variableStep and
 * [4] fixedStep sections, [5] overlapping items (members of clusters of several items, applied in file order), [6] bytes
 * uploaded, [7] bytes inflated */
int pc_track_bigwig_stats(pc_track *t, int64_t *out8);
/* milliseconds of the last pc_track_add_bigwig on the engine's stream: [0] upload, [1] inflate + Adler-32, [2] sections +
 * items, [3] contigs, storage, sort and apply */
int pc_track_bigwig_timing(pc_track *t, double *ms4);
/* BigWigGenomeArray.get (genome_array.py:1171-1217) over the ntrack readers of one strand, all on one engine: element by
 * element 0.0 + r1 + r2 + ..., in the order of `tracks`.  The segment table is pc_track_gather's, but contig and
 * strand_slot hold ntrack rows of nseg entries: row k is the segments' contig index and strand slot IN track k (-1: the
 * track lacks it: zeros).  One launch per track, each adding onto the output in HBM: every track cuts its own items (its
 * contigs and extents are its own), and the order of the launches is the order of the sum.  normalize 0: none; 1:
 * v / sum * 1e6 (BigWigGenomeArray, :1212); 2: 1e6 * v / sum (GenomeArray, :1528); `sum` is the caller's. */
int pc_track_gather_sum(int ntrack, pc_track *const *tracks, int64_t nseg, const int32_t *contig, const int32_t *strand_slot, const int64_t *start,
                        const int64_t *end, const int64_t *out_off, const int8_t *out_step, int64_t out_elems, int normalize, double sum, double *host_out);
/* The fixed-tree sum over nrange ranges of cells: positions [start[r], end[r]) of public contig contig[r] on strand_slot[r]
 * (beyond the extent: zeros; -1: nothing).  The order of the additions depends on the ranges alone. */
int pc_track_sum_ranges(pc_track *t, int64_t nrange, const int32_t *contig, const int32_t *strand_slot, const int64_t *start, const int64_t *end, double *sum);

/* The twin of pc_inflate_zlib (revision 19): n independent inputs, input k the len[k] <= 24 600 bytes at image + off[k], each
 * encoded by one workgroup of k_zlib_deflate (csrc/deflate_kernels.hip.h) into one zlib stream (RFC 1950: 78 01, one
 * DEFLATE block -- LZ77 matches of 4 .. 258 bytes under the fixed Huffman codes, or a stored block when that is not
 * smaller -- and the Adler-32).  The bytes are those of the host model (csrc/deflate_host.h, pb_deflate_zlib of the host
 * library), a pure function of the input.  out: the streams back to back, stream k the out_len[k] <= len[k] + 11 bytes at
 * out + out_off[k].  PC_ERR_ARG: an input above 24 600 bytes, out_capacity below the sum of len[k] + 11. */
int pc_deflate_zlib(pc_engine *e, const void *image, int64_t n, const int64_t *off, const int64_t *len, void *out, int64_t out_capacity, int64_t *out_off,
                    int64_t *out_len);
/* pc_deflate_zlib with a choice of codes (revision 20).  mode 1: the fixed Huffman codes, pc_deflate_zlib itself.  mode 2:
 * dynamic codes -- the same matches and the same tokens, under Huffman codes built for the block (lengths within 15, 15
 * and 7, every code complete, the block header by zlib's run-length rule; csrc/deflate_host.h states every step).  The
 * body is the dynamic block iff it takes fewer bytes than the fixed block and than the stored block, else what mode 1
 * gives: a mode-2 stream is never longer than the mode-1 stream.  The bytes are those of pb_deflate_zlib_mode of the
 * host library.  PC_ERR_ARG as pc_deflate_zlib, and for any other mode. */
int pc_deflate_zlib_mode(pc_engine *e, const void *image, int64_t n, const int64_t *off, const int64_t *len, void *out, int64_t out_capacity, int64_t *out_off,
                         int64_t *out_len, int mode);
/* The code lengths the encoder gives n symbols (2 .. 286) of the counts counts[0, n) under a length limit (1 .. 15, 2^limit
 * >= n), on the device (k_huffman_lengths: the rank sort and the length function k_zlib_deflate compiles): with fewer
 * than two counts above 0 the lowest-numbered zeros count 1; Huffman's merge over the order (count, symbol), a leaf before
 * an internal node of equal weight; depths above the limit repaired as csrc/deflate_host.h states; lengths handed out
 * longest first in that order.  The code is complete (the Kraft sum is 1); unused symbols get 0.  pb_huffman_lengths of
 * the host library is the model.  PC_ERR_ARG: n or limit out of range, counts that add up to 2^32 or more. */
int pc_huffman_lengths(pc_engine *e, const uint32_t *counts, int64_t n, int limit, uint8_t *lengths_out);

/* One strand slot of a track as a bigWig file (revision 19; csrc/bigwig_writer.hip.h, the container: csrc/bigwig_write_host.h).
 * A cell is written iff its value != 0.0 (NaN is, -0.0 is not); neighbouring written cells of a contig form one item while
 * their float64 values compare equal; the value is cast to float32 afterwards.  Contigs stand in the sorted order of their
 * names, every contig of the track is in the chromosome tree at max(length, cells stored); every items_per_slot items of
 * a contig make one bedGraph section; block_size is the fan-out of both trees; compress: 1 every section through
 * k_zlib_deflate under the fixed codes, 2 under dynamic codes (pc_deflate_zlib_mode; uncompressBufSize: the largest raw
 * section), 0 stored sections (uncompressBufSize 0); any other value is PC_ERR_ARG.  Little-endian, version 4, no zoom levels
 * (pc_track_export_bigwig_zoom, below, writes them);
 * the total summary stands at offset 64 when the file has items.  Items, sections, summary and blocks are built in HBM;
 * the section table comes back, the host lays out offsets and trees, and the blocks cross PCIe once (through the transfer
 * ring when they are large).  *bytes: the size of the file, which waits on the host for pc_track_export_bigwig_read.
 * PC_ERR_ARG, before anything is built: items_per_slot outside 1 .. 2048, block_size outside 2 .. 65535, a contig of 2^32
 * positions or more, a strand of 2^31 - 1 cells or more (it could hold 2^31 items).  The file is what the host writer
 * (pb_bigwig_write_* of the host library) gives for the same cells, byte for byte, but for the rounding of the
 * summary's two sums, which are added in a fixed tree here and serially there. */
int pc_track_export_bigwig(pc_track *t, int strand_slot, int64_t items_per_slot, int64_t block_size, int compress, int64_t *bytes);
/* The reported length of a contig the track holds becomes `length`: what pc_track_contig_length gives and what a later
 * write grows from.  The cells stay as they are.  For a track filled through pc_track_set_counts over whole contigs, which
 * grows a contig written up to its end by the reference's rule: the exporter of a BAMGenomeArray puts the alignment
 * file's lengths back before it writes the chromosome tree.  PC_ERR_ARG: no such contig. */
int pc_track_set_length(pc_track *t, const char *name, int64_t length);
/* copies the file of the last pc_track_export_bigwig out (`bytes` as it reported) and frees it */
int pc_track_export_bigwig_read(pc_track *t, void *dst, int64_t bytes);
/* the last pc_track_export_bigwig: [0] contigs, [1] items, [2] sections, [3] raw bytes of the sections, [4] bytes of the
 * blocks in the file, [5] sections that fell back to a stored DEFLATE block */
int pc_track_bigwig_export_stats(pc_track *t, int64_t *out6);
/* the last pc_track_export_bigwig: the sections that went out as [0] stored, [1] fixed, [2] dynamic DEFLATE blocks; they
 * add up to the sections when compress was 1 or 2 and are 0 when it was 0 */
int pc_track_bigwig_export_block_types(pc_track *t, int64_t *out3);
/* milliseconds of the last pc_track_export_bigwig: [0] item heads, their sum and the items per contig, [1] items, section
 * headers and the summary, [2] deflate and Adler-32, [3] sizes and compaction (on the engine's stream), [4] read-back,
 * [5] host layout (wall clock) */
int pc_track_bigwig_export_timing(pc_track *t, double *ms6);

/* ---- ZOOM LEVELS of a written bigWig file (revision 21; csrc/bigwig_zoom_kernels.hip.h; what a level is:
 * csrc/bigwig_write_host.h, "zoom levels").  pc_track_export_bigwig_zoom is pc_track_export_bigwig with `zoom`: 0 no zoom
 * levels (pc_track_export_bigwig itself: zoomLevels = 0, the same bytes), -1 the automatic first reduction
 * r0 = 4 x max(10, validCount / items) capped at 2^20, or r0 itself, 8 .. 2^24; any other value is PC_ERR_ARG.
 * Reductions are r_k = r0 x 4^k, at most 10 levels, r_k <= 2^30.  Windows lie on a fixed grid -- window w of level k on a
 * contig covers [w r_k, min((w + 1) r_k, size)) -- and not where Kent's writer, whose windows start where the data does,
 * would put them; Kent's readers take either.  Level 0 takes every window's overlap with the ITEMS in their order
 * (validCount, min and max of the float32 values, sum and sum of squares in float64); level k + 1 adds the float64
 * accumulators of its four children in order, the empty ones skipped.  A window with validCount > 0 gives one 32-byte
 * record (chromId, start, end, validCount u32; minVal, maxVal, sumData, sumSquares f32, cast there alone, a NaN as
 * 0x7fc00000).  Level 0 is written whenever the file has items, level k >= 1 iff it has fewer records than level k - 1;
 * a file without items has no levels and is the zoom = 0 file.  Every min(items_per_slot, 768) records of a contig make
 * one block, stored or encoded as the sections are; uncompressBufSize is the largest raw section or zoom block.  The
 * zoom headers (24 bytes each) stand at offset 64, the total summary behind them; behind the unzoomed R-tree every
 * level has its u32 record count, its blocks and its R-tree.  The accumulators are dense per-window columns in HBM:
 * 28 bytes per level-0 window and a third of that for the levels above; the record counts per (level, contig) and the
 * block tables are all that visits the host.  PC_ERR_ARG also: a grid of 2^31 - 2 windows or more over the levels.
 * The file is what the host writer (pb_bigwig_write_open_zoom of the host library) gives for the same cells, byte for
 * byte (but for the total summary's two sums, as above). */
int pc_track_export_bigwig_zoom(pc_track *t, int strand_slot, int64_t items_per_slot, int64_t block_size, int compress, int64_t zoom, int64_t *bytes);
/* the zoom levels of the last export: *levels (0 .. 10), and per level k at out50 + 5 k: [0] the reduction, [1] records,
 * [2] blocks, [3] raw bytes of the blocks, [4] their bytes in the file.  out50: room for 50 values. */
int pc_track_bigwig_export_zoom_stats(pc_track *t, int64_t *levels, int64_t *out50);
/* milliseconds of the zoom levels of the last export on the engine's stream: [0] level 0 from the items, [1] the levels
 * above, [2] the flags' sum, the record counts' read-back, records and block table, [3] deflate and compaction of the
 * zoom blocks.  All 0 when no level was written.  (pc_track_bigwig_export_timing keeps its six laps: the zoom levels
 * run between its [3] and its [4].) */
int pc_track_bigwig_export_zoom_timing(pc_track *t, double *ms4);

/* ---- BINNED SUMMARIES of a bigWig file (revision 23; csrc/bigwig_summary.hip.h, the kernels: csrc/bigwig_summary_kernels.hip.h,
 * the rules and the model: csrc/bigwig_summary_host.h).  What the summary reader of Kent's library gives
 * (bigWigSummaryArray: bbiRead.c:18-40 and :405-760, bwgQuery.c:155-287), bit for bit: a query (contig, start, end) is cut
 * into n_bins equal bins and answered from the zoom level with the greatest reduction <= ((end - start) / n_bins) / 2, from
 * the items when that is <= 1 or no level is that fine.
 * pc_bigwig_summary_open / _open_path parse the header, the chromosome tree and the zoom headers on the host and upload
 * nothing (open copies the image; open_path maps the file for the life of the handle).  A TABLE -- the records of one
 * level, or the items -- is loaded at the first query that selects it: the host walks its R-tree, the blocks go up as
 * they are, are inflated and Adler-checked by the kernels of the import, and land in HBM as records in file order (32
 * bytes per zoom record, 16 per item), where they stay.  One kernel checks that a table's starts and ends do not decrease
 * within a contig and that a contig's records stand together -- true of every file Kent's writer and ours produce -- and
 * gives the record range of every contig; a table that fails makes the queries that select it PC_ERR_ARG with "<path>:
 * bigWig: summarize needs records in coordinate order" (Kent walks a list where this library searches).  A handle goes
 * with its engine (pc_destroy) unless closed before. */
typedef struct pc_bigwig_summary pc_bigwig_summary;
int pc_bigwig_summary_open(pc_engine *e, const void *image, int64_t size, const char *name, pc_bigwig_summary **out);
int pc_bigwig_summary_open_path(pc_engine *e, const char *path, pc_bigwig_summary **out);
int pc_bigwig_summary_close(pc_bigwig_summary *s);
/* nq queries of n_bins bins each: contig[q] the contig's place in the chromosome list (pc_bigwig_info's order; -1: the
 * file lacks it: no data), 0 <= start[q] < end[q] < 2^31, 1 <= n_bins < 2^31, nq x n_bins < 2^31.  The queries are grouped
 * by table on the host and k_bbi_summarize runs once per table in use, one lane per (query, bin).  out5: five columns of
 * nq x n_bins doubles -- validCount, min, max, sum, sum of squares (Kent's bbiSummaryElement), element q x n_bins + bin of
 * each; a bin without data is all zeros.  The buffer is read back once.  A lane walks its bin serially, because the sums
 * are exact in their order: bins of millions of items in a file without zoom levels are slow by construction. */
int pc_bigwig_summary_query(pc_bigwig_summary *s, int64_t nq, const int32_t *contig, const int64_t *start, const int64_t *end, int64_t n_bins, double *out5);
/* out4: [0] tables the file has (the items and its levels), [1] tables loaded, [2] bytes uploaded, [3] bytes inflated; per
 * table k (0: the items, 1 + j: level j; at most max_tables of them) out3 + 3 k: [0] the reduction (0: the items), [1]
 * records (-1: not loaded), [2] queries answered */
int pc_bigwig_summary_stats(pc_bigwig_summary *s, int64_t *out4, int max_tables, int64_t *out3);
/* milliseconds of the last pc_bigwig_summary_query on the engine's stream: [0] upload, [1] inflate + Adler-32, [2] records /
 * items and the order check (0 - 2 are 0 when no table was loaded), [3] k_bbi_summarize, [4] read-back */
int pc_bigwig_summary_timing(pc_bigwig_summary *s, double *ms5);

#ifdef __cplusplus
}
#endif
#endif /* PLASTID_COUNTS_H */
