// Count tracks on the GPU, host side: the pc_track_* entry points of include/plastid_counts.h.  A pc_track is the
// reference's GenomeArray (plastid/genomics/genome_array.py:1323-1533) as a read-and-count object: float64 cells per
// (contig, strand slot) in one block of HBM, filled by pc_track_add_text / _path (add_from_wiggle, :1978-1994) and read by
// pc_track_gather.  What decides the contigs, their lengths and every cell address is the track's ContigTable
// (track_table.h, HIP-free and CPU-tested); the entry points here check their arguments, ask the table for a layout and
// queue the kernels.  One import is a TrackImport taken through its phases (track_add_impl): upload and line starts
// (both shared with SAM text), classify + state records, fields (+ the host's conversion of the escaped lines), births,
// growth and storage, sort + apply.  The host looks at the state lines, the escaped lines and the growth lines only.
// Revision 16 makes it the reference's mutable GenomeArray (:1535-2104): pc_track_set (one launch per segment or chain),
// pc_track_combine (a new track from a op b or a op scalar), pc_track_equal, pc_track_nonzero_count / _read and
// pc_track_export / _read: the bedGraph / variableStep text of a strand built in HBM by the phases of a TrackExport and
// read back once; of an export the host sees the per-slot sums and the values that are not plain.
// Revision 17: a counted plan as the source.  pc_counts_export / _read write the text BAMGenomeArray gives of its count
// vectors (genome_array.py:990-1111; window borders, runs whose value is > 0, int64 or float64 values) from the plan's
// output in HBM, by the phases of a CountsExport; pc_track_set_counts is pc_track_set for one segment reading that output.
// Part of the one translation unit of plastid_counts.hip (behind sam_decoder.hip.h; the plumbing is device_util.hip.h).
#include "track_kernels.hip.h"

struct pc_track {
    pc_engine *e = nullptr;
    pctrack::ContigTable tab;               // contigs, public order, lengths, the cells of every slot
    DevBuf<double> cells;
    bool sum_valid = false;
    double sum = 0.0;
    int64_t stats[6] = {0, 0, 0, 0, 0, 0};  // lines, yielded, escaped, state records, overlapping lines, growth lines
    double ms[5] = {0, 0, 0, 0, 0};         // upload | line starts | classify + state records | fields | growth + sort + apply
    // the last pc_track_add_bigwig (bigwig_decoder.hip.h)
    int64_t bw_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // blocks, compressed blocks, items by type (3), overlapping items, bytes in, bytes inflated
    double bw_ms[4] = {0, 0, 0, 0};                   // upload | inflate + adler | sections + items | sort + apply
    // the last pc_track_export: its text waits in HBM for pc_track_export_read
    DevBuf<uint8_t> ex_text;
    int64_t ex_bytes = -1;
    int64_t ex_stats[4] = {0, 0, 0, 0};     // lines, runs / non-zero cells, values listed for the host, bytes
    double ex_ms[6] = {0, 0, 0, 0, 0, 0};   // slot sums | run heads + select | listed values | lengths + offsets | format | read-back
    // the last pc_track_nonzero_count: the indices wait in HBM for pc_track_nonzero_read
    DevBuf<int64_t> nz;
    int64_t nz_total = -1;
    pctrack::NzShares nz_shares;            // per slot: its share of nz
    // the last pc_track_export_bigwig (bigwig_writer.hip.h): the file's image waits for pc_track_export_bigwig_read
    std::vector<uint8_t> bwx_image;
    int64_t bwx_bytes = -1;
    int64_t bwx_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // contigs, items, sections, raw bytes, block bytes, sections as stored, fixed, dynamic blocks
    double bwx_ms[6] = {0, 0, 0, 0, 0, 0};       // runs + items | sections + summary | deflate + adler | sizes + compaction | read-back | host layout
    int bwz_levels = 0;                          // the zoom levels of that file; per level: reduction, records, blocks, raw bytes, file bytes
    int64_t bwz_stats[10][5] = {};
    double bwz_ms[4] = {0, 0, 0, 0};             // level 0 | levels above | flags' sum + records + block table | deflate + compaction
};

// an engine that is destroyed takes its tracks with it (pc_destroy): their cells come from its pool
static void destroy_tracks_of(pc_engine *e) {
    for (pc_track *t : e->tracks) delete t;
    e->tracks.clear();
}

namespace {

namespace tk = pctrack;

// text bounds and data index of listed lines, for the host
struct TrackLineInfo { uint64_t b, e; uint32_t line, data_index; };
__global__ __launch_bounds__(256) void k_track_line_info(const uint32_t *__restrict__ lines, uint32_t n, const uint64_t *__restrict__ line_start, uint64_t text_len,
                                                         const uint32_t *__restrict__ data_index, TrackLineInfo *__restrict__ out) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    TrackLineInfo o;
    o.line = lines[k];
    tk::line_bounds(line_start, text_len, (int64_t)o.line, o.b, o.e);
    o.data_index = data_index[o.line];
    out[k] = o;
}
// contig and end of the growth lines, for the host's fold
__global__ __launch_bounds__(256) void k_track_growth_info(const uint32_t *__restrict__ lines, uint32_t n, const tk::LineRec *__restrict__ recs,
                                                           const int32_t *__restrict__ contig_of, tk::GrowthLine *__restrict__ out) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    tk::GrowthLine o;
    o.line = lines[k]; o.stop = recs[o.line].stop; o.contig = contig_of[o.line];
    out[k] = o;
}

inline unsigned grid256(int64_t n) { return (unsigned)((n + 255) / 256); }

// What the phases of one import share.  The host vectors that feed an upload live here, behind the stream's last use.
struct TrackImport {
    pc_track *t;
    const uint8_t *text;
    int64_t size;
    int strand;
    BamDecode d;
    hipStream_t st;
    LapEvents<6> ev;                   // reserved | uploaded | line starts | states | fields | applied
    SamLines ln;
    int64_t n = 0;                     // lines
    unsigned g = 0;
    int ncontig = 0;
    tk::TrackCounters cnt;
    unsigned long long host_err = tk::kNoDefect;
    std::vector<TrackLineInfo> info;
    std::vector<tk::StateRec> recs;
    std::vector<tk::LineRec> patch;
    std::vector<int32_t> patch_contig;
    std::vector<uint32_t> lines, first_line;
    std::vector<int64_t> len0, off;
    std::vector<unsigned long long> furthest;
    DevBuf<uint8_t> d_cls, d_tmp;
    DevBuf<int32_t> d_sig, d_prev_sig, d_contig_of, d_head, d_patch_contig;
    DevBuf<uint32_t> d_is_data, d_data_index, d_list, d_idx, d_idx2, d_first_line, d_long;
    DevBuf<uint64_t> d_key, d_key2, d_end_key, d_prev_end, d_multi, d_multi2;
    DevBuf<tk::TrackCounters> d_cnt;
    DevBuf<tk::StateRec> d_recs;
    DevBuf<tk::LineRec> d_line, d_patch;
    DevBuf<int64_t> d_len0, d_off;
    DevBuf<unsigned long long> d_furthest;
    DevBuf<tk::GrowthLine> d_growth;
    TrackImport(pc_track *t_, const uint8_t *text_, int64_t size_, const char *name, int strand_)
        : t(t_), text(text_), size(size_), strand(strand_), d{t_->e, t_->e->stream, name ? name : "<memory>", BamKnobs()}, st(d.st) {}
    uint64_t text_len() const { return (uint64_t)size; }
    void note_defect(uint32_t line, int err) { if (err != tk::kTrkOk) host_err = std::min(host_err, ((unsigned long long)line << 8) | (unsigned long long)err); }
    int read_counters() {
        HIP_TRY(hipMemcpyAsync(&cnt, d_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return PC_OK;
    }
};

// the first `count` lines of d_list with their text bounds, sorted by line, into c.info
int fetch_line_info(TrackImport &c, uint32_t count) {
    c.info.resize(count);
    if (!count) return PC_OK;
    DevBuf<TrackLineInfo> d_info;
    DrainOnExit drained{c.st};
    PC_TRY(d_info.reserve(count));
    hipLaunchKernelGGL(k_track_line_info, dim3(grid256(count)), dim3(256), 0, c.st, c.d_list.p, count, c.ln.d_line_start.p, c.text_len(), c.d_data_index.p, d_info.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c.info.data(), d_info.p, (size_t)count * sizeof(TrackLineInfo), hipMemcpyDeviceToHost, c.st));
    HIP_TRY(hipStreamSynchronize(c.st));
    drained.armed = false;
    std::sort(c.info.begin(), c.info.end(), [](const TrackLineInfo &a, const TrackLineInfo &b) { return a.line < b.line; });
    return PC_OK;
}

// Phases 1, 2: the text to HBM, the line starts (sam_decoder.hip.h).
int import_upload_and_lines(TrackImport &c) {
    {
        Upload u;
        Drain drain{c.d.e, true};
        PC_TRY(c.d.d_stream.reserve((size_t)c.size + 64));
        HIP_TRY(hipEventRecord(c.ev[0], c.st));
        PC_TRY(sam_upload(c.d, c.text, c.size, nullptr, u));
        HIP_TRY(hipEventRecord(c.ev[1], c.st));
        PC_TRY(sam_line_starts(c.d, c.size, c.text[c.size - 1] != (uint8_t)'\n', c.ln));
        drain.armed = false;
    }
    HIP_TRY(hipEventRecord(c.ev[2], c.st));
    c.n = c.ln.nrec;
    c.g = grid256(c.n);
    c.t->stats[0] = c.n;
    return PC_OK;
}

// Phase 3: classes, the state lines (parsed here: they name the contigs), the data-line prefix count.
int import_classify_and_states(TrackImport &c) {
    hipStream_t st = c.st;
    const int64_t n = c.n;
    int rc = PC_OK;
    room(rc, c.d_cls, (size_t)n); room(rc, c.d_sig, (size_t)n); room(rc, c.d_prev_sig, (size_t)n); room(rc, c.d_is_data, (size_t)n);
    room(rc, c.d_data_index, (size_t)n); room(rc, c.d_list, (size_t)n); room(rc, c.d_cnt, 1);
    if (rc != PC_OK) return rc;
    memset(&c.cnt, 0, sizeof(c.cnt));
    c.cnt.first_err = tk::kNoDefect;
    HIP_TRY(hipMemcpyAsync(c.d_cnt.p, &c.cnt, sizeof(c.cnt), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(tk::k_track_classify, dim3(c.g), dim3(256), 0, st, c.d.d_stream.p, c.text_len(), c.ln.d_line_start.p, n, c.d_cls.p, c.d_sig.p, c.d_is_data.p);
    HIP_TRY(hipGetLastError());
    const auto last_sig = [&](void *tmp, size_t &b) { return hipcub::DeviceScan::ExclusiveScan(tmp, b, c.d_sig.p, c.d_prev_sig.p, hipcub::Max(), (int32_t)-1, (int)n, st); };
    const auto data_index = [&](void *tmp, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(tmp, b, c.d_is_data.p, c.d_data_index.p, (int)n, st); };
    size_t need = 16, b_sig = 0, b_data = 0;
    PC_TRY(cub_need(need, b_sig, last_sig)); PC_TRY(cub_need(need, b_data, data_index));
    PC_TRY(c.d_tmp.reserve(need));
    PC_TRY(cub_run_sized(c.d_tmp, b_sig, last_sig)); PC_TRY(cub_run_sized(c.d_tmp, b_data, data_index));
    hipLaunchKernelGGL(tk::k_track_states, dim3(c.g), dim3(256), 0, st, c.d.d_stream.p, c.text_len(), c.ln.d_line_start.p, n, c.d_cls.p, c.d_prev_sig.p, c.d_list.p,
                       &c.d_cnt.p->n_state);
    HIP_TRY(hipGetLastError());
    PC_TRY(c.read_counters());
    PC_TRY(fetch_line_info(c, c.cnt.n_state));
    c.recs.resize(c.info.size());
    pc_track *t = c.t;
    for (size_t k = 0; k < c.info.size(); ++k) {
        const TrackLineInfo &i = c.info[k];
        c.note_defect(i.line, tk::parse_state(c.text + i.b, c.text + i.e, (int64_t)i.line, (int64_t)i.data_index,
                                              [t](const std::string &nm) { return t->tab.id_of(nm); }, c.recs[k]));
    }
    t->stats[3] = (int64_t)c.recs.size();
    HIP_TRY(hipEventRecord(c.ev[3], st));
    return PC_OK;
}

// the escaped lines (c.info), converted by the host: c.patch, c.patch_contig
void convert_escaped(TrackImport &c) {
    c.patch.resize(c.info.size()); c.patch_contig.resize(c.info.size());
    for (size_t k = 0; k < c.info.size(); ++k) {
        const TrackLineInfo &i = c.info[k];
        const tk::LineClass lc = tk::classify_line(c.text + i.b, c.text + i.e);
        const int64_t gv = tk::governing(c.recs.data(), (int64_t)c.recs.size(), (int64_t)i.line);
        const tk::LineOut o = tk::line_fields<tk::FastThenFull>(lc, gv >= 0 ? &c.recs[(size_t)gv] : nullptr, (int64_t)i.data_index);
        const int err = o.err == tk::kTrkOk ? tk::check_fields(o) : o.err;
        c.note_defect(i.line, err);
        c.patch[k].start = o.start; c.patch[k].stop = o.stop; c.patch[k].value = o.value;
        c.patch_contig[k] = err == tk::kTrkOk ? o.contig : -1;
    }
}

// Phase 4: the fields of every yielding line; the escaped ones on the host; the lowest defect of the text ends the import.
int import_fields(TrackImport &c) {
    hipStream_t st = c.st;
    pc_track *t = c.t;
    int rc = PC_OK;
    room(rc, c.d_recs, std::max<size_t>(c.recs.size(), 1)); room(rc, c.d_line, (size_t)c.n); room(rc, c.d_contig_of, (size_t)c.n);
    if (rc != PC_OK) return rc;
    if (!c.recs.empty()) HIP_TRY(hipMemcpyAsync(c.d_recs.p, c.recs.data(), c.recs.size() * sizeof(tk::StateRec), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(tk::k_track_fields, dim3(c.g), dim3(256), 0, st, c.d.d_stream.p, c.text_len(), c.ln.d_line_start.p, c.n, c.d_cls.p, c.d_data_index.p, c.d_recs.p,
                       (int64_t)c.recs.size(), c.d_line.p, c.d_contig_of.p, c.d_list.p, c.d_cnt.p);
    HIP_TRY(hipGetLastError());
    PC_TRY(c.read_counters());
    t->stats[1] = c.cnt.n_yield; t->stats[2] = c.cnt.n_escaped;
    if (c.cnt.n_escaped) {
        PC_TRY(fetch_line_info(c, c.cnt.n_escaped));
        convert_escaped(c);
    }
    const unsigned long long first_err = std::min(c.host_err, c.cnt.first_err);
    if (first_err != tk::kNoDefect)
        return fail(PC_ERR_ARG, "%s", tk::track_defect_message(c.d.path.c_str(), (int64_t)(first_err >> 8) + 1, (int)(first_err & 0xffu)).c_str());
    if (c.cnt.n_escaped) {
        // (d_list still holds the escaped lines, in the order fetch_line_info saw them: patch by line)
        c.lines.resize(c.info.size());
        for (size_t k = 0; k < c.info.size(); ++k) c.lines[k] = c.info[k].line;
        PC_TRY(c.d_patch.upload(c.patch, st)); PC_TRY(c.d_patch_contig.upload(c.patch_contig, st)); PC_TRY(c.d_list.upload(c.lines, st));
        hipLaunchKernelGGL(tk::k_track_patch, dim3(grid256((int64_t)c.lines.size())), dim3(256), 0, st, c.d_list.p, c.d_patch.p, c.d_patch_contig.p,
                           (uint32_t)c.lines.size(), c.d_line.p, c.d_contig_of.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    HIP_TRY(hipEventRecord(c.ev[4], st));
    return PC_OK;
}

// Storage of the strand slots as the plan lays them out: a fresh block, zeroed, every slot's cells copied to their new place.
int track_grow_storage(pc_track *t, const tk::StoragePlan &plan, hipStream_t st) {
    if (!plan.grows) return PC_OK;
    DevBuf<double> fresh;
    fresh.pool = &t->e->pool;
    PC_TRY(fresh.reserve((size_t)plan.total));
    HIP_TRY(hipMemsetAsync(fresh.p, 0, (size_t)plan.total * sizeof(double), st));
    for (size_t s = 0; s < t->tab.ext.size(); ++s)
        if (t->tab.ext[s] > 0)
            HIP_TRY(hipMemcpyAsync(fresh.p + plan.off[s], t->cells.p + t->tab.cell_off[s], (size_t)t->tab.ext[s] * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // (the old block goes back to the pool)
    t->cells.swap(fresh);
    t->tab.commit(plan);
    return PC_OK;
}

// Phase 5: per contig the first yielding line and the furthest end, the sort keys; births, growth, storage.
int import_births_growth_storage(TrackImport &c) {
    hipStream_t st = c.st;
    pc_track *t = c.t;
    c.ncontig = (int)t->tab.names.size();
    if (c.ncontig >= (1 << 22)) return fail(PC_ERR_ARG, "%s: more than 2^22 contigs", c.d.path.c_str());
    if (c.ncontig == 0) return PC_OK;
    c.furthest.assign((size_t)c.ncontig, 0ull);
    c.first_line.assign((size_t)c.ncontig, tk::kNoLine);
    c.len0 = t->tab.lengths_before();
    int rc = PC_OK;
    room(rc, c.d_key, (size_t)c.n); room(rc, c.d_idx, (size_t)c.n); room(rc, c.d_key2, (size_t)c.n); room(rc, c.d_idx2, (size_t)c.n);
    if (rc != PC_OK) return rc;
    PC_TRY(c.d_len0.upload(c.len0, st)); PC_TRY(c.d_furthest.upload(c.furthest, st)); PC_TRY(c.d_first_line.upload(c.first_line, st));
    hipLaunchKernelGGL(tk::k_track_keys, dim3(c.g), dim3(256), 0, st, c.d_line.p, c.d_contig_of.p, c.d_cls.p, c.n, c.d_len0.p, c.ncontig, c.d_furthest.p, c.d_first_line.p,
                       c.d_list.p, c.d_key.p, c.d_idx.p, c.d_cnt.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c.furthest.data(), c.d_furthest.p, (size_t)c.ncontig * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c.first_line.data(), c.d_first_line.p, (size_t)c.ncontig * 4, hipMemcpyDeviceToHost, st));
    PC_TRY(c.read_counters());
    for (int32_t id : t->tab.births(c.first_line)) t->tab.bear(id);
    t->stats[5] = c.cnt.n_growth;
    if (c.cnt.n_growth) {
        std::vector<tk::GrowthLine> gr(c.cnt.n_growth);
        PC_TRY(c.d_growth.reserve(c.cnt.n_growth));
        hipLaunchKernelGGL(k_track_growth_info, dim3(grid256(c.cnt.n_growth)), dim3(256), 0, st, c.d_list.p, c.cnt.n_growth, c.d_line.p, c.d_contig_of.p, c.d_growth.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(gr.data(), c.d_growth.p, gr.size() * sizeof(tk::GrowthLine), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        t->tab.fold_growth(gr);
    }
    return track_grow_storage(t, t->tab.plan_storage(c.strand, c.furthest), st);
}

// Phase 6: sort by (contig, start), clusters, fills.  kAssign: the lines write their values (bigwig_decoder.hip.h).
template <bool kAssign = false> int import_sort_and_apply(TrackImport &c) {
    hipStream_t st = c.st;
    pc_track *t = c.t;
    const int64_t n = c.n, nv = c.ncontig > 0 ? (int64_t)c.cnt.n_valid : 0;
    if (nv == 0) return PC_OK;
    c.off = t->tab.strand_offsets(c.strand);
    PC_TRY(c.d_off.upload(c.off, st));
    int rc = PC_OK;
    room(rc, c.d_end_key, (size_t)nv); room(rc, c.d_prev_end, (size_t)nv); room(rc, c.d_head, (size_t)nv); room(rc, c.d_long, (size_t)nv);
    room(rc, c.d_multi, (size_t)nv); room(rc, c.d_multi2, (size_t)nv);
    if (rc != PC_OK) return rc;
    int64_t nm = nv;   // (the ordered pass sorts the lines of the larger clusters: at most nv, known behind k_track_fill_short)
    const auto sort_lines = [&](void *tmp, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(tmp, b, c.d_key.p, c.d_key2.p, c.d_idx.p, c.d_idx2.p, (int)n, 0, 64, st); };
    const auto prev_end = [&](void *tmp, size_t &b) { return hipcub::DeviceScan::ExclusiveScan(tmp, b, c.d_end_key.p, c.d_prev_end.p, hipcub::Max(), (uint64_t)0, (int)nv, st); };
    const auto heads = [&](void *tmp, size_t &b) { return hipcub::DeviceScan::InclusiveScan(tmp, b, c.d_head.p, c.d_head.p, hipcub::Max(), (int)nv, st); };
    const auto sort_multi = [&](void *tmp, size_t &b) { return hipcub::DeviceRadixSort::SortKeys(tmp, b, c.d_multi.p, c.d_multi2.p, (int)nm, 0, 64, st); };
    size_t need = 16, b_sort = 0, b_prev = 0, b_heads = 0, b_multi = 0;
    PC_TRY(cub_need(need, b_sort, sort_lines)); PC_TRY(cub_need(need, b_prev, prev_end)); PC_TRY(cub_need(need, b_heads, heads));
    PC_TRY(cub_need(need, b_multi, sort_multi));
    PC_TRY(c.d_tmp.reserve(need));
    PC_TRY(cub_run_sized(c.d_tmp, b_sort, sort_lines));
    const unsigned gv = grid256(nv);
    hipLaunchKernelGGL(tk::k_track_end_keys, dim3(gv), dim3(256), 0, st, c.d_key2.p, c.d_idx2.p, c.d_line.p, nv, c.d_end_key.p);
    HIP_TRY(hipGetLastError());
    PC_TRY(cub_run_sized(c.d_tmp, b_prev, prev_end));
    hipLaunchKernelGGL(tk::k_track_clusters, dim3(gv), dim3(256), 0, st, c.d_key2.p, c.d_prev_end.p, nv, c.d_head.p);
    HIP_TRY(hipGetLastError());
    PC_TRY(cub_run_sized(c.d_tmp, b_heads, heads));
    hipLaunchKernelGGL(tk::k_track_fill_short<kAssign>, dim3(gv), dim3(256), 0, st, c.d_idx2.p, c.d_head.p, nv, c.d_line.p, c.d_contig_of.p, c.d_off.p, t->cells.p, c.d_long.p,
                       c.d_multi.p, c.d_cnt.p);
    HIP_TRY(hipGetLastError());
    PC_TRY(c.read_counters());
    t->stats[4] = c.cnt.n_multi;
    if (c.cnt.n_long) {
        hipLaunchKernelGGL(tk::k_track_fill<kAssign>, dim3(c.cnt.n_long), dim3(256), 0, st, c.d_long.p, c.d_line.p, c.d_contig_of.p, c.d_off.p, t->cells.p);
        HIP_TRY(hipGetLastError());
    }
    if (c.cnt.n_multi) {
        nm = c.cnt.n_multi;
        PC_TRY(cub_run_sized(c.d_tmp, b_multi, sort_multi));
        hipLaunchKernelGGL(tk::k_track_fill_ordered<kAssign>, dim3(c.cnt.n_multi), dim3(256), 0, st, c.d_multi2.p, c.cnt.n_multi, c.d_line.p, c.d_contig_of.p, c.d_off.p, t->cells.p);
        HIP_TRY(hipGetLastError());
    }
    return PC_OK;
}

int track_add_impl(pc_track *t, const void *image, int64_t size, const char *name, int strand) {
    if (!t || size < 0 || (size > 0 && !image)) return fail(PC_ERR_ARG, "pc_track_add_text: bad arguments");
    if (strand < 0 || strand >= t->tab.nstrands) return fail(PC_ERR_ARG, "pc_track_add_text: strand slot %d of %d", strand, t->tab.nstrands);
    HIP_TRY(hipSetDevice(t->e->device));
    PoolScope pool_scope(&t->e->pool);
    TrackImport c(t, (const uint8_t *)image, size, name, strand);
    for (auto &x : t->stats) x = 0;
    for (auto &x : t->ms) x = 0.0;
    if (size == 0) return PC_OK;
    PC_TRY(c.ev.create());
    PC_TRY(import_upload_and_lines(c));
    if (c.n == 0) return PC_OK;
    DrainOnExit drained{c.st};
    PC_TRY(import_classify_and_states(c));
    PC_TRY(import_fields(c));
    PC_TRY(import_births_growth_storage(c));
    PC_TRY(import_sort_and_apply(c));
    t->sum_valid = false;
    HIP_TRY(hipEventRecord(c.ev[5], c.st));
    HIP_TRY(hipStreamSynchronize(c.st));
    drained.armed = false;
    c.ev.laps(t->ms, 5);
    return PC_OK;
}

// ---------------------------------------------------------------- export

// What the phases of one export share.
struct TrackExport {
    pc_track *t;
    int kind, strand;
    hipStream_t st;
    LapEvents<6> ev;                   // start | slot sums | run table | listed values | lengths + offsets | formatted
    tk::ExportSlots slots;             // the strand's contigs in the order of the text
    std::vector<tk::SlotStat> stat;
    tk::ExportRanges xr;
    int K = 0;                         // written contigs
    int64_t R = 0, nlines = 0, total = 0;   // runs, lines, bytes
    uint32_t n_listed = 0;
    std::vector<uint8_t> strs, lens;
    tk::ExportView view;
    DevBuf<tk::SlotCells> d_slots;
    DevBuf<tk::SlotStat> d_stat;
    DevBuf<double> d_partial, d_listed_val;
    DevBuf<tk::ExRange> d_ranges;
    DevBuf<uint32_t> d_flags, d_idx, d_run_e, d_listed_slot, d_n_listed;
    DevBuf<uint8_t> d_tmp, d_names, d_strs, d_lens;
    DevBuf<int64_t> d_len, d_off;
};

// The listed values of an export come to the host, are formatted by float_repr and go back as text: kReprMax bytes apart
// in strs, their lengths in lens (both at least one entry long).
int listed_values_as_text(hipStream_t st, uint32_t n_listed, DevBuf<double> &d_listed_val, std::vector<uint8_t> &strs, std::vector<uint8_t> &lens,
                          DevBuf<uint8_t> &d_strs, DevBuf<uint8_t> &d_lens) {
    strs.assign((size_t)std::max<uint32_t>(n_listed, 1) * tk::kReprMax, 0); lens.assign((size_t)std::max<uint32_t>(n_listed, 1), 0);
    if (n_listed) {
        std::vector<double> vals(n_listed);
        HIP_TRY(hipMemcpyAsync(vals.data(), d_listed_val.p, (size_t)n_listed * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t k = 0; k < n_listed; ++k) lens[k] = (uint8_t)tk::float_repr(vals[k], (char *)strs.data() + (size_t)tk::kReprMax * k);
    }
    PC_TRY(d_strs.upload(strs, st)); PC_TRY(d_lens.upload(lens, st));
    return PC_OK;
}

// Phase 1: per slot the fixed-tree sum, first and last non-zero; from them the contigs that are written.
int export_slot_sums(TrackExport &c) {
    hipStream_t st = c.st;
    const int K0 = (int)c.slots.ids.size();
    c.stat.assign((size_t)K0, tk::SlotStat{0.0, ~0ull, 0ull});
    int64_t max_tiles = 1;
    for (const tk::SlotCells &s : c.slots.cells) max_tiles = std::max(max_tiles, (s.n + tk::kSumTile - 1) / tk::kSumTile);
    HIP_TRY(hipEventRecord(c.ev[0], st));
    PC_TRY(c.d_slots.upload(c.slots.cells, st)); PC_TRY(c.d_stat.upload(c.stat, st));
    PC_TRY(c.d_partial.reserve((size_t)K0 * (size_t)max_tiles));
    hipLaunchKernelGGL(tk::k_export_slot_partial, dim3((unsigned)max_tiles, (unsigned)K0), dim3(256), 0, st, c.d_slots.p, c.t->cells.p, max_tiles, c.d_partial.p, c.d_stat.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(tk::k_export_slot_final, dim3((unsigned)K0), dim3(256), 0, st, c.d_slots.p, c.d_partial.p, max_tiles, c.d_stat.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c.stat.data(), c.d_stat.p, c.stat.size() * sizeof(tk::SlotStat), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventRecord(c.ev[1], st));
    c.xr = c.t->tab.export_ranges(c.kind, c.slots, c.stat);
    c.K = c.xr.ranges.empty() ? 0 : (int)c.xr.ranges.size() - 1;
    return PC_OK;
}

// Phase 2: run heads, count, exclusive sum, select into the run table.
int export_run_table(TrackExport &c) {
    hipStream_t st = c.st;
    const int64_t E = c.xr.cells;
    if (E >= (int64_t)0x7fffffff || c.xr.names.size() >= (size_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_track_export: more than 2^31 cells to export");
    PC_TRY(c.d_ranges.upload(c.xr.ranges, st)); PC_TRY(c.d_names.upload(c.xr.names, st));
    if (E > 0) {
        int rc = PC_OK;
        room(rc, c.d_flags, (size_t)E); room(rc, c.d_idx, (size_t)E);
        if (rc != PC_OK) return rc;
        hipLaunchKernelGGL(tk::k_export_flags, dim3((unsigned)((E + tk::kExportTile - 1) / tk::kExportTile)), dim3(256), 0, st, c.kind, c.d_ranges.p, c.K, E, c.t->cells.p,
                           c.d_flags.p);
        HIP_TRY(hipGetLastError());
        PC_TRY(cub_run(c.d_tmp, [&](void *tmp, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(tmp, b, c.d_flags.p, c.d_idx.p, (int)E, st); }));
        hipLaunchKernelGGL(tk::k_export_bases, dim3(grid256(c.K + 1)), dim3(256), 0, st, c.d_flags.p, c.d_idx.p, E, c.d_ranges.p, c.K);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&c.R, &c.d_ranges.p[c.K].run_base, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (c.R > 0) {
            PC_TRY(c.d_run_e.reserve((size_t)c.R));
            hipLaunchKernelGGL(tk::k_export_select, dim3(grid256(E)), dim3(256), 0, st, c.d_flags.p, c.d_idx.p, E, c.d_run_e.p);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipEventRecord(c.ev[2], st));
    return PC_OK;
}

// Phase 3: the values that are not plain go to the host and come back as text.
int export_listed_values(TrackExport &c) {
    hipStream_t st = c.st;
    const int64_t R = c.R;
    int rc = PC_OK;
    room(rc, c.d_listed_slot, (size_t)std::max<int64_t>(R, 1)); room(rc, c.d_listed_val, (size_t)std::max<int64_t>(R, 1)); room(rc, c.d_n_listed, 1);
    if (rc != PC_OK) return rc;
    if (R > 0) {
        HIP_TRY(hipMemsetAsync(c.d_n_listed.p, 0, sizeof(uint32_t), st));
        hipLaunchKernelGGL(tk::k_export_classify, dim3(grid256(R)), dim3(256), 0, st, c.d_ranges.p, c.K, c.d_run_e.p, R, c.t->cells.p, c.d_listed_slot.p, c.d_listed_val.p,
                           c.d_n_listed.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&c.n_listed, c.d_n_listed.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    PC_TRY(listed_values_as_text(st, c.n_listed, c.d_listed_val, c.strs, c.lens, c.d_strs, c.d_lens));
    HIP_TRY(hipEventRecord(c.ev[3], st));
    return PC_OK;
}

// Phase 4: a byte length per line and their exclusive sum: every line's offset, the size of the text.
int export_lengths_and_offsets(TrackExport &c) {
    hipStream_t st = c.st;
    const int64_t nlines = c.nlines = c.R + c.K;
    if (nlines >= (int64_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_track_export: more than 2^31 lines");
    tk::ExportView &v = c.view;
    v.kind = c.kind; v.ranges = c.d_ranges.p; v.K = c.K; v.run_e = c.d_run_e.p; v.cells = c.t->cells.p; v.names = c.d_names.p;
    v.listed_slot = c.d_listed_slot.p; v.strs = c.d_strs.p; v.lens = c.d_lens.p;
    int rc = PC_OK;
    room(rc, c.d_len, (size_t)nlines); room(rc, c.d_off, (size_t)nlines);
    if (rc != PC_OK) return rc;
    hipLaunchKernelGGL(tk::k_export_lengths, dim3((unsigned)((nlines + tk::kFormatRuns - 1) / tk::kFormatRuns)), dim3(tk::kFormatRuns), 0, st, v, nlines, c.d_len.p);
    HIP_TRY(hipGetLastError());
    PC_TRY(cub_run(c.d_tmp, [&](void *tmp, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(tmp, b, c.d_len.p, c.d_off.p, (int)nlines, st); }));
    int64_t last_off = 0, last_len = 0;
    HIP_TRY(hipMemcpyAsync(&last_off, c.d_off.p + (nlines - 1), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&last_len, c.d_len.p + (nlines - 1), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c.total = last_off + last_len;
    HIP_TRY(hipEventRecord(c.ev[4], st));
    return PC_OK;
}

// Phase 5: every line's bytes at its offset.
int export_format(TrackExport &c) {
    PC_TRY(c.t->ex_text.reserve((size_t)c.total));
    hipLaunchKernelGGL(tk::k_export_format, dim3((unsigned)((c.nlines + tk::kFormatRuns - 1) / tk::kFormatRuns)), dim3(tk::kFormatRuns), 0, c.st, c.view, c.nlines,
                       c.d_off.p, c.t->ex_text.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c.ev[5], c.st));
    return PC_OK;
}

// ---------------------------------------------------------------- export of a counted plan (pc_counts_export)

// What the phases of one export of a plan's output share.  The phases that launch typed kernels are templates over the
// plan's output dtype (int64_t, double).
struct CountsExport {
    pc_engine *e;
    pc_plan *p;
    int kind;
    int64_t period;
    hipStream_t st;
    LapEvents<6> ev;                   // start | run heads | run table + lines | listed values | lengths + offsets | formatted
    tk::ExportRanges xr;               // the ranges of the batch and the sentinel behind them
    int K = 0;                         // ranges
    int64_t E = 0, R = 0, nvalues = 0, nlines = 0, total = 0;   // elements, runs, classified values, lines, bytes
    uint32_t n_listed = 0;
    std::vector<uint8_t> strs, lens;
    DevBuf<tk::ExRange> d_ranges;
    DevBuf<uint32_t> d_flags, d_idx, d_run_e, d_line_run, d_listed_slot, d_n_listed;
    DevBuf<double> d_listed_val;
    DevBuf<uint8_t> d_tmp, d_names, d_strs, d_lens;
    DevBuf<int64_t> d_len, d_off;
    template <typename T> tk::CountView<T> view(bool listed) const {
        tk::CountView<T> v;
        v.kind = kind; v.ranges = d_ranges.p; v.K = K; v.run_e = d_run_e.p; v.line_run = d_line_run.p; v.out = (const T *)p->d_out.p; v.names = d_names.p;
        v.listed_slot = listed ? d_listed_slot.p : nullptr; v.strs = listed ? d_strs.p : nullptr; v.lens = listed ? d_lens.p : nullptr;
        return v;
    }
};

// flags in front of position n of an exclusive sum over n flags
int flags_total(hipStream_t st, const uint32_t *d_flags, const uint32_t *d_idx, int64_t n, int64_t &total) {
    uint32_t last[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&last[0], d_idx + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&last[1], d_flags + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    total = (int64_t)last[0] + (int64_t)last[1];
    return PC_OK;
}

// Phase 1: run-head flags over the 8-byte output.
template <typename T> int counts_run_heads(CountsExport &c) {
    hipStream_t st = c.st;
    PC_TRY(c.d_ranges.upload(c.xr.ranges, st));
    PC_TRY(c.d_names.upload(c.xr.names, st));
    if (c.E > 0) {
        int rc = PC_OK;
        room(rc, c.d_flags, (size_t)c.E); room(rc, c.d_idx, (size_t)c.E);
        if (rc != PC_OK) return rc;
        const uint32_t period = tk::count_period32(c.kind, c.period);
        hipLaunchKernelGGL(tk::k_counts_flags<T>, dim3((unsigned)((c.E + tk::kExportTile - 1) / tk::kExportTile)), dim3(256), 0, st, c.kind, period, c.d_ranges.p, c.K, c.E,
                           (const T *)c.p->d_out.p, c.d_flags.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(c.ev[1], st));
    return PC_OK;
}

// Phases 2, 3: exclusive sum and select into the run table, the runs in front of every range; bedGraph: a second flag,
// sum and select pass keeps the runs whose value is > 0 as the lines.
template <typename T> int counts_run_table(CountsExport &c) {
    hipStream_t st = c.st;
    const int64_t E = c.E;
    int64_t kept = 0;
    if (E > 0) {
        PC_TRY(cub_run(c.d_tmp, [&](void *tmp, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(tmp, b, c.d_flags.p, c.d_idx.p, (int)E, st); }));
        hipLaunchKernelGGL(tk::k_export_bases, dim3(grid256(c.K + 1)), dim3(256), 0, st, c.d_flags.p, c.d_idx.p, E, c.d_ranges.p, c.K);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&c.R, &c.d_ranges.p[c.K].run_base, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    int rc = PC_OK;
    room(rc, c.d_run_e, (size_t)std::max<int64_t>(c.R, 1)); room(rc, c.d_line_run, (size_t)std::max<int64_t>(c.R, 1));
    if (rc != PC_OK) return rc;
    if (c.R > 0) {
        hipLaunchKernelGGL(tk::k_export_select, dim3(grid256(E)), dim3(256), 0, st, c.d_flags.p, c.d_idx.p, E, c.d_run_e.p);
        HIP_TRY(hipGetLastError());
        if (c.kind == 0) {
            // (the element flags are spent: the run flags take their place)
            hipLaunchKernelGGL(tk::k_counts_keep<T>, dim3(grid256(c.R)), dim3(256), 0, st, c.d_ranges.p, c.K, c.d_run_e.p, c.R, (const T *)c.p->d_out.p, c.d_flags.p);
            HIP_TRY(hipGetLastError());
            PC_TRY(cub_run(c.d_tmp, [&](void *tmp, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(tmp, b, c.d_flags.p, c.d_idx.p, (int)c.R, st); }));
            PC_TRY(flags_total(st, c.d_flags.p, c.d_idx.p, c.R, kept));
            if (kept > 0) {
                hipLaunchKernelGGL(tk::k_export_select, dim3(grid256(c.R)), dim3(256), 0, st, c.d_flags.p, c.d_idx.p, c.R, c.d_line_run.p);
                HIP_TRY(hipGetLastError());
            }
        }
    }
    c.nlines = c.kind == 0 ? kept : c.R + c.K;
    c.nvalues = c.kind == 0 ? kept : c.R;
    HIP_TRY(hipEventRecord(c.ev[2], st));
    return PC_OK;
}

// Phase 4 (float64): the values of the lines that are not plain go to the host and come back as text.
int counts_listed_values(CountsExport &c) {
    hipStream_t st = c.st;
    int rc = PC_OK;
    room(rc, c.d_listed_slot, (size_t)std::max<int64_t>(c.nvalues, 1)); room(rc, c.d_listed_val, (size_t)std::max<int64_t>(c.nvalues, 1)); room(rc, c.d_n_listed, 1);
    if (rc != PC_OK) return rc;
    if (c.nvalues > 0) {
        HIP_TRY(hipMemsetAsync(c.d_n_listed.p, 0, sizeof(uint32_t), st));
        hipLaunchKernelGGL(tk::k_counts_classify, dim3(grid256(c.nvalues)), dim3(256), 0, st, c.view<double>(false), c.nvalues, c.d_listed_slot.p, c.d_listed_val.p, c.d_n_listed.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&c.n_listed, c.d_n_listed.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return listed_values_as_text(st, c.n_listed, c.d_listed_val, c.strs, c.lens, c.d_strs, c.d_lens);
}

// Phases 5, 6: a byte length per line into a counting sink and their exclusive sum; the format kernel stores every line
// at its offset.
template <typename T> int counts_lengths_and_format(CountsExport &c, bool listed) {
    hipStream_t st = c.st;
    const int64_t nlines = c.nlines;
    const tk::CountView<T> v = c.view<T>(listed);
    const unsigned grid = (unsigned)((nlines + tk::kFormatRuns - 1) / tk::kFormatRuns);
    int rc = PC_OK;
    room(rc, c.d_len, (size_t)nlines); room(rc, c.d_off, (size_t)nlines);
    if (rc != PC_OK) return rc;
    hipLaunchKernelGGL(tk::k_counts_lengths<T>, dim3(grid), dim3(tk::kFormatRuns), 0, st, v, nlines, c.d_len.p);
    HIP_TRY(hipGetLastError());
    PC_TRY(cub_run(c.d_tmp, [&](void *tmp, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(tmp, b, c.d_len.p, c.d_off.p, (int)nlines, st); }));
    int64_t last_off = 0, last_len = 0;
    HIP_TRY(hipMemcpyAsync(&last_off, c.d_off.p + (nlines - 1), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&last_len, c.d_len.p + (nlines - 1), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c.total = last_off + last_len;
    HIP_TRY(hipEventRecord(c.ev[4], st));
    PC_TRY(c.e->cx_text.reserve((size_t)c.total));
    hipLaunchKernelGGL(tk::k_counts_format<T>, dim3(grid), dim3(tk::kFormatRuns), 0, st, v, nlines, c.d_off.p, c.e->cx_text.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c.ev[5], st));
    return PC_OK;
}

template <typename T> int counts_export_phases(CountsExport &c, bool is_float) {
    PC_TRY(counts_run_heads<T>(c));
    PC_TRY(counts_run_table<T>(c));
    if (c.nlines >= (int64_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_counts_export: more than 2^31 lines");
    if (is_float) PC_TRY(counts_listed_values(c));
    HIP_TRY(hipEventRecord(c.ev[3], c.st));
    if (c.nlines > 0) PC_TRY(counts_lengths_and_format<T>(c, is_float));
    else { HIP_TRY(hipEventRecord(c.ev[4], c.st)); HIP_TRY(hipEventRecord(c.ev[5], c.st)); }
    return PC_OK;
}

// a counted one-row plan without summed slices on engine e, its results complete
int counts_source_check(const char *who, pc_engine *e, pc_plan *p) {
    if (p->e != e) return fail(PC_ERR_ARG, "%s: the plan lives on another engine", who);
    if (!p->counted) return fail(PC_ERR_STATE, "%s: nothing counted yet", who);
    if (p->rows != 1 || p->has_sums) return fail(PC_ERR_ARG, "%s: needs a plan of one row per position without summed slices", who);
    return PC_OK;
}

} // namespace

extern "C" {

int pc_track_create(pc_engine *e, int nstrands, int64_t min_chr_size, pc_track **out) {
    if (!e || !out || nstrands < 1 || nstrands > 8 || min_chr_size < 0) return fail(PC_ERR_ARG, "pc_track_create: bad arguments");
    pc_track *t = new pc_track();
    t->e = e; t->tab.nstrands = nstrands; t->tab.min_chr_size = min_chr_size;
    t->cells.pool = &e->pool; t->ex_text.pool = &e->pool; t->nz.pool = &e->pool;
    e->tracks.push_back(t);
    *out = t;
    return PC_OK;
}

int pc_track_destroy(pc_track *t) {
    if (!t) return PC_OK;
    (void)hipSetDevice(t->e->device);
    (void)hipStreamSynchronize(t->e->stream);
    auto &list = t->e->tracks;
    list.erase(std::remove(list.begin(), list.end(), t), list.end());
    delete t;
    return PC_OK;
}

int pc_track_declare(pc_track *t, const char *name, int64_t length) {
    if (!t || !name || length < 0) return fail(PC_ERR_ARG, "pc_track_declare: bad arguments");
    if (!t->tab.declare(name, length)) return fail(PC_ERR_ARG, "pc_track_declare: %s is declared already", name);
    return PC_OK;
}

int pc_track_add_text(pc_track *t, const void *image, int64_t size, const char *name, int strand_slot) {
    return track_add_impl(t, image, size, name, strand_slot);
}

int pc_track_add_path(pc_track *t, const char *path, int strand_slot) {
    if (!t || !path) return fail(PC_ERR_ARG, "pc_track_add_path: bad arguments");
    const BamKnobs knobs;
    MappedFile mf;
    PC_TRY(mf.open(path, -1, knobs.touch));
    return track_add_impl(t, mf.p, (int64_t)mf.size, path, strand_slot);
}

int pc_track_num_contigs(pc_track *t) { return t ? t->tab.num_public() : -1; }

const char *pc_track_contig_name(pc_track *t, int i) {
    const int32_t id = t ? t->tab.public_id(i) : -1;
    return id < 0 ? nullptr : t->tab.names[(size_t)id].c_str();
}

int64_t pc_track_contig_length(pc_track *t, int i) {
    const int32_t id = t ? t->tab.public_id(i) : -1;
    return id < 0 ? -1 : t->tab.length[(size_t)id];
}

int64_t pc_track_contig_extent(pc_track *t, int i, int strand_slot) {
    const int64_t at = t ? t->tab.public_slot(i, strand_slot) : -1;
    return at < 0 ? -1 : t->tab.ext[(size_t)at];
}

int pc_track_gather(pc_track *t, int64_t nseg, const int32_t *contig, const int32_t *strand_slot, const int64_t *start, const int64_t *end,
                    const int64_t *out_off, const int8_t *out_step, int64_t out_elems, int normalize, double *host_out) {
    if (!t || nseg < 0 || out_elems < 0 || (nseg > 0 && (!contig || !strand_slot || !start || !end || !out_off || !out_step)) || (out_elems > 0 && !host_out))
        return fail(PC_ERR_ARG, "pc_track_gather: bad arguments");
    if (out_elems == 0) return PC_OK;
    pc_engine *e = t->e;
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    double sum = 1.0;
    if (normalize) PC_TRY(pc_track_sum(t, &sum));
    const std::string bad = tk::check_segments(tk::kGatherWords, nseg, start, end, out_off, out_step, out_elems, false);
    if (!bad.empty()) return fail(PC_ERR_ARG, "%s", bad.c_str());
    std::vector<pcdense::Item> items;
    t->tab.cut_items(nseg, start, end, out_off, out_step, [&](int64_t s) { return t->tab.public_slot(contig[s], strand_slot[s]); }, items);
    DevBuf<pcdense::Item> d_items;
    DevBuf<double> d_out;
    DrainOnExit drained{st};
    PC_TRY(d_out.reserve((size_t)out_elems));
    HIP_TRY(hipMemsetAsync(d_out.p, 0, (size_t)out_elems * sizeof(double), st));
    if (!items.empty()) {
        if (items.size() >= (size_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_track_gather: too many items");
        PC_TRY(d_items.upload(items, st));
        hipLaunchKernelGGL(pctrack::k_track_gather, dim3((unsigned)items.size()), dim3(pcdense::kGatherWG), 0, st, d_items.p, t->cells.p, d_out.p, normalize ? 1 : 0, sum);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(host_out, d_out.p, (size_t)out_elems * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    return PC_OK;
}

int pc_track_sum(pc_track *t, double *sum) {
    if (!t || !sum) return fail(PC_ERR_ARG, "pc_track_sum: bad arguments");
    if (!t->sum_valid) {
        double s = 0.0;
        const int64_t ncells = t->tab.ncells;
        if (ncells > 0) {
            pc_engine *e = t->e;
            HIP_TRY(hipSetDevice(e->device));
            PoolScope pool_scope(&e->pool);
            hipStream_t st = e->stream;
            const int64_t nb = (ncells + pctrack::kSumTile - 1) / pctrack::kSumTile;
            DevBuf<double> d_partial;
            DrainOnExit drained{st};
            PC_TRY(d_partial.reserve((size_t)nb + 1));
            hipLaunchKernelGGL(pctrack::k_track_sum_partial, dim3((unsigned)nb), dim3(256), 0, st, t->cells.p, ncells, d_partial.p);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(pctrack::k_track_sum_final, dim3(1), dim3(256), 0, st, d_partial.p, nb, d_partial.p + nb);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&s, d_partial.p + nb, sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            drained.armed = false;
        }
        t->sum = s;
        t->sum_valid = true;
    }
    *sum = t->sum;
    return PC_OK;
}

int pc_track_stats(pc_track *t, int64_t *out6) {
    if (!t || !out6) return fail(PC_ERR_ARG, "pc_track_stats: bad arguments");
    for (int k = 0; k < 6; ++k) out6[k] = t->stats[k];
    return PC_OK;
}

int pc_track_timing(pc_track *t, double *ms5) {
    if (!t || !ms5) return fail(PC_ERR_ARG, "pc_track_timing: bad arguments");
    for (int k = 0; k < 5; ++k) ms5[k] = t->ms[k];
    return PC_OK;
}

// ---------------------------------------------------------------- writes

int pc_track_set(pc_track *t, const char *contig, int strand_slot, int64_t nseg, const int64_t *start, const int64_t *end, const int64_t *val_off,
                 const int8_t *val_step, const double *values, int64_t nvalues, double scalar) {
    if (!t || !contig || nseg < 0 || (nseg > 0 && (!start || !end)) || nvalues < 0 || (values && nseg > 0 && (!val_off || !val_step)))
        return fail(PC_ERR_ARG, "pc_track_set: bad arguments");
    if (strand_slot < 0 || strand_slot >= t->tab.nstrands) return fail(PC_ERR_ARG, "pc_track_set: strand slot %d of %d", strand_slot, t->tab.nstrands);
    // everything is checked before anything changes
    const std::string bad = tk::check_segments(tk::kSetWords, nseg, start, end, values ? val_off : nullptr, val_step, nvalues, true);
    if (!bad.empty()) return fail(PC_ERR_ARG, "%s", bad.c_str());
    pc_engine *e = t->e;
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    const int32_t id = t->tab.id_of(contig);
    const int64_t furthest = t->tab.grow_for_set(id, start, end, nseg);
    t->sum_valid = false;
    if (furthest == 0) return PC_OK;
    PC_TRY(track_grow_storage(t, t->tab.plan_storage(id, strand_slot, furthest), st));
    const int64_t slot = (int64_t)t->tab.slot(id, strand_slot);
    std::vector<pcdense::Item> items;
    t->tab.cut_items(nseg, start, end, values ? val_off : nullptr, val_step, [slot](int64_t) { return slot; }, items);
    if (items.size() >= (size_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_track_set: too many items");
    DevBuf<pcdense::Item> d_items;
    DevBuf<double> d_values;
    DrainOnExit drained{st};
    PC_TRY(d_items.upload(items, st));
    if (values) PC_TRY(d_values.upload(values, (size_t)nvalues, st));
    hipLaunchKernelGGL(tk::k_track_set, dim3((unsigned)items.size()), dim3(pcdense::kGatherWG), 0, st, d_items.p, t->cells.p, values ? d_values.p : nullptr, scalar);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    return PC_OK;
}

// ---------------------------------------------------------------- arithmetic, equality

int pc_track_combine(pc_track *a, pc_track *b, double scalar, int op, int mode_all, int64_t length_pad, int nstrands_out, const int32_t *slot_a,
                     const int32_t *slot_b, pc_track **out) {
    if (!a || !out || length_pad < 0 || nstrands_out < 1 || nstrands_out > 8 || !slot_a || (b && !slot_b) || op < tk::kOpAdd || op > tk::kOpMul)
        return fail(PC_ERR_ARG, "pc_track_combine: bad arguments");
    if (b && b->e != a->e) return fail(PC_ERR_ARG, "pc_track_combine: the operands live on different engines");
    pc_engine *e = a->e;
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    pc_track *r = nullptr;
    PC_TRY(pc_track_create(e, nstrands_out, a->tab.min_chr_size, &r));
    struct Undo { pc_track *r; ~Undo() { if (r) (void)pc_track_destroy(r); } } undo{r};
    std::vector<tk::OpSlot> slots;
    const int64_t total = tk::ContigTable::combine_layout(a->tab, b ? &b->tab : nullptr, mode_all != 0, length_pad, slot_a, slot_b, r->tab, slots);
    if (total > 0) {
        DevBuf<tk::OpSlot> d_slots;
        DrainOnExit drained{st};
        PC_TRY(r->cells.reserve((size_t)total));
        PC_TRY(d_slots.upload(slots, st));
        hipLaunchKernelGGL(tk::k_track_op, dim3(grid256(total)), dim3(256), 0, st, d_slots.p, (int)slots.size(), total, a->cells.p, b ? b->cells.p : nullptr,
                           b ? 1 : 0, scalar, op, r->cells.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        drained.armed = false;
    }
    undo.r = nullptr;
    *out = r;
    return PC_OK;
}

// npair slots to compare: public contig and strand slot in a and in b (-1: the array lacks it, all zero)
int pc_track_equal(pc_track *a, pc_track *b, int64_t npair, const int32_t *contig_a, const int32_t *slot_a, const int32_t *contig_b, const int32_t *slot_b,
                   double tol, int *equal) {
    if (!a || !b || !equal || npair < 0 || (npair > 0 && (!contig_a || !slot_a || !contig_b || !slot_b))) return fail(PC_ERR_ARG, "pc_track_equal: bad arguments");
    if (b->e != a->e) return fail(PC_ERR_ARG, "pc_track_equal: the operands live on different engines");
    pc_engine *e = a->e;
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    std::vector<tk::OpSlot> slots;
    const int64_t total = tk::ContigTable::equal_layout(a->tab, b->tab, npair, contig_a, slot_a, contig_b, slot_b, slots);
    *equal = 1;
    if (total == 0) return PC_OK;
    DevBuf<tk::OpSlot> d_slots;
    DevBuf<uint32_t> d_flag;
    DrainOnExit drained{st};
    PC_TRY(d_slots.upload(slots, st));
    PC_TRY(d_flag.reserve(1));
    HIP_TRY(hipMemsetAsync(d_flag.p, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(tk::k_track_equal, dim3(grid256(total)), dim3(256), 0, st, d_slots.p, (int)slots.size(), total, a->cells.p, b->cells.p, tol, d_flag.p);
    HIP_TRY(hipGetLastError());
    uint32_t differs = 0;
    HIP_TRY(hipMemcpyAsync(&differs, d_flag.p, sizeof(differs), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    *equal = differs ? 0 : 1;
    return PC_OK;
}

// ---------------------------------------------------------------- export

// One strand as bedGraph (kind 0) or variableStep (kind 1) text behind the track line (genome_array.py:1996-2084), built
// in HBM on the engine's stream: slot sums and first / last non-zero; run heads (non-zero cells), count, exclusive sum and
// select into the run table; the values that are not plain to the host and back as text; a byte length per line; their
// exclusive sum; the format kernel.  *bytes: the size of the text, which waits for pc_track_export_read.
int pc_track_export(pc_track *t, int kind, int strand_slot, int64_t *bytes) {
    if (!t || !bytes || (kind != 0 && kind != 1)) return fail(PC_ERR_ARG, "pc_track_export: bad arguments");
    if (strand_slot < 0 || strand_slot >= t->tab.nstrands) return fail(PC_ERR_ARG, "pc_track_export: strand slot %d of %d", strand_slot, t->tab.nstrands);
    pc_engine *e = t->e;
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    for (auto &x : t->ex_stats) x = 0;
    for (auto &x : t->ex_ms) x = 0.0;
    t->ex_bytes = 0;
    *bytes = 0;
    TrackExport c{t, kind, strand_slot, e->stream};
    c.slots = t->tab.export_slots(strand_slot);
    if (c.slots.ids.empty()) return PC_OK;
    if (c.slots.ids.size() > 65535) return fail(PC_ERR_ARG, "pc_track_export: more than 65535 contigs");
    PC_TRY(c.ev.create());
    DrainOnExit drained{c.st};
    PC_TRY(export_slot_sums(c));
    if (c.K == 0) { drained.armed = false; return PC_OK; }
    PC_TRY(export_run_table(c));
    PC_TRY(export_listed_values(c));
    PC_TRY(export_lengths_and_offsets(c));
    PC_TRY(export_format(c));
    HIP_TRY(hipStreamSynchronize(c.st));
    drained.armed = false;
    c.ev.laps(t->ex_ms, 5);
    t->ex_stats[0] = c.nlines; t->ex_stats[1] = c.R; t->ex_stats[2] = (int64_t)c.n_listed; t->ex_stats[3] = c.total;
    t->ex_bytes = c.total;
    *bytes = c.total;
    return PC_OK;
}

// The text of the last pc_track_export (`bytes` as it reported), through the transfer ring when it is large.
int pc_track_export_read(pc_track *t, void *dst, int64_t bytes) {
    if (!t || t->ex_bytes < 0 || bytes != t->ex_bytes || (bytes > 0 && !dst)) return fail(PC_ERR_ARG, "pc_track_export_read: no exported text of this size");
    pc_engine *e = t->e;
    HIP_TRY(hipSetDevice(e->device));
    const auto t0 = std::chrono::steady_clock::now();
    if (bytes > 0) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        const std::vector<TransferJob> job{{dst, t->ex_text.p, (size_t)bytes}};
        PC_TRY(TransferRing::of(e->device).run(e->device, job, TransferRing::kPiece, false, true));
    }
    t->ex_ms[5] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    t->ex_text.release();
    t->ex_bytes = -1;
    return PC_OK;
}

int pc_track_export_stats(pc_track *t, int64_t *out4) {
    if (!t || !out4) return fail(PC_ERR_ARG, "pc_track_export_stats: bad arguments");
    for (int k = 0; k < 4; ++k) out4[k] = t->ex_stats[k];
    return PC_OK;
}

int pc_track_export_timing(pc_track *t, double *ms6) {
    if (!t || !ms6) return fail(PC_ERR_ARG, "pc_track_export_timing: bad arguments");
    for (int k = 0; k < 6; ++k) ms6[k] = t->ex_ms[k];
    return PC_OK;
}

int pc_track_export_geometry(int *out2) {
    if (!out2) return fail(PC_ERR_ARG, "pc_track_export_geometry: bad arguments");
    out2[0] = tk::kExportTile; out2[1] = tk::kFormatRuns;
    return PC_OK;
}

// ---------------------------------------------------------------- a counted plan as text, and into a track (revision 17)

// The contigs of an export in batches of at most `budget` output elements (track_table.h: count_batches).
int pc_counts_export_batches(int64_t n, const int64_t *len, int64_t budget, int32_t *batch_of, int *nbatch) {
    if (n < 0 || !nbatch || (n > 0 && (!len || !batch_of))) return fail(PC_ERR_ARG, "pc_counts_export_batches: bad arguments");
    std::string msg;
    *nbatch = tk::count_batches(n, len, budget > 0 ? budget : tk::kCountBudget, batch_of, msg);
    if (!msg.empty()) return fail(PC_ERR_ARG, "pc_counts_export_batches: %s", msg.c_str());
    // (the scans of pc_counts_export count in int: what the layout admits up to 2^32 - 1 is refused here, where the export is planned)
    for (int64_t k = 0; k < n; ++k)
        if (len[k] >= (int64_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_counts_export_batches: contig %lld has 2^31 - 1 positions or more: a batch of pc_counts_export holds fewer", (long long)k);
    return PC_OK;
}

// BAMGenomeArray's to_bedgraph (kind 0; period: the window size) / to_variable_step (kind 1) over the ranges of a counted
// one-row plan (genome_array.py:990-1111), everything behind the track line, built in HBM on the engine's stream by the
// phases of a CountsExport: run heads over the 8-byte output, exclusive sum and select into the run table, (bedGraph) the
// runs whose value is > 0 as lines, (float64) the values that are not plain to the host and back as text, a byte length
// per line, their exclusive sum, the format kernel.  *bytes: the size of the text, which waits for pc_counts_export_read.
int pc_counts_export(pc_engine *e, pc_plan *p, int kind, int64_t period, int nrange, const char *const *names, const int64_t *elem_off, const int64_t *len,
                     int64_t *bytes) {
    if (!e || !p || !bytes || (kind != 0 && kind != 1) || nrange < 0 || (nrange > 0 && (!names || !elem_off || !len)))
        return fail(PC_ERR_ARG, "pc_counts_export: bad arguments");
    PC_TRY(counts_source_check("pc_counts_export", e, p));
    if (kind == 0 && period < 1) return fail(PC_ERR_ARG, "pc_counts_export: the window of a bedGraph must be at least 1");
    std::string msg;
    CountsExport c{e, p, kind, period, e->stream};
    c.xr = tk::count_ranges(nrange, names, elem_off, len, p->out_elems, msg);
    if (!msg.empty()) return fail(PC_ERR_ARG, "pc_counts_export: %s", msg.c_str());
    c.K = nrange; c.E = c.xr.cells;
    if (c.E >= (int64_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_counts_export: more than 2^31 elements in one batch");
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    PC_TRY(check_grid_guard(e, p));
    for (auto &x : e->cx_stats) x = 0;
    for (auto &x : e->cx_ms) x = 0.0;
    e->cx_text.pool = &e->pool;
    e->cx_bytes = 0;
    *bytes = 0;
    if (nrange == 0 || (kind == 0 && c.E == 0)) return PC_OK;
    PC_TRY(c.ev.create());
    DrainOnExit drained{c.st};
    HIP_TRY(hipEventRecord(c.ev[0], c.st));
    const bool is_float = p->last_dtype == PC_OUT_FLOAT64;
    e->cx_bytes = -1;
    if (is_float) PC_TRY(counts_export_phases<double>(c, true)); else PC_TRY(counts_export_phases<int64_t>(c, false));
    HIP_TRY(hipStreamSynchronize(c.st));
    drained.armed = false;
    c.ev.laps(e->cx_ms, 5);
    e->cx_stats[0] = c.nlines; e->cx_stats[1] = c.R; e->cx_stats[2] = (int64_t)c.n_listed; e->cx_stats[3] = c.total;
    e->cx_bytes = c.total;
    *bytes = c.total;
    return PC_OK;
}

// The text of the last pc_counts_export (`bytes` as it reported), through the transfer ring when it is large.
int pc_counts_export_read(pc_engine *e, void *dst, int64_t bytes) {
    if (!e || e->cx_bytes < 0 || bytes != e->cx_bytes || (bytes > 0 && !dst)) return fail(PC_ERR_ARG, "pc_counts_export_read: no exported text of this size");
    HIP_TRY(hipSetDevice(e->device));
    const auto t0 = std::chrono::steady_clock::now();
    if (bytes > 0) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        const std::vector<TransferJob> job{{dst, e->cx_text.p, (size_t)bytes}};
        PC_TRY(TransferRing::of(e->device).run(e->device, job, TransferRing::kPiece, false, true));
    }
    e->cx_ms[5] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    e->cx_text.release();
    e->cx_bytes = -1;
    return PC_OK;
}

int pc_counts_export_stats(pc_engine *e, int64_t *out4) {
    if (!e || !out4) return fail(PC_ERR_ARG, "pc_counts_export_stats: bad arguments");
    for (int k = 0; k < 4; ++k) out4[k] = e->cx_stats[k];
    return PC_OK;
}

int pc_counts_export_timing(pc_engine *e, double *ms6) {
    if (!e || !ms6) return fail(PC_ERR_ARG, "pc_counts_export_timing: bad arguments");
    for (int k = 0; k < 6; ++k) ms6[k] = e->cx_ms[k];
    return PC_OK;
}

// pc_track_set for one segment [start, start + n) whose values are output elements [elem_off, elem_off + n) of a counted
// one-row plan on the track's engine, converted to double: no count crosses to the host.
int pc_track_set_counts(pc_track *t, const char *contig, int strand_slot, int64_t start, pc_plan *p, int64_t elem_off, int64_t n) {
    if (!t || !contig || !p) return fail(PC_ERR_ARG, "pc_track_set_counts: bad arguments");
    if (strand_slot < 0 || strand_slot >= t->tab.nstrands) return fail(PC_ERR_ARG, "pc_track_set_counts: strand slot %d of %d", strand_slot, t->tab.nstrands);
    // everything is checked before anything changes
    pc_engine *e = t->e;
    PC_TRY(counts_source_check("pc_track_set_counts", e, p));
    if (start < 0 || n < 0 || start > tk::kMaxCoord || n > tk::kMaxCoord - start) return fail(PC_ERR_ARG, "pc_track_set_counts: the segment lies outside [0, 2^40]");
    if (n > 0 && (elem_off < 0 || elem_off > p->out_elems || n > p->out_elems - elem_off)) return fail(PC_ERR_ARG, "pc_track_set_counts: reads outside the plan's output");
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    PC_TRY(check_grid_guard(e, p));
    const int64_t end = start + n;
    const int8_t step = 1;
    const int32_t id = t->tab.id_of(contig);
    const int64_t furthest = t->tab.grow_for_set(id, &start, &end, 1);
    t->sum_valid = false;
    if (furthest == 0) return PC_OK;
    PC_TRY(track_grow_storage(t, t->tab.plan_storage(id, strand_slot, furthest), st));
    const int64_t slot = (int64_t)t->tab.slot(id, strand_slot);
    std::vector<pcdense::Item> items;
    t->tab.cut_items(1, &start, &end, &elem_off, &step, [slot](int64_t) { return slot; }, items);
    if (items.empty()) return PC_OK;
    if (items.size() >= (size_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_track_set_counts: too many items");
    DevBuf<pcdense::Item> d_items;
    DrainOnExit drained{st};
    PC_TRY(d_items.upload(items, st));
    if (p->last_dtype == PC_OUT_FLOAT64)
        hipLaunchKernelGGL(tk::k_track_set_counts<double>, dim3((unsigned)items.size()), dim3(pcdense::kGatherWG), 0, st, d_items.p, t->cells.p, (const double *)p->d_out.p);
    else
        hipLaunchKernelGGL(tk::k_track_set_counts<int64_t>, dim3((unsigned)items.size()), dim3(pcdense::kGatherWG), 0, st, d_items.p, t->cells.p, (const int64_t *)p->d_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    return PC_OK;
}

// ---------------------------------------------------------------- nonzero

// counts[i * nstrands + s]: non-zero cells of public contig i on strand slot s; the indices wait for pc_track_nonzero_read
int pc_track_nonzero_count(pc_track *t, int64_t *counts) {
    if (!t || (!counts && t->tab.num_public() > 0)) return fail(PC_ERR_ARG, "pc_track_nonzero_count: bad arguments");
    for (int k = 0; k < t->tab.num_public() * t->tab.nstrands; ++k) counts[k] = 0;
    t->nz_total = 0;
    const int64_t n = t->tab.ncells;
    if (n == 0) return PC_OK;
    if (n >= (int64_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_track_nonzero: more than 2^31 stored cells");
    pc_engine *e = t->e;
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    tk::NzShares &z = t->nz_shares;
    z = t->tab.nonzero_slots();
    std::vector<int64_t> picked(z.at.size());
    DevBuf<uint32_t> d_flags, d_idx;
    DevBuf<uint8_t> d_tmp;
    DevBuf<int64_t> d_at, d_picked;
    DrainOnExit drained{st};
    int rc = PC_OK;
    room(rc, d_flags, (size_t)n); room(rc, d_idx, (size_t)n); room(rc, d_picked, z.at.size());
    if (rc != PC_OK) return rc;
    PC_TRY(d_at.upload(z.at, st));
    hipLaunchKernelGGL(tk::k_track_nz_flags, dim3(grid256(n)), dim3(256), 0, st, t->cells.p, n, d_flags.p);
    HIP_TRY(hipGetLastError());
    PC_TRY(cub_run(d_tmp, [&](void *tmp, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(tmp, b, d_flags.p, d_idx.p, (int)n, st); }));
    hipLaunchKernelGGL(tk::k_track_pick, dim3(grid256((int64_t)z.at.size())), dim3(256), 0, st, d_flags.p, d_idx.p, n, d_at.p, (int)z.at.size(), d_picked.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(picked.data(), d_picked.p, picked.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t total = picked.back();
    if (total > 0) {
        PC_TRY(t->nz.reserve((size_t)total));
        // (d_at: the live slots' first cells, ascending, in front of its last entry)
        hipLaunchKernelGGL(tk::k_track_nz_select, dim3(grid256(n)), dim3(256), 0, st, d_flags.p, d_idx.p, n, d_at.p, (int)z.live.size(), t->nz.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    drained.armed = false;
    t->tab.nonzero_counts(z, picked, counts);
    t->nz_total = total;
    return PC_OK;
}

// The indices of the last pc_track_nonzero_count, slot after slot in public order (contig-major), `total` of them.
int pc_track_nonzero_read(pc_track *t, int64_t *out, int64_t total) {
    if (!t || t->nz_total < 0 || total != t->nz_total || (total > 0 && !out)) return fail(PC_ERR_ARG, "pc_track_nonzero_read: no counted indices of this size");
    if (total == 0) { t->nz_total = -1; return PC_OK; }
    pc_engine *e = t->e;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    std::vector<int64_t> all((size_t)total);
    HIP_TRY(hipMemcpyAsync(all.data(), t->nz.p, (size_t)total * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    t->tab.nonzero_regroup(t->nz_shares, all.data(), out);
    t->nz.release();
    t->nz_total = -1;
    return PC_OK;
}

} // extern "C"
