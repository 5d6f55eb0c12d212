// Count tracks on the GPU, host side: the pc_track_* entry points of include/plastid_counts.h.  A pc_track is the
// reference's GenomeArray (plastid/genomics/genome_array.py:1323-1533) as a read-and-count object: float64 cells per
// (contig, strand slot) in one block of HBM, filled by pc_track_add_text / _path (add_from_wiggle, :1978-1994) and read by
// pc_track_gather.  One import is six phases (track_add_impl): upload, line starts (both shared with SAM text),
// classify + state records, fields (+ the host's conversion of the escaped lines), growth and storage, sort + apply.
// The host looks at the state lines, the escaped lines and the growth lines only.
// Revision 16 makes it the reference's mutable GenomeArray (:1535-2104): pc_track_set (one launch per segment or chain),
// pc_track_combine (a new track from a op b or a op scalar), pc_track_equal, pc_track_nonzero_count / _read and
// pc_track_export / _read: the bedGraph / variableStep text of a strand built in HBM in five phases and read back once;
// of an export the host sees the per-slot sums and the values that are not plain.
// Part of the one translation unit of plastid_counts.hip (behind sam_decoder.hip.h).
#include "track_kernels.hip.h"

struct pc_track {
    pc_engine *e = nullptr;
    int nstrands = 2;
    int64_t min_chr_size = 10000000;
    struct Contig { std::string name; int64_t length = 0; bool born = false; };
    std::vector<Contig> contigs;            // by internal id, in order of first mention
    std::map<std::string, int32_t> ids;
    std::vector<int32_t> order;             // the public order: declared contigs, then the others by first yielded line
    std::vector<int64_t> ext, cell_off;     // per slot (id * nstrands + strand): cells [cell_off, cell_off + ext)
    int64_t ncells = 0;
    DevBuf<double> cells;
    bool sum_valid = false;
    double sum = 0.0;
    int64_t stats[6] = {0, 0, 0, 0, 0, 0};  // lines, yielded, escaped, state records, overlapping lines, growth lines
    double ms[5] = {0, 0, 0, 0, 0};         // upload | line starts | classify + state records | fields | growth + sort + apply
    // the last pc_track_export: its text waits in HBM for pc_track_export_read
    DevBuf<uint8_t> ex_text;
    int64_t ex_bytes = -1;
    int64_t ex_stats[4] = {0, 0, 0, 0};     // lines, runs / non-zero cells, values listed for the host, bytes
    double ex_ms[6] = {0, 0, 0, 0, 0, 0};   // slot sums | run heads + select | listed values | lengths + offsets | format | read-back
    // the last pc_track_nonzero_count: the indices wait in HBM for pc_track_nonzero_read
    DevBuf<int64_t> nz;
    int64_t nz_total = -1;
    std::vector<int64_t> nz_begin, nz_cnt;  // per slot: its share of nz
};

// an engine that is destroyed takes its tracks with it (pc_destroy): their cells come from its pool
static void destroy_tracks_of(pc_engine *e) {
    for (pc_track *t : e->tracks) delete t;
    e->tracks.clear();
}

namespace {

namespace tk = pctrack;

int32_t track_contig_id(pc_track *t, const std::string &name) {
    auto it = t->ids.find(name);
    if (it != t->ids.end()) return it->second;
    const int32_t id = (int32_t)t->contigs.size();
    pc_track::Contig c;
    c.name = name; c.length = t->min_chr_size; c.born = false;
    t->contigs.push_back(c);
    t->ids.emplace(name, id);
    t->ext.resize(t->contigs.size() * (size_t)t->nstrands, 0);
    t->cell_off.resize(t->contigs.size() * (size_t)t->nstrands, 0);
    return id;
}

// an undeclared contig is born at min_chr_size, behind the contigs the array holds already (import and pc_track_set)
void track_bear(pc_track *t, int32_t id) {
    pc_track::Contig &c = t->contigs[(size_t)id];
    if (c.born) return;
    c.born = true; c.length = t->min_chr_size;
    t->order.push_back(id);
}

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
struct TrackGrowth { int64_t stop; uint32_t line; int32_t contig; };
__global__ __launch_bounds__(256) void k_track_growth_info(const uint32_t *__restrict__ lines, uint32_t n, const tk::LineRec *__restrict__ recs,
                                                           const int32_t *__restrict__ contig_of, TrackGrowth *__restrict__ out) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    TrackGrowth o;
    o.line = lines[k]; o.stop = recs[o.line].stop; o.contig = contig_of[o.line];
    out[k] = o;
}

inline unsigned grid256(int64_t n) { return (unsigned)((n + 255) / 256); }

int read_counters(hipStream_t st, const DevBuf<tk::TrackCounters> &d, tk::TrackCounters &h) {
    HIP_TRY(hipMemcpyAsync(&h, d.p, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PC_OK;
}

// listed lines with their text bounds, sorted by line
int fetch_line_info(hipStream_t st, const DevBuf<uint32_t> &lines, uint32_t n, const SamLines &ln, uint64_t text_len, const DevBuf<uint32_t> &data_index,
                    std::vector<TrackLineInfo> &out) {
    out.resize(n);
    if (!n) return PC_OK;
    DevBuf<TrackLineInfo> d_info;
    DrainOnExit drained{st};
    PC_TRY(d_info.reserve(n));
    hipLaunchKernelGGL(k_track_line_info, dim3(grid256(n)), dim3(256), 0, st, lines.p, n, ln.d_line_start.p, text_len, data_index.p, d_info.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out.data(), d_info.p, (size_t)n * sizeof(TrackLineInfo), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    std::sort(out.begin(), out.end(), [](const TrackLineInfo &a, const TrackLineInfo &b) { return a.line < b.line; });
    return PC_OK;
}

// Storage of the strand slots: every slot keeps its cells, slot (c, strand) reaches at least furthest[c].
int track_grow_storage(pc_track *t, int strand, const std::vector<unsigned long long> &furthest, hipStream_t st) {
    const size_t nslot = t->contigs.size() * (size_t)t->nstrands;
    std::vector<int64_t> ext(t->ext.begin(), t->ext.end()), off(nslot, 0);
    ext.resize(nslot, 0);
    bool grows = false;
    for (size_t c = 0; c < furthest.size(); ++c) {
        int64_t &x = ext[c * (size_t)t->nstrands + (size_t)strand];
        if ((int64_t)furthest[c] > x) { x = (int64_t)furthest[c]; grows = true; }
    }
    if (!grows) return PC_OK;
    int64_t total = 0;
    for (size_t s = 0; s < nslot; ++s) { off[s] = total; total += ext[s]; }
    DevBuf<double> fresh;
    fresh.pool = &t->e->pool;
    PC_TRY(fresh.reserve((size_t)total));
    HIP_TRY(hipMemsetAsync(fresh.p, 0, (size_t)total * sizeof(double), st));
    for (size_t s = 0; s < nslot && s < t->ext.size(); ++s)
        if (t->ext[s] > 0)
            HIP_TRY(hipMemcpyAsync(fresh.p + off[s], t->cells.p + t->cell_off[s], (size_t)t->ext[s] * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // (the old block goes back to the pool)
    t->cells.swap(fresh);
    t->ext = ext; t->cell_off = off; t->ncells = total;
    return PC_OK;
}

int track_add_impl(pc_track *t, const void *image_, int64_t size, const char *name, int strand) {
    if (!t || size < 0 || (size > 0 && !image_)) return fail(PC_ERR_ARG, "pc_track_add_text: bad arguments");
    if (strand < 0 || strand >= t->nstrands) return fail(PC_ERR_ARG, "pc_track_add_text: strand slot %d of %d", strand, t->nstrands);
    pc_engine *e = t->e;
    const uint8_t *text = (const uint8_t *)image_;
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    BamDecode d{e, e->stream, name ? name : "<memory>", BamKnobs()};
    hipStream_t st = d.st;
    for (int k = 0; k < 6; ++k) t->stats[k] = 0;
    for (int k = 0; k < 5; ++k) t->ms[k] = 0.0;
    if (size == 0) return PC_OK;
    hipEvent_t ev[6] = {};
    for (auto &x : ev) HIP_TRY(hipEventCreate(&x));
    struct EvGuard { hipEvent_t *ev; ~EvGuard() { for (int i = 0; i < 6; ++i) (void)hipEventDestroy(ev[i]); } } evg{ev};
    const bool open_end = text[size - 1] != (uint8_t)'\n';
    SamLines ln;
    {
        // phases 1, 2: the text to HBM, the line starts (sam_decoder.hip.h)
        Upload u;
        Drain drain{e, true};
        PC_TRY(d.d_stream.reserve((size_t)size + 64));
        HIP_TRY(hipEventRecord(ev[0], st));
        PC_TRY(sam_upload(d, text, size, nullptr, u));
        HIP_TRY(hipEventRecord(ev[1], st));
        PC_TRY(sam_line_starts(d, size, open_end, ln));
        drain.armed = false;
    }
    HIP_TRY(hipEventRecord(ev[2], st));
    const int64_t n = ln.nrec;
    t->stats[0] = n;
    if (n == 0) return PC_OK;
    const uint64_t text_len = (uint64_t)size;
    const unsigned g = grid256(n);

    // phase 3: classes, the state lines, the data-line prefix count
    DevBuf<uint8_t> d_cls, d_tmp;
    DevBuf<int32_t> d_sig, d_prev_sig, d_contig_of, d_head;
    DevBuf<uint32_t> d_is_data, d_data_index, d_list, d_idx, d_idx2, d_first_line, d_long;
    DevBuf<uint64_t> d_key, d_key2, d_end_key, d_prev_end, d_multi, d_multi2;
    DevBuf<tk::TrackCounters> d_cnt;
    DevBuf<tk::StateRec> d_recs;
    DevBuf<tk::LineRec> d_line, d_patch;
    DevBuf<int32_t> d_patch_contig;
    DevBuf<int64_t> d_len0, d_off;
    DevBuf<unsigned long long> d_furthest;
    DevBuf<TrackGrowth> d_growth;
    DrainOnExit drained{st};
    int rc = PC_OK;
    room(rc, d_cls, (size_t)n); room(rc, d_sig, (size_t)n); room(rc, d_prev_sig, (size_t)n); room(rc, d_is_data, (size_t)n);
    room(rc, d_data_index, (size_t)n); room(rc, d_list, (size_t)n); room(rc, d_cnt, 1);
    if (rc != PC_OK) return rc;
    tk::TrackCounters cnt;
    memset(&cnt, 0, sizeof(cnt));
    cnt.first_err = tk::kNoDefect;
    HIP_TRY(hipMemcpyAsync(d_cnt.p, &cnt, sizeof(cnt), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(tk::k_track_classify, dim3(g), dim3(256), 0, st, d.d_stream.p, text_len, ln.d_line_start.p, n, d_cls.p, d_sig.p, d_is_data.p);
    HIP_TRY(hipGetLastError());
    {
        size_t b1 = 0, b2 = 0;
        HIP_TRY(hipcub::DeviceScan::ExclusiveScan(nullptr, b1, d_sig.p, d_prev_sig.p, hipcub::Max(), (int32_t)-1, (int)n, st));
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b2, d_is_data.p, d_data_index.p, (int)n, st));
        PC_TRY(d_tmp.reserve(std::max<size_t>(std::max(b1, b2), 16)));
        HIP_TRY(hipcub::DeviceScan::ExclusiveScan(d_tmp.p, b1, d_sig.p, d_prev_sig.p, hipcub::Max(), (int32_t)-1, (int)n, st));
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, b2, d_is_data.p, d_data_index.p, (int)n, st));
    }
    hipLaunchKernelGGL(tk::k_track_states, dim3(g), dim3(256), 0, st, d.d_stream.p, text_len, ln.d_line_start.p, n, d_cls.p, d_prev_sig.p, d_list.p, &d_cnt.p->n_state);
    HIP_TRY(hipGetLastError());
    PC_TRY(read_counters(st, d_cnt, cnt));
    std::vector<TrackLineInfo> info;
    PC_TRY(fetch_line_info(st, d_list, cnt.n_state, ln, text_len, d_data_index, info));
    unsigned long long host_err = tk::kNoDefect;
    std::vector<tk::StateRec> recs(info.size());
    for (size_t k = 0; k < info.size(); ++k) {
        const int err = tk::parse_state(text + info[k].b, text + info[k].e, (int64_t)info[k].line, (int64_t)info[k].data_index,
                                        [t](const std::string &nm) { return track_contig_id(t, nm); }, recs[k]);
        if (err != tk::kTrkOk) host_err = std::min(host_err, ((unsigned long long)info[k].line << 8) | (unsigned long long)err);
    }
    t->stats[3] = (int64_t)recs.size();
    HIP_TRY(hipEventRecord(ev[3], st));

    // phase 4: the fields of every yielding line; the escaped ones on the host
    room(rc, d_recs, std::max<size_t>(recs.size(), 1)); room(rc, d_line, (size_t)n); room(rc, d_contig_of, (size_t)n);
    if (rc != PC_OK) return rc;
    if (!recs.empty()) HIP_TRY(hipMemcpyAsync(d_recs.p, recs.data(), recs.size() * sizeof(tk::StateRec), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(tk::k_track_fields, dim3(g), dim3(256), 0, st, d.d_stream.p, text_len, ln.d_line_start.p, n, d_cls.p, d_data_index.p, d_recs.p,
                       (int64_t)recs.size(), d_line.p, d_contig_of.p, d_list.p, d_cnt.p);
    HIP_TRY(hipGetLastError());
    PC_TRY(read_counters(st, d_cnt, cnt));
    t->stats[1] = cnt.n_yield; t->stats[2] = cnt.n_escaped;
    std::vector<tk::LineRec> patch;
    std::vector<int32_t> patch_contig;
    if (cnt.n_escaped) {
        PC_TRY(fetch_line_info(st, d_list, cnt.n_escaped, ln, text_len, d_data_index, info));
        patch.resize(info.size()); patch_contig.resize(info.size());
        for (size_t k = 0; k < info.size(); ++k) {
            const tk::LineClass lc = tk::classify_line(text + info[k].b, text + info[k].e);
            const int64_t gv = tk::governing(recs.data(), (int64_t)recs.size(), (int64_t)info[k].line);
            const tk::LineOut o = tk::line_fields<tk::FastThenFull>(lc, gv >= 0 ? &recs[(size_t)gv] : nullptr, (int64_t)info[k].data_index);
            int err = o.err;
            if (err == tk::kTrkOk) err = tk::check_fields(o);
            if (err != tk::kTrkOk) host_err = std::min(host_err, ((unsigned long long)info[k].line << 8) | (unsigned long long)err);
            patch[k].start = o.start; patch[k].stop = o.stop; patch[k].value = o.value;
            patch_contig[k] = err == tk::kTrkOk ? o.contig : -1;
        }
    }
    const unsigned long long first_err = std::min(host_err, cnt.first_err);
    if (first_err != tk::kNoDefect)
        return fail(PC_ERR_ARG, "%s", tk::track_defect_message(d.path.c_str(), (int64_t)(first_err >> 8) + 1, (int)(first_err & 0xffu)).c_str());
    if (cnt.n_escaped) {
        // (d_list still holds the escaped lines, in the order fetch_line_info saw them: patch by line)
        std::vector<uint32_t> lines(info.size());
        for (size_t k = 0; k < info.size(); ++k) lines[k] = info[k].line;
        PC_TRY(d_patch.upload(patch, st)); PC_TRY(d_patch_contig.upload(patch_contig, st)); PC_TRY(d_list.upload(lines, st));
        hipLaunchKernelGGL(tk::k_track_patch, dim3(grid256((int64_t)lines.size())), dim3(256), 0, st, d_list.p, d_patch.p, d_patch_contig.p, (uint32_t)lines.size(),
                           d_line.p, d_contig_of.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));   // (the host vectors above)
    }
    HIP_TRY(hipEventRecord(ev[4], st));

    // phase 5: births, growth, storage
    const int ncontig = (int)t->contigs.size();
    if (ncontig >= (1 << 22)) return fail(PC_ERR_ARG, "%s: more than 2^22 contigs", d.path.c_str());
    std::vector<unsigned long long> furthest((size_t)std::max(ncontig, 1), 0ull);
    std::vector<uint32_t> first_line((size_t)std::max(ncontig, 1), tk::kNoLine);
    if (ncontig > 0) {
        std::vector<int64_t> len0((size_t)ncontig);
        for (int c = 0; c < ncontig; ++c) len0[(size_t)c] = t->contigs[(size_t)c].born ? t->contigs[(size_t)c].length : t->min_chr_size;
        room(rc, d_key, (size_t)n); room(rc, d_idx, (size_t)n); room(rc, d_key2, (size_t)n); room(rc, d_idx2, (size_t)n);
        if (rc != PC_OK) return rc;
        PC_TRY(d_len0.upload(len0, st)); PC_TRY(d_furthest.upload(furthest, st)); PC_TRY(d_first_line.upload(first_line, st));
        hipLaunchKernelGGL(tk::k_track_keys, dim3(g), dim3(256), 0, st, d_line.p, d_contig_of.p, d_cls.p, n, d_len0.p, ncontig, d_furthest.p, d_first_line.p,
                           d_list.p, d_key.p, d_idx.p, d_cnt.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(furthest.data(), d_furthest.p, (size_t)ncontig * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(first_line.data(), d_first_line.p, (size_t)ncontig * 4, hipMemcpyDeviceToHost, st));
        PC_TRY(read_counters(st, d_cnt, cnt));
        // births, in order of the first yielded line
        std::vector<std::pair<uint32_t, int32_t>> born;
        for (int c = 0; c < ncontig; ++c)
            if (!t->contigs[(size_t)c].born && first_line[(size_t)c] != tk::kNoLine) born.emplace_back(first_line[(size_t)c], c);
        std::sort(born.begin(), born.end());
        for (auto &b : born) track_bear(t, b.second);
        // growth: the reference's rule (genome_array.py:1593-1602), folded in file order over the lines that can matter
        t->stats[5] = cnt.n_growth;
        if (cnt.n_growth) {
            std::vector<TrackGrowth> gr(cnt.n_growth);
            PC_TRY(d_growth.reserve(cnt.n_growth));
            hipLaunchKernelGGL(k_track_growth_info, dim3(grid256(cnt.n_growth)), dim3(256), 0, st, d_list.p, cnt.n_growth, d_line.p, d_contig_of.p, d_growth.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(gr.data(), d_growth.p, gr.size() * sizeof(TrackGrowth), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            std::sort(gr.begin(), gr.end(), [](const TrackGrowth &a, const TrackGrowth &b) { return a.line < b.line; });
            for (const TrackGrowth &x : gr) {
                int64_t &len = t->contigs[(size_t)x.contig].length;
                len = tk::grown_length(len, x.stop);
            }
        }
        PC_TRY(track_grow_storage(t, strand, furthest, st));
    }

    // phase 6: sort by (contig, start), clusters, fills
    const int64_t nv = ncontig > 0 ? (int64_t)cnt.n_valid : 0;
    if (nv > 0) {
        std::vector<int64_t> off((size_t)ncontig);
        for (int c = 0; c < ncontig; ++c) off[(size_t)c] = t->cell_off[(size_t)c * (size_t)t->nstrands + (size_t)strand];
        PC_TRY(d_off.upload(off, st));
        room(rc, d_end_key, (size_t)nv); room(rc, d_prev_end, (size_t)nv); room(rc, d_head, (size_t)nv); room(rc, d_long, (size_t)nv);
        room(rc, d_multi, (size_t)nv); room(rc, d_multi2, (size_t)nv);
        if (rc != PC_OK) return rc;
        size_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b0, d_key.p, d_key2.p, d_idx.p, d_idx2.p, (int)n, 0, 64, st));
        HIP_TRY(hipcub::DeviceScan::ExclusiveScan(nullptr, b1, d_end_key.p, d_prev_end.p, hipcub::Max(), (uint64_t)0, (int)nv, st));
        HIP_TRY(hipcub::DeviceScan::InclusiveScan(nullptr, b2, d_head.p, d_head.p, hipcub::Max(), (int)nv, st));
        HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, b3, d_multi.p, d_multi2.p, (int)nv, 0, 64, st));
        PC_TRY(d_tmp.reserve(std::max<size_t>(std::max(std::max(b0, b1), std::max(b2, b3)), 16)));
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, b0, d_key.p, d_key2.p, d_idx.p, d_idx2.p, (int)n, 0, 64, st));
        const unsigned gv = grid256(nv);
        hipLaunchKernelGGL(tk::k_track_end_keys, dim3(gv), dim3(256), 0, st, d_key2.p, d_idx2.p, d_line.p, nv, d_end_key.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipcub::DeviceScan::ExclusiveScan(d_tmp.p, b1, d_end_key.p, d_prev_end.p, hipcub::Max(), (uint64_t)0, (int)nv, st));
        hipLaunchKernelGGL(tk::k_track_clusters, dim3(gv), dim3(256), 0, st, d_key2.p, d_prev_end.p, nv, d_head.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipcub::DeviceScan::InclusiveScan(d_tmp.p, b2, d_head.p, d_head.p, hipcub::Max(), (int)nv, st));
        hipLaunchKernelGGL(tk::k_track_fill_short, dim3(gv), dim3(256), 0, st, d_idx2.p, d_head.p, nv, d_line.p, d_contig_of.p, d_off.p, t->cells.p, d_long.p,
                           d_multi.p, d_cnt.p);
        HIP_TRY(hipGetLastError());
        PC_TRY(read_counters(st, d_cnt, cnt));
        t->stats[4] = cnt.n_multi;
        if (cnt.n_long) {
            hipLaunchKernelGGL(tk::k_track_fill, dim3(cnt.n_long), dim3(256), 0, st, d_long.p, d_line.p, d_contig_of.p, d_off.p, t->cells.p);
            HIP_TRY(hipGetLastError());
        }
        if (cnt.n_multi) {
            HIP_TRY(hipcub::DeviceRadixSort::SortKeys(d_tmp.p, b3, d_multi.p, d_multi2.p, (int)cnt.n_multi, 0, 64, st));
            hipLaunchKernelGGL(tk::k_track_fill_ordered, dim3(cnt.n_multi), dim3(256), 0, st, d_multi2.p, cnt.n_multi, d_line.p, d_contig_of.p, d_off.p, t->cells.p);
            HIP_TRY(hipGetLastError());
        }
    }
    t->sum_valid = false;
    HIP_TRY(hipEventRecord(ev[5], st));
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    for (int k = 0; k < 5; ++k) t->ms[k] = ms_between(ev[k], ev[k + 1]);
    return PC_OK;
}

} // namespace

extern "C" {

int pc_track_create(pc_engine *e, int nstrands, int64_t min_chr_size, pc_track **out) {
    if (!e || !out || nstrands < 1 || nstrands > 8 || min_chr_size < 0) return fail(PC_ERR_ARG, "pc_track_create: bad arguments");
    pc_track *t = new pc_track();
    t->e = e; t->nstrands = nstrands; t->min_chr_size = min_chr_size;
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
    if (t->ids.count(name)) return fail(PC_ERR_ARG, "pc_track_declare: %s is declared already", name);
    const int32_t id = track_contig_id(t, name);
    t->contigs[(size_t)id].born = true;
    t->contigs[(size_t)id].length = length;
    t->order.push_back(id);
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

int pc_track_num_contigs(pc_track *t) { return t ? (int)t->order.size() : -1; }

const char *pc_track_contig_name(pc_track *t, int i) {
    if (!t || i < 0 || i >= (int)t->order.size()) return nullptr;
    return t->contigs[(size_t)t->order[(size_t)i]].name.c_str();
}

int64_t pc_track_contig_length(pc_track *t, int i) {
    if (!t || i < 0 || i >= (int)t->order.size()) return -1;
    return t->contigs[(size_t)t->order[(size_t)i]].length;
}

int64_t pc_track_contig_extent(pc_track *t, int i, int strand_slot) {
    if (!t || i < 0 || i >= (int)t->order.size() || strand_slot < 0 || strand_slot >= t->nstrands) return -1;
    return t->ext[(size_t)t->order[(size_t)i] * (size_t)t->nstrands + (size_t)strand_slot];
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
    // the items, cut on the host by the function the dense vector's item kernel runs (dense_host.h)
    std::vector<pcdense::Item> items;
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t len = end[s] - start[s];
        if (len <= 0) continue;
        if (out_step[s] != 1 && out_step[s] != -1) return fail(PC_ERR_ARG, "pc_track_gather: out_step of segment %lld is not +1 / -1", (long long)s);
        const int64_t first = out_off[s], last = out_off[s] + (int64_t)out_step[s] * (len - 1);
        if (first < 0 || first >= out_elems || last < 0 || last >= out_elems)
            return fail(PC_ERR_ARG, "pc_track_gather: segment %lld writes outside the output", (long long)s);
        pcdense::SegIn in;
        in.out_off = out_off[s]; in.len = len; in.clip_lo = 0; in.clip_hi = len; in.start = start[s]; in.step = out_step[s];
        in.known = contig[s] >= 0 && contig[s] < (int32_t)t->order.size() && strand_slot[s] >= 0 && strand_slot[s] < t->nstrands;
        if (in.known) {
            const size_t slot = (size_t)t->order[(size_t)contig[s]] * (size_t)t->nstrands + (size_t)strand_slot[s];
            in.cell_base = t->cell_off[slot];
            in.ext = t->ext[slot];
        }
        const int64_t k_end = pcdense::items_of(len);
        for (int64_t k = 0; k < k_end; ++k) items.push_back(pcdense::cut_item(in, k));
    }
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
        if (t->ncells > 0) {
            pc_engine *e = t->e;
            HIP_TRY(hipSetDevice(e->device));
            PoolScope pool_scope(&e->pool);
            hipStream_t st = e->stream;
            const int64_t nb = (t->ncells + pctrack::kSumTile - 1) / pctrack::kSumTile;
            DevBuf<double> d_partial;
            DrainOnExit drained{st};
            PC_TRY(d_partial.reserve((size_t)nb + 1));
            hipLaunchKernelGGL(pctrack::k_track_sum_partial, dim3((unsigned)nb), dim3(256), 0, st, t->cells.p, t->ncells, d_partial.p);
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
    if (strand_slot < 0 || strand_slot >= t->nstrands) return fail(PC_ERR_ARG, "pc_track_set: strand slot %d of %d", strand_slot, t->nstrands);
    // everything is checked before anything changes
    int64_t furthest = 0;
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t len = end[s] - start[s];
        if (start[s] < 0 || len < 0 || end[s] > tk::kMaxCoord) return fail(PC_ERR_ARG, "pc_track_set: segment %lld lies outside [0, 2^40]", (long long)s);
        if (values && len > 0) {
            if (val_step[s] != 1 && val_step[s] != -1) return fail(PC_ERR_ARG, "pc_track_set: val_step of segment %lld is not +1 / -1", (long long)s);
            const int64_t a = val_off[s], b = val_off[s] + (int64_t)val_step[s] * (len - 1);
            if (a < 0 || a >= nvalues || b < 0 || b >= nvalues) return fail(PC_ERR_ARG, "pc_track_set: segment %lld reads outside the vector", (long long)s);
        }
        if (len > 0) furthest = std::max(furthest, end[s]);
    }
    pc_engine *e = t->e;
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    // birth and growth, segment by segment as the reference's loop meets them (genome_array.py:1593-1608)
    const int32_t id = track_contig_id(t, contig);
    track_bear(t, id);
    for (int64_t s = 0; s < nseg; ++s) t->contigs[(size_t)id].length = tk::grown_length(t->contigs[(size_t)id].length, end[s]);
    t->sum_valid = false;
    if (furthest == 0) return PC_OK;
    std::vector<unsigned long long> far((size_t)id + 1, 0ull);
    far[(size_t)id] = (unsigned long long)furthest;
    PC_TRY(track_grow_storage(t, strand_slot, far, st));
    const size_t slot = (size_t)id * (size_t)t->nstrands + (size_t)strand_slot;
    std::vector<pcdense::Item> items;
    for (int64_t s = 0; s < nseg; ++s) {
        pcdense::SegIn in;
        in.len = end[s] - start[s];
        if (in.len <= 0) continue;
        in.out_off = values ? val_off[s] : 0; in.step = values ? val_step[s] : 1;
        in.clip_lo = 0; in.clip_hi = in.len; in.start = start[s]; in.known = true;
        in.cell_base = t->cell_off[slot]; in.ext = t->ext[slot];
        const int64_t k_end = pcdense::items_of(in.len);
        for (int64_t k = 0; k < k_end; ++k) items.push_back(pcdense::cut_item(in, k));
    }
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

namespace {
// cells of public contig i (-1: none) on strand slot s (-1: none) of t: first cell and count, -1 / 0 where t has none
void slot_cells(const pc_track *t, int i, int s, int64_t &c0, int64_t &n) {
    c0 = -1; n = 0;
    if (!t || i < 0 || i >= (int)t->order.size() || s < 0 || s >= t->nstrands) return;
    const size_t slot = (size_t)t->order[(size_t)i] * (size_t)t->nstrands + (size_t)s;
    c0 = t->cell_off[slot]; n = t->ext[slot];
}
int public_index(const pc_track *t, const std::string &name) {
    auto it = t->ids.find(name);
    if (it == t->ids.end() || !t->contigs[(size_t)it->second].born) return -1;
    for (size_t i = 0; i < t->order.size(); ++i) if (t->order[i] == it->second) return (int)i;
    return -1;
}
} // namespace

int pc_track_combine(pc_track *a, pc_track *b, double scalar, int op, int mode_all, int64_t length_pad, int nstrands_out, const int32_t *slot_a,
                     const int32_t *slot_b, pc_track **out) {
    if (!a || !out || length_pad < 0 || nstrands_out < 1 || nstrands_out > 8 || !slot_a || (b && !slot_b) || op < tk::kOpAdd || op > tk::kOpMul)
        return fail(PC_ERR_ARG, "pc_track_combine: bad arguments");
    if (b && b->e != a->e) return fail(PC_ERR_ARG, "pc_track_combine: the operands live on different engines");
    pc_engine *e = a->e;
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    // the contigs of the result: a's in a's order, then (mode all) b's remaining ones; truncate: the common ones
    struct Pick { std::string name; int ia, ib; int64_t length; };
    std::vector<Pick> picks;
    for (size_t i = 0; i < a->order.size(); ++i) {
        const pc_track::Contig &c = a->contigs[(size_t)a->order[i]];
        const int ib = b ? public_index(b, c.name) : -1;
        if (b && ib < 0 && !mode_all) continue;
        int64_t len = c.length;
        if (ib >= 0) { const int64_t lb = b->contigs[(size_t)b->order[(size_t)ib]].length; len = mode_all ? std::max(len, lb) : std::min(len, lb); }
        picks.push_back({c.name, (int)i, ib, len});
    }
    if (b && mode_all)
        for (size_t i = 0; i < b->order.size(); ++i) {
            const pc_track::Contig &c = b->contigs[(size_t)b->order[i]];
            if (public_index(a, c.name) < 0) picks.push_back({c.name, -1, (int)i, c.length});
        }
    pc_track *r = nullptr;
    PC_TRY(pc_track_create(e, nstrands_out, a->min_chr_size, &r));
    struct Undo { pc_track *r; ~Undo() { if (r) (void)pc_track_destroy(r); } } undo{r};
    std::vector<tk::OpSlot> slots;
    int64_t total = 0;
    for (const Pick &p : picks) {
        PC_TRY(pc_track_declare(r, p.name.c_str(), p.length + length_pad));
        const int32_t id = r->ids[p.name];
        for (int s = 0; s < nstrands_out; ++s) {
            tk::OpSlot o;
            slot_cells(a, p.ia, slot_a[s], o.a0, o.an);
            slot_cells(b, p.ib, b ? slot_b[s] : -1, o.b0, o.bn);
            // a scalar acts on every cell up to the length; arrays: up to the furthest cell either side stores
            o.n = b ? std::min(std::max(o.an, o.bn), p.length) : p.length;
            o.out0 = total;
            r->ext[(size_t)id * (size_t)nstrands_out + (size_t)s] = o.n;
            r->cell_off[(size_t)id * (size_t)nstrands_out + (size_t)s] = total;
            total += o.n;
            slots.push_back(o);
        }
    }
    r->ncells = total;
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
    int64_t total = 0;
    for (int64_t k = 0; k < npair; ++k) {
        tk::OpSlot o;
        slot_cells(a, contig_a[k], slot_a[k], o.a0, o.an);
        slot_cells(b, contig_b[k], slot_b[k], o.b0, o.bn);
        o.n = std::max(o.an, o.bn); o.out0 = total;
        total += o.n;
        slots.push_back(o);
    }
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
    if (strand_slot < 0 || strand_slot >= t->nstrands) return fail(PC_ERR_ARG, "pc_track_export: strand slot %d of %d", strand_slot, t->nstrands);
    pc_engine *e = t->e;
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    for (auto &x : t->ex_stats) x = 0;
    for (auto &x : t->ex_ms) x = 0.0;
    t->ex_bytes = 0;
    *bytes = 0;
    // the contigs in sorted() order of their names (code points: the bytes of UTF-8 sort alike)
    std::vector<int32_t> ids(t->order.begin(), t->order.end());
    std::sort(ids.begin(), ids.end(), [t](int32_t a, int32_t b) { return t->contigs[(size_t)a].name < t->contigs[(size_t)b].name; });
    const int K0 = (int)ids.size();
    if (K0 == 0) return PC_OK;
    if (K0 > 65535) return fail(PC_ERR_ARG, "pc_track_export: more than 65535 contigs");
    hipEvent_t ev[6] = {};
    for (auto &x : ev) HIP_TRY(hipEventCreate(&x));
    struct EvGuard { hipEvent_t *ev; ~EvGuard() { for (int i = 0; i < 6; ++i) (void)hipEventDestroy(ev[i]); } } evg{ev};
    DevBuf<tk::SlotCells> d_slots;
    DevBuf<tk::SlotStat> d_stat;
    DevBuf<double> d_partial, d_listed_val;
    DevBuf<tk::ExRange> d_ranges;
    DevBuf<uint32_t> d_flags, d_idx, d_run_e, d_listed_slot, d_n_listed;
    DevBuf<uint8_t> d_tmp, d_names, d_strs, d_lens;
    DevBuf<int64_t> d_len, d_off;
    DrainOnExit drained{st};

    // phase 1: per slot the fixed-tree sum, first and last non-zero
    std::vector<tk::SlotCells> slots((size_t)K0);
    std::vector<tk::SlotStat> stat((size_t)K0);
    int64_t max_tiles = 1;
    for (int k = 0; k < K0; ++k) {
        const size_t slot = (size_t)ids[(size_t)k] * (size_t)t->nstrands + (size_t)strand_slot;
        slots[(size_t)k].cell0 = t->cell_off[slot]; slots[(size_t)k].n = t->ext[slot];
        stat[(size_t)k].sum = 0.0; stat[(size_t)k].first = ~0ull; stat[(size_t)k].last1 = 0ull;
        max_tiles = std::max(max_tiles, (t->ext[slot] + tk::kSumTile - 1) / tk::kSumTile);
    }
    HIP_TRY(hipEventRecord(ev[0], st));
    PC_TRY(d_slots.upload(slots, st)); PC_TRY(d_stat.upload(stat, st));
    PC_TRY(d_partial.reserve((size_t)K0 * (size_t)max_tiles));
    hipLaunchKernelGGL(tk::k_export_slot_partial, dim3((unsigned)max_tiles, (unsigned)K0), dim3(256), 0, st, d_slots.p, t->cells.p, max_tiles, d_partial.p, d_stat.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(tk::k_export_slot_final, dim3((unsigned)K0), dim3(256), 0, st, d_slots.p, d_partial.p, max_tiles, d_stat.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(stat.data(), d_stat.p, stat.size() * sizeof(tk::SlotStat), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventRecord(ev[1], st));

    // the contigs that are written and their export cells
    std::vector<tk::ExRange> ranges;
    std::vector<uint8_t> names;
    int64_t E = 0;
    for (int k = 0; k < K0; ++k) {
        const tk::SlotStat &s = stat[(size_t)k];
        const bool nonzero = s.first != ~0ull;
        if (kind == 0 && !(s.sum > 0.0 && nonzero)) continue;
        const std::string &nm = t->contigs[(size_t)ids[(size_t)k]].name;
        tk::ExRange r;
        r.e0 = E; r.run_base = 0;
        r.pos0 = kind == 0 ? (int64_t)s.first : 0;
        r.n = kind == 0 ? (int64_t)(s.last1 - s.first) : slots[(size_t)k].n;
        r.cell0 = slots[(size_t)k].cell0 + r.pos0;
        r.name_off = (int32_t)names.size(); r.name_len = (int32_t)nm.size();
        names.insert(names.end(), nm.begin(), nm.end());
        E += r.n;
        ranges.push_back(r);
    }
    const int K = (int)ranges.size();
    if (K == 0) { drained.armed = false; return PC_OK; }
    if (E >= (int64_t)0x7fffffff || names.size() >= (size_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_track_export: more than 2^31 cells to export");
    { tk::ExRange end; end.e0 = E; end.n = 0; end.cell0 = 0; end.pos0 = 0; end.run_base = 0; end.name_off = 0; end.name_len = 0; ranges.push_back(end); }
    PC_TRY(d_ranges.upload(ranges, st)); PC_TRY(d_names.upload(names, st));

    // phase 2: run heads, count, exclusive sum, select
    int64_t R = 0;
    if (E > 0) {
        int rc = PC_OK;
        room(rc, d_flags, (size_t)E); room(rc, d_idx, (size_t)E);
        if (rc != PC_OK) return rc;
        hipLaunchKernelGGL(tk::k_export_flags, dim3((unsigned)((E + tk::kExportTile - 1) / tk::kExportTile)), dim3(256), 0, st, kind, d_ranges.p, K, E, t->cells.p, d_flags.p);
        HIP_TRY(hipGetLastError());
        size_t b0 = 0;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b0, d_flags.p, d_idx.p, (int)E, st));
        PC_TRY(d_tmp.reserve(std::max<size_t>(b0, 16)));
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, b0, d_flags.p, d_idx.p, (int)E, st));
        hipLaunchKernelGGL(tk::k_export_bases, dim3(grid256(K + 1)), dim3(256), 0, st, d_flags.p, d_idx.p, E, d_ranges.p, K);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&R, &d_ranges.p[K].run_base, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (R > 0) {
            PC_TRY(d_run_e.reserve((size_t)R));
            hipLaunchKernelGGL(tk::k_export_select, dim3(grid256(E)), dim3(256), 0, st, d_flags.p, d_idx.p, E, d_run_e.p);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipEventRecord(ev[2], st));

    // phase 3: the values that are not plain go to the host and come back as text
    uint32_t n_listed = 0;
    {
        int rc = PC_OK;
        room(rc, d_listed_slot, (size_t)std::max<int64_t>(R, 1)); room(rc, d_listed_val, (size_t)std::max<int64_t>(R, 1)); room(rc, d_n_listed, 1);
        if (rc != PC_OK) return rc;
    }
    if (R > 0) {
        HIP_TRY(hipMemsetAsync(d_n_listed.p, 0, sizeof(uint32_t), st));
        hipLaunchKernelGGL(tk::k_export_classify, dim3(grid256(R)), dim3(256), 0, st, d_ranges.p, K, d_run_e.p, R, t->cells.p, d_listed_slot.p, d_listed_val.p, d_n_listed.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&n_listed, d_n_listed.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    std::vector<uint8_t> strs((size_t)std::max<uint32_t>(n_listed, 1) * tk::kReprMax, 0), lens((size_t)std::max<uint32_t>(n_listed, 1), 0);
    if (n_listed) {
        std::vector<double> vals(n_listed);
        HIP_TRY(hipMemcpyAsync(vals.data(), d_listed_val.p, (size_t)n_listed * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t k = 0; k < n_listed; ++k) lens[k] = (uint8_t)tk::float_repr(vals[k], (char *)strs.data() + (size_t)tk::kReprMax * k);
    }
    PC_TRY(d_strs.upload(strs, st)); PC_TRY(d_lens.upload(lens, st));
    HIP_TRY(hipEventRecord(ev[3], st));

    // phases 4, 5: a byte length per line, their exclusive sum, the bytes
    const int64_t nlines = R + K;
    if (nlines >= (int64_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_track_export: more than 2^31 lines");
    tk::ExportView view;
    view.kind = kind; view.ranges = d_ranges.p; view.K = K; view.run_e = d_run_e.p; view.cells = t->cells.p; view.names = d_names.p;
    view.listed_slot = d_listed_slot.p; view.strs = d_strs.p; view.lens = d_lens.p;
    {
        int rc = PC_OK;
        room(rc, d_len, (size_t)nlines); room(rc, d_off, (size_t)nlines);
        if (rc != PC_OK) return rc;
    }
    const unsigned gl = (unsigned)((nlines + tk::kFormatRuns - 1) / tk::kFormatRuns);
    hipLaunchKernelGGL(tk::k_export_lengths, dim3(gl), dim3(tk::kFormatRuns), 0, st, view, nlines, d_len.p);
    HIP_TRY(hipGetLastError());
    {
        size_t b0 = 0;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b0, d_len.p, d_off.p, (int)nlines, st));
        PC_TRY(d_tmp.reserve(std::max<size_t>(b0, 16)));
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, b0, d_len.p, d_off.p, (int)nlines, st));
    }
    int64_t last_off = 0, last_len = 0;
    HIP_TRY(hipMemcpyAsync(&last_off, d_off.p + (nlines - 1), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&last_len, d_len.p + (nlines - 1), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t total = last_off + last_len;
    HIP_TRY(hipEventRecord(ev[4], st));
    PC_TRY(t->ex_text.reserve((size_t)total));
    hipLaunchKernelGGL(tk::k_export_format, dim3(gl), dim3(tk::kFormatRuns), 0, st, view, nlines, d_off.p, t->ex_text.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[5], st));
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    for (int k = 0; k < 5; ++k) t->ex_ms[k] = ms_between(ev[k], ev[k + 1]);
    t->ex_stats[0] = nlines; t->ex_stats[1] = R; t->ex_stats[2] = (int64_t)n_listed; t->ex_stats[3] = total;
    t->ex_bytes = total;
    *bytes = total;
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

// ---------------------------------------------------------------- nonzero

// counts[i * nstrands + s]: non-zero cells of public contig i on strand slot s; the indices wait for pc_track_nonzero_read
int pc_track_nonzero_count(pc_track *t, int64_t *counts) {
    if (!t || (!counts && !t->order.empty())) return fail(PC_ERR_ARG, "pc_track_nonzero_count: bad arguments");
    const int nslot = (int)t->order.size() * t->nstrands;
    for (int k = 0; k < nslot; ++k) counts[k] = 0;
    t->nz_total = 0;
    if (t->ncells == 0) return PC_OK;
    if (t->ncells >= (int64_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_track_nonzero: more than 2^31 stored cells");
    pc_engine *e = t->e;
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    // the slots that hold cells, in the order of their cells (that of the internal ids)
    const int nint = (int)(t->contigs.size() * (size_t)t->nstrands);
    std::vector<int> live;
    std::vector<int64_t> at;
    for (int k = 0; k < nint; ++k)
        if (t->ext[(size_t)k] > 0) { live.push_back(k); at.push_back(t->cell_off[(size_t)k]); }
    at.push_back(t->ncells);
    std::vector<int64_t> picked(at.size());
    const int64_t n = t->ncells;
    DevBuf<uint32_t> d_flags, d_idx;
    DevBuf<uint8_t> d_tmp;
    DevBuf<int64_t> d_at, d_picked;
    DrainOnExit drained{st};
    int rc = PC_OK;
    room(rc, d_flags, (size_t)n); room(rc, d_idx, (size_t)n); room(rc, d_picked, at.size());
    if (rc != PC_OK) return rc;
    PC_TRY(d_at.upload(at, st));
    hipLaunchKernelGGL(tk::k_track_nz_flags, dim3(grid256(n)), dim3(256), 0, st, t->cells.p, n, d_flags.p);
    HIP_TRY(hipGetLastError());
    size_t b0 = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b0, d_flags.p, d_idx.p, (int)n, st));
    PC_TRY(d_tmp.reserve(std::max<size_t>(b0, 16)));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, b0, d_flags.p, d_idx.p, (int)n, st));
    hipLaunchKernelGGL(tk::k_track_pick, dim3(grid256((int64_t)at.size())), dim3(256), 0, st, d_flags.p, d_idx.p, n, d_at.p, (int)at.size(), d_picked.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(picked.data(), d_picked.p, picked.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t total = picked.back();
    if (total > 0) {
        PC_TRY(t->nz.reserve((size_t)total));
        // (d_at: the live slots' first cells, ascending, in front of its last entry)
        hipLaunchKernelGGL(tk::k_track_nz_select, dim3(grid256(n)), dim3(256), 0, st, d_flags.p, d_idx.p, n, d_at.p, (int)live.size(), t->nz.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    drained.armed = false;
    t->nz_begin.assign((size_t)nint, 0); t->nz_cnt.assign((size_t)nint, 0);
    for (size_t j = 0; j < live.size(); ++j) { t->nz_begin[(size_t)live[j]] = picked[j]; t->nz_cnt[(size_t)live[j]] = picked[j + 1] - picked[j]; }
    for (size_t i = 0; i < t->order.size(); ++i)
        for (int s = 0; s < t->nstrands; ++s)
            counts[i * (size_t)t->nstrands + (size_t)s] = t->nz_cnt[(size_t)t->order[i] * (size_t)t->nstrands + (size_t)s];
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
    // the order of the cells (internal ids) -> public order
    const std::vector<int64_t> &cnt = t->nz_cnt, &begin = t->nz_begin;
    int64_t w = 0;
    for (size_t i = 0; i < t->order.size(); ++i)
        for (int s = 0; s < t->nstrands; ++s) {
            const size_t k = (size_t)t->order[i] * (size_t)t->nstrands + (size_t)s;
            if (cnt[k]) memcpy(out + w, all.data() + begin[k], (size_t)cnt[k] * 8);
            w += cnt[k];
        }
    t->nz.release();
    t->nz_total = -1;
    return PC_OK;
}

} // extern "C"
