// Count tracks on the GPU, host side: the pc_track_* entry points of include/plastid_counts.h.  A pc_track is the
// reference's GenomeArray (plastid/genomics/genome_array.py:1323-1533) as a read-and-count object: float64 cells per
// (contig, strand slot) in one block of HBM, filled by pc_track_add_text / _path (add_from_wiggle, :1978-1994) and read by
// pc_track_gather.  One import is six phases (track_add_impl): upload, line starts (both shared with SAM text),
// classify + state records, fields (+ the host's conversion of the escaped lines), growth and storage, sort + apply.
// The host looks at the state lines, the escaped lines and the growth lines only.
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
        for (auto &b : born) { t->contigs[(size_t)b.second].born = true; t->contigs[(size_t)b.second].length = t->min_chr_size; t->order.push_back(b.second); }
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
                if (x.stop >= len) len = x.stop + 10000;
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
    t->cells.pool = &e->pool;
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

} // extern "C"
