// Binned summaries of a bigWig file on the GPU, host side (revision 23): pc_bigwig_summary_* of include/plastid_counts.h.
// A handle holds the file (mapped, or a copy of the image), its header, chromosome tree and zoom headers, and one TABLE
// per zoom level plus one for the items, loaded into HBM at the first query that selects it (load_zoom / load_items: the
// host walks the R-tree, the blocks go up as they are through the import's bigwig_load_blocks, their statuses come to
// the host and the first failed block is reported here (summary_load_blocks: a zoom level has no section pass that would
// find it), the items' sections go through the import's bigwig_sections, the records are gathered into file order by
// this file's kernels, k_bbi_index checks the order and gives the contigs' ranges).  A query groups its rows by
// table (bigwig_summary_host.h: choose_level) and launches k_bbi_summarize once per table in use.
// Part of the one translation unit of plastid_counts.hip (behind bigwig_decoder.hip.h, whose helpers it uses; the plumbing is device_util.hip.h).
#include <memory>

#include "bigwig_summary_kernels.hip.h"

struct pc_bigwig_summary {
    struct Table {
        bool loaded = false;
        int64_t n = 0, queries = 0;
        DevBuf<pcbws::ZoomRec> zoom;
        DevBuf<pcbws::ItemRec> items;
        pcbws::Ranges ranges;
    };
    pc_engine *e = nullptr;
    std::string path;
    MappedFile mf;
    std::vector<uint8_t> own;
    const uint8_t *image = nullptr;
    uint64_t size = 0;
    pcbw::BigWig f;
    std::vector<pcbww::ZoomHeader> levels;
    std::vector<uint32_t> reduction;
    std::vector<std::unique_ptr<Table>> tables;      // [0] the items, [1 + k] level k
    int64_t bytes_uploaded = 0, bytes_inflated = 0;
    double ms[5] = {0, 0, 0, 0, 0};                  // upload | inflate + adler | records + order check | summarize | read-back
};

static void destroy_summaries_of(pc_engine *e) {
    for (pc_bigwig_summary *s : e->summaries) delete s;
    e->summaries.clear();
}

namespace {

namespace ws = pcbws;

// What one load shares with the phases of the import it reuses.
struct SummaryLoad {
    pc_bigwig_summary *s;
    BamDecode d;
    hipStream_t st;
    LapEvents<4> ev;                   // start | uploaded | inflated + checked | records in order, indexed
    BigWigBlocks k;
    BigWigSections sec;
    std::vector<uint32_t> words;       // the blocks' statuses, then their lengths
    DevBuf<uint8_t> d_tmp;
    DevBuf<uint32_t> d_first, d_flag_runs;
    DevBuf<int64_t> d_lohi;
    explicit SummaryLoad(pc_bigwig_summary *s_) : s(s_), d{s_->e, s_->e->stream, s_->path, BamKnobs()}, st(d.st) {}
};

// The blocks of `f` (a file's, or a level's) to HBM (bigwig_load_blocks: the laps 0 and 1; no blocks: empty laps), their
// statuses and lengths to the host (x.words); the first block whose stream failed ends the load.
int summary_load_blocks(SummaryLoad &x, const bw::BigWig &f, const char *what) {
    pc_bigwig_summary *s = x.s;
    const int64_t nb = (int64_t)f.blocks.size();
    if (nb == 0) {
        for (int k = 0; k < 3; ++k) HIP_TRY(hipEventRecord(x.ev[k], x.st));
        return PC_OK;
    }
    PC_TRY(bigwig_load_blocks(x.d, s->image, f, x.ev[0], x.ev[1], x.ev[2], x.k));
    s->bytes_uploaded += (int64_t)(f.data_hi - f.data_lo);
    PC_TRY(bigwig_block_words(x.st, x.k, x.words));
    if (!f.compressed()) return PC_OK;
    for (int64_t b = 0; b < nb; ++b) {
        const uint32_t stt = x.words[(size_t)b];
        if (stt != 0u)
            return fail(PC_ERR_ARG, "%s: bigWig: %sblock %lld: %s", s->path.c_str(), what, (long long)b, bw::defect_text(stt == (uint32_t)pcbam::kInfCrc ? bw::kBwAdler : bw::kBwDeflate));
        s->bytes_inflated += x.words[(size_t)(nb + b)];
    }
    return PC_OK;
}

// The order flag and the contigs' ranges of a table of n records in HBM.
template <typename R> int summary_index(SummaryLoad &x, const R *d_recs, int64_t n, ws::Ranges &g) {
    hipStream_t st = x.st;
    const uint32_t nids = (uint32_t)x.s->f.of_id.size();
    g.lo.assign(nids, 0); g.hi.assign(nids, 0); g.ordered = true;
    if (n == 0 || nids == 0) { g.ordered = n == 0; return PC_OK; }
    int rc = PC_OK;
    room(rc, x.d_flag_runs, (size_t)nids + 1); room(rc, x.d_lohi, 2 * (size_t)nids);
    if (rc != PC_OK) return rc;
    HIP_TRY(hipMemsetAsync(x.d_flag_runs.p, 0, ((size_t)nids + 1) * 4, st));
    HIP_TRY(hipMemsetAsync(x.d_lohi.p, 0, 2 * (size_t)nids * 8, st));
    hipLaunchKernelGGL(ws::k_bbi_index<R>, dim3(grid256(n)), dim3(256), 0, st, d_recs, n, nids, x.d_flag_runs.p, x.d_flag_runs.p + 1, x.d_lohi.p, x.d_lohi.p + nids);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> flag_runs((size_t)nids + 1);
    HIP_TRY(hipMemcpyAsync(flag_runs.data(), x.d_flag_runs.p, flag_runs.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(g.lo.data(), x.d_lohi.p, (size_t)nids * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(g.hi.data(), x.d_lohi.p + nids, (size_t)nids * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    g.ordered = flag_runs[0] == 0u;
    for (uint32_t c = 0; c < nids; ++c) {
        if (flag_runs[1 + c] > 1u) g.ordered = false;
        // (the bounds a kernel will walk between: inside the table, whatever the records said)
        if (g.lo[c] < 0 || g.hi[c] > n || g.lo[c] > g.hi[c]) { g.ordered = false; g.lo[c] = 0; g.hi[c] = 0; }
    }
    return PC_OK;
}

int summary_load_zoom(SummaryLoad &x, int level, pc_bigwig_summary::Table &t) {
    pc_bigwig_summary *s = x.s;
    hipStream_t st = x.st;
    bw::BigWig blocks;
    const std::string bad = ws::level_blocks(s->image, s->size, s->f.uncompress_buf, s->levels, level, blocks);
    if (!bad.empty()) return fail(PC_ERR_ARG, "%s: bigWig: %s", s->path.c_str(), bad.c_str());
    const std::string lvl = "zoom level " + std::to_string(level) + ": ";
    const int64_t nb = (int64_t)blocks.blocks.size();
    int64_t n = 0;
    PC_TRY(summary_load_blocks(x, blocks, lvl.c_str()));
    std::vector<uint32_t> first((size_t)nb + 1, 0u);
    for (int64_t b = 0; b < nb; ++b) {
        const uint32_t len = x.words[(size_t)(nb + b)];
        if (len % pcbww::kZoomRecordBytes != 0u) return fail(PC_ERR_ARG, "%s: bigWig: %sblock %lld: not a whole number of 32-byte records", s->path.c_str(), lvl.c_str(), (long long)b);
        n += len / pcbww::kZoomRecordBytes;
        if (n >= ((int64_t)1 << 31)) return fail(PC_ERR_ARG, "%s: bigWig: %smore than 2^31 - 1 records", s->path.c_str(), lvl.c_str());
        first[(size_t)b + 1] = (uint32_t)n;
    }
    if (n > 0) {
        PC_TRY(x.d_first.upload(first, st));
        PC_TRY(t.zoom.reserve((size_t)n));
        hipLaunchKernelGGL(ws::k_bbi_zoom_records, dim3(grid256(n)), dim3(256), 0, st, x.k.data, x.k.d_off.p, x.d_first.p, nb, n, t.zoom.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));   // (first goes out of scope)
    }
    if (n != (int64_t)s->levels[(size_t)level].records)
        return fail(PC_ERR_ARG, "%s: bigWig: %sthe blocks hold %lld records, the level's count says %u", s->path.c_str(), lvl.c_str(), (long long)n, s->levels[(size_t)level].records);
    PC_TRY(summary_index(x, t.zoom.p, n, t.ranges));
    t.n = n;
    return PC_OK;
}

int summary_load_items(SummaryLoad &x, pc_bigwig_summary::Table &t) {
    pc_bigwig_summary *s = x.s;
    hipStream_t st = x.st;
    const bw::BigWig &f = s->f;
    const int64_t nb = (int64_t)f.blocks.size();
    BigWigSections &sec = x.sec;
    PC_TRY(summary_load_blocks(x, f, ""));
    if (nb > 0) {
        PC_TRY(bigwig_sections(st, x.d_tmp, s->path, x.k, nb, f.of_id, sec));
        if (sec.cnt.first_err != bw::kNoDefect) return fail(PC_ERR_ARG, "%s", bw::defect_message(s->path.c_str(), sec.cnt.first_err).c_str());
        if (sec.nitems > 0) {
            PC_TRY(t.items.reserve((size_t)sec.nitems));
            hipLaunchKernelGGL(ws::k_bbi_items, dim3(grid256(sec.nitems)), dim3(256), 0, st, x.k.data, x.k.d_off.p, sec.d_first.p, nb, sec.nitems, sec.d_ids.p, t.items.p, sec.d_cnt.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&sec.cnt, sec.d_cnt.p, sizeof(sec.cnt), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (sec.cnt.first_err != bw::kNoDefect) return fail(PC_ERR_ARG, "%s", bw::defect_message(s->path.c_str(), sec.cnt.first_err).c_str());
        }
    }
    PC_TRY(summary_index(x, t.items.p, sec.nitems, t.ranges));
    t.n = sec.nitems;
    return PC_OK;
}

// table 0: the items, 1 + k: level k.  A table that is refused stays unloaded and is tried again by the next query.
int summary_load(pc_bigwig_summary *s, int table) {
    pc_bigwig_summary::Table &t = *s->tables[(size_t)table];
    if (t.loaded) return PC_OK;
    SummaryLoad x(s);
    PC_TRY(x.ev.create());
    DrainOnExit drained{x.st};
    const int rc = table == 0 ? summary_load_items(x, t) : summary_load_zoom(x, table - 1, t);
    if (rc != PC_OK) { t.zoom.release(); t.items.release(); return rc; }
    HIP_TRY(hipEventRecord(x.ev[3], x.st));
    HIP_TRY(hipStreamSynchronize(x.st));
    drained.armed = false;
    double ms[3];
    x.ev.laps(ms, 3);
    for (int k = 0; k < 3; ++k) s->ms[k] += ms[k];
    t.loaded = true;
    return PC_OK;
}

// The handle over a copy of the image, named `path`, or (size < 0) over the file at `path`, mapped.
int summary_open_impl(pc_engine *e, const char *path, const void *image, int64_t size, pc_bigwig_summary **out) {
    std::unique_ptr<pc_bigwig_summary> s(new pc_bigwig_summary());
    s->path = path;
    if (size >= 0) {
        s->own.assign((const uint8_t *)image, (const uint8_t *)image + size);
        s->image = s->own.data(); s->size = (uint64_t)size;
    } else {
        PC_TRY(s->mf.open(path, 0, 0));
        s->image = (const uint8_t *)s->mf.p; s->size = (uint64_t)s->mf.size;
    }
    const unsigned long long d = bw::parse(s->image, s->size, s->f);
    if (d != bw::kNoDefect) return fail(PC_ERR_ARG, "%s", bw::defect_message(s->path.c_str(), d).c_str());
    const std::string bad = pcbww::zoom_headers(s->image, s->size, s->levels);
    if (!bad.empty()) return fail(PC_ERR_ARG, "%s: bigWig: %s", s->path.c_str(), bad.c_str());
    for (const pcbww::ZoomHeader &z : s->levels) s->reduction.push_back(z.reduction);
    for (size_t k = 0; k < s->levels.size() + 1; ++k) {
        s->tables.emplace_back(new pc_bigwig_summary::Table());
        s->tables.back()->zoom.pool = &e->pool; s->tables.back()->items.pool = &e->pool;
    }
    s->e = e;
    e->summaries.push_back(s.get());
    *out = s.release();
    return PC_OK;
}

}   // namespace

extern "C" {

int pc_bigwig_summary_open(pc_engine *e, const void *image, int64_t size, const char *name, pc_bigwig_summary **out) {
    if (!e || !out || size < 0 || (size > 0 && !image)) return fail(PC_ERR_ARG, "pc_bigwig_summary_open: bad arguments");
    return summary_open_impl(e, name ? name : "<memory>", image, size, out);
}

int pc_bigwig_summary_open_path(pc_engine *e, const char *path, pc_bigwig_summary **out) {
    if (!e || !out || !path) return fail(PC_ERR_ARG, "pc_bigwig_summary_open_path: bad arguments");
    return summary_open_impl(e, path, nullptr, -1, out);
}

int pc_bigwig_summary_close(pc_bigwig_summary *s) {
    if (!s) return PC_OK;
    (void)hipSetDevice(s->e->device);
    (void)hipStreamSynchronize(s->e->stream);
    auto &list = s->e->summaries;
    list.erase(std::remove(list.begin(), list.end(), s), list.end());
    delete s;
    return PC_OK;
}

int pc_bigwig_summary_query(pc_bigwig_summary *s, int64_t nq, const int32_t *contig, const int64_t *start, const int64_t *end, int64_t n_bins, double *out5) {
    if (!s || nq < 0 || (nq > 0 && (!contig || !start || !end || !out5))) return fail(PC_ERR_ARG, "pc_bigwig_summary_query: bad arguments");
    const std::string bad = ws::check_queries(nq, start, end, n_bins);
    if (!bad.empty()) return fail(PC_ERR_ARG, "pc_bigwig_summary_query: %s", bad.c_str());
    for (double &v : s->ms) v = 0.0;
    if (nq == 0) return PC_OK;
    if (nq >= ((int64_t)1 << 31) / n_bins) return fail(PC_ERR_ARG, "pc_bigwig_summary_query: %lld queries of %lld bins are 2^31 elements or more", (long long)nq, (long long)n_bins);
    const int64_t total = nq * n_bins;
    pc_engine *e = s->e;
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    // the rows of every table, in the caller's order
    const size_t ntab = s->tables.size();
    std::vector<std::vector<ws::DevQuery>> rows(ntab);
    for (int64_t q = 0; q < nq; ++q) {
        if (contig[q] < 0 || contig[q] >= (int32_t)s->f.chroms.size()) continue;
        const int level = ws::choose_level(s->reduction.data(), (int)s->reduction.size(), (uint32_t)start[q], (uint32_t)end[q], (uint32_t)n_bins);
        rows[(size_t)(level + 1)].push_back(ws::DevQuery{(uint32_t)start[q], (uint32_t)end[q], (int64_t)contig[q], 0, q});   // (lo: the contig, until the table is there)
    }
    for (size_t k = 0; k < ntab; ++k) {
        if (rows[k].empty()) continue;
        PC_TRY(summary_load(s, (int)k));
        pc_bigwig_summary::Table &t = *s->tables[k];
        if (!t.ranges.ordered) return fail(PC_ERR_ARG, "%s: bigWig: %s", s->path.c_str(), ws::kOrderText);
        for (ws::DevQuery &r : rows[k]) {
            const uint32_t id = s->f.chroms[(size_t)r.lo].id;
            r.lo = t.ranges.lo[id]; r.hi = t.ranges.hi[id];
        }
    }
    LapEvents<3> ev;                   // start | summarized | read back
    PC_TRY(ev.create());
    DevBuf<double> d_out;
    DevBuf<ws::DevQuery> d_rows;
    DrainOnExit drained{st};
    size_t most = 1;
    for (const auto &r : rows) most = std::max(most, r.size());
    int rc = PC_OK;
    room(rc, d_out, 5 * (size_t)total); room(rc, d_rows, most);
    if (rc != PC_OK) return rc;
    HIP_TRY(hipEventRecord(ev[0], st));
    HIP_TRY(hipMemsetAsync(d_out.p, 0, 5 * (size_t)total * sizeof(double), st));   // (rows without a contig: no data)
    for (size_t k = 0; k < ntab; ++k) {
        if (rows[k].empty()) continue;
        pc_bigwig_summary::Table &t = *s->tables[k];
        t.queries += (int64_t)rows[k].size();
        const int64_t nlanes = (int64_t)rows[k].size() * n_bins;
        // (one buffer for the rows of every table: the stream orders the copy behind the launch before it)
        HIP_TRY(hipMemcpyAsync(d_rows.p, rows[k].data(), rows[k].size() * sizeof(ws::DevQuery), hipMemcpyHostToDevice, st));
        if (k == 0) hipLaunchKernelGGL(ws::k_bbi_summarize<ws::ItemRec>, dim3(grid256(nlanes)), dim3(256), 0, st, (const ws::ItemRec *)t.items.p, d_rows.p, nlanes, (uint32_t)n_bins, total, d_out.p);
        else hipLaunchKernelGGL(ws::k_bbi_summarize<ws::ZoomRec>, dim3(grid256(nlanes)), dim3(256), 0, st, (const ws::ZoomRec *)t.zoom.p, d_rows.p, nlanes, (uint32_t)n_bins, total, d_out.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev[1], st));
    HIP_TRY(hipMemcpyAsync(out5, d_out.p, 5 * (size_t)total * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ev[2], st));
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    ev.laps(s->ms + 3, 2);
    return PC_OK;
}

int pc_bigwig_summary_stats(pc_bigwig_summary *s, int64_t *out4, int max_tables, int64_t *out3) {
    if (!s || !out4 || max_tables < 0 || (max_tables > 0 && !out3)) return fail(PC_ERR_ARG, "pc_bigwig_summary_stats: bad arguments");
    int64_t loaded = 0;
    for (const auto &t : s->tables) loaded += t->loaded ? 1 : 0;
    out4[0] = (int64_t)s->tables.size(); out4[1] = loaded; out4[2] = s->bytes_uploaded; out4[3] = s->bytes_inflated;
    for (size_t k = 0; k < s->tables.size() && k < (size_t)max_tables; ++k) {
        out3[3 * k] = k == 0 ? 0 : (int64_t)s->reduction[k - 1];
        out3[3 * k + 1] = s->tables[k]->loaded ? s->tables[k]->n : -1;
        out3[3 * k + 2] = s->tables[k]->queries;
    }
    return PC_OK;
}

int pc_bigwig_summary_timing(pc_bigwig_summary *s, double *ms5) {
    if (!s || !ms5) return fail(PC_ERR_ARG, "pc_bigwig_summary_timing: bad arguments");
    for (int k = 0; k < 5; ++k) ms5[k] = s->ms[k];
    return PC_OK;
}

}   // extern "C"
