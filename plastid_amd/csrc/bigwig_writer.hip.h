// Writing bigWig files from HBM, host side (revision 21): pc_track_export_bigwig / _zoom / _read / pc_track_bigwig_export_stats /
// _block_types / _timing / _zoom_stats / _zoom_timing and pc_track_set_length of include/plastid_counts.h.  One export is a BigWigExport taken through its phases:
//   1  item heads over the cells of the strand's contigs in sorted order, their exclusive sum, the items in front of
//      every contig (one read-back of a word per contig: the host cuts the sections from it);
//   2  the items into their columns and into the raw sections, the section headers, the total summary;
//   3  k_zlib_deflate over the raw sections (compress), 4 the sizes, their exclusive sum, the compaction: the encode
//      stage of deflate_encoder.hip.h (zlib_encode_stage), which the zoom levels' blocks go through as well -- a
//      BwxBlocks each, the raw blocks, their bounds and the stage's buffers;
//   Z  (zoom != 0, the file has items) the zoom levels from the item columns of phase 2 (bigwig_zoom_kernels.hip.h): the
//      window grid of all candidate levels (bigwig_write_host.h: zoom_plan), level 0, the levels above it, the flags'
//      exclusive sum; the records in front of every (level, contig) come back (one word each: the host ends the pyramid
//      and cuts the blocks by them); the records into raw blocks, the block table, the encode stage over the blocks
//      (compress);
//   5  the section table (bounds and sizes) and the zoom levels' block table come back (bwx_read_table), the host lays out offsets and
//      all trees (bigwig_write_host.h: the container code of the host writer), and the blocks cross PCIe once, straight
//      into their place in the image -- through the transfer ring when they are large.
// What is refused is refused before anything is built, and nothing is left behind.
// Part of the one translation unit of plastid_counts.hip (behind deflate_encoder.hip.h; the plumbing is device_util.hip.h).
#include "bigwig_write_kernels.hip.h"
#include "bigwig_zoom_kernels.hip.h"

namespace {

namespace ww = pcbww;

// One set of blocks of the file -- the data sections, or the blocks of all zoom levels: the raw blocks back to back,
// every block's bounds, the encode stage over them (compress; its d_in is filled with the raw blocks' places), and the
// table as bwx_read_table brings it back.
struct BwxBlocks {
    DevBuf<uint8_t> d_raw;
    DevBuf<uint32_t> d_start, d_end;
    ZlibEncodeStage z;
    std::vector<uint32_t> start, end, fell_back;
    std::vector<unsigned long long> sizes;
    const uint8_t *bytes(bool compress) const { return compress ? z.d_out.p : d_raw.p; }   // the blocks as the file holds them
};

struct BigWigExport {
    pc_track *t;
    int strand;
    uint32_t items_per_slot, block_size;
    int compress;                          // 0: stored sections, else the encoder's mode (pcdeflate::kFixed, kDynamic)
    hipStream_t st;
    LapEvents<5> ev;                       // start | items known | sections + summary | encoded | compacted
    tk::ExportSlots slots;                 // the contigs in sorted order and their cells
    std::vector<ww::WContig> contigs;
    std::vector<tk::ExRange> ranges;       // one per contig and the sentinel
    int K = 0;
    int64_t E = 0, N = 0, nsec = 0, raw_bytes = 0, block_bytes = 0, stored = 0, fixed = 0, dynamic = 0;
    std::vector<int64_t> sec_first;        // sections in front of every contig
    std::vector<ww::DevSection> sections;
    ww::DevSummary total = {0ull, ww::kNoKeyMin, ww::kNoKeyMax, 0.0, 0.0};
    DevBuf<tk::ExRange> d_ranges;
    DevBuf<uint32_t> d_flags, d_idx, d_istart, d_iend;
    DevBuf<float> d_ival;
    DevBuf<int64_t> d_sec_first;
    DevBuf<ww::DevSection> d_sections;
    DevBuf<ww::DevSummary> d_summary;      // the total, then the partials
    DevBuf<uint8_t> d_tmp;
    BwxBlocks sec;                         // the data sections
    // the zoom levels
    int64_t zoom = 0;                      // 0: none, -1: the automatic first reduction, else the first reduction
    LapEvents<5> zev;                      // start | level 0 | levels above | records + block table | encoded + compacted
    ww::ZoomPlan zplan;
    int zlevels = 0;                       // the levels written
    int64_t zrecords = 0, znblk = 0;       // their records and blocks
    std::vector<int64_t> zrec;             // the records in front of every (level, contig)
    std::vector<ww::ZoomBlock> zblk;       // the blocks of the written levels, level by level
    std::vector<int64_t> zblk_first;       // the blocks in front of every written level, and their number
    DevBuf<int64_t> d_zrows, d_zitem_first, d_zrec;
    DevBuf<uint32_t> d_zsizes, d_zvalid, d_zkmin, d_zkmax, d_zflags, d_zidx;
    DevBuf<double> d_zsum, d_zsumsq;
    DevBuf<ww::ZoomBlock> d_zblk;
    BwxBlocks zb;                          // the blocks of the written levels
};

// Phase 1: heads, exclusive sum, items in front of every contig; the host cuts the sections.
int bwx_items_and_sections(BigWigExport &c) {
    hipStream_t st = c.st;
    HIP_TRY(hipEventRecord(c.ev[0], st));
    if (c.E > 0) {
        int rc = PC_OK;
        room(rc, c.d_flags, (size_t)c.E); room(rc, c.d_idx, (size_t)c.E);
        if (rc != PC_OK) return rc;
        PC_TRY(c.d_ranges.upload(c.ranges, st));
        hipLaunchKernelGGL(ww::k_bww_flags, dim3((unsigned)((c.E + tk::kExportTile - 1) / tk::kExportTile)), dim3(256), 0, st, c.d_ranges.p, c.K, c.E, c.t->cells.p, c.d_flags.p);
        HIP_TRY(hipGetLastError());
        PC_TRY(cub_run(c.d_tmp, [&](void *tmp, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(tmp, b, c.d_flags.p, c.d_idx.p, (int)c.E, st); }));
        hipLaunchKernelGGL(tk::k_export_bases, dim3(grid256(c.K + 1)), dim3(256), 0, st, c.d_flags.p, c.d_idx.p, c.E, c.d_ranges.p, c.K);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c.ranges.data(), c.d_ranges.p, c.ranges.size() * sizeof(tk::ExRange), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        c.N = c.ranges[(size_t)c.K].run_base;
    }
    c.sec_first.assign((size_t)c.K + 1, 0);
    for (int k = 0; k < c.K; ++k) {
        const int64_t first = c.ranges[(size_t)k].run_base, cnt = c.ranges[(size_t)k + 1].run_base - first;
        c.sec_first[(size_t)k] = (int64_t)c.sections.size();
        for (int64_t a = 0; a < cnt; a += c.items_per_slot)
            c.sections.push_back({(uint32_t)k, (uint32_t)std::min<int64_t>(c.items_per_slot, cnt - a), (uint64_t)(first + a)});
    }
    c.nsec = (int64_t)c.sections.size();
    c.sec_first[(size_t)c.K] = c.nsec;
    c.raw_bytes = 24 * c.nsec + 12 * c.N;
    HIP_TRY(hipEventRecord(c.ev[1], st));
    return PC_OK;
}

// Phase 2: the items, the section headers, the total summary.
int bwx_fill_sections(BigWigExport &c) {
    hipStream_t st = c.st;
    const int64_t ntile = (c.N + ww::kSummaryTile - 1) / ww::kSummaryTile;
    int rc = PC_OK;
    room(rc, c.d_istart, (size_t)c.N); room(rc, c.d_iend, (size_t)c.N); room(rc, c.d_ival, (size_t)c.N); room(rc, c.sec.d_raw, (size_t)c.raw_bytes + 64);
    room(rc, c.sec.d_start, (size_t)c.nsec); room(rc, c.sec.d_end, (size_t)c.nsec); room(rc, c.sec.z.d_in, 2 * (size_t)c.nsec); room(rc, c.d_summary, 1 + (size_t)ntile);
    if (rc != PC_OK) return rc;
    PC_TRY(c.d_sec_first.upload(c.sec_first, st)); PC_TRY(c.d_sections.upload(c.sections, st));
    HIP_TRY(hipMemcpyAsync(c.d_summary.p, &c.total, sizeof(c.total), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ww::k_bww_items, dim3((unsigned)((c.E + tk::kExportTile - 1) / tk::kExportTile)), dim3(256), 0, st, c.d_ranges.p, c.K, c.E, c.t->cells.p, c.d_flags.p,
                       c.d_idx.p, c.d_sec_first.p, c.items_per_slot, c.d_istart.p, c.d_iend.p, c.d_ival.p, c.sec.d_raw.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ww::k_bww_headers, dim3(grid256(c.nsec)), dim3(256), 0, st, c.d_sections.p, c.nsec, c.d_istart.p, c.d_iend.p, c.sec.d_raw.p, c.sec.d_start.p, c.sec.d_end.p,
                       c.sec.z.d_in.p, c.sec.z.d_in.p + c.nsec);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ww::k_bww_summary, dim3((unsigned)ntile), dim3(256), 0, st, c.d_istart.p, c.d_iend.p, c.d_ival.p, c.N, c.d_summary.p + 1, c.d_summary.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ww::k_bww_summary_final, dim3(1), dim3(256), 0, st, c.d_summary.p + 1, ntile, c.d_summary.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&c.total, c.d_summary.p, sizeof(c.total), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(c.ev[2], st));
    return PC_OK;
}

// Phase Z: the zoom levels.  The item columns of phase 2 are in place; c.total has arrived when the stream has drained.
int bwx_zoom(BigWigExport &c) {
    hipStream_t st = c.st;
    HIP_TRY(hipStreamSynchronize(st));     // (the total summary: the automatic first reduction reads it)
    const std::string bad = ww::zoom_plan(c.contigs, ww::zoom_first_reduction(c.zoom, (uint64_t)c.N, (uint64_t)c.total.valid), c.zplan);
    if (!bad.empty()) return fail(PC_ERR_ARG, "pc_track_export_bigwig: %s", bad.c_str());
    const ww::ZoomGrid &g = c.zplan.g;
    const int64_t W = c.zplan.windows(), nrow = (int64_t)c.zplan.rows.size();
    std::vector<uint32_t> sizes((size_t)c.K);
    std::vector<int64_t> item_first((size_t)c.K + 1);
    for (int k = 0; k < c.K; ++k) sizes[(size_t)k] = c.contigs[(size_t)k].size;
    for (int k = 0; k <= c.K; ++k) item_first[(size_t)k] = c.ranges[(size_t)k].run_base;
    DrainOnExit drained{st};               // (sizes and item_first are read by what is queued below)
    int rc = PC_OK;
    room(rc, c.d_zvalid, (size_t)W); room(rc, c.d_zkmin, (size_t)W); room(rc, c.d_zkmax, (size_t)W); room(rc, c.d_zsum, (size_t)W); room(rc, c.d_zsumsq, (size_t)W);
    room(rc, c.d_zflags, (size_t)W + 1); room(rc, c.d_zidx, (size_t)W + 1); room(rc, c.d_zrec, (size_t)nrow);
    if (rc != PC_OK) return rc;
    PC_TRY(c.d_zrows.upload(c.zplan.rows, st)); PC_TRY(c.d_zsizes.upload(sizes, st)); PC_TRY(c.d_zitem_first.upload(item_first, st));
    const ww::ZoomColumns col{c.d_zvalid.p, c.d_zkmin.p, c.d_zkmax.p, c.d_zsum.p, c.d_zsumsq.p};
    HIP_TRY(hipEventRecord(c.zev[0], st));
    hipLaunchKernelGGL(ww::k_bwz_level0, dim3(grid256(g.level_off[1])), dim3(256), 0, st, g, c.d_zrows.p, c.d_zsizes.p, c.d_zitem_first.p, c.d_istart.p, c.d_iend.p, c.d_ival.p,
                       col, c.d_zflags.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c.zev[1], st));
    for (int k = 1; k < g.levels; ++k) {
        hipLaunchKernelGGL(ww::k_bwz_reduce, dim3(grid256(g.level_off[k + 1] - g.level_off[k])), dim3(256), 0, st, g, k, c.d_zrows.p, col, c.d_zflags.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(c.zev[2], st));
    HIP_TRY(hipMemsetAsync(c.d_zflags.p + W, 0, 4, st));
    PC_TRY(cub_run(c.d_tmp, [&](void *tmp, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(tmp, b, c.d_zflags.p, c.d_zidx.p, (int)(W + 1), st); }));
    hipLaunchKernelGGL(ww::k_bwz_bases, dim3(grid256(nrow)), dim3(256), 0, st, c.d_zrows.p, nrow, c.d_zidx.p, c.d_zrec.p);
    HIP_TRY(hipGetLastError());
    c.zrec.resize((size_t)nrow);
    HIP_TRY(hipMemcpyAsync(c.zrec.data(), c.d_zrec.p, (size_t)nrow * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c.zlevels = ww::zoom_levels_written(c.zplan, c.zrec);
    c.zrecords = c.zrec[(size_t)(c.zlevels - 1) * (size_t)(c.K + 1) + (size_t)c.K];
    for (int k = 0; k < c.zlevels; ++k) {
        c.zblk_first.push_back((int64_t)c.zblk.size());
        ww::zoom_cut_blocks(c.zplan, c.zrec, k, ww::zoom_block_records(c.items_per_slot), c.zblk);
    }
    c.znblk = (int64_t)c.zblk.size();
    c.zblk_first.push_back(c.znblk);
    room(rc, c.zb.d_raw, (size_t)c.zrecords * ww::kZoomRecordBytes + 64); room(rc, c.zb.d_start, (size_t)c.znblk); room(rc, c.zb.d_end, (size_t)c.znblk);
    room(rc, c.zb.z.d_in, 2 * (size_t)c.znblk);
    if (rc != PC_OK) return rc;
    PC_TRY(c.d_zblk.upload(c.zblk, st));
    hipLaunchKernelGGL(ww::k_bwz_records, dim3(grid256(g.level_off[c.zlevels])), dim3(256), 0, st, g, g.level_off[c.zlevels], c.d_zrows.p, c.d_zsizes.p, col, c.d_zflags.p,
                       c.d_zidx.p, c.zb.d_raw.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ww::k_bwz_blocks, dim3(grid256(c.znblk)), dim3(256), 0, st, c.d_zblk.p, c.znblk, c.zb.d_raw.p, c.zb.d_start.p, c.zb.d_end.p, c.zb.z.d_in.p,
                       c.zb.z.d_in.p + c.znblk);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c.zev[3], st));
    if (c.compress)
        PC_TRY(zlib_encode_stage(st, c.zb.d_raw.p, c.znblk, [&c](int64_t b) { return (uint64_t)ww::kZoomRecordBytes * c.zblk[(size_t)b].count; }, (uint32_t)c.compress, c.d_tmp, c.zb.z, nullptr,
                                 c.zev[4]));
    else HIP_TRY(hipEventRecord(c.zev[4], st));
    drained.armed = false;                 // (the stream has drained behind the record counts' read-back)
    return PC_OK;
}

// The table of n blocks comes back: their bounds and (compress) their streams' sizes and, where the caller counts the
// block types, how far their blocks fell back.  Queued on `st`: the caller waits.
int bwx_read_table(hipStream_t st, BwxBlocks &b, int64_t n, int compress, bool types) {
    b.start.resize((size_t)n); b.end.resize((size_t)n); b.sizes.resize((size_t)n); b.fell_back.resize((size_t)n);
    if (n == 0) return PC_OK;
    HIP_TRY(hipMemcpyAsync(b.start.data(), b.d_start.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(b.end.data(), b.d_end.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (compress) HIP_TRY(hipMemcpyAsync(b.sizes.data(), b.z.d_res.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    if (compress && types) HIP_TRY(hipMemcpyAsync(b.fell_back.data(), b.z.d_stored.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    return PC_OK;
}

// Phase 5: the block tables come back, the host lays the file out, the blocks land in their place.
int bwx_layout_and_read(BigWigExport &c) {
    hipStream_t st = c.st;
    pc_track *t = c.t;
    const auto t0 = std::chrono::steady_clock::now();
    PC_TRY(bwx_read_table(st, c.zb, c.znblk, c.compress, false));
    PC_TRY(bwx_read_table(st, c.sec, c.nsec, c.compress, true));
    if (c.nsec > 0) HIP_TRY(hipStreamSynchronize(st));
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<ww::WSection> sections((size_t)c.nsec);
    uint32_t largest = 0;
    for (int64_t s = 0; s < c.nsec; ++s) {
        const uint32_t raw = 24u + 12u * c.sections[(size_t)s].count;
        sections[(size_t)s] = {c.sections[(size_t)s].chrom, c.sec.start[(size_t)s], c.sec.end[(size_t)s], c.compress ? (uint64_t)c.sec.sizes[(size_t)s] : (uint64_t)raw};
        largest = std::max(largest, raw);
        if (c.compress) {
            const uint32_t type = (uint32_t)c.compress - c.sec.fell_back[(size_t)s];     // (the encoder reports the steps its block fell back)
            c.stored += type == pcdeflate::kStored; c.fixed += type == pcdeflate::kFixed; c.dynamic += type == pcdeflate::kDynamic;
        }
    }
    ww::Summary sm;
    sm.valid = c.total.valid; sm.kmin = c.total.kmin; sm.kmax = c.total.kmax; sm.sum = c.total.sum; sm.sumsq = c.total.sumsq;
    // the zoom levels: every block's bounds and bytes, level by level
    std::vector<ww::ZoomLevel> levels((size_t)c.zlevels);
    for (int k = 0; k < c.zlevels; ++k) {
        const size_t row = (size_t)k * (size_t)(c.K + 1);
        levels[(size_t)k].reduction = c.zplan.g.r[k];
        levels[(size_t)k].records = (uint64_t)(c.zrec[row + (size_t)c.K] - c.zrec[row]);
        int64_t *zs = t->bwz_stats[k];
        zs[0] = c.zplan.g.r[k]; zs[1] = (int64_t)levels[(size_t)k].records; zs[2] = c.zblk_first[(size_t)k + 1] - c.zblk_first[(size_t)k]; zs[3] = zs[1] * (int64_t)ww::kZoomRecordBytes; zs[4] = 0;
        for (int64_t b = c.zblk_first[(size_t)k]; b < c.zblk_first[(size_t)k + 1]; ++b) {
            const uint32_t raw = ww::kZoomRecordBytes * c.zblk[(size_t)b].count;
            levels[(size_t)k].blocks.push_back({c.zblk[(size_t)b].chrom, c.zb.start[(size_t)b], c.zb.end[(size_t)b], c.compress ? (uint64_t)c.zb.sizes[(size_t)b] : (uint64_t)raw});
            zs[4] += (int64_t)levels[(size_t)k].blocks.back().size;
            largest = std::max(largest, raw);
        }
    }
    t->bwz_levels = c.zlevels;
    ww::Container box;
    ww::build_container(c.contigs, sections, c.block_size, c.compress ? largest : 0u, c.N > 0 ? &sm : nullptr, box, levels);
    c.block_bytes = (int64_t)box.block_bytes;
    t->bwx_image.resize((size_t)box.total());
    // the host's pieces into their places; the blocks' places and where they stand in HBM
    std::vector<TransferJob> job;
    size_t at = 0, most = 0;
    auto host_piece = [&](const std::vector<uint8_t> &v) { memcpy(t->bwx_image.data() + at, v.data(), v.size()); at += v.size(); };
    auto block_piece = [&](const uint8_t *src, uint64_t bytes) {
        if (bytes) job.push_back({t->bwx_image.data() + at, src, (size_t)bytes});
        at += (size_t)bytes; most = std::max(most, (size_t)bytes);
    };
    host_piece(box.front);
    block_piece(c.sec.bytes(c.compress), box.block_bytes);
    host_piece(box.back);
    uint64_t zat = 0;
    for (int k = 0; k < c.zlevels; ++k) {
        host_piece(box.zoom[(size_t)k].front);
        block_piece(c.zb.bytes(c.compress) + zat, box.zoom[(size_t)k].block_bytes);
        zat += box.zoom[(size_t)k].block_bytes;
        host_piece(box.zoom[(size_t)k].back);
    }
    const auto t2 = std::chrono::steady_clock::now();
    if (!job.empty()) {
        const char *knob = getenv("PC_STAGE_SLICE");   // (test knob: the ring for every size, in pieces of so many 4 KiB pages)
        if (most >= 4 * TransferRing::kPiece || knob) {
            const size_t piece = knob ? (size_t)std::max<int64_t>(1, std::min<int64_t>(atoll(knob), 4096)) * 4096 : TransferRing::kPiece;
            PC_TRY(TransferRing::of(t->e->device).run(t->e->device, job, piece, knob != nullptr, true));
        } else {
            for (const TransferJob &j : job) HIP_TRY(hipMemcpyAsync(j.dst, j.src, j.bytes, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
    }
    const auto t3 = std::chrono::steady_clock::now();
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    t->bwx_ms[4] = ms(t0, t1) + ms(t2, t3); t->bwx_ms[5] = ms(t1, t2);
    return PC_OK;
}

}   // namespace

extern "C" {

int pc_track_export_bigwig(pc_track *t, int strand_slot, int64_t items_per_slot, int64_t block_size, int compress, int64_t *bytes) {
    return pc_track_export_bigwig_zoom(t, strand_slot, items_per_slot, block_size, compress, 0, bytes);
}

int pc_track_export_bigwig_zoom(pc_track *t, int strand_slot, int64_t items_per_slot, int64_t block_size, int compress, int64_t zoom, int64_t *bytes) {
    if (!t || !bytes) return fail(PC_ERR_ARG, "pc_track_export_bigwig: bad arguments");
    if (strand_slot < 0 || strand_slot >= t->tab.nstrands) return fail(PC_ERR_ARG, "pc_track_export_bigwig: strand slot %d of %d", strand_slot, t->tab.nstrands);
    const std::string bad = ww::check_params(items_per_slot, block_size);
    if (!bad.empty()) return fail(PC_ERR_ARG, "pc_track_export_bigwig: %s", bad.c_str());
    if (compress < 0 || compress > 2) return fail(PC_ERR_ARG, "pc_track_export_bigwig: compress %d is none of 0 (stored sections), 1 (fixed codes), 2 (dynamic codes)", compress);
    const std::string bad_zoom = ww::check_zoom(zoom);
    if (!bad_zoom.empty()) return fail(PC_ERR_ARG, "pc_track_export_bigwig: %s", bad_zoom.c_str());
    pc_engine *e = t->e;
    BigWigExport c{t, strand_slot, (uint32_t)items_per_slot, (uint32_t)block_size, compress, e->stream};
    c.zoom = zoom;
    c.slots = t->tab.export_slots(strand_slot);
    c.K = (int)c.slots.ids.size();
    for (int k = 0; k < c.K; ++k) {
        const int32_t id = c.slots.ids[(size_t)k];
        const int64_t size = std::max(t->tab.length[(size_t)id], c.slots.cells[(size_t)k].n);
        if (size >= ((int64_t)1 << 32)) return fail(PC_ERR_ARG, "pc_track_export_bigwig: contig %s has 2^32 positions or more", t->tab.names[(size_t)id].c_str());
        c.contigs.push_back({t->tab.names[(size_t)id], (uint32_t)size});
        c.ranges.push_back(tk::ExRange{c.E, c.slots.cells[(size_t)k].n, c.slots.cells[(size_t)k].cell0, 0, 0, 0, 0});
        c.E += c.slots.cells[(size_t)k].n;
    }
    c.ranges.push_back(tk::ExRange{c.E, 0, 0, 0, 0, 0, 0});
    // (the scans count in int: a strand of 2^31 - 1 cells or more could hold 2^31 items, and is refused as a whole)
    if (c.E >= (int64_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_track_export_bigwig: 2^31 - 1 cells or more on the strand: the items are counted in 31 bits");
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    for (auto &x : t->bwx_stats) x = 0;
    for (auto &x : t->bwx_ms) x = 0.0;
    for (auto &x : t->bwz_ms) x = 0.0;
    t->bwz_levels = 0;
    t->bwx_bytes = -1;
    std::vector<uint8_t>().swap(t->bwx_image);
    *bytes = 0;
    PC_TRY(c.ev.create());
    if (c.zoom) PC_TRY(c.zev.create());
    DrainOnExit drained{c.st};
    PC_TRY(bwx_items_and_sections(c));
    if (c.N > 0) PC_TRY(bwx_fill_sections(c)); else HIP_TRY(hipEventRecord(c.ev[2], c.st));
    if (c.N > 0 && c.compress)             // phases 3, 4: every raw section through the encode stage
        PC_TRY(zlib_encode_stage(c.st, c.sec.d_raw.p, c.nsec, [&c](int64_t s) { return 24u + 12u * (uint64_t)c.sections[(size_t)s].count; }, (uint32_t)c.compress, c.d_tmp, c.sec.z, c.ev[3]));
    else HIP_TRY(hipEventRecord(c.ev[3], c.st));
    HIP_TRY(hipEventRecord(c.ev[4], c.st));
    const bool zoomed = c.zoom && c.N > 0;      // (a file without items has no levels)
    if (zoomed) PC_TRY(bwx_zoom(c));
    HIP_TRY(hipStreamSynchronize(c.st));
    const int rc = bwx_layout_and_read(c);
    if (rc != PC_OK) { std::vector<uint8_t>().swap(t->bwx_image); t->bwz_levels = 0; return rc; }
    drained.armed = false;
    c.ev.laps(t->bwx_ms, 4);
    if (zoomed) c.zev.laps(t->bwz_ms, 4);
    t->bwx_stats[0] = c.K; t->bwx_stats[1] = c.N; t->bwx_stats[2] = c.nsec; t->bwx_stats[3] = c.raw_bytes; t->bwx_stats[4] = c.block_bytes; t->bwx_stats[5] = c.stored; t->bwx_stats[6] = c.fixed; t->bwx_stats[7] = c.dynamic;
    t->bwx_bytes = (int64_t)t->bwx_image.size();
    *bytes = t->bwx_bytes;
    return PC_OK;
}

int pc_track_set_length(pc_track *t, const char *name, int64_t length) {
    if (!t || !name || length < 0) return fail(PC_ERR_ARG, "pc_track_set_length: bad arguments");
    const int i = t->tab.public_index(name);
    if (i < 0) return fail(PC_ERR_ARG, "pc_track_set_length: the track holds no contig %s", name);
    t->tab.length[(size_t)t->tab.public_id(i)] = length;
    return PC_OK;
}

int pc_track_export_bigwig_read(pc_track *t, void *dst, int64_t bytes) {
    if (!t || t->bwx_bytes < 0 || bytes != t->bwx_bytes || (bytes > 0 && !dst)) return fail(PC_ERR_ARG, "pc_track_export_bigwig_read: no exported file of this size");
    if (bytes > 0) memcpy(dst, t->bwx_image.data(), (size_t)bytes);
    std::vector<uint8_t>().swap(t->bwx_image);
    t->bwx_bytes = -1;
    return PC_OK;
}

int pc_track_bigwig_export_stats(pc_track *t, int64_t *out6) {
    if (!t || !out6) return fail(PC_ERR_ARG, "pc_track_bigwig_export_stats: bad arguments");
    for (int k = 0; k < 6; ++k) out6[k] = t->bwx_stats[k];
    return PC_OK;
}

int pc_track_bigwig_export_block_types(pc_track *t, int64_t *out3) {
    if (!t || !out3) return fail(PC_ERR_ARG, "pc_track_bigwig_export_block_types: bad arguments");
    out3[0] = t->bwx_stats[5]; out3[1] = t->bwx_stats[6]; out3[2] = t->bwx_stats[7];
    return PC_OK;
}

int pc_track_bigwig_export_zoom_stats(pc_track *t, int64_t *levels, int64_t *out50) {
    if (!t || !levels || !out50) return fail(PC_ERR_ARG, "pc_track_bigwig_export_zoom_stats: bad arguments");
    *levels = t->bwz_levels;
    for (int k = 0; k < t->bwz_levels; ++k)
        for (int j = 0; j < 5; ++j) out50[5 * k + j] = t->bwz_stats[k][j];
    return PC_OK;
}

int pc_track_bigwig_export_zoom_timing(pc_track *t, double *ms4) {
    if (!t || !ms4) return fail(PC_ERR_ARG, "pc_track_bigwig_export_zoom_timing: bad arguments");
    for (int k = 0; k < 4; ++k) ms4[k] = t->bwz_ms[k];
    return PC_OK;
}

int pc_track_bigwig_export_timing(pc_track *t, double *ms6) {
    if (!t || !ms6) return fail(PC_ERR_ARG, "pc_track_bigwig_export_timing: bad arguments");
    for (int k = 0; k < 6; ++k) ms6[k] = t->bwx_ms[k];
    return PC_OK;
}

}   // extern "C"
