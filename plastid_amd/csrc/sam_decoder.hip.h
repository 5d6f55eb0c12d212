// SAM text on the GPU, host side: the entry points of include/plastid_counts.h that read an aligner's text output with
// the kernels of sam_kernels.hip.h.  One open is seven phases (sam_open_impl): the file is mapped by the caller
// (MappedFile), the header parsed on the host (sam_host.h), the body uploaded (through the page-locked halves when it is
// large), the line starts found, the fields parsed, the records placed (place_records of bam_decoder.hip.h: order checks,
// scans, the radix sort of PC_BAM_SORT) and the columns written.  The result is a pc_bam like any other.
// Part of the one translation unit of plastid_counts.hip (behind bam_decoder.hip.h; the plumbing is device_util.hip.h).
#include "sam_kernels.hip.h"

namespace {

namespace sh = pcsam;

// Phase 3: the body goes to d.d_stream; returns with the copy queued, and the main stream behind it.
int sam_upload(BamDecode &d, const uint8_t *body, int64_t len, const UploadedHook *uploaded, Upload &u) {
    pc_engine *e = d.e;
    hipStream_t st = d.st;
    const int64_t piece = d.knobs.piece_bytes;
    u.up = st;
    u.ring = e->side_stream && len >= 2 * piece && !d.knobs.no_ring;
    for (int k = 0; k < 2 && u.ring; ++k) {
        if (e->bam_ring[k].reserve((size_t)piece + ((size_t)1 << 17)) != PC_OK) u.ring = false;
        if (u.ring && !e->ev_ring[k] && hipEventCreateWithFlags(&e->ev_ring[k], hipEventDisableTiming) != hipSuccess) u.ring = false;
    }
    (void)hipGetLastError();
    if (u.ring) {
        // through the two page-locked halves, filled by every host thread: the copy of one overlaps the filling of the other
        u.up = e->side_stream;
        u.ring_threads = std::max(1, std::min(usable_cpus(), 16));
        PC_TRY(u.mark(st));
        HIP_TRY(hipStreamWaitEvent(u.up, u.landed[0], 0));
        int piece_no = 0;
        for (int64_t off = 0; off < len; off += piece, ++piece_no) {
            const int slot = piece_no & 1;
            const int64_t n = std::min(piece, len - off);
            if (u.ring_busy[slot]) HIP_TRY(hipEventSynchronize(e->ev_ring[slot]));
            uint8_t *half = e->bam_ring[slot].p;
            const int64_t blk = (int64_t)1 << 20;
            parallel_chunks((n + blk - 1) / blk, u.ring_threads, [&](int, int64_t b0, int64_t b1) {
                const int64_t lo = b0 * blk, hi = std::min(n, b1 * blk);
                if (hi > lo) std::memcpy(half + lo, body + off + lo, (size_t)(hi - lo));
            });
            HIP_TRY(hipMemcpyAsync(d.d_stream.p + off, half, (size_t)n, hipMemcpyHostToDevice, u.up));
            HIP_TRY(hipEventRecord(e->ev_ring[slot], u.up));
            u.ring_busy[slot] = true;
        }
        PC_TRY(u.mark(u.up));
        HIP_TRY(hipStreamWaitEvent(st, u.landed.back(), 0));
    } else if (len > 0)
        HIP_TRY(hipMemcpyAsync(d.d_stream.p, body, (size_t)len, hipMemcpyHostToDevice, st));
    if (uploaded) (*uploaded)(u.up);
    return PC_OK;
}

// What the line-start phase leaves: the table (nrec + 1 entries) and the number of lines.
struct SamLines {
    DevBuf<uint64_t> d_line_start;
    int64_t nrec = 0;
};

// Phase 4: '\n' bytes per tile, their exclusive sum, every line's start.  `open_end`: the body does not end with '\n'.
int sam_line_starts(BamDecode &d, int64_t len, bool open_end, SamLines &ln) {
    hipStream_t st = d.st;
    const int64_t ntile = (len + sh::kSamTile - 1) / sh::kSamTile;
    DevBuf<uint32_t> d_tile, d_first;
    DevBuf<uint8_t> d_tmp;
    uint32_t newlines = 0;
    uint64_t end_entry = (uint64_t)len + 1;
    DrainOnExit drained{st};
    if (ntile >= (int64_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_sam_open: %s is too large", d.path.c_str());
    int rc = PC_OK;
    room(rc, d_tile, (size_t)ntile + 1); room(rc, d_first, (size_t)ntile + 1);
    if (rc != PC_OK) return rc;
    HIP_TRY(hipMemsetAsync(d_tile.p + ntile, 0, 4, st));
    if (ntile) hipLaunchKernelGGL(sh::k_sam_count_lines, dim3((unsigned)ntile), dim3(sh::kSamTileThreads), 0, st, d.d_stream.p, (uint64_t)len, d_tile.p);
    HIP_TRY(hipGetLastError());
    PC_TRY(cub_run(d_tmp, [&](void *tmp, size_t &bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, d_tile.p, d_first.p, (int)(ntile + 1), st); }));
    HIP_TRY(hipMemcpyAsync(&newlines, d_first.p + ntile, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    ln.nrec = (int64_t)newlines + (open_end ? 1 : 0);
    if (ln.nrec >= (int64_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_sam_open: more than 2^31-2 records per file are not supported");
    PC_TRY(ln.d_line_start.reserve((size_t)ln.nrec + 1));
    HIP_TRY(hipMemsetAsync(ln.d_line_start.p, 0, 8, st));
    if (open_end) HIP_TRY(hipMemcpyAsync(ln.d_line_start.p + ln.nrec, &end_entry, 8, hipMemcpyHostToDevice, st));
    if (ntile) hipLaunchKernelGGL(sh::k_sam_line_starts, dim3((unsigned)ntile), dim3(sh::kSamTileThreads), 0, st, d.d_stream.p, (uint64_t)len, d_first.p,
                                  ln.d_line_start.p, (uint64_t)ln.nrec + 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // (the tile tables and end_entry go out of scope)
    drained.armed = false;
    return PC_OK;
}

// the reference names where the kernels look them up
struct SamDevRefs {
    DevBuf<uint64_t> hash;
    DevBuf<int32_t> tid;
    DevBuf<uint8_t> names;
    DevBuf<uint32_t> name_off;
    int upload(const sh::SamRefTable &t, hipStream_t st, sh::SamRefs &view) {
        PC_TRY(hash.upload(t.hash, st));
        PC_TRY(tid.upload(t.tid, st));
        PC_TRY(names.reserve(std::max<size_t>(t.names.size(), 1)));
        if (!t.names.empty()) HIP_TRY(hipMemcpyAsync(names.p, t.names.data(), t.names.size(), hipMemcpyHostToDevice, st));
        PC_TRY(name_off.upload(t.name_off, st));
        view.hash = hash.p; view.tid = tid.p; view.mask = t.mask; view.names = names.p; view.name_off = name_off.p;
        return PC_OK;
    }
};

// a defect of SAM's own, worded with its line; the codes the formats share keep record_defect's words
int sam_defect(int rc, unsigned long long first_err, int64_t header_lines, const char *path) {
    if (rc == PC_OK || first_err == ~0ull) return rc;
    const int code = (int)(first_err & 0xffu);
    if (code < sh::kSamOwnCodes) return rc;
    const int64_t rec = (int64_t)((first_err >> 8) & ((1ull << 54) - 1));
    return fail(PC_ERR_ARG, "%s", sh::sam_defect_message(path, header_lines + rec + 1, code).c_str());
}

} // namespace

static int sam_open_impl(pc_engine *e, const void *image_, int64_t size, const char *name, pc_bam **out, const UploadedHook *uploaded, uint32_t flags) {
    if (!e || !out || size < 0 || (size > 0 && !image_)) return fail(PC_ERR_ARG, "pc_sam_open: bad arguments");
    *out = nullptr;
    if (flags & ~(uint32_t)PC_BAM_SORT) return fail(PC_ERR_ARG, "pc_sam_open: unknown flags (PC_BAM_SORT is the one there is)");
    const bool sort = (flags & PC_BAM_SORT) != 0;
    const uint8_t *image = (const uint8_t *)image_;
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    BamDecode d{e, e->stream, name ? name : "<memory>", BamKnobs()};
    hipStream_t st = d.st;
    // phase 2: the header, on the host
    if (sh::sam_looks_compressed(image, (size_t)size)) return fail(PC_ERR_ARG, "%s: %s", d.path.c_str(), sh::sam_compressed_text());
    sh::SamHeader hd;
    sh::SamRefTable table;
    sh::parse_sam_header(image, (size_t)size, hd, table);
    if (hd.defect != sh::kSamOk) return fail(PC_ERR_ARG, "%s", sh::sam_defect_message(d.path.c_str(), hd.defect_line, hd.defect).c_str());
    const uint8_t *body = image + hd.body_off;
    const int64_t len = size - (int64_t)hd.body_off;
    const bool open_end = len > 0 && body[len - 1] != (uint8_t)'\n';   // (read now: the mapping goes once the body is uploaded)
    d.clk.lap("header");
    pc_bam *b = new pc_bam();
    b->e = e; b->name = d.path; b->compressed_bytes = size; b->uploaded_bytes = len; b->runs = len > 0 ? 1 : 0;
    b->ref_names = hd.ref_names; b->ref_lengths = hd.ref_lengths;
    b->sort_requested = sort;
    struct Guard { pc_bam *b; ~Guard() { if (b) pc_bam_close(b); } } guard{b};
    PC_TRY(d.ev.create());
    BamHeader h;
    h.n_ref = (uint32_t)hd.ref_names.size();
    BamRecords recs;
    SamLines ln;
    {
        // phase 3: the body to HBM
        Upload u;
        Drain drain{e, true};
        PC_TRY(d.d_stream.reserve((size_t)len + 64));
        HIP_TRY(hipEventRecord(d.ev[0], st));
        PC_TRY(sam_upload(d, body, len, uploaded, u));
        HIP_TRY(hipEventRecord(d.ev[1], st));
        // phase 4: line starts (ends with the main stream drained, and the side stream in front of it)
        PC_TRY(sam_line_starts(d, len, open_end, ln));
        drain.armed = false;
    }
    HIP_TRY(hipEventRecord(d.ev[2], st));
    d.clk.lap("upload + line starts");
    recs.nrec = ln.nrec;
    b->total = ln.nrec;
    const int64_t nrec = ln.nrec;
    ColumnWork w;
    SamDevRefs drefs;
    DrainOnExit drained{st};   // (misc: [1] mapped, [2] unplaced; with `sort`: [3] out of order, [4] records moved)
    if (nrec > 0) {
        // phase 5: the fields of every line, and the order checks (or the sort keys)
        RecordTable &t = w.t;
        static const unsigned long long misc0[6] = {~0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
        PC_TRY(t.d_misc.reserve(6));
        HIP_TRY(hipMemcpyAsync(t.d_misc.p, misc0, sizeof(misc0), hipMemcpyHostToDevice, st));
        sh::SamRefs refs;
        int rc = drefs.upload(table, st, refs);
        room(rc, t.d_recs, (size_t)nrec); room(rc, t.d_placed, (size_t)nrec + 1);
        if (sort) { room(rc, t.d_key, (size_t)nrec); room(rc, t.d_idx, (size_t)nrec); }
        if (rc == PC_OK && sort) rc = t.sev.create();
        room(rc, w.d_runs, (size_t)nrec + 1); room(rc, w.d_staged_at, (size_t)nrec + 1); room(rc, w.d_run_at, (size_t)nrec + 1);
        if (rc != PC_OK) return rc;
        t.g256 = (unsigned)((nrec + 255) / 256);
        hipLaunchKernelGGL(sh::k_sam_fields, dim3(t.g256), dim3(256), 0, st, d.d_stream.p, (uint64_t)len, ln.d_line_start.p, nrec, refs, t.d_recs.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(d.ev[3], st));
        PC_TRY(check_order(d, nrec, sort, t));
        if (sort) b->sorted_input = !t.disorder;
        // phase 6: the shared placement
        rc = place_records(d, h, recs, sort, w, *b);
        if (rc != PC_OK) return sam_defect(rc, w.first_err, hd.header_lines, d.path.c_str());
        // phase 7: the columns
        const size_t ns = (size_t)std::max<int64_t>(w.n_staged, 1), nrun = (size_t)std::max<int64_t>(w.n_runs, 1);
        room(rc, b->tid, ns); room(rc, b->pos, ns); room(rc, b->alen, ns); room(rc, b->flags, ns); room(rc, b->nblk, ns);
        room(rc, b->flag16, ns); room(rc, b->mapq, ns); room(rc, b->lseq, ns); room(rc, b->nh, ns);
        room(rc, b->blk_start, nrun); room(rc, b->blk_len, nrun);
        room(rc, w.d_wide, ns);
        if (rc != PC_OK) return rc;
        HIP_TRY(hipMemsetAsync(w.d_wide.p, 0, ns * 4, st));
        hipLaunchKernelGGL(sh::k_sam_columns, dim3(t.g256), dim3(256), 0, st, d.d_stream.p, (uint64_t)len, ln.d_line_start.p, t.d_recs.p, nrec, w.d_staged_at.p,
                           w.d_run_at.p, b->tid.p, b->pos.p, b->alen.p, b->flags.p, b->nblk.p, b->blk_start.p, b->blk_len.p, w.d_wide.p, b->flag16.p,
                           b->mapq.p, b->lseq.p, b->nh.p);
        HIP_TRY(hipGetLastError());
        PC_TRY(collect_wide(d, nrec, w, *b));
    } else HIP_TRY(hipEventRecord(d.ev[3], st));
    HIP_TRY(hipEventRecord(d.ev[4], st));
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    d.clk.lap("fields + placement + columns");
    b->n = w.n_staged; b->nrun = w.n_runs;
    // upload | line starts | fields | placement + columns
    d.ev.laps(b->ms, 4);
    guard.b = nullptr;
    *out = b;
    return PC_OK;
}

// map the file, then open it (`out`) or stage it (`mapped`)
static int with_mapped_sam(pc_engine *e, const char *path, uint32_t flags, pc_bam **out, int64_t *mapped) {
    const BamKnobs knobs;
    MappedFile mf;
    int rc = mf.open(path, -1, knobs.touch);
    if (rc != PC_OK) return rc;
    const int device = e->device;
    const UploadedHook release = [&mf, device](hipStream_t up) { mf.release_behind(up, device); };
    if (out) return sam_open_impl(e, mf.p, (int64_t)mf.size, path, out, &release, flags);
    pc_bam *b = nullptr;
    rc = sam_open_impl(e, mf.p, (int64_t)mf.size, path, &b, &release, flags);
    return rc != PC_OK ? rc : stage_opened(e, b, mapped, knobs);
}

extern "C" {

int pc_sam_open_flags(pc_engine *e, const void *image, int64_t size, const char *name, uint32_t flags, pc_bam **out) {
    return sam_open_impl(e, image, size, name, out, nullptr, flags);
}

int pc_sam_open_path_flags(pc_engine *e, const char *path, uint32_t flags, pc_bam **out) {
    if (!e || !path || !out) return fail(PC_ERR_ARG, "pc_sam_open_path_flags: bad arguments");
    return with_mapped_sam(e, path, flags, out, nullptr);
}

int pc_add_alignment_sam_path_flags(pc_engine *e, const char *path, uint32_t flags, int64_t *mapped) {
    if (!e || !path) return fail(PC_ERR_ARG, "pc_add_alignment_sam_path_flags: bad arguments");
    if (flags & ~(uint32_t)PC_BAM_SORT) return fail(PC_ERR_ARG, "pc_add_alignment_sam_path_flags: unknown flags (PC_BAM_SORT is the one there is)");
    return with_mapped_sam(e, path, flags, nullptr, mapped);
}

} // extern "C"
