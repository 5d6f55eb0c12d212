// bigWig files on the GPU, host side (revision 18): pc_bigwig_info, pc_inflate_zlib, pc_track_add_bigwig / _path,
// pc_track_bigwig_stats / _timing, pc_track_gather_sum and pc_track_sum_ranges of include/plastid_counts.h.  One import is
// a BigWigImport taken through its phases (bigwig_add_impl): the host walks the header and the two trees (bigwig_host.h:
// what is refused there is refused before anything is uploaded); the bytes that hold the data blocks cross PCIe once,
// through the page-locked halves when they are large (sam_upload); every block is inflated by a wave and its Adler-32
// checked (stored blocks skip both); sections, an exclusive sum of their item counts, and the items as the line records of
// a text import; then the contigs of the chromosome tree are declared at their sizes (no growth: an item cannot pass its
// contig's size), the storage is made and the records are sorted and applied by the kernels of the text import in their
// ASSIGN mode.  Every defect is known before the track changes: a refused file leaves it as it was.
// Upload, inflate and Adler-32 are bigwig_load_blocks over a BigWigBlocks, the section pass is bigwig_sections over a
// BigWigSections: the summary reader (bigwig_summary.hip.h) loads its tables through the same two, and reads the
// statuses on the host through bigwig_block_words.  bigwig_parse is the prologue of pc_bigwig_info / _blocks.
// Part of the one translation unit of plastid_counts.hip (behind track_decoder.hip.h; the plumbing is device_util.hip.h).
#include "bigwig_kernels.hip.h"

namespace {

namespace bw = pcbw;

// the members of the inflate kernel for the compressed blocks of a file whose bytes [data_lo, data_hi) stand at offset 0
std::vector<pcbam::Member> zlib_members(const bw::BigWig &f) {
    std::vector<pcbam::Member> ms(f.blocks.size());
    for (size_t b = 0; b < ms.size(); ++b) {
        pcbam::Member &m = ms[b];
        m.coff = f.blocks[b].off - f.data_lo + 2; m.clen = (uint32_t)(f.blocks[b].size - 6); m.ulen = f.uncompress_buf;
        m.uoff = (uint64_t)b * f.slot_bytes(); m.crc = f.blocks[b].adler; m.hdr = 2;
    }
    return ms;
}

// inflate + Adler-32 of nm zlib streams on `st`: image and members in HBM, every stream into its slot of `out`;
// d_status: 2 x nm words, the statuses and behind them the bytes every stream gave
int queue_zlib_inflate(hipStream_t st, const uint8_t *d_image, const pcbam::Member *d_members, int nm, uint8_t *d_out, uint32_t *d_status) {
    if (nm == 0) return PC_OK;
    hipLaunchKernelGGL(pcbam::k_zlib_inflate, dim3((unsigned)nm), dim3(pcbam::kInflWG), 0, st, d_image, d_members, 0, nm, d_out, d_status);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(bw::k_zlib_adler, dim3((unsigned)nm), dim3(64), 0, st, (const uint8_t *)d_out, d_members, nm, (const uint32_t *)(d_status + nm), d_status);
    HIP_TRY(hipGetLastError());
    return PC_OK;
}

// The blocks of a file, or of one zoom level of it, in HBM: inflated and Adler-checked when the file is compressed, as
// they stand in the file otherwise.  Block b is bytes [off[b], off[b] + len[b]) of data.
struct BigWigBlocks {
    std::vector<uint64_t> off;
    std::vector<uint32_t> sizes;       // stored blocks: what d_len is uploaded from
    DevBuf<uint8_t> d_inflated;
    DevBuf<uint32_t> d_status, d_len;  // d_status (compressed): the statuses, then the bytes every block inflated to; d_len (stored): the sizes
    DevBuf<uint64_t> d_off;
    const uint8_t *data = nullptr;
    const uint32_t *len = nullptr, *status = nullptr;   // status: null for stored blocks
};

// The bytes [data_lo, data_hi) of `f` cross PCIe once into d.d_stream; inflate and Adler-32; the blocks' offsets.  The
// three events are recorded in front of the upload, behind it, and behind everything queued here.
int bigwig_load_blocks(BamDecode &d, const uint8_t *image, const bw::BigWig &f, hipEvent_t start, hipEvent_t uploaded, hipEvent_t inflated, BigWigBlocks &k) {
    hipStream_t st = d.st;
    const int64_t nb = (int64_t)f.blocks.size(), bytes = (int64_t)(f.data_hi - f.data_lo);
    {
        Upload u;
        Drain drain{d.e, true};
        PC_TRY(d.d_stream.reserve((size_t)bytes + 64));
        HIP_TRY(hipEventRecord(start, st));
        PC_TRY(sam_upload(d, image + f.data_lo, bytes, nullptr, u));
        HIP_TRY(hipStreamSynchronize(st));   // (the ring's halves and its events are the engine's: the next user finds them idle)
        drain.armed = false;
    }
    HIP_TRY(hipEventRecord(uploaded, st));
    k.off.resize((size_t)nb);
    if (f.compressed()) {
        const std::vector<pcbam::Member> ms = zlib_members(f);
        for (int64_t b = 0; b < nb; ++b) k.off[(size_t)b] = ms[(size_t)b].uoff;
        int rc = PC_OK;
        room(rc, k.d_inflated, (size_t)nb * (size_t)f.slot_bytes() + 64); room(rc, k.d_status, 2 * (size_t)nb);
        room(rc, d.d_members, (size_t)nb);
        if (rc != PC_OK) return rc;
        HIP_TRY(hipMemcpyAsync(d.d_members.p, ms.data(), ms.size() * sizeof(pcbam::Member), hipMemcpyHostToDevice, st));
        PC_TRY(queue_zlib_inflate(st, d.d_stream.p, d.d_members.p, (int)nb, k.d_inflated.p, k.d_status.p));
        HIP_TRY(hipStreamSynchronize(st));   // (ms goes out of scope)
        k.data = k.d_inflated.p; k.len = k.d_status.p + nb; k.status = k.d_status.p;
    } else {
        k.sizes.resize((size_t)nb);
        for (int64_t b = 0; b < nb; ++b) { k.off[(size_t)b] = f.blocks[(size_t)b].off - f.data_lo; k.sizes[(size_t)b] = (uint32_t)f.blocks[(size_t)b].size; }
        PC_TRY(k.d_len.upload(k.sizes, st));
        k.data = d.d_stream.p; k.len = k.d_len.p;
    }
    PC_TRY(k.d_off.upload(k.off, st));
    HIP_TRY(hipEventRecord(inflated, st));
    return PC_OK;
}

// The statuses of the nb loaded blocks and behind them their lengths, on the host (stored blocks: zeros and the sizes).
int bigwig_block_words(hipStream_t st, const BigWigBlocks &k, std::vector<uint32_t> &words) {
    const size_t nb = k.off.size();
    words.assign(2 * nb, 0u);
    if (!k.status) {
        std::copy(k.sizes.begin(), k.sizes.end(), words.begin() + (ptrdiff_t)nb);
        return PC_OK;
    }
    HIP_TRY(hipMemcpyAsync(words.data(), k.status, 2 * nb * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PC_OK;
}

// What the sections pass leaves: every block's item count and the items in front of it (nb + 1 entries each), the
// contigs by chromId, the counters in HBM and as they stood behind the pass, the number of items.
struct BigWigSections {
    DevBuf<uint32_t> d_count, d_first;
    DevBuf<bw::ChromOfId> d_ids;
    DevBuf<bw::BwCounters> d_cnt;
    bw::BwCounters cnt = {bw::kNoDefect, {0ull, 0ull, 0ull}, 0ull};
    int64_t nitems = 0;
};

// Section headers and the exclusive sum of their item counts.  A defective block has no items and leaves its defect in
// s.cnt.first_err: the caller reports it, behind its items' when it goes on to them.
int bigwig_sections(hipStream_t st, DevBuf<uint8_t> &d_tmp, const std::string &path, const BigWigBlocks &k, int64_t nb, const std::vector<bw::ChromOfId> &of_id,
                    BigWigSections &s) {
    int rc = PC_OK;
    room(rc, s.d_count, (size_t)nb + 1); room(rc, s.d_first, (size_t)nb + 1); room(rc, s.d_cnt, 1);
    if (rc != PC_OK) return rc;
    PC_TRY(s.d_ids.upload(of_id, st));
    memset(&s.cnt, 0, sizeof(s.cnt));
    s.cnt.first_err = bw::kNoDefect;
    HIP_TRY(hipMemcpyAsync(s.d_cnt.p, &s.cnt, sizeof(s.cnt), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(s.d_count.p + nb, 0, 4, st));
    hipLaunchKernelGGL(bw::k_bw_sections, dim3(grid256(nb)), dim3(256), 0, st, k.data, k.d_off.p, k.len, k.status, nb, s.d_ids.p, (uint32_t)of_id.size(), s.d_count.p, s.d_cnt.p);
    HIP_TRY(hipGetLastError());
    // (nb + 1 entries: the last sum is the number of items -- below 2^32 for fewer than 2^16 blocks, checked otherwise)
    uint64_t total64 = 0;
    if (nb >= 65536) {
        std::vector<uint32_t> counts((size_t)nb);
        HIP_TRY(hipMemcpyAsync(counts.data(), s.d_count.p, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t v : counts) total64 += v;
        if (total64 >= ((uint64_t)1 << 31)) return fail(PC_ERR_ARG, "%s: bigWig: more than 2^31 - 1 items", path.c_str());
    }
    PC_TRY(cub_run(d_tmp, [&](void *tmp, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(tmp, b, s.d_count.p, s.d_first.p, (int)nb + 1, st); }));
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, s.d_first.p + nb, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&s.cnt, s.d_cnt.p, sizeof(s.cnt), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    s.nitems = (int64_t)total;
    if (s.nitems >= ((int64_t)1 << 31)) return fail(PC_ERR_ARG, "%s: bigWig: more than 2^31 - 1 items", path.c_str());
    return PC_OK;
}

struct BigWigImport {
    TrackImport c;                     // the phases behind the items are the text import's
    bw::BigWig f;
    LapEvents<5> ev;                   // start | uploaded | inflated + checked | sections + items | applied
    std::vector<bw::ChromOfId> of_id;  // by chromId: the TRACK's contig and the size
    std::vector<int32_t> track_id;     // by place in f.chroms
    BigWigBlocks k;
    BigWigSections s;
    BigWigImport(pc_track *t, const char *name, int strand) : c(t, nullptr, 0, name, strand) {}
};

// Phase 4: the sections pass, the items as line records; the lowest defect ends the import.
int bigwig_sections_and_items(BigWigImport &x) {
    TrackImport &c = x.c;
    hipStream_t st = c.st;
    BigWigSections &s = x.s;
    const int64_t nb = (int64_t)x.f.blocks.size();
    PC_TRY(bigwig_sections(st, c.d_tmp, c.d.path, x.k, nb, x.of_id, s));
    // (with a defective block too: an item of a block in front of it may hold the lower defect; such a block has no items here)
    if (s.nitems > 0) {
        c.n = s.nitems; c.g = grid256(c.n);
        int rc = PC_OK;
        room(rc, c.d_line, (size_t)c.n); room(rc, c.d_contig_of, (size_t)c.n); room(rc, c.d_cls, (size_t)c.n);
        if (rc != PC_OK) return rc;
        hipLaunchKernelGGL(bw::k_bw_items, dim3(c.g), dim3(256), 0, st, x.k.data, x.k.d_off.p, s.d_first.p, nb, c.n, s.d_ids.p, c.d_line.p, c.d_contig_of.p, c.d_cls.p, s.d_cnt.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&s.cnt, s.d_cnt.p, sizeof(s.cnt), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (s.cnt.first_err != bw::kNoDefect) return fail(PC_ERR_ARG, "%s", bw::defect_message(c.d.path.c_str(), s.cnt.first_err).c_str());
    HIP_TRY(hipEventRecord(x.ev[3], st));
    return PC_OK;
}

// Phase 5: the contigs of the chromosome tree, the sort keys, the storage; then the text import's sort and apply, assigning.
int bigwig_declare_and_apply(BigWigImport &x) {
    TrackImport &c = x.c;
    hipStream_t st = c.st;
    pc_track *t = c.t;
    for (size_t k = 0; k < x.f.chroms.size(); ++k) {
        const int32_t id = x.track_id[k];
        if (!t->tab.born[(size_t)id]) { t->tab.bear(id); t->tab.length[(size_t)id] = (int64_t)x.f.chroms[k].size; }
    }
    c.ncontig = (int)t->tab.names.size();
    if (c.n == 0 || c.ncontig == 0) return PC_OK;
    c.furthest.assign((size_t)c.ncontig, 0ull);
    c.first_line.assign((size_t)c.ncontig, tk::kNoLine);
    c.len0.assign((size_t)c.ncontig, INT64_MAX);   // (no line reaches it: the contigs keep their sizes)
    int rc = PC_OK;
    room(rc, c.d_key, (size_t)c.n); room(rc, c.d_idx, (size_t)c.n); room(rc, c.d_key2, (size_t)c.n); room(rc, c.d_idx2, (size_t)c.n);
    room(rc, c.d_list, (size_t)c.n); room(rc, c.d_cnt, 1);
    if (rc != PC_OK) return rc;
    memset(&c.cnt, 0, sizeof(c.cnt));
    c.cnt.first_err = tk::kNoDefect;
    HIP_TRY(hipMemcpyAsync(c.d_cnt.p, &c.cnt, sizeof(c.cnt), hipMemcpyHostToDevice, st));
    PC_TRY(c.d_len0.upload(c.len0, st)); PC_TRY(c.d_furthest.upload(c.furthest, st)); PC_TRY(c.d_first_line.upload(c.first_line, st));
    hipLaunchKernelGGL(tk::k_track_keys, dim3(c.g), dim3(256), 0, st, c.d_line.p, c.d_contig_of.p, c.d_cls.p, c.n, c.d_len0.p, c.ncontig, c.d_furthest.p, c.d_first_line.p,
                       c.d_list.p, c.d_key.p, c.d_idx.p, c.d_cnt.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c.furthest.data(), c.d_furthest.p, (size_t)c.ncontig * 8, hipMemcpyDeviceToHost, st));
    PC_TRY(c.read_counters());
    PC_TRY(track_grow_storage(t, t->tab.plan_storage(c.strand, c.furthest), st));
    return import_sort_and_apply<true>(c);
}

int bigwig_add_impl(pc_track *t, const void *image, int64_t size, const char *name, int strand) {
    if (!t || size < 0 || (size > 0 && !image)) return fail(PC_ERR_ARG, "pc_track_add_bigwig: bad arguments");
    if (strand < 0 || strand >= t->tab.nstrands) return fail(PC_ERR_ARG, "pc_track_add_bigwig: strand slot %d of %d", strand, t->tab.nstrands);
    HIP_TRY(hipSetDevice(t->e->device));
    PoolScope pool_scope(&t->e->pool);
    BigWigImport x(t, name, strand);
    for (auto &v : t->bw_stats) v = 0;
    for (auto &v : t->bw_ms) v = 0.0;
    const unsigned long long d = bw::parse((const uint8_t *)image, (uint64_t)size, x.f);
    if (d != bw::kNoDefect) return fail(PC_ERR_ARG, "%s", bw::defect_message(x.c.d.path.c_str(), d).c_str());
    // the track's id of every contig (an unknown name becomes an unborn contig, as a name a text import meets)
    x.of_id = x.f.of_id;
    x.track_id.resize(x.f.chroms.size());
    for (size_t k = 0; k < x.f.chroms.size(); ++k) {
        x.track_id[k] = t->tab.id_of(x.f.chroms[k].name);
        x.of_id[x.f.chroms[k].id].contig = x.track_id[k];
    }
    if (t->tab.names.size() >= ((size_t)1 << 22)) return fail(PC_ERR_ARG, "%s: more than 2^22 contigs", x.c.d.path.c_str());
    PC_TRY(x.ev.create());
    DrainOnExit drained{x.c.st};
    if (!x.f.blocks.empty()) {
        PC_TRY(bigwig_load_blocks(x.c.d, (const uint8_t *)image, x.f, x.ev[0], x.ev[1], x.ev[2], x.k));   // phases 2, 3
        PC_TRY(bigwig_sections_and_items(x));
    } else {
        for (int k = 0; k < 4; ++k) HIP_TRY(hipEventRecord(x.ev[k], x.c.st));
    }
    PC_TRY(bigwig_declare_and_apply(x));
    t->sum_valid = false;
    HIP_TRY(hipEventRecord(x.ev[4], x.c.st));
    HIP_TRY(hipStreamSynchronize(x.c.st));
    drained.armed = false;
    x.ev.laps(t->bw_ms, 4);
    const int64_t nb = (int64_t)x.f.blocks.size();
    t->bw_stats[0] = nb; t->bw_stats[1] = x.f.compressed() ? nb : 0;
    for (int k = 0; k < 3; ++k) t->bw_stats[2 + k] = (int64_t)x.s.cnt.by_type[k];
    t->bw_stats[5] = x.s.nitems > 0 ? (int64_t)x.c.cnt.n_multi : 0;
    t->bw_stats[6] = (int64_t)(x.f.data_hi - x.f.data_lo); t->bw_stats[7] = x.f.compressed() ? (int64_t)x.s.cnt.bytes : 0;
    return PC_OK;
}

// The container of the image, or of the file at `path` when there is no image (mapped into mf), parsed into f.
int bigwig_parse(const char *path, const void *image, int64_t size, MappedFile &mf, bw::BigWig &f) {
    if (!image) {
        PC_TRY(mf.open(path, 0, 0));
        image = mf.p; size = (int64_t)mf.size;
    }
    const unsigned long long d = bw::parse((const uint8_t *)image, (uint64_t)size, f);
    if (d != bw::kNoDefect) return fail(PC_ERR_ARG, "%s", bw::defect_message(path, d).c_str());
    return PC_OK;
}

}   // namespace

extern "C" {

int pc_bigwig_info(const char *path, const void *image, int64_t size, int64_t *out5, int max_contigs, char *names, int64_t names_bytes, int64_t *sizes) {
    if ((!path && !image) || !out5 || size < 0 || max_contigs < 0 || names_bytes < 0) return fail(PC_ERR_ARG, "pc_bigwig_info: bad arguments");
    MappedFile mf;
    bw::BigWig f;
    PC_TRY(bigwig_parse(path, image, size, mf, f));
    int64_t need = 0;
    for (const bw::Chrom &c : f.chroms) need += (int64_t)c.name.size() + 1;
    out5[0] = (int64_t)f.chroms.size(); out5[1] = (int64_t)f.blocks.size(); out5[2] = f.uncompress_buf; out5[3] = f.version; out5[4] = need;
    if (names && sizes && max_contigs >= (int)f.chroms.size() && names_bytes >= need) {
        char *q = names;
        for (size_t k = 0; k < f.chroms.size(); ++k) {
            memcpy(q, f.chroms[k].name.c_str(), f.chroms[k].name.size() + 1);
            q += f.chroms[k].name.size() + 1;
            sizes[k] = (int64_t)f.chroms[k].size;
        }
    }
    return PC_OK;
}

int pc_bigwig_blocks(const char *path, const void *image, int64_t size, int64_t nblocks, int64_t *off, int64_t *bytes) {
    if ((!path && !image) || size < 0 || nblocks < 0 || (nblocks > 0 && (!off || !bytes))) return fail(PC_ERR_ARG, "pc_bigwig_blocks: bad arguments");
    MappedFile mf;
    bw::BigWig f;
    PC_TRY(bigwig_parse(path, image, size, mf, f));
    if (nblocks != (int64_t)f.blocks.size()) return fail(PC_ERR_ARG, "pc_bigwig_blocks: the file has %lld blocks", (long long)f.blocks.size());
    for (size_t b = 0; b < f.blocks.size(); ++b) { off[b] = (int64_t)f.blocks[b].off; bytes[b] = (int64_t)f.blocks[b].size; }
    return PC_OK;
}

int pc_inflate_zlib(pc_engine *e, const void *image, int64_t n, const int64_t *off, const int64_t *len, int64_t capacity, void *out, int64_t *out_len, int32_t *status) {
    if (!e || n < 0 || capacity < 0 || capacity > (int64_t)bw::kMaxInflated || n >= ((int64_t)1 << 31) || (n > 0 && (!image || !off || !len || !out_len || !status)) || (n > 0 && capacity > 0 && !out))
        return fail(PC_ERR_ARG, "pc_inflate_zlib: bad arguments");
    if (n == 0) return PC_OK;
    int64_t image_bytes = 0;
    for (int64_t k = 0; k < n; ++k) {
        if (off[k] < 0 || len[k] < 0 || len[k] > (int64_t)bw::kMaxBlockBytes) return fail(PC_ERR_ARG, "pc_inflate_zlib: stream %lld lies below 0 or holds more than 2^28 bytes", (long long)k);
        image_bytes = std::max(image_bytes, off[k] + len[k]);
    }
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    const uint8_t *img = (const uint8_t *)image;
    const uint64_t slot = ((uint64_t)capacity + 15u) & ~(uint64_t)15u;
    // a stream whose header the host refuses is an empty member here, and gets its status behind the kernels
    std::vector<pcbam::Member> ms((size_t)n);
    std::vector<uint8_t> bad((size_t)n, 0);
    for (int64_t k = 0; k < n; ++k) {
        const uint8_t *p = img + off[k];
        bad[(size_t)k] = len[k] < 6 || (p[0] & 15u) != 8u || (p[0] >> 4) > 7u || (((uint32_t)p[0] << 8) | p[1]) % 31u != 0u || (p[1] & 0x20u);
        pcbam::Member &m = ms[(size_t)k];
        m.coff = (uint64_t)off[k] + 2; m.clen = bad[(size_t)k] ? 0u : (uint32_t)(len[k] - 6); m.ulen = (uint32_t)capacity; m.uoff = (uint64_t)k * slot; m.hdr = 2;
        m.crc = 0u;
        if (!bad[(size_t)k]) {
            const uint8_t *t = p + len[k] - 4;
            m.crc = ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | (uint32_t)t[3];
        }
    }
    DevBuf<uint8_t> d_image, d_out;
    DevBuf<pcbam::Member> d_members;
    DevBuf<uint32_t> d_status;
    std::vector<uint32_t> h_status(2 * (size_t)n);   // the statuses, then the bytes every stream gave
    DrainOnExit drained{st};
    int rc = PC_OK;
    room(rc, d_image, (size_t)image_bytes + 64); room(rc, d_out, (size_t)n * (size_t)slot + 64); room(rc, d_members, (size_t)n);
    room(rc, d_status, 2 * (size_t)n);
    if (rc != PC_OK) return rc;
    HIP_TRY(hipMemcpyAsync(d_image.p, img, (size_t)image_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_members.p, ms.data(), ms.size() * sizeof(pcbam::Member), hipMemcpyHostToDevice, st));
    PC_TRY(queue_zlib_inflate(st, d_image.p, d_members.p, (int)n, d_out.p, d_status.p));
    HIP_TRY(hipMemcpyAsync(h_status.data(), d_status.p, 2 * (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (capacity > 0) HIP_TRY(hipMemcpy2DAsync(out, (size_t)capacity, d_out.p, (size_t)slot, (size_t)capacity, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    for (int64_t k = 0; k < n; ++k) {
        status[k] = bad[(size_t)k] ? bw::kInfZlibHeader : (int32_t)h_status[(size_t)k];
        out_len[k] = status[k] ? 0 : (int64_t)h_status[(size_t)(n + k)];
    }
    return PC_OK;
}

int pc_track_add_bigwig(pc_track *t, const void *image, int64_t size, const char *name, int strand_slot) {
    return bigwig_add_impl(t, image, size, name, strand_slot);
}

int pc_track_add_bigwig_path(pc_track *t, const char *path, int strand_slot) {
    if (!t || !path) return fail(PC_ERR_ARG, "pc_track_add_bigwig_path: bad arguments");
    const BamKnobs knobs;
    MappedFile mf;
    PC_TRY(mf.open(path, -1, knobs.touch));
    return bigwig_add_impl(t, mf.p, (int64_t)mf.size, path, strand_slot);
}

int pc_track_bigwig_stats(pc_track *t, int64_t *out8) {
    if (!t || !out8) return fail(PC_ERR_ARG, "pc_track_bigwig_stats: bad arguments");
    for (int k = 0; k < 8; ++k) out8[k] = t->bw_stats[k];
    return PC_OK;
}

int pc_track_bigwig_timing(pc_track *t, double *ms4) {
    if (!t || !ms4) return fail(PC_ERR_ARG, "pc_track_bigwig_timing: bad arguments");
    for (int k = 0; k < 4; ++k) ms4[k] = t->bw_ms[k];
    return PC_OK;
}

int pc_track_gather_sum(int ntrack, pc_track *const *tracks, int64_t nseg, const int32_t *contig, const int32_t *strand_slot, const int64_t *start, const int64_t *end,
                        const int64_t *out_off, const int8_t *out_step, int64_t out_elems, int normalize, double sum, double *host_out) {
    if (ntrack < 0 || (ntrack > 0 && !tracks) || nseg < 0 || out_elems < 0 || (nseg > 0 && (!start || !end || !out_off || !out_step)) ||
        (nseg > 0 && ntrack > 0 && (!contig || !strand_slot)) || (out_elems > 0 && !host_out) || normalize < 0 || normalize > 2)
        return fail(PC_ERR_ARG, "pc_track_gather_sum: bad arguments");
    for (int k = 0; k < ntrack; ++k)
        if (!tracks[k] || tracks[k]->e != tracks[0]->e) return fail(PC_ERR_ARG, "pc_track_gather_sum: the tracks live on different engines");
    if (out_elems == 0) return PC_OK;
    const std::string bad = tk::check_segments(tk::kGatherWords, nseg, start, end, out_off, out_step, out_elems, false);
    if (!bad.empty()) return fail(PC_ERR_ARG, "%s", bad.c_str());
    if (ntrack == 0) {   // (no reader on the strand: the zeros of the reference, normalised as they are)
        for (int64_t i = 0; i < out_elems; ++i) host_out[i] = normalize == 1 ? 0.0 / sum * 1e6 : (normalize == 2 ? 1e6 * 0.0 / sum : 0.0);
        return PC_OK;
    }
    pc_engine *e = tracks[0]->e;
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    DevBuf<pcdense::Item> d_items;
    DevBuf<double> d_out;
    std::vector<std::vector<pcdense::Item>> items((size_t)ntrack);   // (every reader's items outlive their upload)
    DrainOnExit drained{st};
    PC_TRY(d_out.reserve((size_t)out_elems));
    HIP_TRY(hipMemsetAsync(d_out.p, 0, (size_t)out_elems * sizeof(double), st));
    size_t most = 0;
    for (int k = 0; k < ntrack; ++k) {
        const pc_track *t = tracks[k];
        const int32_t *ck = contig + (int64_t)k * nseg, *sk = strand_slot + (int64_t)k * nseg;
        t->tab.cut_items(nseg, start, end, out_off, out_step, [&](int64_t s) { return t->tab.public_slot(ck[s], sk[s]); }, items[(size_t)k]);
        if (items[(size_t)k].size() >= (size_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_track_gather_sum: too many items");
        most = std::max(most, items[(size_t)k].size());
    }
    // one launch per reader, in reader order, each adding onto the output: 0.0 + r1 + r2 + ... per element
    PC_TRY(d_items.reserve(std::max<size_t>(most, 1)));
    for (int k = 0; k < ntrack; ++k) {
        if (items[(size_t)k].empty()) continue;
        HIP_TRY(hipMemcpyAsync(d_items.p, items[(size_t)k].data(), items[(size_t)k].size() * sizeof(pcdense::Item), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(bw::k_track_gather_acc, dim3((unsigned)items[(size_t)k].size()), dim3(pcdense::kGatherWG), 0, st, d_items.p, tracks[k]->cells.p, d_out.p);
        HIP_TRY(hipGetLastError());
    }
    if (normalize) {
        hipLaunchKernelGGL(bw::k_track_scale, dim3(grid256(out_elems)), dim3(256), 0, st, d_out.p, out_elems, sum, normalize == 1 ? 0 : 1);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(host_out, d_out.p, (size_t)out_elems * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    return PC_OK;
}

int pc_track_sum_ranges(pc_track *t, int64_t nrange, const int32_t *contig, const int32_t *strand_slot, const int64_t *start, const int64_t *end, double *sum) {
    if (!t || !sum || nrange < 0 || (nrange > 0 && (!contig || !strand_slot || !start || !end))) return fail(PC_ERR_ARG, "pc_track_sum_ranges: bad arguments");
    std::vector<bw::SumTile> tiles;
    for (int64_t r = 0; r < nrange; ++r) {
        const int64_t at = t->tab.public_slot(contig[r], strand_slot[r]);
        if (at < 0) continue;
        const int64_t lo = std::max<int64_t>(start[r], 0), hi = std::min(end[r], t->tab.ext[(size_t)at]);   // (beyond the extent: zeros)
        for (int64_t p = lo; p < hi; p += pctrack::kSumTile) tiles.push_back(bw::SumTile{t->tab.cell_off[(size_t)at] + p, std::min<int64_t>(pctrack::kSumTile, hi - p)});
    }
    *sum = 0.0;
    if (tiles.empty()) return PC_OK;
    if (tiles.size() >= (size_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_track_sum_ranges: too many tiles");
    pc_engine *e = t->e;
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    DevBuf<bw::SumTile> d_tiles;
    DevBuf<double> d_partial;
    DrainOnExit drained{st};
    const int64_t nt = (int64_t)tiles.size();
    PC_TRY(d_partial.reserve((size_t)nt + 1));
    PC_TRY(d_tiles.upload(tiles, st));
    hipLaunchKernelGGL(bw::k_track_sum_tiles, dim3((unsigned)nt), dim3(256), 0, st, d_tiles.p, t->cells.p, d_partial.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pctrack::k_track_sum_final, dim3(1), dim3(256), 0, st, d_partial.p, nt, d_partial.p + nt);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sum, d_partial.p + nt, sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    return PC_OK;
}

}   // extern "C"
