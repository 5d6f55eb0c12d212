// Compressed BAM on the GPU, host side: the entry points of include/plastid_counts.h that decode a BAM file with the
// kernels of bam_kernels.hip.h.  One open is five phases (bam_open_impl): plan_members, upload_and_inflate, read_header,
// chain_records, decode_columns.  The index build (bam_index_impl: BAI or CSI) runs the first four and index_records in place of the fifth.  Part of the one translation unit of plastid_counts.hip.
#include "bam_kernels.hip.h"
#include "sort_kernels.hip.h"
#include "index_kernels.hip.h"
#include "bam_index.h"

struct pc_bam {
    pc_engine *e = nullptr;
    std::string name;
    int64_t n = 0, nrun = 0, mapped = 0, unplaced = 0, total = 0;
    std::vector<std::string> ref_names;
    std::vector<int32_t> ref_lengths;
    DevBuf<int32_t> tid, pos, blk_start, blk_len;
    DevBuf<uint16_t> alen;
    DevBuf<uint8_t> flags, nblk;
    DevBuf<uint16_t> flag16;           // the SAM FLAG word, MAPQ and l_seq of every staged record (pc_bam_read_sam; the
    DevBuf<uint8_t> mapq;              // first two stay with the staged file for the FLAG / MAPQ filter)
    DevBuf<int32_t> lseq;
    DevBuf<uint16_t> nh;               // the NH:i tag of every staged record, 0 without one (pc_bam_read_nh; stays with the staged file for the NH filter)
    std::vector<int64_t> wide_idx;
    std::vector<int32_t> wide_alen, wide_nblk;
    double ms[4] = {0, 0, 0, 0};     // upload, inflate (+ CRC), record chain, fields + columns
    int64_t members = 0, inflated_bytes = 0, compressed_bytes = 0;
    int64_t uploaded_bytes = 0, runs = 0;   // bytes of the file image that went to HBM, contiguous stretches they came from
    int chain_restarts = 0;
    // PC_BAM_SORT (pc_bam_sort_stats, pc_bam_read_file_order)
    bool sort_requested = false, sorted_input = true;
    int64_t moved = 0, key_bits = 0;   // records staged elsewhere than their rank in the file; key bits the radix sort looked at
    double sort_ms = 0;                // GPU time of the key kernel (+ sort, ranks and run offsets when the file was out of order)
    DevBuf<uint32_t> file_order;       // moved > 0: the record number in the file of every staged record
};

namespace {

uint16_t brd16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
uint32_t brd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// CRC-32 tables (RFC 1952): the byte table, and the operator that advances the register over kCrcSlice zero bytes
// split by register byte (k_bgzf_crc combines 64 slice remainders with it)
struct CrcTables {
    uint32_t tab[256];
    uint32_t shift[4 * 256];
    CrcTables() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            tab[i] = c;
        }
        for (int b = 0; b < 4; ++b)
            for (uint32_t v = 0; v < 256; ++v) {
                uint32_t c = v << (8 * b);
                for (int k = 0; k < pcbam::kCrcSlice; ++k) c = tab[c & 0xffu] ^ (c >> 8);
                shift[b * 256 + v] = c;
            }
    }
};
const CrcTables &crc_tables() { static const CrcTables t; return t; }

double ms_between(hipEvent_t a, hipEvent_t b) { float t = 0.f; return hipEventElapsedTime(&t, a, b) == hipSuccess ? (double)t : 0.0; }
// one more buffer of a phase, unless an earlier one has failed
template <typename Buf> void room(int &rc, Buf &buf, size_t n) { if (rc == PC_OK) rc = buf.reserve(n); }

// The decoder's experiment and test switches, read at the top of every open (the tests flip them between opens on one engine).
struct BamKnobs {
    bool timing = getenv("PC_BAM_TIMING") != nullptr;        // wall-clock laps of the host side on stderr
    bool debug = getenv("PC_BAM_DEBUG") != nullptr;          // which member failed to inflate
    bool serial_symbols = getenv("PC_BGZF_SERIAL") && atoi(getenv("PC_BGZF_SERIAL")) != 0;   // (round 4's first kernel, for comparison)
    bool no_ring = getenv("PC_BAM_NO_RING") != nullptr;      // upload straight from the mapping, whatever the size
    bool stage_host = getenv("PC_BAM_STAGE_HOST") != nullptr;   // pc_add_alignment_bam*: the columns go through host arrays
    int streams = getenv("PC_BAM_STREAMS") ? atoi(getenv("PC_BAM_STREAMS")) : 2;   // streams the inflate launches take turns on, 1 .. 4
    int touch = getenv("PC_BAM_TOUCH") ? (atoi(getenv("PC_BAM_TOUCH")) != 0 ? 1 : 0) : -1;   // whole-file reads: fault the mapping's pages up front (-1: by size)
    int64_t walk_min = getenv("PC_BAM_WALK_MIN") ? atoll(getenv("PC_BAM_WALK_MIN")) : ((int64_t)32 << 20);   // (tests: the parallel walk on small files)
    int64_t piece_bytes = getenv("PC_BAM_PIECE") ? std::max<int64_t>(1, atoll(getenv("PC_BAM_PIECE"))) : ((int64_t)64 << 20);
    // region reads: compressed bytes from the start of the file searched for the header, grown on retry (tests: a header longer than the first slice)
    int64_t header_bytes = getenv("PC_BAM_HEADER_BYTES") ? std::max<int64_t>(1, atoll(getenv("PC_BAM_HEADER_BYTES"))) : ((int64_t)256 << 10);
};

struct BamClock {   // PC_BAM_TIMING=1: wall-clock laps of the host side of the GPU decoder
    bool on;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char *what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[bam] %-34s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
    void note(const char *what) {   // time since the last lap, the lap goes on
        if (!on) return;
        fprintf(stderr, "[bam]   (%s: %.2f ms into the lap)\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count());
    }
};

// `uploaded` (optional): called once, with the stream the image is uploaded on, when the last piece has been queued -- once
// that stream has drained the host copy of the file is not read again (pc_bam_open_path takes its mapping down while the
// GPU is still inflating).
typedef std::function<void(hipStream_t)> UploadedHook;
// A region read (pc_bam_open_chunks; pc_bam_open_span is the same with one chunk): only the members the chunks
// [cbeg[k], cend[k]) of the BAI index touch go to HBM (plus the leading members that hold the header); chunks that share or
// touch a member form one run (one contiguous upload, one record chain from the run's first chunk start to its last chunk
// end), and only the records that overlap one of the regions stay.
struct BamSpan {
    int nchunk = 0;                          // 0: header only
    const uint64_t *cbeg = nullptr, *cend = nullptr;   // (file offset of a member << 16 | offset in its payload), ascending, disjoint
    int nreg = 0;                            // merged regions, ascending by (reference id, start)
    const int32_t *tid = nullptr;
    const int64_t *beg = nullptr, *end = nullptr;
    int64_t header_bytes = 0;                // compressed bytes from the start of the file searched for the header (BamKnobs, grown on retry)
};
constexpr int PC_RETRY_HEADER = -1000;   // (internal) the header did not fit the leading members that were inflated

// ---- member boundaries (host: a walk over the gzip headers; 18 + bytes per 64 KiB of payload)
// What goes to the GPU and where it lands: the non-empty members, the runs of the file they come from, and where the
// chunks of a region read start and end.
struct BamPlan {
    // [file_lo, file_hi) lands at image offset dev_lo and holds members [m0, m1) (a whole-file read: one run)
    struct Run { int64_t file_lo, file_hi, dev_lo; int m0, m1; };
    // where a chunk starts and ends, by member (index in `members` of the member at the offset -- of the next non-empty
    // one for an empty member, members.size() past the last) and offset in its payload
    struct ChunkAt { int64_t cb; int s_idx, e_idx; uint32_t ub, ue; };
    std::vector<pcbam::Member> members;
    std::vector<Run> runs;
    std::vector<uint32_t> member_run;   // the run each member belongs to
    std::vector<ChunkAt> chunk_at;
    uint64_t total_u = 0;               // bytes of the inflated stream
    int64_t image_bytes = 0;            // bytes of the file that go to the device
    int nm() const { return (int)members.size(); }
    // stream offset at which member index m starts (total_u past the last)
    uint64_t uoff_of(int m) const { return m < nm() ? members[(size_t)m].uoff : total_u; }
};

// one member at `off`: 0, or which defect (walk_error's messages)
int parse_member(const uint8_t *image, int64_t size, int64_t off, pcbam::Member &mb, int64_t &clen_out) {
    if (off + 18 > size) return 1;
    const uint8_t *h = image + off;
    if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) return 2;
    const uint16_t xlen = brd16(h + 10);
    if (off + 12 + xlen > size) return 3;
    int bsize = -1;
    for (size_t x = 0; x + 4 <= xlen;) {
        const uint8_t *sf = h + 12 + x;
        const uint16_t slen = brd16(sf + 2);
        if (sf[0] == 'B' && sf[1] == 'C' && slen == 2 && x + 6 <= xlen) bsize = brd16(sf + 4);
        x += 4 + slen;
    }
    if (bsize < 0) return 4;
    const int64_t clen = (int64_t)bsize + 1;
    if (off + clen > size) return 5;
    const uint32_t isize = brd32(image + off + clen - 4);
    if (isize > (1u << 16)) return 6;
    const int64_t hdr = 12 + xlen;
    if (clen < hdr + 8) return 7;
    mb.coff = (uint64_t)(off + hdr); mb.clen = (uint32_t)(clen - hdr - 8); mb.ulen = isize; mb.uoff = 0;
    mb.crc = brd32(image + off + clen - 8); mb.hdr = (uint32_t)hdr;
    clen_out = clen;
    return 0;
}
int walk_error(int code, const char *path) {
    switch (code) {
    case 1: return fail(PC_ERR_ARG, "truncated BGZF header");
    case 2: return fail(PC_ERR_ARG, "not a BGZF file (bad gzip member header)");
    case 3: return fail(PC_ERR_ARG, "truncated BGZF extra field");
    case 4: return fail(PC_ERR_ARG, "BGZF member without BC subfield");
    case 5: return fail(PC_ERR_ARG, "truncated BGZF member");
    case 6: return fail(PC_ERR_ARG, "corrupt BGZF member (more than 64 KiB of payload)");
    default: return fail(PC_ERR_ARG, "BGZF inflate failed in %s", path);
    }
}
int belongs_not(const char *why, const char *path) { return fail(PC_ERR_ARG, "the index does not belong to this BAM file (%s): %s", why, path); }

// A region read's members: the header's from the start of the file, then every chunk's.
int plan_region(const uint8_t *image, int64_t size, const BamSpan &span, const char *path, BamPlan &pl) {
    std::vector<pcbam::Member> &members = pl.members;
    std::vector<BamPlan::Run> &runs = pl.runs;
    // every member walked: its file offset, its index in `members` (see ChunkAt) and its payload length
    struct Walked { int64_t off; int idx; uint32_t ulen; };
    std::vector<Walked> walked;
    // members from `off` on while they start before `hi_excl` (or at `last`, with_last); a new run unless `off` continues the last
    auto walk = [&](int64_t off, int64_t hi_excl, bool with_last, int64_t last) -> int {
        if (runs.empty() || runs.back().file_hi != off) runs.push_back(BamPlan::Run{off, off, 0, (int)members.size(), (int)members.size()});
        const int64_t first = off;
        while (off < size && (off < hi_excl || (with_last && off <= last))) {
            pcbam::Member mb;
            int64_t clen = 0;
            const int code = parse_member(image, size, off, mb, clen);
            if (code) return off == first && first > 0 ? belongs_not("a chunk does not start at a BGZF member", path) : walk_error(code, path);
            walked.push_back(Walked{off, (int)members.size(), mb.ulen});
            if (mb.ulen) members.push_back(mb);
            off += clen;
        }
        runs.back().file_hi = off; runs.back().m1 = (int)members.size();
        if (runs.back().file_hi == runs.back().file_lo) runs.pop_back();
        return PC_OK;
    };
    auto find = [&](int64_t off) -> const Walked * {
        auto it = std::lower_bound(walked.begin(), walked.end(), off, [](const Walked &w, int64_t o) { return w.off < o; });
        return it != walked.end() && it->off == off ? &*it : nullptr;
    };
    const int64_t cb0 = span.nchunk > 0 ? (int64_t)(span.cbeg[0] >> 16) : size;
    int rc = walk(0, std::min<int64_t>(span.header_bytes, cb0), false, 0);
    if (rc != PC_OK) return rc;
    for (int k = 0; k < span.nchunk; ++k) {
        const uint64_t vb = span.cbeg[k], ve = span.cend[k];
        const int64_t cb = (int64_t)(vb >> 16), ce = (int64_t)(ve >> 16);
        const uint32_t ub = (uint32_t)(vb & 0xffffu), ue = (uint32_t)(ve & 0xffffu);
        if (cb >= size || ce > size || (ue && ce >= size)) return belongs_not("a chunk lies beyond its end", path);
        const int64_t hi = runs.empty() ? 0 : runs.back().file_hi;
        if (cb < hi && !find(cb)) return belongs_not("a chunk does not start at a BGZF member", path);
        rc = walk(std::max(cb, hi), ce, ue != 0, ce);
        if (rc != PC_OK) return rc;
        BamPlan::ChunkAt c{cb, 0, 0, ub, ue};
        const Walked *ws = find(cb);
        if (!ws || ub > ws->ulen) return belongs_not("a chunk does not start at a BGZF member", path);
        c.s_idx = ws->idx;
        if (ue) {
            const Walked *we = find(ce);
            if (!we || ue > we->ulen) return belongs_not("a chunk does not end at a BGZF member", path);
            c.e_idx = we->idx;
        } else {
            if (runs.empty() || runs.back().file_hi != ce) return belongs_not("a chunk does not end at a BGZF member", path);
            c.e_idx = (int)members.size();
        }
        pl.chunk_at.push_back(c);
    }
    // adjacent runs become one (a run is uploaded as one contiguous copy)
    for (size_t k = 1; k < runs.size();)
        if (runs[k].file_lo == runs[k - 1].file_hi) { runs[k - 1].file_hi = runs[k].file_hi; runs[k - 1].m1 = runs[k].m1; runs.erase(runs.begin() + (long)k); }
        else ++k;
    int64_t dev = 0;
    for (BamPlan::Run &r : runs) {   // the members' streams by their place in the image on the device
        r.dev_lo = dev;
        for (int m = r.m0; m < r.m1; ++m) members[(size_t)m].coff = (uint64_t)((int64_t)members[(size_t)m].coff - r.file_lo + r.dev_lo);
        dev += r.file_hi - r.file_lo;
    }
    return PC_OK;
}

// Every member of the file, as one run.
int plan_whole_file(const uint8_t *image, int64_t size, const char *path, int64_t walk_min, BamPlan &pl) {
    std::vector<pcbam::Member> &members = pl.members;
    int64_t walked_to = 0;
    // Large files: the walk is a chain of dependent cache misses (40 k members: 5.6 ms), so every host thread walks its
    // own stretch of the file from the first offset in it where three members in a row parse; a stretch counts only if
    // the walk of the stretch before it LANDS on its first member -- whatever does not chain is walked again, serially.
    const int WT = size >= walk_min && size >= 64 ? std::max(1, std::min(usable_cpus(), 16)) : 1;
    if (WT > 1) {
        struct Stretch { int64_t first = -1, landing = -1; std::vector<pcbam::Member> mem; };
        std::vector<Stretch> str((size_t)WT);
        parallel_chunks((int64_t)WT, WT, [&](int, int64_t kb, int64_t ke) {
            for (int64_t k = kb; k < ke; ++k) {
                Stretch &sx = str[(size_t)k];
                const int64_t lo = size * k / WT, hi = size * (k + 1) / WT;
                int64_t off = lo;
                if (k > 0) {   // the first offset from which three members parse
                    off = -1;
                    for (int64_t c = lo; c < hi && c + 18 <= size; ++c) {
                        if (image[c] != 31 || image[c + 1] != 139) continue;
                        int64_t q = c;
                        bool ok = true;
                        for (int r = 0; r < 3 && ok && q < size; ++r) {
                            pcbam::Member mb;
                            int64_t cl = 0;
                            ok = parse_member(image, size, q, mb, cl) == 0;
                            q += cl;
                        }
                        if (ok) { off = c; break; }
                    }
                    if (off < 0) continue;
                }
                sx.first = off;
                while (off < hi && off < size) {
                    pcbam::Member mb;
                    int64_t cl = 0;
                    if (parse_member(image, size, off, mb, cl) != 0) { sx.first = -1; break; }   // (a defect: the serial walk below reports it)
                    if (mb.ulen) sx.mem.push_back(mb);
                    off += cl;
                }
                sx.landing = off;
            }
        });
        int64_t expected = 0;
        for (int k = 0; k < WT; ++k) {
            const Stretch &sx = str[(size_t)k];
            if (sx.first < 0 || sx.first != expected) break;
            members.insert(members.end(), sx.mem.begin(), sx.mem.end());
            expected = sx.landing;
        }
        walked_to = expected;
    }
    for (int64_t off = walked_to; off < size;) {
        pcbam::Member mb;
        int64_t clen = 0;
        const int code = parse_member(image, size, off, mb, clen);
        if (code) return walk_error(code, path);
        if (mb.ulen) members.push_back(mb);      // (empty members -- the end-of-file marker -- hold nothing)
        off += clen;
    }
    pl.runs.push_back(BamPlan::Run{0, size, 0, 0, (int)members.size()});
    return PC_OK;
}

// Phase 1 (host only): which members go to the GPU (`span`: those of a region read; nullptr: the whole file), in which
// runs, and where they land in the image on the device and in the inflated stream.
int plan_members(const uint8_t *image, int64_t size, const BamSpan *span, const char *path, int64_t walk_min, BamPlan &pl) {
    const int rc = span ? plan_region(image, size, *span, path, pl) : plan_whole_file(image, size, path, walk_min, pl);
    if (rc != PC_OK) return rc;
    for (pcbam::Member &mb : pl.members) { mb.uoff = pl.total_u; pl.total_u += mb.ulen; }
    for (const BamPlan::Run &r : pl.runs) pl.image_bytes += r.file_hi - r.file_lo;
    pl.member_run.assign((size_t)std::max(pl.nm(), 1), 0u);
    for (size_t r = 0; r < pl.runs.size(); ++r)
        for (int m = pl.runs[r].m0; m < pl.runs[r].m1; ++m) pl.member_run[(size_t)m] = (uint32_t)r;
    return PC_OK;
}

// What the phases of one open share (phases 2 - 5 queue on `st`; each leaves it drained of everything that reads a buffer it owns).
struct BamDecode {
    pc_engine *e;
    hipStream_t st;
    std::string path;
    BamKnobs knobs;
    BamClock clk{knobs.timing};
    hipEvent_t ev[5] = {};             // allocations done | tables queued | inflated | records chained | columns written
    DevBuf<uint8_t> d_stream;          // the inflated stream (+ 64 zero bytes)
    DevBuf<pcbam::Member> d_members;
    DevBuf<pcbam::MemberChain> d_chain;   // every member's walk over its records' length prefixes, and the record offsets it found
    DevBuf<uint32_t> d_rec_off;
};

// Phase 2: the image goes to HBM and is inflated there, piece by piece; returns with every stream drained, every member's
// status and CRC checked, and the image given back.
int upload_and_inflate(BamDecode &d, const uint8_t *image, const BamPlan &pl, const UploadedHook *uploaded) {
    using namespace pcbam;
    pc_engine *e = d.e;
    hipStream_t st = d.st;
    const std::vector<Member> &members = pl.members;
    const std::vector<BamPlan::Run> &runs = pl.runs;
    const int nm = pl.nm();
    DevBuf<uint8_t> d_image;
    DevBuf<uint32_t> d_status, d_crc;
    // (pieces of the image gathered from several runs, for an upload straight from pageable memory: they outlive `drain`)
    std::vector<std::vector<uint8_t>> gathered;
    int rc = PC_OK;
    room(rc, d_image, (size_t)std::max<int64_t>(pl.image_bytes, 16) + 16); room(rc, d.d_stream, (size_t)pl.total_u + 64);
    room(rc, d.d_members, (size_t)std::max(nm, 1)); room(rc, d_status, (size_t)std::max(nm, 1)); room(rc, d_crc, 5 * 256);
    if (rc != PC_OK) return rc;
    // An early return between here and the synchronisation behind the inflate launches must not hand the image, the
    // stream buffer or the page-locked ring back (nor let the caller unmap the file) while the side / auxiliary streams
    // still use them: drain every stream the decoder queues on before the buffers above go out of scope.
    struct Drain {
        pc_engine *e; bool armed;
        ~Drain() {
            if (!armed) return;
            if (e->side_stream) (void)hipStreamSynchronize(e->side_stream);
            for (int k = 0; k < pc_engine::kAux; ++k) if (e->aux_stream[k]) (void)hipStreamSynchronize(e->aux_stream[k]);
            (void)hipStreamSynchronize(e->stream);
        }
    } drain{e, true};
    d.clk.lap("allocations (image, stream)");
    HIP_TRY(hipEventRecord(d.ev[0], st));
    if (nm) HIP_TRY(hipMemcpyAsync(d.d_members.p, members.data(), (size_t)nm * sizeof(Member), hipMemcpyHostToDevice, st));
    const CrcTables &ct = crc_tables();
    HIP_TRY(hipMemcpyAsync(d_crc.p, ct.tab, sizeof(ct.tab), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_crc.p + 256, ct.shift, sizeof(ct.shift), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d.d_stream.p + pl.total_u, 0, 64, st));
    HIP_TRY(hipEventRecord(d.ev[1], st));
    // ---- upload + inflate, piece by piece: the file image crosses PCIe on the side stream in pieces of ~128 MiB of
    // whole members while the members of the pieces before are inflated on the main one (one wave per member).  (Every
    // launch ends in a tail of half-empty CUs -- a member takes ~4 ms and ~3 000 are in flight -- so the pieces are
    // large: 20 M aligner-like records, 578 MB: one piece 87 ms, 48 MiB pieces 67 ms, 128 MiB 58 ms, 256 MiB 61 ms.)
    std::vector<uint32_t> status((size_t)nm, 0u);
    if (nm) {
        const int64_t piece_bytes = d.knobs.piece_bytes;
        hipStream_t up = e->side_stream ? e->side_stream : st;
        std::vector<hipEvent_t> landed;
        struct EvList { std::vector<hipEvent_t> &v; ~EvList() { for (auto x : v) (void)hipEventDestroy(x); } } landed_guard{landed};
        if (up != st) {   // the side stream starts behind what the main one has queued so far (the buffers' previous users)
            hipEvent_t x;
            HIP_TRY(hipEventCreateWithFlags(&x, hipEventDisableTiming));
            landed.push_back(x);
            HIP_TRY(hipEventRecord(x, st));
            HIP_TRY(hipStreamWaitEvent(up, x, 0));
        }
        // The inflate launches alternate between the main stream and an auxiliary one: a launch ends in a tail of
        // half-empty CUs (a member takes ~4 ms, ~3 000 are in flight), which the launch of the next piece fills.
        // (two streams in turn: measured on two boxes, 64 MiB pieces, 20 M aligner-like records: one stream 56 - 58 ms, two
        // 46.6 - 53.5, four 48.6; PC_BAM_STREAMS = 1 .. 4 for experiments)
        const int naux = up != st ? std::max(0, std::min(pc_engine::kAux, d.knobs.streams - 1)) : 0;
        for (int k = 0; k < naux; ++k)   // (behind what the main stream has queued: the members table, the previous users of the buffers)
            HIP_TRY(hipStreamWaitEvent(e->aux_stream[k], landed[0], 0));
        // large files cross PCIe through two page-locked halves of one piece each (made once per engine)
        bool ring = up != st && pl.image_bytes >= 2 * piece_bytes && !d.knobs.no_ring;
        bool ring_busy[2] = {false, false};
        const int ring_threads = std::max(1, std::min(usable_cpus(), 16));
        if (ring) {
            // (a piece ends with a whole member: up to 64 KiB beyond piece_bytes)
            for (int k = 0; k < 2 && ring; ++k) {
                if (e->bam_ring[k].reserve((size_t)piece_bytes + ((size_t)1 << 17)) != PC_OK) ring = false;
                if (ring && !e->ev_ring[k] && hipEventCreateWithFlags(&e->ev_ring[k], hipEventDisableTiming) != hipSuccess) ring = false;
            }
            (void)hipGetLastError();
        }
        // bytes [lo, hi) of the image on the device, from the file, to dst: run by run (the file's bytes of run r start at
        // r.file_lo - r.dev_lo before its offsets in the image on the device)
        auto copy_image = [&](uint8_t *dst, int64_t lo, int64_t hi) {
            auto it = std::upper_bound(runs.begin(), runs.end(), lo, [](int64_t x, const BamPlan::Run &r) { return x < r.dev_lo; });
            for (size_t r = (size_t)(it - runs.begin()) - 1; r < runs.size() && lo < hi; ++r) {
                const int64_t rhi = std::min(hi, runs[r].dev_lo + (runs[r].file_hi - runs[r].file_lo));
                if (rhi > lo) std::memcpy(dst, image + (runs[r].file_lo - runs[r].dev_lo) + lo, (size_t)(rhi - lo));
                dst += std::max<int64_t>(rhi - lo, 0);
                lo = std::max(lo, rhi);
            }
        };
        const std::vector<uint32_t> &run_of = pl.member_run;   // (pieces end where a run ends; one piece may hold several short runs)
        int piece_no = 0;
        int64_t byte0 = 0;                   // the image is uploaded from here on (gzip headers and trailers ride along)
        for (int m0 = 0; m0 < nm; ++piece_no) {
            int m1 = m0;
            int64_t byte1 = byte0;
            while (m1 < nm && (byte1 - byte0 < piece_bytes || m1 == m0)) {
                byte1 = (int64_t)(members[(size_t)m1].coff + members[(size_t)m1].clen);
                ++m1;
            }
            if (m1 == nm) byte1 = pl.image_bytes;
            else if (run_of[(size_t)m1] != run_of[(size_t)m1 - 1]) byte1 = runs[run_of[(size_t)m1]].dev_lo;   // (the rest of the run before)
            const uint32_t r0 = run_of[(size_t)m0];
            const bool one_run = byte1 <= runs[r0].dev_lo + (runs[r0].file_hi - runs[r0].file_lo);
            const uint8_t *run_src = image + (runs[r0].file_lo - runs[r0].dev_lo);   // (one_run: the piece's bytes in the file)
            if (ring) {
                // through a page-locked half: the runtime's own staging of a pageable copy runs on one thread (12 - 20 GB/s);
                // here every host thread copies its share, and the DMA of one half overlaps the filling of the other
                const int slot = piece_no & 1;
                if (ring_busy[slot]) HIP_TRY(hipEventSynchronize(e->ev_ring[slot]));
                uint8_t *dstp = e->bam_ring[slot].p;
                const uint8_t *srcp = run_src + byte0;
                const int64_t len = byte1 - byte0, blk = (int64_t)1 << 20;
                parallel_chunks((len + blk - 1) / blk, ring_threads, [&](int, int64_t b, int64_t en) {
                    const int64_t lo = b * blk, hi = std::min(len, en * blk);
                    if (hi > lo && one_run) std::memcpy(dstp + lo, srcp + lo, (size_t)(hi - lo));
                    else if (hi > lo) copy_image(dstp + lo, byte0 + lo, byte0 + hi);
                });
                HIP_TRY(hipMemcpyAsync(d_image.p + byte0, dstp, (size_t)len, hipMemcpyHostToDevice, up));
                HIP_TRY(hipEventRecord(e->ev_ring[slot], up));
                ring_busy[slot] = true;
            } else if (one_run)
                HIP_TRY(hipMemcpyAsync(d_image.p + byte0, run_src + byte0, (size_t)(byte1 - byte0), hipMemcpyHostToDevice, up));
            else {   // several runs in one piece: gathered, one copy
                gathered.emplace_back((size_t)(byte1 - byte0));
                copy_image(gathered.back().data(), byte0, byte1);
                HIP_TRY(hipMemcpyAsync(d_image.p + byte0, gathered.back().data(), (size_t)(byte1 - byte0), hipMemcpyHostToDevice, up));
            }
            if (up != st) {
                hipEvent_t x;
                HIP_TRY(hipEventCreateWithFlags(&x, hipEventDisableTiming));
                landed.push_back(x);
                HIP_TRY(hipEventRecord(x, up));
            }
            hipStream_t ks = (piece_no % (naux + 1)) ? e->aux_stream[piece_no % (naux + 1) - 1] : st;
            if (up != st) HIP_TRY(hipStreamWaitEvent(ks, landed.back(), 0));
            if (d.knobs.serial_symbols) hipLaunchKernelGGL(k_bgzf_inflate<false>, dim3((unsigned)(m1 - m0)), dim3(kInflWG), 0, ks, d_image.p, d.d_members.p, m0, m1, d.d_stream.p, d_status.p);
            else hipLaunchKernelGGL(k_bgzf_inflate<true>, dim3((unsigned)(m1 - m0)), dim3(kInflWG), 0, ks, d_image.p, d.d_members.p, m0, m1, d.d_stream.p, d_status.p);
            // (the piece's CRC check right behind it, on the same stream: it runs while other pieces are still inflated)
            hipLaunchKernelGGL(k_bgzf_crc, dim3((unsigned)(m1 - m0)), dim3(64), 0, ks, d.d_stream.p, d.d_members.p, m0, m1, d_crc.p, d_crc.p + 256, d_status.p);
            byte0 = byte1;
            m0 = m1;
        }
        d.clk.note("every piece copied into the page-locked ring and queued");
        for (int k = 0; k < naux; ++k) {   // the main stream goes on behind all of them
            hipEvent_t x;
            HIP_TRY(hipEventCreateWithFlags(&x, hipEventDisableTiming));
            landed.push_back(x);
            HIP_TRY(hipEventRecord(x, e->aux_stream[k]));
            HIP_TRY(hipStreamWaitEvent(st, x, 0));
        }
        if (uploaded) (*uploaded)(up);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(status.data(), d_status.p, (size_t)nm * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipEventRecord(d.ev[2], st));
    HIP_TRY(hipStreamSynchronize(st));
    drain.armed = false;   // (the main stream went on behind the side and auxiliary ones: all of them have drained)
    d.clk.lap("upload + inflate + crc (sync)");
    for (int m = 0; m < nm; ++m)
        if (status[(size_t)m]) {
            if (d.knobs.debug) fprintf(stderr, "[bam] member %d of %d (%u compressed -> %u bytes at %llu): inflate status %u\n", m, nm,
                                       members[(size_t)m].clen, members[(size_t)m].ulen, (unsigned long long)members[(size_t)m].uoff, status[(size_t)m]);
            return fail(PC_ERR_ARG, "%s%s", status[(size_t)m] == (uint32_t)kInfCrc ? "BGZF CRC mismatch in " : "BGZF inflate failed in ", d.path.c_str());
        }
    d_image.release();
    d.clk.lap("status check + image release");
    return PC_OK;
}

struct BamHeader {
    uint64_t first_record = 0;   // stream offset of the first record
    uint32_t n_ref = 0;
    std::vector<std::string> ref_names;
    std::vector<int32_t> ref_lengths;
};

// Phase 3: the BAM header (host, from the head of the inflated stream).  A region read looks for it in the leading run
// only -- what follows is some chunk, from a record in the middle of the file on; PC_RETRY_HEADER: it does not fit that
// run, and the caller comes back with more of the file's head.
int read_header(BamDecode &d, const BamPlan &pl, int64_t size, const BamSpan *span, BamHeader &h) {
    const size_t header_limit = span ? (size_t)(pl.runs.empty() ? 0 : pl.uoff_of(pl.runs[0].m1)) : (size_t)pl.total_u;
    std::vector<uint8_t> head;
    size_t want = std::min<size_t>(header_limit, (size_t)1 << 16);
    for (;;) {
        head.resize(want);
        if (want) HIP_TRY(hipMemcpy(head.data(), d.d_stream.p, want, hipMemcpyDeviceToHost));
        const uint8_t *p = head.data(), *end = p + want;
        bool more = false;
        auto need = [&](size_t k) { if ((size_t)(end - p) < k) { more = true; return false; } return true; };
        bool ok = true;
        if (!need(12)) ok = false;
        if (ok && std::memcmp(p, "BAM\1", 4) != 0) return fail(PC_ERR_ARG, "not a BAM file (bad magic)");
        uint32_t l_text = 0;
        if (ok) { l_text = brd32(p + 4); p += 8; if (!need((size_t)l_text + 4)) ok = false; }
        if (ok) { p += l_text; h.n_ref = brd32(p); p += 4; }
        h.ref_names.clear(); h.ref_lengths.clear();
        for (uint32_t r = 0; ok && r < h.n_ref; ++r) {
            if (!need(4)) { ok = false; break; }
            const uint32_t l_name = brd32(p);
            p += 4;
            if (!need((size_t)l_name + 4)) { ok = false; break; }
            h.ref_names.emplace_back((const char *)p, l_name ? l_name - 1 : 0);
            p += l_name;
            h.ref_lengths.push_back((int32_t)brd32(p));
            p += 4;
        }
        if (ok) { h.first_record = (uint64_t)(p - head.data()); return PC_OK; }
        if (more && want >= header_limit && span && header_limit < (size_t)pl.total_u + 1 && span->header_bytes < size) return PC_RETRY_HEADER;
        if (!more || want >= header_limit)
            return fail(PC_ERR_ARG, want < 12 ? "not a BAM file (bad magic)" : (h.ref_names.empty() && h.n_ref == 0 ? "truncated BAM header" : "truncated BAM reference list"));
        want = std::min<size_t>(header_limit, want * 4);
    }
}

struct BamRecords {
    std::vector<uint64_t> rec_base;   // records before each member (nm + 1 entries)
    int64_t nrec = 0;
    bool truncated = false;           // the last record runs past the end of the stream (reported after every other defect)
    int chain_restarts = 0;
};

// Phase 4: record starts.  Every member guesses its first record start and walks the chain of length prefixes; the host
// confirms that the walks chain, and restarts the members whose guess did not.  A whole-file read chains from the header's
// end to the end of the stream; a region read chains every run from its first chunk's start to its last chunk's end, which
// the index gives and the chain has to hit exactly (a run without a chunk -- the header's -- has no record).
int chain_records(BamDecode &d, const BamPlan &pl, const BamSpan *span, const BamHeader &h, BamRecords &out) {
    using namespace pcbam;
    hipStream_t st = d.st;
    const std::vector<Member> &members = pl.members;
    const std::vector<BamPlan::Run> &runs = pl.runs;
    const std::vector<uint32_t> &member_run = pl.member_run;
    const int nm = pl.nm();
    const uint64_t total_u = pl.total_u, first_record = h.first_record;
    auto belongs_not_here = [&](const char *why) { return belongs_not(why, d.path.c_str()); };
    DevBuf<uint64_t> d_forced;
    int rc = PC_OK;
    room(rc, d.d_chain, (size_t)std::max(nm, 1)); room(rc, d.d_rec_off, (size_t)std::max(nm, 1) * kMaxRecPerMember); room(rc, d_forced, (size_t)std::max(nm, 1));
    if (rc != PC_OK) return rc;
    std::vector<uint64_t> run_bounds;   // region read: {start, stop} of every run's record chain
    DevBuf<uint64_t> d_run_bounds;
    DevBuf<uint32_t> d_member_run;
    if (span) {
        run_bounds.assign(2 * std::max<size_t>(runs.size(), 1), ~0ull);
        for (const BamPlan::ChunkAt &c : pl.chunk_at) {
            const uint64_t a = pl.uoff_of(c.s_idx) + c.ub, z = pl.uoff_of(c.e_idx) + c.ue;
            if (a < first_record || z < a || z > total_u) return belongs_not_here("a chunk starts inside the header or ends before it starts");
            // (the run that holds the chunk's first member; runs ascend by file offset)
            auto it = std::upper_bound(runs.begin(), runs.end(), c.cb, [](int64_t x, const BamPlan::Run &r) { return x < r.file_lo; });
            const size_t r = (size_t)(it - runs.begin()) - 1;
            if (run_bounds[2 * r] == ~0ull) run_bounds[2 * r] = a;
            run_bounds[2 * r + 1] = z;
        }
        for (size_t r = 0; r < runs.size(); ++r)
            if (run_bounds[2 * r] == ~0ull) run_bounds[2 * r] = run_bounds[2 * r + 1] = pl.uoff_of(runs[r].m1);
        rc = d_run_bounds.upload(run_bounds, st);
        if (rc == PC_OK) rc = d_member_run.upload(member_run, st);
        if (rc != PC_OK) return rc;
    }
    std::vector<MemberChain> chain((size_t)nm);
    std::vector<uint64_t> forced((size_t)nm, ~0ull);
    std::vector<uint32_t> nrec_of((size_t)nm, 0u);
    out.rec_base.assign((size_t)nm + 1, 0);
    if (nm) {
        HIP_TRY(hipMemsetAsync(d_forced.p, 0xff, (size_t)nm * 8, st));
        int from = 0;
        uint32_t cur_run = span ? member_run[0] : 0u;   // (region read: the run whose chain `expected` follows)
        uint64_t expected = span ? run_bounds[2 * (size_t)cur_run] : first_record;
        uint64_t stop_at = total_u;
        for (int round = 0;; ++round) {
            // (a whole-file read: one chain, no run tables -- both pointers are null)
            hipLaunchKernelGGL(span ? k_bam_chain<true> : k_bam_chain<false>, dim3((unsigned)(nm - from)), dim3(64), 0, st, d.d_stream.p, total_u, d.d_members.p, nm, from,
                               h.n_ref, first_record, d_forced.p, d.d_chain.p, d.d_rec_off.p, stop_at, (const uint32_t *)d_member_run.p, (const uint64_t *)d_run_bounds.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(chain.data() + from, d.d_chain.p + from, (size_t)(nm - from) * sizeof(MemberChain), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            int redo = -1;
            for (int m = from; m < nm; ++m) {
                if (span && member_run[(size_t)m] != cur_run) {   // each run settles from its forced start and has to end exactly at its stop
                    if (expected != run_bounds[2 * (size_t)cur_run + 1]) return belongs_not_here("a chunk ends inside a record");
                    cur_run = member_run[(size_t)m];
                    expected = run_bounds[2 * (size_t)cur_run];
                }
                const uint64_t stop_m = span ? run_bounds[2 * (size_t)cur_run + 1] : stop_at;
                const uint64_t begin = members[(size_t)m].uoff, end = std::min<uint64_t>(begin + members[(size_t)m].ulen, stop_m);
                nrec_of[(size_t)m] = 0;
                if (expected >= end) continue;                      // no record starts in this member (or it lies behind its run's last chunk)
                const MemberChain &mc = chain[(size_t)m];
                if (mc.first != expected) {                         // the guess was off (or there was none): walk again from the right place
                    forced[(size_t)m] = expected;
                    redo = m;
                    break;
                }
                nrec_of[(size_t)m] = mc.nrec;
                if (mc.flags & 2u) { out.truncated = true; from = nm; break; }   // a length prefix that cannot be: the walk ends here
                expected = mc.next;
            }
            if (redo < 0) break;
            out.chain_restarts += 1;
            HIP_TRY(hipMemcpyAsync(d_forced.p + redo, &forced[(size_t)redo], 8, hipMemcpyHostToDevice, st));
            from = redo;
            if (round > nm + 8) return fail(PC_ERR_STATE, "pc_bam_open: the record chain of %s did not settle", d.path.c_str());
        }
        if (span) stop_at = run_bounds[2 * (size_t)cur_run + 1];
        if (expected != stop_at) {   // the last record runs past (or stops short of) the end of the stream
            if (span) return belongs_not_here("a chunk ends inside a record");
            out.truncated = true;
        }
        for (int m = 0; m < nm; ++m) out.rec_base[(size_t)m + 1] = out.rec_base[(size_t)m] + nrec_of[(size_t)m];
        out.nrec = (int64_t)out.rec_base[(size_t)nm];
    } else if (total_u != first_record && !span) out.truncated = true;
    HIP_TRY(hipEventRecord(d.ev[3], st));
    d.clk.lap("header + record chain");
    return PC_OK;
}

// The first defect the record decode found (k_bam_order's lowest record index), as the error the host reader gives for it;
// PC_OK for kRecTruncated / kRecBadSize, which the caller reports after every other defect.
int record_defect(int code, const char *path) {
    using namespace pcbam;
    switch (code) {
    case kRecTidRange: return fail(PC_ERR_ARG, "BAM record with reference id out of range");
    case kRecNegPos: return fail(PC_ERR_ARG, "placed BAM record with a negative position");
    case kRecUnsorted: return fail(PC_ERR_UNSORTED, "BAM file is not coordinate sorted: %s", path);
    case kRecCigarOverrun: return fail(PC_ERR_ARG, "corrupt BAM record (cigar overruns block)");
    case kRecUnknownOp: return fail(PC_ERR_ARG, "unknown CIGAR operation in %s", path);
    case kRecEndBeyond: return fail(PC_ERR_ARG, "alignment ends beyond 2^31 - 1");
    case kRecTooLong: return fail(PC_ERR_ARG, "alignment with more than 2^31 - 1 aligned positions");
    case kRecDeletionOrder: return fail(PC_ERR_ARG, "alignment starting with a deletion breaks coordinate order; not supported");
    default: return PC_OK;
    }
}

// the member of every 256th record (k_bam_fields and its kin walk forward from there)
std::vector<uint32_t> group_members(const std::vector<uint64_t> &rec_base, int64_t nrec, int nm) {
    std::vector<uint32_t> rec_member((size_t)((nrec + 255) >> 8));
    int m = 0;
    for (size_t g = 0; g < rec_member.size(); ++g) {
        const uint64_t i = (uint64_t)g << 8;
        while (m + 1 < nm && rec_base[(size_t)m + 1] <= i) ++m;
        rec_member[g] = (uint32_t)m;
    }
    return rec_member;
}

// the events around the sort phase of an open with PC_BAM_SORT: key kernel [0, 1]; sort, ranks and run offsets [2, 3]
struct SortEvents {
    hipEvent_t ev[4] = {};
    int create() {
        for (auto &x : ev) HIP_TRY(hipEventCreate(&x));
        return PC_OK;
    }
    ~SortEvents() { for (auto x : ev) if (x) (void)hipEventDestroy(x); }
};

// Phase 5: fields, order checks (or, with `sort`, the coordinate sort), the region filter, the scans that place every kept record, and the columns of `b`.
int decode_columns(BamDecode &d, const BamPlan &pl, const BamSpan *span, const BamHeader &h, const BamRecords &recs, pc_bam &b, bool sort) {
    using namespace pcbam;
    hipStream_t st = d.st;
    const int nm = pl.nm();
    const uint64_t total_u = pl.total_u;
    const int64_t nrec = recs.nrec;
    bool truncated = recs.truncated;
    DevBuf<uint64_t> d_rec_base;
    DevBuf<uint32_t> d_rec_member, d_placed, d_runs, d_staged_at, d_run_at, d_wide;
    DevBuf<RecOut> d_recs;
    DevBuf<unsigned long long> d_misc;   // [0] first error (index << 8 | code), [1] mapped, [2] unplaced; with `sort`: [3] out of order, [4] records moved
    int rc = d_misc.reserve(6);
    if (rc != PC_OK) return rc;
    const unsigned long long misc0[6] = {~0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    HIP_TRY(hipMemcpyAsync(d_misc.p, misc0, sizeof(misc0), hipMemcpyHostToDevice, st));
    int64_t n_staged = 0, n_runs = 0;
    if (nrec > 0) {
        const std::vector<uint32_t> rec_member = group_members(recs.rec_base, nrec, nm);
        rc = d_rec_base.upload(recs.rec_base, st);
        if (rc == PC_OK) rc = d_rec_member.upload(rec_member, st);
        room(rc, d_recs, (size_t)nrec);
        room(rc, d_placed, (size_t)nrec + 1); room(rc, d_runs, (size_t)nrec + 1); room(rc, d_staged_at, (size_t)nrec + 1); room(rc, d_run_at, (size_t)nrec + 1);
        if (rc != PC_OK) return rc;
        const unsigned g256 = (unsigned)((nrec + 255) / 256);
        hipLaunchKernelGGL(k_bam_fields, dim3(g256), dim3(256), 0, st, d.d_stream.p, total_u, d.d_members.p, d_rec_base.p, d.d_chain.p, d.d_rec_off.p, nm, nrec,
                           h.n_ref, d_rec_member.p, d_recs.p);
        // `sort`: the keys first; a file they find in order goes on exactly as without the flag
        DevBuf<uint64_t> d_key, d_key2;
        DevBuf<uint32_t> d_idx, d_idx2, d_runs_sorted;
        SortEvents sev;
        bool disorder = false;
        if (sort) {
            room(rc, d_key, (size_t)nrec); room(rc, d_idx, (size_t)nrec);
            if (rc == PC_OK) rc = sev.create();
            if (rc != PC_OK) return rc;
            unsigned long long dis = 0;
            HIP_TRY(hipEventRecord(sev.ev[0], st));
            hipLaunchKernelGGL(k_bam_sort_keys, dim3(g256), dim3(256), 0, st, d_recs.p, nrec, d_key.p, d_idx.p, d_misc.p + 3);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(sev.ev[1], st));
            HIP_TRY(hipMemcpyAsync(&dis, d_misc.p + 3, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            disorder = dis != 0;
            b.sorted_input = !disorder;
            if (!disorder) { d_key.release(); d_idx.release(); }
        }
        if (!disorder) hipLaunchKernelGGL(k_bam_order, dim3(g256), dim3(256), 0, st, d_recs.p, nrec, d_placed.p, d_misc.p);
        DevBuf<int32_t> d_rtid;
        DevBuf<int64_t> d_rbe;
        if (span) {   // keep what overlaps a requested region (htslib's overlap rule); everything else is as if it were not in the file
            const size_t nr = (size_t)std::max(span->nreg, 0);
            rc = d_rtid.upload(span->tid, nr, st);
            if (rc == PC_OK) rc = d_rbe.reserve(2 * std::max<size_t>(nr, 1));
            if (rc != PC_OK) return rc;
            if (nr) {
                HIP_TRY(hipMemcpyAsync(d_rbe.p, span->beg, nr * 8, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(d_rbe.p + nr, span->end, nr * 8, hipMemcpyHostToDevice, st));
            }
            hipLaunchKernelGGL(k_bam_region_filter, dim3(g256), dim3(256), 0, st, d_recs.p, nrec, (int)nr, d_rtid.p, d_rbe.p, d_rbe.p + nr);
        }
        HIP_TRY(hipMemsetAsync(d_placed.p + nrec, 0, 4, st));
        HIP_TRY(hipMemsetAsync(d_runs.p + nrec, 0, 4, st));
        hipLaunchKernelGGL(k_bam_scan_inputs, dim3((unsigned)((nrec + 256 * kScanInputsPerThread - 1) / (256 * kScanInputsPerThread))), dim3(256), 0, st, d_recs.p, nrec, d_placed.p, d_runs.p, d_misc.p + 1);
        {
            size_t tmp_bytes = 0;
            HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_placed.p, d_staged_at.p, (int)(nrec + 1), st));
            DevBuf<uint8_t> d_tmp;
            rc = d_tmp.reserve(std::max<size_t>(tmp_bytes, 16));
            if (rc != PC_OK) return rc;
            HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, tmp_bytes, d_placed.p, d_staged_at.p, (int)(nrec + 1), st));
            HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, tmp_bytes, d_runs.p, d_run_at.p, (int)(nrec + 1), st));
            // Out of order: one stable radix sort of (key, record number) over the key bits in use, then staged_at and run_at
            // by rank in the sorted order (the totals stay those of the two scans above).  Placed records sort first.
            DevBuf<uint8_t> d_sort_tmp;
            if (disorder) {
                const int key_bits = sort_key_bits(h.n_ref);
                room(rc, d_key2, (size_t)nrec); room(rc, d_idx2, (size_t)nrec); room(rc, d_runs_sorted, (size_t)nrec + 1);
                if (rc != PC_OK) return rc;
                HIP_TRY(hipEventRecord(sev.ev[2], st));
                // (double buffers: the passes go back and forth between the two halves, and the sort says which half holds the result)
                hipcub::DoubleBuffer<uint64_t> keys(d_key.p, d_key2.p);
                hipcub::DoubleBuffer<uint32_t> vals(d_idx.p, d_idx2.p);
                size_t sort_bytes = 0;
                HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, keys, vals, (int)nrec, 0, key_bits, st));
                rc = d_sort_tmp.reserve(std::max<size_t>(sort_bytes, 16));
                if (rc != PC_OK) { (void)hipStreamSynchronize(st); return rc; }
                HIP_TRY(hipcub::DeviceRadixSort::SortPairs(d_sort_tmp.p, sort_bytes, keys, vals, (int)nrec, 0, key_bits, st));
                const uint32_t *perm = vals.Current();
                b.file_order.swap(perm == d_idx.p ? d_idx : d_idx2);   // (the permutation is the staged records' numbers in the file)
                HIP_TRY(hipMemsetAsync(d_runs_sorted.p + nrec, 0, 4, st));
                hipLaunchKernelGGL(k_bam_sort_rank, dim3(g256), dim3(256), 0, st, d_recs.p, nrec, perm, d_staged_at.p, d_runs_sorted.p, d_misc.p, d_misc.p + 4);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, tmp_bytes, d_runs_sorted.p, d_runs_sorted.p, (int)(nrec + 1), st));   // (in place)
                hipLaunchKernelGGL(k_bam_sort_run_at, dim3(g256), dim3(256), 0, st, perm, d_runs_sorted.p, nrec, d_run_at.p);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipEventRecord(sev.ev[3], st));
                b.key_bits = key_bits;
            }
            uint32_t tot[2] = {0, 0};
            unsigned long long misc[5] = {0, 0, 0, 0, 0};
            HIP_TRY(hipMemcpyAsync(&tot[0], d_staged_at.p + nrec, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(&tot[1], d_run_at.p + nrec, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(misc, d_misc.p, sizeof(misc), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));   // (d_tmp and the sort's buffers go out of scope)
            n_staged = tot[0]; n_runs = tot[1];
            b.mapped = (int64_t)misc[1]; b.unplaced = (int64_t)misc[2];
            if (sort) {
                b.sort_ms = ms_between(sev.ev[0], sev.ev[1]) + (disorder ? ms_between(sev.ev[2], sev.ev[3]) : 0.0);
                b.moved = (int64_t)misc[4];
                if (!b.moved) b.file_order.release();
            }
            if (misc[0] != ~0ull) {
                rc = record_defect((int)(misc[0] & 0xffu), d.path.c_str());
                if (rc != PC_OK) return rc;
                truncated = true;   // kRecTruncated / kRecBadSize: reported below, after every other defect
            }
        }
        if (truncated) return fail(PC_ERR_ARG, "truncated BAM record");
        const size_t ns = (size_t)std::max<int64_t>(n_staged, 1), nrun = (size_t)std::max<int64_t>(n_runs, 1);   // (no empty column)
        room(rc, b.tid, ns); room(rc, b.pos, ns); room(rc, b.alen, ns); room(rc, b.flags, ns); room(rc, b.nblk, ns);
        room(rc, b.flag16, ns); room(rc, b.mapq, ns); room(rc, b.lseq, ns); room(rc, b.nh, ns);
        room(rc, b.blk_start, nrun); room(rc, b.blk_len, nrun);
        room(rc, d_wide, ns);
        if (rc != PC_OK) return rc;
        HIP_TRY(hipMemsetAsync(d_wide.p, 0, ns * 4, st));
        hipLaunchKernelGGL(k_bam_columns, dim3(g256), dim3(256), 0, st, d.d_stream.p, d.d_members.p, d_rec_base.p, d.d_rec_off.p, nm, d_rec_member.p, d_recs.p,
                           nrec, d_staged_at.p, d_run_at.p, b.tid.p, b.pos.p, b.alen.p, b.flags.p, b.nblk.p, b.blk_start.p, b.blk_len.p, d_wide.p,
                           b.flag16.p, b.mapq.p, b.lseq.p, b.nh.p);
        HIP_TRY(hipGetLastError());
        // wide records (beyond the 16-bit / 8-bit columns): rare -- their staged indices are found from the markers on
        // the host side of pc_bam_read; the true values are read back here, record by record
        {
            // count the flagged records (a sum reduction through the scan buffers would do; a plain read-back of the
            // flags is only paid when the file has any: probe with a device-side total first)
            DevBuf<uint32_t> d_wsum;
            rc = d_wsum.reserve((size_t)n_staged + 1);
            if (rc != PC_OK) return rc;
            size_t tmp_bytes = 0;
            HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_wide.p, d_wsum.p, (int)std::max<int64_t>(n_staged, 1), st));
            DevBuf<uint8_t> d_tmp;
            rc = d_tmp.reserve(std::max<size_t>(tmp_bytes, 16));
            if (rc != PC_OK) return rc;
            uint32_t last_sum = 0, last_flag = 0;
            if (n_staged > 0) {
                HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, tmp_bytes, d_wide.p, d_wsum.p, (int)n_staged, st));
                HIP_TRY(hipMemcpyAsync(&last_sum, d_wsum.p + (n_staged - 1), 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpyAsync(&last_flag, d_wide.p + (n_staged - 1), 4, hipMemcpyDeviceToHost, st));
            }
            HIP_TRY(hipStreamSynchronize(st));
            const uint32_t nwide = last_sum + last_flag;
            if (nwide) {
                std::vector<uint32_t> wf((size_t)n_staged), sa((size_t)nrec);
                std::vector<RecOut> ro((size_t)nrec);
                HIP_TRY(hipMemcpy(wf.data(), d_wide.p, (size_t)n_staged * 4, hipMemcpyDeviceToHost));
                HIP_TRY(hipMemcpy(sa.data(), d_staged_at.p, (size_t)nrec * 4, hipMemcpyDeviceToHost));
                HIP_TRY(hipMemcpy(ro.data(), d_recs.p, (size_t)nrec * sizeof(RecOut), hipMemcpyDeviceToHost));
                for (int64_t i = 0; i < nrec; ++i)
                    if (ro[(size_t)i].placed == 1 && wf[sa[(size_t)i]]) {
                        b.wide_idx.push_back((int64_t)sa[(size_t)i]);
                        b.wide_alen.push_back((int32_t)ro[(size_t)i].L);
                        b.wide_nblk.push_back((int32_t)ro[(size_t)i].nruns);
                    }
                if (b.moved) {   // the walk above is in file order: the list is kept ascending by staged index
                    std::vector<size_t> by((size_t)b.wide_idx.size());
                    std::iota(by.begin(), by.end(), (size_t)0);
                    std::sort(by.begin(), by.end(), [&](size_t x, size_t y) { return b.wide_idx[x] < b.wide_idx[y]; });
                    const std::vector<int64_t> wi = b.wide_idx;
                    const std::vector<int32_t> wa = b.wide_alen, wn = b.wide_nblk;
                    for (size_t k = 0; k < by.size(); ++k) { b.wide_idx[k] = wi[by[k]]; b.wide_alen[k] = wa[by[k]]; b.wide_nblk[k] = wn[by[k]]; }
                }
            }
        }
    } else if (truncated) return fail(PC_ERR_ARG, "truncated BAM record");
    HIP_TRY(hipEventRecord(d.ev[4], st));
    HIP_TRY(hipStreamSynchronize(st));
    d.clk.lap("fields + scans + columns");
    b.n = n_staged; b.nrun = n_runs;
    return PC_OK;
}

using pcshape::IndexShape;   // the index to build: BAI (min_shift 14, 5 levels), or a CSI of the given shape

// What index_records brings down for pc_bam_index_finish / pc_bam_index_finish_csi.
struct IndexParts {
    std::vector<int32_t> run_tid;
    std::vector<uint32_t> run_bin;
    std::vector<uint64_t> run_beg, run_end, run_loff, linear, ref_beg, ref_end;   // linear: BAI only; run_loff: CSI only
    std::vector<int64_t> lin_start, ref_mapped, ref_unmapped;
    int64_t n_no_coor = 0, n_windows = 0;
    double ms_fields = 0, ms_kernels = 0, ms_readback = 0;   // wall clock between the phase's synchronisations
};

// The index build's phase 5 (whole-file reads only): k_bam_fields and the order checks as decode_columns runs them -- no
// column is written or read back -- then the kernels of index_kernels.hip.h; the sorted runs, the linear arrays (BAI) or
// the runs' loff (CSI: the windows stay in HBM) and the per-reference counts come down.
int index_records(BamDecode &d, const BamPlan &pl, int64_t size, const BamHeader &h, const BamRecords &recs, const IndexShape &shape, IndexParts &out) {
    using namespace pcbam;
    using namespace pcidx;
    hipStream_t st = d.st;
    const int nm = pl.nm();
    const int64_t nrec = recs.nrec;
    const int n_ref = (int)h.n_ref;
    const auto t0 = std::chrono::steady_clock::now();
    auto ms_since = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); };
    out.lin_start.assign((size_t)n_ref + 1, 0);
    out.ref_beg.assign((size_t)n_ref, 0); out.ref_end.assign((size_t)n_ref, 0);
    out.ref_mapped.assign((size_t)n_ref, 0); out.ref_unmapped.assign((size_t)n_ref, 0);
    if (nrec == 0) {
        if (recs.truncated) return fail(PC_ERR_ARG, "truncated BAM record");
        return PC_OK;
    }
    // where bgzf_tell places a stream position (bgzf.c:569-572): per member, the file offset of the first gzip header whose
    // payload begins where the member's does -- an empty member in front of it, if there is one -- and of its own header; the
    // end of the stream lies in the first member behind the last payload (the EOF block), or at the end of the file
    std::vector<uint64_t> blk(2 * (size_t)nm + 2);
    {
        uint64_t prev_end = 0;
        for (int m = 0; m < nm; ++m) {
            const Member &mb = pl.members[(size_t)m];
            const uint64_t own = mb.coff - mb.hdr;
            blk[2 * (size_t)m] = std::min(prev_end, own); blk[2 * (size_t)m + 1] = own;
            prev_end = mb.coff + mb.clen + 8;
        }
        blk[2 * (size_t)nm] = blk[2 * (size_t)nm + 1] = std::min<uint64_t>(prev_end, (uint64_t)size);
    }
    DevBuf<uint64_t> d_rec_base, d_blk, d_key, d_voff, d_cov, d_covered;
    DevBuf<uint32_t> d_rec_member, d_placed, d_mapped, d_mapped_before, d_head, d_slot;
    DevBuf<int32_t> d_win_a;
    DevBuf<RecOut> d_recs;
    DevBuf<unsigned long long> d_misc;   // [0] first error (index << 8 | code); [1] (as uint32) a record reaches beyond 2^29
    DevBuf<int64_t> d_ref_fl;            // first record of every reference, then the last
    const size_t n1 = (size_t)nrec + 1, nr = (size_t)std::max(n_ref, 1);
    int rc = d_misc.reserve(2);
    room(rc, d_recs, (size_t)nrec); room(rc, d_placed, 1);
    room(rc, d_key, (size_t)nrec); room(rc, d_voff, n1); room(rc, d_cov, n1); room(rc, d_covered, n1); room(rc, d_win_a, (size_t)nrec);
    room(rc, d_mapped, n1); room(rc, d_mapped_before, n1); room(rc, d_head, n1); room(rc, d_slot, n1); room(rc, d_ref_fl, 2 * nr);
    if (rc == PC_OK) rc = d_rec_base.upload(recs.rec_base, st);
    const std::vector<uint32_t> rec_member = group_members(recs.rec_base, nrec, nm);
    if (rc == PC_OK) rc = d_rec_member.upload(rec_member, st);
    if (rc == PC_OK) rc = d_blk.upload(blk, st);
    if (rc != PC_OK) return rc;
    const unsigned long long misc0[2] = {~0ull, 0ull};
    HIP_TRY(hipMemcpyAsync(d_misc.p, misc0, sizeof(misc0), hipMemcpyHostToDevice, st));
    const unsigned g256 = (unsigned)((nrec + 255) / 256), g256p = (unsigned)((nrec + 1 + 255) / 256);
    hipLaunchKernelGGL(k_bam_fields, dim3(g256), dim3(256), 0, st, d.d_stream.p, pl.total_u, d.d_members.p, d_rec_base.p, d.d_chain.p, d.d_rec_off.p, nm, nrec,
                       h.n_ref, d_rec_member.p, d_recs.p);
    hipLaunchKernelGGL(k_bam_order, dim3(g256), dim3(256), 0, st, d_recs.p, nrec, d_placed.p, d_misc.p);
    HIP_TRY(hipGetLastError());
    unsigned long long misc[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(misc, d_misc.p, sizeof(misc), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out.ms_fields = ms_since(t0);
    if (misc[0] != ~0ull) {   // the decoder's own refusals, in its order
        rc = record_defect((int)(misc[0] & 0xffu), d.path.c_str());
        return rc != PC_OK ? rc : fail(PC_ERR_ARG, "truncated BAM record");
    }
    if (recs.truncated) return fail(PC_ERR_ARG, "truncated BAM record");
    const auto t1 = std::chrono::steady_clock::now();
    // ---- keys, runs, per-reference bounds, covered windows
    const auto idx_keys = shape.csi ? k_idx_keys<false> : k_idx_keys<true>;
    hipLaunchKernelGGL(idx_keys, dim3(g256p), dim3(256), 0, st, d.d_stream.p, d.d_members.p, d_blk.p, d_rec_base.p, d.d_rec_off.p, nm, nrec, d_rec_member.p,
                       d_recs.p, d_key.p, d_voff.p, d_win_a.p, d_cov.p, d_mapped.p, (uint32_t *)(d_misc.p + 1), shape.min_shift, shape.n_lvls);
    HIP_TRY(hipMemsetAsync(d_ref_fl.p, 0xff, 2 * nr * sizeof(int64_t), st));
    hipLaunchKernelGGL(k_idx_heads, dim3(g256p), dim3(256), 0, st, d_key.p, nrec, d_head.p, d_ref_fl.p, d_ref_fl.p + nr);
    HIP_TRY(hipGetLastError());
    DevBuf<uint8_t> d_tmp;
    {
        size_t a = 0, b = 0;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, a, d_head.p, d_slot.p, (int)n1, st));
        HIP_TRY(hipcub::DeviceScan::ExclusiveScan(nullptr, b, d_cov.p, d_covered.p, hipcub::Max(), (uint64_t)0, (int)n1, st));
        size_t tmp_bytes = std::max<size_t>(std::max(a, b), 16);
        rc = d_tmp.reserve(tmp_bytes);
        if (rc != PC_OK) return rc;
        a = b = tmp_bytes;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, a, d_head.p, d_slot.p, (int)n1, st));
        a = tmp_bytes;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, a, d_mapped.p, d_mapped_before.p, (int)n1, st));
        HIP_TRY(hipcub::DeviceScan::ExclusiveScan(d_tmp.p, b, d_cov.p, d_covered.p, hipcub::Max(), (uint64_t)0, (int)n1, st));
    }
    DevBuf<uint64_t> d_ref_be;     // per reference: offset of its first record, then of the first record behind its last
    DevBuf<int64_t> d_ref_cnt;     // mapped, then unmapped
    DevBuf<int32_t> d_n_intv;
    room(rc, d_ref_be, 2 * nr); room(rc, d_ref_cnt, 2 * nr); room(rc, d_n_intv, nr);
    if (rc != PC_OK) return rc;
    std::vector<int32_t> n_intv((size_t)n_ref, 0);
    uint32_t n_runs32 = 0;
    if (n_ref) {
        hipLaunchKernelGGL(k_idx_ref_stats, dim3((unsigned)((n_ref + 255) / 256)), dim3(256), 0, st, n_ref, d_ref_fl.p, d_ref_fl.p + nr, d_voff.p, d_mapped_before.p,
                           d_covered.p, d_ref_be.p, d_ref_be.p + nr, d_ref_cnt.p, d_ref_cnt.p + nr, d_n_intv.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(n_intv.data(), d_n_intv.p, (size_t)n_ref * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out.ref_beg.data(), d_ref_be.p, (size_t)n_ref * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out.ref_end.data(), d_ref_be.p + nr, (size_t)n_ref * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out.ref_mapped.data(), d_ref_cnt.p, (size_t)n_ref * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out.ref_unmapped.data(), d_ref_cnt.p + nr, (size_t)n_ref * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(&n_runs32, d_slot.p + nrec, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(misc, d_misc.p, sizeof(misc), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((uint32_t)misc[1]) {
        if (!shape.csi) return fail(PC_ERR_ARG, "a BAI index cannot hold %s: an alignment reaches beyond 2^29", d.path.c_str());
        return fail(PC_ERR_ARG, "a CSI index of min_shift %d and depth %d cannot hold %s: an alignment reaches beyond %lld", shape.min_shift, shape.n_lvls,
                    d.path.c_str(), (long long)shape.reach());
    }
    int64_t placed = 0;
    for (int t = 0; t < n_ref; ++t) {
        out.lin_start[(size_t)t + 1] = out.lin_start[(size_t)t] + n_intv[(size_t)t];
        placed += out.ref_mapped[(size_t)t] + out.ref_unmapped[(size_t)t];
    }
    out.n_no_coor = nrec - placed;
    const int64_t n_runs = (int64_t)n_runs32, n_lin = out.lin_start[(size_t)n_ref];
    out.n_windows = n_lin;
    if (shape.csi && n_lin > kMaxWindows)
        return fail(PC_ERR_ARG, "a CSI index of min_shift %d of %s has %lld windows, more than 2^28: use a larger min_shift", shape.min_shift, d.path.c_str(),
                    (long long)n_lin);
    // ---- the runs in (tid, bin) order, the linear windows
    DevBuf<uint64_t> d_run_key, d_run_key2, d_run_beg, d_run_end, d_sbeg, d_send, d_linear, d_filled, d_sloff;
    DevBuf<uint32_t> d_order, d_order2, d_sbin;
    DevBuf<int32_t> d_stid;
    DevBuf<int64_t> d_lin_base;
    const size_t nrun = (size_t)std::max<int64_t>(n_runs, 1);
    room(rc, d_run_key, nrun); room(rc, d_run_key2, nrun); room(rc, d_run_beg, nrun); room(rc, d_run_end, nrun); room(rc, d_sbeg, nrun); room(rc, d_send, nrun);
    room(rc, d_order, nrun); room(rc, d_order2, nrun); room(rc, d_sbin, nrun); room(rc, d_stid, nrun);
    room(rc, d_linear, (size_t)std::max<int64_t>(n_lin, 1));
    if (shape.csi) { room(rc, d_filled, (size_t)std::max<int64_t>(n_lin, 1)); room(rc, d_sloff, nrun); }
    if (rc == PC_OK) rc = d_lin_base.upload(out.lin_start, st);
    if (rc != PC_OK) return rc;
    out.run_tid.resize((size_t)n_runs); out.run_bin.resize((size_t)n_runs); out.run_beg.resize((size_t)n_runs); out.run_end.resize((size_t)n_runs);
    if (shape.csi) out.run_loff.resize((size_t)n_runs);
    else out.linear.resize((size_t)n_lin);
    if (n_runs) {
        hipLaunchKernelGGL(k_idx_runs, dim3(g256p), dim3(256), 0, st, d_key.p, d_voff.p, d_head.p, d_slot.p, nrec, d_run_key.p, d_run_beg.p, d_run_end.p);
        // (hipcub's iota: the slots 0 .. n_runs - 1 are the values of the sort)
        std::vector<uint32_t> iota((size_t)n_runs);
        std::iota(iota.begin(), iota.end(), 0u);
        HIP_TRY(hipMemcpyAsync(d_order.p, iota.data(), (size_t)n_runs * 4, hipMemcpyHostToDevice, st));
        int key_bits = 32;   // bin below, then as many bits as the reference ids take
        while (key_bits < 64 && ((uint64_t)n_ref >> (key_bits - 32))) ++key_bits;
        size_t sort_bytes = 0;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, d_run_key.p, d_run_key2.p, d_order.p, d_order2.p, (int)n_runs, 0, key_bits, st));
        DevBuf<uint8_t> d_sort_tmp;
        rc = d_sort_tmp.reserve(std::max<size_t>(sort_bytes, 16));
        if (rc != PC_OK) { (void)hipStreamSynchronize(st); return rc; }
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(d_sort_tmp.p, sort_bytes, d_run_key.p, d_run_key2.p, d_order.p, d_order2.p, (int)n_runs, 0, key_bits, st));
        hipLaunchKernelGGL(k_idx_gather, dim3((unsigned)((n_runs + 255) / 256)), dim3(256), 0, st, d_run_key2.p, d_order2.p, d_run_beg.p, d_run_end.p, n_runs,
                           d_stid.p, d_sbin.p, d_sbeg.p, d_send.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));   // (iota and the sort's scratch go out of scope)
    }
    if (n_lin) {
        HIP_TRY(hipMemsetAsync(d_linear.p, 0, (size_t)n_lin * 8, st));
        hipLaunchKernelGGL(k_idx_linear, dim3(g256), dim3(256), 0, st, d_cov.p, d_covered.p, d_win_a.p, d_voff.p, nrec, d_lin_base.p, d_linear.p);
        HIP_TRY(hipGetLastError());
    }
    DevBuf<uint8_t> d_fill_tmp;   // (the scan's scratch: alive up to the synchronisation below)
    if (shape.csi && n_runs) {   // the forward fill (one running maximum over the windows of all references), then loff per run
        if (n_lin) {
            hipLaunchKernelGGL(k_idx_first_window, dim3((unsigned)((n_ref + 255) / 256)), dim3(256), 0, st, n_ref, d_n_intv.p, d_lin_base.p, d_ref_be.p, d_linear.p);
            HIP_TRY(hipGetLastError());
            size_t fill_bytes = 0;
            HIP_TRY(hipcub::DeviceScan::InclusiveScan(nullptr, fill_bytes, d_linear.p, d_filled.p, hipcub::Max(), (int)n_lin, st));
            rc = d_fill_tmp.reserve(std::max<size_t>(fill_bytes, 16));
            if (rc != PC_OK) { (void)hipStreamSynchronize(st); return rc; }
            HIP_TRY(hipcub::DeviceScan::InclusiveScan(d_fill_tmp.p, fill_bytes, d_linear.p, d_filled.p, hipcub::Max(), (int)n_lin, st));
        }
        hipLaunchKernelGGL(k_idx_loff, dim3((unsigned)((n_runs + 255) / 256)), dim3(256), 0, st, d_stid.p, d_sbin.p, n_runs, shape.n_lvls, d_n_intv.p,
                           d_lin_base.p, d_filled.p, d_sloff.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));
    out.ms_kernels = ms_since(t1);
    const auto t2 = std::chrono::steady_clock::now();
    if (n_runs) {
        HIP_TRY(hipMemcpyAsync(out.run_tid.data(), d_stid.p, (size_t)n_runs * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out.run_bin.data(), d_sbin.p, (size_t)n_runs * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out.run_beg.data(), d_sbeg.p, (size_t)n_runs * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out.run_end.data(), d_send.p, (size_t)n_runs * 8, hipMemcpyDeviceToHost, st));
    }
    if (shape.csi) { if (n_runs) HIP_TRY(hipMemcpyAsync(out.run_loff.data(), d_sloff.p, (size_t)n_runs * 8, hipMemcpyDeviceToHost, st)); }
    else if (n_lin) HIP_TRY(hipMemcpyAsync(out.linear.data(), d_linear.p, (size_t)n_lin * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out.ms_readback = ms_since(t2);
    d.clk.lap("fields + index kernels + read-back");
    return PC_OK;
}

} // namespace

// One open: the five phases above, in order.  `span`: a region read (its chunk list and regions); nullptr: the whole file.
static int bam_open_impl(pc_engine *e, const void *image_, int64_t size, const char *name, pc_bam **out, const UploadedHook *uploaded, const BamSpan *span,
                         const BamKnobs &knobs, uint32_t flags = 0) {
    if (!e || !out || size < 0 || (size > 0 && !image_)) return fail(PC_ERR_ARG, "pc_bam_open: bad arguments");
    *out = nullptr;
    if ((flags & ~(uint32_t)PC_BAM_SORT) || (flags && span)) return fail(PC_ERR_ARG, "pc_bam_open: unknown flags (PC_BAM_SORT is the one there is, for whole-file reads)");
    const bool sort = (flags & PC_BAM_SORT) != 0;
    const uint8_t *image = (const uint8_t *)image_;
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);   // (the decoder's scratch -- image, inflated stream, record table -- is recycled through the engine's pool)
    BamDecode d{e, e->stream, name ? name : "<memory>", knobs};
    BamPlan pl;
    int rc = plan_members(image, size, span, d.path.c_str(), knobs.walk_min, pl);
    if (rc != PC_OK) return rc;
    pc_bam *b = new pc_bam();
    d.clk.lap("member walk");
    b->e = e; b->name = d.path; b->members = (int64_t)pl.nm(); b->inflated_bytes = (int64_t)pl.total_u; b->compressed_bytes = size;
    b->uploaded_bytes = pl.image_bytes; b->runs = (int64_t)pl.runs.size();
    struct Guard { pc_bam *b; ~Guard() { if (b) pc_bam_close(b); } } guard{b};
    for (auto &x : d.ev) HIP_TRY(hipEventCreate(&x));
    struct EvGuard { hipEvent_t *ev; ~EvGuard() { for (int i = 0; i < 5; ++i) (void)hipEventDestroy(ev[i]); } } evg{d.ev};
    rc = upload_and_inflate(d, image, pl, uploaded);
    if (rc != PC_OK) return rc;
    BamHeader h;
    rc = read_header(d, pl, size, span, h);
    if (rc != PC_OK) return rc;
    BamRecords recs;
    rc = chain_records(d, pl, span, h, recs);
    if (rc != PC_OK) return rc;
    b->ref_names = std::move(h.ref_names); b->ref_lengths = std::move(h.ref_lengths);
    b->chain_restarts = recs.chain_restarts; b->total = recs.nrec;
    if (recs.nrec >= (int64_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_bam_open: more than 2^31-2 records per file are not supported");
    b->sort_requested = sort;
    b->key_bits = 0;
    rc = decode_columns(d, pl, span, h, recs, *b, sort);
    if (rc != PC_OK) return rc;
    for (int k = 0; k < 4; ++k) b->ms[k] = ms_between(d.ev[k], d.ev[k + 1]);
    guard.b = nullptr;
    *out = b;
    return PC_OK;
}

// The index build: phases 1 - 4 of a whole-file open, index_records, pc_bam_index_finish.
// min_shift 0: a BAI; otherwise the CSI with leaves of 2^min_shift positions (its range is the caller's check) and the depth the header asks for.
static int bam_index_impl(pc_engine *e, const void *image_, int64_t size, const char *name, pc_bam_index **out, const UploadedHook *uploaded, const BamKnobs &knobs,
                          int min_shift = 0) {
    if (!e || !out || size < 0 || (size > 0 && !image_)) return fail(PC_ERR_ARG, "pc_bam_index_build: bad arguments");
    *out = nullptr;
    const auto t_0 = std::chrono::steady_clock::now();
    const uint8_t *image = (const uint8_t *)image_;
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    BamDecode d{e, e->stream, name ? name : "<memory>", knobs};
    BamPlan pl;
    int rc = plan_members(image, size, nullptr, d.path.c_str(), knobs.walk_min, pl);
    if (rc != PC_OK) return rc;
    d.clk.lap("member walk");
    for (auto &x : d.ev) HIP_TRY(hipEventCreate(&x));
    struct EvGuard { hipEvent_t *ev; ~EvGuard() { for (int i = 0; i < 5; ++i) (void)hipEventDestroy(ev[i]); } } evg{d.ev};
    rc = upload_and_inflate(d, image, pl, uploaded);
    if (rc != PC_OK) return rc;
    BamHeader h;
    rc = read_header(d, pl, size, nullptr, h);
    if (rc != PC_OK) return rc;
    BamRecords recs;
    rc = chain_records(d, pl, nullptr, h, recs);
    if (rc != PC_OK) return rc;
    if (recs.nrec >= (int64_t)0x7fffffff) return fail(PC_ERR_ARG, "pc_bam_index_build: more than 2^31-2 records per file are not supported");
    IndexShape shape;
    if (min_shift) {   // the depth as htslib takes it from the header (sam.c:478-482)
        int64_t max_len = 0;
        for (size_t t = 0; t < h.ref_lengths.size(); ++t) max_len = std::max<int64_t>(max_len, (int64_t)(uint32_t)h.ref_lengths[t]);
        max_len += 256;
        shape.csi = true; shape.min_shift = min_shift; shape.n_lvls = 0;
        while (max_len > shape.reach()) ++shape.n_lvls;
    }
    IndexParts parts;
    rc = index_records(d, pl, size, h, recs, shape, parts);
    if (rc != PC_OK) return rc;
    if (!shape.csi)
        for (size_t t = 0; t < h.ref_lengths.size(); ++t)   // (behind the decoder's own refusals)
            if ((int64_t)h.ref_lengths[t] > pcidx::kBaiReach || h.ref_lengths[t] < 0)
                return fail(PC_ERR_ARG, "a BAI index cannot hold %s: reference %s is longer than 2^29", d.path.c_str(), h.ref_names[t].c_str());
    const auto t_f = std::chrono::steady_clock::now();
    pc_bam_index *idx = nullptr;
    if (shape.csi)
        rc = pc_bam_index_finish_csi(shape.min_shift, shape.n_lvls, (int)h.n_ref, (int64_t)parts.run_tid.size(), parts.run_tid.data(), parts.run_bin.data(),
                                     parts.run_beg.data(), parts.run_end.data(), parts.run_loff.data(), parts.ref_beg.data(), parts.ref_end.data(),
                                     parts.ref_mapped.data(), parts.ref_unmapped.data(), parts.n_no_coor, &idx);
    else rc = pc_bam_index_finish((int)h.n_ref, (int64_t)parts.run_tid.size(), parts.run_tid.data(), parts.run_bin.data(), parts.run_beg.data(), parts.run_end.data(),
                             parts.lin_start.data(), parts.linear.data(), parts.ref_beg.data(), parts.ref_end.data(), parts.ref_mapped.data(),
                             parts.ref_unmapped.data(), parts.n_no_coor, &idx);
    if (rc != PC_OK) return rc;
    if (shape.csi) idx->stats[5] = parts.n_windows;
    const auto t_e = std::chrono::steady_clock::now();
    for (int k = 0; k < 3; ++k) idx->ms[k] = ms_between(d.ev[k], d.ev[k + 1]);
    idx->ms[3] = parts.ms_fields; idx->ms[4] = parts.ms_kernels; idx->ms[5] = parts.ms_readback;
    idx->ms[6] = std::chrono::duration<double, std::milli>(t_e - t_f).count();
    idx->ms[7] = std::chrono::duration<double, std::milli>(t_e - t_0).count();
    *out = idx;
    return PC_OK;
}

// a region read comes back for a larger slice of the file's head when the header did not fit the first one
static int bam_open_span_retry(pc_engine *e, const void *image, int64_t size, const char *name, pc_bam **out, const UploadedHook *uploaded, const BamSpan *span,
                               const BamKnobs &knobs, uint32_t flags = 0) {
    if (!span) return bam_open_impl(e, image, size, name, out, uploaded, nullptr, knobs, flags);
    BamSpan sp = *span;
    sp.header_bytes = knobs.header_bytes;
    for (;;) {
        const int rc = bam_open_impl(e, image, size, name, out, uploaded, &sp, knobs);
        if (rc != PC_RETRY_HEADER) return rc;
        sp.header_bytes = std::min<int64_t>(size, sp.header_bytes * 16);
    }
}

static int add_alignment_bam_impl(pc_engine *e, const void *image, int64_t size, const char *name, int64_t *mapped, const UploadedHook *uploaded,
                                  const BamSpan *span, const BamKnobs &knobs, uint32_t open_flags = 0) {
    pc_bam *b = nullptr;
    int rc = bam_open_span_retry(e, image, size, name, &b, uploaded, span, knobs, open_flags);
    if (rc != PC_OK) return rc;
    struct Closer { pc_bam *b; ~Closer() { pc_bam_close(b); } } closer{b};
    PoolScope pool_scope(&e->pool);
    const int64_t n = b->n, m = b->nrun, nw = (int64_t)b->wide_idx.size();
    const int ntid = std::max(1, (int)b->ref_names.size());
    if (mapped) *mapped = b->mapped;
    // the decoder's columns never leave HBM
    // (PC_BAM_STAGE_HOST=1: read them back and hand them over as host arrays, as a caller of pc_bam_read + pc_add_alignment_file does)
    if (!knobs.stage_host) {
        pcstage::DevCols dc = {};   // (the wide records go up in stage_file, from the host arrays)
        dc.tid = b->tid.p; dc.pos = b->pos.p; dc.alen = b->alen.p; dc.flags = b->flags.p; dc.nblk = b->nblk.p;
        dc.blk_start = b->blk_start.p; dc.blk_len = b->blk_len.p;
        StageInput in;
        in.n = n; in.ntid = ntid; in.nrun = m; in.dev = &dc;
        in.n_wide = nw; in.wide_idx = b->wide_idx.data(); in.wide_alen = b->wide_alen.data(); in.wide_nblk = b->wide_nblk.data();
        rc = stage_file(e, in);
        if (rc != PC_OK) return rc;
        // the FLAG / MAPQ columns stay with the staged file (no copy: the decoder's blocks change hands)
        StagedFile *sf = e->files.back();
        sf->sam_flag.swap(b->flag16);
        sf->sam_mapq.swap(b->mapq);
        sf->have_sam = true;
        sf->sam_nh.swap(b->nh);
        sf->have_nh = true;
        return sync_flag_filter(e);
    }
    std::vector<int32_t> tid((size_t)n), pos((size_t)n), bs((size_t)m), bl((size_t)m), wa((size_t)nw), wn((size_t)nw);
    std::vector<uint16_t> alen((size_t)n);
    std::vector<uint8_t> flags((size_t)n), nblk((size_t)n);
    std::vector<int64_t> wi((size_t)nw);
    rc = pc_bam_read(b, tid.data(), pos.data(), alen.data(), flags.data(), nblk.data(), bs.data(), bl.data(), wi.data(), wa.data(), wn.data());
    if (rc != PC_OK) return rc;
    std::vector<uint16_t> f16((size_t)n);
    std::vector<uint8_t> mq((size_t)n);
    rc = pc_bam_read_sam(b, f16.data(), mq.data(), nullptr);
    if (rc != PC_OK) return rc;
    rc = pc_add_alignment_file_wide(e, n, ntid, tid.data(), pos.data(), alen.data(), flags.data(), nblk.data(), m, bs.data(), bl.data(),
                                    nw, wi.data(), wa.data(), wn.data());
    if (rc != PC_OK) return rc;
    rc = pc_set_alignment_sam(e, (int)e->files.size() - 1, n, f16.data(), mq.data());
    if (rc != PC_OK) return rc;
    std::vector<uint16_t> nhv((size_t)n);
    rc = pc_bam_read_nh(b, nhv.data());
    if (rc != PC_OK) return rc;
    return pc_set_alignment_nh(e, (int)e->files.size() - 1, n, nhv.data());
}

namespace {
// A file mapped for one call: every host thread touches its share of the pages (soft faults in parallel: 578 MB in ~2 ms
// instead of the 15 of MAP_POPULATE's one thread), and the mapping is taken down by a helper thread as soon as the
// image has been uploaded -- while the caller's thread waits for the GPU.
struct MappedFile {
    void *p = nullptr;
    size_t size = 0;
    // (a region read maps only, and faults what it uploads)
    // touch_mode 1: fault every page in up front (all host threads); 0: map only; -1 (whole-file reads): up front for a
    // file that is uploaded straight from the mapping (below two upload pieces: the runtime's one staging thread would take
    // the faults one by one), map only for a larger one -- its pieces are copied into the page-locked ring by all host
    // threads, which take the faults as they go, beside the GPU's work (the 2.9 GB file of 10^8 aligner-like records:
    // file -> staged 169 - 180 ms with the pages touched up front, 147 - 149 without; `forced` = 0 / 1, BamKnobs::touch, forces either)
    int open(const char *path, int touch_mode, int forced) {
        bool touch = touch_mode > 0;
        const int fd = ::open(path, O_RDONLY);
        if (fd < 0) return fail(PC_ERR_ARG, "cannot open %s: %s", path, strerror(errno));
        struct stat sb;
        if (fstat(fd, &sb) != 0) { ::close(fd); return fail(PC_ERR_ARG, "cannot stat %s: %s", path, strerror(errno)); }
        size = (size_t)sb.st_size;
        if (touch_mode < 0) touch = forced >= 0 ? forced != 0 : size < ((size_t)128 << 20);
        if (size) {
            p = mmap(nullptr, size, PROT_READ, MAP_SHARED, fd, 0);
            if (p == MAP_FAILED) { p = nullptr; ::close(fd); return fail(PC_ERR_NOMEM, "cannot map %s: %s", path, strerror(errno)); }
            if (touch) {
                (void)madvise(p, size, MADV_WILLNEED);
                const int64_t pages = (int64_t)((size + 4095) / 4096);
                const volatile uint8_t *q = (const volatile uint8_t *)p;
                parallel_chunks(pages, std::min(usable_cpus(), 32), [&](int, int64_t b, int64_t en) {
                    uint8_t acc = 0;
                    for (int64_t k = b; k < en; ++k) acc ^= q[(size_t)k * 4096];
                    (void)acc;
                });
            }
        }
        ::close(fd);
        return PC_OK;
    }
    // the mapping goes as soon as the image has crossed PCIe -- on a helper thread, while the caller's thread waits for
    // the GPU (munmap holds the address-space lock of the process: done later, it would stall the caller's next page faults)
    std::thread helper;
    void release_behind(hipStream_t up, int device) {
        if (!p || helper.joinable()) return;
        void *q = p;
        const size_t n = size;
        p = nullptr;
        try {
            helper = std::thread([q, n, up, device]() {
                if (hipSetDevice(device) == hipSuccess) (void)hipStreamSynchronize(up);
                (void)munmap(q, n);
            });
        } catch (...) { p = q; }
    }
    ~MappedFile() {
        if (helper.joinable()) helper.join();
        if (p) (void)munmap(p, size);
    }
};
} // namespace

// The path-taking entry points: map the file, then open it (`out`) or stage it (`mapped`).  A whole-file read faults the
// pages as MappedFile::open decides and takes the mapping down as soon as the image has been uploaded; a region read maps
// only, faults what it uploads, and keeps the mapping to the end (a retry for a longer header reads the file again).
static int with_mapped_file(pc_engine *e, const char *path, const BamSpan *span, pc_bam **out, int64_t *mapped, uint32_t flags = 0) {
    const BamKnobs knobs;
    MappedFile mf;
    const int rc = mf.open(path, span ? 0 : -1, knobs.touch);
    if (rc != PC_OK) return rc;
    const int device = e->device;
    const UploadedHook release = [&mf, device](hipStream_t up) { mf.release_behind(up, device); };
    const UploadedHook *hook = span ? nullptr : &release;
    // (the open entry points pass `out`, the staging ones leave it null and may pass `mapped`)
    return out ? bam_open_span_retry(e, mf.p, (int64_t)mf.size, path, out, hook, span, knobs, flags)
               : add_alignment_bam_impl(e, mf.p, (int64_t)mf.size, path, mapped, hook, span, knobs, flags);
}

static int chunk_args(const char *what, int nchunk, const uint64_t *voff_beg, const uint64_t *voff_end, int nreg, const int32_t *tid, const int64_t *beg,
                      const int64_t *end, BamSpan &sp) {
    if (nchunk < 0 || (nchunk > 0 && (!voff_beg || !voff_end))) return fail(PC_ERR_ARG, "%s: bad chunk list", what);
    for (int k = 0; k < nchunk; ++k)
        if (voff_end[k] <= voff_beg[k] || (k > 0 && voff_beg[k] < voff_end[k - 1]))
            return fail(PC_ERR_ARG, "%s: chunks must be non-empty, ascending and disjoint", what);
    if (nreg < 0 || (nreg > 0 && (!tid || !beg || !end))) return fail(PC_ERR_ARG, "%s: bad span / regions", what);
    for (int k = 0; k < nreg; ++k) {
        if (tid[k] < 0 || end[k] <= beg[k]) return fail(PC_ERR_ARG, "%s: region %d is empty or has no reference id", what, k);
        if (k > 0 && (tid[k] < tid[k - 1] || (tid[k] == tid[k - 1] && beg[k] < end[k - 1])))
            return fail(PC_ERR_ARG, "%s: regions must be ascending by (reference id, start) and must not overlap", what);
    }
    sp.nchunk = nchunk; sp.cbeg = voff_beg; sp.cend = voff_end; sp.nreg = nreg; sp.tid = tid; sp.beg = beg; sp.end = end;
    return PC_OK;
}

// a span is the chunk list of its one chunk (none when it is empty): the caller's two offsets, where they are for the length of the call
static int span_args(const char *what, const uint64_t *voff_begin, const uint64_t *voff_end, int nreg, const int32_t *tid, const int64_t *beg, const int64_t *end, BamSpan &sp) {
    if (*voff_end < *voff_begin) return fail(PC_ERR_ARG, "%s: bad span / regions", what);
    return chunk_args(what, *voff_end > *voff_begin ? 1 : 0, voff_begin, voff_end, nreg, tid, beg, end, sp);
}

extern "C" {

int pc_bam_close(pc_bam *b) {
    if (!b) return PC_OK;
    if (b->e) { (void)hipSetDevice(b->e->device); (void)hipStreamSynchronize(b->e->stream); }
    delete b;
    return PC_OK;
}

int pc_bam_open_flags(pc_engine *e, const void *image, int64_t size, const char *name, uint32_t flags, pc_bam **out) {
    return bam_open_impl(e, image, size, name, out, nullptr, nullptr, BamKnobs(), flags);
}
int pc_bam_open(pc_engine *e, const void *image, int64_t size, const char *name, pc_bam **out) { return pc_bam_open_flags(e, image, size, name, 0u, out); }

static int sort_flags_ok(const char *what, uint32_t flags) {
    return (flags & ~(uint32_t)PC_BAM_SORT) ? fail(PC_ERR_ARG, "%s: unknown flags (PC_BAM_SORT is the one there is)", what) : PC_OK;
}

int pc_add_alignment_bam_flags(pc_engine *e, const void *image, int64_t size, const char *name, uint32_t flags, int64_t *mapped) {
    const int rc = sort_flags_ok("pc_add_alignment_bam_flags", flags);
    return rc != PC_OK ? rc : add_alignment_bam_impl(e, image, size, name, mapped, nullptr, nullptr, BamKnobs(), flags);
}
int pc_add_alignment_bam(pc_engine *e, const void *image, int64_t size, const char *name, int64_t *mapped) {
    return pc_add_alignment_bam_flags(e, image, size, name, 0u, mapped);
}

int pc_bam_open_path_flags(pc_engine *e, const char *path, uint32_t flags, pc_bam **out) {
    if (!e || !path || !out) return fail(PC_ERR_ARG, "pc_bam_open_path: bad arguments");
    const int rc = sort_flags_ok("pc_bam_open_path_flags", flags);
    return rc != PC_OK ? rc : with_mapped_file(e, path, nullptr, out, nullptr, flags);
}
int pc_bam_open_path(pc_engine *e, const char *path, pc_bam **out) { return pc_bam_open_path_flags(e, path, 0u, out); }

int pc_add_alignment_bam_path_flags(pc_engine *e, const char *path, uint32_t flags, int64_t *mapped) {
    if (!e || !path) return fail(PC_ERR_ARG, "pc_add_alignment_bam_path: bad arguments");
    const int rc = sort_flags_ok("pc_add_alignment_bam_path_flags", flags);
    return rc != PC_OK ? rc : with_mapped_file(e, path, nullptr, nullptr, mapped, flags);
}
int pc_add_alignment_bam_path(pc_engine *e, const char *path, int64_t *mapped) { return pc_add_alignment_bam_path_flags(e, path, 0u, mapped); }

int pc_bam_sort_stats(pc_bam *b, int64_t *out4, double *ms) {
    if (!b || !out4) return fail(PC_ERR_ARG, "pc_bam_sort_stats: bad arguments");
    out4[0] = b->sort_requested ? 1 : 0; out4[1] = b->sorted_input ? 1 : 0; out4[2] = b->moved; out4[3] = b->key_bits;
    if (ms) *ms = b->sort_ms;
    return PC_OK;
}

int pc_bam_read_file_order(pc_bam *b, int64_t *rec_no) {
    if (!b) return fail(PC_ERR_ARG, "pc_bam_read_file_order: NULL handle");
    if (!b->moved) return fail(PC_ERR_STATE, "pc_bam_read_file_order: no record was moved (the records are in the order of the file)");
    if (b->n > 0 && !rec_no) return fail(PC_ERR_ARG, "pc_bam_read_file_order: NULL array");
    HIP_TRY(hipSetDevice(b->e->device));
    HIP_TRY(hipStreamSynchronize(b->e->stream));
    std::vector<uint32_t> fo((size_t)b->n);
    if (b->n) HIP_TRY(hipMemcpy(fo.data(), b->file_order.p, (size_t)b->n * 4, hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < b->n; ++k) rec_no[k] = (int64_t)fo[(size_t)k];
    return PC_OK;
}

int pc_bam_open_span(pc_engine *e, const char *path, uint64_t voff_begin, uint64_t voff_end, int nreg, const int32_t *tid, const int64_t *beg,
                     const int64_t *end, pc_bam **out) {
    if (!e || !path || !out) return fail(PC_ERR_ARG, "pc_bam_open_span: bad arguments");
    BamSpan sp;
    const int rc = span_args("pc_bam_open_span", &voff_begin, &voff_end, nreg, tid, beg, end, sp);
    return rc != PC_OK ? rc : with_mapped_file(e, path, &sp, out, nullptr);
}

int pc_add_alignment_bam_span(pc_engine *e, const char *path, uint64_t voff_begin, uint64_t voff_end, int nreg, const int32_t *tid,
                              const int64_t *beg, const int64_t *end, int64_t *mapped) {
    if (!e || !path) return fail(PC_ERR_ARG, "pc_add_alignment_bam_span: bad arguments");
    BamSpan sp;
    const int rc = span_args("pc_add_alignment_bam_span", &voff_begin, &voff_end, nreg, tid, beg, end, sp);
    return rc != PC_OK ? rc : with_mapped_file(e, path, &sp, nullptr, mapped);
}

int pc_bam_open_chunks(pc_engine *e, const char *path, int nchunk, const uint64_t *voff_beg, const uint64_t *voff_end, int nreg, const int32_t *tid,
                       const int64_t *beg, const int64_t *end, pc_bam **out) {
    if (!e || !path || !out) return fail(PC_ERR_ARG, "pc_bam_open_chunks: bad arguments");
    BamSpan sp;
    const int rc = chunk_args("pc_bam_open_chunks", nchunk, voff_beg, voff_end, nreg, tid, beg, end, sp);
    return rc != PC_OK ? rc : with_mapped_file(e, path, &sp, out, nullptr);
}

int pc_add_alignment_bam_chunks(pc_engine *e, const char *path, int nchunk, const uint64_t *voff_beg, const uint64_t *voff_end, int nreg,
                                const int32_t *tid, const int64_t *beg, const int64_t *end, int64_t *mapped) {
    if (!e || !path) return fail(PC_ERR_ARG, "pc_add_alignment_bam_chunks: bad arguments");
    BamSpan sp;
    const int rc = chunk_args("pc_add_alignment_bam_chunks", nchunk, voff_beg, voff_end, nreg, tid, beg, end, sp);
    return rc != PC_OK ? rc : with_mapped_file(e, path, &sp, nullptr, mapped);
}

int pc_bam_counts(pc_bam *b, int64_t *counts) {
    if (!b || !counts) return fail(PC_ERR_ARG, "pc_bam_counts: bad arguments");
    counts[0] = b->n; counts[1] = b->nrun; counts[2] = b->mapped; counts[3] = b->total; counts[4] = (int64_t)b->wide_idx.size();
    counts[5] = b->members; counts[6] = b->inflated_bytes; counts[7] = b->chain_restarts;
    return PC_OK;
}
int pc_bam_stats(pc_bam *b, int64_t *out4) {
    if (!b || !out4) return fail(PC_ERR_ARG, "pc_bam_stats: bad arguments");
    out4[0] = b->uploaded_bytes; out4[1] = b->runs; out4[2] = b->members; out4[3] = b->inflated_bytes;
    return PC_OK;
}
int pc_bam_timing(pc_bam *b, double *ms4) {
    if (!b || !ms4) return fail(PC_ERR_ARG, "pc_bam_timing: bad arguments");
    for (int k = 0; k < 4; ++k) ms4[k] = b->ms[k];
    return PC_OK;
}
int pc_bam_nref(pc_bam *b) { return b ? (int)b->ref_names.size() : -1; }
const char *pc_bam_ref_name(pc_bam *b, int i) { return (b && i >= 0 && i < (int)b->ref_names.size()) ? b->ref_names[(size_t)i].c_str() : nullptr; }
int32_t pc_bam_ref_length(pc_bam *b, int i) { return (b && i >= 0 && i < (int)b->ref_lengths.size()) ? b->ref_lengths[(size_t)i] : -1; }

int pc_bam_read(pc_bam *b, int32_t *tid, int32_t *pos, uint16_t *alen, uint8_t *flags, uint8_t *nblk, int32_t *blk_start, int32_t *blk_len,
                int64_t *wide_idx, int32_t *wide_alen, int32_t *wide_nblk) {
    if (!b) return fail(PC_ERR_ARG, "pc_bam_read: NULL handle");
    if (b->n > 0 && (!tid || !pos || !alen || !flags || !nblk)) return fail(PC_ERR_ARG, "pc_bam_read: NULL array");
    if (b->nrun > 0 && (!blk_start || !blk_len)) return fail(PC_ERR_ARG, "pc_bam_read: NULL run array");
    if (!b->wide_idx.empty() && (!wide_idx || !wide_alen || !wide_nblk)) return fail(PC_ERR_ARG, "pc_bam_read: NULL wide array");
    HIP_TRY(hipSetDevice(b->e->device));
    hipStream_t st = b->e->stream;
    BamClock rclk{getenv("PC_BAM_TIMING") != nullptr};
    const size_t n = (size_t)b->n, m = (size_t)b->nrun;
    // (through the ring of page-locked pieces when the columns are large: the caller's arrays are pageable, see TransferRing)
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<TransferJob> jobs;
    if (n) {
        jobs.push_back({tid, b->tid.p, n * 4});
        jobs.push_back({pos, b->pos.p, n * 4});
        jobs.push_back({alen, b->alen.p, n * 2});
        jobs.push_back({flags, b->flags.p, n});
        jobs.push_back({nblk, b->nblk.p, n});
    }
    if (m) {
        jobs.push_back({blk_start, b->blk_start.p, m * 4});
        jobs.push_back({blk_len, b->blk_len.p, m * 4});
    }
    {
        const int rc = TransferRing::of(b->e->device).run(b->e->device, jobs, TransferRing::kPiece, false, true);
        if (rc != PC_OK) return rc;
    }
    rclk.lap("columns to the host");
    for (size_t k = 0; k < b->wide_idx.size(); ++k) { wide_idx[k] = b->wide_idx[k]; wide_alen[k] = b->wide_alen[k]; wide_nblk[k] = b->wide_nblk[k]; }
    return PC_OK;
}

int pc_bam_read_sam(pc_bam *b, uint16_t *flag, uint8_t *mapq, int32_t *lseq) {
    if (!b) return fail(PC_ERR_ARG, "pc_bam_read_sam: NULL handle");
    HIP_TRY(hipSetDevice(b->e->device));
    hipStream_t st = b->e->stream;
    const size_t n = (size_t)b->n;
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<TransferJob> jobs;
    if (n && flag) jobs.push_back({flag, b->flag16.p, n * 2});
    if (n && mapq) jobs.push_back({mapq, b->mapq.p, n});
    if (n && lseq) jobs.push_back({lseq, b->lseq.p, n * 4});
    return TransferRing::of(b->e->device).run(b->e->device, jobs, TransferRing::kPiece, false, true);
}

int pc_bam_read_nh(pc_bam *b, uint16_t *nh) {
    if (!b) return fail(PC_ERR_ARG, "pc_bam_read_nh: NULL handle");
    HIP_TRY(hipSetDevice(b->e->device));
    HIP_TRY(hipStreamSynchronize(b->e->stream));
    std::vector<TransferJob> jobs;
    if (b->n && nh) jobs.push_back({nh, b->nh.p, (size_t)b->n * 2});
    return TransferRing::of(b->e->device).run(b->e->device, jobs, TransferRing::kPiece, false, true);
}

int pc_bam_index_build(pc_engine *e, const char *path, pc_bam_index **out) {
    if (!e || !path || !out) return fail(PC_ERR_ARG, "pc_bam_index_build: bad arguments");
    const BamKnobs knobs;
    MappedFile mf;
    const int rc = mf.open(path, -1, knobs.touch);
    if (rc != PC_OK) return rc;
    const int device = e->device;
    const UploadedHook release = [&mf, device](hipStream_t up) { mf.release_behind(up, device); };
    return bam_index_impl(e, mf.p, (int64_t)mf.size, path, out, &release, knobs);
}

int pc_bam_index_build_csi(pc_engine *e, const char *path, int min_shift, pc_bam_index **out) {
    if (!e || !path || !out) return fail(PC_ERR_ARG, "pc_bam_index_build_csi: bad arguments");
    *out = nullptr;
    if (min_shift < pcidx::kMinShiftLo || min_shift > pcidx::kMinShiftHi)
        return fail(PC_ERR_ARG, "pc_bam_index_build_csi: min_shift %d is not in %d .. %d", min_shift, pcidx::kMinShiftLo, pcidx::kMinShiftHi);
    const BamKnobs knobs;
    MappedFile mf;
    const int rc = mf.open(path, -1, knobs.touch);
    if (rc != PC_OK) return rc;
    const int device = e->device;
    const UploadedHook release = [&mf, device](hipStream_t up) { mf.release_behind(up, device); };
    return bam_index_impl(e, mf.p, (int64_t)mf.size, path, out, &release, knobs, min_shift);
}

int pc_bam_index_finish_csi(int min_shift, int n_lvls, int n_ref, int64_t n_runs, const int32_t *run_tid, const uint32_t *run_bin, const uint64_t *run_beg,
                            const uint64_t *run_end, const uint64_t *run_loff, const uint64_t *ref_beg, const uint64_t *ref_end, const int64_t *ref_mapped,
                            const int64_t *ref_unmapped, int64_t n_no_coor, pc_bam_index **out) {
    if (!out) return fail(PC_ERR_ARG, "pc_bam_index_finish_csi: bad arguments");
    *out = nullptr;
    pc_bam_index *idx = new pc_bam_index();
    const auto t0 = std::chrono::steady_clock::now();
    const char *msg = pcidxhost::finish_csi(min_shift, n_lvls, n_ref, n_runs, run_tid, run_bin, run_beg, run_end, run_loff, ref_beg, ref_end, ref_mapped,
                                            ref_unmapped, n_no_coor, *idx);
    if (msg) { delete idx; return fail(PC_ERR_ARG, "%s", msg); }
    idx->ms[6] = idx->ms[7] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = idx;
    return PC_OK;
}

int pc_bam_index_finish(int n_ref, int64_t n_runs, const int32_t *run_tid, const uint32_t *run_bin, const uint64_t *run_beg, const uint64_t *run_end,
                        const int64_t *lin_start, const uint64_t *linear, const uint64_t *ref_beg, const uint64_t *ref_end, const int64_t *ref_mapped,
                        const int64_t *ref_unmapped, int64_t n_no_coor, pc_bam_index **out) {
    if (!out) return fail(PC_ERR_ARG, "pc_bam_index_finish: bad arguments");
    *out = nullptr;
    pc_bam_index *idx = new pc_bam_index();
    const auto t0 = std::chrono::steady_clock::now();
    const char *msg = pcidxhost::finish(n_ref, n_runs, run_tid, run_bin, run_beg, run_end, lin_start, linear, ref_beg, ref_end, ref_mapped, ref_unmapped, n_no_coor, *idx);
    if (msg) { delete idx; return fail(PC_ERR_ARG, "%s", msg); }
    idx->ms[6] = idx->ms[7] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = idx;
    return PC_OK;
}

int pc_bam_index_bytes(pc_bam_index *idx, void *buf, int64_t cap, int64_t *bytes) {
    if (!idx || !bytes || cap < 0 || (cap > 0 && !buf)) return fail(PC_ERR_ARG, "pc_bam_index_bytes: bad arguments");
    *bytes = (int64_t)idx->bytes.size();
    if (cap >= *bytes && *bytes) std::memcpy(buf, idx->bytes.data(), idx->bytes.size());   // (a smaller buffer: the caller comes back with *bytes)
    return PC_OK;
}

int pc_bam_index_stats(pc_bam_index *idx, int64_t *out8) {
    if (!idx || !out8) return fail(PC_ERR_ARG, "pc_bam_index_stats: bad arguments");
    for (int k = 0; k < 8; ++k) out8[k] = idx->stats[k];
    return PC_OK;
}

int pc_bam_index_timing(pc_bam_index *idx, double *ms8) {
    if (!idx || !ms8) return fail(PC_ERR_ARG, "pc_bam_index_timing: bad arguments");
    for (int k = 0; k < 8; ++k) ms8[k] = idx->ms[k];
    return PC_OK;
}

int pc_bam_index_close(pc_bam_index *idx) {
    delete idx;
    return PC_OK;
}

} // extern "C"
