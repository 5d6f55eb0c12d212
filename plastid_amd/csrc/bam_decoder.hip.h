// Compressed BAM on the GPU, host side: the entry points of include/plastid_counts.h that decode a BAM file with the
// kernels of bam_kernels.hip.h.  One open is five phases (bam_open_impl): plan_members (bam_host.h), upload_and_inflate,
// read_header, chain_records, decode_columns.  The index build (bam_index_impl: BAI or CSI) runs the first four and
// index_records in place of the fifth.  Every phase is a list of steps: HIP calls, and the host arithmetic of bam_host.h
// (plain C++, tested on the CPU by tests/bam_host_test.cpp).  Part of the one translation unit of plastid_counts.hip;
// the plumbing -- buffers, room, DrainOnExit, the hipcub seam -- is device_util.hip.h.
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

namespace bh = pcbamhost;
using bh::BamHeader;
using bh::BamPlan;
using bh::BamSpan;

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
constexpr int PC_RETRY_HEADER = -1000;   // (internal) the header did not fit the leading members that were inflated

// a defect of bam_host.h (a member header's, or a chunk list that is not this file's) as this library's error
int host_defect(int code, const char *path) {
    if (bh::chunk_defect(code)) return fail(PC_ERR_ARG, "the index does not belong to this BAM file (%s): %s", bh::defect_text(code), path);
    return fail(PC_ERR_ARG, "%s%s", bh::defect_text(code), code == bh::kMemberTiny ? path : "");
}

// What the phases of one open share (phase 1, bh::plan_members, is host only; phases 2 - 5 queue on `st`, and each leaves
// it drained of everything that reads a buffer it owns).
struct BamDecode {
    pc_engine *e;
    hipStream_t st;
    std::string path;
    BamKnobs knobs;
    BamClock clk{knobs.timing};
    LapEvents<5> ev;                   // allocations done | tables queued | inflated | records chained | columns written
    DevBuf<uint8_t> d_stream;          // the inflated stream (+ 64 zero bytes)
    DevBuf<pcbam::Member> d_members;
    DevBuf<pcbam::MemberChain> d_chain;   // every member's walk over its records' length prefixes, and the record offsets it found
    DevBuf<uint32_t> d_rec_off;
};

// ---- phase 2: upload + inflate, piece by piece (bh::cut_pieces): the file image crosses PCIe on the side stream in
// pieces of whole members while the members of the pieces before are inflated on the main one (one wave per member).
// (Every launch ends in a tail of half-empty CUs -- a member takes ~4 ms and ~3 000 are in flight -- so the pieces are
// large: 20 M aligner-like records, 578 MB: one piece 87 ms, 48 MiB pieces 67 ms, 128 MiB 58 ms, 256 MiB 61 ms.)
// What its steps share:
struct Upload {
    DevBuf<uint8_t> d_image;
    DevBuf<uint32_t> d_status, d_crc;
    // (pieces of the image gathered from several runs, for an upload straight from pageable memory: they outlive the drain)
    std::vector<std::vector<uint8_t>> gathered;
    hipStream_t up = nullptr;          // the stream the image is uploaded on: the side stream, or the main one
    int naux = 0;                      // auxiliary streams the inflate launches take turns on, beside the main one
    bool ring = false, ring_busy[2] = {false, false};
    int ring_threads = 1;
    std::vector<hipEvent_t> landed;    // [0]: what the main stream had queued when the side stream started; then one per piece
    ~Upload() { for (auto x : landed) (void)hipEventDestroy(x); }
    int mark(hipStream_t on) {         // one more event, recorded on `on`
        hipEvent_t x;
        HIP_TRY(hipEventCreateWithFlags(&x, hipEventDisableTiming));
        landed.push_back(x);
        HIP_TRY(hipEventRecord(x, on));
        return PC_OK;
    }
};
// An early return between the first queued copy and the synchronisation behind the inflate launches must not hand the
// image, the stream buffer or the page-locked ring back (nor let the caller unmap the file) while the side / auxiliary
// streams still use them: drain every stream the decoder queues on before the buffers of Upload go out of scope.
struct Drain {
    pc_engine *e; bool armed;
    ~Drain() {
        if (!armed) return;
        if (e->side_stream) (void)hipStreamSynchronize(e->side_stream);
        for (int k = 0; k < pc_engine::kAux; ++k) if (e->aux_stream[k]) (void)hipStreamSynchronize(e->aux_stream[k]);
        (void)hipStreamSynchronize(e->stream);
    }
};

// Step 1: the buffers, and the tables of the kernels (members, CRC) on their way.
int reserve_and_queue_tables(BamDecode &d, const BamPlan &pl, Upload &u) {
    hipStream_t st = d.st;
    const int nm = pl.nm();
    int rc = PC_OK;
    room(rc, u.d_image, (size_t)std::max<int64_t>(pl.image_bytes, 16) + 16); room(rc, d.d_stream, (size_t)pl.total_u + 64);
    room(rc, d.d_members, (size_t)std::max(nm, 1)); room(rc, u.d_status, (size_t)std::max(nm, 1)); room(rc, u.d_crc, 5 * 256);
    if (rc != PC_OK) return rc;
    d.clk.lap("allocations (image, stream)");
    HIP_TRY(hipEventRecord(d.ev[0], st));
    if (nm) HIP_TRY(hipMemcpyAsync(d.d_members.p, pl.members.data(), (size_t)nm * sizeof(pcbam::Member), hipMemcpyHostToDevice, st));
    const CrcTables &ct = crc_tables();
    HIP_TRY(hipMemcpyAsync(u.d_crc.p, ct.tab, sizeof(ct.tab), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(u.d_crc.p + 256, ct.shift, sizeof(ct.shift), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d.d_stream.p + pl.total_u, 0, 64, st));
    HIP_TRY(hipEventRecord(d.ev[1], st));
    return PC_OK;
}

// Step 2: the streams of the upload and of the inflate launches behind the main one, and the page-locked ring.
int start_streams(BamDecode &d, const BamPlan &pl, Upload &u) {
    pc_engine *e = d.e;
    hipStream_t st = d.st;
    u.up = e->side_stream ? e->side_stream : st;
    if (u.up != st) {   // the side stream starts behind what the main one has queued so far (the buffers' previous users)
        PC_TRY(u.mark(st));
        HIP_TRY(hipStreamWaitEvent(u.up, u.landed[0], 0));
    }
    // The inflate launches alternate between the main stream and an auxiliary one: a launch ends in a tail of
    // half-empty CUs (a member takes ~4 ms, ~3 000 are in flight), which the launch of the next piece fills.
    // (two streams in turn: measured on two boxes, 64 MiB pieces, 20 M aligner-like records: one stream 56 - 58 ms, two
    // 46.6 - 53.5, four 48.6; PC_BAM_STREAMS = 1 .. 4 for experiments)
    u.naux = u.up != st ? std::max(0, std::min(pc_engine::kAux, d.knobs.streams - 1)) : 0;
    for (int k = 0; k < u.naux; ++k)   // (behind what the main stream has queued: the members table, the previous users of the buffers)
        HIP_TRY(hipStreamWaitEvent(e->aux_stream[k], u.landed[0], 0));
    // large files cross PCIe through two page-locked halves of one piece each (made once per engine)
    const int64_t piece_bytes = d.knobs.piece_bytes;
    u.ring = u.up != st && pl.image_bytes >= 2 * piece_bytes && !d.knobs.no_ring;
    u.ring_threads = std::max(1, std::min(usable_cpus(), 16));
    if (u.ring) {
        // (a piece ends with a whole member: up to 64 KiB beyond piece_bytes)
        for (int k = 0; k < 2 && u.ring; ++k) {
            if (e->bam_ring[k].reserve((size_t)piece_bytes + ((size_t)1 << 17)) != PC_OK) u.ring = false;
            if (u.ring && !e->ev_ring[k] && hipEventCreateWithFlags(&e->ev_ring[k], hipEventDisableTiming) != hipSuccess) u.ring = false;
        }
        (void)hipGetLastError();
    }
    return PC_OK;
}

// Step 3: one piece of the image on its way to the device, by one of three ways.
int upload_piece(BamDecode &d, const uint8_t *image, const BamPlan &pl, const bh::ImagePiece &pc, int piece_no, Upload &u) {
    pc_engine *e = d.e;
    const uint8_t *src = bh::piece_source(image, pl, pc);   // (one_run only)
    uint8_t *dst = u.d_image.p + pc.byte0;
    const int64_t len = pc.byte1 - pc.byte0;
    if (u.ring) {
        // through a page-locked half: the runtime's own staging of a pageable copy runs on one thread (12 - 20 GB/s);
        // here every host thread copies its share, and the DMA of one half overlaps the filling of the other
        const int slot = piece_no & 1;
        if (u.ring_busy[slot]) HIP_TRY(hipEventSynchronize(e->ev_ring[slot]));
        uint8_t *half = e->bam_ring[slot].p;
        const int64_t blk = (int64_t)1 << 20;
        parallel_chunks((len + blk - 1) / blk, u.ring_threads, [&](int, int64_t b, int64_t en) {
            const int64_t lo = b * blk, hi = std::min(len, en * blk);
            if (hi > lo && pc.one_run) std::memcpy(half + lo, src + lo, (size_t)(hi - lo));
            else if (hi > lo) bh::copy_image(image, pl.runs, half + lo, pc.byte0 + lo, pc.byte0 + hi);
        });
        HIP_TRY(hipMemcpyAsync(dst, half, (size_t)len, hipMemcpyHostToDevice, u.up));
        HIP_TRY(hipEventRecord(e->ev_ring[slot], u.up));
        u.ring_busy[slot] = true;
    } else if (pc.one_run)
        HIP_TRY(hipMemcpyAsync(dst, src, (size_t)len, hipMemcpyHostToDevice, u.up));
    else {   // several runs in one piece: gathered, one copy
        u.gathered.emplace_back((size_t)len);
        bh::copy_image(image, pl.runs, u.gathered.back().data(), pc.byte0, pc.byte1);
        HIP_TRY(hipMemcpyAsync(dst, u.gathered.back().data(), (size_t)len, hipMemcpyHostToDevice, u.up));
    }
    return PC_OK;
}

// Step 4: the piece's members inflated and their CRCs checked, behind its upload, on the stream whose turn it is.
int inflate_piece(BamDecode &d, const bh::ImagePiece &pc, int piece_no, Upload &u) {
    using namespace pcbam;
    hipStream_t st = d.st;
    if (u.up != st) PC_TRY(u.mark(u.up));
    hipStream_t ks = (piece_no % (u.naux + 1)) ? d.e->aux_stream[piece_no % (u.naux + 1) - 1] : st;
    if (u.up != st) HIP_TRY(hipStreamWaitEvent(ks, u.landed.back(), 0));
    const dim3 grid((unsigned)(pc.m1 - pc.m0));
    if (d.knobs.serial_symbols) hipLaunchKernelGGL(k_bgzf_inflate<false>, grid, dim3(kInflWG), 0, ks, u.d_image.p, d.d_members.p, pc.m0, pc.m1, d.d_stream.p, u.d_status.p);
    else hipLaunchKernelGGL(k_bgzf_inflate<true>, grid, dim3(kInflWG), 0, ks, u.d_image.p, d.d_members.p, pc.m0, pc.m1, d.d_stream.p, u.d_status.p);
    // (the piece's CRC check right behind it, on the same stream: it runs while other pieces are still inflated)
    hipLaunchKernelGGL(k_bgzf_crc, grid, dim3(64), 0, ks, d.d_stream.p, d.d_members.p, pc.m0, pc.m1, u.d_crc.p, u.d_crc.p + 256, u.d_status.p);
    return PC_OK;
}

// Step 5: every member's status, as the kernels left it.
int check_status(BamDecode &d, const BamPlan &pl, const std::vector<uint32_t> &status) {
    const int nm = pl.nm();
    for (int m = 0; m < nm; ++m)
        if (status[(size_t)m]) {
            const pcbam::Member &mb = pl.members[(size_t)m];
            if (d.knobs.debug) fprintf(stderr, "[bam] member %d of %d (%u compressed -> %u bytes at %llu): inflate status %u\n", m, nm,
                                       mb.clen, mb.ulen, (unsigned long long)mb.uoff, status[(size_t)m]);
            return fail(PC_ERR_ARG, "%s%s", status[(size_t)m] == (uint32_t)pcbam::kInfCrc ? bh::kCrcMismatchIn : bh::kInflateFailedIn, d.path.c_str());
        }
    return PC_OK;
}

// Phase 2: the image goes to HBM and is inflated there, piece by piece; returns with every stream drained, every member's
// status and CRC checked, and the image given back.
int upload_and_inflate(BamDecode &d, const uint8_t *image, const BamPlan &pl, const UploadedHook *uploaded) {
    pc_engine *e = d.e;
    hipStream_t st = d.st;
    const int nm = pl.nm();
    Upload u;
    Drain drain{e, true};
    PC_TRY(reserve_and_queue_tables(d, pl, u));
    std::vector<uint32_t> status((size_t)nm, 0u);
    if (nm) {
        PC_TRY(start_streams(d, pl, u));
        int piece_no = 0;
        for (const bh::ImagePiece &pc : bh::cut_pieces(pl, d.knobs.piece_bytes)) {
            PC_TRY(upload_piece(d, image, pl, pc, piece_no, u));
            PC_TRY(inflate_piece(d, pc, piece_no, u));
            ++piece_no;
        }
        d.clk.note("every piece copied into the page-locked ring and queued");
        for (int k = 0; k < u.naux; ++k) {   // the main stream goes on behind all of them
            PC_TRY(u.mark(e->aux_stream[k]));
            HIP_TRY(hipStreamWaitEvent(st, u.landed.back(), 0));
        }
        if (uploaded) (*uploaded)(u.up);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(status.data(), u.d_status.p, (size_t)nm * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipEventRecord(d.ev[2], st));
    HIP_TRY(hipStreamSynchronize(st));
    drain.armed = false;   // (the main stream went on behind the side and auxiliary ones: all of them have drained)
    d.clk.lap("upload + inflate + crc (sync)");
    PC_TRY(check_status(d, pl, status));
    u.d_image.release();
    d.clk.lap("status check + image release");
    return PC_OK;
}

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
        const bh::HeaderParse hp = bh::parse_bam_header(head.data(), want, h);
        if (hp.status == bh::kHeaderOk) return PC_OK;
        if (hp.status == bh::kHeaderMore && want < header_limit) { want = std::min<size_t>(header_limit, want * 4); continue; }
        if (hp.status == bh::kHeaderMore && span && header_limit < (size_t)pl.total_u + 1 && span->header_bytes < size) return PC_RETRY_HEADER;
        return fail(PC_ERR_ARG, "%s", hp.text);
    }
}

struct BamRecords {
    std::vector<uint64_t> rec_base;   // records before each member (nm + 1 entries)
    int64_t nrec = 0;
    bool truncated = false;           // the last record runs past the end of the stream (reported after every other defect)
    int chain_restarts = 0;
};

// Phase 4: record starts.  Every member guesses its first record start and walks the chain of length prefixes; the host
// confirms that the walks chain (bh::settle_round), and restarts the members whose guess did not.  A whole-file read chains
// from the header's end to the end of the stream; a region read chains every run from its first chunk's start to its last
// chunk's end (bh::run_bounds), which the index gives and the chain has to hit exactly.
int chain_records(BamDecode &d, const BamPlan &pl, const BamSpan *span, const BamHeader &h, BamRecords &out) {
    using namespace pcbam;
    hipStream_t st = d.st;
    const int nm = pl.nm();
    DevBuf<uint64_t> d_forced, d_run_bounds;
    DevBuf<uint32_t> d_member_run;
    int rc = PC_OK;
    room(rc, d.d_chain, (size_t)std::max(nm, 1)); room(rc, d.d_rec_off, (size_t)std::max(nm, 1) * kMaxRecPerMember); room(rc, d_forced, (size_t)std::max(nm, 1));
    if (rc != PC_OK) return rc;
    std::vector<uint64_t> bounds;   // region read: {start, stop} of every run's record chain
    if (span) {
        const int defect = bh::run_bounds(pl, h.first_record, bounds);
        if (defect) return host_defect(defect, d.path.c_str());
        rc = d_run_bounds.upload(bounds, st);
        if (rc == PC_OK) rc = d_member_run.upload(pl.member_run, st);
        if (rc != PC_OK) return rc;
    }
    std::vector<MemberChain> chain((size_t)nm);
    std::vector<uint64_t> forced((size_t)nm, ~0ull);
    DrainOnExit drained{st};   // (the tables above and the two vectors are read and written by what is queued below)
    bh::ChainState state(pl, span ? &bounds : nullptr, h.first_record);
    if (nm) {
        HIP_TRY(hipMemsetAsync(d_forced.p, 0xff, (size_t)nm * 8, st));
        int from = 0;
        for (int round = 0;; ++round) {
            // (a whole-file read: one chain, no run tables -- both pointers are null)
            hipLaunchKernelGGL(span ? k_bam_chain<true> : k_bam_chain<false>, dim3((unsigned)(nm - from)), dim3(64), 0, st, d.d_stream.p, pl.total_u, d.d_members.p, nm, from,
                               h.n_ref, h.first_record, d_forced.p, d.d_chain.p, d.d_rec_off.p, pl.total_u, (const uint32_t *)d_member_run.p, (const uint64_t *)d_run_bounds.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(chain.data() + from, d.d_chain.p + from, (size_t)(nm - from) * sizeof(MemberChain), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const bh::Settle s = bh::settle_round(pl, span ? &bounds : nullptr, chain.data(), from, state);
            if (s.kind == bh::kInsideRecord) return host_defect(bh::kChunkInRecord, d.path.c_str());
            if (s.kind == bh::kTruncated) out.truncated = true;
            if (s.kind != bh::kRedo) break;
            out.chain_restarts += 1;
            forced[(size_t)s.m] = s.forced;
            HIP_TRY(hipMemcpyAsync(d_forced.p + s.m, &forced[(size_t)s.m], 8, hipMemcpyHostToDevice, st));
            from = s.m;
            if (round > nm + 8) return fail(PC_ERR_STATE, "pc_bam_open: the record chain of %s did not settle", d.path.c_str());
        }
    } else if (pl.total_u != h.first_record && !span) out.truncated = true;
    out.rec_base = bh::record_bases(state.nrec_of);
    out.nrec = (int64_t)out.rec_base[(size_t)nm];
    drained.armed = false;   // (every round ends in a synchronisation)
    HIP_TRY(hipEventRecord(d.ev[3], st));
    d.clk.lap("header + record chain");
    return PC_OK;
}

// The first defect the record decode found (k_bam_order's lowest record index: `first_err` = index << 8 | code, ~0: none),
// as the error the host reader gives for it; kRecTruncated / kRecBadSize and a chain that ended short (`truncated`) are
// reported after every other defect.
int record_defect(unsigned long long first_err, bool truncated, const char *path) {
    using namespace pcbam;
    if (first_err != ~0ull) switch ((int)(first_err & 0xffu)) {
    case kRecTidRange: return fail(PC_ERR_ARG, "BAM record with reference id out of range");
    case kRecNegPos: return fail(PC_ERR_ARG, "placed BAM record with a negative position");
    case kRecUnsorted: return fail(PC_ERR_UNSORTED, "BAM file is not coordinate sorted: %s", path);
    case kRecCigarOverrun: return fail(PC_ERR_ARG, "corrupt BAM record (cigar overruns block)");
    case kRecUnknownOp: return fail(PC_ERR_ARG, "unknown CIGAR operation in %s", path);
    case kRecEndBeyond: return fail(PC_ERR_ARG, "alignment ends beyond 2^31 - 1");
    case kRecTooLong: return fail(PC_ERR_ARG, "alignment with more than 2^31 - 1 aligned positions");
    case kRecDeletionOrder: return fail(PC_ERR_ARG, "alignment starting with a deletion breaks coordinate order; not supported");
    default: truncated = true;
    }
    return truncated ? fail(PC_ERR_ARG, "truncated BAM record") : PC_OK;
}

// the events around the sort phase of an open with PC_BAM_SORT: key kernel [0, 1]; sort, ranks and run offsets [2, 3]
typedef LapEvents<4> SortEvents;

// ---- the common head of phase 5 (decode_columns, index_records): the record table on the device and every record's fields
struct RecordTable {
    std::vector<uint32_t> rec_member;    // (host copy of d_rec_member: alive while its upload is)
    DevBuf<uint64_t> d_rec_base;
    DevBuf<uint32_t> d_rec_member, d_placed;
    DevBuf<pcbam::RecOut> d_recs;
    DevBuf<unsigned long long> d_misc;   // [0] first error (index << 8 | code); the rest is the phase's own
    unsigned g256 = 0;                   // blocks of 256 threads over the records
    // PC_BAM_SORT: the sort keys, and whether they found the file out of order
    DevBuf<uint64_t> d_key;
    DevBuf<uint32_t> d_idx;
    SortEvents sev;
    bool disorder = false;
};
int check_order(BamDecode &d, int64_t nrec, bool sort, RecordTable &t);
// k_bam_fields, then the order checks -- or, with `sort`, the keys first: a file they find in order goes on exactly as
// without the flag.  `n_misc` counters ([0] = ~0, the others 0) and `n_placed` entries of d_placed are the caller's to use.
int decode_fields(BamDecode &d, const BamPlan &pl, const BamHeader &h, const BamRecords &recs, size_t n_misc, size_t n_placed, bool sort, RecordTable &t) {
    using namespace pcbam;
    hipStream_t st = d.st;
    const int64_t nrec = recs.nrec;
    static const unsigned long long misc0[6] = {~0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    PC_TRY(t.d_misc.reserve(n_misc));
    HIP_TRY(hipMemcpyAsync(t.d_misc.p, misc0, n_misc * 8, hipMemcpyHostToDevice, st));
    if (nrec <= 0) return PC_OK;
    t.rec_member = bh::group_members(recs.rec_base, nrec, pl.nm());
    int rc = t.d_rec_base.upload(recs.rec_base, st);
    if (rc == PC_OK) rc = t.d_rec_member.upload(t.rec_member, st);
    room(rc, t.d_recs, (size_t)nrec); room(rc, t.d_placed, n_placed);
    if (sort) { room(rc, t.d_key, (size_t)nrec); room(rc, t.d_idx, (size_t)nrec); }
    if (rc == PC_OK && sort) rc = t.sev.create();
    if (rc != PC_OK) return rc;
    t.g256 = (unsigned)((nrec + 255) / 256);
    hipLaunchKernelGGL(k_bam_fields, dim3(t.g256), dim3(256), 0, st, d.d_stream.p, pl.total_u, d.d_members.p, t.d_rec_base.p, d.d_chain.p, d.d_rec_off.p, pl.nm(), nrec,
                       h.n_ref, t.d_rec_member.p, t.d_recs.p);
    return check_order(d, nrec, sort, t);
}
// Behind the fields kernel of either format (k_bam_fields, k_sam_fields), on the table it filled:
int check_order(BamDecode &d, int64_t nrec, bool sort, RecordTable &t) {
    using namespace pcbam;
    hipStream_t st = d.st;
    if (sort) {
        unsigned long long dis = 0;
        HIP_TRY(hipEventRecord(t.sev.ev[0], st));
        hipLaunchKernelGGL(k_bam_sort_keys, dim3(t.g256), dim3(256), 0, st, t.d_recs.p, nrec, t.d_key.p, t.d_idx.p, t.d_misc.p + 3);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(t.sev.ev[1], st));
        HIP_TRY(hipMemcpyAsync(&dis, t.d_misc.p + 3, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        t.disorder = dis != 0;
        if (!t.disorder) { t.d_key.release(); t.d_idx.release(); }
    }
    if (!t.disorder) hipLaunchKernelGGL(k_bam_order, dim3(t.g256), dim3(256), 0, st, t.d_recs.p, nrec, t.d_placed.p, t.d_misc.p);
    HIP_TRY(hipGetLastError());
    return PC_OK;
}

// ---- phase 5 of an open.  What its steps share beside the record table:
struct ColumnWork {
    RecordTable t;
    DevBuf<int32_t> d_rtid;              // region read: the regions' reference ids, starts and ends
    DevBuf<int64_t> d_rbe;
    DevBuf<uint32_t> d_runs, d_staged_at, d_run_at, d_wide;   // per record: its runs, where it is staged and where its runs go; per staged record: wide or not
    int64_t n_staged = 0, n_runs = 0;
    unsigned long long first_err = ~0ull;   // what place_records brought down (the SAM decoder words its own codes itself)
};

// Step 1 (region reads): keep what overlaps a requested region (htslib's overlap rule); everything else is as if it were not in the file.
int filter_regions(BamDecode &d, const BamSpan &span, int64_t nrec, ColumnWork &w) {
    hipStream_t st = d.st;
    const size_t nr = (size_t)std::max(span.nreg, 0);
    int rc = w.d_rtid.upload(span.tid, nr, st);
    room(rc, w.d_rbe, 2 * std::max<size_t>(nr, 1));
    if (rc != PC_OK) return rc;
    if (nr) {
        HIP_TRY(hipMemcpyAsync(w.d_rbe.p, span.beg, nr * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(w.d_rbe.p + nr, span.end, nr * 8, hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(pcbam::k_bam_region_filter, dim3(w.t.g256), dim3(256), 0, st, w.t.d_recs.p, nrec, (int)nr, w.d_rtid.p, w.d_rbe.p, w.d_rbe.p + nr);
    return PC_OK;
}

// Step 2: where every kept record and its runs go -- two exclusive sums; out of order: one stable radix sort of (key,
// record number) over the key bits in use, then staged_at and run_at by rank in the sorted order (the totals stay those
// of the two sums; placed records sort first).  The totals, the counts of `b` and the first defect come down.
int place_records(BamDecode &d, const BamHeader &h, const BamRecords &recs, bool sort, ColumnWork &w, pc_bam &b) {
    using namespace pcbam;
    hipStream_t st = d.st;
    RecordTable &t = w.t;
    const int64_t nrec = recs.nrec;
    uint32_t tot[2] = {0, 0};
    unsigned long long misc[5] = {0, 0, 0, 0, 0};
    DevBuf<uint8_t> d_tmp, d_sort_tmp;
    DevBuf<uint64_t> d_key2;
    DevBuf<uint32_t> d_idx2, d_runs_sorted;
    DrainOnExit drained{st};
    HIP_TRY(hipMemsetAsync(t.d_placed.p + nrec, 0, 4, st));
    HIP_TRY(hipMemsetAsync(w.d_runs.p + nrec, 0, 4, st));
    hipLaunchKernelGGL(k_bam_scan_inputs, dim3((unsigned)((nrec + 256 * kScanInputsPerThread - 1) / (256 * kScanInputsPerThread))), dim3(256), 0, st, t.d_recs.p, nrec, t.d_placed.p, w.d_runs.p, t.d_misc.p + 1);
    auto sum = [=](uint32_t *from, uint32_t *to) { return [=](void *tmp, size_t &bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, from, to, (int)(nrec + 1), st); }; };
    size_t most = 16, tmp_bytes = 0;
    PC_TRY(cub_need(most, tmp_bytes, sum(t.d_placed.p, w.d_staged_at.p)));
    PC_TRY(d_tmp.reserve(most));
    PC_TRY(cub_run_sized(d_tmp, tmp_bytes, sum(t.d_placed.p, w.d_staged_at.p)));
    PC_TRY(cub_run_sized(d_tmp, tmp_bytes, sum(w.d_runs.p, w.d_run_at.p)));
    if (t.disorder) {
        const int key_bits = sort_key_bits(h.n_ref);
        int rc = PC_OK;
        room(rc, d_key2, (size_t)nrec); room(rc, d_idx2, (size_t)nrec); room(rc, d_runs_sorted, (size_t)nrec + 1);
        if (rc != PC_OK) return rc;
        HIP_TRY(hipEventRecord(t.sev.ev[2], st));
        // (double buffers: the passes go back and forth between the two halves, and the sort says which half holds the result)
        hipcub::DoubleBuffer<uint64_t> keys(t.d_key.p, d_key2.p);
        hipcub::DoubleBuffer<uint32_t> vals(t.d_idx.p, d_idx2.p);
        PC_TRY(cub_run(d_sort_tmp, [&](void *tmp, size_t &bytes) { return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys, vals, (int)nrec, 0, key_bits, st); }));
        const uint32_t *perm = vals.Current();
        b.file_order.swap(perm == t.d_idx.p ? t.d_idx : d_idx2);   // (the permutation is the staged records' numbers in the file)
        HIP_TRY(hipMemsetAsync(d_runs_sorted.p + nrec, 0, 4, st));
        hipLaunchKernelGGL(k_bam_sort_rank, dim3(t.g256), dim3(256), 0, st, t.d_recs.p, nrec, perm, w.d_staged_at.p, d_runs_sorted.p, t.d_misc.p, t.d_misc.p + 4);
        HIP_TRY(hipGetLastError());
        PC_TRY(cub_run_sized(d_tmp, tmp_bytes, sum(d_runs_sorted.p, d_runs_sorted.p)));   // (in place)
        hipLaunchKernelGGL(k_bam_sort_run_at, dim3(t.g256), dim3(256), 0, st, perm, d_runs_sorted.p, nrec, w.d_run_at.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(t.sev.ev[3], st));
        b.key_bits = key_bits;
    }
    HIP_TRY(hipMemcpyAsync(&tot[0], w.d_staged_at.p + nrec, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&tot[1], w.d_run_at.p + nrec, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(misc, t.d_misc.p, sizeof(misc), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    w.n_staged = tot[0]; w.n_runs = tot[1]; w.first_err = misc[0];
    b.mapped = (int64_t)misc[1]; b.unplaced = (int64_t)misc[2];
    if (sort) {
        b.sort_ms = ms_between(t.sev.ev[0], t.sev.ev[1]) + (t.disorder ? ms_between(t.sev.ev[2], t.sev.ev[3]) : 0.0);
        b.moved = (int64_t)misc[4];
        if (!b.moved) b.file_order.release();
    }
    return record_defect(misc[0], recs.truncated, d.path.c_str());
}

// Step 3: the columns of `b`, and the marker of every staged record that is wide.
int write_columns(BamDecode &d, const BamPlan &pl, int64_t nrec, ColumnWork &w, pc_bam &b) {
    hipStream_t st = d.st;
    const RecordTable &t = w.t;
    const size_t ns = (size_t)std::max<int64_t>(w.n_staged, 1), nrun = (size_t)std::max<int64_t>(w.n_runs, 1);   // (no empty column)
    int rc = PC_OK;
    room(rc, b.tid, ns); room(rc, b.pos, ns); room(rc, b.alen, ns); room(rc, b.flags, ns); room(rc, b.nblk, ns);
    room(rc, b.flag16, ns); room(rc, b.mapq, ns); room(rc, b.lseq, ns); room(rc, b.nh, ns);
    room(rc, b.blk_start, nrun); room(rc, b.blk_len, nrun);
    room(rc, w.d_wide, ns);
    if (rc != PC_OK) return rc;
    HIP_TRY(hipMemsetAsync(w.d_wide.p, 0, ns * 4, st));
    hipLaunchKernelGGL(pcbam::k_bam_columns, dim3(t.g256), dim3(256), 0, st, d.d_stream.p, d.d_members.p, t.d_rec_base.p, d.d_rec_off.p, pl.nm(), t.d_rec_member.p, t.d_recs.p,
                       nrec, w.d_staged_at.p, w.d_run_at.p, b.tid.p, b.pos.p, b.alen.p, b.flags.p, b.nblk.p, b.blk_start.p, b.blk_len.p, w.d_wide.p,
                       b.flag16.p, b.mapq.p, b.lseq.p, b.nh.p);
    HIP_TRY(hipGetLastError());
    return PC_OK;
}

// Step 4: wide records (beyond the 16-bit / 8-bit columns): rare -- their staged indices are found from the markers on
// the host side of pc_bam_read; the true values are read back here, record by record.  A plain read-back of the markers is
// only paid when the file has any: a device-side total first.
int collect_wide(BamDecode &d, int64_t nrec, ColumnWork &w, pc_bam &b) {
    hipStream_t st = d.st;
    const int64_t n_staged = w.n_staged;
    uint32_t last_sum = 0, last_flag = 0;
    DevBuf<uint32_t> d_wsum;
    DevBuf<uint8_t> d_tmp;
    DrainOnExit drained{st};
    PC_TRY(d_wsum.reserve((size_t)n_staged + 1));
    auto sum_wide = [&](int64_t cnt) { return [&, cnt](void *tmp, size_t &bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, w.d_wide.p, d_wsum.p, (int)cnt, st); }; };
    size_t most = 16, tmp_bytes = 0;
    PC_TRY(cub_need(most, tmp_bytes, sum_wide(std::max<int64_t>(n_staged, 1))));
    PC_TRY(d_tmp.reserve(most));
    if (n_staged > 0) {
        PC_TRY(cub_run_sized(d_tmp, tmp_bytes, sum_wide(n_staged)));
        HIP_TRY(hipMemcpyAsync(&last_sum, d_wsum.p + (n_staged - 1), 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&last_flag, w.d_wide.p + (n_staged - 1), 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    if (last_sum + last_flag == 0) return PC_OK;
    std::vector<uint32_t> wf((size_t)n_staged), sa((size_t)nrec);
    std::vector<pcbam::RecOut> ro((size_t)nrec);
    HIP_TRY(hipMemcpy(wf.data(), w.d_wide.p, (size_t)n_staged * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sa.data(), w.d_staged_at.p, (size_t)nrec * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ro.data(), w.t.d_recs.p, (size_t)nrec * sizeof(pcbam::RecOut), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < nrec; ++i)
        if (ro[(size_t)i].placed == 1 && wf[sa[(size_t)i]]) {
            b.wide_idx.push_back((int64_t)sa[(size_t)i]);
            b.wide_alen.push_back((int32_t)ro[(size_t)i].L);
            b.wide_nblk.push_back((int32_t)ro[(size_t)i].nruns);
        }
    if (b.moved) bh::order_wide_list(b.wide_idx, b.wide_alen, b.wide_nblk);   // (the walk above is in file order)
    return PC_OK;
}

// Phase 5: fields, order checks (or, with `sort`, the coordinate sort), the region filter, the scans that place every kept record, and the columns of `b`.
int decode_columns(BamDecode &d, const BamPlan &pl, const BamSpan *span, const BamHeader &h, const BamRecords &recs, pc_bam &b, bool sort) {
    hipStream_t st = d.st;
    const int64_t nrec = recs.nrec;
    ColumnWork w;
    DrainOnExit drained{st};   // (misc: [1] mapped, [2] unplaced; with `sort`: [3] out of order, [4] records moved)
    PC_TRY(decode_fields(d, pl, h, recs, 6, (size_t)nrec + 1, sort, w.t));
    if (nrec > 0) {
        int rc = PC_OK;
        room(rc, w.d_runs, (size_t)nrec + 1); room(rc, w.d_staged_at, (size_t)nrec + 1); room(rc, w.d_run_at, (size_t)nrec + 1);
        if (rc != PC_OK) return rc;
        if (sort) b.sorted_input = !w.t.disorder;
        if (span) PC_TRY(filter_regions(d, *span, nrec, w));
        PC_TRY(place_records(d, h, recs, sort, w, b));
        PC_TRY(write_columns(d, pl, nrec, w, b));
        PC_TRY(collect_wide(d, nrec, w, b));
    } else if (recs.truncated) return fail(PC_ERR_ARG, "truncated BAM record");
    HIP_TRY(hipEventRecord(d.ev[4], st));
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    d.clk.lap("fields + scans + columns");
    b.n = w.n_staged; b.nrun = w.n_runs;
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

// ---- the index build's phase 5.  What its steps share beside the record table:
struct IndexWork {
    RecordTable t;
    std::vector<uint64_t> blk;           // bh::tell_table (host copy: alive while its upload is)
    DevBuf<uint64_t> d_blk, d_key, d_voff, d_cov, d_covered;
    DevBuf<uint32_t> d_mapped, d_mapped_before, d_head, d_slot;
    DevBuf<int32_t> d_win_a;
    DevBuf<int64_t> d_ref_fl;            // first record of every reference, then the last
    DevBuf<uint64_t> d_ref_be;           // per reference: offset of its first record, then of the first record behind its last
    DevBuf<int64_t> d_ref_cnt;           // mapped, then unmapped
    DevBuf<int32_t> d_n_intv;
    DevBuf<int64_t> d_lin_base;
    DevBuf<uint64_t> d_sbeg, d_send, d_linear, d_filled, d_sloff;   // the runs in (tid, bin) order; the windows
    DevBuf<uint32_t> d_sbin;
    DevBuf<int32_t> d_stid;
    size_t nr = 1;                       // references, at least one
    int64_t n_runs = 0, n_lin = 0;
    unsigned g256p = 0;                  // blocks of 256 threads over the records and the end entry
    int reserve(int64_t nrec, int n_ref) {
        const size_t n1 = (size_t)nrec + 1;
        nr = (size_t)std::max(n_ref, 1);
        g256p = (unsigned)((nrec + 1 + 255) / 256);
        int rc = PC_OK;
        room(rc, d_key, (size_t)nrec); room(rc, d_voff, n1); room(rc, d_cov, n1); room(rc, d_covered, n1); room(rc, d_win_a, (size_t)nrec);
        room(rc, d_mapped, n1); room(rc, d_mapped_before, n1); room(rc, d_head, n1); room(rc, d_slot, n1); room(rc, d_ref_fl, 2 * nr);
        return rc;
    }
};

// Step 1: keys, run heads, per-reference bounds and counts, covered windows; what sizes the rest comes down.
int index_keys_and_stats(BamDecode &d, const BamPlan &pl, const BamHeader &h, const BamRecords &recs, const IndexShape &shape, IndexWork &w, IndexParts &out) {
    using namespace pcbam;
    using namespace pcidx;
    hipStream_t st = d.st;
    const RecordTable &t = w.t;
    const int64_t nrec = recs.nrec;
    const int n_ref = (int)h.n_ref, nm = pl.nm();
    const size_t n1 = (size_t)nrec + 1, nr = w.nr;
    std::vector<int32_t> n_intv((size_t)n_ref, 0);
    uint32_t n_runs32 = 0;
    unsigned long long misc[2] = {0, 0};
    DevBuf<uint8_t> d_tmp;
    DrainOnExit drained{st};
    const auto idx_keys = shape.csi ? k_idx_keys<false> : k_idx_keys<true>;
    hipLaunchKernelGGL(idx_keys, dim3(w.g256p), dim3(256), 0, st, d.d_stream.p, d.d_members.p, w.d_blk.p, t.d_rec_base.p, d.d_rec_off.p, nm, nrec, t.d_rec_member.p,
                       t.d_recs.p, w.d_key.p, w.d_voff.p, w.d_win_a.p, w.d_cov.p, w.d_mapped.p, (uint32_t *)(t.d_misc.p + 1), shape.min_shift, shape.n_lvls);
    HIP_TRY(hipMemsetAsync(w.d_ref_fl.p, 0xff, 2 * nr * sizeof(int64_t), st));
    hipLaunchKernelGGL(k_idx_heads, dim3(w.g256p), dim3(256), 0, st, w.d_key.p, nrec, w.d_head.p, w.d_ref_fl.p, w.d_ref_fl.p + nr);
    HIP_TRY(hipGetLastError());
    {
        auto sum = [=](uint32_t *from, uint32_t *to) { return [=](void *tmp, size_t &bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, from, to, (int)n1, st); }; };
        auto max_cov = [&](void *tmp, size_t &bytes) { return hipcub::DeviceScan::ExclusiveScan(tmp, bytes, w.d_cov.p, w.d_covered.p, hipcub::Max(), (uint64_t)0, (int)n1, st); };
        size_t most = 16, asked = 0;   // (one temporary for the three: each runs with all of it)
        PC_TRY(cub_need(most, asked, sum(w.d_head.p, w.d_slot.p)));
        PC_TRY(cub_need(most, asked, max_cov));
        PC_TRY(d_tmp.reserve(most));
        PC_TRY(cub_run_sized(d_tmp, most, sum(w.d_head.p, w.d_slot.p)));
        PC_TRY(cub_run_sized(d_tmp, most, sum(w.d_mapped.p, w.d_mapped_before.p)));
        PC_TRY(cub_run_sized(d_tmp, most, max_cov));
    }
    int rc = PC_OK;
    room(rc, w.d_ref_be, 2 * nr); room(rc, w.d_ref_cnt, 2 * nr); room(rc, w.d_n_intv, nr);
    if (rc != PC_OK) return rc;
    if (n_ref) {
        hipLaunchKernelGGL(k_idx_ref_stats, dim3((unsigned)((n_ref + 255) / 256)), dim3(256), 0, st, n_ref, w.d_ref_fl.p, w.d_ref_fl.p + nr, w.d_voff.p, w.d_mapped_before.p,
                           w.d_covered.p, w.d_ref_be.p, w.d_ref_be.p + nr, w.d_ref_cnt.p, w.d_ref_cnt.p + nr, w.d_n_intv.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(n_intv.data(), w.d_n_intv.p, (size_t)n_ref * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out.ref_beg.data(), w.d_ref_be.p, (size_t)n_ref * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out.ref_end.data(), w.d_ref_be.p + nr, (size_t)n_ref * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out.ref_mapped.data(), w.d_ref_cnt.p, (size_t)n_ref * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out.ref_unmapped.data(), w.d_ref_cnt.p + nr, (size_t)n_ref * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(&n_runs32, w.d_slot.p + nrec, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(misc, t.d_misc.p, sizeof(misc), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    if ((uint32_t)misc[1]) {
        if (!shape.csi) return fail(PC_ERR_ARG, "a BAI index cannot hold %s: an alignment reaches beyond 2^29", d.path.c_str());
        return fail(PC_ERR_ARG, "a CSI index of min_shift %d and depth %d cannot hold %s: an alignment reaches beyond %lld", shape.min_shift, shape.n_lvls,
                    d.path.c_str(), (long long)shape.reach());
    }
    int64_t placed = 0;
    for (int r = 0; r < n_ref; ++r) {
        out.lin_start[(size_t)r + 1] = out.lin_start[(size_t)r] + n_intv[(size_t)r];
        placed += out.ref_mapped[(size_t)r] + out.ref_unmapped[(size_t)r];
    }
    out.n_no_coor = nrec - placed;
    w.n_runs = (int64_t)n_runs32;
    w.n_lin = out.n_windows = out.lin_start[(size_t)n_ref];
    if (shape.csi && w.n_lin > kMaxWindows)
        return fail(PC_ERR_ARG, "a CSI index of min_shift %d of %s has %lld windows, more than 2^28: use a larger min_shift", shape.min_shift, d.path.c_str(),
                    (long long)w.n_lin);
    return PC_OK;
}

// Step 2: the buffers of the sorted runs and the windows; the runs, sorted by (tid, bin), gathered in that order.
int index_sort_runs(BamDecode &d, const BamRecords &recs, int n_ref, const IndexShape &shape, IndexWork &w, const IndexParts &out) {
    using namespace pcidx;
    hipStream_t st = d.st;
    const int64_t nrec = recs.nrec, n_runs = w.n_runs, n_lin = w.n_lin;
    std::vector<uint32_t> iota((size_t)n_runs);   // (hipcub's iota: the slots 0 .. n_runs - 1 are the values of the sort)
    DevBuf<uint64_t> d_run_key, d_run_key2, d_run_beg, d_run_end;
    DevBuf<uint32_t> d_order, d_order2;
    DevBuf<uint8_t> d_sort_tmp;
    DrainOnExit drained{st};
    const size_t nrun = (size_t)std::max<int64_t>(n_runs, 1);
    int rc = PC_OK;
    room(rc, d_run_key, nrun); room(rc, d_run_key2, nrun); room(rc, d_run_beg, nrun); room(rc, d_run_end, nrun); room(rc, w.d_sbeg, nrun); room(rc, w.d_send, nrun);
    room(rc, d_order, nrun); room(rc, d_order2, nrun); room(rc, w.d_sbin, nrun); room(rc, w.d_stid, nrun);
    room(rc, w.d_linear, (size_t)std::max<int64_t>(n_lin, 1));
    if (shape.csi) { room(rc, w.d_filled, (size_t)std::max<int64_t>(n_lin, 1)); room(rc, w.d_sloff, nrun); }
    if (rc == PC_OK) rc = w.d_lin_base.upload(out.lin_start, st);
    if (rc != PC_OK) return rc;
    if (!n_runs) { drained.armed = false; return PC_OK; }   // (nothing queued but the upload of lin_start, which `out` outlives)
    hipLaunchKernelGGL(k_idx_runs, dim3(w.g256p), dim3(256), 0, st, w.d_key.p, w.d_voff.p, w.d_head.p, w.d_slot.p, nrec, d_run_key.p, d_run_beg.p, d_run_end.p);
    std::iota(iota.begin(), iota.end(), 0u);
    HIP_TRY(hipMemcpyAsync(d_order.p, iota.data(), (size_t)n_runs * 4, hipMemcpyHostToDevice, st));
    const int key_bits = bh::index_key_bits((uint64_t)n_ref);
    PC_TRY(cub_run(d_sort_tmp, [&](void *tmp, size_t &bytes) { return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, d_run_key.p, d_run_key2.p, d_order.p, d_order2.p, (int)n_runs, 0, key_bits, st); }));
    hipLaunchKernelGGL(k_idx_gather, dim3((unsigned)((n_runs + 255) / 256)), dim3(256), 0, st, d_run_key2.p, d_order2.p, d_run_beg.p, d_run_end.p, n_runs,
                       w.d_stid.p, w.d_sbin.p, w.d_sbeg.p, w.d_send.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // (iota and the sort's scratch go out of scope)
    drained.armed = false;
    return PC_OK;
}

// Step 3: the linear windows; CSI: the forward fill (one running maximum over the windows of all references), then loff per run.
int index_windows(BamDecode &d, int64_t nrec, int n_ref, const IndexShape &shape, IndexWork &w) {
    using namespace pcidx;
    hipStream_t st = d.st;
    const int64_t n_runs = w.n_runs, n_lin = w.n_lin;
    DevBuf<uint8_t> d_fill_tmp;   // (the scan's scratch: alive up to the synchronisation below)
    DrainOnExit drained{st};
    if (n_lin) {
        HIP_TRY(hipMemsetAsync(w.d_linear.p, 0, (size_t)n_lin * 8, st));
        hipLaunchKernelGGL(k_idx_linear, dim3(w.t.g256), dim3(256), 0, st, w.d_cov.p, w.d_covered.p, w.d_win_a.p, w.d_voff.p, nrec, w.d_lin_base.p, w.d_linear.p);
        HIP_TRY(hipGetLastError());
    }
    if (shape.csi && n_runs) {
        if (n_lin) {
            hipLaunchKernelGGL(k_idx_first_window, dim3((unsigned)((n_ref + 255) / 256)), dim3(256), 0, st, n_ref, w.d_n_intv.p, w.d_lin_base.p, w.d_ref_be.p, w.d_linear.p);
            HIP_TRY(hipGetLastError());
            PC_TRY(cub_run(d_fill_tmp, [&](void *tmp, size_t &bytes) { return hipcub::DeviceScan::InclusiveScan(tmp, bytes, w.d_linear.p, w.d_filled.p, hipcub::Max(), (int)n_lin, st); }));
        }
        hipLaunchKernelGGL(k_idx_loff, dim3((unsigned)((n_runs + 255) / 256)), dim3(256), 0, st, w.d_stid.p, w.d_sbin.p, n_runs, shape.n_lvls, w.d_n_intv.p,
                           w.d_lin_base.p, w.d_filled.p, w.d_sloff.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    return PC_OK;
}

// Step 4: the sorted runs and the linear arrays (BAI) or the runs' loff (CSI: the windows stay in HBM) come down.
int index_read_back(BamDecode &d, const IndexShape &shape, IndexWork &w, IndexParts &out) {
    hipStream_t st = d.st;
    const size_t n_runs = (size_t)w.n_runs, n_lin = (size_t)w.n_lin;
    out.run_tid.resize(n_runs); out.run_bin.resize(n_runs); out.run_beg.resize(n_runs); out.run_end.resize(n_runs);
    if (shape.csi) out.run_loff.resize(n_runs);
    else out.linear.resize(n_lin);
    DrainOnExit drained{st};
    if (n_runs) {
        HIP_TRY(hipMemcpyAsync(out.run_tid.data(), w.d_stid.p, n_runs * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out.run_bin.data(), w.d_sbin.p, n_runs * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out.run_beg.data(), w.d_sbeg.p, n_runs * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out.run_end.data(), w.d_send.p, n_runs * 8, hipMemcpyDeviceToHost, st));
    }
    if (shape.csi) { if (n_runs) HIP_TRY(hipMemcpyAsync(out.run_loff.data(), w.d_sloff.p, n_runs * 8, hipMemcpyDeviceToHost, st)); }
    else if (n_lin) HIP_TRY(hipMemcpyAsync(out.linear.data(), w.d_linear.p, n_lin * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    return PC_OK;
}

// The index build's phase 5 (whole-file reads only): k_bam_fields and the order checks as decode_columns runs them -- no
// column is written or read back -- then the kernels of index_kernels.hip.h; the sorted runs, the linear arrays (BAI) or
// the runs' loff (CSI) and the per-reference counts come down.
int index_records(BamDecode &d, const BamPlan &pl, int64_t size, const BamHeader &h, const BamRecords &recs, const IndexShape &shape, IndexParts &out) {
    hipStream_t st = d.st;
    const int64_t nrec = recs.nrec;
    const int n_ref = (int)h.n_ref;
    const auto t0 = std::chrono::steady_clock::now();
    auto ms_since = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); };
    out.lin_start.assign((size_t)n_ref + 1, 0);
    out.ref_beg.assign((size_t)n_ref, 0); out.ref_end.assign((size_t)n_ref, 0);
    out.ref_mapped.assign((size_t)n_ref, 0); out.ref_unmapped.assign((size_t)n_ref, 0);
    if (nrec == 0) return record_defect(~0ull, recs.truncated, d.path.c_str());
    IndexWork w;
    unsigned long long first_err = ~0ull;
    DrainOnExit drained{st};
    // (misc: [1] (as uint32) a record reaches beyond the index's range)
    PC_TRY(decode_fields(d, pl, h, recs, 2, 1, false, w.t));
    PC_TRY(w.reserve(nrec, n_ref));   // (behind the record table, as ever: the pool hands the blocks out in this order)
    w.blk = bh::tell_table(pl.members, size);
    PC_TRY(w.d_blk.upload(w.blk, st));
    HIP_TRY(hipMemcpyAsync(&first_err, w.t.d_misc.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out.ms_fields = ms_since(t0);
    PC_TRY(record_defect(first_err, recs.truncated, d.path.c_str()));   // the decoder's own refusals, in its order
    const auto t1 = std::chrono::steady_clock::now();
    PC_TRY(index_keys_and_stats(d, pl, h, recs, shape, w, out));
    PC_TRY(index_sort_runs(d, recs, n_ref, shape, w, out));
    PC_TRY(index_windows(d, nrec, n_ref, shape, w));
    out.ms_kernels = ms_since(t1);
    const auto t2 = std::chrono::steady_clock::now();
    PC_TRY(index_read_back(d, shape, w, out));
    drained.armed = false;
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
    const int defect = bh::plan_members(image, size, span, knobs.walk_min, pl);
    if (defect) return host_defect(defect, d.path.c_str());
    pc_bam *b = new pc_bam();
    d.clk.lap("member walk");
    b->e = e; b->name = d.path; b->members = (int64_t)pl.nm(); b->inflated_bytes = (int64_t)pl.total_u; b->compressed_bytes = size;
    b->uploaded_bytes = pl.image_bytes; b->runs = (int64_t)pl.runs.size();
    struct Guard { pc_bam *b; ~Guard() { if (b) pc_bam_close(b); } } guard{b};
    PC_TRY(d.ev.create());
    int rc = upload_and_inflate(d, image, pl, uploaded);
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
    d.ev.laps(b->ms, 4);
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
    const int defect = bh::plan_members(image, size, nullptr, knobs.walk_min, pl);
    if (defect) return host_defect(defect, d.path.c_str());
    d.clk.lap("member walk");
    PC_TRY(d.ev.create());
    int rc = upload_and_inflate(d, image, pl, uploaded);
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
    d.ev.laps(idx->ms, 3);
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

static int stage_opened(pc_engine *e, pc_bam *b, int64_t *mapped, const BamKnobs &knobs);
static int add_alignment_bam_impl(pc_engine *e, const void *image, int64_t size, const char *name, int64_t *mapped, const UploadedHook *uploaded,
                                  const BamSpan *span, const BamKnobs &knobs, uint32_t open_flags = 0) {
    pc_bam *b = nullptr;
    const int rc = bam_open_span_retry(e, image, size, name, &b, uploaded, span, knobs, open_flags);
    return rc != PC_OK ? rc : stage_opened(e, b, mapped, knobs);
}
// The tail of every staging entry point (BAM and SAM text): the opened file's columns become a staged file of the engine,
// and the handle is closed.
static int stage_opened(pc_engine *e, pc_bam *b, int64_t *mapped, const BamKnobs &knobs) {
    int rc = PC_OK;
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
