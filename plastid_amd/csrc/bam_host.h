// bam_host.h -- the host logic of the two BAM decoders that touches neither HIP nor zlib: the gzip / BGZF member header
// and the BAM header (one parser each, for the GPU decoder of bam_decoder.hip.h and the host decoder of bam_stager.cpp:
// their messages agree because they are the same), and the host arithmetic of the GPU decoder's phases -- which members
// go to the device and where they land (plan_members), the pieces the image is uploaded in, the bounds of a region
// read's record chains, one round of the host's look at the members' chains, and the small tables of the field and index
// phases.  A defect is a code with its text beside it (defect_text); the caller makes an error of it.  Plain C++17, so
// that tests/test_host_logic.py can compile tests/bam_host_test.cpp against it on a machine without a GPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "host_util.h"
#include "index_shape.h"

namespace pcbam {

struct Member {
    uint64_t coff;     // offset of the raw DEFLATE stream in the file image (behind the gzip header)
    uint32_t clen;     // its length (the 8-byte trailer excluded)
    uint32_t ulen;     // ISIZE: bytes it inflates to
    uint64_t uoff;     // where they go in the inflated stream
    uint32_t crc;      // CRC-32 of the payload (gzip trailer)
    uint32_t hdr;      // bytes of its gzip header (host side: the member starts at coff - hdr in the file)
};

struct MemberChain {
    uint64_t first;      // stream offset of the first record start at or behind the member's begin (guessed or given)
    uint64_t next;       // where the chain from `first` leaves the member: the first record start at or behind its end
    uint32_t nrec;       // record starts in [first, member end)
    uint32_t flags;      // 1: no plausible start found, 2: a length prefix below the fixed fields met on the way
};

} // namespace pcbam

namespace pcbamhost {

using pcbam::Member;
using pcbam::MemberChain;

inline uint16_t rd16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// ---- defects: of a member header (1 .. 7, in the order parse_member looks for them), of a region read's chunk list
// against the file (the index does not belong to it)
enum Defect {
    kOk = 0, kMemberShort = 1, kMemberMagic = 2, kMemberExtraCut = 3, kMemberNoBC = 4, kMemberCut = 5, kMemberIsize = 6, kMemberTiny = 7,
    kChunkNoStart = 8, kChunkNoEnd = 9, kChunkBeyond = 10, kChunkInHeader = 11, kChunkInRecord = 12
};
constexpr const char *kInflateFailedIn = "BGZF inflate failed in ", *kCrcMismatchIn = "BGZF CRC mismatch in ";   // (the file's name follows)
inline bool chunk_defect(int code) { return code >= kChunkNoStart; }
// the text of a member defect (kMemberTiny: the file's name follows); of a chunk defect: the reason inside
// "the index does not belong to this BAM file (...)"
inline const char *defect_text(int code) {
    static const char *const text[] = {"", "truncated BGZF header", "not a BGZF file (bad gzip member header)", "truncated BGZF extra field",
                                       "BGZF member without BC subfield", "truncated BGZF member", "corrupt BGZF member (more than 64 KiB of payload)",
                                       kInflateFailedIn, "a chunk does not start at a BGZF member", "a chunk does not end at a BGZF member",
                                       "a chunk lies beyond its end", "a chunk starts inside the header or ends before it starts",
                                       "a chunk ends inside a record"};
    return text[code];
}

// One member at `off` of an image of `size` bytes: kOk, or which defect.  kMemberTiny (no room for header and trailer)
// still sets clen_out and mb.ulen (0 where the member has no room for an ISIZE word either): the host decoder walks on
// and refuses the member when it inflates it.  kMemberCut sets clen_out too: a reader that holds only the head of the
// member then knows how much to fetch.
inline int parse_member(const uint8_t *image, int64_t size, int64_t off, Member &mb, int64_t &clen_out) {
    if (off + 18 > size) return kMemberShort;
    const uint8_t *h = image + off;
    if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) return kMemberMagic;
    const uint16_t xlen = rd16(h + 10);
    if (off + 12 + xlen > size) return kMemberExtraCut;
    int bsize = -1;
    for (size_t x = 0; x + 4 <= xlen;) {
        const uint8_t *sf = h + 12 + x;
        const uint16_t slen = rd16(sf + 2);
        if (sf[0] == 'B' && sf[1] == 'C' && slen == 2 && x + 6 <= xlen) bsize = rd16(sf + 4);   // (the two payload bytes lie inside the extra field)
        x += 4 + slen;
    }
    if (bsize < 0) return kMemberNoBC;
    const int64_t clen = (int64_t)bsize + 1;
    clen_out = clen;
    if (off + clen > size) return kMemberCut;
    const uint32_t isize = clen >= 4 ? rd32(image + off + clen - 4) : 0u;
    if (isize > (1u << 16)) return kMemberIsize;
    const int64_t hdr = 12 + xlen;
    mb.ulen = isize;
    if (clen < hdr + 8) return kMemberTiny;
    mb.coff = (uint64_t)(off + hdr); mb.clen = (uint32_t)(clen - hdr - 8); mb.uoff = 0;
    mb.crc = rd32(image + off + clen - 8); mb.hdr = (uint32_t)hdr;
    return kOk;
}

// ---- the BAM header (magic, text, reference list) at the head of the inflated stream
struct BamHeader {
    uint64_t first_record = 0;   // stream offset of the first record
    uint32_t n_ref = 0;
    std::vector<std::string> ref_names;
    std::vector<int32_t> ref_lengths;
};
// kHeaderMore: the bytes end inside the header; `text` is what a caller reports that has no more of them
enum HeaderStatus { kHeaderOk = 0, kHeaderMore = 1, kHeaderDefect = 2 };
struct HeaderParse { HeaderStatus status; const char *text; };
inline HeaderParse parse_bam_header(const uint8_t *p, size_t n, BamHeader &h) {
    const uint8_t *const begin = p, *const end = p + n;
    const char *const magic = "not a BAM file (bad magic)";
    if (n >= 4 && std::memcmp(p, "BAM\1", 4) != 0) return {kHeaderDefect, magic};
    if (n < 12) return {kHeaderMore, magic};
    const uint32_t l_text = rd32(p + 4);
    p += 8;
    if ((size_t)(end - p) < (size_t)l_text + 4) return {kHeaderMore, "truncated BAM header"};
    p += l_text;
    h.n_ref = rd32(p);
    p += 4;
    h.ref_names.clear(); h.ref_lengths.clear();
    for (uint32_t r = 0; r < h.n_ref; ++r) {
        if (end - p < 4) return {kHeaderMore, "truncated BAM reference list"};
        const uint32_t l_name = rd32(p);
        p += 4;
        if ((size_t)(end - p) < (size_t)l_name + 4) return {kHeaderMore, "truncated BAM reference list"};
        h.ref_names.emplace_back((const char *)p, l_name ? l_name - 1 : 0);
        p += l_name;
        h.ref_lengths.push_back((int32_t)rd32(p));
        p += 4;
    }
    h.first_record = (uint64_t)(p - begin);
    return {kHeaderOk, nullptr};
}

// ---- phase 1 of the GPU decoder: member boundaries (a walk over the gzip headers; 18 + bytes per 64 KiB of payload)
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

// What goes to the GPU and where it lands: the non-empty members, the runs of the file they come from, and where the
// chunks of a region read start and end.
struct BamPlan {
    // [file_lo, file_hi) lands at image offset dev_lo and holds members [m0, m1) (a whole-file read: one run)
    struct Run { int64_t file_lo, file_hi, dev_lo; int m0, m1; };
    // where a chunk starts and ends, by member (index in `members` of the member at the offset -- of the next non-empty
    // one for an empty member, members.size() past the last) and offset in its payload
    struct ChunkAt { int64_t cb; int s_idx, e_idx; uint32_t ub, ue; };
    std::vector<Member> members;
    std::vector<Run> runs;
    std::vector<uint32_t> member_run;   // the run each member belongs to
    std::vector<ChunkAt> chunk_at;
    uint64_t total_u = 0;               // bytes of the inflated stream
    int64_t image_bytes = 0;            // bytes of the file that go to the device
    int nm() const { return (int)members.size(); }
    // stream offset at which member index m starts (total_u past the last)
    uint64_t uoff_of(int m) const { return m < nm() ? members[(size_t)m].uoff : total_u; }
};

// A region read's members: the header's from the start of the file, then every chunk's.
inline int plan_region(const uint8_t *image, int64_t size, const BamSpan &span, BamPlan &pl) {
    std::vector<Member> &members = pl.members;
    std::vector<BamPlan::Run> &runs = pl.runs;
    // every member walked: its file offset, its index in `members` (see ChunkAt) and its payload length
    struct Walked { int64_t off; int idx; uint32_t ulen; };
    std::vector<Walked> walked;
    // members from `off` on while they start before `hi_excl` (or at `last`, with_last); a new run unless `off` continues the last
    auto walk = [&](int64_t off, int64_t hi_excl, bool with_last, int64_t last) -> int {
        if (runs.empty() || runs.back().file_hi != off) runs.push_back(BamPlan::Run{off, off, 0, (int)members.size(), (int)members.size()});
        const int64_t first = off;
        while (off < size && (off < hi_excl || (with_last && off <= last))) {
            Member mb;
            int64_t clen = 0;
            const int code = parse_member(image, size, off, mb, clen);
            if (code) return off == first && first > 0 ? (int)kChunkNoStart : code;
            walked.push_back(Walked{off, (int)members.size(), mb.ulen});
            if (mb.ulen) members.push_back(mb);
            off += clen;
        }
        runs.back().file_hi = off; runs.back().m1 = (int)members.size();
        if (runs.back().file_hi == runs.back().file_lo) runs.pop_back();
        return kOk;
    };
    auto find = [&](int64_t off) -> const Walked * {
        auto it = std::lower_bound(walked.begin(), walked.end(), off, [](const Walked &w, int64_t o) { return w.off < o; });
        return it != walked.end() && it->off == off ? &*it : nullptr;
    };
    const int64_t cb0 = span.nchunk > 0 ? (int64_t)(span.cbeg[0] >> 16) : size;
    int rc = walk(0, std::min<int64_t>(span.header_bytes, cb0), false, 0);
    if (rc != kOk) return rc;
    for (int k = 0; k < span.nchunk; ++k) {
        const uint64_t vb = span.cbeg[k], ve = span.cend[k];
        const int64_t cb = (int64_t)(vb >> 16), ce = (int64_t)(ve >> 16);
        const uint32_t ub = (uint32_t)(vb & 0xffffu), ue = (uint32_t)(ve & 0xffffu);
        if (cb >= size || ce > size || (ue && ce >= size)) return kChunkBeyond;
        const int64_t hi = runs.empty() ? 0 : runs.back().file_hi;
        if (cb < hi && !find(cb)) return kChunkNoStart;
        rc = walk(std::max(cb, hi), ce, ue != 0, ce);
        if (rc != kOk) return rc;
        BamPlan::ChunkAt c{cb, 0, 0, ub, ue};
        const Walked *ws = find(cb);
        if (!ws || ub > ws->ulen) return kChunkNoStart;
        c.s_idx = ws->idx;
        if (ue) {
            const Walked *we = find(ce);
            if (!we || ue > we->ulen) return kChunkNoEnd;
            c.e_idx = we->idx;
        } else {
            if (runs.empty() || runs.back().file_hi != ce) return kChunkNoEnd;
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
    return kOk;
}

// Every member of the file, as one run.
inline int plan_whole_file(const uint8_t *image, int64_t size, int64_t walk_min, BamPlan &pl, int threads = 0) {
    std::vector<Member> &members = pl.members;
    int64_t walked_to = 0;
    // Large files: the walk is a chain of dependent cache misses (40 k members: 5.6 ms), so every host thread walks its
    // own stretch of the file from the first offset in it where three members in a row parse; a stretch counts only if
    // the walk of the stretch before it LANDS on its first member -- whatever does not chain is walked again, serially.
    const int WT = size >= walk_min && size >= 64 ? std::max(1, std::min(threads > 0 ? threads : usable_cpus(), 16)) : 1;
    if (WT > 1) {
        struct Stretch { int64_t first = -1, landing = -1; std::vector<Member> mem; };
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
                            Member mb;
                            int64_t cl = 0;
                            ok = parse_member(image, size, q, mb, cl) == kOk;
                            q += cl;
                        }
                        if (ok) { off = c; break; }
                    }
                    if (off < 0) continue;
                }
                sx.first = off;
                while (off < hi && off < size) {
                    Member mb;
                    int64_t cl = 0;
                    if (parse_member(image, size, off, mb, cl) != kOk) { sx.first = -1; break; }   // (a defect: the serial walk below reports it)
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
        Member mb;
        int64_t clen = 0;
        const int code = parse_member(image, size, off, mb, clen);
        if (code) return code;
        if (mb.ulen) members.push_back(mb);      // (empty members -- the end-of-file marker -- hold nothing)
        off += clen;
    }
    pl.runs.push_back(BamPlan::Run{0, size, 0, 0, (int)members.size()});
    return kOk;
}

// Phase 1 (host only): which members go to the GPU (`span`: those of a region read; nullptr: the whole file), in which
// runs, and where they land in the image on the device and in the inflated stream.  kOk, or the defect.
// (`threads`: of the parallel member walk; 0: as many as the process may use, at most 16)
inline int plan_members(const uint8_t *image, int64_t size, const BamSpan *span, int64_t walk_min, BamPlan &pl, int threads = 0) {
    const int rc = span ? plan_region(image, size, *span, pl) : plan_whole_file(image, size, walk_min, pl, threads);
    if (rc != kOk) return rc;
    for (Member &mb : pl.members) { mb.uoff = pl.total_u; pl.total_u += mb.ulen; }
    for (const BamPlan::Run &r : pl.runs) pl.image_bytes += r.file_hi - r.file_lo;
    pl.member_run.assign((size_t)std::max(pl.nm(), 1), 0u);
    for (size_t r = 0; r < pl.runs.size(); ++r)
        for (int m = pl.runs[r].m0; m < pl.runs[r].m1; ++m) pl.member_run[(size_t)m] = (uint32_t)r;
    return kOk;
}

// ---- phase 2: the pieces the image is uploaded and inflated in.  Members [m0, m1), bytes [byte0, byte1) of the image on
// the device (gzip headers and trailers ride along); one_run: the bytes are contiguous in the file.  A piece ends with a
// whole member (up to 64 KiB beyond piece_bytes) and where a run ends (one piece may hold several short runs); the last
// one takes the rest of the image.
struct ImagePiece { int m0, m1; int64_t byte0, byte1; bool one_run; };
inline std::vector<ImagePiece> cut_pieces(const BamPlan &pl, int64_t piece_bytes) {
    const std::vector<Member> &members = pl.members;
    const std::vector<BamPlan::Run> &runs = pl.runs;
    const std::vector<uint32_t> &run_of = pl.member_run;
    const int nm = pl.nm();
    std::vector<ImagePiece> pieces;
    int64_t byte0 = 0;
    for (int m0 = 0; m0 < nm;) {
        int m1 = m0;
        int64_t byte1 = byte0;
        while (m1 < nm && (byte1 - byte0 < piece_bytes || m1 == m0)) {
            byte1 = (int64_t)(members[(size_t)m1].coff + members[(size_t)m1].clen);
            ++m1;
        }
        if (m1 == nm) byte1 = pl.image_bytes;
        else if (run_of[(size_t)m1] != run_of[(size_t)m1 - 1]) byte1 = runs[run_of[(size_t)m1]].dev_lo;   // (the rest of the run before)
        const BamPlan::Run &r0 = runs[run_of[(size_t)m0]];
        pieces.push_back(ImagePiece{m0, m1, byte0, byte1, byte1 <= r0.dev_lo + (r0.file_hi - r0.file_lo)});
        byte0 = byte1;
        m0 = m1;
    }
    return pieces;
}

// where the bytes of a piece that lies in one run are in the file
inline const uint8_t *piece_source(const uint8_t *image, const BamPlan &pl, const ImagePiece &pc) {
    const BamPlan::Run &r0 = pl.runs[pl.member_run[(size_t)pc.m0]];
    return image + (r0.file_lo - r0.dev_lo) + pc.byte0;
}

// bytes [lo, hi) of the image on the device, from the file, to dst: run by run (the file's bytes of run r start at
// r.file_lo - r.dev_lo before its offsets in the image on the device)
inline void copy_image(const uint8_t *image, const std::vector<BamPlan::Run> &runs, uint8_t *dst, int64_t lo, int64_t hi) {
    auto it = std::upper_bound(runs.begin(), runs.end(), lo, [](int64_t x, const BamPlan::Run &r) { return x < r.dev_lo; });
    for (size_t r = (size_t)(it - runs.begin()) - 1; r < runs.size() && lo < hi; ++r) {
        const int64_t rhi = std::min(hi, runs[r].dev_lo + (runs[r].file_hi - runs[r].file_lo));
        if (rhi > lo) std::memcpy(dst, image + (runs[r].file_lo - runs[r].dev_lo) + lo, (size_t)(rhi - lo));
        dst += std::max<int64_t>(rhi - lo, 0);
        lo = std::max(lo, rhi);
    }
}

// ---- phase 4: the record chains.  A region read chains every run from its first chunk's start to its last chunk's end:
// bounds[2 r], bounds[2 r + 1] in the inflated stream (a run without a chunk -- the header's -- has no record: both at its end).
inline int run_bounds(const BamPlan &pl, uint64_t first_record, std::vector<uint64_t> &bounds) {
    const std::vector<BamPlan::Run> &runs = pl.runs;
    bounds.assign(2 * std::max<size_t>(runs.size(), 1), ~0ull);
    for (const BamPlan::ChunkAt &c : pl.chunk_at) {
        const uint64_t a = pl.uoff_of(c.s_idx) + c.ub, z = pl.uoff_of(c.e_idx) + c.ue;
        if (a < first_record || z < a || z > pl.total_u) return kChunkInHeader;
        // (the run that holds the chunk's first member; runs ascend by file offset)
        auto it = std::upper_bound(runs.begin(), runs.end(), c.cb, [](int64_t x, const BamPlan::Run &r) { return x < r.file_lo; });
        const size_t r = (size_t)(it - runs.begin()) - 1;
        if (bounds[2 * r] == ~0ull) bounds[2 * r] = a;
        bounds[2 * r + 1] = z;
    }
    for (size_t r = 0; r < runs.size(); ++r)
        if (bounds[2 * r] == ~0ull) bounds[2 * r] = bounds[2 * r + 1] = pl.uoff_of(runs[r].m1);
    return kOk;
}

// What the host knows of the chains between two rounds: the record start the next member has to confirm, the run it
// belongs to (region reads), and the records of every member settled so far.
struct ChainState {
    uint32_t cur_run = 0;
    uint64_t expected = 0;
    std::vector<uint32_t> nrec_of;
    // `bounds`: run_bounds of a region read; nullptr: a whole-file read, one chain from the header's end
    ChainState(const BamPlan &pl, const std::vector<uint64_t> *bounds, uint64_t first_record)
        : cur_run(bounds ? pl.member_run[0] : 0u), expected(bounds ? (*bounds)[2 * (size_t)cur_run] : first_record), nrec_of((size_t)pl.nm(), 0u) {}
};
// kSettled: every walk chains and ends where it has to.  kRedo: member m guessed wrong (or not at all) and walks again
// from `forced`.  kTruncated (whole-file reads): member m met a length prefix that cannot be, or (m = nm) the last record
// stops short of or runs past the end of the stream.  kInsideRecord (region reads): a chunk ends inside a record.
enum SettleKind { kSettled = 0, kRedo = 1, kTruncated = 2, kInsideRecord = 3 };
struct Settle { SettleKind kind; int m; uint64_t forced; };
// One round: the members from `from` on, whose walks `chain` holds as the device left them, against the state.
inline Settle settle_round(const BamPlan &pl, const std::vector<uint64_t> *bounds, const MemberChain *chain, int from, ChainState &s) {
    const int nm = pl.nm();
    for (int m = from; m < nm; ++m) {
        if (bounds && pl.member_run[(size_t)m] != s.cur_run) {   // each run settles from its forced start and has to end exactly at its stop
            if (s.expected != (*bounds)[2 * (size_t)s.cur_run + 1]) return {kInsideRecord, m, 0};
            s.cur_run = pl.member_run[(size_t)m];
            s.expected = (*bounds)[2 * (size_t)s.cur_run];
        }
        const uint64_t stop_m = bounds ? (*bounds)[2 * (size_t)s.cur_run + 1] : pl.total_u;
        const uint64_t begin = pl.members[(size_t)m].uoff, end = std::min<uint64_t>(begin + pl.members[(size_t)m].ulen, stop_m);
        s.nrec_of[(size_t)m] = 0;
        if (s.expected >= end) continue;                        // no record starts in this member (or it lies behind its run's last chunk)
        const MemberChain &mc = chain[(size_t)m];
        if (mc.first != s.expected) return {kRedo, m, s.expected};   // the guess was off (or there was none): walk again from the right place
        s.nrec_of[(size_t)m] = mc.nrec;
        if (mc.flags & 2u) return {bounds ? kInsideRecord : kTruncated, m, 0};   // a length prefix that cannot be: the walk ends here
        s.expected = mc.next;
    }
    const uint64_t stop_at = bounds ? (*bounds)[2 * (size_t)s.cur_run + 1] : pl.total_u;
    if (s.expected != stop_at) return {bounds ? kInsideRecord : kTruncated, nm, 0};   // the last record runs past (or stops short of) the end
    return {kSettled, nm, 0};
}

// records before each member (nm + 1 entries)
inline std::vector<uint64_t> record_bases(const std::vector<uint32_t> &nrec_of) {
    std::vector<uint64_t> rec_base(nrec_of.size() + 1, 0);
    for (size_t m = 0; m < nrec_of.size(); ++m) rec_base[m + 1] = rec_base[m] + nrec_of[m];
    return rec_base;
}

// ---- phase 5: the member of every 256th record (k_bam_fields and its kin walk forward from there)
inline std::vector<uint32_t> group_members(const std::vector<uint64_t> &rec_base, int64_t nrec, int nm) {
    std::vector<uint32_t> rec_member((size_t)((nrec + 255) >> 8));
    int m = 0;
    for (size_t g = 0; g < rec_member.size(); ++g) {
        const uint64_t i = (uint64_t)g << 8;
        while (m + 1 < nm && rec_base[(size_t)m + 1] <= i) ++m;
        rec_member[g] = (uint32_t)m;
    }
    return rec_member;
}

// The wide-record list, collected in file order, in ascending staged order (after a sort that moved records).
inline void order_wide_list(std::vector<int64_t> &idx, std::vector<int32_t> &alen, std::vector<int32_t> &nblk) {
    std::vector<size_t> by(idx.size());
    std::iota(by.begin(), by.end(), (size_t)0);
    std::sort(by.begin(), by.end(), [&](size_t x, size_t y) { return idx[x] < idx[y]; });
    const std::vector<int64_t> wi = idx;
    const std::vector<int32_t> wa = alen, wn = nblk;
    for (size_t k = 0; k < by.size(); ++k) { idx[k] = wi[by[k]]; alen[k] = wa[by[k]]; nblk[k] = wn[by[k]]; }
}

// ---- the index build.  Where bgzf_tell places a stream position (bgzf.c:569-572): per member, the file offset of the
// first gzip header whose payload begins where the member's does -- an empty member in front of it, if there is one -- and
// of its own header; the end of the stream lies in the first member behind the last payload (the EOF block), or at the end
// of the file.  Two entries per member plus the end's two.
inline std::vector<uint64_t> tell_table(const std::vector<Member> &members, int64_t size) {
    const size_t nm = members.size();
    std::vector<uint64_t> blk(2 * nm + 2);
    uint64_t prev_end = 0;
    for (size_t m = 0; m < nm; ++m) {
        const uint64_t own = members[m].coff - members[m].hdr;
        blk[2 * m] = std::min(prev_end, own); blk[2 * m + 1] = own;
        prev_end = members[m].coff + members[m].clen + 8;
    }
    blk[2 * nm] = blk[2 * nm + 1] = std::min<uint64_t>(prev_end, (uint64_t)size);
    return blk;
}

// key bits the radix sort of the index runs looks at: the bin below, then as many bits as the reference ids take
inline int index_key_bits(uint64_t n_ref) {
    int key_bits = 32;
    while (key_bits < 64 && (n_ref >> (key_bits - 32))) ++key_bits;
    return key_bits;
}

} // namespace pcbamhost
