// bam_stager.cpp -- native BAM -> packed-array stager (host side, no GPU code).
//
// The step *before* the counting path: the reference gets its reads from pysam/htslib
// (`pysam.AlignmentFile(X, "rb")`, `.fetch`, `read.positions`, `read.is_reverse`, `.mapped`;
// plastid/genomics/genome_array.py:660, 669, 690, 800-815).  pysam is not part of this
// product; this file reads a coordinate-sorted BAM (SAM/BAM spec v1: BGZF blocks, BAM
// records) straight into the flat arrays `pc_add_alignment_file` stages to HBM:
//   tid, pos, alen (= number of M/=/X reference positions), flags (bit0 = reverse strand),
//   nblk (maximal runs of contiguous aligned positions), runs of the gapped records.
// BGZF members are independent, so they are inflated (and the records in them decoded) by a pool of threads.
//
// C ABI (ctypes: plastid_amd/_hostlib.py, which lists every pb_* function of this file and of host_shims.h):
//   pb_open / pb_open_indexed / pb_close, pb_nref / pb_ref_name / pb_ref_length,
//   pb_load  (decode the whole file), pb_counts, pb_fill (copy into caller arrays)
#include <dlfcn.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <chrono>
#include <mutex>
#include <thread>
#include <fcntl.h>
#include <functional>
#include <sched.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

#include "bam_host.h"
#include "index_shape.h"
#include "sam_host.h"

namespace {

thread_local std::string g_err;
int fail(const std::string &m) {
    g_err = m;
    return -1;
}

namespace bh = pcbamhost;   // the member and header parsers both decoders use

struct Block {
    size_t coff;   // offset of the gzip member in the file
    uint32_t clen; // compressed member length
    uint32_t ulen; // uncompressed length (ISIZE)
    size_t uoff;   // offset in the inflated stream
    uint32_t hdr;  // bytes of its gzip header (0: the member has no room for header and trailer)
};

// Records decoded from one contiguous piece of the inflated stream (the pieces are decoded in
// parallel and stitched in file order).
struct Part {
    // the columns: n records, nrun runs of the gapped ones, held by the load's Arena
    int32_t *tid = nullptr, *pos = nullptr, *blk_start = nullptr, *blk_len = nullptr;
    uint16_t *alen = nullptr;
    uint8_t *flags = nullptr, *nblk = nullptr;
    // what a read filter may look at beyond strand and length (genome_array.py:697-722: filters take the pysam read):
    // the SAM FLAG word, MAPQ and l_seq (pysam's query_length) of every staged record
    uint16_t *flag16 = nullptr;
    uint8_t *mapq = nullptr;
    int32_t *lseq = nullptr;
    // ... and the NH:i tag (number of reported alignments of the query; `read.get_tag("NH") == 1` is the usual unique-mapper
    // filter): its value clamped to 65 535, 0 when the record carries none
    uint16_t *nh = nullptr;
    size_t n = 0, nrun = 0;
    int64_t mapped = 0, unplaced = 0, total = 0;
    // wide records of the piece (more than 65 535 aligned positions or more than 255 aligned runs: markers 65535 / 255 in
    // the packed columns, true values here): record index within the piece, aligned length, run count
    std::vector<int64_t> wide_idx;
    std::vector<int32_t> wide_alen, wide_nblk;
    // first defect found inside the piece: record index within the piece, message; `before_order` marks
    // the checks the serial walk makes before it looks at the sort order of a record
    int64_t err_rec = INT64_MAX;
    bool err_before_order = false;
    std::string err;
    // what the stitching needs to know about the piece
    bool any_placed = false, saw_unplaced = false;
    int64_t first_placed_rec = -1;
    int32_t first_tid = -1, first_pos = -1, first_spos = -1;
    int32_t last_tid = -1, last_pos = -1, last_spos = -1;
    bool bad_size = false;            // decode_span stopped at a length prefix below the fixed record size
    // pb_load_sorted only: the POS field of every staged record (the sort key; `pos` holds the first aligned position), its
    // record number within the piece (all records counted), and the number of the piece's first unplaced record
    int32_t *rpos = nullptr, *rno = nullptr;
    int64_t first_unplaced_rec = -1;
};

// Column storage of one load: 64 MiB anonymous mappings (on huge pages where the host grants them), handed
// out by bumping a pointer.  Thousands of per-piece vectors cost more in mmap/munmap and page faults than
// the decoding itself.  Regions released by a closed file wait in a process-wide pool (at most PB_POOL_MB,
// default 2048) for the next load -- several BAM files are the normal case -- which then neither faults
// them in again nor unmaps them.
struct RegionPool {
    static constexpr size_t kRegion = (size_t)64 << 20;
    std::mutex mu;
    std::vector<void *> idle;
    size_t cap = 2048;   // MiB
    RegionPool() { if (const char *env = getenv("PB_POOL_MB")) cap = (size_t)std::max(0, atoi(env)); }
    ~RegionPool() { for (void *q : idle) munmap(q, kRegion); }
    void *get() {
        {
            std::lock_guard<std::mutex> lock(mu);
            if (!idle.empty()) { void *q = idle.back(); idle.pop_back(); return q; }
        }
        void *q = mmap(nullptr, kRegion, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (q == MAP_FAILED) return nullptr;
        (void)madvise(q, kRegion, MADV_HUGEPAGE);
        return q;
    }
    void put(void *q) {
        {
            std::lock_guard<std::mutex> lock(mu);
            if ((idle.size() + 1) * (kRegion >> 20) <= cap) { idle.push_back(q); return; }
        }
        munmap(q, kRegion);
    }
};
RegionPool &region_pool() {
    static RegionPool pool;
    return pool;
}

struct Arena {
    std::mutex mu;
    std::vector<std::pair<void *, size_t>> regions;
    uint8_t *cur = nullptr;
    size_t left = 0;
    void *alloc(size_t bytes) {
        bytes = (bytes + 63) & ~(size_t)63;
        std::lock_guard<std::mutex> lock(mu);
        if (bytes > left) {
            void *q;
            size_t sz = RegionPool::kRegion;
            if (bytes <= sz) {
                q = region_pool().get();
            } else {                                      // an outsize piece gets a mapping of its own
                sz = (bytes + 4095) & ~(size_t)4095;
                q = mmap(nullptr, sz, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
                if (q == MAP_FAILED) q = nullptr;
            }
            if (!q) return nullptr;
            regions.emplace_back(q, sz);
            cur = (uint8_t *)q;
            left = sz;
        }
        void *r = cur;
        cur += bytes;
        left -= bytes;
        return r;
    }
    void clear() {
        for (auto &r : regions) {
            if (r.second == RegionPool::kRegion) region_pool().put(r.first);
            else munmap(r.first, r.second);
        }
        regions.clear();
        cur = nullptr;
        left = 0;
    }
    ~Arena() { clear(); }
};

// The records of the piece being decoded (scratch: reused from piece to piece, so it stays in cache; the
// finished columns are copied into the Arena at their exact size).
struct Cols {
    std::vector<int32_t> tid, pos, blk_start, blk_len;
    std::vector<uint16_t> alen, flag16, nh;
    std::vector<uint8_t> flags, nblk, mapq;
    std::vector<int32_t> lseq;
    std::vector<int32_t> rpos, rno;   // (pb_load_sorted: see Part)
    size_t n = 0;   // records held: the five per-record columns are sized for the piece up front and written by index
    void clear() { n = 0; blk_start.clear(); blk_len.clear(); }
    void room(size_t records) {
        if (tid.size() < records) { tid.resize(records); pos.resize(records); alen.resize(records); flags.resize(records); nblk.resize(records);
                                      flag16.resize(records); mapq.resize(records); lseq.resize(records); nh.resize(records); }
    }
    void room_sorted(size_t records) { if (rpos.size() < records) { rpos.resize(records); rno.resize(records); } }
};

struct Bam {
    std::string path;
    std::string index_path;   // pb_open_indexed: the index file to use instead of path + ".bai" / stem + ".bai"
    Arena arena;
    std::vector<std::string> ref_names;
    std::vector<int32_t> ref_lengths;
    std::vector<Part> parts;          // decoded records, in file order
    std::vector<size_t> rec_off, run_off; // where each part starts in the flat arrays
    int64_t mapped = 0, unplaced = 0, total = 0;
    size_t nrec = 0, nrun = 0;
    int threads = 1;
    bool loaded = false;
    // pb_load_sorted: the decode leaves the checks between records out (`sorting`); perm[k] = the flat (file order) index of
    // the record staged at k, empty when no record moved; file_order[k] = its record number in the file
    bool sorting = false, sort_requested = false, sorted_input = true;
    int64_t moved = 0;
    std::vector<uint32_t> perm;
    std::vector<int64_t> file_order;
    bool is_sam = false;   // pb_open_sam: the file is SAM text (decode_sam reads it)
};

bool read_file(const std::string &path, std::vector<uint8_t> &buf) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    buf.resize((size_t)n);
    size_t got = n > 0 ? fread(buf.data(), 1, (size_t)n, f) : 0;
    fclose(f);
    return got == (size_t)n;
}

inline uint16_t rd16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// index the BGZF members (RFC 1952 gzip header with the 'BC' extra subfield carrying BSIZE)
// a read-only view of a whole file (mapped: the inflate threads read the page cache directly)
struct FileMap {
    const uint8_t *p = nullptr;
    size_t n = 0;
    bool ok = false;
    explicit FileMap(const std::string &path) {
        const int fd = open(path.c_str(), O_RDONLY);
        if (fd < 0) return;
        struct stat st;
        if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) {
            n = (size_t)st.st_size;
            if (n == 0) ok = true;
            else {
                void *q = mmap(nullptr, n, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0);
                if (q != MAP_FAILED) { p = (const uint8_t *)q; ok = true; }
            }
        }
        close(fd);
    }
    ~FileMap() { if (p) munmap(const_cast<uint8_t *>(p), n); }
    const uint8_t *data() const { return p; }
    size_t size() const { return n; }
};

int scan_blocks(const FileMap &file, std::vector<Block> &blocks, size_t &total_u) {
    total_u = 0;
    for (int64_t off = 0, clen = 0; off < (int64_t)file.size(); off += clen) {
        bh::Member mb;
        mb.hdr = 0;
        const int code = bh::parse_member(file.data(), (int64_t)file.size(), off, mb, clen);
        if (code && code != bh::kMemberTiny) return fail(bh::defect_text(code));   // (kMemberTiny: inflate_block refuses it)
        blocks.push_back({(size_t)off, (uint32_t)clen, mb.ulen, total_u, mb.hdr});
        total_u += mb.ulen;
    }
    return 0;
}

// libdeflate, when the host has it (looked up at run time; nothing links against it): its raw-deflate
// decoder and its carry-less-multiply CRC-32 are several times faster than zlib 1.2's.  PB_ZLIB=1 keeps
// to zlib.  One decompressor per thread.
struct LibDeflate {
    void *(*alloc)() = nullptr;
    int (*decompress)(void *, const void *, size_t, void *, size_t, size_t *) = nullptr;
    void (*release)(void *) = nullptr;
    uint32_t (*crc32)(uint32_t, const void *, size_t) = nullptr;
    bool ok = false;
    LibDeflate() {
        void *h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        alloc = reinterpret_cast<decltype(alloc)>(dlsym(h, "libdeflate_alloc_decompressor"));
        decompress = reinterpret_cast<decltype(decompress)>(dlsym(h, "libdeflate_deflate_decompress"));
        release = reinterpret_cast<decltype(release)>(dlsym(h, "libdeflate_free_decompressor"));
        crc32 = reinterpret_cast<decltype(crc32)>(dlsym(h, "libdeflate_crc32"));
        ok = alloc && decompress && release && crc32;
    }
};
const LibDeflate &libdeflate() {
    static const LibDeflate ld;
    return ld;
}
struct ThreadDecompressor {
    void *d = nullptr;
    ~ThreadDecompressor() { if (d) libdeflate().release(d); }
};

// raw deflate stream -> exactly `out_n` bytes with CRC-32 `crc`; 0, -1 (damaged stream) or -2 (CRC)
int raw_inflate(const uint8_t *in, size_t in_n, uint8_t *out, size_t out_n, uint32_t crc) {
    const LibDeflate &ld = libdeflate();
    if (ld.ok && getenv("PB_ZLIB") == nullptr) {
        thread_local ThreadDecompressor td;
        if (!td.d) td.d = ld.alloc();
        if (td.d) {
            if (ld.decompress(td.d, in, in_n, out, out_n, nullptr) != 0) return -1;
            return ld.crc32(0, out, out_n) == crc ? 0 : -2;
        }
    }
    z_stream zs;
    std::memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) return -1;
    zs.next_in = const_cast<uint8_t *>(in);
    zs.avail_in = (uInt)in_n;
    zs.next_out = out;
    zs.avail_out = (uInt)out_n;
    const int rc = inflate(&zs, Z_FINISH);
    inflateEnd(&zs);
    if (rc != Z_STREAM_END || zs.avail_out != 0) return -1;
    return (uint32_t)::crc32(::crc32(0L, Z_NULL, 0), out, (uInt)out_n) == crc ? 0 : -2;
}

int inflate_block(const FileMap &file, const Block &b, uint8_t *dst) {
    if (b.ulen == 0) return 0;
    const uint8_t *h = file.data() + b.coff;
    if (!b.hdr) return -1;
    return raw_inflate(h + b.hdr, b.clen - b.hdr - 8, dst, b.ulen, rd32(h + b.clen - 8));
}

// PB_TIMING=1: print the phases of a load to stderr
struct Lap {
    bool on = getenv("PB_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void operator()(const char *what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[bam] %-24s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

// BAM header (magic, text, reference list) at `p`; leaves `p` at the first alignment record.
// need_more (optional): set when the buffer ends inside the header (a caller that inflates lazily
// fetches more and retries) instead of reporting truncation.
int parse_header(Bam &bam, const uint8_t *&p, const uint8_t *end, uint32_t &n_ref_out, bool *need_more = nullptr) {
    bh::BamHeader h;
    const bh::HeaderParse hp = bh::parse_bam_header(p, (size_t)(end - p), h);
    if (hp.status == bh::kHeaderMore && need_more) { *need_more = true; return -1; }
    if (hp.status != bh::kHeaderOk) return fail(hp.text);
    bam.ref_names = std::move(h.ref_names);
    bam.ref_lengths = std::move(h.ref_lengths);
    n_ref_out = h.n_ref;
    p += h.first_record;
    return 0;
}

// Decodes the records that start at `q` and lie wholly inside [q, limit), at most `max_rec` of them, into
// `pt` with every per-record format check and the order checks inside the piece.  Returns where it
// stopped: `limit`, the start of the first record that crosses `limit`, or the record whose length
// prefix is impossible (pt.bad_size).  A defect ends the piece (pt.err, pt.err_rec).
// NH:i of a record: the auxiliary fields follow the packed sequence ((l_seq + 1) / 2 bytes) and the qualities (l_seq bytes)
// behind the CIGAR; each is {tag[2], type, value} (SAM spec 4.2.4; walked as htslib's bam_aux_get does, sam.c:915-965 in the
// vendored tree: A c C one byte, s S two, i I f four, Z H NUL-terminated, B {subtype, count:u32, elements}).  The value of
// an integer-typed NH, clamped to [0, 65 535]; 0 when the record has no such field (or the fields are malformed).
static inline uint16_t aux_nh(const uint8_t *after_cigar, int32_t l_seq, const uint8_t *end) {
    if (l_seq < 0) return 0;
    const uint8_t *a = after_cigar + ((size_t)l_seq + 1) / 2 + (size_t)l_seq;
    while (a + 3 <= end && a >= after_cigar) {
        const uint8_t t0 = a[0], t1 = a[1], type = a[2];
        a += 3;
        size_t sz;
        switch (type) {
        case 'A': case 'c': case 'C': sz = 1; break;
        case 's': case 'S': sz = 2; break;
        case 'i': case 'I': case 'f': sz = 4; break;
        case 'Z': case 'H': { const uint8_t *z = a; while (z < end && *z) ++z; if (z >= end) return 0; sz = (size_t)(z - a) + 1; break; }
        case 'B': {
            if (a + 5 > end) return 0;
            const uint8_t sub = a[0];
            const uint32_t cnt = rd32(a + 1);
            const size_t es = (sub == 'c' || sub == 'C') ? 1 : ((sub == 's' || sub == 'S') ? 2 : ((sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0));
            if (!es) return 0;
            sz = 5 + (size_t)cnt * es;
            break;
        }
        default: return 0;
        }
        if ((size_t)(end - a) < sz) return 0;
        if (t0 == 'N' && t1 == 'H') {
            int64_t v;
            switch (type) {
            case 'c': v = (int8_t)a[0]; break;
            case 'C': v = a[0]; break;
            case 's': v = (int16_t)rd16(a); break;
            case 'S': v = rd16(a); break;
            case 'i': v = (int32_t)rd32(a); break;
            case 'I': v = rd32(a); break;
            default: return 0;
            }
            return (uint16_t)(v < 0 ? 0 : (v > 65535 ? 65535 : v));
        }
        a += sz;
    }
    return 0;
}

// kSort (pb_load_sorted): no check between a record and the one in front (the file may be in any order); POS and the
// record number of every staged record are kept for the sort.
template <bool kSort>
const uint8_t *decode_span_cols(const Bam &bam, Part &pt, Cols &cols, const uint8_t *q, const uint8_t *limit, uint32_t n_ref, int64_t max_rec) {
    std::vector<std::pair<int32_t, int32_t>> runs;
    cols.clear();
    cols.room(limit > q ? (size_t)(limit - q) / 36 + 1 : 1);   // a record takes at least 36 bytes
    if (kSort) cols.room_sorted(limit > q ? (size_t)(limit - q) / 36 + 1 : 1);
    int32_t *const c_rpos = cols.rpos.data(), *const c_rno = cols.rno.data();
    // the state every record touches lives in locals (the columns are int32 / uint8 arrays: through `pt` and `cols`
    // the compiler has to assume that every store may change them) and is written back on the way out
    int32_t *const c_tid = cols.tid.data(), *const c_pos = cols.pos.data();
    uint16_t *const c_alen = cols.alen.data();
    uint8_t *const c_flags = cols.flags.data(), *const c_nblk = cols.nblk.data(), *const c_mapq = cols.mapq.data();
    uint16_t *const c_flag16 = cols.flag16.data();
    int32_t *const c_lseq = cols.lseq.data();
    uint16_t *const c_nh = cols.nh.data();
    size_t n = 0;
    int64_t total = pt.total, mapped = pt.mapped, unplaced = pt.unplaced;
    bool any_placed = pt.any_placed, saw_unplaced = pt.saw_unplaced;
    int32_t last_tid = pt.last_tid, last_pos = pt.last_pos, last_spos = pt.last_spos;
    const uint8_t *ret = nullptr;
    auto bad = [&](int64_t i, bool before_order, const std::string &m) {
        pt.err_rec = i; pt.err_before_order = before_order; pt.err = m;
        return q;
    };
    for (int64_t i = 0; i < max_rec; ++i) {
        if (limit - q < 4) break;
        const uint32_t block_size = rd32(q);
        if (block_size < 32) { pt.bad_size = true; break; }
        if ((size_t)(limit - q - 4) < block_size) break;
        const uint8_t *r = q + 4;
        q = r + block_size;
        const int32_t tid = (int32_t)rd32(r), pos = (int32_t)rd32(r + 4);
        const uint8_t l_read_name = r[8], mapq = r[9];
        const uint16_t n_cigar = rd16(r + 12), flag = rd16(r + 14);
        const int32_t l_seq = (int32_t)rd32(r + 16);
        total += 1;
        if (!(flag & 0x4)) mapped += 1;
        if (tid < 0) { // unplaced reads sit at the end of a sorted BAM; fetch() never returns them
            unplaced += 1;
            if (kSort && !saw_unplaced) pt.first_unplaced_rec = i;
            saw_unplaced = true;
            continue;
        }
        if (tid >= (int32_t)n_ref) { ret = bad(i, true, "BAM record with reference id out of range"); break; }
        if (pos < 0) { ret = bad(i, true, "placed BAM record with a negative position"); break; }
        if (kSort) {
            any_placed = true;
            c_rpos[n] = pos; c_rno[n] = (int32_t)i;
        } else if (!any_placed) {        // its order against the previous piece is checked when stitching
            any_placed = true;
            pt.first_placed_rec = i;
            pt.first_tid = tid; pt.first_pos = pos;
            if (saw_unplaced) { ret = bad(i, false, "BAM file is not coordinate sorted: " + bam.path); break; }
        } else if (saw_unplaced || tid < last_tid || (tid == last_tid && pos < last_pos)) {
            ret = bad(i, false, "BAM file is not coordinate sorted: " + bam.path);
            break;
        }
        const bool first = n == 0;
        if ((size_t)32 + l_read_name + (size_t)n_cigar * 4 > block_size) { ret = bad(i, false, "corrupt BAM record (cigar overruns block)"); break; }
        const uint8_t *cig = r + 32 + l_read_name;
        const uint16_t nh = aux_nh(cig + (size_t)n_cigar * 4, l_seq, q);
        if (n_cigar == 1) {   // the common record: one M / = / X operation (one aligned run starting at pos)
            const uint32_t v = rd32(cig), op = v & 0xf, len = v >> 4;
            if ((op == 0 || op == 7 || op == 8) && len > 0 && len <= 65535 && (int64_t)pos + len <= 0x7fffffffLL) {
                if (first) pt.first_spos = pos;
                else if (!kSort && last_tid == tid && last_spos > pos) {
                    ret = bad(i, false, "alignment starting with a deletion breaks coordinate order; not supported");
                    break;
                }
                last_tid = tid; last_pos = pos; last_spos = pos;
                c_tid[n] = tid;
                c_pos[n] = pos;
                c_alen[n] = (uint16_t)len;
                c_flags[n] = (flag & 0x10) ? 1 : 0;
                c_nblk[n] = 1;
                c_flag16[n] = flag; c_mapq[n] = mapq; c_lseq[n] = l_seq; c_nh[n] = nh;
                ++n;
                continue;
            }
        }
        runs.clear();
        int64_t ref = pos, L = 0;
        bool unknown_op = false;
        for (uint16_t c = 0; c < n_cigar && !unknown_op; ++c) {
            const uint32_t v = rd32(cig + 4 * c);
            const uint32_t op = v & 0xf, len = v >> 4;
            switch (op) {
            case 0: case 7: case 8: // M = X : aligned positions
                if (len) {
                    if (!runs.empty() && (int64_t)runs.back().first + runs.back().second == ref) runs.back().second += (int32_t)len;
                    else runs.emplace_back((int32_t)ref, (int32_t)len);
                    ref += len;
                    L += len;
                }
                break;
            case 2: case 3: // D N : reference only
                ref += len;
                break;
            case 1: case 4: case 5: case 6: // I S H P
                break;
            default:
                unknown_op = true;
                break;
            }
        }
        if (unknown_op) { ret = bad(i, false, "unknown CIGAR operation in " + bam.path); break; }
        if (ref > 0x7fffffffLL) { ret = bad(i, false, "alignment ends beyond 2^31 - 1"); break; }   // run starts are int32
        if (L > 0x7fffffffLL) { ret = bad(i, false, "alignment with more than 2^31 - 1 aligned positions"); break; }
        // beyond the 16-bit / 8-bit columns (or equal to both markers): a wide record, its true values aside
        const bool wide = L > 65535 || runs.size() > 255 || (L == 65535 && runs.size() == 255);
        if (wide) { pt.wide_idx.push_back((int64_t)n); pt.wide_alen.push_back((int32_t)L); pt.wide_nblk.push_back((int32_t)runs.size()); }
        // the packed format keys a record on its first aligned position; a CIGAR that opens with
        // D/N (not produced by aligners) is accepted only if that keeps the file order
        const int32_t spos = runs.empty() ? pos : runs[0].first;
        if (first) pt.first_spos = spos;
        else if (!kSort && last_tid == tid && last_spos > spos) {
            ret = bad(i, false, "alignment starting with a deletion breaks coordinate order; not supported");
            break;
        }
        last_tid = tid; last_pos = pos; last_spos = spos;
        c_tid[n] = tid;
        c_pos[n] = spos;
        c_alen[n] = wide ? (uint16_t)65535 : (uint16_t)L;
        c_flags[n] = (flag & 0x10) ? 1 : 0;
        c_nblk[n] = wide ? (uint8_t)255 : (uint8_t)runs.size();
        c_flag16[n] = flag; c_mapq[n] = mapq; c_lseq[n] = l_seq; c_nh[n] = nh;
        ++n;
        if (runs.size() >= 2)
            for (auto &x : runs) {
                cols.blk_start.push_back(x.first);
                cols.blk_len.push_back(x.second);
            }
    }
    cols.n = n;
    pt.total = total; pt.mapped = mapped; pt.unplaced = unplaced;
    pt.any_placed = any_placed; pt.saw_unplaced = saw_unplaced;
    pt.last_tid = last_tid; pt.last_pos = last_pos; pt.last_spos = last_spos;
    return ret ? ret : q;
}

void keep_columns(Bam &bam, Part &pt, const Cols &cols);
const uint8_t *decode_span(Bam &bam, Part &pt, const uint8_t *q, const uint8_t *limit, uint32_t n_ref, int64_t max_rec) {
    thread_local Cols cols;
    const uint8_t *stop = bam.sorting ? decode_span_cols<true>(bam, pt, cols, q, limit, n_ref, max_rec) : decode_span_cols<false>(bam, pt, cols, q, limit, n_ref, max_rec);
    keep_columns(bam, pt, cols);
    return stop;
}

// the finished columns of a piece, at their exact size, into the load's arena
void keep_columns(Bam &bam, Part &pt, const Cols &cols) {
    const size_t n = cols.n, m = cols.blk_start.size();
    if (n) {
        uint8_t *mem = (uint8_t *)bam.arena.alloc(n * 21 + 64 * 9 + m * 8 + 64 * 2 + (bam.sorting ? n * 8 + 64 * 2 : 0));
        if (!mem) {
            if (pt.err_rec == INT64_MAX) { pt.err_rec = 0; pt.err_before_order = true; pt.err = "out of memory reading " + bam.path; }
            return;
        }
        auto take = [&](size_t bytes) { uint8_t *r = mem; mem += (bytes + 63) & ~(size_t)63; return r; };
        pt.tid = (int32_t *)take(n * 4); pt.pos = (int32_t *)take(n * 4); pt.alen = (uint16_t *)take(n * 2);
        pt.flags = take(n); pt.nblk = take(n);
        std::memcpy(pt.tid, cols.tid.data(), n * 4); std::memcpy(pt.pos, cols.pos.data(), n * 4);
        std::memcpy(pt.alen, cols.alen.data(), n * 2); std::memcpy(pt.flags, cols.flags.data(), n); std::memcpy(pt.nblk, cols.nblk.data(), n);
        pt.flag16 = (uint16_t *)take(n * 2); pt.mapq = take(n); pt.lseq = (int32_t *)take(n * 4);
        std::memcpy(pt.flag16, cols.flag16.data(), n * 2); std::memcpy(pt.mapq, cols.mapq.data(), n); std::memcpy(pt.lseq, cols.lseq.data(), n * 4);
        pt.nh = (uint16_t *)take(n * 2);
        std::memcpy(pt.nh, cols.nh.data(), n * 2);
        if (bam.sorting) {
            pt.rpos = (int32_t *)take(n * 4); pt.rno = (int32_t *)take(n * 4);
            std::memcpy(pt.rpos, cols.rpos.data(), n * 4); std::memcpy(pt.rno, cols.rno.data(), n * 4);
        }
        if (m) {
            pt.blk_start = (int32_t *)take(m * 4); pt.blk_len = (int32_t *)take(m * 4);
            std::memcpy(pt.blk_start, cols.blk_start.data(), m * 4); std::memcpy(pt.blk_len, cols.blk_len.data(), m * 4);
        }
    }
    pt.n = n;
    pt.nrun = m;
}

// The checks that span two pieces, and the flat offsets of every piece (bam.parts in file order).  The
// defect reported is the one of the lowest record index, as in a serial walk (where one record fails
// two checks, the serial order of the checks decides).
int stitch_parts(Bam &bam, bool truncated, int nthreads) {
    const size_t nparts = bam.parts.size();
    bool seen_unplaced = false, have_prev = false;
    int32_t prev_tid = -1, prev_pos = -1, prev_spos = -1;
    bam.rec_off.assign(nparts + 1, 0);
    bam.run_off.assign(nparts + 1, 0);
    for (size_t k = 0; k < nparts; ++k) {
        const Part &pt = bam.parts[k];
        int64_t at = INT64_MAX;
        std::string msg;
        if (pt.any_placed && !bam.sorting) {
            const int64_t f = pt.first_placed_rec;
            if (seen_unplaced || (have_prev && (pt.first_tid < prev_tid || (pt.first_tid == prev_tid && pt.first_pos < prev_pos)))) {
                at = f; msg = "BAM file is not coordinate sorted: " + bam.path;
            } else if (have_prev && prev_tid == pt.first_tid && prev_spos > pt.first_spos && pt.err_rec != f) {
                at = f; msg = "alignment starting with a deletion breaks coordinate order; not supported";
            }
        }
        if (pt.err_rec < at || (pt.err_rec == at && pt.err_before_order)) { at = pt.err_rec; msg = pt.err; }
        if (at != INT64_MAX) return fail(msg);
        if (pt.any_placed && pt.n > 0) { have_prev = true; prev_tid = pt.last_tid; prev_pos = pt.last_pos; prev_spos = pt.last_spos; }
        seen_unplaced |= pt.saw_unplaced;
        bam.mapped += pt.mapped; bam.unplaced += pt.unplaced; bam.total += pt.total;
        bam.rec_off[k + 1] = bam.rec_off[k] + pt.n;
        bam.run_off[k + 1] = bam.run_off[k] + pt.nrun;
    }
    if (truncated) return fail("truncated BAM record");
    bam.nrec = bam.rec_off[nparts];
    bam.nrun = bam.run_off[nparts];
    bam.threads = nthreads;
    return 0;
}

// Alignment records in [p, end) -> bam.parts (file order), with every order / format check.
int decode_records(Bam &bam, const uint8_t *p, const uint8_t *end, uint32_t n_ref, int nthreads, Lap &lap) {
    // A serial walk over the length prefixes cuts the stream into pieces of kPiece records; the pieces
    // are decoded by the thread pool and stitched.  (The region loader's path: its buffers are small.
    // Whole files go through decode(), which needs no serial walk.)
    int64_t kPiece = 1 << 16;
    if (const char *env = getenv("PB_PIECE")) kPiece = std::max(1, atoi(env));   // test knob: tiny pieces exercise the stitching
    std::vector<const uint8_t *> cuts;
    int64_t nwalk = 0;
    bool walk_truncated = false;
    {
        const uint8_t *q = p;
        while (q < end) {
            if (end - q < 4) { walk_truncated = true; break; }
            const uint32_t block_size = rd32(q);
            if ((size_t)(end - q - 4) < block_size || block_size < 32) { walk_truncated = true; break; }
            if (nwalk % kPiece == 0) cuts.push_back(q);
            q += 4 + (size_t)block_size;
            nwalk += 1;
        }
        cuts.push_back(q);
    }
    lap("walk records");
    const size_t nparts = cuts.size() - 1;
    bam.parts.assign(nparts, Part());
    {
        std::atomic<size_t> nextp(0);
        auto pworker = [&]() {
            for (;;) {
                const size_t k = nextp.fetch_add(1);
                if (k >= nparts) return;
                decode_span(bam, bam.parts[k], cuts[k], cuts[k + 1], n_ref, INT64_MAX);
            }
        };
        std::vector<std::thread> ppool;
        const int nt = (int)std::min<size_t>((size_t)nthreads, std::max<size_t>(nparts, 1));
        for (int t = 1; t < nt; ++t) ppool.emplace_back(pworker);
        pworker();
        for (auto &t : ppool) t.join();
    }
    lap("decode records");
    const int rc = stitch_parts(bam, walk_truncated, nthreads);
    lap("stitch");
    return rc;
}

// Where a record starts in [lo, hi), for a worker that holds a chunk of the inflated stream but not
// what precedes it: the first offset from which three records in a row look like BAM records (or
// fewer, when they reach the end of the chunk).  Only a guess -- decode() keeps what was decoded from
// it only if the preceding chunk's last record ends exactly there.
const uint8_t *guess_record_start(const uint8_t *lo, const uint8_t *hi, uint32_t n_ref) {
    auto plausible = [&](const uint8_t *q, const uint8_t *&next) {
        if (hi - q < 36) return false;
        const uint32_t bs = rd32(q);
        if (bs < 32 || bs > (1u << 26)) return false;
        const int32_t tid = (int32_t)rd32(q + 4), pos = (int32_t)rd32(q + 8);
        const uint32_t l_name = q[12], n_cigar = rd16(q + 16);
        const int32_t l_seq = (int32_t)rd32(q + 20), mtid = (int32_t)rd32(q + 24), mpos = (int32_t)rd32(q + 28);
        if (tid < -1 || tid >= (int32_t)n_ref || mtid < -1 || mtid >= (int32_t)n_ref || pos < -1 || mpos < -1) return false;
        if (l_name == 0 || l_seq < 0 || l_seq > (1 << 28)) return false;
        if ((uint64_t)32 + l_name + 4ull * n_cigar + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq > bs) return false;
        const uint8_t *nul = q + 36 + l_name - 1;
        if (nul < hi && *nul != 0) return false;
        next = q + 4 + (size_t)bs;
        return true;
    };
    const uint8_t *stop = hi - lo > (1 << 20) ? lo + (1 << 20) : hi;
    for (const uint8_t *q = lo; q < stop; ++q) {
        const uint8_t *a = q, *next = nullptr;
        int k = 0;
        while (k < 3 && plausible(a, next)) {
            ++k;
            if (next >= hi) { k = 3; break; }
            a = next;
        }
        if (k == 3) return q;
    }
    return nullptr;
}

// Whole file.  The BGZF members are grouped into chunks of about 1 MiB of inflated stream; a worker
// inflates a chunk into its own scratch buffer and, while it is still in its cache, decodes the
// records that start in it from a guessed record boundary (guess_record_start).  The inflated stream
// is never held as a whole: of each chunk only the first bytes and the bytes behind its last whole
// record are kept.  The serial pass that follows only chains the chunks: it confirms each guess
// against the end of the preceding chunk's last record (inflating and decoding the chunk again from
// the right offset where a guess was wrong), and decodes the one record that straddles each chunk
// boundary.  No pass walks the whole stream on one thread.  Positions are offsets in the inflated
// stream.
int decode(Bam &bam, int nthreads) {
    Lap lap;
    FileMap file(bam.path);
    if (!file.ok) return fail("cannot read " + bam.path);
    std::vector<Block> blocks;
    size_t total_u = 0;
    if (scan_blocks(file, blocks, total_u) != 0) return -1;
    lap("map + index members");
    auto inflate_error = [&](int rc) { return fail(std::string(rc == -2 ? "BGZF CRC mismatch in " : "BGZF inflate failed in ") + bam.path); };

    // ---- BAM header: inflate members from the start until it is complete
    uint32_t n_ref = 0;
    size_t pre = 0;                       // members inflated here
    std::vector<uint8_t> hbuf;
    size_t first_rec = 0;
    for (;;) {
        if (pre < blocks.size()) {
            hbuf.resize(blocks[pre].uoff + blocks[pre].ulen);
            const int rc = inflate_block(file, blocks[pre], hbuf.data() + blocks[pre].uoff);
            if (rc != 0) return inflate_error(rc);
            ++pre;
        }
        const uint8_t *p = hbuf.data();
        bool more = false;
        if (parse_header(bam, p, hbuf.data() + hbuf.size(), n_ref, pre < blocks.size() ? &more : nullptr) == 0) {
            first_rec = (size_t)(p - hbuf.data());
            break;
        }
        if (!more) return -1;
    }
    lap("header");

    // ---- chunks of members; chunk 0 = what the header pass inflated (its first record is known)
    size_t chunk_bytes = (size_t)1 << 20;
    if (const char *env = getenv("PB_CHUNK")) chunk_bytes = (size_t)std::max(1, atoi(env));   // test knob: tiny chunks exercise the chaining
    const size_t kNone = (size_t)-1;
    size_t kHead = (size_t)32 << 10;
    if (const char *env = getenv("PB_HEAD")) kHead = (size_t)std::max(0, atoi(env));            // test knob: records longer than a head
    struct Chunk {
        size_t b0, b1;                    // members
        size_t lo, hi;                    // its bytes of the inflated stream
        size_t guess, stop;               // where decoding started / stopped
        std::vector<uint8_t> head, tail;  // stream bytes [lo, lo + head.size()) and [stop, hi)
        Part part;
    };
    std::vector<Chunk> chunks;
    size_t max_chunk = 0;
    {
        Chunk c0;
        c0.b0 = 0; c0.b1 = pre; c0.lo = 0; c0.hi = hbuf.size();
        c0.guess = c0.stop = kNone;
        chunks.push_back(std::move(c0));
        for (size_t b = pre; b < blocks.size();) {
            Chunk c;
            c.b0 = b;
            size_t bytes = 0;
            while (b < blocks.size() && (bytes < chunk_bytes || blocks[b].ulen == 0)) bytes += blocks[b++].ulen;
            c.b1 = b;
            c.lo = blocks[c.b0].uoff;
            c.hi = c.lo + bytes;
            c.guess = c.stop = kNone;
            max_chunk = std::max(max_chunk, bytes);
            chunks.push_back(std::move(c));
        }
    }
    // chunk k inflated into buf (resized to its length)
    auto inflate_chunk = [&](const Chunk &c, std::vector<uint8_t> &buf) {
        buf.resize(c.hi - c.lo);
        for (size_t b = c.b0; b < c.b1; ++b) {
            const int rc = inflate_block(file, blocks[b], buf.data() + (blocks[b].uoff - c.lo));
            if (rc != 0) return rc;
        }
        return 0;
    };
    // decode chunk c, held in `base` (= stream offset c.lo), from stream offset `from`; keeps head and tail
    auto decode_chunk = [&](Chunk &c, const uint8_t *base, size_t from) {
        const size_t len = c.hi - c.lo;
        c.part = Part();
        const uint8_t *q = decode_span(bam, c.part, base + (from - c.lo), base + len, n_ref, INT64_MAX);
        c.guess = from;
        c.stop = c.lo + (size_t)(q - base);
        c.head.assign(base, base + std::min(len, kHead));
        c.tail.assign(q, base + len);
    };
    if (first_rec < chunks[0].hi) decode_chunk(chunks[0], hbuf.data(), first_rec);
    std::atomic<size_t> next(1);
    std::atomic<int> bad(0);
    if (nthreads < 1) nthreads = 1;
    nthreads = (int)std::min<size_t>((size_t)nthreads, chunks.size());
    const bool timing = getenv("PB_TIMING") != nullptr;
    std::atomic<int64_t> ns_inflate(0), ns_decode(0), ns_start(0);
    const auto t_spawn = std::chrono::steady_clock::now();
    auto worker = [&]() {
        auto now = [] { return std::chrono::steady_clock::now(); };
        auto t0 = now();
        if (timing) ns_start += std::chrono::duration_cast<std::chrono::nanoseconds>(t0 - t_spawn).count();
        std::vector<uint8_t> buf;
        buf.reserve(max_chunk);
        for (;;) {
            const size_t k = next.fetch_add(1);
            if (k >= chunks.size()) return;
            Chunk &c = chunks[k];
            if (timing) t0 = now();
            const int rc = inflate_chunk(c, buf);
            if (rc != 0) { bad.store(rc); continue; }
            if (bad.load() != 0) continue;
            auto t1 = t0;
            if (timing) { t1 = now(); ns_inflate += std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count(); }
            const uint8_t *g = guess_record_start(buf.data(), buf.data() + buf.size(), n_ref);
            if (g) decode_chunk(c, buf.data(), c.lo + (size_t)(g - buf.data()));
            else c.head.assign(buf.data(), buf.data() + std::min(buf.size(), kHead));
            if (timing) ns_decode += std::chrono::duration_cast<std::chrono::nanoseconds>(now() - t1).count();
        }
    };
    {
        std::vector<std::thread> pool;
        for (int t = 1; t < nthreads; ++t) pool.emplace_back(worker);
        worker();
        for (auto &t : pool) t.join();
    }
    if (bad.load() != 0) return inflate_error(bad.load());
    if (timing)
        fprintf(stderr, "[bam] %d threads: summed over threads, inflate %.1f ms, decode %.1f ms; mean start delay %.2f ms\n", nthreads,
                ns_inflate.load() / 1e6, ns_decode.load() / 1e6, ns_start.load() / 1e6 / nthreads);
    lap("inflate + decode chunks");

    // ---- chain the chunks
    bam.parts.clear();
    bam.parts.reserve(2 * chunks.size());
    bool truncated = false;
    int64_t redone = 0, refetched = 0;
    size_t expected = first_rec;
    std::vector<uint8_t> buf, rec;
    size_t buf_holds = kNone;                                // the chunk `buf` holds inflated
    for (size_t k = 0; k < chunks.size(); ++k) {
        Chunk &c = chunks[k];
        if (expected >= c.hi) continue;                      // a record (or the header) covers the whole chunk
        if (c.guess != expected) {                           // decode it from where the records really resume
            if (buf_holds != k) {
                if (k == 0) buf = hbuf;
                else if (const int rc = inflate_chunk(c, buf)) return inflate_error(rc);
                buf_holds = k;
            }
            decode_chunk(c, buf.data(), expected);
            ++redone;
        }
        const bool defect = c.part.err_rec != INT64_MAX, bad_size = c.part.bad_size;
        const size_t q = c.stop;
        bam.parts.push_back(std::move(c.part));
        if (defect) break;                                   // stitch_parts reports it
        if (bad_size) { truncated = true; break; }
        expected = q;
        if (q == c.hi) continue;
        // the record that starts at q and ends in a later chunk: its first bytes are c.tail, the rest
        // comes from the heads of the following chunks (or, for a record longer than a head, from
        // inflating them again)
        rec = c.tail;
        size_t j = k + 1, used = 0;                          // next unread stream byte: chunk j, offset `used`
        int pull_rc = 0;
        auto pull = [&](size_t want) {                       // appends up to `want` further stream bytes to rec
            while (want > 0 && j < chunks.size()) {
                const Chunk &d = chunks[j];
                const size_t len = d.hi - d.lo;
                if (used >= len) { ++j; used = 0; continue; }
                const size_t take = std::min(want, len - used);
                if (used + take <= d.head.size()) {
                    rec.insert(rec.end(), d.head.begin() + (long)used, d.head.begin() + (long)(used + take));
                } else {
                    if (buf_holds != j) {
                        if (j == 0) buf = hbuf;
                        else if ((pull_rc = inflate_chunk(d, buf)) != 0) return;
                        buf_holds = j;
                        ++refetched;
                    }
                    rec.insert(rec.end(), buf.begin() + (long)used, buf.begin() + (long)(used + take));
                }
                used += take;
                want -= take;
            }
        };
        if (rec.size() < 4) pull(4 - rec.size());
        if (pull_rc != 0) return inflate_error(pull_rc);
        if (rec.size() < 4) { truncated = true; break; }
        const uint32_t block_size = rd32(rec.data());
        const size_t need = 4 + (size_t)block_size;
        if (block_size < 32 || need > total_u - q) { truncated = true; break; }
        if (rec.size() < need) pull(need - rec.size());
        if (pull_rc != 0) return inflate_error(pull_rc);
        if (rec.size() < need) { truncated = true; break; }
        Part tail;
        decode_span(bam, tail, rec.data(), rec.data() + need, n_ref, 1);
        const bool tail_defect = tail.err_rec != INT64_MAX;
        bam.parts.push_back(std::move(tail));
        if (tail_defect) break;
        expected = q + need;
    }
    if (getenv("PB_TIMING"))
        fprintf(stderr, "[bam] %zu chunks, %lld decoded again serially, %lld inflated again for a long record\n", chunks.size(),
                (long long)redone, (long long)refetched);
    lap("chain chunks");
    if (stitch_parts(bam, truncated, nthreads) != 0) return -1;
    lap("stitch");
    bam.loaded = true;
    return 0;
}

// ---------------------------------------------------------------- SAM text (pb_open_sam)
// The lines of [q, limit) -- whole lines, `nlines` of them, the first being line `first_line` of the file -- into `pt`,
// with the checks of decode_span_cols in its order: a line's own defects (sam_host.h), the order against the record in
// front, the CIGAR defects the formats share, the order of the first aligned positions.
template <bool kSort>
void decode_sam_lines(const Bam &bam, Part &pt, Cols &cols, const uint8_t *q, const uint8_t *limit, int64_t nlines, int64_t first_line,
                      const pcsam::SamRefs &refs) {
    cols.clear();
    cols.room((size_t)nlines + 1);
    if (kSort) cols.room_sorted((size_t)nlines + 1);
    size_t n = 0;
    bool saw_unplaced = false, any_placed = false;
    int32_t last_tid = -1, last_pos = -1, last_spos = -1;
    auto bad = [&](int64_t i, bool before_order, const std::string &m) { pt.err_rec = i; pt.err_before_order = before_order; pt.err = m; };
    for (int64_t i = 0; q < limit; ++i) {
        const uint8_t *le = (const uint8_t *)std::memchr(q, '\n', (size_t)(limit - q));
        const uint8_t *const lb = q;
        if (!le) le = limit;
        q = le < limit ? le + 1 : limit;
        pcsam::SamRec r;
        if (pcsam::sam_parse_line(lb, le, refs, r) >= pcsam::kSamOwnCodes) { bad(i, true, pcsam::sam_defect_message(bam.path.c_str(), first_line + i, r.err)); break; }
        pt.total += 1;
        if (!(r.flag & 0x4)) pt.mapped += 1;
        if (!r.placed) {
            pt.unplaced += 1;
            if (kSort && !saw_unplaced) pt.first_unplaced_rec = i;
            saw_unplaced = true;
            continue;
        }
        if (kSort) {
            any_placed = true;
            cols.rpos[n] = r.pos; cols.rno[n] = (int32_t)i;
        } else if (!any_placed) {        // its order against the previous piece is checked when stitching
            any_placed = true;
            pt.first_placed_rec = i;
            pt.first_tid = r.tid; pt.first_pos = r.pos;
            if (saw_unplaced) { bad(i, false, "BAM file is not coordinate sorted: " + bam.path); break; }
        } else if (saw_unplaced || r.tid < last_tid || (r.tid == last_tid && r.pos < last_pos)) {
            bad(i, false, "BAM file is not coordinate sorted: " + bam.path);
            break;
        }
        if (r.err == pcsam::kSamUnknownOp) { bad(i, false, "unknown CIGAR operation in " + bam.path); break; }
        if (r.err == pcsam::kSamEndBeyond) { bad(i, false, "alignment ends beyond 2^31 - 1"); break; }
        if (r.err == pcsam::kSamTooLong) { bad(i, false, "alignment with more than 2^31 - 1 aligned positions"); break; }
        const bool wide = r.L > 65535u || r.nruns > 255u || (r.L == 65535u && r.nruns == 255u);
        if (wide) { pt.wide_idx.push_back((int64_t)n); pt.wide_alen.push_back((int32_t)r.L); pt.wide_nblk.push_back((int32_t)r.nruns); }
        if (n == 0) pt.first_spos = r.spos;
        else if (!kSort && last_tid == r.tid && last_spos > r.spos) {
            bad(i, false, "alignment starting with a deletion breaks coordinate order; not supported");
            break;
        }
        last_tid = r.tid; last_pos = r.pos; last_spos = r.spos;
        cols.tid[n] = r.tid;
        cols.pos[n] = r.spos;
        cols.alen[n] = wide ? (uint16_t)65535 : (uint16_t)r.L;
        cols.flags[n] = (r.flag & 0x10) ? 1 : 0;
        cols.nblk[n] = wide ? (uint8_t)255 : (uint8_t)r.nruns;
        cols.flag16[n] = r.flag; cols.mapq[n] = (uint8_t)r.mapq; cols.lseq[n] = r.lseq; cols.nh[n] = (uint16_t)(r.mapq >> 16);
        ++n;
        if (r.nruns >= 2) {
            const uint8_t *cb, *ce, *end = le;
            if (end > lb && end[-1] == '\r') --end;
            pcsam::sam_cigar_field(lb, end, cb, ce);
            (void)pcsam::sam_walk_cigar(cb, ce, (int64_t)r.pos, [&](int64_t ref, uint32_t len, bool new_run) {
                if (new_run) { cols.blk_start.push_back((int32_t)ref); cols.blk_len.push_back((int32_t)len); }
                else cols.blk_len.back() += (int32_t)len;
            });
        }
    }
    cols.n = n;
    pt.any_placed = any_placed; pt.saw_unplaced = saw_unplaced;
    pt.last_tid = last_tid; pt.last_pos = last_pos; pt.last_spos = last_spos;
}

// the header of a SAM file: the references into `bam`; `table`: their names as the line parser looks them up
int sam_header(Bam &bam, const FileMap &file, pcsam::SamHeader &hd, pcsam::SamRefTable &table) {
    if (!file.ok) return fail("cannot open " + bam.path);
    if (pcsam::sam_looks_compressed(file.data(), file.size())) return fail(bam.path + ": " + pcsam::sam_compressed_text());
    pcsam::parse_sam_header(file.data(), file.size(), hd, table);
    if (hd.defect != pcsam::kSamOk) return fail(pcsam::sam_defect_message(bam.path.c_str(), hd.defect_line, hd.defect));
    bam.ref_names = hd.ref_names;
    bam.ref_lengths = hd.ref_lengths;
    return 0;
}

// A whole SAM file -> bam.parts: the body is cut at line ends into pieces of about PB_SAM_PIECE bytes (default 4 MiB);
// the worker pool counts the lines of every piece (which gives each piece its first line number), then parses them.
int decode_sam(Bam &bam, int nthreads) {
    Lap lap;
    FileMap file(bam.path);
    pcsam::SamHeader hd;
    pcsam::SamRefTable table;
    if (sam_header(bam, file, hd, table) != 0) return -1;
    const pcsam::SamRefs refs = table.view();
    const uint8_t *const body = file.data() + hd.body_off, *const end = file.data() + file.size();
    int64_t piece = (int64_t)4 << 20;
    if (const char *env = getenv("PB_SAM_PIECE")) piece = std::max(1, atoi(env));   // test knob: tiny pieces exercise the stitching
    std::vector<const uint8_t *> cuts;
    for (const uint8_t *q = body; q < end;) {
        cuts.push_back(q);
        if (end - q <= piece) break;
        const uint8_t *nl = (const uint8_t *)std::memchr(q + piece - 1, '\n', (size_t)(end - (q + piece - 1)));
        if (!nl) break;
        q = nl + 1;
    }
    cuts.push_back(end);
    const size_t nparts = cuts.size() - 1;
    bam.parts.assign(nparts, Part());
    std::vector<int64_t> nlines(nparts, 0), first_line(nparts + 1, hd.header_lines + 1);
    auto on_pool = [&](const std::function<void(size_t)> &job) {
        std::atomic<size_t> nextp(0);
        auto worker = [&]() {
            for (;;) {
                const size_t k = nextp.fetch_add(1);
                if (k >= nparts) return;
                job(k);
            }
        };
        std::vector<std::thread> pool;
        const int nt = (int)std::min<size_t>((size_t)nthreads, std::max<size_t>(nparts, 1));
        for (int t = 1; t < nt; ++t) pool.emplace_back(worker);
        worker();
        for (auto &t : pool) t.join();
    };
    on_pool([&](size_t k) { nlines[k] = pcsam::sam_count_lines(cuts[k], cuts[k + 1]); });
    for (size_t k = 0; k < nparts; ++k) first_line[k + 1] = first_line[k] + nlines[k];
    if (first_line[nparts] - first_line[0] >= (int64_t)0x7fffffff) return fail("more than 2^31-2 records per file are not supported: " + bam.path);
    lap("sam line count");
    on_pool([&](size_t k) {
        thread_local Cols cols;
        if (bam.sorting) decode_sam_lines<true>(bam, bam.parts[k], cols, cuts[k], cuts[k + 1], nlines[k], first_line[k], refs);
        else decode_sam_lines<false>(bam, bam.parts[k], cols, cuts[k], cuts[k + 1], nlines[k], first_line[k], refs);
        keep_columns(bam, bam.parts[k], cols);
    });
    lap("sam parse");
    if (stitch_parts(bam, false, nthreads) != 0) return -1;
    bam.loaded = true;
    return 0;
}

// ---------------------------------------------------------------- coordinate sort at load (pb_load_sorted)
// The wide records of a load as flat (file order) record indices.
void flat_wide(const Bam &b, std::vector<int64_t> &idx, std::vector<int32_t> &alen, std::vector<int32_t> &nblk) {
    for (size_t k = 0; k < b.parts.size(); ++k) {
        const Part &pt = b.parts[k];
        for (size_t j = 0; j < pt.wide_idx.size(); ++j) {
            idx.push_back((int64_t)b.rec_off[k] + pt.wide_idx[j]);
            alen.push_back(pt.wide_alen[j]);
            nblk.push_back(pt.wide_nblk[j]);
        }
    }
}

// Behind a decode with `sorting`: is the file in order by the test of pb_load ((tid, POS) non-decreasing, no placed
// record behind an unplaced one)?  Then nothing moves.  Otherwise the staged order is a stable sort of the placed records
// on (tid, POS, reverse strand) -- the order the device decoder's radix sort gives (sort_kernels.hip.h) -- kept as a
// permutation that pb_fill* apply.  Either way the first aligned positions of neighbours have to be in order too.
int sort_loaded(Bam &bam) {
    const size_t n = bam.nrec;
    std::vector<int32_t> tid(n), rpos(n), spos(n);
    std::vector<uint8_t> rev(n);
    std::vector<int64_t> recno(n);
    int64_t base = 0, first_unplaced = -1, last_placed = -1;
    for (size_t k = 0; k < bam.parts.size(); ++k) {
        const Part &pt = bam.parts[k];
        const size_t at = bam.rec_off[k];
        for (size_t j = 0; j < pt.n; ++j) {
            tid[at + j] = pt.tid[j]; rpos[at + j] = pt.rpos[j]; spos[at + j] = pt.pos[j]; rev[at + j] = pt.flags[j];
            recno[at + j] = base + pt.rno[j];
        }
        if (pt.n) last_placed = base + pt.rno[pt.n - 1];
        if (first_unplaced < 0 && pt.first_unplaced_rec >= 0) first_unplaced = base + pt.first_unplaced_rec;
        base += pt.total;
    }
    bool disorder = first_unplaced >= 0 && last_placed > first_unplaced;
    for (size_t i = 1; i < n && !disorder; ++i)
        disorder = tid[i] < tid[i - 1] || (tid[i] == tid[i - 1] && rpos[i] < rpos[i - 1]);
    bam.sorted_input = !disorder;
    std::vector<uint32_t> perm;
    if (disorder) {
        perm.resize(n);
        std::iota(perm.begin(), perm.end(), 0u);
        std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
            if (tid[a] != tid[b]) return tid[a] < tid[b];
            if (rpos[a] != rpos[b]) return rpos[a] < rpos[b];
            return rev[a] < rev[b];
        });
    }
    auto at = [&](size_t k) { return disorder ? (size_t)perm[k] : k; };
    for (size_t k = 1; k < n; ++k)
        if (tid[at(k)] == tid[at(k - 1)] && spos[at(k - 1)] > spos[at(k)])
            return fail("alignment starting with a deletion breaks coordinate order; not supported");
    bam.moved = 0;
    for (size_t k = 0; k < perm.size(); ++k) bam.moved += perm[k] != (uint32_t)k ? 1 : 0;
    if (bam.moved) {
        bam.file_order.resize(n);
        for (size_t k = 0; k < n; ++k) bam.file_order[k] = recno[perm[k]];
        bam.perm.swap(perm);
    }
    return 0;
}

template <typename T> void permute_column(T *col, const std::vector<uint32_t> &perm) {
    if (!col) return;
    const std::vector<T> old(col, col + perm.size());
    for (size_t k = 0; k < perm.size(); ++k) col[k] = old[perm[k]];
}

// ---------------------------------------------------------------- region-limited loading (BAI / CSI)
// The reference fetches per region through the BAM index (genome_array.py:800-809 via pysam; bin /
// chunk / linear-index scheme of the SAM specification, section 5).  Here the regions of a whole
// query set are resolved at once: bins -> chunks of virtual offsets, clipped by the linear index,
// merged; only the BGZF members those chunks touch are read and inflated; the records then go
// through the same decoder as a whole file and are filtered by htslib's overlap test
// (pos < end && endpos > start).  `mapped` comes from the index's per-reference counts, as
// pysam's AlignmentFile.mapped does.
struct BaiRef {
    std::vector<uint32_t> bin_id;
    std::vector<std::vector<std::pair<uint64_t, uint64_t>>> chunks;
    std::vector<uint64_t> loff;     // CSI: per bin, the offset of its first window (beside bin_id); BAI: empty
    std::vector<uint64_t> linear;   // BAI only
    uint64_t n_mapped = 0, n_unmapped = 0;
    bool has_meta = false;
};

using pcshape::IndexShape;   // the shape of a loaded index: BAI is (14, 5); a CSI carries its own (SAM specification 5.3)

// the BGZF member at file offset `coff`, inflated and appended to `out`; returns its compressed
// length, 0 at end of file, -1 on a damaged member
long read_member(FILE *f, uint64_t coff, std::vector<uint8_t> &out) {
    thread_local std::vector<uint8_t> buf;   // the member as it is in the file: its first 18 bytes say how long it is
    if (fseeko(f, (off_t)coff, SEEK_SET) != 0) return -1;
    buf.resize(18);
    size_t got = fread(buf.data(), 1, 18, f);
    if (got == 0) return 0;
    bh::Member mb;
    int64_t clen = 0;
    int code = bh::parse_member(buf.data(), (int64_t)got, 0, mb, clen);
    if (code == bh::kMemberExtraCut) clen = (int64_t)1 << 16;   // (subfields in front of BC: as much as a member can be)
    if ((code == bh::kMemberCut || code == bh::kMemberExtraCut) && got == 18) {   // the rest of it, and the same parse again
        buf.resize((size_t)clen);
        got += fread(buf.data() + 18, 1, (size_t)clen - 18, f);
        code = bh::parse_member(buf.data(), (int64_t)got, 0, mb, clen);
    }
    if (code != bh::kOk) return -1;
    const size_t at = out.size();
    out.resize(at + mb.ulen);
    if (mb.ulen && raw_inflate(buf.data() + mb.coff, mb.clen, out.data() + at, mb.ulen, mb.crc) != 0) return -1;
    return (long)clen;
}

// The index of `bam_path`: the file `index_path`, or the first of x.bam.bai, x.bai, x.bam.csi, x.csi beside it (htslib
// looks for the .csi first, hts.c:2042-2043; here a file that resolved before this reader knew CSI resolves to the same
// index).  A BAI as it is; a CSI in its BGZF members (or as the bare payload).  No count is trusted before the bytes
// behind it are there.
int load_bai(const std::string &bam_path, const std::string &index_path, std::vector<BaiRef> &refs, IndexShape &shape) {
    std::vector<uint8_t> buf;
    std::string ipath = index_path;
    if (!index_path.empty()) {
        if (!read_file(ipath, buf)) return fail("cannot read the index of " + bam_path + " (" + ipath + ")");
    } else {
        const std::string stem = bam_path.size() > 4 ? bam_path.substr(0, bam_path.size() - 4) : bam_path;
        const std::string cand[4] = {bam_path + ".bai", stem + ".bai", bam_path + ".csi", stem + ".csi"};
        bool found = false;
        for (int k = 0; k < 4 && !found; ++k) { ipath = cand[k]; found = read_file(ipath, buf); }
        if (!found) return fail("cannot read the index of " + bam_path + " (.bam.bai / .bai / .bam.csi / .csi)");
    }
    if (buf.size() >= 2 && buf[0] == 31 && buf[1] == 139) {   // BGZF: member by member, from the bytes read
        FILE *f = fmemopen(buf.data(), buf.size(), "rb");
        if (!f) return fail("cannot read the index of " + bam_path + " (" + ipath + ")");
        std::vector<uint8_t> payload;
        uint64_t coff = 0;
        long cl;
        while ((cl = read_member(f, coff, payload)) > 0) {
            coff += (uint64_t)cl;
            if (payload.size() > ((size_t)1 << 32)) { cl = -1; break; }
        }
        fclose(f);
        if (cl < 0) return fail("damaged BGZF member in the index: " + ipath);
        buf.swap(payload);
        if (buf.size() < 4 || std::memcmp(buf.data(), "CSI\1", 4) != 0) return fail("not a CSI index: " + ipath);
    }
    const uint8_t *p = buf.data(), *end = p + buf.size();
    auto need = [&](size_t n) { return (size_t)(end - p) >= n; };
    shape = IndexShape();
    if (need(4) && std::memcmp(p, "CSI\1", 4) == 0) {
        if (!need(16)) return fail("truncated CSI index: " + ipath);
        const int32_t min_shift = (int32_t)rd32(p + 4), depth = (int32_t)rd32(p + 8), l_aux = (int32_t)rd32(p + 12);
        p += 16;
        if (min_shift < 1 || min_shift > 30 || depth < 0 || depth > 9 || min_shift + 3 * depth > 40) return fail("corrupt CSI index (min_shift / depth): " + ipath);
        if (l_aux < 0 || !need((size_t)l_aux)) return fail("truncated CSI index: " + ipath);
        p += (size_t)l_aux;
        shape.csi = true; shape.min_shift = min_shift; shape.n_lvls = depth;
    } else if (need(4) && std::memcmp(p, "BAI\1", 4) == 0) p += 4;
    else return fail("not a BAI index: " + ipath);
    const char *kind = shape.csi ? "CSI" : "BAI";
    const std::string truncated = std::string("truncated ") + kind + " index: " + ipath;
    if (!need(4)) return fail(truncated);
    const uint32_t n_ref = rd32(p);
    p += 4;
    if (n_ref > (1u << 24)) return fail(std::string("corrupt ") + kind + " index (reference count): " + ipath);
    refs.assign(n_ref, BaiRef());
    auto rd64 = [](const uint8_t *q) { return (uint64_t)rd32(q) | ((uint64_t)rd32(q + 4) << 32); };
    const uint32_t meta_bin = shape.meta_bin();
    const size_t bin_head = shape.csi ? 16 : 8;
    for (uint32_t r = 0; r < n_ref; ++r) {
        BaiRef &br = refs[r];
        if (!need(4)) return fail(truncated);
        const uint32_t n_bin = rd32(p);
        p += 4;
        if ((size_t)(end - p) / bin_head < (size_t)n_bin) return fail(truncated);   // (every bin takes its head at least)
        for (uint32_t b = 0; b < n_bin; ++b) {
            if (!need(bin_head)) return fail(truncated);
            const uint32_t bin = rd32(p), n_chunk = rd32(p + bin_head - 4);
            const uint64_t loff = shape.csi ? rd64(p + 4) : 0;
            p += bin_head;
            if (n_chunk > (1u << 28) || !need((size_t)n_chunk * 16)) return fail(truncated);
            if (bin == meta_bin) { // samtools' metadata pseudo-bin: (file range), (mapped, unmapped)
                if (n_chunk >= 2) { br.n_mapped = rd64(p + 16); br.n_unmapped = rd64(p + 24); br.has_meta = true; }
            } else {
                br.bin_id.push_back(bin);
                if (shape.csi) br.loff.push_back(loff);
                br.chunks.emplace_back();
                auto &v = br.chunks.back();
                v.reserve(n_chunk);
                for (uint32_t c = 0; c < n_chunk; ++c) v.emplace_back(rd64(p + 16 * (size_t)c), rd64(p + 16 * (size_t)c + 8));
            }
            p += (size_t)n_chunk * 16;
        }
        if (shape.csi) {   // no linear index; the bins ascending, for csi_min_off's lookups (htslib writes them in hash order)
            std::vector<size_t> order(br.bin_id.size());
            std::iota(order.begin(), order.end(), (size_t)0);
            std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return br.bin_id[a] < br.bin_id[b]; });
            BaiRef sorted;
            for (size_t k : order) { sorted.bin_id.push_back(br.bin_id[k]); sorted.loff.push_back(br.loff[k]); sorted.chunks.emplace_back(std::move(br.chunks[k])); }
            br.bin_id.swap(sorted.bin_id); br.loff.swap(sorted.loff); br.chunks.swap(sorted.chunks);
            continue;
        }
        if (!need(4)) return fail(truncated);
        const uint32_t n_intv = rd32(p);
        p += 4;
        if (n_intv > (1u << 28) || !need((size_t)n_intv * 8)) return fail(truncated);
        br.linear.resize(n_intv);
        for (uint32_t i = 0; i < n_intv; ++i) br.linear[i] = rd64(p + 8 * (size_t)i);
        p += (size_t)n_intv * 8;
    }
    return 0;
}

// whether `bin` is one of the bins a region may have records in (reg2bins, hts.c:1690-1706): at the bin's level, the
// bins from the one of `beg` to the one of `end - 1`.  Asked per bin the index holds, so a region costs the reference's
// bins and not the leaves it spans (2^24 of them for a whole reference at min_shift 8).
bool in_reg2bins(uint32_t bin, int64_t beg, int64_t end, const IndexShape &shape) {
    if (bin >= shape.n_bins()) return false;
    int l = 0;
    while (l < shape.n_lvls && bin >= pcshape::level_first(l + 1)) ++l;
    const int s = shape.min_shift + 3 * (shape.n_lvls - l);
    const int64_t k = (int64_t)bin - (int64_t)pcshape::level_first(l);
    return k >= (beg >> s) && k <= ((end - 1) >> s);
}

// A CSI has no linear index: the lower bound of a region's chunks is the loff of the nearest bin at or before the leaf of
// `beg` -- from that leaf, step to the previous sibling, or to the parent at a first sibling, until a bin exists
// (hts.c:1773-1784); bin 0's loff when the walk ends there, 0 without one.  bin_id is ascending (load_bai).
uint64_t csi_min_off(const BaiRef &br, const IndexShape &shape, int64_t beg) {
    auto find = [&](uint32_t bin) -> const uint64_t * {
        const auto it = std::lower_bound(br.bin_id.begin(), br.bin_id.end(), bin);
        return it != br.bin_id.end() && *it == bin ? &br.loff[(size_t)(it - br.bin_id.begin())] : nullptr;
    };
    uint32_t bin = pcshape::level_first(shape.n_lvls) + (uint32_t)(beg >> shape.min_shift);
    while (bin > 0) {
        if (const uint64_t *l = find(bin)) return *l;
        const uint32_t parent = (bin - 1) >> 3;
        if (bin > (parent << 3) + 1) --bin;
        else bin = parent;
    }
    const uint64_t *l = find(0);
    return l ? *l : 0;
}

// the BAM header from the leading BGZF members of `f`: as many as it takes
int read_header_members(Bam &bam, FILE *f, uint32_t &n_ref) {
    std::vector<uint8_t> hbuf;
    uint64_t coff = 0;
    for (;;) {
        const long cl = read_member(f, coff, hbuf);
        if (cl <= 0) return fail(cl == 0 ? "truncated BAM header" : "not a BGZF file (bad gzip member header)");
        coff += (uint64_t)cl;
        const uint8_t *p = hbuf.data();
        bool more = false;
        if (parse_header(bam, p, hbuf.data() + hbuf.size(), n_ref, &more) == 0) return 0;
        if (!more) return -1;
    }
}

// A requested region by reference id (sorted, overlapping / adjacent ones merged).
struct RegionSpan { int32_t tid; int64_t s, e; };

// Regions (reference name, 0-based half-open) -> merged regions by reference id and the chunks of virtual offsets
// that hold every record overlapping one of them: the bins of each region (in_reg2bins), clipped by the 16 kb linear
// index (BAI) or the loff of the bin in front of the region (CSI), sorted and merged (SAM specification section 5; what hts_itr_query does per region, hts.c:1924-1960).
int resolve_regions(const Bam &bam, uint32_t n_ref, int nreg, const char *const *rname, const int64_t *rstart, const int64_t *rend,
                    std::vector<BaiRef> &refs, std::vector<RegionSpan> &merged, std::vector<std::pair<uint64_t, uint64_t>> &chunks) {
    IndexShape shape;
    if (load_bai(bam.path, bam.index_path, refs, shape) != 0) return -1;
    if (refs.size() != (size_t)n_ref) return fail("the index does not belong to this BAM file (reference count differs): " + bam.path);
    std::vector<RegionSpan> regs;
    for (int i = 0; i < nreg; ++i) {
        int32_t tid = -1;
        for (uint32_t r = 0; r < n_ref; ++r)
            if (bam.ref_names[r] == rname[i]) { tid = (int32_t)r; break; }
        if (tid < 0) continue;                           // unknown chromosome: fetch() finds nothing there
        const int64_t s = std::max<int64_t>(rstart[i], 0), e = std::min<int64_t>(rend[i], shape.reach());
        if (e > s) regs.push_back({tid, s, e});
    }
    std::sort(regs.begin(), regs.end(), [](const RegionSpan &a, const RegionSpan &b) { return a.tid != b.tid ? a.tid < b.tid : (a.s != b.s ? a.s < b.s : a.e < b.e); });
    merged.clear();
    for (const RegionSpan &r : regs) {
        if (!merged.empty() && merged.back().tid == r.tid && r.s <= merged.back().e) merged.back().e = std::max(merged.back().e, r.e);
        else merged.push_back(r);
    }
    std::vector<std::pair<uint64_t, uint64_t>> ch;
    for (const RegionSpan &r : merged) {
        const BaiRef &br = refs[(size_t)r.tid];
        uint64_t min_off;
        if (shape.csi) min_off = csi_min_off(br, shape, r.s);
        else {
            const size_t w = (size_t)(r.s >> 14);
            if (br.linear.empty()) continue;
            min_off = w < br.linear.size() ? br.linear[w] : br.linear.back();
        }
        for (size_t b = 0; b < br.bin_id.size(); ++b) {
            if (!in_reg2bins(br.bin_id[b], r.s, r.e, shape)) continue;
            for (const auto &c : br.chunks[b])
                if (c.second > min_off && c.second > c.first) ch.push_back(c);
        }
    }
    std::sort(ch.begin(), ch.end());
    chunks.clear();
    for (const auto &c : ch) {
        if (!chunks.empty() && c.first <= chunks.back().second) chunks.back().second = std::max(chunks.back().second, c.second);
        else chunks.push_back(c);
    }
    return 0;
}

int decode_regions(Bam &bam, int nthreads, int nreg, const char *const *rname, const int64_t *rstart, const int64_t *rend) {
    Lap lap;
    FILE *f = fopen(bam.path.c_str(), "rb");
    if (!f) return fail("cannot read " + bam.path);
    struct Closer { FILE *f; ~Closer() { if (f) fclose(f); } } closer{f};
    // ---- header: inflate members from the start of the file until it is complete
    uint32_t n_ref = 0;
    if (read_header_members(bam, f, n_ref) != 0) return -1;
    std::vector<BaiRef> refs;
    std::vector<RegionSpan> merged;
    std::vector<std::pair<uint64_t, uint64_t>> chunks;
    if (resolve_regions(bam, n_ref, nreg, rname, rstart, rend, refs, merged, chunks) != 0) return -1;
    lap("header + index");
    // ---- read and inflate what the chunks touch (threads over chunks, one file handle each)
    std::vector<std::vector<uint8_t>> bytes(chunks.size());
    std::atomic<size_t> next(0);
    std::atomic<int> bad(0);
    auto worker = [&]() {
        FILE *g = fopen(bam.path.c_str(), "rb");
        if (!g) { bad.store(1); return; }
        std::vector<uint8_t> buf;
        for (;;) {
            const size_t k = next.fetch_add(1);
            if (k >= chunks.size()) break;
            const uint64_t vb = chunks[k].first, ve = chunks[k].second;
            const uint64_t cb = vb >> 16, ce = ve >> 16;
            const size_t ub = (size_t)(vb & 0xffff), ue = (size_t)(ve & 0xffff);
            buf.clear();
            uint64_t cur = cb;
            size_t stop = (size_t)-1;
            bool ok = true;
            while (cur < ce || (cur == ce && ue > 0)) {
                const size_t before = buf.size();
                const long cl = read_member(g, cur, buf);
                if (cl <= 0) { ok = false; break; }
                if (cur == ce) { stop = before + ue; break; }
                cur += (uint64_t)cl;
            }
            if (stop == (size_t)-1) stop = buf.size();
            if (!ok || ub > stop || stop > buf.size()) { bad.store(2); continue; }
            bytes[k].assign(buf.begin() + (long)ub, buf.begin() + (long)stop);
        }
        fclose(g);
    };
    {
        std::vector<std::thread> pool;
        const int nt = (int)std::min<size_t>((size_t)std::max(nthreads, 1), std::max<size_t>(chunks.size(), 1));
        for (int t = 1; t < nt; ++t) pool.emplace_back(worker);
        worker();
        for (auto &t : pool) t.join();
    }
    if (bad.load() != 0) return fail("damaged BGZF member or index out of step with " + bam.path);
    size_t total = 0;
    for (const auto &b : bytes) total += b.size();
    std::vector<uint8_t> data;
    data.reserve(total);
    for (const auto &b : bytes) data.insert(data.end(), b.begin(), b.end());
    bytes.clear();
    lap("read + inflate chunks");
    if (decode_records(bam, data.data(), data.data() + data.size(), n_ref, nthreads, lap) != 0) return -1;
    // ---- keep what overlaps a requested region (htslib: pos < end && endpos > start)
    std::vector<size_t> first_reg((size_t)n_ref + 1, merged.size());
    for (size_t i = merged.size(); i-- > 0;) first_reg[(size_t)merged[i].tid] = i;
    auto overlaps = [&](int32_t tid, int64_t pos, int64_t endpos) {
        size_t lo = first_reg[(size_t)tid], hi = lo;
        while (hi < merged.size() && merged[hi].tid == tid) ++hi;
        // first region of this reference whose end lies beyond pos
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            if (merged[mid].e <= pos) lo = mid + 1; else hi = mid;
        }
        return lo < merged.size() && merged[lo].tid == tid && merged[lo].s < endpos;
    };
    for (Part &pt : bam.parts) {
        size_t w = 0, rw = 0, rr = 0, wk = 0, ww = 0;   // wk / ww: wide records seen / kept
        for (size_t i = 0; i < pt.n; ++i) {
            int64_t nb = pt.nblk[i], L = pt.alen[i];
            const bool wide = wk < pt.wide_idx.size() && pt.wide_idx[wk] == (int64_t)i;   // true values aside
            if (wide) { nb = pt.wide_nblk[wk]; L = pt.wide_alen[wk]; }
            const size_t runs = nb >= 2 ? (size_t)nb : 0;
            const int64_t endpos = nb >= 2 ? (int64_t)pt.blk_start[rr + runs - 1] + pt.blk_len[rr + runs - 1]
                                           : (int64_t)pt.pos[i] + std::max<int64_t>(L, 1);
            if (overlaps(pt.tid[i], pt.pos[i], endpos)) {
                pt.tid[w] = pt.tid[i]; pt.pos[w] = pt.pos[i]; pt.alen[w] = pt.alen[i]; pt.flags[w] = pt.flags[i]; pt.nblk[w] = pt.nblk[i];
                pt.flag16[w] = pt.flag16[i]; pt.mapq[w] = pt.mapq[i]; pt.lseq[w] = pt.lseq[i]; pt.nh[w] = pt.nh[i];
                for (size_t k = 0; k < runs; ++k) { pt.blk_start[rw + k] = pt.blk_start[rr + k]; pt.blk_len[rw + k] = pt.blk_len[rr + k]; }
                if (wide) { pt.wide_idx[ww] = (int64_t)w; pt.wide_alen[ww] = pt.wide_alen[wk]; pt.wide_nblk[ww] = pt.wide_nblk[wk]; ++ww; }
                ++w;
                rw += runs;
            }
            if (wide) ++wk;
            rr += runs;
        }
        pt.n = w;
        pt.nrun = rw;
        pt.wide_idx.resize(ww); pt.wide_alen.resize(ww); pt.wide_nblk.resize(ww);
    }
    for (size_t k = 0; k < bam.parts.size(); ++k) {
        bam.rec_off[k + 1] = bam.rec_off[k] + bam.parts[k].n;
        bam.run_off[k + 1] = bam.run_off[k] + bam.parts[k].nrun;
    }
    bam.nrec = bam.parts.empty() ? 0 : bam.rec_off[bam.parts.size()];
    bam.nrun = bam.parts.empty() ? 0 : bam.run_off[bam.parts.size()];
    // `mapped` as pysam reports it: from the index, for the whole file
    bool any_meta = false;
    int64_t mapped = 0;
    for (const BaiRef &br : refs) { any_meta |= br.has_meta; mapped += (int64_t)br.n_mapped; }
    bam.mapped = any_meta ? mapped : -1;
    lap("filter");
    bam.loaded = true;
    return 0;
}

// one thread per usable CPU, at most 128 (starting hundreds of threads costs more than they return)
int default_threads() { return std::min(128, usable_cpus()); }

} // namespace

extern "C" {

const char *pb_last_error(void) { return g_err.c_str(); }

void *pb_open(const char *path) {
    if (!path) {
        fail("pb_open: NULL path");
        return nullptr;
    }
    FILE *f = fopen(path, "rb");
    if (!f) {
        fail(std::string("cannot open ") + path);
        return nullptr;
    }
    fclose(f);
    Bam *b = new Bam();
    b->path = path;
    return b;
}

// pb_open with an explicit index file (a BAM file in a read-only directory, an index built elsewhere): the region calls
// read `index_path` instead of looking beside the file
void *pb_open_indexed(const char *path, const char *index_path) {
    void *h = pb_open(path);
    if (h && index_path) static_cast<Bam *>(h)->index_path = index_path;
    return h;
}

// A SAM TEXT file (an aligner's output as written; what pysam reads with AlignmentFile(path), and what `samtools view -b`
// turns into BAM): the header is parsed here (pb_nref / pb_ref_name / pb_ref_length answer at once), pb_load and
// pb_load_sorted read the lines with the parser of sam_host.h on the worker pool, and every pb_* accessor works as for BAM.
// NULL (pb_last_error): the file cannot be opened, is compressed, or its header is malformed.
void *pb_open_sam(const char *path) {
    Bam *b = static_cast<Bam *>(pb_open(path));
    if (!b) return nullptr;
    b->is_sam = true;
    FileMap file(b->path);
    pcsam::SamHeader hd;
    pcsam::SamRefTable table;
    if (sam_header(*b, file, hd, table) != 0) { delete b; return nullptr; }
    return b;
}

void pb_close(void *h) { delete static_cast<Bam *>(h); }

// decode the whole file with `nthreads` inflate threads (<= 0: hardware concurrency)
int pb_load(void *h, int nthreads) {
    Bam *b = static_cast<Bam *>(h);
    if (!b) return fail("pb_load: NULL handle");
    if (b->loaded) return 0;
    if (nthreads <= 0) nthreads = default_threads();
    return b->is_sam ? decode_sam(*b, nthreads) : decode(*b, nthreads);
}

// region-limited load through the BAI index: only records that overlap one of the `nreg` regions
// (reference name, 0-based half-open) are staged; counts[2] (`mapped`) then comes from the index (-1 if
// the index carries no per-reference counts)
int pb_load_regions(void *h, int nthreads, int nreg, const char *const *names, const int64_t *start, const int64_t *end) {
    Bam *b = static_cast<Bam *>(h);
    if (!b || nreg < 0 || (nreg > 0 && (!names || !start || !end))) return fail("pb_load_regions: bad arguments");
    if (b->is_sam) return fail("pb_load_regions: SAM text has no index: " + b->path);
    if (b->loaded) return fail("pb_load_regions: file already loaded");
    if (nthreads <= 0) nthreads = default_threads();
    return decode_regions(*b, nthreads, nreg, names, start, end);
}

// What a decoder that reads the file itself (pc_bam_open_span: BGZF inflate and record decode on the GPU) needs to know
// about a set of regions: the merged regions by reference id (m_tid / m_start / m_end, capacity nreg; *nmerged of them)
// and the SPAN of virtual offsets [*voff_begin, *voff_end) that holds every chunk of every region (0, 0: no record
// overlaps any of them); *mapped = the index's mapped-read count of the whole file (-1: the index carries none).  The
// header is read as a side effect (pb_nref / pb_ref_name / pb_ref_length answer afterwards).
int pb_resolve_regions(void *h, int nreg, const char *const *names, const int64_t *start, const int64_t *end, uint64_t *voff_begin,
                       uint64_t *voff_end, int64_t *mapped, int *nmerged, int32_t *m_tid, int64_t *m_start, int64_t *m_end) {
    Bam *b = static_cast<Bam *>(h);
    if (!b || nreg < 0 || (nreg > 0 && (!names || !start || !end)) || !voff_begin || !voff_end || !mapped || !nmerged)
        return fail("pb_resolve_regions: bad arguments");
    FILE *f = fopen(b->path.c_str(), "rb");
    if (!f) return fail("cannot read " + b->path);
    uint32_t n_ref = 0;
    const int hrc = read_header_members(*b, f, n_ref);
    fclose(f);
    if (hrc != 0) return -1;
    std::vector<BaiRef> refs;
    std::vector<RegionSpan> merged;
    std::vector<std::pair<uint64_t, uint64_t>> chunks;
    if (resolve_regions(*b, n_ref, nreg, names, start, end, refs, merged, chunks) != 0) return -1;
    *voff_begin = chunks.empty() ? 0 : chunks.front().first;
    *voff_end = 0;
    for (const auto &c : chunks) *voff_end = std::max(*voff_end, c.second);
    int64_t m = 0;
    bool any_meta = false;
    for (const BaiRef &br : refs) { m += (int64_t)br.n_mapped; any_meta |= br.has_meta; }
    *mapped = any_meta ? m : -1;
    *nmerged = (int)merged.size();
    for (size_t k = 0; k < merged.size() && m_tid && m_start && m_end; ++k) { m_tid[k] = merged[k].tid; m_start[k] = merged[k].s; m_end[k] = merged[k].e; }
    return 0;
}

// pb_resolve_regions with the merged chunk list itself instead of its span (pc_bam_open_chunks: only the members the
// chunks touch go to the GPU): *nchunk = the number of chunks, ascending and disjoint [voff_beg[k], voff_end[k]); at most
// `cap` of them are written (call again with a larger `cap` when *nchunk > cap).  Merged regions and *mapped as there.
int pb_resolve_chunks(void *h, int nreg, const char *const *names, const int64_t *start, const int64_t *end, int64_t cap, uint64_t *voff_beg,
                      uint64_t *voff_end, int64_t *nchunk, int64_t *mapped, int *nmerged, int32_t *m_tid, int64_t *m_start, int64_t *m_end) {
    Bam *b = static_cast<Bam *>(h);
    if (!b || nreg < 0 || (nreg > 0 && (!names || !start || !end)) || cap < 0 || (cap > 0 && (!voff_beg || !voff_end)) || !nchunk || !mapped ||
        !nmerged)
        return fail("pb_resolve_chunks: bad arguments");
    FILE *f = fopen(b->path.c_str(), "rb");
    if (!f) return fail("cannot read " + b->path);
    uint32_t n_ref = 0;
    const int hrc = read_header_members(*b, f, n_ref);
    fclose(f);
    if (hrc != 0) return -1;
    std::vector<BaiRef> refs;
    std::vector<RegionSpan> merged;
    std::vector<std::pair<uint64_t, uint64_t>> chunks;
    if (resolve_regions(*b, n_ref, nreg, names, start, end, refs, merged, chunks) != 0) return -1;
    *nchunk = (int64_t)chunks.size();
    for (size_t k = 0; k < chunks.size() && (int64_t)k < cap; ++k) { voff_beg[k] = chunks[k].first; voff_end[k] = chunks[k].second; }
    int64_t m = 0;
    bool any_meta = false;
    for (const BaiRef &br : refs) { m += (int64_t)br.n_mapped; any_meta |= br.has_meta; }
    *mapped = any_meta ? m : -1;
    *nmerged = (int)merged.size();
    for (size_t k = 0; k < merged.size() && m_tid && m_start && m_end; ++k) { m_tid[k] = merged[k].tid; m_start[k] = merged[k].s; m_end[k] = merged[k].e; }
    return 0;
}

int pb_nref(void *h) { return h ? (int)static_cast<Bam *>(h)->ref_names.size() : -1; }
const char *pb_ref_name(void *h, int i) { return static_cast<Bam *>(h)->ref_names[(size_t)i].c_str(); }
int32_t pb_ref_length(void *h, int i) { return static_cast<Bam *>(h)->ref_lengths[(size_t)i]; }

// counts[0] = staged (placed) records, [1] = runs of gapped records, [2] = mapped reads
// (flag 0x4 unset, what pysam's AlignmentFile.mapped reports), [3] = all records
int pb_counts(void *h, int64_t *counts) {
    Bam *b = static_cast<Bam *>(h);
    if (!b || !b->loaded) return fail("pb_counts: file not loaded");
    counts[0] = (int64_t)b->nrec;
    counts[1] = (int64_t)b->nrun;
    counts[2] = b->mapped;
    counts[3] = b->total;
    return 0;
}

// wide records (see Part): how many, and their flat record indices / true aligned lengths / run counts
int64_t pb_wide_count(void *h) {
    Bam *b = static_cast<Bam *>(h);
    if (!b || !b->loaded) return -1;
    int64_t n = 0;
    for (const Part &pt : b->parts) n += (int64_t)pt.wide_idx.size();
    return n;
}

int pb_fill_wide(void *h, int64_t *idx, int32_t *alen, int32_t *nblk) {
    Bam *b = static_cast<Bam *>(h);
    if (!b || !b->loaded) return fail("pb_fill_wide: file not loaded");
    if (!b->perm.empty()) {   // (pb_load_sorted) by staged index, ascending
        std::vector<int64_t> fi;
        std::vector<int32_t> fa, fn;
        flat_wide(*b, fi, fa, fn);
        std::vector<uint32_t> inv(b->perm.size());
        for (size_t k = 0; k < b->perm.size(); ++k) inv[b->perm[k]] = (uint32_t)k;
        std::vector<size_t> by(fi.size());
        std::iota(by.begin(), by.end(), (size_t)0);
        std::sort(by.begin(), by.end(), [&](size_t x, size_t y) { return inv[(size_t)fi[x]] < inv[(size_t)fi[y]]; });
        for (size_t k = 0; k < by.size(); ++k) { idx[k] = (int64_t)inv[(size_t)fi[by[k]]]; alen[k] = fa[by[k]]; nblk[k] = fn[by[k]]; }
        return 0;
    }
    size_t at = 0;
    for (size_t k = 0; k < b->parts.size(); ++k) {
        const Part &pt = b->parts[k];
        for (size_t j = 0; j < pt.wide_idx.size(); ++j, ++at) {
            idx[at] = (int64_t)b->rec_off[k] + pt.wide_idx[j];
            alen[at] = pt.wide_alen[j];
            nblk[at] = pt.wide_nblk[j];
        }
    }
    return 0;
}

int pb_fill(void *h, int32_t *tid, int32_t *pos, uint16_t *alen, uint8_t *flags, uint8_t *nblk, int32_t *blk_start,
            int32_t *blk_len) {
    Bam *b = static_cast<Bam *>(h);
    if (!b || !b->loaded) return fail("pb_fill: file not loaded");
    const size_t nparts = b->parts.size();
    std::atomic<size_t> next(0);
    auto worker = [&]() {
        for (;;) {
            const size_t k = next.fetch_add(1);
            if (k >= nparts) return;
            const Part &pt = b->parts[k];
            const size_t at = b->rec_off[k], n = pt.n, rat = b->run_off[k], m = pt.nrun;
            if (n) {
                std::memcpy(tid + at, pt.tid, n * 4);
                std::memcpy(pos + at, pt.pos, n * 4);
                std::memcpy(alen + at, pt.alen, n * 2);
                std::memcpy(flags + at, pt.flags, n);
                std::memcpy(nblk + at, pt.nblk, n);
            }
            if (m) {
                std::memcpy(blk_start + rat, pt.blk_start, m * 4);
                std::memcpy(blk_len + rat, pt.blk_len, m * 4);
            }
        }
    };
    std::vector<std::thread> pool;
    const int nt = (int)std::min<size_t>((size_t)std::min(std::max(b->threads, 1), 32), std::max<size_t>(nparts, 1));   // a copy: memory-bound
    for (int t = 1; t < nt; ++t) pool.emplace_back(worker);
    worker();
    for (auto &t : pool) t.join();
    if (!b->perm.empty()) {   // (pb_load_sorted) the columns by staged index; every record's runs follow it
        const std::vector<uint32_t> &perm = b->perm;
        const size_t n = perm.size();
        std::vector<int64_t> cnt(nblk, nblk + n), fi;
        std::vector<int32_t> fa, fn;
        flat_wide(*b, fi, fa, fn);
        for (size_t k = 0; k < fi.size(); ++k) cnt[(size_t)fi[k]] = fn[k];   // (a wide record's column holds the marker)
        std::vector<size_t> roff(n + 1, 0);
        for (size_t i = 0; i < n; ++i) roff[i + 1] = roff[i] + (cnt[i] >= 2 ? (size_t)cnt[i] : 0);
        const std::vector<int32_t> os(blk_start, blk_start + roff[n]), ol(blk_len, blk_len + roff[n]);
        size_t w = 0;
        for (size_t k = 0; k < n; ++k)
            for (size_t r = roff[perm[k]]; r < roff[perm[k] + 1]; ++r, ++w) { blk_start[w] = os[r]; blk_len[w] = ol[r]; }
        permute_column(tid, perm); permute_column(pos, perm); permute_column(alen, perm); permute_column(flags, perm); permute_column(nblk, perm);
    }
    return 0;
}


// The SAM FLAG word, MAPQ and l_seq of every staged record (same order as pb_fill's columns): what pysam exposes as
// read.flag / .mapping_quality / .query_length (and the is_* properties derived from the flag bits) to the filter
// functions of BAMGenomeArray.add_filter (genome_array.py:697-722).  Any pointer may be NULL.
// The NH:i tag of every staged record (same order): its value clamped to 65 535, 0 where a record has none -- what
// `read.get_tag("NH")` / `read.has_tag("NH")` answer from in a filter function (genome_array.py:697-722, 819-820).
int pb_fill_nh(void *h, uint16_t *nh) {
    Bam *b = static_cast<Bam *>(h);
    if (!b || !b->loaded) return fail("pb_fill_nh: file not loaded");
    for (size_t k = 0; k < b->parts.size(); ++k) {
        const Part &pt = b->parts[k];
        if (pt.n && nh) std::memcpy(nh + b->rec_off[k], pt.nh, pt.n * 2);
    }
    if (!b->perm.empty()) permute_column(nh, b->perm);
    return 0;
}

int pb_fill_sam(void *h, uint16_t *flag16, uint8_t *mapq, int32_t *lseq) {
    Bam *b = static_cast<Bam *>(h);
    if (!b || !b->loaded) return fail("pb_fill_sam: file not loaded");
    for (size_t k = 0; k < b->parts.size(); ++k) {
        const Part &pt = b->parts[k];
        const size_t at = b->rec_off[k], n = pt.n;
        if (!n) continue;
        if (flag16) std::memcpy(flag16 + at, pt.flag16, n * 2);
        if (mapq) std::memcpy(mapq + at, pt.mapq, n);
        if (lseq) std::memcpy(lseq + at, pt.lseq, n * 4);
    }
    if (!b->perm.empty()) { permute_column(flag16, b->perm); permute_column(mapq, b->perm); permute_column(lseq, b->perm); }
    return 0;
}

// pb_load for a file in ANY record order (an aligner's output, a name-sorted file): the records are decoded without the
// checks between neighbours, and staged placed records first, in the stable order of (reference id, POS, reverse strand)
// -- a coordinate sorter's comparator; unplaced records are not staged, as ever.  A file that pb_load's own order test
// accepts is left exactly as pb_load gives it.  pb_fill* then hand the columns over in the staged order.
int pb_load_sorted(void *h, int nthreads) {
    Bam *b = static_cast<Bam *>(h);
    if (!b) return fail("pb_load_sorted: NULL handle");
    if (b->loaded) return b->sort_requested ? 0 : fail("pb_load_sorted: file already loaded");
    if (nthreads <= 0) nthreads = default_threads();
    b->sorting = b->sort_requested = true;
    if ((b->is_sam ? decode_sam(*b, nthreads) : decode(*b, nthreads)) != 0) return -1;
    if (sort_loaded(*b) != 0) { b->loaded = false; return -1; }
    return 0;
}

// out3: [0] 1 after pb_load_sorted, [1] 1 if the file was in order, [2] records staged elsewhere than their rank in the file
int pb_sort_stats(void *h, int64_t *out3) {
    Bam *b = static_cast<Bam *>(h);
    if (!b || !b->loaded || !out3) return fail("pb_sort_stats: file not loaded");
    out3[0] = b->sort_requested ? 1 : 0; out3[1] = b->sorted_input ? 1 : 0; out3[2] = b->moved;
    return 0;
}

// the 0-based record number in the file (all records counted) of every staged record; fails when no record was moved
int pb_file_order(void *h, int64_t *rec_no) {
    Bam *b = static_cast<Bam *>(h);
    if (!b || !b->loaded) return fail("pb_file_order: file not loaded");
    if (b->perm.empty()) return fail("pb_file_order: no record was moved (the records are in the order of the file)");
    std::memcpy(rec_no, b->file_order.data(), b->file_order.size() * 8);
    return 0;
}
} // extern "C"

#include "host_shims.h"   // the pb_* functions of the host models: tracks, bigWig, deflate
