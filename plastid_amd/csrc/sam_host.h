// sam_host.h -- SAM TEXT, line by line: the one parser of the host reader (bam_stager.cpp, pb_open_sam) and of the device
// decoder (sam_kernels.hip.h).  A line gives the fields the packed format keeps -- what k_bam_fields takes from a BAM
// record: reference id, POS, FLAG, MAPQ, the CIGAR's aligned positions and runs, l_seq, NH:i -- with the meanings of
// pcbam::RecOut, so that everything behind the fields (order checks, sort, placement, columns) is shared with BAM.
// The per-line functions carry PC_SAM_HD: __host__ __device__ under hipcc, nothing under a host compiler, so both paths
// run this source.  The header parse and the defect messages are host only.
// Plain C++17 (no HIP): tests/sam_host_test.cpp compiles it on a machine without a GPU, under the sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define PC_SAM_HD __host__ __device__
#else
#define PC_SAM_HD
#endif

namespace pcsam {

// Defect codes.  Below 32: the codes of the BAM record decode (bam_kernels.hip.h, kRec*) that a SAM line can raise too,
// with the BAM decoders' messages; from 32: SAM text's own, reported as "<path>: SAM line <n>: <what>".
enum {
    kSamOk = 0,
    kSamUnsorted = 5, kSamUnknownOp = 7, kSamEndBeyond = 8, kSamTooLong = 9, kSamDeletionOrder = 10,
    kSamEmptyLine = 32, kSamHeaderInBody, kSamFewFields, kSamBadFlag, kSamUnknownRef, kSamBadPos, kSamNoPos, kSamBadMapq,
    kSamCigarLength, kSamEmptyField,
    kSamSqNoName, kSamSqNoLength, kSamSqBadLength, kSamSqDuplicate, kSamNoReferences,
    kSamCodeEnd
};
constexpr int kSamOwnCodes = 32;   // codes from here on are SAM's own
constexpr uint32_t kMaxCigarLen = (1u << 28) - 1;

inline const char *sam_defect_text(int code) {
    switch (code) {
    case kSamEmptyLine: return "empty line";
    case kSamHeaderInBody: return "header line ('@') behind the first alignment line";
    case kSamFewFields: return "fewer than 11 tab-separated fields";
    case kSamBadFlag: return "FLAG is not a decimal number in 0 .. 65535";
    case kSamUnknownRef: return "RNAME is not the SN of any @SQ header line";
    case kSamBadPos: return "POS is not a decimal number in 0 .. 2^31 - 1";
    case kSamNoPos: return "alignment with a reference name and POS 0";
    case kSamBadMapq: return "MAPQ is not a decimal number in 0 .. 255";
    case kSamCigarLength: return "CIGAR operation without a length, or with one above 2^28 - 1";
    case kSamEmptyField: return "empty mandatory field";
    case kSamSqNoName: return "@SQ line without an SN field";
    case kSamSqNoLength: return "@SQ line without an LN field";
    case kSamSqBadLength: return "@SQ LN is not a decimal number in 1 .. 2^31 - 1";
    case kSamSqDuplicate: return "@SQ line repeats the SN of an earlier one";
    case kSamNoReferences: return "alignment lines in a file without any @SQ header line";
    default: return "malformed line";
    }
}
// `line`: 1-based, header lines counted
inline std::string sam_defect_message(const char *path, int64_t line, int code) {
    return std::string(path ? path : "<memory>") + ": SAM line " + std::to_string((long long)line) + ": " + sam_defect_text(code);
}

// The fields of one line: pcbam::RecOut, member for member (the fields kernel copies one into the other).
struct SamRec {
    int32_t tid, spos, pos;     // reference id (-1: RNAME '*'), first aligned position, POS - 1
    uint32_t L, nruns;          // aligned positions; maximal runs of them
    uint16_t flag;
    uint8_t err;                // a defect code above
    uint8_t placed;             // 1: has a reference and no defect of SAM's own; a line with one of those counts as unplaced
    int32_t lseq;               // length of SEQ, 0 for '*'
    uint32_t mapq;              // bits 0-7 MAPQ; bits 16-31 NH:i clamped to 65 535 (0: none)
    int32_t end;                // one past the last aligned position (spos + 1 without aligned bases)
};

// The reference names as the parser looks them up: an open-addressing table of (FNV-1a of the name, id), a power of two
// of slots with at least one empty (tid -1); a hit is confirmed on the bytes.
struct SamRefs {
    const uint64_t *hash = nullptr;
    const int32_t *tid = nullptr;
    uint32_t mask = 0;
    const uint8_t *names = nullptr;      // all names, back to back
    const uint32_t *name_off = nullptr;  // n_ref + 1 offsets into `names`
};

PC_SAM_HD inline uint64_t sam_fnv1a(const uint8_t *b, const uint8_t *e) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (; b < e; ++b) { h ^= (uint64_t)*b; h *= 0x100000001b3ull; }
    return h;
}

PC_SAM_HD inline int32_t sam_lookup_ref(const SamRefs &r, const uint8_t *b, const uint8_t *e) {
    if (!r.tid) return -1;
    const uint64_t h = sam_fnv1a(b, e);
    const size_t len = (size_t)(e - b);
    for (uint32_t s = (uint32_t)h & r.mask;; s = (s + 1u) & r.mask) {
        const int32_t t = r.tid[s];
        if (t < 0) return -1;
        if (r.hash[s] != h) continue;
        const uint32_t o = r.name_off[t];
        if ((size_t)(r.name_off[t + 1] - o) != len) continue;
        size_t k = 0;
        while (k < len && r.names[o + k] == b[k]) ++k;
        if (k == len) return t;
    }
}

// plain decimal in [b, e): digits only, at least one, value <= max
PC_SAM_HD inline bool sam_decimal(const uint8_t *b, const uint8_t *e, uint64_t max, uint64_t &v) {
    if (b >= e) return false;
    uint64_t x = 0;
    for (; b < e; ++b) {
        const uint32_t d = (uint32_t)*b - (uint32_t)'0';
        if (d > 9u) return false;
        x = x * 10u + d;
        if (x > max) return false;       // (max < 2^32: no overflow before this trips)
    }
    v = x;
    return true;
}

// the first tab in [b, e), or e
PC_SAM_HD inline const uint8_t *sam_field_end(const uint8_t *b, const uint8_t *e) {
    while (b < e && *b != (uint8_t)'\t') ++b;
    return b;
}

// What a CIGAR text gives, by the rules of k_bam_fields: M = X are aligned positions, D N move along the reference,
// I S H P do neither; a run is a maximal stretch of aligned positions.  `emit(start, len, new_run)` sees every aligned
// operation of non-zero length (the columns kernel writes the runs with it).  The walk stops at a defect.
struct CigarWalk {
    int64_t ref, L, run_end;
    int32_t first_run;
    uint32_t nruns;
    int err;
};
template <typename Emit>
PC_SAM_HD inline CigarWalk sam_walk_cigar(const uint8_t *c, const uint8_t *ce, int64_t pos, Emit emit) {
    CigarWalk w;
    w.ref = pos; w.L = 0; w.run_end = -1; w.first_run = -1; w.nruns = 0; w.err = kSamOk;
    if (ce - c == 1 && *c == (uint8_t)'*') return w;
    while (c < ce) {
        uint32_t len = 0;
        bool have = false, big = false;
        while (c < ce && (uint32_t)*c - (uint32_t)'0' <= 9u) {
            len = len * 10u + ((uint32_t)*c - (uint32_t)'0');
            if (len > kMaxCigarLen) { big = true; len = kMaxCigarLen; }
            have = true;
            ++c;
        }
        if (c >= ce) { w.err = kSamUnknownOp; break; }            // digits and no operation behind them
        const uint8_t op = *c++;
        const bool aligned = op == 'M' || op == '=' || op == 'X', refonly = op == 'D' || op == 'N';
        if (!aligned && !refonly && op != 'I' && op != 'S' && op != 'H' && op != 'P') { w.err = kSamUnknownOp; break; }
        if (!have || big) { w.err = kSamCigarLength; break; }
        if (aligned) {
            if (len) {
                const bool new_run = w.run_end != w.ref;
                if (new_run) { ++w.nruns; if (w.first_run < 0) w.first_run = (int32_t)w.ref; }
                emit(w.ref, len, new_run);
                w.ref += len; w.L += len; w.run_end = w.ref;
            }
        } else if (refonly) w.ref += len;
    }
    return w;
}
struct CigarNoEmit { PC_SAM_HD void operator()(int64_t, uint32_t, bool) const {} };

// The CIGAR field (the sixth) of a line the parser has accepted.
PC_SAM_HD inline void sam_cigar_field(const uint8_t *begin, const uint8_t *end, const uint8_t *&cb, const uint8_t *&ce) {
    const uint8_t *f = begin;
    for (int k = 0; k < 5; ++k) { f = sam_field_end(f, end); if (f < end) ++f; }
    cb = f; ce = sam_field_end(f, end);
}

// One line, [begin, end) without its '\n' (a trailing '\r' is dropped here) -> out; returns out.err.  Reads nothing
// outside [begin, end).  The first defect from the left is the line's.
PC_SAM_HD inline int sam_parse_line(const uint8_t *begin, const uint8_t *end, const SamRefs &refs, SamRec &out) {
    out.tid = -1; out.spos = 0; out.pos = 0; out.L = 0; out.nruns = 0; out.flag = 0; out.err = kSamOk; out.placed = 0;
    out.lseq = 0; out.mapq = 0; out.end = 0;
    if (end > begin && end[-1] == (uint8_t)'\r') --end;
    if (end <= begin) { out.err = kSamEmptyLine; return out.err; }
    if (*begin == (uint8_t)'@') { out.err = kSamHeaderInBody; return out.err; }
    // the eleven mandatory fields: f[k] .. g[k]
    const uint8_t *f = begin, *g = begin;
    const uint8_t *cb = begin, *ce = begin;
    int32_t tid = -1;
    uint64_t v = 0;
    for (int k = 0; k < 11; ++k) {
        if (k) {
            if (g >= end) { out.err = kSamFewFields; return out.err; }
            f = g + 1;
        }
        g = sam_field_end(f, end);
        switch (k) {
        case 1:
            if (!sam_decimal(f, g, 65535u, v)) { out.err = kSamBadFlag; return out.err; }
            out.flag = (uint16_t)v;
            break;
        case 2:
            if (f == g) { out.err = kSamEmptyField; return out.err; }
            if (!(g - f == 1 && *f == (uint8_t)'*')) {
                tid = sam_lookup_ref(refs, f, g);
                if (tid < 0) { out.err = kSamUnknownRef; return out.err; }
            }
            break;
        case 3:
            if (!sam_decimal(f, g, 0x7fffffffu, v)) { out.err = kSamBadPos; return out.err; }
            out.pos = (int32_t)((int64_t)v - 1);
            if (tid >= 0 && v == 0) { out.err = kSamNoPos; return out.err; }
            break;
        case 4:
            if (!sam_decimal(f, g, 255u, v)) { out.err = kSamBadMapq; return out.err; }
            out.mapq = (uint32_t)v;
            break;
        case 5:
            if (f == g) { out.err = kSamEmptyField; return out.err; }
            cb = f; ce = g;
            break;
        case 9:
            if (f == g) { out.err = kSamEmptyField; return out.err; }
            out.lseq = (g - f == 1 && *f == (uint8_t)'*') ? 0 : (int32_t)(g - f);
            break;
        default: break;                                       // QNAME RNEXT PNEXT TLEN QUAL: they exist
        }
    }
    // optional fields: the first that begins with NH:i:
    while (g < end) {
        f = g + 1;
        g = sam_field_end(f, end);
        if (g - f >= 5 && f[0] == 'N' && f[1] == 'H' && f[2] == ':' && f[3] == 'i' && f[4] == ':') {
            const uint8_t *q = f + 5;
            const bool neg = q < g && *q == (uint8_t)'-';
            if (neg) ++q;
            uint32_t nh = 0;
            for (; q < g && (uint32_t)*q - (uint32_t)'0' <= 9u; ++q) { nh = nh * 10u + ((uint32_t)*q - (uint32_t)'0'); if (nh > 65535u) nh = 65535u; }
            out.mapq |= (neg ? 0u : nh) << 16;
            break;
        }
    }
    const CigarWalk w = sam_walk_cigar(cb, ce, (int64_t)out.pos, CigarNoEmit());
    out.spos = out.pos;
    if (w.err >= kSamOwnCodes) { out.err = (uint8_t)w.err; return out.err; }
    if (tid < 0) return out.err;                              // unplaced: counted, not staged (as k_bam_fields leaves it)
    out.tid = tid;
    out.placed = 1;
    int err = w.err;
    if (err == kSamOk && w.ref > 0x7fffffffLL) err = kSamEndBeyond;
    if (err == kSamOk && w.L > 0x7fffffffLL) err = kSamTooLong;
    out.err = (uint8_t)err;
    out.L = (uint32_t)w.L; out.nruns = w.nruns;
    if (w.nruns) out.spos = w.first_run;
    out.end = (int32_t)(w.nruns ? (w.run_end > 0x7fffffffLL ? 0x7fffffffLL : w.run_end) : (int64_t)out.pos + 1);
    return out.err;
}

// ---------------------------------------------------------------- host only: the header, and the table of its names

struct SamHeader {
    std::vector<std::string> ref_names;
    std::vector<int32_t> ref_lengths;
    size_t body_off = 0;             // where the first line that does not begin with '@' starts (the size: none)
    int64_t header_lines = 0;
    int defect = kSamOk;             // the first defect, and its 1-based line
    int64_t defect_line = 0;
};

struct SamRefTable {                 // what SamRefs points into
    std::vector<uint64_t> hash;
    std::vector<int32_t> tid;
    std::vector<uint8_t> names;
    std::vector<uint32_t> name_off;
    uint32_t mask = 0;
    void reset(size_t n_expected) {
        size_t slots = 4;
        while (slots < 2 * n_expected + 2) slots <<= 1;
        hash.assign(slots, 0); tid.assign(slots, -1); names.clear(); name_off.assign(1, 0u);
        mask = (uint32_t)(slots - 1);
    }
    SamRefs view() const {
        SamRefs r;
        r.hash = hash.data(); r.tid = tid.data(); r.mask = mask; r.names = names.data(); r.name_off = name_off.data();
        return r;
    }
    // the next reference id for the name; false: the name is in the table already
    bool add(const uint8_t *b, const uint8_t *e) {
        if (sam_lookup_ref(view(), b, e) >= 0) return false;
        const int32_t t = (int32_t)name_off.size() - 1;
        if (2 * ((size_t)t + 1) + 2 > hash.size()) {   // grow: insert everything again
            SamRefTable big;
            big.reset(4 * ((size_t)t + 1));
            for (int32_t k = 0; k < t; ++k) big.add(names.data() + name_off[(size_t)k], names.data() + name_off[(size_t)k + 1]);
            *this = big;
        }
        names.insert(names.end(), b, e);
        name_off.push_back((uint32_t)names.size());
        const uint64_t h = sam_fnv1a(b, e);
        uint32_t s = (uint32_t)h & mask;
        while (tid[s] >= 0) s = (s + 1u) & mask;
        hash[s] = h; tid[s] = t;
        return true;
    }
};

// The leading '@' lines of the text [p, p + n): every @SQ gives one reference (SN, LN; any field order), in line order.
// h.defect != kSamOk: refused, at h.defect_line.  `table` ends up holding the names.
inline void parse_sam_header(const uint8_t *p, size_t n, SamHeader &h, SamRefTable &table) {
    const uint8_t *q = p, *const end = p + n;
    table.reset(64);
    auto bad = [&](int code) { if (h.defect == kSamOk) { h.defect = code; h.defect_line = h.header_lines; } };
    while (q < end && *q == (uint8_t)'@') {
        const uint8_t *le = q;
        while (le < end && *le != (uint8_t)'\n') ++le;
        const uint8_t *next = le < end ? le + 1 : le;
        if (le > q && le[-1] == (uint8_t)'\r') --le;
        h.header_lines += 1;
        if (le - q >= 3 && q[1] == 'S' && q[2] == 'Q' && (le - q == 3 || q[3] == (uint8_t)'\t')) {
            const uint8_t *sn_b = nullptr, *sn_e = nullptr, *ln_b = nullptr, *ln_e = nullptr;
            const uint8_t *g = sam_field_end(q, le);
            while (g < le) {
                const uint8_t *f = g + 1;
                g = sam_field_end(f, le);
                if (g - f >= 3 && f[2] == ':') {
                    if (f[0] == 'S' && f[1] == 'N' && !sn_b) { sn_b = f + 3; sn_e = g; }
                    if (f[0] == 'L' && f[1] == 'N' && !ln_b) { ln_b = f + 3; ln_e = g; }
                }
            }
            uint64_t len = 0;
            if (!sn_b || sn_b == sn_e) bad(kSamSqNoName);
            else if (!ln_b) bad(kSamSqNoLength);
            else if (!sam_decimal(ln_b, ln_e, 0x7fffffffu, len) || len == 0) bad(kSamSqBadLength);
            else if (!table.add(sn_b, sn_e)) bad(kSamSqDuplicate);
            else { h.ref_names.emplace_back((const char *)sn_b, (size_t)(sn_e - sn_b)); h.ref_lengths.push_back((int32_t)len); }
        }
        q = next;
    }
    h.body_off = (size_t)(q - p);
    if (h.defect == kSamOk && q < end && h.ref_names.empty()) { h.defect = kSamNoReferences; h.defect_line = h.header_lines + 1; }
}

// lines of the body [b, e): its '\n' bytes, and one more for a last line without one
inline int64_t sam_count_lines(const uint8_t *b, const uint8_t *e) {
    int64_t n = 0;
    for (const uint8_t *q = b; q < e; ++q) n += *q == (uint8_t)'\n';
    return n + ((e > b && e[-1] != (uint8_t)'\n') ? 1 : 0);
}

// gzip / BGZF magic: compressed SAM is refused by every reader
inline bool sam_looks_compressed(const uint8_t *p, size_t n) { return n >= 2 && p[0] == 0x1f && p[1] == 0x8b; }
inline const char *sam_compressed_text() { return "compressed SAM (gzip / BGZF) is not supported: decompress it, or convert it to BAM"; }

} // namespace pcsam
