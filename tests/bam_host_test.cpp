// CPU test of plastid_amd/csrc/bam_host.h, the host logic of the BAM decoders (compiled and run by
// tests/test_host_logic.py; test infrastructure).  BGZF images are built here by hand: a gzip header with a BC subfield,
// arbitrary payload bytes, a CRC word and an ISIZE word -- nothing is inflated on the host, so no payload is DEFLATE.
// Expected values are written out by hand or come from a model that shares no code with the header.
#include <cstdio>
#include <random>
#include <string>
#include "bam_host.h"

using namespace pcbamhost;

namespace {

long bad = 0;
#define CHECK(cond) do { if (!(cond)) { ++bad; printf("line %d: %s\n", __LINE__, #cond); } } while (0)

typedef std::vector<uint8_t> Bytes;
void put16(Bytes &b, uint32_t v) { b.push_back((uint8_t)v); b.push_back((uint8_t)(v >> 8)); }
void put32(Bytes &b, uint32_t v) { put16(b, v & 0xffffu); put16(b, v >> 16); }
void append(Bytes &to, const Bytes &x) { to.insert(to.end(), x.begin(), x.end()); }

// one member: `payload`, ISIZE `isize`, CRC `crc`; `extra`: subfields in front of BC
Bytes member(const Bytes &payload, uint32_t isize, uint32_t crc = 0xc0ffee11u, const Bytes &extra = Bytes()) {
    Bytes m = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255};
    put16(m, (uint32_t)extra.size() + 6);
    append(m, extra);
    m.push_back('B'); m.push_back('C'); put16(m, 2);
    put16(m, (uint32_t)(m.size() + 2 + payload.size() + 8 - 1));
    append(m, payload);
    put32(m, crc); put32(m, isize);
    return m;
}
Bytes filler(size_t n, uint32_t seed) {   // bytes that never look like a gzip magic
    Bytes p(n);
    for (size_t k = 0; k < n; ++k) p[k] = (uint8_t)(1 + (seed * 31 + k * 7) % 29);
    return p;
}
int parse(const Bytes &img, int64_t off, Member &mb, int64_t &clen) { return parse_member(img.data(), (int64_t)img.size(), off, mb, clen); }
bool same(const Member &a, const Member &b) { return a.coff == b.coff && a.clen == b.clen && a.ulen == b.ulen && a.uoff == b.uoff && a.crc == b.crc && a.hdr == b.hdr; }
bool same(const BamPlan &a, const BamPlan &b) {
    if (a.members.size() != b.members.size() || a.runs.size() != b.runs.size() || a.total_u != b.total_u || a.image_bytes != b.image_bytes) return false;
    for (size_t m = 0; m < a.members.size(); ++m) if (!same(a.members[m], b.members[m])) return false;
    for (size_t r = 0; r < a.runs.size(); ++r)
        if (a.runs[r].file_lo != b.runs[r].file_lo || a.runs[r].file_hi != b.runs[r].file_hi || a.runs[r].m0 != b.runs[r].m0 || a.runs[r].m1 != b.runs[r].m1) return false;
    return a.member_run == b.member_run;
}

void test_parse_member() {
    Member mb;
    int64_t clen = 0;
    const Bytes good = member(filler(10, 1), 100);   // 18 + 10 + 8 bytes
    CHECK(good.size() == 36 && parse(good, 0, mb, clen) == kOk);
    CHECK(clen == 36 && mb.coff == 18 && mb.clen == 10 && mb.ulen == 100 && mb.uoff == 0 && mb.crc == 0xc0ffee11u && mb.hdr == 18);
    // each code from the smallest image that provokes it
    CHECK(parse(Bytes(good.begin(), good.begin() + 17), 0, mb, clen) == kMemberShort);
    Bytes x(good.begin(), good.begin() + 18);
    x[3] = 0;                                                          // no FEXTRA flag
    CHECK(parse(x, 0, mb, clen) == kMemberMagic);
    x = Bytes(good.begin(), good.begin() + 18); x[10] = 7;            // an extra field of 7 bytes in an image of 18
    CHECK(parse(x, 0, mb, clen) == kMemberExtraCut);
    x = Bytes(good.begin(), good.begin() + 18); x[12] = 'X';          // the one subfield is not BC
    CHECK(parse(x, 0, mb, clen) == kMemberNoBC);
    x = Bytes(good.begin(), good.begin() + 18); x[14] = 1;            // ... or BC of the wrong length
    CHECK(parse(x, 0, mb, clen) == kMemberNoBC);
    clen = 0;
    CHECK(parse(Bytes(good.begin(), good.begin() + 35), 0, mb, clen) == kMemberCut && clen == 36);   // (the length it claims)
    CHECK(parse(Bytes(good.begin(), good.begin() + 18), 0, mb, clen) == kMemberCut && clen == 36);
    x = member(Bytes(), 65537);                                        // header and trailer alone, ISIZE beyond 64 KiB
    CHECK(x.size() == 26 && parse(x, 0, mb, clen) == kMemberIsize);
    x[22] = 0; x[23] = 0; x[24] = 1; x[25] = 0;                        // exactly 64 KiB is fine
    CHECK(parse(x, 0, mb, clen) == kOk && mb.ulen == 65536 && mb.clen == 0);
    x = Bytes(good.begin(), good.begin() + 18); x[16] = 21; x.resize(22, 0);   // BSIZE + 1 = 22 bytes: no room for the trailer
    CHECK(parse(x, 0, mb, clen) == kMemberTiny && clen == 22 && mb.ulen == 0);
    for (uint8_t bsize = 0; bsize < 3; ++bsize) {                      // BSIZE + 1 below 4: not even an ISIZE word, and nothing in front of the image is read
        x = Bytes(good.begin(), good.begin() + 18); x[16] = bsize;
        mb.ulen = 9;
        CHECK(parse(x, 0, mb, clen) == kMemberTiny && clen == bsize + 1 && mb.ulen == 0);
    }
    for (int code = kMemberShort; code <= kChunkInRecord; ++code) CHECK(defect_text(code) && defect_text(code)[0]);
    CHECK(std::string(defect_text(kMemberShort)) == "truncated BGZF header" && std::string(defect_text(kMemberIsize)) == "corrupt BGZF member (more than 64 KiB of payload)");
    CHECK(std::string(defect_text(kMemberTiny)) == "BGZF inflate failed in " && chunk_defect(kChunkNoStart) && !chunk_defect(kMemberTiny));
    // subfields in front of BC (one of them an odd length); an empty member; a member behind another
    const Bytes extra = {'R', 'A', 3, 0, 9, 9, 9, 'Z', 'Z', 0, 0};
    Bytes img = member(filler(5, 2), 77, 0x01020304u, extra);
    const size_t first = img.size();
    append(img, member(Bytes{3, 0}, 0, 0));
    CHECK(parse(img, 0, mb, clen) == kOk && clen == (int64_t)first && mb.hdr == 18 + 11 && mb.coff == 29 && mb.clen == 5 && mb.ulen == 77 && mb.crc == 0x01020304u);
    CHECK(parse(img, (int64_t)first, mb, clen) == kOk && clen == 28 && mb.ulen == 0 && mb.clen == 2 && mb.coff == first + 18);
    CHECK(parse(img, (int64_t)first + 1, mb, clen) == kMemberMagic && parse(img, (int64_t)img.size() - 3, mb, clen) == kMemberShort);
}

// serial (walk_min above the size) and parallel (walk_min 1, seven threads whatever the machine has: stretches that begin inside members) walks of one image
void both_walks(const Bytes &img, int want_code, size_t want_members) {
    BamPlan s, p;
    const int cs = plan_members(img.data(), (int64_t)img.size(), nullptr, (int64_t)img.size() + 1, s);
    const int cp = plan_members(img.data(), (int64_t)img.size(), nullptr, 1, p, 7);
    CHECK(cs == want_code && cp == want_code);
    if (want_code == kOk) {
        CHECK(same(s, p) && s.members.size() == want_members && s.runs.size() == 1 && s.runs[0].file_hi == (int64_t)img.size() && s.image_bytes == (int64_t)img.size());
        uint64_t u = 0;
        for (const Member &mb : s.members) { CHECK(mb.uoff == u && mb.ulen > 0); u += mb.ulen; }
        CHECK(u == s.total_u);
    }
}

void test_plan_whole_file() {
    // 220 small members, every eleventh empty
    Bytes img;
    size_t full = 0;
    for (int k = 0; k < 220; ++k) {
        const bool empty = k % 11 == 5;
        append(img, member(filler(1 + (size_t)(k * 37 % 90), (uint32_t)k), empty ? 0 : 50 + (uint32_t)k, (uint32_t)k * 2654435761u));
        full += !empty;
    }
    both_walks(img, kOk, full);
    // every payload holds two false members and the head of a third that ends with the true member: a stretch of the
    // parallel walk that begins inside a member starts on a false one, walks into the true chain and must not be taken
    Bytes fakes = member(Bytes(), 5);
    append(fakes, member(Bytes(), 6));
    Bytes third = member(filler(4, 3), 7);
    third.resize(18);   // (its BSIZE reaches over the 4 bytes of filler and the true trailer)
    append(fakes, third);
    append(fakes, filler(4, 3));
    img.clear();
    for (int k = 0; k < 300; ++k) append(img, member(fakes, 7, (uint32_t)k));
    {
        Member mb;
        int64_t clen = 0;
        CHECK(parse(img, 18, mb, clen) == kOk && clen == 26 && parse(img, 18 + 26, mb, clen) == kOk && clen == 26);
        CHECK(parse(img, 18 + 52, mb, clen) == kOk && 18 + 52 + clen == (int64_t)img.size() / 300 && mb.ulen == 7);   // the false chain lands on the next true member
    }
    both_walks(img, kOk, 300);
    // a defect in the last third is the serial walk's
    const size_t each = img.size() / 300;
    Bytes broken = img;
    broken[each * 240 + 1] = 0;
    both_walks(broken, kMemberMagic, 0);
    broken = img;
    broken.resize(each * 290 + 30);
    both_walks(broken, kMemberCut, 0);
    both_walks(Bytes(), kOk, 0);
}

// 40 members of 36 bytes, 100 bytes of stream each, member 7 empty: member f lies at 36 f
Bytes image40() {
    Bytes img;
    for (int f = 0; f < 40; ++f) append(img, member(filler(10, (uint32_t)f), f == 7 ? 0 : 100, (uint32_t)f));
    return img;
}
uint64_t voff(int member_no, uint32_t u) { return ((uint64_t)(36 * member_no) << 16) | u; }
int region(const Bytes &img, int64_t header_bytes, const std::vector<uint64_t> &cb, const std::vector<uint64_t> &ce, BamPlan &pl) {
    BamSpan sp;
    sp.nchunk = (int)cb.size(); sp.cbeg = cb.data(); sp.cend = ce.data(); sp.header_bytes = header_bytes;
    pl = BamPlan();
    return plan_members(img.data(), (int64_t)img.size(), &sp, 1, pl);
}
bool run_is(const BamPlan::Run &r, int64_t lo, int64_t hi, int64_t dev, int m0, int m1) { return r.file_lo == lo && r.file_hi == hi && r.dev_lo == dev && r.m0 == m0 && r.m1 == m1; }
bool chunk_is(const BamPlan::ChunkAt &c, int64_t cb, int s, int e, uint32_t ub, uint32_t ue) { return c.cb == cb && c.s_idx == s && c.e_idx == e && c.ub == ub && c.ue == ue; }

void test_plan_region() {
    const Bytes img = image40();
    BamPlan pl;
    std::vector<uint64_t> bounds;
    // two chunks that share member 12 (the second one's first member is already walked): one run beside the header's
    CHECK(region(img, 36, {voff(10, 5), voff(12, 20)}, {voff(12, 20), voff(13, 7)}, pl) == kOk);
    CHECK(pl.runs.size() == 2 && run_is(pl.runs[0], 0, 36, 0, 0, 1) && run_is(pl.runs[1], 360, 504, 36, 1, 5));
    CHECK(pl.chunk_at.size() == 2 && chunk_is(pl.chunk_at[0], 360, 1, 3, 5, 20) && chunk_is(pl.chunk_at[1], 432, 3, 4, 20, 7));
    CHECK(pl.nm() == 5 && pl.total_u == 500 && pl.image_bytes == 180 && pl.member_run == std::vector<uint32_t>({0, 1, 1, 1, 1}));
    CHECK(pl.members[0].coff == 18 && pl.members[1].coff == 36 + 18 && pl.members[4].coff == 36 + 3 * 36 + 18 && pl.members[4].uoff == 400 && pl.members[3].crc == 12);
    CHECK(run_bounds(pl, 30, bounds) == kOk && bounds == std::vector<uint64_t>({100, 100, 105, 407}));
    CHECK(run_bounds(pl, 106, bounds) == kChunkInHeader);
    // a chunk that starts where the run before ends goes on with that run
    CHECK(region(img, 72, {voff(2, 0)}, {voff(3, 0)}, pl) == kOk);
    CHECK(pl.runs.size() == 1 && run_is(pl.runs[0], 0, 108, 0, 0, 3) && chunk_is(pl.chunk_at[0], 72, 2, 3, 0, 0) && pl.image_bytes == 108);
    CHECK(run_bounds(pl, 200, bounds) == kOk && bounds == std::vector<uint64_t>({200, 300}));
    // a chunk that ends on a member border against one that ends inside the member behind it
    CHECK(region(img, 36, {voff(10, 0)}, {voff(12, 0)}, pl) == kOk);
    CHECK(pl.runs.size() == 2 && run_is(pl.runs[1], 360, 432, 36, 1, 3) && chunk_is(pl.chunk_at[0], 360, 1, 3, 0, 0) && pl.total_u == 300);
    CHECK(run_bounds(pl, 30, bounds) == kOk && bounds == std::vector<uint64_t>({100, 100, 100, 300}));
    CHECK(region(img, 36, {voff(10, 0)}, {voff(12, 3)}, pl) == kOk);
    CHECK(run_is(pl.runs[1], 360, 468, 36, 1, 4) && chunk_is(pl.chunk_at[0], 360, 1, 3, 0, 3) && pl.total_u == 400);
    CHECK(run_bounds(pl, 30, bounds) == kOk && bounds == std::vector<uint64_t>({100, 100, 100, 303}));
    // a chunk that starts at the empty member: at the next one that holds something
    CHECK(region(img, 36, {voff(7, 0)}, {voff(9, 0)}, pl) == kOk);
    CHECK(run_is(pl.runs[1], 252, 324, 36, 1, 2) && chunk_is(pl.chunk_at[0], 252, 1, 2, 0, 0) && pl.members[1].coff == 36 + 36 + 18 && pl.image_bytes == 108);
    // the header's bytes end inside the first chunk: the header's members stop at the chunk, and the run goes on
    CHECK(region(img, 400, {voff(10, 0), voff(20, 50)}, {voff(10, 60), voff(21, 0)}, pl) == kOk);
    CHECK(pl.runs.size() == 2 && run_is(pl.runs[0], 0, 396, 0, 0, 10) && run_is(pl.runs[1], 720, 756, 396, 10, 11));
    CHECK(chunk_is(pl.chunk_at[0], 360, 9, 9, 0, 60) && chunk_is(pl.chunk_at[1], 720, 10, 11, 50, 0) && pl.members[10].coff == 396 + 18 && pl.total_u == 1100);
    CHECK(run_bounds(pl, 30, bounds) == kOk && bounds == std::vector<uint64_t>({900, 960, 1050, 1100}));
    // no chunk: the header alone
    CHECK(region(img, 100, {}, {}, pl) == kOk && pl.runs.size() == 1 && run_is(pl.runs[0], 0, 108, 0, 0, 3) && pl.chunk_at.empty());
    // every reason for which an index does not belong to the file
    CHECK(region(img, 36, {voff(40, 0)}, {voff(41, 0)}, pl) == kChunkBeyond);
    CHECK(region(img, 36, {voff(39, 0)}, {voff(40, 1)}, pl) == kChunkBeyond);
    CHECK(region(img, 36, {voff(10, 0) + (1ull << 16)}, {voff(11, 0)}, pl) == kChunkNoStart);   // no member at 361
    CHECK(region(img, 72, {voff(1, 0) + (1ull << 16)}, {voff(3, 0)}, pl) == kChunkNoStart);     // ... inside what is walked
    CHECK(region(img, 36, {voff(10, 101)}, {voff(11, 0)}, pl) == kChunkNoStart);                // beyond the member's payload
    CHECK(region(img, 36, {voff(10, 0)}, {voff(11, 101)}, pl) == kChunkNoEnd);
    CHECK(region(img, 36, {voff(10, 0)}, {voff(11, 0) + (4ull << 16)}, pl) == kChunkNoEnd);      // ends at 400: no border
    CHECK(region(img, 36, {voff(10, 50)}, {voff(10, 20)}, pl) == kOk && run_bounds(pl, 30, bounds) == kChunkInHeader);   // ends before it starts
    Bytes broken = img;
    broken[36 * 11] = 0;
    CHECK(region(broken, 36, {voff(10, 0)}, {voff(12, 0)}, pl) == kMemberMagic && region(broken, 36, {voff(11, 0)}, {voff(12, 0)}, pl) == kChunkNoStart);
}

void test_pieces() {
    const Bytes img = image40();
    BamPlan pl;   // three runs: [0, 36) [360, 504) [720, 828), members 1 + 4 + 3
    CHECK(region(img, 36, {voff(10, 0), voff(20, 0)}, {voff(14, 0), voff(23, 0)}, pl) == kOk && pl.runs.size() == 3 && pl.nm() == 8 && pl.image_bytes == 288);
    auto tiles = [&](const std::vector<ImagePiece> &pc) {
        int m = 0;
        int64_t at = 0;
        for (const ImagePiece &x : pc) { CHECK(x.m0 == m && x.m1 > x.m0 && x.byte0 == at && x.byte1 > x.byte0); m = x.m1; at = x.byte1; }
        CHECK(m == pl.nm() && at == pl.image_bytes);
    };
    auto is = [](const ImagePiece &x, int m0, int m1, int64_t b0, int64_t b1, bool one) { return x.m0 == m0 && x.m1 == m1 && x.byte0 == b0 && x.byte1 == b1 && x.one_run == one; };
    std::vector<ImagePiece> pc = cut_pieces(pl, 1);   // every member its own piece; a piece ends with the member's payload, or with its run
    tiles(pc);
    const int64_t ends[8] = {36, 64, 100, 136, 180, 208, 244, 288};
    CHECK(pc.size() == 8);
    for (size_t k = 0; k < pc.size() && k < 8; ++k) CHECK(is(pc[k], (int)k, (int)k + 1, k ? ends[k - 1] : 0, ends[k], true));
    pc = cut_pieces(pl, 100);    // pieces that straddle a run border are not one run
    tiles(pc);
    CHECK(pc.size() == 3 && is(pc[0], 0, 3, 0, 100, false) && is(pc[1], 3, 6, 100, 208, false) && is(pc[2], 6, 8, 208, 288, true));
    pc = cut_pieces(pl, 150);    // full with the last member of a run: the rest of the run rides along
    tiles(pc);
    CHECK(pc.size() == 2 && is(pc[0], 0, 5, 0, 180, false) && is(pc[1], 5, 8, 180, 288, true));
    pc = cut_pieces(pl, 1000);
    tiles(pc);
    CHECK(pc.size() == 1 && is(pc[0], 0, 8, 0, 288, false));
    CHECK(piece_source(img.data(), pl, cut_pieces(pl, 1)[2]) == img.data() + 360 + (64 - 36));
    CHECK(cut_pieces(BamPlan(), 5).empty());
    // the gather of every [lo, hi) against the runs' bytes, one behind the other
    Bytes dev(img.begin(), img.begin() + 36);
    dev.insert(dev.end(), img.begin() + 360, img.begin() + 504);
    dev.insert(dev.end(), img.begin() + 720, img.begin() + 828);
    for (int64_t lo = 0; lo <= 288; ++lo)
        for (int64_t hi = lo; hi <= 288; ++hi) {
            Bytes got((size_t)(hi - lo) + 1, 0xee);
            copy_image(img.data(), pl.runs, got.data(), lo, hi);
            if (!std::equal(got.begin(), got.end() - 1, dev.begin() + lo) || got.back() != 0xee) { CHECK(!"gather"); return; }
        }
}

void test_header() {
    Bytes h = {'B', 'A', 'M', 1};
    const std::string text = "@HD\tVN:1\n";
    put32(h, (uint32_t)text.size());
    h.insert(h.end(), text.begin(), text.end());
    const size_t text_end = h.size();
    put32(h, 3);
    const char *names[3] = {"chr1", "c2", ""};
    const int32_t lengths[3] = {1000, 0x7fffffff, 16571};
    for (int r = 0; r < 3; ++r) {
        const std::string nm = names[r];
        put32(h, (uint32_t)nm.size() + 1);
        h.insert(h.end(), nm.begin(), nm.end());
        h.push_back(0);
        put32(h, (uint32_t)lengths[r]);
    }
    Bytes all = h;
    append(all, filler(40, 9));   // (records follow)
    for (size_t n = 0; n < h.size(); ++n) {   // every proper prefix needs more; with no more, each decoder says:
        BamHeader bh_;
        const Bytes prefix(h.begin(), h.begin() + (long)n);
        const HeaderParse hp = parse_bam_header(prefix.data(), n, bh_);
        CHECK(hp.status == kHeaderMore);
        const std::string want = n < 12 ? "not a BAM file (bad magic)" : (n < text_end + 4 ? "truncated BAM header" : "truncated BAM reference list");
        CHECK(hp.text && want == hp.text);
    }
    BamHeader bh_;
    HeaderParse hp = parse_bam_header(all.data(), all.size(), bh_);
    CHECK(hp.status == kHeaderOk && bh_.n_ref == 3 && bh_.first_record == h.size());
    CHECK(bh_.ref_names == std::vector<std::string>({"chr1", "c2", ""}) && bh_.ref_lengths == std::vector<int32_t>({1000, 0x7fffffff, 16571}));
    hp = parse_bam_header(h.data(), h.size(), bh_);
    CHECK(hp.status == kHeaderOk && bh_.first_record == h.size());
    Bytes x = h;
    x[2] = 'X';
    hp = parse_bam_header(x.data(), 4, bh_);
    CHECK(hp.status == kHeaderDefect && std::string(hp.text) == "not a BAM file (bad magic)");
    CHECK(parse_bam_header(x.data(), 3, bh_).status == kHeaderMore && parse_bam_header(x.data(), x.size(), bh_).status == kHeaderDefect);
    CHECK(parse_bam_header(nullptr, 0, bh_).status == kHeaderMore);
}

BamPlan plan4(bool two_runs) {   // four members of 100 bytes of stream
    BamPlan pl;
    for (int m = 0; m < 4; ++m) pl.members.push_back(Member{(uint64_t)(36 * m + 18), 10, 100, (uint64_t)(100 * m), 0, 18});
    pl.total_u = 400;
    pl.member_run = two_runs ? std::vector<uint32_t>({0, 0, 1, 1}) : std::vector<uint32_t>(4, 0u);
    return pl;
}

void test_settle() {
    const BamPlan pl = plan4(false);
    const std::vector<MemberChain> holds = {{30, 110, 3, 0}, {110, 205, 4, 0}, {205, 300, 2, 0}, {300, 400, 5, 0}};
    {   // a chain that holds
        ChainState s(pl, nullptr, 30);
        const Settle r = settle_round(pl, nullptr, holds.data(), 0, s);
        CHECK(r.kind == kSettled && s.nrec_of == std::vector<uint32_t>({3, 4, 2, 5}) && s.expected == 400);
        CHECK(record_bases(s.nrec_of) == std::vector<uint64_t>({0, 3, 7, 9, 14}));
    }
    {   // member 2 guessed wrong: again from where member 1's chain ends; the state goes on from there
        std::vector<MemberChain> c = holds;
        c[2] = MemberChain{212, 300, 1, 0};
        c[3] = MemberChain{300, 400, 5, 1};   // (flag 1 alone means nothing once the start is confirmed)
        ChainState s(pl, nullptr, 30);
        Settle r = settle_round(pl, nullptr, c.data(), 0, s);
        CHECK(r.kind == kRedo && r.m == 2 && r.forced == 205 && s.expected == 205 && s.nrec_of == std::vector<uint32_t>({3, 4, 0, 0}));
        c[2] = holds[2];
        r = settle_round(pl, nullptr, c.data(), 2, s);
        CHECK(r.kind == kSettled && s.nrec_of == std::vector<uint32_t>({3, 4, 2, 5}));
    }
    {   // no record starts in member 2 (one of member 1 reaches over it): whatever its walk says is not looked at
        std::vector<MemberChain> c = holds;
        c[1].next = 320; c[2] = MemberChain{~0ull, 0, 77, 3}; c[3].first = 320;
        ChainState s(pl, nullptr, 30);
        CHECK(settle_round(pl, nullptr, c.data(), 0, s).kind == kSettled && s.nrec_of == std::vector<uint32_t>({3, 4, 0, 5}));
        c[3].first = 300;
        ChainState s2(pl, nullptr, 30);
        const Settle r = settle_round(pl, nullptr, c.data(), 0, s2);
        CHECK(r.kind == kRedo && r.m == 3 && r.forced == 320);
    }
    {   // a length prefix that cannot be: the records found up to it count, the file is truncated there
        std::vector<MemberChain> c = holds;
        c[1] = MemberChain{110, 150, 2, 2};
        ChainState s(pl, nullptr, 30);
        const Settle r = settle_round(pl, nullptr, c.data(), 0, s);
        CHECK(r.kind == kTruncated && r.m == 1 && s.nrec_of == std::vector<uint32_t>({3, 2, 0, 0}));
    }
    for (uint64_t last : {380ull, 420ull}) {   // the chain stops short of the end of the stream, or runs past it
        std::vector<MemberChain> c = holds;
        c[3].next = last;
        ChainState s(pl, nullptr, 30);
        const Settle r = settle_round(pl, nullptr, c.data(), 0, s);
        CHECK(r.kind == kTruncated && r.m == 4 && s.nrec_of == std::vector<uint32_t>({3, 4, 2, 5}));
    }
    // two runs: records from 30 to 150, and from 220 to 390
    const BamPlan pr = plan4(true);
    const std::vector<uint64_t> bounds = {30, 150, 220, 390};
    const std::vector<MemberChain> runs = {{30, 110, 3, 0}, {110, 150, 2, 0}, {220, 300, 2, 0}, {300, 390, 3, 0}};
    {
        ChainState s(pr, &bounds, 12);
        CHECK(s.cur_run == 0 && s.expected == 30);
        CHECK(settle_round(pr, &bounds, runs.data(), 0, s).kind == kSettled && s.nrec_of == std::vector<uint32_t>({3, 2, 2, 3}) && s.cur_run == 1);
    }
    {   // the first run has to end exactly at its stop
        std::vector<MemberChain> c = runs;
        c[1].next = 160;
        ChainState s(pr, &bounds, 12);
        const Settle r = settle_round(pr, &bounds, c.data(), 0, s);
        CHECK(r.kind == kInsideRecord && r.m == 2);
    }
    {   // ... and so has the last; a length prefix that cannot be is the same refusal
        std::vector<MemberChain> c = runs;
        c[3].next = 395;
        ChainState s(pr, &bounds, 12);
        CHECK(settle_round(pr, &bounds, c.data(), 0, s).kind == kInsideRecord);
        c = runs;
        c[2].flags = 2;
        ChainState s2(pr, &bounds, 12);
        CHECK(settle_round(pr, &bounds, c.data(), 0, s2).kind == kInsideRecord);
    }
    {   // a member behind its run's last chunk holds no record of the read; a wrong guess in the second run
        const std::vector<uint64_t> early = {30, 95, 220, 390};
        std::vector<MemberChain> c = runs;
        c[0].next = 95; c[1] = MemberChain{1, 2, 9, 3}; c[2].first = 230;
        ChainState s(pr, &early, 12);
        const Settle r = settle_round(pr, &early, c.data(), 0, s);
        CHECK(r.kind == kRedo && r.m == 2 && r.forced == 220 && s.nrec_of == std::vector<uint32_t>({3, 0, 0, 0}));
    }
}

void test_tables() {
    // group_members against the member that holds the record, looked up record by record
    std::mt19937 rng(5);
    for (int trial = 0; trial < 200; ++trial) {
        const int nm = 1 + (int)(rng() % 12);
        std::vector<uint32_t> nrec_of((size_t)nm);
        for (auto &x : nrec_of) x = rng() % 3 ? (uint32_t)(rng() % 700) : 0u;
        const std::vector<uint64_t> rec_base = record_bases(nrec_of);
        const int64_t nrec = (int64_t)rec_base.back();
        const std::vector<uint32_t> got = group_members(rec_base, nrec, nm);
        CHECK((int64_t)got.size() == (nrec + 255) / 256);
        for (size_t g = 0; g < got.size(); ++g) {
            int holds = -1;
            for (int m = 0; m < nm; ++m) if (rec_base[(size_t)m] <= g * 256 && g * 256 < rec_base[(size_t)m + 1]) holds = m;
            CHECK(holds >= 0 && got[g] == (uint32_t)holds);
        }
    }
    CHECK(group_members({0}, 0, 0).empty());
    // bgzf_tell: a payload member at 0, an empty one at 36, a payload member at 64, the EOF block at 100
    const std::vector<Member> two = {Member{18, 10, 100, 0, 0, 18}, Member{82, 10, 100, 100, 0, 18}};
    CHECK(tell_table(two, 128) == std::vector<uint64_t>({0, 0, 36, 64, 100, 100}));
    CHECK(tell_table(two, 100) == std::vector<uint64_t>({0, 0, 36, 64, 100, 100}) && tell_table(two, 99) == std::vector<uint64_t>({0, 0, 36, 64, 99, 99}));
    const std::vector<Member> lead = {Member{28 + 18, 10, 100, 0, 0, 18}};   // an empty member in front of the first payload
    CHECK(tell_table(lead, 64) == std::vector<uint64_t>({0, 28, 64, 64}) && tell_table({}, 28) == std::vector<uint64_t>({0, 0}));
    CHECK(index_key_bits(0) == 32 && index_key_bits(1) == 33 && index_key_bits(1ull << 16) == 49 && index_key_bits(1ull << 31) == 64);
    CHECK(index_key_bits(65535) == 48 && index_key_bits(~0ull) == 64);
    std::vector<int64_t> idx = {9, 2, 5};
    std::vector<int32_t> alen = {90, 20, 50}, nblk = {3, 1, 2};
    order_wide_list(idx, alen, nblk);
    CHECK(idx == std::vector<int64_t>({2, 5, 9}) && alen == std::vector<int32_t>({20, 50, 90}) && nblk == std::vector<int32_t>({1, 2, 3}));
}

} // namespace

int main() {
    test_parse_member();
    test_plan_whole_file();
    test_plan_region();
    test_pieces();
    test_header();
    test_settle();
    test_tables();
    CHECK(usable_cpus() >= 1);
    if (bad) { printf("bam_host: %ld checks failed\n", bad); return 1; }
    printf("bam_host: ok\n");
    return 0;
}
