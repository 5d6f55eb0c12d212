// sam_host_test.cpp -- plastid_amd/csrc/sam_host.h on the CPU: the line parser the host reader and the device kernels
// share, the header parse and the defect messages, on hand-worked lines.  Every line is parsed from a heap buffer of
// exactly its length, so that under the address sanitizer a read outside [begin, end) is an error: the parser on every
// prefix of a valid line and on lines of 0xff bytes is the bounds check of the kernels that run the same source.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sam_host.h"

using namespace pcsam;

static int g_fail = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static SamRefTable g_table;

// parse `s` from a buffer that ends exactly at its last byte
static SamRec parse(const std::string &s) {
    std::unique_ptr<uint8_t[]> buf(new uint8_t[s.size() ? s.size() : 1]);
    if (!s.empty()) std::memcpy(buf.get(), s.data(), s.size());
    SamRec r;
    const int err = sam_parse_line(buf.get(), buf.get() + s.size(), g_table.view(), r);
    CHECK(err == r.err);
    return r;
}

static std::string line(const char *flag, const char *rname, const char *pos, const char *mapq, const char *cigar, const char *seq, const char *tags = nullptr) {
    std::string s = std::string("q1\t") + flag + "\t" + rname + "\t" + pos + "\t" + mapq + "\t" + cigar + "\t*\t0\t0\t" + seq + "\t*";
    if (tags) s += std::string("\t") + tags;
    return s;
}

static void test_fields() {
    SamRec r = parse(line("16", "chrB", "101", "37", "30M", "ACGTACGTACGTACGTACGTACGTACGTAC", "NH:i:3"));
    CHECK(r.err == kSamOk && r.placed == 1 && r.tid == 1 && r.pos == 100 && r.spos == 100 && r.L == 30 && r.nruns == 1 && r.end == 130);
    CHECK(r.flag == 16 && (r.mapq & 0xff) == 37 && (r.mapq >> 16) == 3 && r.lseq == 30);
    // M = X are aligned, D N move, I S H P do neither; adjacent aligned operations are one run; a deletion splits the run
    r = parse(line("0", "chrA", "11", "0", "2H3S5M2I4=1P3X10N6M2D7M4S", "*"));
    CHECK(r.err == kSamOk && r.pos == 10 && r.spos == 10 && r.L == 5 + 4 + 3 + 6 + 7 && r.nruns == 3 && r.end == 10 + 12 + 10 + 6 + 2 + 7 && r.lseq == 0);
    // a CIGAR that opens with a deletion: the first aligned position is behind POS
    r = parse(line("0", "chrA", "101", "9", "50D20M", "*"));
    CHECK(r.err == kSamOk && r.pos == 100 && r.spos == 150 && r.L == 20 && r.nruns == 1 && r.end == 170);
    // no CIGAR: no aligned bases, end = POS + 1
    r = parse(line("4", "chrA", "101", "0", "*", "ACGT"));
    CHECK(r.err == kSamOk && r.placed == 1 && r.L == 0 && r.nruns == 0 && r.spos == 100 && r.end == 101 && r.lseq == 4);
    // zero-length operations add nothing
    r = parse(line("0", "chrA", "1", "0", "0M5M0N5M", "*"));
    CHECK(r.err == kSamOk && r.L == 10 && r.nruns == 1 && r.pos == 0);
    // unplaced: counted, nothing else looked at
    r = parse(line("4", "*", "0", "0", "*", "*"));
    CHECK(r.err == kSamOk && r.placed == 0 && r.tid == -1 && r.pos == -1 && r.flag == 4);
    r = parse(line("77", "*", "500", "255", "10M", "ACGTACGTAC"));
    CHECK(r.err == kSamOk && r.placed == 0 && r.tid == -1 && r.flag == 77 && (r.mapq & 0xff) == 255);
    // a trailing carriage return is not part of the line
    r = parse(line("0", "chrA", "5", "1", "3M", "ACG", "NH:i:2") + "\r");
    CHECK(r.err == kSamOk && (r.mapq >> 16) == 2 && r.L == 3);
    r = parse(line("0", "chrA", "5", "1", "3M", "ACG") + "\r");
    CHECK(r.err == kSamOk && r.L == 3);
    // limits
    r = parse(line("65535", "chrEnd", "2147483647", "255", "1M", "*"));
    CHECK(r.err == kSamOk && r.flag == 65535 && r.pos == 2147483646 && r.end == 2147483647);
    r = parse(line("0", "chrEnd", "2147483647", "0", "2M", "*"));
    CHECK(r.err == kSamEndBeyond && r.placed == 1);
    r = parse(line("0", "chrEnd", "1", "0", "268435455M268435455M268435455M268435455M268435455M268435455M268435455M268435455M1M", "*"));
    CHECK(r.err == kSamOk && r.L == 2147483641u && r.end == 2147483641);   // (8 (2^28 - 1) + 1 positions from 0: fits)
    r = parse(line("0", "chrEnd", "1", "0", "268435455M268435455M268435455M268435455M268435455M268435455M268435455M268435455M8M", "*"));
    CHECK(r.err == kSamEndBeyond);                                   // (2^31 positions from 0: ends beyond 2^31 - 1)
    r = parse(line("0", "chrEnd", "1", "0", "268435455M", "*"));
    CHECK(r.err == kSamOk && r.L == 268435455u);
    r = parse(line("007", "chrA", "0005", "010", "3M", "*"));        // leading zeros are decimal digits
    CHECK(r.err == kSamOk && r.flag == 7 && r.pos == 4 && (r.mapq & 0xff) == 10);
}

static void test_defects() {
    struct Case { std::string s; int code; const char *text; };
    const Case cases[] = {
        {"", kSamEmptyLine, "empty line"},
        {"\r", kSamEmptyLine, "empty line"},
        {"@CO\tx", kSamHeaderInBody, "header line ('@') behind the first alignment line"},
        {"q1", kSamFewFields, "fewer than 11 tab-separated fields"},
        {"q1\t0\tchrA\t1\t0\t1M\t*\t0\t0\t*", kSamFewFields, "fewer than 11 tab-separated fields"},
        {line("0x10", "chrA", "1", "0", "1M", "*"), kSamBadFlag, "FLAG is not a decimal number in 0 .. 65535"},
        {line("+5", "chrA", "1", "0", "1M", "*"), kSamBadFlag, "FLAG is not a decimal number in 0 .. 65535"},
        {line("-0", "chrA", "1", "0", "1M", "*"), kSamBadFlag, "FLAG is not a decimal number in 0 .. 65535"},
        {line("", "chrA", "1", "0", "1M", "*"), kSamBadFlag, "FLAG is not a decimal number in 0 .. 65535"},
        {line("65536", "chrA", "1", "0", "1M", "*"), kSamBadFlag, "FLAG is not a decimal number in 0 .. 65535"},
        {line("99999999999999999999999", "chrA", "1", "0", "1M", "*"), kSamBadFlag, "FLAG is not a decimal number in 0 .. 65535"},
        {line("0", "chrZ", "1", "0", "1M", "*"), kSamUnknownRef, "RNAME is not the SN of any @SQ header line"},
        {line("0", "chr", "1", "0", "1M", "*"), kSamUnknownRef, "RNAME is not the SN of any @SQ header line"},
        {line("0", "chrAA", "1", "0", "1M", "*"), kSamUnknownRef, "RNAME is not the SN of any @SQ header line"},
        {line("0", "", "1", "0", "1M", "*"), kSamEmptyField, "empty mandatory field"},
        {line("0", "chrA", "-1", "0", "1M", "*"), kSamBadPos, "POS is not a decimal number in 0 .. 2^31 - 1"},
        {line("0", "chrA", "2147483648", "0", "1M", "*"), kSamBadPos, "POS is not a decimal number in 0 .. 2^31 - 1"},
        {line("0", "chrA", "1e3", "0", "1M", "*"), kSamBadPos, "POS is not a decimal number in 0 .. 2^31 - 1"},
        {line("0", "chrA", "0", "0", "1M", "*"), kSamNoPos, "alignment with a reference name and POS 0"},
        {line("0", "chrA", "1", "256", "1M", "*"), kSamBadMapq, "MAPQ is not a decimal number in 0 .. 255"},
        {line("0", "chrA", "1", "", "1M", "*"), kSamBadMapq, "MAPQ is not a decimal number in 0 .. 255"},
        {line("0", "chrA", "1", "0", "M", "*"), kSamCigarLength, "CIGAR operation without a length, or with one above 2^28 - 1"},
        {line("0", "chrA", "1", "0", "5MM", "*"), kSamCigarLength, "CIGAR operation without a length, or with one above 2^28 - 1"},
        {line("0", "chrA", "1", "0", "268435456M", "*"), kSamCigarLength, "CIGAR operation without a length, or with one above 2^28 - 1"},
        {line("0", "chrA", "1", "0", "99999999999999999999M", "*"), kSamCigarLength, "CIGAR operation without a length, or with one above 2^28 - 1"},
        {line("0", "chrA", "1", "0", "", "*"), kSamEmptyField, "empty mandatory field"},
        {line("0", "chrA", "1", "0", "1M", ""), kSamEmptyField, "empty mandatory field"},
    };
    for (const Case &c : cases) {
        const SamRec r = parse(c.s);
        if (r.err != c.code) std::printf("  line '%s': code %d, expected %d\n", c.s.c_str(), r.err, c.code);
        CHECK(r.err == c.code && r.placed == 0 && r.tid == -1);
        CHECK(std::string(sam_defect_text(c.code)) == c.text);
    }
    CHECK(sam_defect_message("dir/x.sam", 12, kSamBadFlag) == "dir/x.sam: SAM line 12: FLAG is not a decimal number in 0 .. 65535");
    // the defects the formats share leave a placed record (the order check comes before them, as for BAM)
    SamRec r = parse(line("0", "chrA", "1", "0", "5M3Q", "*"));
    CHECK(r.err == kSamUnknownOp && r.placed == 1 && r.tid == 0);
    r = parse(line("0", "chrA", "1", "0", "5m", "*"));
    CHECK(r.err == kSamUnknownOp);
    r = parse(line("0", "chrA", "1", "0", "30", "*"));
    CHECK(r.err == kSamUnknownOp);
    r = parse(line("0", "chrA", "1", "0", "Q", "*"));                // an unknown character is that, with or without a length
    CHECK(r.err == kSamUnknownOp);
    // the first defect from the left is the line's
    r = parse(line("x", "chrZ", "-1", "999", "Q", "*"));
    CHECK(r.err == kSamBadFlag);
    r = parse(line("0", "chrZ", "-1", "999", "Q", "*"));
    CHECK(r.err == kSamUnknownRef);
}

static void test_nh() {
    struct Case { const char *tags; unsigned nh; };
    const Case cases[] = {
        {"XX:Z:aNH:i:5", 0}, {"NH:Z:3", 0}, {"NH:i:0", 0}, {"NH:i:70000", 65535}, {"NH:i:-1", 0}, {"NH:i:65535", 65535}, {"NH:i:65536", 65535},
        {"NH:i:4000000000", 65535}, {"NH:i:99999999999999999999999999", 65535}, {"NH:i:1", 1}, {"XS:A:+\tNM:i:2\tNH:i:12", 12},
        {"NH:i:7\tNH:i:9", 7}, {"nh:i:4", 0}, {"NH:i:", 0}, {"NH:i", 0}, {"NH", 0}, {"XNH:i:5", 0}, {"NH:i:-70000", 0}, {"MD:Z:NH:i:3\tNH:i:2", 2},
    };
    for (const Case &c : cases) {
        const SamRec r = parse(line("0", "chrA", "10", "3", "4M", "ACGT", c.tags));
        if ((r.mapq >> 16) != c.nh) std::printf("  tags '%s': nh %u, expected %u\n", c.tags, r.mapq >> 16, c.nh);
        CHECK(r.err == kSamOk && (r.mapq >> 16) == c.nh && (r.mapq & 0xffffu) == 3);
    }
    const SamRec r = parse(line("0", "chrA", "10", "3", "4M", "ACGT"));
    CHECK(r.err == kSamOk && (r.mapq >> 16) == 0);
}

static void test_long_cigars() {
    // 300 runs: beyond the 8-bit column; the walk that writes the runs gives the same runs
    std::string cig;
    for (int k = 0; k < 300; ++k) cig += (k ? "7N" : "") + std::string("5M");
    SamRec r = parse(line("0", "chrA", "1001", "0", cig.c_str(), "*"));
    CHECK(r.err == kSamOk && r.nruns == 300 && r.L == 1500 && r.spos == 1000 && r.end == 1000 + 300 * 5 + 299 * 7);
    const std::string s = line("0", "chrA", "1001", "0", cig.c_str(), "*");
    const uint8_t *b = (const uint8_t *)s.data(), *cb, *ce;
    sam_cigar_field(b, b + s.size(), cb, ce);
    CHECK(std::string((const char *)cb, (size_t)(ce - cb)) == cig);
    std::vector<std::pair<int64_t, int64_t>> runs;
    const CigarWalk w = sam_walk_cigar(cb, ce, 1000, [&](int64_t ref, uint32_t len, bool new_run) {
        if (new_run) runs.emplace_back(ref, (int64_t)len); else runs.back().second += len;
    });
    CHECK(w.err == kSamOk && runs.size() == 300 && runs[0].first == 1000 && runs[299].first == 1000 + 299 * 12 && runs[299].second == 5);
    // more than 65 535 aligned bases, in one run and in several
    r = parse(line("0", "chrA", "1", "0", "70000M", "*"));
    CHECK(r.err == kSamOk && r.L == 70000 && r.nruns == 1);
    r = parse(line("0", "chrA", "1", "0", "40000M1D40000=5I10X", "*"));
    CHECK(r.err == kSamOk && r.L == 80010 && r.nruns == 2 && r.end == 80011);
}

static void test_header() {
    auto parse_header = [](const std::string &text, SamHeader &h) {
        SamRefTable t;
        std::unique_ptr<uint8_t[]> buf(new uint8_t[text.size() ? text.size() : 1]);
        if (!text.empty()) std::memcpy(buf.get(), text.data(), text.size());
        parse_sam_header(buf.get(), text.size(), h, t);
        return t;
    };
    {
        SamHeader h;
        const SamRefTable t = parse_header("@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:one\tLN:10\n@CO\tSN:no\tLN:5\n@SQ\tM5:aa\tLN:2147483647\tUR:x\tSN:two\r\n@PG\tID:p\nread\t0\n", h);
        CHECK(h.defect == kSamOk && h.header_lines == 5 && h.ref_names.size() == 2 && h.ref_names[0] == "one" && h.ref_names[1] == "two");
        CHECK(h.ref_lengths[0] == 10 && h.ref_lengths[1] == 2147483647);
        const std::string three = "onetwothree";
        const uint8_t *p = (const uint8_t *)three.data();
        CHECK(sam_lookup_ref(t.view(), p, p + 3) == 0 && sam_lookup_ref(t.view(), p + 3, p + 6) == 1 && sam_lookup_ref(t.view(), p + 6, p + 11) == -1);
        CHECK(sam_lookup_ref(t.view(), p, p) == -1);
    }
    struct Case { const char *text; int code; int64_t line; };
    const Case cases[] = {
        {"@SQ\tLN:5\n", kSamSqNoName, 1},
        {"@HD\tVN:1\n@SQ\tSN:\tLN:5\n", kSamSqNoName, 2},
        {"@SQ\tSN:a\n", kSamSqNoLength, 1},
        {"@SQ\tSN:a\tLN:0\n", kSamSqBadLength, 1},
        {"@SQ\tSN:a\tLN:2147483648\n", kSamSqBadLength, 1},
        {"@SQ\tSN:a\tLN:12x\n", kSamSqBadLength, 1},
        {"@SQ\tSN:a\tLN:5\n@SQ\tSN:b\tLN:5\n@SQ\tLN:6\tSN:a\n", kSamSqDuplicate, 3},
        {"@HD\tVN:1\nread\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n", kSamNoReferences, 2},
        {"read\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*", kSamNoReferences, 1},
        {"@SQ\tSN:a\n@SQ\tLN:5\n", kSamSqNoLength, 1},            // the first defect is the file's
    };
    for (const Case &c : cases) {
        SamHeader h;
        parse_header(c.text, h);
        if (h.defect != c.code || h.defect_line != c.line) std::printf("  header '%s': code %d line %lld\n", c.text, h.defect, (long long)h.defect_line);
        CHECK(h.defect == c.code && h.defect_line == c.line);
    }
    for (const char *text : {"", "@HD\tVN:1\n", "@HD\tVN:1", "@SQ\tSN:a\tLN:5", "@SQ\tSN:a\tLN:5\n"}) {   // no records: fine, with or without references
        SamHeader h;
        parse_header(text, h);
        CHECK(h.defect == kSamOk && h.body_off == std::strlen(text));
    }
    // many references: the table grows, and finds every name
    std::string text;
    for (int k = 0; k < 3000; ++k) text += "@SQ\tSN:contig_" + std::to_string(k) + "\tLN:" + std::to_string(k + 1) + "\n";
    SamHeader h;
    const SamRefTable t = parse_header(text, h);
    CHECK(h.defect == kSamOk && h.ref_names.size() == 3000);
    for (int k = 0; k < 3000; k += 7) {
        const std::string nm = "contig_" + std::to_string(k);
        CHECK(sam_lookup_ref(t.view(), (const uint8_t *)nm.data(), (const uint8_t *)nm.data() + nm.size()) == k);
    }
    CHECK(sam_count_lines((const uint8_t *)"a\nb\n", (const uint8_t *)"a\nb\n" + 4) == 2);
    CHECK(sam_count_lines((const uint8_t *)"a\nb", (const uint8_t *)"a\nb" + 3) == 2);
    CHECK(sam_count_lines((const uint8_t *)"", (const uint8_t *)"") == 0);
    CHECK(sam_looks_compressed((const uint8_t *)"\x1f\x8b\x08", 3) && !sam_looks_compressed((const uint8_t *)"@HD", 3));
}

// the parser never reads outside [begin, end): every prefix of valid lines, and lines of 0xff bytes, from buffers that end
// exactly at `end` (the address sanitizer is the oracle)
static void test_bounds() {
    std::string cig;
    for (int k = 0; k < 40; ++k) cig += "3M2N";
    const std::string lines[] = {
        line("16", "chrB", "101", "37", "10M200N20M", "ACGTACGTACGTACGTACGTACGTACGTAC", "XS:A:-\tNH:i:3\tMD:Z:30"),
        line("0", "chrA", "7", "0", (cig + "1M").c_str(), "*", "NH:i:65535") + "\r",
        line("4", "*", "0", "0", "*", "*", "NH:i:-"),
    };
    long parsed = 0;
    for (const std::string &s : lines)
        for (size_t n = 0; n <= s.size(); ++n) {
            const SamRec r = parse(s.substr(0, n));
            parsed += 1;
            if (n == s.size()) CHECK(r.err == kSamOk);
            // the cigar field of a prefix, and its walk, stay inside the prefix too
            std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);
            if (n) std::memcpy(buf.get(), s.data(), n);
            const uint8_t *cb, *ce;
            sam_cigar_field(buf.get(), buf.get() + n, cb, ce);
            CHECK(cb >= buf.get() && ce <= buf.get() + n && cb <= ce);
            (void)sam_walk_cigar(cb, ce, 0, CigarNoEmit());
        }
    for (size_t n : {(size_t)1, (size_t)2, (size_t)63, (size_t)64, (size_t)65, (size_t)4096}) {
        const SamRec r = parse(std::string(n, (char)0xff));
        CHECK(r.err == kSamFewFields);
        std::string t(n, (char)0xff);
        for (size_t k = 3; k < n; k += 5) t[k] = '\t';              // 0xff fields
        const SamRec r2 = parse(t);
        CHECK(r2.err != kSamOk);
    }
    CHECK(parsed > 300);
}

int main() {
    const char *hdr = "@SQ\tSN:chrA\tLN:5000000\n@SQ\tSN:chrB\tLN:3000000\n@SQ\tSN:chrEnd\tLN:2147483647\n";
    SamHeader h;
    parse_sam_header((const uint8_t *)hdr, std::strlen(hdr), h, g_table);
    CHECK(h.defect == kSamOk && h.ref_names.size() == 3);
    test_fields();
    test_defects();
    test_nh();
    test_long_cigars();
    test_header();
    test_bounds();
    if (g_fail) { std::printf("sam_host: %d checks failed\n", g_fail); return 1; }
    std::printf("sam_host: ok\n");
    return 0;
}
