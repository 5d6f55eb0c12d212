// The export half of plastid_amd/csrc/track_host.h as a stand-alone program (tests/test_track_export_host.py builds it under
// the address and undefined-behaviour sanitizers): float_repr on its boundaries -- every text must read back through strtod
// as the same bits and keep Python's layout -- the serial writers over arrays with runs at position 0 and at the last
// cell, and over the golden cases of the file named on the command line (written by the test from
// tests/golden/track_export_fixture.npz: cells as hex floats, expected texts as hex bytes).
#include "track_host.h"

#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <sstream>

using namespace pctrack;

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failed; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static std::string repr_of(double v) {
    // (exactly kReprMax bytes on the heap: a formatter that writes one byte too many is caught)
    std::vector<char> buf((size_t)kReprMax);
    const int n = float_repr(v, buf.data());
    return std::string(buf.data(), (size_t)n);
}

static void check_value(double v) {
    const std::string s = repr_of(v);
    CHECK(s.size() >= 3 && s.size() <= (size_t)kReprMax, "length of %s", s.c_str());
    if (v != v) { CHECK(s == "nan", "nan prints as %s", s.c_str()); return; }
    char *end = nullptr;
    const double back = std::strtod(s.c_str(), &end);
    CHECK(end && *end == 0, "%s is not a number", s.c_str());
    uint64_t a, b;
    memcpy(&a, &v, 8); memcpy(&b, &back, 8);
    CHECK(a == b, "%s reads back as other bits (%016" PRIx64 " vs %016" PRIx64 ")", s.c_str(), b, a);
    if (v - v != 0.0) return;   // inf
    const double m = v < 0 ? -v : v;
    const bool expo = s.find('e') != std::string::npos;
    CHECK(expo == (m != 0.0 && (m < 1e-4 || m >= 1e16)), "layout of %s", s.c_str());
    if (!expo) CHECK(s.find('.') != std::string::npos, "%s has no point", s.c_str());
    // a plain value is what the kernel prints: the counted length equals the text's
    if (value_class(v) == kValPlain) {
        CountSink c;
        put_simple_value(c, v);
        CHECK(c.n == (int64_t)s.size(), "counted %lld bytes for %s", (long long)c.n, s.c_str());
    }
}

static std::string bed(const std::string &name, const std::vector<double> &v, ExportStats &st) {
    std::string out;
    // (the cells in a heap block of their exact size)
    std::vector<double> exact(v);
    write_bedgraph_contig(out, name, exact.data(), (int64_t)exact.size(), st);
    return out;
}
static std::string var(const std::string &name, const std::vector<double> &v, ExportStats &st) {
    std::string out;
    std::vector<double> exact(v);
    write_variable_step_contig(out, name, exact.data(), (int64_t)exact.size(), st);
    return out;
}

static std::string unhex(const std::string &h) {
    std::string out;
    for (size_t k = 0; k + 1 < h.size(); k += 2) out.push_back((char)std::stoi(h.substr(k, 2), nullptr, 16));
    return out;
}

static void golden(const char *path) {
    std::ifstream in(path);
    CHECK(in.good(), "cannot read %s", path);
    std::string line, name, strand, got_bed, got_var;
    int ncase = 0, ntext = 0;
    ExportStats st;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string word;
        ls >> word;
        if (word == "case") { ls >> name >> strand; got_bed.clear(); got_var.clear(); ntext = 0; ++ncase; }
        else if (word == "contig") {
            std::string hexname;
            long long n = 0;
            ls >> hexname >> n;
            std::getline(in, line);
            std::vector<double> v;
            std::istringstream vs(line);
            std::string tok;
            while (vs >> tok) v.push_back(std::strtod(tok.c_str(), nullptr));
            CHECK((long long)v.size() == n, "%s: %zu cells of %lld", name.c_str(), v.size(), n);
            write_bedgraph_contig(got_bed, unhex(hexname), v.data(), (int64_t)v.size(), st);
            write_variable_step_contig(got_var, unhex(hexname), v.data(), (int64_t)v.size(), st);
            for (double x : v) if (x != 0.0) check_value(x);
        } else if (word == "text") {
            std::string h;
            ls >> h;
            const std::string &got = ntext == 0 ? got_bed : got_var;
            CHECK(unhex(h) == got, "%s %s: %s differs", name.c_str(), strand.c_str(), ntext == 0 ? "bedGraph" : "variableStep");
            ++ntext;
        }
    }
    CHECK(ncase > 0, "no golden case in %s", path);
    printf("golden: %d case strands, %lld lines\n", ncase, (long long)st.lines);
}

int main(int argc, char **argv) {
    // the growth rule
    CHECK(grown_length(300, 299) == 300 && grown_length(300, 300) == 10300 && grown_length(300, 450) == 10450 && grown_length(0, 0) == 10000, "grown_length");
    // the formatter
    const double edge[] = {0.0, -0.0, 1.0, -1.0, 3.0, 0.1, 1.0 / 3.0, 1e15, 1e16, 9999999999999998.0, 9007199254740991.0, 9007199254740992.0, 1e-4, 1e-5,
                           9.999999999999999e-05, 5e-324, 1.7976931348623157e308, -1.7976931348623157e308, -7.0, 999999999999999.9, 1e22, 1e23, 123456.789,
                           2.2250738585072014e-308, -2.2250738585072011e-308, 1.5e16, -1.5e-7, HUGE_VAL, -HUGE_VAL, std::strtod("nan", nullptr), 0.5, 100.0};
    for (double v : edge) check_value(v);
    CHECK(repr_of(3.0) == "3.0" && repr_of(-0.0) == "-0.0" && repr_of(1e16) == "1e+16" && repr_of(1e15) == "1000000000000000.0", "plain layouts");
    CHECK(repr_of(1e-5) == "1e-05" && repr_of(1e-4) == "0.0001" && repr_of(1.5e16) == "1.5e+16" && repr_of(5e-324) == "5e-324", "exponent layouts");
    CHECK(repr_of(-1.7976931348623157e308) == "-1.7976931348623157e+308" && repr_of(HUGE_VAL) == "inf" && repr_of(-HUGE_VAL) == "-inf", "long and special");
    uint64_t x = 88172645463325252ull;
    for (int k = 0; k < 200000; ++k) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        double v;
        memcpy(&v, &x, 8);
        check_value(v);
    }
    // the writers: runs at position 0 and at the last cell, a single cell, nothing at all
    ExportStats st;
    CHECK(bed("c", {2, 2, 0, 0, 5}, st) == "c\t0\t0\t0\nc\t0\t2\t2.0\nc\t2\t4\t0.0\nc\t4\t5\t5.0\n", "runs at both ends: %s", bed("c", {2, 2, 0, 0, 5}, st).c_str());
    CHECK(bed("c", {0, 0, 0, 0, 0.5}, st) == "c\t0\t4\t0\nc\t4\t5\t0.5\n", "a run at the last cell");
    CHECK(bed("c", {7}, st) == "c\t0\t0\t0\nc\t0\t1\t7.0\n", "one cell");
    CHECK(bed("c", {}, st).empty() && bed("c", {0, -0.0}, st).empty() && bed("c", {1, -1}, st).empty() && bed("c", {1, -3}, st).empty(), "nothing to write");
    CHECK(bed("c", {1, std::strtod("nan", nullptr)}, st).empty(), "a NaN sum writes nothing");
    CHECK(bed("c", {3, -0.0, 0.0, 3}, st) == "c\t0\t0\t0\nc\t0\t1\t3.0\nc\t1\t3\t-0.0\nc\t3\t4\t3.0\n", "-0.0 heads a zero run");
    CHECK(var("c", {2, 0, 0, 0, 5}, st) == "variableStep chrom=c span=1\n1\t2.0\n5\t5.0\n", "variableStep at both ends");
    CHECK(var("c", {}, st) == "variableStep chrom=c span=1\n" && var("c", {0, -0.0}, st) == "variableStep chrom=c span=1\n", "a header alone");
    const double nan = std::strtod("nan", nullptr);
    CHECK(var("c", {nan, nan, HUGE_VAL}, st) == "variableStep chrom=c span=1\n1\tnan\n2\tnan\n3\tinf\n", "NaN cells are their own lines");
    if (argc > 1) golden(argv[1]);
    if (g_failed) { printf("track_export_host: %d checks failed\n", g_failed); return 1; }
    printf("track_export_host: ok\n");
    return 0;
}
