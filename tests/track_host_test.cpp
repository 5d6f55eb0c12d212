// CPU test of plastid_amd/csrc/track_host.h (no GPU, no HIP): the plain predicate and both converters against strtod at
// their boundaries (significands 2^53 - 1, 2^53, 2^53 + 1; net exponents +-22 and +-23; 18 and 19 integer digits),
// Python's int / float grammar, and the line contract on every prefix of sample lines from heap buffers that end exactly
// where the line ends (the sanitizers see a read one byte too far).  Built and run by tests/test_track_host.py.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "track_host.h"

using namespace pctrack;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                  \
    do {                                                                                  \
        if (!(cond)) { ++g_failed; printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static const uint8_t *U(const std::string &s) { return (const uint8_t *)s.data(); }

static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

// the token is plain and converts to what strtod gives / is not plain
static void expect_plain(const std::string &tok, bool plain) {
    double v = 0;
    const bool got = value_plain(U(tok), U(tok) + tok.size(), v);
    CHECK(got == plain, "%s: plain %d, expected %d", tok.c_str(), (int)got, (int)plain);
    if (got) {
        const double ref = std::strtod(tok.c_str(), nullptr);
        CHECK(same(v, ref), "%s: %.17g, strtod %.17g", tok.c_str(), v, ref);
    }
    double w = 0;
    CHECK(value_full(U(tok), U(tok) + tok.size(), w), "%s refused by value_full", tok.c_str());
    CHECK(same(w, std::strtod(tok.c_str(), nullptr)), "%s: value_full differs from strtod", tok.c_str());
}

// the digits of `sig` with a point `frac` digits from the right (frac <= digits), and an exponent
static std::string spell(uint64_t sig, int frac, int ex, bool with_e) {
    std::string d = std::to_string((unsigned long long)sig);
    while ((int)d.size() <= frac) d.insert(d.begin(), '0');
    if (frac > 0) d.insert(d.size() - (size_t)frac, ".");
    if (with_e) d += "e" + std::to_string(ex);
    return d;
}

static void test_values() {
    const uint64_t two53 = (uint64_t)1 << 53;
    for (uint64_t sig : {two53 - 1, two53, two53 + 1, (uint64_t)1, (uint64_t)3, (uint64_t)123456789, (uint64_t)99999999999999999ull}) {
        for (int frac = 0; frac <= 16; ++frac)
            for (int ex = -40; ex <= 40; ++ex) {
                const int net = ex - frac;
                const bool plain = sig <= two53 && net >= -22 && net <= 22;
                expect_plain(spell(sig, frac, ex, true), plain);
                expect_plain("-" + spell(sig, frac, ex, true), plain);
            }
        for (int frac = 0; frac <= 16; ++frac) expect_plain(spell(sig, frac, 0, false), sig <= two53 && frac <= 22);
    }
    // the edges by name
    expect_plain("1e22", true); expect_plain("1e23", false); expect_plain("1e-22", true); expect_plain("1e-23", false);
    expect_plain("9007199254740991", true); expect_plain("9007199254740992", true); expect_plain("9007199254740993", false);
    expect_plain("0009007199254740992", true);               // leading zeros are stripped
    expect_plain("9007199254740992.000", false);            // trailing zeros belong to the significand
    expect_plain("0.1", true); expect_plain("0.30000000000000004", false); expect_plain("-0.0", true); expect_plain("+5", true);
    expect_plain("0e0", true); expect_plain("0.000", true); expect_plain("1E5", true); expect_plain("1e+05", true);
    expect_plain("123456789012345678", false);              // 18 digits: beyond 17
    expect_plain("0.000000000000000000000001", false);       // net exponent -24
    expect_plain("1e0000000000000000000001", true);
    double v = 1;
    const std::string mz("-0.0"), us("1_0.5"), ninf("-Infinity"), nan("nan");
    CHECK(value_plain(U(mz), U(mz) + mz.size(), v) && std::signbit(v) && v == 0.0, "-0.0 keeps its sign");
    // random decimals of up to 15 significant digits are all plain, and right
    std::mt19937_64 rng(12345);
    for (int k = 0; k < 200000; ++k) {
        const int nd = 1 + (int)(rng() % 15);
        uint64_t sig = 0;
        for (int i = 0; i < nd; ++i) sig = sig * 10 + rng() % 10;
        const int frac = (int)(rng() % (unsigned)(nd + 1));
        const bool with_e = rng() % 4 == 0;
        const int ex = with_e ? (int)(rng() % 13) - 6 : 0;
        expect_plain(spell(sig, frac, ex, with_e), true);
    }
    // not plain, but Python floats: value_full takes them
    for (const char *t : {"1.", ".5", "1_0.5", "1e1_0", "inf", "-Infinity", "+INF", "nan", "NaN", "-nan", "1_000.000_1e-1_0", "1.e5", ".5e1"}) {
        const std::string s(t);
        double a = 0, b = 0;
        CHECK(!value_plain(U(s), U(s) + s.size(), a), "%s is not plain", t);
        CHECK(value_full(U(s), U(s) + s.size(), b), "%s is a Python float", t);
    }
    double x = 0;
    CHECK(value_full(U(us), U(us) + us.size(), x) && x == 10.5, "1_0.5");
    CHECK(value_full(U(ninf), U(ninf) + ninf.size(), x) && std::isinf(x) && x < 0, "-Infinity");
    CHECK(value_full(U(nan), U(nan) + nan.size(), x) && std::isnan(x), "nan");
    // refused by Python's float
    for (const char *t : {"", "+", "-", ".", "e5", "1e", "1e+", "1__0", "_1", "1_", "1._5", "1_.5", "0x10", "0x1p3", "1.5.2", "abc", "in", "infinit", "nane", "1 ",
                          "1e5.0", "--1", "1e_5", "١"}) {
        const std::string s(t);
        double a = 0;
        CHECK(!value_plain(U(s), U(s) + s.size(), a), "'%s' is not plain", t);
        CHECK(!value_full(U(s), U(s) + s.size(), a), "'%s' is not a Python float", t);
    }
}

static void test_ints() {
    struct { const char *t; bool fast, full; int64_t v; } cases[] = {
        {"0", true, true, 0}, {"007", true, true, 7}, {"+5", true, true, 5}, {"-12", true, true, -12},
        {"999999999999999999", true, true, 999999999999999999ll},           // 18 digits
        {"1000000000000000000", false, false, 0},                           // 19 digits
        {"0000000000000000000001", false, true, 1},                         // 22 digits, one significant
        {"1_0", false, true, 10}, {"0_0_8", false, true, 8}, {"-1_000", false, true, -1000},
        {"", false, false, 0}, {"+", false, false, 0}, {"1__0", false, false, 0}, {"_1", false, false, 0}, {"1_", false, false, 0}, {"0x1", false, false, 0},
        {"1.5", false, false, 0}, {"1e3", false, false, 0}, {"12a", false, false, 0}, {" 1", false, false, 0},
    };
    for (auto &c : cases) {
        const std::string s(c.t);
        int64_t a = -777, b = -777;
        const bool fast = int_fast(U(s), U(s) + s.size(), a), full = int_full(U(s), U(s) + s.size(), b);
        CHECK(fast == c.fast, "'%s': int_fast %d", c.t, (int)fast);
        CHECK(full == c.full, "'%s': int_full %d", c.t, (int)full);
        if (fast) CHECK(a == c.v, "'%s': int_fast %" PRId64, c.t, a);
        if (full) CHECK(b == c.v, "'%s': int_full %" PRId64, c.t, b);
    }
}

// the text in a heap block of exactly its size
static std::unique_ptr<uint8_t[]> exact(const std::string &s) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[s.size() ? s.size() : 1]);
    if (!s.empty()) std::memcpy(p.get(), s.data(), s.size());
    return p;
}

static void test_lines() {
    struct { const char *line; int cls, ntok; } cases[] = {
        {"", kSkip, 0}, {"   \t\r", kSkip, 0}, {"# chrA 1 2 3", kSkip, 5}, {"track type=bedGraph name=x", kTrackLine, 3},
        {"variableStep chrom=chrA span=2", kHeader, 3}, {"fixedStep chrom=chrA start=1 step=2 span=3", kHeader, 5},
        {"chrA\t1\t2\t3", kBed, 4}, {"chrA 1 2 3\r", kBed, 4}, {"  chrA   1  2  3  ", kBed, 4}, {"12 3", kData, 2}, {"7", kData, 1}, {"1 2 3", kData, 3},
        {"1 2 3 4 5", kData, 5}, {"1 2 3 4 5 6 7", kData, 5}, {" #x 1", kData, 2}, {"trackx 1 2 3", kBed, 4}, {"variableStepper", kData, 1},
    };
    for (auto &c : cases) {
        const std::string s(c.line);
        auto p = exact(s);
        const LineClass lc = classify_line(p.get(), p.get() + s.size());
        CHECK(lc.cls == c.cls && lc.ntok == c.ntok, "'%s': class %d tokens %d", c.line, lc.cls, lc.ntok);
    }
    // every prefix of these texts, from a block that ends at the prefix's last byte: the reader neither reads beyond it nor
    // yields anything but rows or a defect with a line inside the text
    const std::string texts[] = {
        "track type=bedGraph\nchrA\t10\t20\t3.5\nchrA\t20\t25\t1e-3\r\nchrB 1 2 nan\n",
        "variableStep chrom=chrA span=3\n11 3\n12 5.25\n# c\n\nfixedStep chrom=chrB start=5 step=2 span=1\n1\n2\n3 \nchrA 1_0 +20 007\n",
        "fixedStep chrom=chrA start=1 description=span=9\n0.12345678901234567\n9007199254740993e-30\n-inf\n",
    };
    for (const std::string &t : texts)
        for (size_t n = 0; n <= t.size(); ++n) {
            const std::string s = t.substr(0, n);
            auto p = exact(s);
            TrackTable tab;
            read_track(p.get(), s.size(), tab);
            const int64_t lines = (int64_t)std::count(s.begin(), s.end(), '\n') + ((s.empty() || s.back() == '\n') ? 0 : 1);
            CHECK(tab.lines <= lines, "prefix %zu: %" PRId64 " lines of %" PRId64, n, tab.lines, lines);
            if (tab.defect != kTrkOk) CHECK(tab.defect_line >= 1 && tab.defect_line <= lines, "prefix %zu: defect at line %" PRId64, n, tab.defect_line);
            else CHECK(tab.lines == lines, "prefix %zu: read %" PRId64 " lines of %" PRId64, n, tab.lines, lines);
            for (size_t r = 0; r < tab.start.size(); ++r) CHECK(tab.start[r] >= 0 && tab.contig[r] >= 0, "prefix %zu row %zu", n, r);
        }
    // the whole texts, by hand
    {
        TrackTable tab;
        read_track(U(texts[1]), texts[1].size(), tab);
        CHECK(tab.defect == kTrkOk, "defect %d at %" PRId64, tab.defect, tab.defect_line);
        const int64_t start[] = {10, 11, 4, 6, 8, 10}, stop[] = {13, 14, 5, 7, 9, 20};
        const double val[] = {3, 5.25, 1, 2, 3, 7};
        CHECK(tab.start.size() == 6, "%zu rows", tab.start.size());
        for (size_t r = 0; r < tab.start.size() && r < 6; ++r)
            CHECK(tab.start[r] == start[r] && tab.stop[r] == stop[r] && tab.value[r] == val[r], "row %zu: %" PRId64 " %" PRId64 " %g", r, tab.start[r], tab.stop[r], tab.value[r]);
        CHECK(tab.names.size() == 2 && tab.names[0] == "chrA" && tab.names[1] == "chrB", "names");
        CHECK(tab.states == 3 && tab.n_escaped == 1, "states %" PRId64 " escaped %" PRId64, tab.states, tab.n_escaped);
    }
    {
        TrackTable tab;
        read_track(U(texts[2]), texts[2].size(), tab);   // "description" ends the header: span stays 1
        CHECK(tab.defect == kTrkOk && tab.stop.size() == 3 && tab.stop[0] == 1 && tab.stop[2] == 3, "description stops the header scan");
        CHECK(tab.escaped[0] == 1 && tab.escaped[1] == 1 && tab.escaped[2] == 1, "three escaped values");
        CHECK(same(tab.value[1], std::strtod("9007199254740993e-30", nullptr)), "escaped value is strtod's");
    }
    // governing: the last record at or above the line
    StateRec recs[3];
    recs[0].line = 2; recs[1].line = 5; recs[2].line = 9;
    const int64_t want[] = {-1, -1, 0, 0, 0, 1, 1, 1, 1, 2, 2};
    for (int64_t l = 0; l < 11; ++l) CHECK(governing(recs, 3, l) == want[l], "governing(%" PRId64 ")", l);
    CHECK(governing(recs, 0, 4) == -1, "no records");
}

int main() {
    test_values();
    test_ints();
    test_lines();
    if (g_failed) { printf("track_host: %d checks FAILED\n", g_failed); return 1; }
    printf("track_host: ok\n");
    return 0;
}
