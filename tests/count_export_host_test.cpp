// The host side of the export of a counted plan (plastid_amd/csrc/track_table.h, track_host.h) as a stand-alone program
// (tests/test_count_export_host.py builds it under the address and undefined-behaviour sanitizers), without a GPU:
//   - count_batches: budgets of 1, exactly a contig, one less, larger than everything; a contig over the budget alone;
//     the refusal beyond 2^32 - 1 positions;
//   - count_ranges: the range table of a batch, ranges outside the output refused;
//   - the phases of the device export replayed serially -- run-head flags and kept runs by the predicates the kernels
//     run (count_is_head, count_is_line), exclusive sum, select, the runs in front of every range -- and every line
//     written through count_line_of and the put_count_* line functions, against the serial writers: the line -> run ->
//     range mapping, for int64 and float64 cells, and for more ranges than 16 bits count.
#include "track_table.h"

#include <cinttypes>
#include <cstdio>

using namespace pctrack;

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failed; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// ---------------------------------------------------------------- batches

static std::vector<int32_t> batches(const std::vector<int64_t> &len, int64_t budget, int &nb, std::string &msg) {
    std::vector<int32_t> b(len.size() + 1, -1);
    nb = count_batches((int64_t)len.size(), len.data(), budget, b.data(), msg);
    b.resize(len.size());
    return b;
}

// every batch holds at most `budget` elements, or one contig with positions; the ids ascend without a gap; a contig never
// opens a batch it would have fitted in front of
static void check_batch_rules(const std::vector<int64_t> &len, int64_t budget) {
    int nb = 0;
    std::string msg;
    const std::vector<int32_t> b = batches(len, budget, nb, msg);
    CHECK(msg.empty(), "budget %lld: %s", (long long)budget, msg.c_str());
    std::vector<int64_t> sum((size_t)nb, 0), live((size_t)nb, 0);
    for (size_t k = 0; k < len.size(); ++k) {
        CHECK(b[k] >= 0 && b[k] < nb && (k == 0 ? b[k] == 0 : (b[k] == b[k - 1] || b[k] == b[k - 1] + 1)), "budget %lld: contig %zu in batch %d of %d", (long long)budget, k, b[k], nb);
        if (b[k] < 0 || b[k] >= nb) return;
        sum[(size_t)b[k]] += len[k] > 0 ? len[k] : 0;
        live[(size_t)b[k]] += len[k] > 0 ? 1 : 0;
        if (k > 0 && b[k] == b[k - 1] + 1)
            CHECK(sum[(size_t)b[k - 1]] + (len[k] > 0 ? len[k] : 0) > budget, "budget %lld: contig %zu would have fitted into batch %d", (long long)budget, k, b[k - 1]);
    }
    for (int i = 0; i < nb; ++i) CHECK(sum[(size_t)i] <= budget || live[(size_t)i] == 1, "budget %lld: batch %d holds %lld elements of %lld contigs", (long long)budget, i, (long long)sum[(size_t)i], (long long)live[(size_t)i]);
    CHECK(len.empty() ? nb == 0 : nb == b.back() + 1, "budget %lld: %d batches", (long long)budget, nb);
}

static void test_batches() {
    const std::vector<int64_t> len{5000, 3000, 900, 1};
    int nb = 0;
    std::string msg;
    CHECK(batches(len, 1, nb, msg) == (std::vector<int32_t>{0, 1, 2, 3}) && nb == 4, "budget 1: every contig alone");
    CHECK(batches(len, 3000, nb, msg) == (std::vector<int32_t>{0, 1, 2, 2}) && nb == 3, "budget 3000: 5000 alone, 3000 fills one, 900 + 1");
    CHECK(batches(len, 2999, nb, msg) == (std::vector<int32_t>{0, 1, 2, 2}) && nb == 3, "budget 2999: 5000 and 3000 over budget, alone");
    CHECK(batches(len, 8000, nb, msg) == (std::vector<int32_t>{0, 0, 1, 1}) && nb == 2, "budget 8000: exactly the first two");
    CHECK(batches(len, 7999, nb, msg) == (std::vector<int32_t>{0, 1, 1, 1}) && nb == 2, "budget 7999: one less");
    CHECK(batches(len, 8901, nb, msg) == (std::vector<int32_t>{0, 0, 0, 0}) && nb == 1, "budget 8901: exactly everything");
    CHECK(batches(len, 8900, nb, msg) == (std::vector<int32_t>{0, 0, 0, 1}) && nb == 2, "budget 8900: one less than everything");
    CHECK(batches(len, kCountBudget, nb, msg) == (std::vector<int32_t>{0, 0, 0, 0}) && nb == 1, "the default budget");
    CHECK(batches({}, 10, nb, msg).empty() && nb == 0 && msg.empty(), "no contig, no batch");
    CHECK(batches({0, 0}, 10, nb, msg) == (std::vector<int32_t>{0, 0}) && nb == 1, "contigs without positions share a batch");
    batches(len, 0, nb, msg);
    CHECK(!msg.empty() && nb == 0, "a budget of 0 is refused");
    batches({7, kCountBatchMax}, 10, nb, msg);
    CHECK(msg.empty() && nb == 2, "2^32 - 1 positions are fine: %s", msg.c_str());
    batches({7, kCountBatchMax + 1}, 10, nb, msg);
    CHECK(!msg.empty() && msg.find("32 bits") != std::string::npos, "beyond 2^32 - 1 positions is refused: %s", msg.c_str());
    uint64_t seed = 12345;
    for (int round = 0; round < 200; ++round) {
        std::vector<int64_t> v;
        const int n = (int)((seed = seed * 6364136223846793005ull + 1442695040888963407ull) >> 60);
        for (int k = 0; k < n; ++k) v.push_back((int64_t)(((seed = seed * 6364136223846793005ull + 1442695040888963407ull) >> 33) % 50) - 5);
        for (int64_t budget : {1, 2, 7, 44, 45, 1000}) check_batch_rules(v, budget);
    }
    check_batch_rules(len, 3000);
}

// ---------------------------------------------------------------- ranges

static void test_ranges() {
    const char *names[4] = {"chrA", "b", "", "chrD"};
    const int64_t off[4] = {10, 0, 3, 40}, len[4] = {5, 0, 2, 60};
    std::string msg;
    const ExportRanges x = count_ranges(4, names, off, len, 100, msg);
    CHECK(msg.empty() && x.ranges.size() == 5 && x.cells == 67, "count_ranges: %s, %zu ranges, %lld cells", msg.c_str(), x.ranges.size(), (long long)x.cells);
    if (x.ranges.size() == 5) {
        CHECK(x.ranges[0].e0 == 0 && x.ranges[1].e0 == 5 && x.ranges[2].e0 == 5 && x.ranges[3].e0 == 7 && x.ranges[4].e0 == 67, "the export elements are the running sum");
        CHECK(x.ranges[0].cell0 == 10 && x.ranges[2].cell0 == 3 && x.ranges[3].cell0 == 40 && x.ranges[3].n == 60 && x.ranges[1].n == 0, "first output element and length");
        CHECK(std::string(x.names.begin(), x.names.end()) == "chrAbchrD" && x.ranges[3].name_off == 5 && x.ranges[3].name_len == 4 && x.ranges[2].name_len == 0, "the names");
        for (int64_t e = 0; e < 67; ++e) {
            const int want = e < 5 ? 0 : e < 7 ? 2 : 3;
            CHECK(ex_range_of(x.ranges.data(), 4, e) == want, "ex_range_of(%lld)", (long long)e);
        }
    }
    const int64_t far[1] = {41};
    count_ranges(1, names, far, len + 3, 100, msg);
    CHECK(!msg.empty(), "a range beyond the output is refused");
    const int64_t neg[1] = {-1};
    count_ranges(1, names, neg, len, 100, msg);
    CHECK(!msg.empty(), "a range in front of the output is refused");
    count_ranges(1, names, neg, len + 1, 100, msg);
    CHECK(msg.empty(), "an empty range reads nothing: %s", msg.c_str());
}

// ---------------------------------------------------------------- the device phases, serially

template <typename T> struct Contig { std::string name; std::vector<T> v; };

// the text the device export gives for these contigs laid out in one plan output (with gaps between the ranges)
template <typename T> static std::string replay(int kind, int64_t period, const std::vector<Contig<T>> &contigs, ExportStats &st) {
    std::vector<T> out;
    std::vector<int64_t> off, len;
    std::vector<const char *> names;
    for (const Contig<T> &c : contigs) {
        out.push_back((T)77);                                         // (never read: between the ranges)
        off.push_back((int64_t)out.size()); len.push_back((int64_t)c.v.size()); names.push_back(c.name.c_str());
        out.insert(out.end(), c.v.begin(), c.v.end());
    }
    std::string msg;
    ExportRanges xr = count_ranges((int)contigs.size(), names.data(), off.data(), len.data(), (int64_t)out.size(), msg);
    CHECK(msg.empty(), "replay: %s", msg.c_str());
    const int K = (int)contigs.size();
    const int64_t E = xr.cells;
    std::string text;
    if (K == 0 || (kind == 0 && E == 0)) return text;
    // phase 1: run-head flags (k_counts_flags); phase 2: exclusive sum, run table, runs in front of every range
    const uint32_t p32 = count_period32(kind, period);
    std::vector<uint32_t> flags((size_t)E), idx((size_t)E), run_e, line_run;
    for (int64_t e = 0; e < E; ++e) {
        const ExRange r = xr.ranges[(size_t)ex_range_of(xr.ranges.data(), K, e)];
        flags[(size_t)e] = count_is_head(kind, p32, out.data() + r.cell0, e - r.e0) ? 1u : 0u;
    }
    uint32_t acc = 0;
    for (int64_t e = 0; e < E; ++e) { idx[(size_t)e] = acc; acc += flags[(size_t)e]; }
    run_e.resize(acc);
    for (int64_t e = 0; e < E; ++e) if (flags[(size_t)e]) run_e[idx[(size_t)e]] = (uint32_t)e;
    for (int k = 0; k <= K; ++k) xr.ranges[(size_t)k].run_base = xr.ranges[(size_t)k].e0 < E ? (int64_t)idx[(size_t)xr.ranges[(size_t)k].e0] : (int64_t)acc;
    const int64_t R = (int64_t)acc;
    // phase 3 (bedGraph): the runs whose value is > 0 are the lines
    int64_t nlines = R + K;
    if (kind == 0) {
        for (int64_t r = 0; r < R; ++r) {
            const int64_t e = (int64_t)run_e[(size_t)r];
            const ExRange g = xr.ranges[(size_t)ex_range_of(xr.ranges.data(), K, e)];
            if (count_is_line(out[(size_t)(g.cell0 + (e - g.e0))])) line_run.push_back((uint32_t)r);
        }
        nlines = (int64_t)line_run.size();
    }
    if (run_e.empty()) run_e.push_back(0);
    if (line_run.empty()) line_run.push_back(0);
    // phases 5, 6: every line through the mapping, counted and stored
    char buf[kReprMax + 8];
    for (int64_t L = 0; L < nlines; ++L) {
        const CountLine c = count_line_of(kind, xr.ranges.data(), K, run_e.data(), line_run.data(), L);
        const ExRange g = xr.ranges[(size_t)c.k];
        const uint8_t *name = xr.names.data() + g.name_off;
        CountSink cs;
        StringSink ss{&text};
        const size_t before = text.size();
        if (c.header) { put_var_header(cs, name, g.name_len); put_var_header(ss, name, g.name_len); }
        else {
            CHECK(c.j >= 0 && c.j < g.n && c.end > c.j && c.end <= g.n, "line %lld: element %lld .. %lld of %lld", (long long)L, (long long)c.j, (long long)c.end, (long long)g.n);
            const T v = out[(size_t)(g.cell0 + c.j)];
            const uint8_t *vt; int vl;
            host_count_value(v, buf, vt, vl, st);
            if (kind == 0) { put_count_bed_line(cs, name, g.name_len, c.j, c.end, v, vt, vl); put_count_bed_line(ss, name, g.name_len, c.j, c.end, v, vt, vl); }
            else { put_count_var_line(cs, c.j, v, vt, vl); put_count_var_line(ss, c.j, v, vt, vl); }
        }
        CHECK((size_t)cs.n == text.size() - before, "line %lld: the counting sink saw %lld bytes of %zu", (long long)L, (long long)cs.n, text.size() - before);
    }
    st.lines = nlines; st.runs = R; st.bytes = (int64_t)text.size();
    return text;
}

template <typename T> static void compare(const char *what, const std::vector<Contig<T>> &contigs, bool few_windows = false) {
    int64_t longest = 1;
    for (const Contig<T> &c : contigs) longest = std::max<int64_t>(longest, (int64_t)c.v.size());
    std::vector<int64_t> periods{1, 2, 3, 7, longest - 1 > 0 ? longest - 1 : 1, longest, longest + 1, 100000, (int64_t)1 << 40};
    if (few_windows) periods = {1, 100000};
    for (int kind = 0; kind < 2; ++kind)
        for (int64_t period : periods) {
            std::string want;
            ExportStats ws, gs;
            for (const Contig<T> &c : contigs) {
                if (kind == 0) write_count_bedgraph_contig(want, c.name, c.v.data(), (int64_t)c.v.size(), period, ws);
                else write_count_variable_step_contig(want, c.name, c.v.data(), (int64_t)c.v.size(), ws);
            }
            const std::string got = replay(kind, period, contigs, gs);
            CHECK(got == want, "%s, kind %d, window %lld:\n--- replayed\n%s--- serial writer\n%s", what, kind, (long long)period, got.c_str(), want.c_str());
            CHECK(gs.lines == ws.lines && gs.runs == ws.runs && gs.listed == ws.listed && gs.bytes == ws.bytes, "%s, kind %d, window %lld: stats %lld %lld %lld %lld, not %lld %lld %lld %lld",
                  what, kind, (long long)period, (long long)gs.lines, (long long)gs.runs, (long long)gs.listed, (long long)gs.bytes, (long long)ws.lines, (long long)ws.runs,
                  (long long)ws.listed, (long long)ws.bytes);
        }
}

static void test_lines() {
    std::string text;
    ExportStats st;
    const std::vector<int64_t> v{0, 3, 3, 0, 0, 10, 10, 10, 99, 100, 1000000000000000ll, 0};
    write_count_bedgraph_contig(text, "c", v.data(), (int64_t)v.size(), 7, st);
    CHECK(text == "c\t1\t3\t3\nc\t5\t7\t10\nc\t7\t8\t10\nc\t8\t9\t99\nc\t9\t10\t100\nc\t10\t11\t1000000000000000\n", "the bedGraph of a designed vector:\n%s", text.c_str());
    CHECK(st.lines == 6 && st.runs == 9 && st.listed == 0 && st.bytes == (int64_t)text.size(), "its stats: %lld lines, %lld runs", (long long)st.lines, (long long)st.runs);
    text.clear();
    const std::vector<double> f{0.5, 0.5, 1e-05, 1.0 / 3.0, 1e16, 3.0, 0.0};
    ExportStats sf;
    write_count_variable_step_contig(text, "chr", f.data(), (int64_t)f.size(), sf);
    CHECK(text == "variableStep chrom=chr span=1\n1\t0.5\n2\t0.5\n3\t1e-05\n4\t0.3333333333333333\n5\t1e+16\n6\t3.0\n", "the variableStep of float cells:\n%s", text.c_str());
    CHECK(sf.lines == 7 && sf.runs == 6 && sf.listed == 5, "its stats: %lld listed", (long long)sf.listed);

    std::vector<Contig<int64_t>> ci{{"chr2", {0, 0, 5, 5, 5, 0, 9, 10, 10, 0}}, {"empty", {}}, {"zeros", {0, 0, 0, 0}}, {"one", {4}}, {"two", {1, 1}},
                                    {"chr10", {7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7}}, {"last", {0, 0, 1}}};
    compare("int64 cells", ci);
    compare<int64_t>("one contig without positions", {{"e", {}}});
    compare<int64_t>("no contig", {});
    std::vector<Contig<double>> cf{{"a", {0.0, 0.5, 0.5, 1e-05, 1.0 / 3.0, 1e16, 3.0, 3.0, 0.0, 2.5}}, {"z", {0.0, 0.0}}, {"", {}}, {"b", {1e6 / 7.0, 1e6 / 7.0, 2e6 / 7.0}}};
    compare("float64 cells", cf);
    // more ranges than 16 bits count: 70 000 contigs of 0 .. 2 positions (a transcriptome, a scaffold-level assembly)
    std::vector<Contig<int64_t>> many;
    for (int k = 0; k < 70000; ++k) {
        Contig<int64_t> x;
        x.name = "t" + std::to_string(k);
        for (int i = 0; i < k % 3; ++i) x.v.push_back((int64_t)((k / 3 + i) % 4));
        many.push_back(x);
    }
    compare("70 000 contigs", many, true);
    {
        std::vector<int64_t> ones(70000, 1);
        int nb = 0;
        std::string msg;
        const std::vector<int32_t> b = batches(ones, kCountBudget, nb, msg);
        CHECK(msg.empty() && nb == 1 && b.back() == 0, "70 000 contigs of one position are one batch: %d, %s", nb, msg.c_str());
    }
    uint64_t seed = 99;
    for (int round = 0; round < 40; ++round) {
        std::vector<Contig<int64_t>> c;
        const int n = 1 + (int)((seed = seed * 6364136223846793005ull + 1442695040888963407ull) >> 62);
        for (int k = 0; k < n; ++k) {
            Contig<int64_t> x;
            x.name = "s" + std::to_string(k);
            const int len = (int)(((seed = seed * 6364136223846793005ull + 1442695040888963407ull) >> 40) % 40);
            for (int i = 0; i < len; ++i) x.v.push_back((int64_t)(((seed = seed * 6364136223846793005ull + 1442695040888963407ull) >> 45) % 3));
            c.push_back(x);
        }
        compare("seeded cells", c);
    }
}

int main() {
    test_batches();
    test_ranges();
    test_lines();
    if (g_failed) { printf("count_export_host: %d checks FAILED\n", g_failed); return 1; }
    printf("count_export_host: ok\n");
    return 0;
}
