// dense_host_test.cpp -- plastid_amd/csrc/dense_host.h on a machine without a GPU (tests/test_dense_host.py compiles it
// under the address and undefined-behaviour sanitizers and runs it).
//   dense_host_test check          hand-worked extents, cell offsets and eligibility decisions; prints "dense_host: ok"
//   dense_host_test items FILE     one segment per line of FILE (out_off len clip_lo clip_hi start step known cell_base
//                                  ext); prints every item of every segment as "seg k out_off cell0 len step lo hi" --
//                                  the test compares them with its numpy model position by position
#include "dense_host.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace pcdense;

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static int check() {
    // extents: the larger of the declared length and the furthest aligned end; nothing known: 0
    CHECK(extent(0, 0) == 0);
    CHECK(extent(1, 0) == 1);
    CHECK(extent(0, 1) == 1);
    CHECK(extent(1000, 1200) == 1200);   // a read runs past the declared end
    CHECK(extent(1000, 999) == 1000);
    CHECK(extent(-5, -1) == 0);
    // cell offsets: contigs of extent 0, 1, 1200 (declared 1000, furthest end 1200) and 7
    const int64_t ext[4] = {extent(0, 0), extent(1, 0), extent(1000, 1200), extent(7, 3)};
    int64_t off[9];
    std::memset(off, 0xff, sizeof(off));
    CHECK(layout(4, ext, off) == 2 * (0 + 1 + 1200 + 7));
    const int64_t want[9] = {0, 0, 0, 1, 2, 1202, 2402, 2409, 2416};
    for (int k = 0; k < 9; ++k) CHECK(off[k] == want[k]);
    int64_t none[1] = {-1};
    CHECK(layout(0, ext, none) == 0 && none[0] == 0);
    // the size rule, on both sides of equality: 2 bytes per cell against 4 per stream entry
    CHECK(size_rule(200, 100));
    CHECK(!size_rule(201, 100));
    CHECK(size_rule(199, 100));
    CHECK(size_rule(2, 1) && !size_rule(3, 1));
    CHECK(!size_rule(0, 100));          // no cells: nothing to serve
    CHECK(!size_rule(1, 0));
    // the build's block: 8 bytes per cell within kBuildBlockCap
    CHECK(build_fits(kBuildBlockCap / 8) && !build_fits(kBuildBlockCap / 8 + 1));
    // the plan conditions
    PlanIn p;
    p.nfiles = 1; p.kind = PC_MAP_FIVE; p.rows = 1; p.modes = 3u; p.cells = 200; p.stream_entries = 100;
    CHECK(eligible(p));
    { PlanIn q = p; q.modes = 1u; CHECK(eligible(q)); q.modes = 2u; CHECK(eligible(q)); }
    { PlanIn q = p; q.modes = 0u; CHECK(!eligible(q)); }
    { PlanIn q = p; q.modes = 4u; CHECK(!eligible(q)); q.modes = 7u; CHECK(!eligible(q)); q.modes = 8u; CHECK(!eligible(q)); }   // a '.' window
    { PlanIn q = p; q.nfiles = 2; CHECK(!eligible(q)); }
    { PlanIn q = p; q.kind = PC_MAP_CENTER; CHECK(!eligible(q)); q.kind = PC_MAP_STRAT5; CHECK(!eligible(q)); q.kind = PC_MAP_THREE; CHECK(eligible(q)); q.kind = PC_MAP_VAR5; CHECK(eligible(q)); }
    { PlanIn q = p; q.rows = 11; CHECK(!eligible(q)); }
    { PlanIn q = p; q.has_sums = true; CHECK(!eligible(q)); }
    { PlanIn q = p; q.forbidden = true; CHECK(!eligible(q)); }
    { PlanIn q = p; q.cells = 201; CHECK(!eligible(q)); }
    { PlanIn q = p; q.cells = kBuildBlockCap / 8 + 1; q.stream_entries = q.cells; CHECK(!eligible(q)); }
    // items per segment
    CHECK(items_of(0) == 0 && items_of(1) == 1 && items_of(2047) == 1 && items_of(2048) == 1 && items_of(2049) == 2 && items_of(4097) == 3);
    if (failures) { fprintf(stderr, "dense_host: %d failure(s)\n", failures); return 1; }
    printf("dense_host: ok\n");
    return 0;
}

static int items(const char *path) {
    FILE *f = fopen(path, "r");
    if (!f) { perror(path); return 2; }
    SegIn s;
    int known = 0, step = 0;
    for (int seg = 0; fscanf(f, "%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %d %d %" SCNd64 " %" SCNd64, &s.out_off, &s.len, &s.clip_lo,
                             &s.clip_hi, &s.start, &step, &known, &s.cell_base, &s.ext) == 9; ++seg) {
        s.step = step; s.known = known != 0;
        std::vector<Item> its((size_t)items_of(s.len));   // (a heap block per segment: the sanitizer sees every write)
        for (int64_t k = 0; k < (int64_t)its.size(); ++k) its[(size_t)k] = cut_item(s, k);
        for (size_t k = 0; k < its.size(); ++k)
            printf("%d %zu %" PRId64 " %" PRId64 " %d %d %d %d\n", seg, k, its[k].out_off, its[k].cell0, its[k].len, its[k].step, its[k].lo, its[k].hi);
    }
    fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "check")) return check();
    if (argc == 3 && !std::strcmp(argv[1], "items")) return items(argv[2]);
    fprintf(stderr, "usage: dense_host_test check | items FILE\n");
    return 2;
}
