// dense_batches_test.cpp -- the pair and batch arithmetic of plastid_amd/csrc/dense_host.h (pair_cut, pair_slot,
// batches_of) on a machine without a GPU; tests/test_dense_batches.py compiles it under the address and
// undefined-behaviour sanitizers and runs it.
//   dense_batches_test pairs FILE    one item per line of FILE (out_off step len); prints every store of every item as
//                                    "item width element position [element position]" -- width 1: the head or the tail,
//                                    width 2: a pair, lower element first -- in the order head, pairs, tail
//   dense_batches_test batch         items per batch
//   dense_batches_test batches N..   for every N: "N batches" and then "first count" of every batch of an N-item plan
#include "dense_host.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace pcdense;

static int pairs(const char *path) {
    FILE *f = fopen(path, "r");
    if (!f) { perror(path); return 2; }
    int64_t out_off = 0;
    int step = 0, len = 0;
    for (int item = 0; fscanf(f, "%" SCNd64 " %d %d", &out_off, &step, &len) == 3; ++item) {
        const PairCut c = pair_cut(out_off, step, len);
        if (c.head) printf("%d 1 %" PRId64 " 0\n", item, out_off);
        std::vector<int64_t> slots((size_t)c.pairs);   // (a heap block per item: the sanitizer sees every write)
        for (int p = 0; p < c.pairs; ++p) slots[(size_t)p] = pair_slot(out_off, step, c, p);
        for (int p = 0; p < c.pairs; ++p) {
            const int i0 = c.head + 2 * p;
            printf("%d 2 %" PRId64 " %d %" PRId64 " %d\n", item, slots[(size_t)p], step > 0 ? i0 : i0 + 1, slots[(size_t)p] + 1, step > 0 ? i0 + 1 : i0);
        }
        if (c.tail) printf("%d 1 %" PRId64 " %d\n", item, out_off + (int64_t)step * (len - 1), len - 1);
    }
    fclose(f);
    return 0;
}

static int batches(int argc, char **argv) {
    for (int a = 2; a < argc; ++a) {
        const int64_t n = strtoll(argv[a], nullptr, 10), nb = batches_of(n);
        printf("%" PRId64 " %" PRId64 "\n", n, nb);
        for (int64_t g = 0; g < nb; ++g) {
            const int64_t first = g * kBatch, count = n - first < kBatch ? n - first : kBatch;
            printf("%" PRId64 " %" PRId64 "\n", first, count);
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !std::strcmp(argv[1], "pairs")) return pairs(argv[2]);
    if (argc >= 3 && !std::strcmp(argv[1], "batches")) return batches(argc, argv);
    if (argc == 2 && !std::strcmp(argv[1], "batch")) { printf("%d\n", kBatch); return 0; }
    fprintf(stderr, "usage: dense_batches_test pairs FILE | batch | batches N...\n");
    return 2;
}
