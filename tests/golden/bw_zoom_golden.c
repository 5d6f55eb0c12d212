/* Harness of tests/golden/make_bigwig_zoom_golden.py: the summary reader of Kent's bigWig library (the library the reference
 * links, kent/src/lib) on files with OUR zoom levels.  Runs in the build container only; nothing of it is committed but
 * this file.
 *
 *   bw_zoom_golden FILE.bw CHROM START END BINS
 *       LEVELS <n> <reduction> ...          the zoom levels bbiFileOpen found
 *       <type> <value> x BINS               bigWigSummaryArray for mean, min, max, coverage and std; a bin the call left
 *                                           untouched prints as nan
 * Values print as %.17g. */
#include "common.h"
#include "bbiFile.h"
#include "bigWig.h"

int main(int argc, char **argv) {
    if (argc != 6) errAbort("usage: bw_zoom_golden FILE.bw CHROM START END BINS");
    struct bbiFile *bbi = bigWigFileOpen(argv[1]);
    unsigned start = (unsigned)strtoul(argv[3], NULL, 10), end = (unsigned)strtoul(argv[4], NULL, 10);
    int bins = atoi(argv[5]), i, t;
    struct bbiZoomLevel *z;
    printf("LEVELS %d", slCount(bbi->levelList));
    for (z = bbi->levelList; z != NULL; z = z->next) printf(" %u", z->reductionLevel);
    printf("\n");
    enum bbiSummaryType types[5] = {bbiSumMean, bbiSumMin, bbiSumMax, bbiSumCoverage, bbiSumStandardDeviation};
    const char *names[5] = {"mean", "min", "max", "coverage", "std"};
    double *values = needMem(sizeof(double) * bins);
    for (t = 0; t < 5; ++t) {
        for (i = 0; i < bins; ++i) values[i] = NAN;
        bigWigSummaryArray(bbi, argv[2], start, end, types[t], bins, values);
        printf("%s", names[t]);
        for (i = 0; i < bins; ++i) printf(" %.17g", values[i]);
        printf("\n");
    }
    bbiFileClose(&bbi);
    return 0;
}
