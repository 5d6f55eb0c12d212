/* Harness of tests/golden/make_bigwig_golden.py: Kent's own bigWig writer and readers (the library the reference links,
 * kent/src/lib) on files of the fixture.  Runs in the build container only; nothing of it is committed but this file.
 *
 *   bw_golden write IN.wig CHROM.sizes BLOCKSIZE ITEMSPERSLOT COMPRESS OUT.bw     bigWigFileCreate
 *   bw_golden read FILE.bw NREG SEED
 *       CHROM <name> <id> <size>            bbiChromList, in its order
 *       BLOCK <chrom> <offset> <size>       the unzoomed blocks of every contig (bbiOverlappingBlocks over the contig)
 *       RUN <chrom> <start> <end> <value>   bigWigValsOnChromFetchData: the runs of equal non-zero value of valBuf
 *       REG <chrom> <start> <end> <n>       a seeded region, then its n intervals of bigWigIntervalQuery:
 *       IV <start> <end> <value>
 * Values print as %.17g (float32 widened: exact). */
#include "common.h"
#include "localmem.h"
#include "bbiFile.h"
#include "bigWig.h"
#include "cirTree.h"

static unsigned long long rng_state;
static unsigned rng(void) {
    rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (unsigned)(rng_state >> 33);
}

int main(int argc, char **argv) {
    if (argc == 8 && sameString(argv[1], "write")) {
        bigWigFileCreate(argv[2], argv[3], atoi(argv[4]), atoi(argv[5]), FALSE, atoi(argv[6]) != 0, argv[7]);
        return 0;
    }
    if (argc != 5 || !sameString(argv[1], "read")) errAbort("usage: bw_golden write ... | read FILE NREG SEED");
    struct bbiFile *bbi = bigWigFileOpen(argv[2]);
    int nreg = atoi(argv[3]);
    rng_state = (unsigned long long)atoll(argv[4]);
    struct bbiChromInfo *chrom, *chroms = bbiChromList(bbi);
    int nchrom = 0;
    for (chrom = chroms; chrom != NULL; chrom = chrom->next, ++nchrom) printf("CHROM %s %u %u\n", chrom->name, chrom->id, chrom->size);
    bbiAttachUnzoomedCir(bbi);
    for (chrom = chroms; chrom != NULL; chrom = chrom->next) {
        struct fileOffsetSize *b, *blocks = bbiOverlappingBlocks(bbi, bbi->unzoomedCir, chrom->name, 0, chrom->size, NULL);
        for (b = blocks; b != NULL; b = b->next) printf("BLOCK %s %llu %llu\n", chrom->name, (unsigned long long)b->offset, (unsigned long long)b->size);
        slFreeList(&blocks);
    }
    struct bigWigValsOnChrom *vals = bigWigValsOnChromNew();
    for (chrom = chroms; chrom != NULL; chrom = chrom->next) {
        if (!bigWigValsOnChromFetchData(vals, chrom->name, bbi)) continue;
        long i = 0, n = vals->chromSize;
        while (i < n) {
            if (vals->valBuf[i] == 0.0) { ++i; continue; }
            long j = i + 1;
            while (j < n && vals->valBuf[j] == vals->valBuf[i]) ++j;
            printf("RUN %s %ld %ld %.17g\n", chrom->name, i, j, vals->valBuf[i]);
            i = j;
        }
    }
    struct lm *lm = lmInit(0);
    int r;
    for (r = 0; r < nreg && nchrom > 0; ++r) {
        int pick = (int)(rng() % (unsigned)nchrom);
        for (chrom = chroms; pick > 0; --pick) chrom = chrom->next;
        unsigned size = chrom->size ? chrom->size : 1;
        unsigned start = rng() % size, len = 1 + rng() % (r % 4 == 0 ? size : 64);
        unsigned end = start + len > size ? size : start + len;
        if (end <= start) continue;
        struct bbiInterval *iv, *list = bigWigIntervalQuery(bbi, chrom->name, start, end, lm);
        printf("REG %s %u %u %d\n", chrom->name, start, end, slCount(list));
        for (iv = list; iv != NULL; iv = iv->next) printf("IV %u %u %.17g\n", iv->start, iv->end, iv->val);
    }
    return 0;
}
