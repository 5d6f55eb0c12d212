/* hts_sam_golden.c -- this project's harness around the reference-held htslib: reads a BAM file with sam_read1 and
 * writes every record as SAM TEXT with htslib's own writer (sam_open "w", sam_hdr_write, sam_write1), so that the text the
 * SAM readers are pinned against is what htslib gives for the records of tests/golden/hts_fixture.npz.
 *
 *     hts_sam_golden in.bam out.sam
 *
 * Built by tests/golden/make_sam_golden.py against oracle/_ref/libhts_ref.a; never part of the product. */
#include <stdio.h>
#include <stdlib.h>

#include "htslib/sam.h"

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bam out.sam\n", argv[0]);
        return 2;
    }
    samFile *in = sam_open(argv[1], "rb");
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    bam_hdr_t *h = sam_hdr_read(in);
    if (!h) { fprintf(stderr, "no header in %s\n", argv[1]); return 1; }
    samFile *out = sam_open(argv[2], "w");
    if (!out) { fprintf(stderr, "cannot create %s\n", argv[2]); return 1; }
    if (sam_hdr_write(out, h) != 0) { fprintf(stderr, "sam_hdr_write failed\n"); return 1; }
    bam1_t *b = bam_init1();
    long n = 0;
    int r;
    while ((r = sam_read1(in, h, b)) >= 0) {
        if (sam_write1(out, h, b) < 0) { fprintf(stderr, "sam_write1 failed at record %ld\n", n); return 1; }
        ++n;
    }
    if (r < -1) { fprintf(stderr, "sam_read1 failed at record %ld\n", n); return 1; }
    bam_destroy1(b);
    bam_hdr_destroy(h);
    sam_close(out);
    sam_close(in);
    printf("%ld records\n", n);
    return 0;
}
