/*
 * hts_csi_golden.c -- fixture generator for the CSI index, run against the REFERENCE-HELD htslib (version 1.3) in the
 * build container, in the style of hts_golden.c.  Test infrastructure: tests/golden/make_csi_golden.py compiles it
 * against oracle/_ref/libhts_ref.a (made by oracle/build_ref.sh) into oracle/_ref/ (never committed) and turns its
 * output into the committed fixture tests/golden/csi_fixture.npz.
 *
 *   hts_csi_golden write-long out.bam [seed]     a BAM file (sam_write1) with references of 2^31 - 1, 700 000 000,
 *       2^30 (no records), 9 000 and 5 000 (placed-unmapped reads only): clusters of reads at 0, 2^29 +- 10, 2^30 +- 10,
 *       2 * 10^9 and at the end of the longest reference, pile-ups, a spliced read whose N run crosses 2^29,
 *       placed-unmapped and unplaced reads
 *   hts_csi_golden write-flat out.bam [seed]     references of at most 16 000: a CSI of depth 0
 *   hts_csi_golden query in.bam min_shift nregions [seed]
 *       sam_index_build(in.bam, min_shift) -> in.bam.csi; every record as htslib reads it back; the result sets of
 *       sam_itr_queryi for seeded regions of the five kinds of hts_golden.c, read through that CSI; the index's counts
 *
 * Output of `query` (stdout), one line per item:
 *   REF name length
 *   REC index tid pos endpos flag mapq l_qseq
 *   REG tid beg end n i0 i1 ...                 (i: the record's index, from its name "r<index>")
 *   STAT tid mapped unmapped
 *   NOCOOR n
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "htslib/hts.h"
#include "htslib/sam.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(void) { /* xorshift64* */
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static int64_t rint_(int64_t lo, int64_t hi) { return lo + (int64_t)(((uint64_t)rnd() << 16 ^ rnd()) % (uint64_t)(hi - lo + 1)); }

#define MAXOPS 8
typedef struct { int tid; int64_t pos; int flag, ncig; uint32_t cig[MAXOPS]; } rec_t;

static rec_t *recs;
static int nrecs, caprecs;

static rec_t *push(int tid, int64_t pos, int flag) {
    if (nrecs == caprecs) { caprecs = caprecs ? 2 * caprecs : 1024; recs = (rec_t *)realloc(recs, sizeof(rec_t) * (size_t)caprecs); }
    rec_t *r = &recs[nrecs++];
    memset(r, 0, sizeof(*r));
    r->tid = tid; r->pos = pos; r->flag = flag;
    return r;
}
static void plain(int tid, int64_t pos, int len, int flag) {
    rec_t *r = push(tid, pos, flag);
    r->ncig = 1; r->cig[0] = bam_cigar_gen(len, BAM_CMATCH);
}
static void spliced(int tid, int64_t pos, int a, int n, int b, int flag) {
    rec_t *r = push(tid, pos, flag);
    r->ncig = 3; r->cig[0] = bam_cigar_gen(a, BAM_CMATCH); r->cig[1] = bam_cigar_gen(n, BAM_CREF_SKIP); r->cig[2] = bam_cigar_gen(b, BAM_CMATCH);
}
static void unmapped(int tid, int64_t pos) { push(tid, pos, BAM_FUNMAP); }

static int by_place(const void *a_, const void *b_) {   /* (tid, pos), ties in the order made */
    const rec_t *a = (const rec_t *)a_, *b = (const rec_t *)b_;
    if (a->tid != b->tid) return a->tid < b->tid ? -1 : 1;
    if (a->pos != b->pos) return a->pos < b->pos ? -1 : 1;
    return a < b ? -1 : a > b;
}

/* a cluster of n reads from `at` on: steps of 0 (pile-ups), a few bases, now and then a few hundred */
static void cluster(int tid, int64_t at, int n, int64_t limit) {
    int64_t pos = at;
    for (int k = 0; k < n; ++k) {
        const uint32_t c = rnd() % 10;
        pos += c < 4 ? 0 : c < 9 ? rint_(1, 6) : rint_(100, 700);
        const int len = (int)rint_(20, 40);
        if (pos + len > limit) pos = limit - len;
        const uint32_t f = rnd() % 30;
        if (f == 0) unmapped(tid, pos);
        else if (f == 1 && pos + 40020 <= limit) spliced(tid, pos, 10, (int)rint_(50, 40000), 10, BAM_FREVERSE);
        else plain(tid, pos, len, (rnd() & 1) ? BAM_FREVERSE : 0);
    }
}

static void fill(bam1_t *b, int idx, const rec_t *r) {
    char name[32];
    snprintf(name, sizeof(name), "r%d", idx);
    int lq = 0;
    for (int k = 0; k < r->ncig; ++k)
        if (bam_cigar_type(bam_cigar_op(r->cig[k])) & 1) lq += bam_cigar_oplen(r->cig[k]);
    if (r->ncig == 0) lq = 12;
    const int l_qname = (int)strlen(name) + 1;
    const int need = l_qname + 4 * r->ncig + (lq + 1) / 2 + lq;
    if ((int)b->m_data < need) { b->m_data = need; b->data = (uint8_t *)realloc(b->data, (size_t)need); }
    b->l_data = need;
    memset(b->data, 0, (size_t)need);
    memcpy(b->data, name, (size_t)l_qname);
    memcpy(b->data + l_qname, r->cig, 4u * (size_t)r->ncig);
    memset(b->data + l_qname + 4 * r->ncig, 0x22, (size_t)((lq + 1) / 2));
    memset(b->data + l_qname + 4 * r->ncig + (lq + 1) / 2, 30, (size_t)lq);
    b->core.tid = r->tid; b->core.pos = (int32_t)r->pos; b->core.qual = (uint8_t)((idx * 29 + 7) % 61); b->core.l_qname = (uint8_t)l_qname;
    b->core.flag = (uint16_t)r->flag; b->core.n_cigar = (uint16_t)r->ncig; b->core.l_qseq = lq;
    b->core.mtid = -1; b->core.mpos = -1; b->core.isize = 0;
    b->core.bin = r->tid < 0 ? hts_reg2bin(-1, 0, 14, 5) : hts_reg2bin(r->pos, bam_endpos(b), 14, 5);   /* (16 bits of it are kept) */
}

static int write_bam(const char *fn, int nref, const char **names, const int64_t *lens) {
    bam_hdr_t *h = bam_hdr_init();
    h->n_targets = nref;
    h->target_len = (uint32_t *)malloc((size_t)nref * sizeof(uint32_t));
    h->target_name = (char **)malloc((size_t)nref * sizeof(char *));
    char text[1024] = "@HD\tVN:1.5\tSO:coordinate\n";
    for (int t = 0; t < nref; ++t) {
        h->target_len[t] = (uint32_t)lens[t];
        h->target_name[t] = strdup(names[t]);
        char line[96];
        snprintf(line, sizeof(line), "@SQ\tSN:%s\tLN:%lld\n", names[t], (long long)lens[t]);
        strcat(text, line);
    }
    h->text = strdup(text);
    h->l_text = (uint32_t)strlen(text);
    qsort(recs, (size_t)nrecs, sizeof(rec_t), by_place);
    samFile *out = sam_open(fn, "wb");
    if (!out || sam_hdr_write(out, h) < 0) { fprintf(stderr, "cannot write %s\n", fn); return 1; }
    bam1_t *b = bam_init1();
    int idx = 0, first_unplaced = 0;
    while (first_unplaced < nrecs && recs[first_unplaced].tid < 0) ++first_unplaced;   /* tid -1 sorts first: written last */
    for (int k = first_unplaced; k < nrecs; ++k, ++idx) { fill(b, idx, &recs[k]); if (sam_write1(out, h, b) < 0) return 1; }
    for (int k = 0; k < first_unplaced; ++k, ++idx) { fill(b, idx, &recs[k]); if (sam_write1(out, h, b) < 0) return 1; }
    bam_destroy1(b);
    sam_close(out);
    bam_hdr_destroy(h);
    return 0;
}

static int write_long(const char *fn) {
    const char *names[5] = {"big", "mid", "empty", "small", "unm"};
    const int64_t lens[5] = {2147483647ll, 700000000ll, 1ll << 30, 9000, 5000};
    const int64_t p29 = 1ll << 29, p30 = 1ll << 30;
    cluster(0, 0, 220, lens[0]);
    cluster(0, p29 - 10, 200, lens[0]);
    cluster(0, p29 + 10, 120, lens[0]);
    cluster(0, p30 - 10, 200, lens[0]);
    cluster(0, p30 + 10, 120, lens[0]);
    cluster(0, 2000000000ll, 250, lens[0]);
    cluster(0, lens[0] - 3000, 200, lens[0]);
    for (int k = 0; k < 40; ++k) plain(0, lens[0] - 30, 30, k & 1 ? BAM_FREVERSE : 0);     /* a pile that ends at the last base */
    spliced(0, p29 - 5000, 20, 10000, 20, 0);                                              /* its N run crosses 2^29 */
    spliced(0, p30 - 70000, 15, 140000, 15, BAM_FREVERSE);                                 /* ... and one across 2^30 */
    for (int k = 0; k < 60; ++k) plain(0, rint_(0, lens[0] - 50), 30, 0);                  /* sparse reads anywhere */
    cluster(1, 100, 120, lens[1]);
    cluster(1, p29 - 10, 150, lens[1]);
    cluster(1, lens[1] - 2000, 60, lens[1]);
    for (int k = 0; k < 120; ++k) plain(1, rint_(0, lens[1] - 50), 25, BAM_FREVERSE);
    cluster(3, 10, 40, lens[3]);
    cluster(3, 8000, 30, lens[3]);
    for (int k = 0; k < 5; ++k) unmapped(4, 100 + 900 * k);
    for (int k = 0; k < 4; ++k) push(-1, -1, BAM_FUNMAP);
    return write_bam(fn, 5, names, lens);
}

static int write_flat(const char *fn) {
    const char *names[2] = {"f1", "f2"};
    const int64_t lens[2] = {16000, 12000};
    cluster(0, 5, 150, lens[0]);
    cluster(0, 9000, 80, lens[0]);
    unmapped(1, 3);
    cluster(1, 2000, 70, lens[1]);
    spliced(1, 100, 10, 11000, 10, 0);
    for (int k = 0; k < 2; ++k) push(-1, -1, BAM_FUNMAP);
    return write_bam(fn, 2, names, lens);
}

static int query(const char *fn, int min_shift, int nreg) {
    if (sam_index_build(fn, min_shift) < 0) { fprintf(stderr, "index build failed\n"); return 1; }
    samFile *in = sam_open(fn, "rb");
    bam_hdr_t *h = sam_hdr_read(in);
    const int nref = h->n_targets;
    for (int t = 0; t < nref; ++t) printf("REF %s %u\n", h->target_name[t], h->target_len[t]);
    bam1_t *b = bam_init1();
    int i = 0;
    while (sam_read1(in, h, b) >= 0) {
        printf("REC %d %d %d %d %d %d %d\n", i, b->core.tid, b->core.pos, (int)bam_endpos(b), b->core.flag, (int)b->core.qual, (int)b->core.l_qseq);
        ++i;
    }
    sam_close(in);

    in = sam_open(fn, "rb");
    bam_hdr_destroy(sam_hdr_read(in));
    char fnidx[4096];
    snprintf(fnidx, sizeof(fnidx), "%s.csi", fn);
    hts_idx_t *ix = hts_idx_load2(fn, fnidx);
    if (!ix) { fprintf(stderr, "cannot load %s\n", fnidx); return 1; }
    /* where reads cluster in a long reference: every second region on such a reference starts near one of them */
    const int64_t marks[7] = {0, 1ll << 29, 1ll << 30, 2000000000ll, 2147483647ll - 1500, (1ll << 29) - 5000, (1ll << 30) - 70000};
    for (int q = 0; q < nreg; ++q) {
        int t = (int)(rnd() % (uint32_t)nref);
        if (rnd() & 1) t = 0;
        const int64_t len = h->target_len[t];
        int64_t beg = rint_(0, len - 1), end;
        if (len > (1ll << 29) && (rnd() & 1)) {
            beg = marks[rnd() % 7] + rint_(-3000, 3000);
            if (beg < 0) beg = 0;
            if (beg > len - 1) beg = len - 1;
        }
        switch (q % 5) {
        case 0: end = beg + rint_(1, 50); break;                                             /* short */
        case 1: end = beg + rint_(100, 20000); break;                                        /* long */
        case 2: beg = (beg >> min_shift) << min_shift; end = beg + (1ll << min_shift); break;   /* one leaf exactly */
        case 3: beg = 0; end = len; break;                                                   /* whole reference */
        default: end = beg + 1; break;                                                       /* one position */
        }
        if (end > len + 100) end = len + 100;
        if (end > 2147483647ll) end = 2147483647ll;
        hts_itr_t *it = sam_itr_queryi(ix, t, (int)beg, (int)end);
        int n = 0, cap = 1024, *got = (int *)malloc(sizeof(int) * (size_t)cap);
        while (it && sam_itr_next(in, it, b) >= 0) {
            if (n == cap) { cap *= 2; got = (int *)realloc(got, sizeof(int) * (size_t)cap); }
            got[n++] = atoi(bam_get_qname(b) + 1);
        }
        printf("REG %d %lld %lld %d", t, (long long)beg, (long long)end, n);
        for (int k = 0; k < n; ++k) printf(" %d", got[k]);
        printf("\n");
        free(got);
        hts_itr_destroy(it);
    }
    for (int t = 0; t < nref; ++t) {
        uint64_t m = 0, u = 0;
        hts_idx_get_stat(ix, t, &m, &u);
        printf("STAT %d %llu %llu\n", t, (unsigned long long)m, (unsigned long long)u);
    }
    printf("NOCOOR %llu\n", (unsigned long long)hts_idx_get_n_no_coor(ix));
    hts_idx_destroy(ix);
    sam_close(in);
    bam_destroy1(b);
    bam_hdr_destroy(h);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: hts_csi_golden write-long|write-flat out.bam [seed] | query in.bam min_shift nregions [seed]\n"); return 2; }
    const int is_query = strcmp(argv[1], "query") == 0;
    const int seed_at = is_query ? 5 : 3;
    if (argc > seed_at) rng_state ^= (uint64_t)atoll(argv[seed_at]) * 0x9E3779B97F4A7C15ull;
    if (strcmp(argv[1], "write-long") == 0) return write_long(argv[2]);
    if (strcmp(argv[1], "write-flat") == 0) return write_flat(argv[2]);
    if (is_query && argc >= 5) return query(argv[2], atoi(argv[3]), atoi(argv[4]));
    return 2;
}
