// dense_chunks_test.cpp -- the chunk table of plastid_amd/csrc/dense_host.h (seg_out_lo, spans_of, cut_span,
// out_overlap, first_of_chunk, make_desc, span_reads, span_cell, span_rows, span_base, base_cell, same_word) on a
// machine without a GPU;
// tests/test_dense_chunks.py compiles it under the address and undefined-behaviour sanitizers and runs it.  The table is
// built in the steps of build_dense_chunks (plastid_counts.hip): sort by first output element, count, place, describe.
//   dense_chunks_test chunk          elements of a chunk
//   dense_chunks_test table FILE     FILE: "out_elems", then one segment per line (out_off step len clip_lo clip_hi start
//                                    known cell_base ext).  Prints "overlap" and nothing else for a plan whose output
//                                    ranges overlap, else per chunk "chunk C spans overflow-spans", per row of 128
//                                    elements "row C R spans-it-reads-through", and per element that reads a cell
//                                    "elem E cell" -- as a workgroup finds them: through the chunk's descriptor -- and per pair of
//                                    elements that both read "pair E one-load".
#include "dense_host.h"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace pcdense;

static int table(const char *path) {
    FILE *f = fopen(path, "r");
    if (!f) { perror(path); return 2; }
    int64_t out_elems = 0;
    if (fscanf(f, "%" SCNd64, &out_elems) != 1) return 2;
    std::vector<SegIn> segs;
    SegIn s;
    int known = 0;
    while (fscanf(f, "%" SCNd64 " %d %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %d %" SCNd64 " %" SCNd64, &s.out_off, &s.step, &s.len, &s.clip_lo, &s.clip_hi,
                  &s.start, &known, &s.cell_base, &s.ext) == 9) {
        s.known = known != 0;
        segs.push_back(s);
    }
    fclose(f);
    const size_t n = segs.size(), nchunks = (size_t)chunks_of(out_elems);
    // sorted by first output element, empty segments last
    std::vector<uint32_t> idx(n);
    for (size_t i = 0; i < n; ++i) idx[i] = (uint32_t)i;
    const auto key = [&](uint32_t i) { return segs[i].len > 0 ? (uint64_t)seg_out_lo(segs[i].out_off, segs[i].step, segs[i].len) : ~(uint64_t)0; };
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
    std::vector<uint32_t> at(n + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        const SegIn &g = segs[idx[i]];
        if (g.len <= 0) { at[i + 1] = at[i]; continue; }
        at[i + 1] = at[i] + (uint32_t)spans_of((int64_t)key(idx[i]), g.len);
        if (i > 0 && out_overlap((int64_t)key(idx[i - 1]), segs[idx[i - 1]].len, (int64_t)key(idx[i]))) { printf("overlap\n"); return 0; }
    }
    std::vector<Span> spans(at[n]);    // (exact sizes: the sanitizer sees every write)
    std::vector<uint32_t> first_of(nchunks, 0), n_of(nchunks, 0);
    for (size_t i = 0; i < n; ++i) {
        const SegIn &g = segs[idx[i]];
        if (g.len <= 0) continue;
        const int64_t lo = (int64_t)key(idx[i]), prev_end = i > 0 ? (int64_t)key(idx[i - 1]) + segs[idx[i - 1]].len : -1;
        for (uint32_t k = 0; k < at[i + 1] - at[i]; ++k) {
            const size_t c = (size_t)(lo / kChunk + k);
            spans.at(at[i] + k) = cut_span(g, (int64_t)k);
            n_of.at(c) += 1;
            if (first_of_chunk(lo, (int64_t)k, prev_end)) first_of.at(c) = at[i] + k;
        }
    }
    for (size_t c = 0; c < nchunks; ++c) {
        const ChunkDesc d = make_desc(spans.data(), n_of[c] ? first_of[c] : 0u, n_of[c]);
        printf("chunk %zu %u %u\n", c, d.n, d.n > (uint32_t)kInlineSpans ? d.n - kInlineSpans : 0u);
        const auto span = [&](uint32_t k) -> const Span & { return k < (uint32_t)kInlineSpans ? d.s[k] : spans.at(d.ovf + (k - kInlineSpans)); };
        const int64_t valid = out_elems - (int64_t)c * kChunk < kChunk ? out_elems - (int64_t)c * kChunk : kChunk;
        for (uint32_t k = 0; k < d.n; ++k) {   // in output order, inside the chunk
            const Span &sp = span(k);
            if (!(sp.a() < sp.b() && sp.b() <= valid && sp.a() <= sp.ra() && sp.ra() <= sp.rb() && sp.rb() <= sp.b() && (k == 0 || span(k - 1).b() <= sp.a()))) {
                fprintf(stderr, "chunk %zu span %u: [%u, %u) reads [%u, %u)\n", c, k, sp.a(), sp.b(), sp.ra(), sp.rb());
                return 1;
            }
        }
        // as the kernel goes: the rows that read (any) and that read through several spans (multi), each span's word
        uint32_t any = 0, multi = 0;
        for (uint32_t k = 0; k < d.n; ++k) { const uint32_t rows = span_rows(span(k)); multi |= any & rows; any |= rows; }
        for (uint32_t row = 0; row < (uint32_t)valid; row += kRow) {
            int hits = 0;
            for (uint32_t k = 0; k < d.n; ++k) hits += span_rows(span(k)) >> (row / kRow) & 1u;
            if ((hits > 0) != ((any >> (row / kRow) & 1u) != 0) || (hits > 1) != ((multi >> (row / kRow) & 1u) != 0)) {
                fprintf(stderr, "chunk %zu row %u: %d spans, any %x multi %x\n", c, row / kRow, hits, any, multi);
                return 1;
            }
            printf("row %zu %u %d\n", c, row / kRow, hits);
        }
        for (uint32_t e = 0; e < (uint32_t)valid; e += 2) {      // a pair, as a lane has it
            uint32_t x[2] = {0, 0};
            bool r[2] = {false, false};
            const uint32_t rowbit = 1u << (e / kRow);
            for (uint32_t k = 0; k < d.n; ++k) {
                const Span &sp = span(k);
                for (uint32_t h = 0; h < 2; ++h) {
                    if (!span_reads(sp, e + h)) continue;
                    if (r[h]) { fprintf(stderr, "chunk %zu element %u reads through two spans\n", c, e + h); return 1; }
                    r[h] = true;
                    // a row of one span takes the span's uniform base; a row of several each element's own span
                    x[h] = (multi & rowbit) ? span_cell(sp, e + h) : base_cell(span_base(sp), sp.dir > 0, e + h);
                    if (x[h] != span_cell(sp, e + h) || !(span_rows(sp) & rowbit)) { fprintf(stderr, "chunk %zu element %u: base form differs\n", c, e + h); return 1; }
                }
            }
            for (uint32_t h = 0; h < 2; ++h)
                if (r[h] && e + h < (uint32_t)valid) printf("elem %" PRId64 " %u\n", (int64_t)c * kChunk + e + h, x[h]);
            if (r[0] && r[1]) printf("pair %" PRId64 " %d\n", (int64_t)c * kChunk + e, same_word(x[0], x[1]) ? 1 : 0);
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !std::strcmp(argv[1], "table")) return table(argv[2]);
    if (argc == 2 && !std::strcmp(argv[1], "chunk")) { printf("%d\n", kChunk); return 0; }
    fprintf(stderr, "usage: dense_chunks_test chunk | table FILE\n");
    return 2;
}
