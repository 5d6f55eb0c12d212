// host_shims.h -- the C ABI of the host models (ctypes: plastid_amd/_hostlib.py): thin pb_* shims over track_host.h,
// bigwig_host.h, deflate_host.h, bigwig_write_host.h and bigwig_summary_host.h.  Not a header of its own: the last part of
// bam_stager.cpp, which includes it at its end (one translation unit, one library) and whose fail() / pb_last_error it uses.
#include "bigwig_host.h"
#include "bigwig_write_host.h"
#include "bigwig_summary_host.h"
#include "deflate_host.h"
#include "track_host.h"

extern "C" {
// ---------------------------------------------------------------- count tracks as text (track_host.h)
// A bedGraph / wiggle text read on the host by the parser the device import runs: the reference's WiggleReader
// (plastid/readers/wiggle.py:43-174) as columns.  NULL (pb_last_error): a malformed line, "<name>: track line <n>: <what>".
void *pb_track_read(const void *image, int64_t size, const char *name) {
    if (size < 0 || (size > 0 && !image)) { fail("pb_track_read: bad arguments"); return nullptr; }
    pctrack::TrackTable *t = new pctrack::TrackTable();
    pctrack::read_track((const uint8_t *)image, (size_t)size, *t);
    if (t->defect != pctrack::kTrkOk) {
        fail(pctrack::track_defect_message(name, t->defect_line, t->defect));
        delete t;
        return nullptr;
    }
    return t;
}
void pb_track_close(void *h) { delete static_cast<pctrack::TrackTable *>(h); }
int64_t pb_track_rows(void *h) { return h ? (int64_t)static_cast<pctrack::TrackTable *>(h)->contig.size() : -1; }
int pb_track_nchrom(void *h) { return h ? (int)static_cast<pctrack::TrackTable *>(h)->names.size() : -1; }
const char *pb_track_chrom(void *h, int i) { return static_cast<pctrack::TrackTable *>(h)->names[(size_t)i].c_str(); }
// the columns, and per row its 0-based line and whether a token of it was not plain
int pb_track_fill(void *h, int32_t *chrom, int64_t *start, int64_t *stop, double *value, int64_t *line, uint8_t *escaped) {
    pctrack::TrackTable *t = static_cast<pctrack::TrackTable *>(h);
    if (!t) return fail("pb_track_fill: NULL handle");
    const size_t n = t->contig.size();
    if (n) {
        std::memcpy(chrom, t->contig.data(), n * 4); std::memcpy(start, t->start.data(), n * 8); std::memcpy(stop, t->stop.data(), n * 8);
        std::memcpy(value, t->value.data(), n * 8); std::memcpy(line, t->line.data(), n * 8); std::memcpy(escaped, t->escaped.data(), n);
    }
    return 0;
}
// [0] lines, [1] yielded lines, [2] escaped lines, [3] state records
int pb_track_stats(void *h, int64_t *out4) {
    pctrack::TrackTable *t = static_cast<pctrack::TrackTable *>(h);
    if (!t || !out4) return fail("pb_track_stats: bad arguments");
    out4[0] = t->lines; out4[1] = (int64_t)t->contig.size(); out4[2] = t->n_escaped; out4[3] = t->states;
    return 0;
}

// A track written on the host by the serial writers of track_host.h (the model of the device export).  A writer is a
// text that grows contig by contig: kind 0 bedGraph, 1 variableStep; the caller passes the contigs in the order of the file.
struct TrackWriter { std::string text; pctrack::ExportStats stats; };
void *pb_track_writer_open(void) { return new TrackWriter(); }
void pb_track_writer_close(void *h) { delete static_cast<TrackWriter *>(h); }
int pb_track_writer_add(void *h, int kind, const char *name, const double *cells, int64_t n) {
    TrackWriter *w = static_cast<TrackWriter *>(h);
    if (!w || !name || n < 0 || (n > 0 && !cells) || (kind != 0 && kind != 1)) return fail("pb_track_writer_add: bad arguments");
    if (kind == 0) pctrack::write_bedgraph_contig(w->text, name, cells, n, w->stats);
    else pctrack::write_variable_step_contig(w->text, name, cells, n, w->stats);
    return 0;
}
// The text BAMGenomeArray writes of one contig's count vector (genome_array.py:990-1111): `cells` are n int64 counts
// (is_float 0) or float64 values (1); bedGraph runs are cut at every multiple of `window`.
int pb_track_writer_add_counts(void *h, int kind, int is_float, const char *name, const void *cells, int64_t n, int64_t window) {
    TrackWriter *w = static_cast<TrackWriter *>(h);
    if (!w || !name || n < 0 || (n > 0 && !cells) || (kind != 0 && kind != 1) || (kind == 0 && window < 1)) return fail("pb_track_writer_add_counts: bad arguments");
    if (kind == 0 && is_float) pctrack::write_count_bedgraph_contig(w->text, name, static_cast<const double *>(cells), n, window, w->stats);
    else if (kind == 0) pctrack::write_count_bedgraph_contig(w->text, name, static_cast<const int64_t *>(cells), n, window, w->stats);
    else if (is_float) pctrack::write_count_variable_step_contig(w->text, name, static_cast<const double *>(cells), n, w->stats);
    else pctrack::write_count_variable_step_contig(w->text, name, static_cast<const int64_t *>(cells), n, w->stats);
    return 0;
}
int64_t pb_track_writer_size(void *h) { return h ? (int64_t)static_cast<TrackWriter *>(h)->text.size() : -1; }
const char *pb_track_writer_text(void *h) { return static_cast<TrackWriter *>(h)->text.data(); }
// [0] lines, [1] runs / non-zero cells, [2] values that are not plain, [3] bytes
int pb_track_writer_stats(void *h, int64_t *out4) {
    TrackWriter *w = static_cast<TrackWriter *>(h);
    if (!w || !out4) return fail("pb_track_writer_stats: bad arguments");
    out4[0] = w->stats.lines; out4[1] = w->stats.runs; out4[2] = w->stats.listed; out4[3] = w->stats.bytes;
    return 0;
}
// repr(float(v[k])) of n values: text k at out + 24 * k, its length in len[k]
int pb_float_repr(const double *v, int64_t n, char *out, uint8_t *len) {
    if (n < 0 || (n > 0 && (!v || !out || !len))) return fail("pb_float_repr: bad arguments");
    for (int64_t k = 0; k < n; ++k) len[k] = (uint8_t)pctrack::float_repr(v[k], out + pctrack::kReprMax * k);
    return 0;
}

// ---------------------------------------------------------------- bigWig (bigwig_host.h)
// A bigWig file read on the host, block by block with zlib: the items Kent's readers apply (bwgQuery.c:155-285), in file
// order, as columns.  The model of the device import.  NULL (pb_last_error): "<name>: bigWig: <what>".
static int zlib_raw_inflate(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t &produced) {
    z_stream zs;
    std::memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) return 1;
    zs.next_in = const_cast<Bytef *>(src); zs.avail_in = (uInt)n;
    zs.next_out = dst; zs.avail_out = (uInt)cap;
    const int rc = inflate(&zs, Z_FINISH);
    produced = (size_t)zs.total_out;
    const bool whole = rc == Z_STREAM_END && zs.avail_in == 0;   // (the stream ends with its last byte: the trailer follows)
    inflateEnd(&zs);
    return whole ? 0 : 1;
}
void *pb_bigwig_read(const void *image, int64_t size, const char *name) {
    if (size < 0 || (size > 0 && !image)) { fail("pb_bigwig_read: bad arguments"); return nullptr; }
    pcbw::ItemTable *t = new pcbw::ItemTable();
    pcbw::read_items((const uint8_t *)image, (uint64_t)size, zlib_raw_inflate, *t);
    if (t->defect != pcbw::kNoDefect) {
        fail(pcbw::defect_message(name, t->defect));
        delete t;
        return nullptr;
    }
    return t;
}
void pb_bigwig_close(void *h) { delete static_cast<pcbw::ItemTable *>(h); }
int64_t pb_bigwig_rows(void *h) { return h ? (int64_t)static_cast<pcbw::ItemTable *>(h)->chrom.size() : -1; }
int pb_bigwig_nchrom(void *h) { return h ? (int)static_cast<pcbw::ItemTable *>(h)->file.chroms.size() : -1; }
const char *pb_bigwig_chrom(void *h, int i) { return static_cast<pcbw::ItemTable *>(h)->file.chroms[(size_t)i].name.c_str(); }
int64_t pb_bigwig_chrom_size(void *h, int i) { return (int64_t)static_cast<pcbw::ItemTable *>(h)->file.chroms[(size_t)i].size; }
int64_t pb_bigwig_nblocks(void *h) { return h ? (int64_t)static_cast<pcbw::ItemTable *>(h)->file.blocks.size() : -1; }
int pb_bigwig_fill(void *h, int32_t *chrom, int64_t *start, int64_t *stop, double *value, int32_t *block, int64_t *block_off, int64_t *block_size) {
    pcbw::ItemTable *t = static_cast<pcbw::ItemTable *>(h);
    if (!t) return fail("pb_bigwig_fill: NULL handle");
    const size_t n = t->chrom.size();
    if (n) {
        std::memcpy(chrom, t->chrom.data(), n * 4); std::memcpy(start, t->start.data(), n * 8); std::memcpy(stop, t->stop.data(), n * 8);
        std::memcpy(value, t->value.data(), n * 8); std::memcpy(block, t->block.data(), n * 4);
    }
    for (size_t b = 0; b < t->file.blocks.size(); ++b) { block_off[b] = (int64_t)t->file.blocks[b].off; block_size[b] = (int64_t)t->file.blocks[b].size; }
    return 0;
}
// [0] blocks, [1] compressed blocks, [2-4] items of bedGraph / variableStep / fixedStep sections, [5] bytes inflated,
// [6] uncompressBufSize, [7] version
int pb_bigwig_stats(void *h, int64_t *out8) {
    pcbw::ItemTable *t = static_cast<pcbw::ItemTable *>(h);
    if (!t || !out8) return fail("pb_bigwig_stats: bad arguments");
    out8[0] = (int64_t)t->file.blocks.size(); out8[1] = t->file.compressed() ? out8[0] : 0;
    out8[2] = t->by_type[0]; out8[3] = t->by_type[1]; out8[4] = t->by_type[2]; out8[5] = t->bytes_inflated;
    out8[6] = t->file.uncompress_buf; out8[7] = t->file.version;
    return 0;
}

// ---------------------------------------------------------------- zlib encoder and bigWig writer (deflate_host.h, bigwig_write_host.h)
// pb_deflate_zlib_mode: pc_deflate_zlib_mode without the engine -- the model encoder over n inputs, the streams back to back.
int pb_deflate_zlib_mode(const void *image, int64_t n, const int64_t *off, const int64_t *len, void *out, int64_t out_capacity, int64_t *out_off, int64_t *out_len,
                         int mode) {
    if (mode != (int)pcdeflate::kFixed && mode != (int)pcdeflate::kDynamic) return fail("pb_deflate_zlib: mode " + std::to_string(mode) + " is neither 1 (fixed) nor 2 (dynamic)");
    if (n < 0 || out_capacity < 0 || (n > 0 && (!off || !len || !out || !out_off || !out_len))) return fail("pb_deflate_zlib: bad arguments");
    int64_t need = 0;
    for (int64_t k = 0; k < n; ++k) {
        if (off[k] < 0 || len[k] < 0 || len[k] > (int64_t)pcdeflate::kMaxInput) return fail("pb_deflate_zlib: input " + std::to_string(k) + " lies below 0 or holds more than 24600 bytes");
        if (len[k] > 0 && !image) return fail("pb_deflate_zlib: bad arguments");
        need += len[k] + (int64_t)pcdeflate::kStreamOverhead;
    }
    if (out_capacity < need) return fail("pb_deflate_zlib: out_capacity below the " + std::to_string(need) + " bytes the streams may take");
    std::vector<uint8_t> stream;
    int64_t at = 0;
    for (int64_t k = 0; k < n; ++k) {
        stream.clear();
        pcdeflate::encode((const uint8_t *)image + off[k], (uint32_t)len[k], stream, (uint32_t)mode);
        std::memcpy((uint8_t *)out + at, stream.data(), stream.size());
        out_off[k] = at; out_len[k] = (int64_t)stream.size();
        at += (int64_t)stream.size();
    }
    return 0;
}

int pb_deflate_zlib(const void *image, int64_t n, const int64_t *off, const int64_t *len, void *out, int64_t out_capacity, int64_t *out_off, int64_t *out_len) {
    return pb_deflate_zlib_mode(image, n, off, len, out, out_capacity, out_off, out_len, (int)pcdeflate::kFixed);
}

// pb_huffman_lengths: pc_huffman_lengths without the engine -- pcdeflate::build_code's lengths of n counts under `limit`.
int pb_huffman_lengths(const uint32_t *counts, int64_t n, int limit, uint8_t *lengths_out) {
    if (!counts || !lengths_out) return fail("pb_huffman_lengths: bad arguments");
    if (n < 2 || n > (int64_t)pcdeflate::kLitSyms || limit < 1 || limit > 15 || ((int64_t)1 << limit) < n)
        return fail("pb_huffman_lengths: " + std::to_string(n) + " symbols under limit " + std::to_string(limit) + " (2 .. 286 symbols, limit 1 .. 15, 2^limit >= symbols)");
    uint64_t sum = 0;
    for (int64_t s = 0; s < n; ++s) sum += counts[s];
    if (sum >= ((uint64_t)1 << 32)) return fail("pb_huffman_lengths: the counts add up to 2^32 or more");
    std::vector<uint32_t> c(counts, counts + n), weight((size_t)n);
    std::vector<uint16_t> order((size_t)n), parent(2 * (size_t)n), depth((size_t)n);
    uint32_t bl_count[16], next_code[16];
    pcdeflate::build_code(c.data(), (uint32_t)n, (uint32_t)limit, order.data(), weight.data(), parent.data(), depth.data(), bl_count, next_code, lengths_out, nullptr);
    return 0;
}

// The serial bigWig writer: open, one add per contig (any order), finish, then the image and the statistics.
// zoom: 0 no zoom levels, -1 the automatic first reduction, 8 .. 2^24 the first reduction (bigwig_write_host.h: "zoom levels")
void *pb_bigwig_write_open_zoom(int64_t items_per_slot, int64_t block_size, int compress, int64_t zoom) {
    const std::string bad = pcbww::check_params(items_per_slot, block_size);
    if (!bad.empty()) { fail("pb_bigwig_write: " + bad); return nullptr; }
    if (compress < 0 || compress > 2) { fail("pb_bigwig_write: compress " + std::to_string(compress) + " is none of 0 (stored sections), 1 (fixed codes), 2 (dynamic codes)"); return nullptr; }
    const std::string bad_zoom = pcbww::check_zoom(zoom);
    if (!bad_zoom.empty()) { fail("pb_bigwig_write: " + bad_zoom); return nullptr; }
    pcbww::HostWriter *w = new pcbww::HostWriter();
    w->items_per_slot = (uint32_t)items_per_slot; w->block_size = (uint32_t)block_size; w->compress = compress; w->zoom = zoom;
    return w;
}
void *pb_bigwig_write_open(int64_t items_per_slot, int64_t block_size, int compress) { return pb_bigwig_write_open_zoom(items_per_slot, block_size, compress, 0); }
void pb_bigwig_write_close(void *h) { delete static_cast<pcbww::HostWriter *>(h); }
int pb_bigwig_write_add(void *h, const char *name, int64_t length, const double *cells, int64_t n) {
    pcbww::HostWriter *w = static_cast<pcbww::HostWriter *>(h);
    if (!w || !name || length < 0 || n < 0 || (n > 0 && !cells)) return fail("pb_bigwig_write_add: bad arguments");
    w->in.push_back({name, length, std::vector<double>(cells, cells + n)});
    return 0;
}
int pb_bigwig_write_finish(void *h) {
    pcbww::HostWriter *w = static_cast<pcbww::HostWriter *>(h);
    if (!w) return fail("pb_bigwig_write_finish: NULL handle");
    return w->finish() ? 0 : fail("pb_bigwig_write: " + w->error);
}
int64_t pb_bigwig_write_size(void *h) { return h ? (int64_t)static_cast<pcbww::HostWriter *>(h)->image.size() : -1; }
const void *pb_bigwig_write_image(void *h) { return static_cast<pcbww::HostWriter *>(h)->image.data(); }
// [0] contigs, [1] items, [2] sections, [3] raw bytes, [4] block bytes, [5] sections that fell back to stored
int pb_bigwig_write_stats(void *h, int64_t *out6) {
    pcbww::HostWriter *w = static_cast<pcbww::HostWriter *>(h);
    if (!w || !out6) return fail("pb_bigwig_write_stats: bad arguments");
    for (int k = 0; k < 6; ++k) out6[k] = w->stats[k];
    return 0;
}
// the sections that went out as [0] stored, [1] fixed, [2] dynamic blocks (all 0 for a file of stored sections)
int pb_bigwig_write_block_types(void *h, int64_t *out3) {
    pcbww::HostWriter *w = static_cast<pcbww::HostWriter *>(h);
    if (!w || !out3) return fail("pb_bigwig_write_block_types: bad arguments");
    for (int k = 0; k < 3; ++k) out3[k] = w->stats[5 + k];
    return 0;
}
// the zoom levels of the file: *levels, and per level (at most max_levels of them) [0] the reduction, [1] records, [2] blocks,
// [3] raw bytes of the blocks, [4] their bytes in the file
int pb_bigwig_write_zoom_stats(void *h, int64_t *levels, int max_levels, int64_t *out5) {
    pcbww::HostWriter *w = static_cast<pcbww::HostWriter *>(h);
    if (!w || !levels || max_levels < 0 || (max_levels > 0 && !out5)) return fail("pb_bigwig_write_zoom_stats: bad arguments");
    *levels = (int64_t)w->zoom_stats.size();
    for (size_t k = 0; k < w->zoom_stats.size() && k < (size_t)max_levels; ++k) {
        const pcbww::HostWriter::LevelStats &s = w->zoom_stats[k];
        out5[5 * k] = s.reduction; out5[5 * k + 1] = s.records; out5[5 * k + 2] = s.blocks; out5[5 * k + 3] = s.raw_bytes; out5[5 * k + 4] = s.file_bytes;
    }
    return 0;
}

// The zoom levels of a bigWig file, read on the host (bigwig_write_host.h: zoom_headers, read_zoom_level).  A file that
// is refused: "<name>: bigWig: <what>" (pb_last_error).
namespace {
struct ZoomRead { std::vector<pcbww::ZoomHeader> levels; pcbww::ZoomTable table; uint32_t uncompress_buf = 0; };
// the file's structure and its zoom headers; false: refused
bool zoom_open(const void *image, int64_t size, const char *name, const char *who, ZoomRead &z) {
    if (size < 0 || (size > 0 && !image)) { fail(std::string(who) + ": bad arguments"); return false; }
    pcbw::BigWig f;
    const unsigned long long d = pcbw::parse((const uint8_t *)image, (uint64_t)size, f);
    if (d != pcbw::kNoDefect) { fail(pcbw::defect_message(name, d)); return false; }
    const std::string bad = pcbww::zoom_headers((const uint8_t *)image, (uint64_t)size, z.levels);
    if (!bad.empty()) { fail(std::string(name ? name : "<memory>") + ": bigWig: " + bad); return false; }
    z.uncompress_buf = f.uncompress_buf;
    return true;
}
}   // namespace
// *levels, and per level (at most max_levels of them) [0] the reduction, [1] dataOffset, [2] indexOffset, [3] records
int pb_bigwig_zoom_info(const void *image, int64_t size, const char *name, int64_t *levels, int max_levels, int64_t *out4) {
    if (!levels || max_levels < 0 || (max_levels > 0 && !out4)) return fail("pb_bigwig_zoom_info: bad arguments");
    ZoomRead z;
    if (!zoom_open(image, size, name, "pb_bigwig_zoom_info", z)) return -1;
    *levels = (int64_t)z.levels.size();
    for (size_t k = 0; k < z.levels.size() && k < (size_t)max_levels; ++k) {
        out4[4 * k] = z.levels[k].reduction; out4[4 * k + 1] = (int64_t)z.levels[k].data; out4[4 * k + 2] = (int64_t)z.levels[k].index; out4[4 * k + 3] = z.levels[k].records;
    }
    return 0;
}
// the records of one level in file order, walked through the level's R-tree; NULL: refused
void *pb_bigwig_zoom_read(const void *image, int64_t size, const char *name, int64_t level) {
    ZoomRead *z = new ZoomRead();
    if (!zoom_open(image, size, name, "pb_bigwig_zoom_read", *z)) { delete z; return nullptr; }
    const std::string bad = pcbww::read_zoom_level((const uint8_t *)image, (uint64_t)size, z->uncompress_buf, z->levels, level, zlib_raw_inflate, z->table);
    if (!bad.empty()) { fail(std::string(name ? name : "<memory>") + ": bigWig: " + bad); delete z; return nullptr; }
    return z;
}
void pb_bigwig_zoom_close(void *h) { delete static_cast<ZoomRead *>(h); }
int64_t pb_bigwig_zoom_rows(void *h) { return h ? (int64_t)static_cast<ZoomRead *>(h)->table.chrom.size() : -1; }
int pb_bigwig_zoom_fill(void *h, uint32_t *chrom, uint32_t *start, uint32_t *end, uint32_t *valid, float *mn, float *mx, float *sum, float *sumsq) {
    ZoomRead *z = static_cast<ZoomRead *>(h);
    if (!z) return fail("pb_bigwig_zoom_fill: NULL handle");
    const pcbww::ZoomTable &t = z->table;
    const size_t n = t.chrom.size() * 4;
    if (n) {
        std::memcpy(chrom, t.chrom.data(), n); std::memcpy(start, t.start.data(), n); std::memcpy(end, t.end.data(), n); std::memcpy(valid, t.valid.data(), n);
        std::memcpy(mn, t.mn.data(), n); std::memcpy(mx, t.mx.data(), n); std::memcpy(sum, t.sum.data(), n); std::memcpy(sumsq, t.sumsq.data(), n);
    }
    return 0;
}

// Binned summaries of a bigWig file on the host (bigwig_summary_host.h): the model of pc_bigwig_summary_query, one thread.
// The handle keeps the image's pointer: the caller keeps the image alive.  NULL / -1 (pb_last_error): "<name>: bigWig: <what>".
namespace {
struct SummaryRead { pcbws::HostSummary s; std::string name; };
}   // namespace
void *pb_bigwig_summary_open(const void *image, int64_t size, const char *name) {
    if (size < 0 || (size > 0 && !image)) { fail("pb_bigwig_summary_open: bad arguments"); return nullptr; }
    SummaryRead *h = new SummaryRead();
    h->name = name ? name : "<memory>";
    const std::string bad = h->s.open((const uint8_t *)image, (uint64_t)size);
    if (!bad.empty()) { fail(h->name + ": bigWig: " + bad); delete h; return nullptr; }
    return h;
}
void pb_bigwig_summary_close(void *h) { delete static_cast<SummaryRead *>(h); }
int pb_bigwig_summary_nchrom(void *h) { return h ? (int)static_cast<SummaryRead *>(h)->s.f.chroms.size() : -1; }
const char *pb_bigwig_summary_chrom(void *h, int i) { return static_cast<SummaryRead *>(h)->s.f.chroms[(size_t)i].name.c_str(); }
// nq queries of n_bins bins: contig[q] the place in the chromosome list (-1: the file lacks it).  out5: five columns of
// nq x n_bins doubles -- validCount, min, max, sum, sum of squares; a bin without data is all zeros.
int pb_bigwig_summary_query(void *h, int64_t nq, const int32_t *contig, const int64_t *start, const int64_t *end, int64_t n_bins, double *out5) {
    SummaryRead *r = static_cast<SummaryRead *>(h);
    if (!r || nq < 0 || (nq > 0 && (!contig || !start || !end || !out5))) return fail("pb_bigwig_summary_query: bad arguments");
    const std::string bad_args = pcbws::check_queries(nq, start, end, n_bins);
    if (!bad_args.empty()) return fail("pb_bigwig_summary_query: " + bad_args);
    std::vector<uint32_t> s32((size_t)nq), e32((size_t)nq);
    for (int64_t q = 0; q < nq; ++q) { s32[(size_t)q] = (uint32_t)start[q]; e32[(size_t)q] = (uint32_t)end[q]; }
    const int64_t total = nq * n_bins;
    std::vector<pcbws::Element> el((size_t)total);
    const std::string bad = r->s.summarize(nq, contig, s32.data(), e32.data(), (uint32_t)n_bins, zlib_raw_inflate, el.data());
    if (!bad.empty()) return fail(r->name + ": bigWig: " + bad);
    for (int64_t k = 0; k < total; ++k) {
        const pcbws::Element &x = el[(size_t)k];
        out5[k] = (double)x.valid; out5[total + k] = x.mn; out5[2 * total + k] = x.mx; out5[3 * total + k] = x.sum; out5[4 * total + k] = x.sumsq;
    }
    return 0;
}
// The five kinds of nq x n_bins elements (five columns, as pb_bigwig_summary_query and pc_bigwig_summary_query give them),
// by value_of: kinds5 holds five columns -- mean, min, max, coverage, std -- and `fill` where valid is 0.  Only the kinds
// whose bit is set in kinds_mask (bit k: kind k) are computed; the other columns are left as they are.
int pb_bigwig_summary_values(int64_t nq, const int64_t *start, const int64_t *end, int64_t n_bins, const double *el5, double fill, int kinds_mask, double *kinds5) {
    if (nq < 0 || (nq > 0 && (!start || !end || !el5 || !kinds5))) return fail("pb_bigwig_summary_values: bad arguments");
    const std::string bad_args = pcbws::check_queries(nq, start, end, n_bins);
    if (!bad_args.empty()) return fail("pb_bigwig_summary_values: " + bad_args);
    const int64_t total = nq * n_bins;
    for (int64_t q = 0; q < nq; ++q)
        for (int64_t i = 0; i < n_bins; ++i) {
            const int64_t k = q * n_bins + i;
            pcbws::Element x;
            x.valid = (uint32_t)el5[k]; x.mn = el5[total + k]; x.mx = el5[2 * total + k]; x.sum = el5[3 * total + k]; x.sumsq = el5[4 * total + k];
            for (int kind = 0; kind < pcbws::kKinds; ++kind)
                if (kinds_mask & (1 << kind)) kinds5[(int64_t)kind * total + k] = x.valid ? pcbws::value_of(x, kind, (uint32_t)start[q], (uint32_t)end[q], (uint32_t)n_bins) : fill;
        }
    return 0;
}
// per table ([0] the items, [1 + k] level k; at most max_tables of them): [0] records (-1: not read), [1] queries; *tables: how many there are
int pb_bigwig_summary_stats(void *h, int64_t *tables, int max_tables, int64_t *out2) {
    SummaryRead *r = static_cast<SummaryRead *>(h);
    if (!r || !tables || max_tables < 0 || (max_tables > 0 && !out2)) return fail("pb_bigwig_summary_stats: bad arguments");
    *tables = (int64_t)r->s.tables.size();
    for (size_t k = 0; k < r->s.tables.size() && k < (size_t)max_tables; ++k) {
        const pcbws::HostTable &t = r->s.tables[k];
        out2[2 * k] = t.loaded ? (int64_t)(k == 0 ? t.items.size() : t.zoom.size()) : -1;
        out2[2 * k + 1] = t.queries;
    }
    return 0;
}

} // extern "C"
