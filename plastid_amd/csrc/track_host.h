// track_host.h -- COUNT TRACKS AS TEXT (bedGraph, variableStep and fixedStep wiggle), line by line: the one parser of the
// host reader (bam_stager.cpp, pb_track_read) and of the device import (track_kernels.hip.h).  The contract is the
// reference's WiggleReader (plastid/readers/wiggle.py:43-174) restated:
//   - a line of white space only, or one whose first byte is '#', is skipped;
//   - the first white-space token decides: "track" changes nothing; "variableStep" / "fixedStep" is a DATA HEADER (state
//     back to chrom none, span 1, step 1, counter 1, then chrom= span= step= start= from its key=value tokens, up to the
//     first token that contains "description"); any other line of exactly four tokens is a bedGraph line whatever the
//     format was (state reset, format bedGraph; yields tok0, int(tok1), int(tok2), float(tok3)); every other line is a
//     data line, which yields under variableStep (int(tok0) - 1, + span, float(tok1)) and fixedStep (counter - 1, + span,
//     float(the line stripped); counter += step) and is skipped silently otherwise.
// Split into what one line can say on its own (classify_line), what the few lines that change the state say (parse_state:
// host only, they are the only lines the host of the device import ever looks at) and what a yielding line gives under
// its state (line_fields).  int / float are Python's: a PLAIN token -- [+-]?[0-9]{1,18}, and a decimal literal whose
// significand is at most 2^53 with a net power of ten within +-22 -- is converted by int_fast / value_plain, on the
// device too; every other token ESCAPES to int_full / value_full (grammar check, then strtod), host only.
// The way back (revision 16): grown_length, the one growth rule of import and writes; value_class / float_repr, Python's
// repr(float) -- plain values by a function the format kernel runs too, the others host only; put_bed_line & co, the bytes
// of an exported line through a sink that counts or stores; write_bedgraph_contig / write_variable_step_contig, the serial
// writers (genome_array.py:1996-2084), the model of the device export.  Revision 17: put_count_bed_line / put_count_var_line
// and write_count_bedgraph_contig / write_count_variable_step_contig, the same for the text BAMGenomeArray writes of a count
// vector (:990-1111; int64 or float64 cells, windows).
// The per-line functions carry PC_TRK_HD: __host__ __device__ under hipcc, nothing under a host compiler.
// Plain C++17 (no HIP): tests/track_host_test.cpp and tests/track_export_host_test.cpp compile it on a machine without a
// GPU, under the sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#if !defined(PC_TRK_NO_CHARCONV) && defined(__has_include)
#if __has_include(<charconv>)
#include <charconv>   // std::to_chars for doubles, where the library has it (float_repr)
#endif
#endif

#if defined(__HIPCC__)
#define PC_TRK_HD __host__ __device__
#else
#define PC_TRK_HD
#endif

namespace pctrack {

enum { kSkip = 0, kTrackLine = 1, kHeader = 2, kBed = 3, kData = 4 };          // class of a line
enum { kFmtNone = 0, kFmtBed = 1, kFmtVariable = 2, kFmtFixed = 3 };           // format of a state record

enum {
    kTrkOk = 0,
    kTrkBadInt = 1, kTrkBadValue, kTrkNegStart, kTrkNoChrom, kTrkFixedTokens, kTrkVarTokens, kTrkHeaderKey, kTrkHeaderEq,
    kTrkHeaderInt, kTrkTooFar, kTrkHeaderRange,
    kTrkCodeEnd
};

inline const char *track_defect_text(int code) {
    switch (code) {
    case kTrkBadInt: return "a coordinate is not an integer";
    case kTrkBadValue: return "the value is not a number";
    case kTrkNegStart: return "negative start";
    case kTrkNoChrom: return "data line under a header without chrom=";
    case kTrkFixedTokens: return "fixedStep data line of more than one token";
    case kTrkVarTokens: return "variableStep data line without a value";
    case kTrkHeaderKey: return "data header token without '=' before any key";
    case kTrkHeaderEq: return "data header token with more than one '='";
    case kTrkHeaderInt: return "span, step or start of a data header is not an integer";
    case kTrkTooFar: return "coordinate beyond 2^40";
    case kTrkHeaderRange: return "span or step beyond 2^31, or start beyond 2^40";
    default: return "malformed line";
    }
}
// `line`: 1-based
inline std::string track_defect_message(const char *path, int64_t line, int code) {
    return std::string(path ? path : "<memory>") + ": track line " + std::to_string((long long)line) + ": " + track_defect_text(code);
}

constexpr int64_t kMaxCoord = (int64_t)1 << 40;      // starts and ends lie in [0, 2^40]
constexpr int64_t kMaxStep = (int64_t)1 << 31;       // |span|, |step| of a header

// str.split()'s white space among the ASCII bytes (bytes from 0x80 on are never white space here)
PC_TRK_HD inline bool is_space(uint8_t c) { return c == 32u || (c >= 9u && c <= 13u) || (c >= 28u && c <= 31u); }

struct Tok { const uint8_t *b, *e; };

// the next token at or behind p (b == e == end: none)
PC_TRK_HD inline Tok next_token(const uint8_t *p, const uint8_t *end) {
    while (p < end && is_space(*p)) ++p;
    Tok t{p, p};
    while (t.e < end && !is_space(*t.e)) ++t.e;
    return t;
}

PC_TRK_HD inline bool tok_is(const Tok &t, const char *word) {
    const uint8_t *p = t.b;
    for (; *word; ++word, ++p)
        if (p >= t.e || *p != (uint8_t)*word) return false;
    return p == t.e;
}

PC_TRK_HD inline bool tok_equal(const Tok &a, const Tok &b) {
    if (a.e - a.b != b.e - b.b) return false;
    for (ptrdiff_t k = 0; k < a.e - a.b; ++k)
        if (a.b[k] != b.b[k]) return false;
    return true;
}

// What a line says on its own.  ntok: its tokens, counted up to 5; tok: the first four.
struct LineClass {
    int cls;
    int ntok;
    Tok tok[4];
};

PC_TRK_HD inline LineClass classify_line(const uint8_t *b, const uint8_t *e) {
    LineClass c;
    c.cls = kSkip; c.ntok = 0;
    for (int k = 0; k < 4; ++k) c.tok[k] = Tok{e, e};
    const bool comment = b < e && *b == (uint8_t)'#';
    const uint8_t *p = b;
    while (c.ntok < 5) {
        const Tok t = next_token(p, e);
        if (t.b == t.e) break;
        if (c.ntok < 4) c.tok[c.ntok] = t;
        ++c.ntok;
        p = t.e;
    }
    if (c.ntok == 0 || comment) return c;
    if (tok_is(c.tok[0], "track")) c.cls = kTrackLine;
    else if (tok_is(c.tok[0], "variableStep") || tok_is(c.tok[0], "fixedStep")) c.cls = kHeader;
    else if (c.ntok == 4) c.cls = kBed;
    else c.cls = kData;
    return c;
}

// ---------------------------------------------------------------- numbers

// [+-]?[0-9]{1,18}
PC_TRK_HD inline bool int_fast(const uint8_t *b, const uint8_t *e, int64_t &v) {
    bool neg = false;
    if (b < e && (*b == (uint8_t)'+' || *b == (uint8_t)'-')) { neg = *b == (uint8_t)'-'; ++b; }
    if (e - b < 1 || e - b > 18) return false;
    int64_t x = 0;
    for (; b < e; ++b) {
        const uint32_t d = (uint32_t)*b - (uint32_t)'0';
        if (d > 9u) return false;
        x = x * 10 + (int64_t)d;
    }
    v = neg ? -x : x;
    return true;
}

// 10^k, k = 0 .. 22: the powers of ten a double holds exactly
PC_TRK_HD inline double pow10_exact(int k) {
    constexpr double t[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20,
                              1e21, 1e22};
    return t[k];
}

// A PLAIN value: [+-]?digits[.digits][e[+-]digits], the significand (leading zeros stripped) at most 2^53, the net power of
// ten within +-22.  Then significand and power are both exact doubles and one IEEE multiply or divide is the correctly
// rounded value, which is what strtod gives.  (The build must not contract or reassociate: -ffp-contract=off.)
PC_TRK_HD inline bool value_plain(const uint8_t *b, const uint8_t *e, double &v) {
    bool neg = false;
    if (b < e && (*b == (uint8_t)'+' || *b == (uint8_t)'-')) { neg = *b == (uint8_t)'-'; ++b; }
    uint64_t sig = 0;
    int nsig = 0, nint = 0, nfrac = 0;
    for (; b < e; ++b, ++nint) {
        const uint32_t d = (uint32_t)*b - (uint32_t)'0';
        if (d > 9u) break;
        if (sig != 0 || d != 0) { if (++nsig > 17) return false; sig = sig * 10u + d; }
    }
    if (nint == 0) return false;
    if (b < e && *b == (uint8_t)'.') {
        ++b;
        for (; b < e; ++b, ++nfrac) {
            const uint32_t d = (uint32_t)*b - (uint32_t)'0';
            if (d > 9u) break;
            if (sig != 0 || d != 0) { if (++nsig > 17) return false; sig = sig * 10u + d; }
        }
        if (nfrac == 0) return false;
    }
    int ex = 0;
    if (b < e && (*b == (uint8_t)'e' || *b == (uint8_t)'E')) {
        ++b;
        bool eneg = false;
        if (b < e && (*b == (uint8_t)'+' || *b == (uint8_t)'-')) { eneg = *b == (uint8_t)'-'; ++b; }
        int nexp = 0;
        for (; b < e; ++b, ++nexp) {
            const uint32_t d = (uint32_t)*b - (uint32_t)'0';
            if (d > 9u) break;
            if (ex < 100000) ex = ex * 10 + (int)d;
        }
        if (nexp == 0) return false;
        if (eneg) ex = -ex;
    }
    if (b != e) return false;
    if (sig > ((uint64_t)1 << 53)) return false;
    const int net = ex - nfrac;
    if (net > 22 || net < -22) return false;
    const double m = (double)sig;                       // exact: sig <= 2^53
    const double x = net >= 0 ? m * pow10_exact(net) : m / pow10_exact(-net);
    v = neg ? -x : x;
    return true;
}

// ---- host only: Python's int() and float() for the tokens that are not plain

inline bool ascii_ieq(const std::string &s, const char *word) {
    size_t k = 0;
    for (; word[k]; ++k)
        if (k >= s.size() || (char)(s[k] | 0x20) != word[k]) return false;
    return k == s.size();
}

// digits with single underscores between them, from s[at]; the digits are appended to `out`.  False: none, or a misplaced '_'
inline bool py_digits(const std::string &s, size_t &at, std::string &out) {
    size_t n = 0;
    bool last_us = false;
    while (at < s.size()) {
        const char c = s[at];
        if (c >= '0' && c <= '9') { out.push_back(c); ++n; last_us = false; }
        else if (c == '_' && n > 0 && !last_us) last_us = true;
        else break;
        ++at;
    }
    return n > 0 && !last_us;
}

// int(token), base 10: sign, digits with single underscores; here within the int64 range
inline bool int_full(const uint8_t *b, const uint8_t *e, int64_t &v) {
    const std::string s((const char *)b, (size_t)(e - b));
    size_t at = 0;
    bool neg = false;
    if (at < s.size() && (s[at] == '+' || s[at] == '-')) { neg = s[at] == '-'; ++at; }
    std::string digits;
    if (!py_digits(s, at, digits) || at != s.size()) return false;
    size_t z = 0;
    while (z + 1 < digits.size() && digits[z] == '0') ++z;
    if (digits.size() - z > 18) return false;
    int64_t x = 0;
    for (; z < digits.size(); ++z) x = x * 10 + (digits[z] - '0');
    v = neg ? -x : x;
    return true;
}

// float(token): sign, then inf / infinity / nan in any case, or a decimal literal (digits with single underscores, at
// least one digit in front of or behind the point, an optional exponent); never hex.  The checked text goes to strtod.
inline bool value_full(const uint8_t *b, const uint8_t *e, double &v) {
    const std::string s((const char *)b, (size_t)(e - b));
    size_t at = 0;
    std::string clean;
    if (at < s.size() && (s[at] == '+' || s[at] == '-')) { clean.push_back(s[at]); ++at; }
    const std::string rest = s.substr(at);
    if (ascii_ieq(rest, "inf") || ascii_ieq(rest, "infinity")) { v = clean == "-" ? -HUGE_VAL : HUGE_VAL; return true; }
    if (ascii_ieq(rest, "nan")) { v = std::strtod("nan", nullptr); return true; }
    bool any = false;
    if (at < s.size() && s[at] != '.') {
        if (!py_digits(s, at, clean)) return false;
        any = true;
    }
    if (at < s.size() && s[at] == '.') {
        clean.push_back('.');
        ++at;
        if (at < s.size() && s[at] >= '0' && s[at] <= '9') {
            if (!py_digits(s, at, clean)) return false;
            any = true;
        }
    }
    if (!any) return false;
    if (at < s.size() && (s[at] == 'e' || s[at] == 'E')) {
        clean.push_back('e');
        ++at;
        if (at < s.size() && (s[at] == '+' || s[at] == '-')) { clean.push_back(s[at]); ++at; }
        if (!py_digits(s, at, clean)) return false;
    }
    if (at != s.size()) return false;
    char *endp = nullptr;
    v = std::strtod(clean.c_str(), &endp);
    return endp && *endp == 0;
}

// ---------------------------------------------------------------- state records

// One line that changes the reader's state: a data header, or a bedGraph line that names another contig than the
// bedGraph line before it (or follows a data header).  Every other line is governed by the last record at or above it.
struct StateRec {
    int64_t line;        // 0-based line number
    int32_t format;      // kFmtBed, kFmtVariable, kFmtFixed
    int32_t contig;      // id of the contig, -1: none (a header without chrom=)
    int64_t span, step, start;
    int64_t data_base;   // data lines in front of the record's line (fixedStep: the counter of data line d is start + step * (d - data_base))
};

// the record that governs `line`: the last one with rec.line <= line, -1: none
PC_TRK_HD inline int64_t governing(const StateRec *recs, int64_t nrec, int64_t line) {
    int64_t lo = 0, hi = nrec;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (recs[mid].line <= line) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// Host only.  The state record of a header or bedGraph line; `contig_of(name)` resolves or creates the id.  Returns a
// defect code.
template <typename ContigOf>
inline int parse_state(const uint8_t *b, const uint8_t *e, int64_t line, int64_t data_base, ContigOf contig_of, StateRec &r) {
    r.line = line; r.contig = -1; r.span = 1; r.step = 1; r.start = 1; r.data_base = data_base;
    const Tok t0 = next_token(b, e);
    const bool var = tok_is(t0, "variableStep"), fixed = tok_is(t0, "fixedStep");
    if (!var && !fixed) {
        r.format = kFmtBed;
        r.contig = contig_of(std::string((const char *)t0.b, (size_t)(t0.e - t0.b)));
        return kTrkOk;
    }
    r.format = var ? kFmtVariable : kFmtFixed;
    std::map<std::string, std::string> kv;
    std::string key;
    bool have_key = false;
    for (const uint8_t *p = t0.e;;) {
        const Tok t = next_token(p, e);
        if (t.b == t.e) break;
        p = t.e;
        const std::string item((const char *)t.b, (size_t)(t.e - t.b));
        if (item.find("description") != std::string::npos) break;
        const size_t eq = item.find('=');
        if (eq == std::string::npos) {
            if (!have_key) return kTrkHeaderKey;
            kv[key] = "true";
            continue;
        }
        if (item.find('=', eq + 1) != std::string::npos) return kTrkHeaderEq;
        key = item.substr(0, eq);
        have_key = true;
        kv[key] = item.substr(eq + 1);
    }
    auto it = kv.find("chrom");
    if (it != kv.end()) r.contig = contig_of(it->second);
    struct Field { const char *name; int64_t *dst; int64_t max; } fields[3] = {{"span", &r.span, kMaxStep}, {"step", &r.step, kMaxStep}, {"start", &r.start, kMaxCoord}};
    for (const Field &f : fields) {
        it = kv.find(f.name);
        if (it == kv.end()) continue;
        const uint8_t *vb = (const uint8_t *)it->second.data(), *ve = vb + it->second.size();
        int64_t x;
        if (!int_fast(vb, ve, x) && !int_full(vb, ve, x)) return kTrkHeaderInt;
        if (x > f.max || x < -f.max) return kTrkHeaderRange;
        *f.dst = x;
    }
    return kTrkOk;
}

// ---------------------------------------------------------------- yielding lines

// converters of the device: a token that is not plain escapes
struct FastOnly {
    PC_TRK_HD static bool to_int(const uint8_t *b, const uint8_t *e, int64_t &v, bool &escaped, int &) {
        if (int_fast(b, e, v)) return true;
        escaped = true; v = 0;
        return true;
    }
    PC_TRK_HD static bool to_value(const uint8_t *b, const uint8_t *e, double &v, bool &escaped, int &) {
        if (value_plain(b, e, v)) return true;
        escaped = true; v = 0.0;
        return true;
    }
};
// converters of the host: the same functions first, Python's grammar behind them
struct FastThenFull {
    static bool to_int(const uint8_t *b, const uint8_t *e, int64_t &v, bool &escaped, int &err) {
        if (int_fast(b, e, v)) return true;
        escaped = true;
        if (int_full(b, e, v)) return true;
        err = kTrkBadInt;
        return false;
    }
    static bool to_value(const uint8_t *b, const uint8_t *e, double &v, bool &escaped, int &err) {
        if (value_plain(b, e, v)) return true;
        escaped = true;
        if (value_full(b, e, v)) return true;
        err = kTrkBadValue;
        return false;
    }
};

struct LineOut {
    int64_t start, stop;
    double value;
    int32_t contig;
    bool yields;      // the line gives a (contig, start, stop, value)
    bool escaped;     // a token was not plain (FastOnly: start / stop / value are not final then)
    int err;
};

// What line `c` yields under record `r` (nullptr: none governs it); data_index: data lines in front of it.
template <typename Conv>
PC_TRK_HD inline LineOut line_fields(const LineClass &c, const StateRec *r, int64_t data_index) {
    LineOut o;
    o.start = 0; o.stop = 0; o.value = 0.0; o.contig = -1; o.yields = false; o.escaped = false; o.err = kTrkOk;
    if (c.cls != kBed && c.cls != kData) return o;
    if (!r) return o;
    if (c.cls == kBed) {
        o.yields = true;
        o.contig = r->contig;
        if (!Conv::to_int(c.tok[1].b, c.tok[1].e, o.start, o.escaped, o.err)) return o;
        if (!Conv::to_int(c.tok[2].b, c.tok[2].e, o.stop, o.escaped, o.err)) return o;
        if (!Conv::to_value(c.tok[3].b, c.tok[3].e, o.value, o.escaped, o.err)) return o;
    } else if (r->format == kFmtVariable) {
        o.yields = true;
        o.contig = r->contig;
        if (c.ntok < 2) { o.err = kTrkVarTokens; return o; }
        int64_t at = 0;
        if (!Conv::to_int(c.tok[0].b, c.tok[0].e, at, o.escaped, o.err)) return o;
        o.start = at - 1;
        o.stop = o.start + r->span;
        if (!Conv::to_value(c.tok[1].b, c.tok[1].e, o.value, o.escaped, o.err)) return o;
    } else if (r->format == kFmtFixed) {
        o.yields = true;
        o.contig = r->contig;
        if (c.ntok != 1) { o.err = kTrkFixedTokens; return o; }
        o.start = r->start + r->step * (data_index - r->data_base) - 1;
        o.stop = o.start + r->span;
        if (!Conv::to_value(c.tok[0].b, c.tok[0].e, o.value, o.escaped, o.err)) return o;
    }
    return o;
}

// the checks on the final numbers of a yielding line
PC_TRK_HD inline int check_fields(const LineOut &o) {
    if (o.contig < 0) return kTrkNoChrom;
    if (o.start < 0) return kTrkNegStart;
    if (o.start > kMaxCoord || o.stop > kMaxCoord) return kTrkTooFar;
    return kTrkOk;
}

// ---------------------------------------------------------------- the host reader (the model of the device import)

struct TrackTable {
    std::vector<std::string> names;            // contigs in order of first appearance among the yielded lines
    std::vector<int32_t> contig;
    std::vector<int64_t> start, stop;
    std::vector<double> value;
    std::vector<int64_t> line;                 // 0-based line of every row
    std::vector<uint8_t> escaped;              // the row had a token that is not plain
    int64_t lines = 0, states = 0, n_escaped = 0;
    int defect = kTrkOk;
    int64_t defect_line = 0;                   // 1-based
};

// Reads the whole text in file order; stops at the first defect (t.defect, t.defect_line).
inline void read_track(const uint8_t *text, size_t size, TrackTable &t) {
    std::map<std::string, int32_t> ids;        // provisional ids, in order of first mention
    std::vector<std::string> mentioned;
    std::vector<int32_t> public_id;            // provisional id -> index into t.names, -1: nothing yielded on it yet
    auto contig_of = [&](const std::string &name) {
        auto it = ids.find(name);
        if (it != ids.end()) return it->second;
        const int32_t id = (int32_t)mentioned.size();
        ids.emplace(name, id);
        mentioned.push_back(name);
        public_id.push_back(-1);
        return id;
    };
    StateRec rec;
    bool have_rec = false;
    Tok last_bed{nullptr, nullptr};
    bool bed_follows_bed = false;              // the last header or bedGraph line was a bedGraph line
    int64_t data_lines = 0, line = 0;
    const uint8_t *p = text, *end = text + size;
    while (p < end) {
        const uint8_t *le = (const uint8_t *)memchr(p, '\n', (size_t)(end - p));
        if (!le) le = end;
        const LineClass c = classify_line(p, le);
        int err = kTrkOk;
        if (c.cls == kHeader || (c.cls == kBed && !(bed_follows_bed && tok_equal(last_bed, c.tok[0])))) {
            err = parse_state(p, le, line, data_lines, contig_of, rec);
            have_rec = true;
            t.states += 1;
        }
        if (c.cls == kHeader) bed_follows_bed = false;
        if (c.cls == kBed) { bed_follows_bed = true; last_bed = c.tok[0]; }
        if (err == kTrkOk) {
            const LineOut o = line_fields<FastThenFull>(c, have_rec ? &rec : nullptr, data_lines);
            err = o.err;
            if (err == kTrkOk && o.yields) err = check_fields(o);
            if (err == kTrkOk && o.yields) {
                if (public_id[(size_t)o.contig] < 0) { public_id[(size_t)o.contig] = (int32_t)t.names.size(); t.names.push_back(mentioned[(size_t)o.contig]); }
                t.contig.push_back(public_id[(size_t)o.contig]);
                t.start.push_back(o.start); t.stop.push_back(o.stop); t.value.push_back(o.value);
                t.line.push_back(line); t.escaped.push_back(o.escaped ? 1 : 0);
                t.n_escaped += o.escaped ? 1 : 0;
            }
        }
        if (err != kTrkOk) { t.defect = err; t.defect_line = line + 1; t.lines = line + 1; return; }
        if (c.cls == kData) ++data_lines;
        ++line;
        p = le < end ? le + 1 : end;
    }
    t.lines = line;
}

// ---------------------------------------------------------------- growth (genome_array.py:1593-1602)

// The length of a contig after a write (or an imported line) that ends at `end`: reaching the length sets it to
// max(len, end) + 10000.  The one rule of the import and of pc_track_set.
PC_TRK_HD inline int64_t grown_length(int64_t len, int64_t end) { return end >= len ? (len > end ? len : end) + 10000 : len; }

// ---------------------------------------------------------------- export: values as text

// A value is PLAIN when it is an integer of magnitude below 10^16: Python's repr is its digits and ".0" (the count-track
// case; -0.0 is "-0.0").  nan / inf / -inf are kSpecial.  Every other finite value is LISTED: float_repr, host only.
enum { kValPlain = 0, kValSpecial = 1, kValListed = 2 };
constexpr int kReprMax = 24;                       // "-1.7976931348623157e+308"

PC_TRK_HD inline int value_class(double v) {
    if (v != v || v - v != 0.0) return kValSpecial;             // nan, +-inf
    const double a = v < 0 ? -v : v;
    if (a < 1e16 && (double)(int64_t)a == a) return kValPlain;
    return kValListed;
}
PC_TRK_HD inline bool sign_bit(double v) {
    uint64_t u;
    __builtin_memcpy(&u, &v, 8);
    return (u >> 63) != 0;
}
PC_TRK_HD inline int dec_digits(uint64_t x) {
    int n = 1;
    while (x >= 10u) { x /= 10u; ++n; }
    return n;
}
// a sink takes bytes: CountSink counts them, WriteSink stores them
struct CountSink {
    int64_t n = 0;
    PC_TRK_HD void put(uint8_t) { ++n; }
};
struct WriteSink {
    uint8_t *p;
    PC_TRK_HD void put(uint8_t c) { *p++ = c; }
};
template <typename Sink> PC_TRK_HD inline void put_uint(Sink &s, uint64_t x) {
    uint8_t d[20];
    int n = 0;
    do { d[n++] = (uint8_t)('0' + x % 10u); x /= 10u; } while (x);
    while (n) s.put(d[--n]);
}
template <typename Sink> PC_TRK_HD inline void put_bytes(Sink &s, const uint8_t *b, int64_t n) {
    for (int64_t k = 0; k < n; ++k) s.put(b[k]);
}
template <typename Sink> PC_TRK_HD inline void put_word(Sink &s, const char *w) {
    for (; *w; ++w) s.put((uint8_t)*w);
}
// a plain or special value (value_class says which)
template <typename Sink> PC_TRK_HD inline void put_simple_value(Sink &s, double v) {
    if (v != v) { put_word(s, "nan"); return; }
    if (v - v != 0.0) { put_word(s, v < 0 ? "-inf" : "inf"); return; }
    if (sign_bit(v)) s.put((uint8_t)'-');
    put_uint(s, (uint64_t)(int64_t)(v < 0 ? -v : v));
    put_word(s, ".0");
}

// Host only.  The shortest digits that read back as `v` (v finite, not zero), without sign or point, and the power of
// ten of the first digit.
inline void shortest_digits(double v, char *digits, int &ndig, int &exp10) {
    char buf[48];
    const double a = v < 0 ? -v : v;
#if defined(__cpp_lib_to_chars) && !defined(PC_TRK_NO_CHARCONV)
    const auto r = std::to_chars(buf, buf + sizeof(buf) - 1, a, std::chars_format::scientific);
    *r.ptr = 0;
#else
    for (int prec = 0; prec < 17; ++prec) {
        snprintf(buf, sizeof(buf), "%.*e", prec, a);
        if (std::strtod(buf, nullptr) == a) break;
    }
#endif
    ndig = 0;
    const char *p = buf;
    for (; *p && *p != 'e'; ++p)
        if (*p >= '0' && *p <= '9') digits[ndig++] = *p;
    exp10 = *p == 'e' ? atoi(p + 1) : 0;
    while (ndig > 1 && digits[ndig - 1] == '0') --ndig;
}

// repr(float(v)) into out (kReprMax bytes at least); returns the length.  Python's layout: the shortest digits that
// round-trip, in exponent form ("d.ddde-05", at least two exponent digits) below 1e-4 and from 1e16 on, else with a point.
inline int float_repr(double v, char *out) {
    WriteSink s{(uint8_t *)out};
    if (value_class(v) != kValListed) { put_simple_value(s, v); return (int)((char *)s.p - out); }
    char dg[24];
    int nd = 0, e10 = 0;
    shortest_digits(v, dg, nd, e10);
    if (v < 0) s.put((uint8_t)'-');
    if (e10 < -4 || e10 >= 16) {
        s.put((uint8_t)dg[0]);
        if (nd > 1) { s.put((uint8_t)'.'); put_bytes(s, (const uint8_t *)dg + 1, nd - 1); }
        s.put((uint8_t)'e');
        s.put((uint8_t)(e10 < 0 ? '-' : '+'));
        const unsigned ae = (unsigned)(e10 < 0 ? -e10 : e10);
        if (ae < 10u) s.put((uint8_t)'0');
        put_uint(s, ae);
    } else if (e10 >= 0) {
        for (int k = 0; k <= e10; ++k) s.put((uint8_t)(k < nd ? dg[k] : '0'));
        s.put((uint8_t)'.');
        if (nd > e10 + 1) put_bytes(s, (const uint8_t *)dg + e10 + 1, nd - e10 - 1); else s.put((uint8_t)'0');
    } else {
        put_word(s, "0.");
        for (int k = 0; k < -e10 - 1; ++k) s.put((uint8_t)'0');
        put_bytes(s, (const uint8_t *)dg, nd);
    }
    return (int)((char *)s.p - out);
}

// ---------------------------------------------------------------- export: the lines (genome_array.py:1996-2084)

// "chrom\tstart\tend\tvalue\n"; `vtext` (length vlen): the value of a listed run, nullptr: plain or special
template <typename Sink> PC_TRK_HD inline void put_bed_line(Sink &s, const uint8_t *name, int64_t name_len, int64_t a, int64_t b, double v,
                                                            const uint8_t *vtext, int vlen) {
    put_bytes(s, name, name_len); s.put(9); put_uint(s, (uint64_t)a); s.put(9); put_uint(s, (uint64_t)b); s.put(9);
    if (vtext) put_bytes(s, vtext, vlen); else put_simple_value(s, v);
    s.put(10);
}
// the leading line of a contig: "chrom\t0\t<first>\t0\n" (the integer 0 the reference's loop starts with)
template <typename Sink> PC_TRK_HD inline void put_bed_lead(Sink &s, const uint8_t *name, int64_t name_len, int64_t first) {
    put_bytes(s, name, name_len); s.put(9); s.put((uint8_t)'0'); s.put(9); put_uint(s, (uint64_t)first); s.put(9); s.put((uint8_t)'0'); s.put(10);
}
template <typename Sink> PC_TRK_HD inline void put_var_header(Sink &s, const uint8_t *name, int64_t name_len) {
    put_word(s, "variableStep chrom="); put_bytes(s, name, name_len); put_word(s, " span=1"); s.put(10);
}
// "<i + 1>\tvalue\n"
template <typename Sink> PC_TRK_HD inline void put_var_line(Sink &s, int64_t i, double v, const uint8_t *vtext, int vlen) {
    put_uint(s, (uint64_t)(i + 1)); s.put(9);
    if (vtext) put_bytes(s, vtext, vlen); else put_simple_value(s, v);
    s.put(10);
}

// Host only: the serial writers, the model of the device export.  stats: lines, runs (bedGraph) or non-zero cells
// (variableStep), values that are not plain (they go through float_repr), bytes.
struct ExportStats { int64_t lines = 0, runs = 0, listed = 0, bytes = 0; };

struct StringSink {
    std::string *out;
    void put(uint8_t c) { out->push_back((char)c); }
};
inline void host_value(const double v, char *buf, const uint8_t *&vtext, int &vlen, ExportStats &st) {
    vtext = nullptr; vlen = 0;
    if (value_class(v) == kValListed) { vlen = float_repr(v, buf); vtext = (const uint8_t *)buf; st.listed += 1; }
}

// One contig's strand as bedGraph: nothing unless its sum is > 0; the leading line, then the runs of equal value (by !=)
// from the first to the last non-zero cell.
inline void write_bedgraph_contig(std::string &out, const std::string &name, const double *v, int64_t n, ExportStats &st) {
    double sum = 0.0;
    int64_t first = -1, last = -1;
    for (int64_t i = 0; i < n; ++i) {
        sum = sum + v[i];
        if (v[i] != 0.0) { if (first < 0) first = i; last = i; }
    }
    if (!(sum > 0.0) || first < 0) return;
    const size_t before = out.size();
    StringSink s{&out};
    const uint8_t *nm = (const uint8_t *)name.data();
    put_bed_lead(s, nm, (int64_t)name.size(), first);
    st.lines += 1;
    char buf[kReprMax + 8];
    int64_t head = first;
    for (int64_t x = first + 1; x <= last + 1; ++x) {
        if (x <= last && !(v[x] != v[head])) continue;
        const uint8_t *vt; int vl;
        host_value(v[head], buf, vt, vl, st);
        put_bed_line(s, nm, (int64_t)name.size(), head, x, v[head], vt, vl);
        st.lines += 1; st.runs += 1;
        head = x;
    }
    st.bytes += (int64_t)(out.size() - before);
}

// One contig's strand as variableStep: the header whatever the cells hold, then a line per non-zero cell.
inline void write_variable_step_contig(std::string &out, const std::string &name, const double *v, int64_t n, ExportStats &st) {
    const size_t before = out.size();
    StringSink s{&out};
    put_var_header(s, (const uint8_t *)name.data(), (int64_t)name.size());
    st.lines += 1;
    char buf[kReprMax + 8];
    for (int64_t i = 0; i < n; ++i) {
        if (!(v[i] != 0.0)) continue;
        const uint8_t *vt; int vl;
        host_value(v[i], buf, vt, vl, st);
        put_var_line(s, i, v[i], vt, vl);
        st.lines += 1; st.runs += 1;
    }
    st.bytes += (int64_t)(out.size() - before);
}

// ---------------------------------------------------------------- export of a COUNT VECTOR (genome_array.py:990-1111)
// BAMGenomeArray's text differs from GenomeArray's: the vector is cut into windows of `window` positions, inside a window
// every maximal run of equal value whose value is > 0 is a bedGraph line (no leading line, no header; a run across a
// window border is two lines); variableStep writes the header, then every non-zero position.  The cells are int64
// counts -- "%s" % numpy.int64: the decimal digits -- or float64 values (normalised counts, the center rule):
// repr(float), plain by put_simple_value, listed by float_repr.  Revision 17.

PC_TRK_HD inline bool count_listed(int64_t) { return false; }
PC_TRK_HD inline bool count_listed(double v) { return value_class(v) == kValListed; }
template <typename Sink> PC_TRK_HD inline void put_count(Sink &s, int64_t v, const uint8_t *, int) {
    if (v < 0) { s.put((uint8_t)'-'); put_uint(s, (uint64_t)0 - (uint64_t)v); } else put_uint(s, (uint64_t)v);
}
template <typename Sink> PC_TRK_HD inline void put_count(Sink &s, double v, const uint8_t *vtext, int vlen) {
    if (vtext) put_bytes(s, vtext, vlen); else put_simple_value(s, v);
}
// "chrom\tstart\tend\tvalue\n"
template <typename Sink, typename T> PC_TRK_HD inline void put_count_bed_line(Sink &s, const uint8_t *name, int64_t name_len, int64_t a, int64_t b, T v,
                                                                              const uint8_t *vtext, int vlen) {
    put_bytes(s, name, name_len); s.put(9); put_uint(s, (uint64_t)a); s.put(9); put_uint(s, (uint64_t)b); s.put(9);
    put_count(s, v, vtext, vlen);
    s.put(10);
}
// "<i + 1>\tvalue\n"
template <typename Sink, typename T> PC_TRK_HD inline void put_count_var_line(Sink &s, int64_t i, T v, const uint8_t *vtext, int vlen) {
    put_uint(s, (uint64_t)(i + 1)); s.put(9);
    put_count(s, v, vtext, vlen);
    s.put(10);
}

inline void host_count_value(int64_t, char *, const uint8_t *&vtext, int &vlen, ExportStats &) { vtext = nullptr; vlen = 0; }
inline void host_count_value(double v, char *buf, const uint8_t *&vtext, int &vlen, ExportStats &st) { host_value(v, buf, vtext, vlen, st); }

// Host only: one contig's vector as bedGraph.  stats: written lines, runs of any value (the run table of the device
// export), listed values among the written lines, bytes.
template <typename T> inline void write_count_bedgraph_contig(std::string &out, const std::string &name, const T *v, int64_t n, int64_t window, ExportStats &st) {
    if (n <= 0 || window < 1) return;
    const size_t before = out.size();
    StringSink s{&out};
    const uint8_t *nm = (const uint8_t *)name.data();
    char buf[kReprMax + 8];
    for (int64_t w0 = 0; w0 < n;) {
        const int64_t w1 = n - w0 > window ? w0 + window : n;
        int64_t head = w0;
        for (int64_t x = w0 + 1; x <= w1; ++x) {
            if (x < w1 && !(v[x] != v[x - 1])) continue;
            st.runs += 1;
            if (v[head] > 0) {
                const uint8_t *vt; int vl;
                host_count_value(v[head], buf, vt, vl, st);
                put_count_bed_line(s, nm, (int64_t)name.size(), head, x, v[head], vt, vl);
                st.lines += 1;
            }
            head = x;
        }
        w0 = w1;
    }
    st.bytes += (int64_t)(out.size() - before);
}

// Host only: one contig's vector as variableStep: the header whatever the length, then a line per non-zero position.
template <typename T> inline void write_count_variable_step_contig(std::string &out, const std::string &name, const T *v, int64_t n, ExportStats &st) {
    const size_t before = out.size();
    StringSink s{&out};
    put_var_header(s, (const uint8_t *)name.data(), (int64_t)name.size());
    st.lines += 1;
    char buf[kReprMax + 8];
    for (int64_t i = 0; i < n; ++i) {
        if (!(v[i] != 0)) continue;
        const uint8_t *vt; int vl;
        host_count_value(v[i], buf, vt, vl, st);
        put_count_var_line(s, i, v[i], vt, vl);
        st.lines += 1; st.runs += 1;
    }
    st.bytes += (int64_t)(out.size() - before);
}

} // namespace pctrack
