// canon_host.h -- host arithmetic of the CANONICAL stream (stage_kernels.hip.h, k_canon_buckets): the stream of a
// staged file regrouped for one point rule.  A point rule bins a single-run read (pos, L, strand) at pos + k(L, strand)
// and looks at L for nothing else, so all reads of a strand that share a mapped position can travel as ONE entry.  The
// window kernels are not told: an entry is an ordinary stream word whose length field names a CANONICAL length Lc of
// its strand -- a valid length with the smallest index kc = k(Lc, strand) -- and whose position is the read's, moved
// right by k(L, strand) - kc >= 0.  The entry table of k_hist_point adds kc back.
// Plain C++17 (no HIP): tests/canon_host_test.cpp compiles it on a machine without a GPU.
#pragma once
#include <cstdint>

namespace pccanon {

constexpr int kLenSlots = 256;      // aligned lengths a stream word can carry (0 .. 255)
constexpr int kMaxShift = 254;      // a shift is k - kc with 0 <= kc <= k <= 254 for a read the stream carries

// What the rule is made of.  kind: 0 fiveprime, 1 threeprime, 3 variable (the KIND of map_kleft); fw / rc: the offset
// tables of the variable rule (table_len entries each, -1: length not mapped); [fast_lo, fast_hi]: the aligned lengths
// the entry table of k_hist_point covers.
struct RuleIn {
    int kind = 0, param = 0;
    int table_len = 0;
    const int32_t *fw = nullptr, *rc = nullptr;
    int filt_on = 0, filt_min = 0, filt_max = -1;
    int fast_lo = 0, fast_hi = 0;
};

struct CanonRule {
    bool usable = false;            // some read is kept and every shift fits (D <= kMaxShift)
    int kc[2] = {-1, -1};           // per strand (0 forward, 1 reverse): the smallest index of a valid length, -1: no valid length
    int Lc[2] = {0, 0};             // ... and the smallest length that attains it
    int D = 0;                      // the largest shift
    int16_t shift[2 * kLenSlots];   // [L * 2 + strand]: k(L, strand) - kc(strand), -1: the read adds to nothing and is dropped
};

// map_kleft<KIND> of pc_kernels.hip.h for the point rules: the index from the left end of the read, -1: not mapped
inline int rule_index(const RuleIn &r, int L, bool rev) {
    if (r.kind == 0) return r.param >= L ? -1 : (rev ? L - 1 - r.param : r.param);
    if (r.kind == 1) return r.param >= L ? -1 : (rev ? r.param : L - 1 - r.param);
    if (r.kind == 3) {
        if (L >= r.table_len) return -1;
        const int32_t *tab = rev ? r.rc : r.fw;
        return tab ? tab[L] : -1;
    }
    return -1;
}

// size_ok of pc_kernels.hip.h
inline bool rule_size_ok(const RuleIn &r, int L) {
    return !r.filt_on || (L >= r.filt_min && (L <= r.filt_max || r.filt_max == -1));
}

inline CanonRule canon_rule(const RuleIn &r) {
    CanonRule c;
    for (int i = 0; i < 2 * kLenSlots; ++i) c.shift[i] = -1;
    if (r.kind != 0 && r.kind != 1 && r.kind != 3) return c;
    const int lo = r.fast_lo < 0 ? 0 : r.fast_lo, hi = r.fast_hi >= kLenSlots ? kLenSlots - 1 : r.fast_hi;
    auto valid_index = [&](int L, int s) {
        const int k = rule_index(r, L, s != 0);
        return (k >= 0 && rule_size_ok(r, L)) ? k : -1;
    };
    for (int s = 0; s < 2; ++s)
        for (int L = lo; L <= hi; ++L) {
            const int k = valid_index(L, s);
            if (k >= 0 && (c.kc[s] < 0 || k < c.kc[s])) { c.kc[s] = k; c.Lc[s] = L; }
        }
    bool fits = true;
    for (int s = 0; s < 2; ++s)
        for (int L = lo; L <= hi && c.kc[s] >= 0; ++L) {
            const int k = valid_index(L, s);
            if (k < 0) continue;
            const int d = k - c.kc[s];
            if (d > kMaxShift) { fits = false; continue; }
            c.shift[L * 2 + s] = (int16_t)d;
            if (d > c.D) c.D = d;
        }
    c.usable = fits && (c.kc[0] >= 0 || c.kc[1] >= 0);
    return c;
}

// The window kernels look for the entries of a window [a, e) at positions [a - Ws + 1, e) (Ws: the halo of the record
// stream); an entry with mapped position m sits at m - kc, so every strand needs kc < Ws.
inline bool canon_fits_halo(const CanonRule &c, int Ws) {
    return (c.kc[0] < 0 || c.kc[0] < Ws) && (c.kc[1] < 0 || c.kc[1] < Ws);
}

// buckets (of 2^shift positions) before its own a bucket's workgroup has to read: reads move right by at most D
inline int canon_buckets_back(const CanonRule &c, int shift) { return (c.D + (1 << shift) - 1) >> shift; }

} // namespace pccanon
