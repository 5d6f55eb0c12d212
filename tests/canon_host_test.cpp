// canon_host_test.cpp -- plastid_amd/csrc/canon_host.h on a machine without a GPU (tests/test_canon_host.py compiles
// and runs it, under the address and undefined-behaviour sanitizers where the compiler has them).  Hand-checked rules,
// then every rule against a brute-force model: the bin a read gets through its canonical entry is the bin it had.
#include "canon_host.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace pccanon;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { ++failures; fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static RuleIn rule(int kind, int param, int lo, int hi, const std::vector<int32_t> *fw = nullptr, const std::vector<int32_t> *rc = nullptr) {
    RuleIn r;
    r.kind = kind; r.param = param; r.fast_lo = lo; r.fast_hi = hi;
    if (fw) { r.fw = fw->data(); r.rc = rc->data(); r.table_len = (int)fw->size(); }
    return r;
}

// every (L, strand) of the stream: dropped exactly when the kernels would bin nothing, else shift + kc == k
static void check_against_model(const RuleIn &r, const CanonRule &c) {
    int D = 0;
    bool any = false;
    for (int s = 0; s < 2; ++s) {
        int kmin = -1, lmin = 0;
        for (int L = 0; L < kLenSlots; ++L) {
            const bool in_table = L >= r.fast_lo && L <= r.fast_hi;
            const int k = rule_index(r, L, s != 0);
            const bool valid = in_table && k >= 0 && rule_size_ok(r, L);
            if (!valid) { CHECK(c.shift[L * 2 + s] == -1); continue; }
            any = true;
            if (kmin < 0 || k < kmin) { kmin = k; lmin = L; }
        }
        CHECK(c.kc[s] == kmin);
        if (kmin < 0) continue;
        CHECK(c.Lc[s] == lmin);
        CHECK(c.shift[c.Lc[s] * 2 + s] == 0);
        for (int L = r.fast_lo; L <= r.fast_hi && L < kLenSlots; ++L) {
            const int k = rule_index(r, L, s != 0);
            if (k < 0 || !rule_size_ok(r, L)) continue;
            CHECK(c.shift[L * 2 + s] >= 0 && c.shift[L * 2 + s] <= kMaxShift);
            CHECK(c.shift[L * 2 + s] + c.kc[s] == k);   // pos + shift + k(Lc) == pos + k(L): the bin the read had
            if (c.shift[L * 2 + s] > D) D = c.shift[L * 2 + s];
        }
    }
    CHECK(c.usable == any);
    CHECK(c.D == D);
    CHECK(canon_buckets_back(c, 7) == (D + 127) / 128);
}

int main() {
    {   // fiveprime 12 over lengths 20 .. 40: forward reads all map at 12 (no shift), reverse at L - 13
        const RuleIn r = rule(0, 12, 20, 40);
        const CanonRule c = canon_rule(r);
        CHECK(c.usable && c.kc[0] == 12 && c.Lc[0] == 20 && c.kc[1] == 7 && c.Lc[1] == 20 && c.D == 20);
        CHECK(c.shift[30 * 2 + 0] == 0 && c.shift[30 * 2 + 1] == 10 && c.shift[40 * 2 + 1] == 20);
        CHECK(c.shift[19 * 2 + 0] == -1 && c.shift[41 * 2 + 1] == -1);
        CHECK(canon_buckets_back(c, 7) == 1);
        CHECK(canon_fits_halo(c, 40) && canon_fits_halo(c, 13) && !canon_fits_halo(c, 12));
        check_against_model(r, c);
    }
    {   // lengths at or below the offset are not mapped: param >= L
        const RuleIn r = rule(0, 12, 5, 40);
        const CanonRule c = canon_rule(r);
        CHECK(c.shift[12 * 2 + 0] == -1 && c.shift[12 * 2 + 1] == -1 && c.shift[13 * 2 + 0] == 0 && c.shift[13 * 2 + 1] == 0);
        CHECK(c.Lc[0] == 13 && c.Lc[1] == 13 && c.kc[1] == 0 && c.D == 27);
        check_against_model(r, c);
    }
    {   // threeprime 3: the strands change places
        const RuleIn r = rule(1, 3, 20, 40);
        const CanonRule c = canon_rule(r);
        CHECK(c.kc[0] == 16 && c.kc[1] == 3 && c.shift[40 * 2 + 0] == 20 && c.shift[40 * 2 + 1] == 0);
        check_against_model(r, c);
    }
    {   // fiveprime 0, one length
        const RuleIn r = rule(0, 0, 30, 30);
        const CanonRule c = canon_rule(r);
        CHECK(c.usable && c.D == 0 && c.kc[0] == 0 && c.kc[1] == 29 && canon_buckets_back(c, 7) == 0);
        CHECK(!canon_fits_halo(c, 29) && canon_fits_halo(c, 30));
        check_against_model(r, c);
    }
    {   // the size filter decides the canonical length; a filter that admits nothing leaves nothing to stream
        RuleIn r = rule(0, 12, 20, 40);
        r.filt_on = 1; r.filt_min = 25; r.filt_max = 30;
        CanonRule c = canon_rule(r);
        CHECK(c.Lc[0] == 25 && c.Lc[1] == 25 && c.kc[1] == 12 && c.D == 5 && c.shift[24 * 2] == -1 && c.shift[31 * 2 + 1] == -1);
        check_against_model(r, c);
        r.filt_max = -1;   // no maximum
        c = canon_rule(r);
        CHECK(c.shift[40 * 2 + 1] == 15 && c.shift[24 * 2 + 1] == -1);
        check_against_model(r, c);
        r.filt_min = 50; r.filt_max = 60;
        c = canon_rule(r);
        CHECK(!c.usable && c.kc[0] == -1 && c.kc[1] == -1);
        check_against_model(r, c);
    }
    {   // variable: missing lengths, a table shorter than the entry table, offsets 0 and 200 (two buckets back)
        std::vector<int32_t> fw(256, -1), rc(256, -1);
        auto set = [&](int L, int off) { fw[(size_t)L] = off; rc[(size_t)L] = L - 1 - off; };
        set(26, 12); set(27, 12); set(28, 13); set(30, 14);
        RuleIn r = rule(3, 0, 20, 40, &fw, &rc);
        CanonRule c = canon_rule(r);
        CHECK(c.usable && c.kc[0] == 12 && c.Lc[0] == 26 && c.kc[1] == 13 && c.Lc[1] == 26 && c.D == 2);
        CHECK(c.shift[29 * 2] == -1 && c.shift[28 * 2 + 0] == 1 && c.shift[30 * 2 + 1] == 2 && c.shift[27 * 2 + 1] == 1);
        check_against_model(r, c);
        set(25, 0); set(250, 200);
        r = rule(3, 0, 20, 255, &fw, &rc);
        c = canon_rule(r);
        CHECK(c.kc[0] == 0 && c.Lc[0] == 25 && c.D == 200 && c.shift[250 * 2] == 200 && canon_buckets_back(c, 7) == 2);
        check_against_model(r, c);
        std::vector<int32_t> fw_short(fw.begin(), fw.begin() + 28), rc_short(rc.begin(), rc.begin() + 28);
        r = rule(3, 0, 20, 40, &fw_short, &rc_short);   // lengths beyond the table are not mapped
        c = canon_rule(r);
        CHECK(c.shift[28 * 2] == -1 && c.shift[27 * 2] == 12 && c.shift[25 * 2] == 0);
        check_against_model(r, c);
    }
    {   // rules the canonical stream does not serve
        CHECK(!canon_rule(rule(2, 0, 20, 40)).usable);
        CHECK(!canon_rule(rule(4, 0, 20, 40)).usable);
    }
    // every rule and filter of a small grid against the model
    for (int kind = 0; kind <= 1; ++kind)
        for (int param = 0; param <= 45; param += 3)
            for (int lo = 0; lo <= 30; lo += 10)
                for (int hi = lo; hi <= 255; hi += 51)
                    for (int f = 0; f < 3; ++f) {
                        RuleIn r = rule(kind, param, lo, hi);
                        if (f) { r.filt_on = 1; r.filt_min = 22; r.filt_max = f == 1 ? 33 : -1; }
                        check_against_model(r, canon_rule(r));
                    }
    {
        unsigned seed = 12345u;
        auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
        for (int round = 0; round < 200; ++round) {
            const int tl = 1 + (int)(rnd() % 300);
            std::vector<int32_t> fw((size_t)tl, -1), rc((size_t)tl, -1);
            for (int L = 1; L < tl; ++L)
                if (rnd() % 3) { const int off = (int)(rnd() % (unsigned)L); fw[(size_t)L] = off; rc[(size_t)L] = L - 1 - off; }
            RuleIn r = rule(3, 0, (int)(rnd() % 40), (int)(rnd() % 256), &fw, &rc);
            if (r.fast_hi < r.fast_lo) r.fast_hi = r.fast_lo;
            if (round & 1) { r.filt_on = 1; r.filt_min = 1 + (int)(rnd() % 50); r.filt_max = (round & 2) ? -1 : r.filt_min + (int)(rnd() % 100); }
            check_against_model(r, canon_rule(r));
        }
    }
    if (failures) { fprintf(stderr, "canon_host: %d failure(s)\n", failures); return 1; }
    printf("canon_host: ok\n");
    return 0;
}
