// plastid_amd/csrc/track_table.h as a stand-alone program (tests/test_track_table_host.py builds it under the address and
// undefined-behaviour sanitizers): the contig table of a count track, without a GPU.  From the file named on the command
// line (written by the test from tests/golden/track_fixture.npz and tests/golden/track_export_fixture.npz): every import
// case through read_track -> births, fold_growth, plan_storage, commit against the fixture's chroms / lengths and against
// the plain serial rule; the construction steps of the export fixture replayed on tables alone; export_ranges against the
// contigs of the golden texts.  Built in: cut_items and check_segments against copies of the two loops they replace, the
// regrouping of nonzero() where the public order differs from the internal one.
#include "track_table.h"

#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <sstream>

using namespace pctrack;

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failed; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static std::string unhex(const std::string &h) {
    std::string out;
    if (h == "-") return out;
    for (size_t k = 0; k + 1 < h.size(); k += 2) out.push_back((char)std::stoi(h.substr(k, 2), nullptr, 16));
    return out;
}

// ---------------------------------------------------------------- import

// the plain serial rule: every row in file order, bear, then grown_length
struct SerialModel {
    int64_t min_chr = 0;
    std::vector<std::string> order;
    std::map<std::string, int64_t> len;
    void row(const std::string &name, int64_t stop) {
        if (!len.count(name)) { order.push_back(name); len[name] = min_chr; }
        len[name] = grown_length(len[name], stop);
    }
};

static void check_public(const ContigTable &tab, const std::vector<std::string> &names, const std::map<std::string, int64_t> &len, const char *what) {
    CHECK(tab.num_public() == (int)names.size(), "%s: %d public contigs of %zu", what, tab.num_public(), names.size());
    for (int i = 0; i < tab.num_public() && i < (int)names.size(); ++i) {
        const int32_t id = tab.public_id(i);
        CHECK(tab.names[(size_t)id] == names[(size_t)i], "%s: contig %d is %s, not %s", what, i, tab.names[(size_t)id].c_str(), names[(size_t)i].c_str());
        CHECK(tab.length[(size_t)id] == len.at(names[(size_t)i]), "%s: %s is %lld long, not %lld", what, names[(size_t)i].c_str(), (long long)tab.length[(size_t)id],
              (long long)len.at(names[(size_t)i]));
        CHECK(tab.public_index(names[(size_t)i]) == i, "%s: public_index(%s)", what, names[(size_t)i].c_str());
    }
    CHECK(tab.public_id(-1) == -1 && tab.public_id(tab.num_public()) == -1 && tab.public_index("no such contig") == -1, "%s: lookups outside", what);
}

// slots keep their extents, the strand's slots reach the furthest end, offsets are the running sum
static void check_plan(const ContigTable &before, const StoragePlan &p, int strand, const std::vector<unsigned long long> &furthest, const char *what) {
    CHECK(p.ext.size() == before.ext.size() && p.off.size() == before.ext.size(), "%s: plan of %zu slots for %zu", what, p.ext.size(), before.ext.size());
    int64_t at = 0;
    bool grows = false;
    for (size_t s = 0; s < p.ext.size() && s < before.ext.size(); ++s) {
        const size_t c = s / (size_t)before.nstrands;
        int64_t want = before.ext[s];
        if ((int)(s % (size_t)before.nstrands) == strand && c < furthest.size()) want = std::max(want, (int64_t)furthest[c]);
        grows = grows || want != before.ext[s];
        CHECK(p.ext[s] == want, "%s: slot %zu gets %lld cells, not %lld", what, s, (long long)p.ext[s], (long long)want);
        CHECK(p.off[s] == at, "%s: slot %zu starts at %lld, not %lld", what, s, (long long)p.off[s], (long long)at);
        at += p.ext[s];
    }
    CHECK(p.total == at && p.grows == grows, "%s: total %lld of %lld, grows %d", what, (long long)p.total, (long long)at, (int)p.grows);
}

// one import on the table alone: what k_track_keys hands back, derived from the host reader's rows
static void import_text(ContigTable &tab, SerialModel &model, const std::string &text, int strand, const char *what) {
    TrackTable rows;
    read_track((const uint8_t *)text.data(), text.size(), rows);
    CHECK(rows.defect == kTrkOk, "%s: the reader refuses line %lld", what, (long long)rows.defect_line);
    // (internal ids follow the first mention, which headers can put in any order: here the reverse of the first yield)
    std::vector<int32_t> id(rows.names.size());
    for (size_t k = rows.names.size(); k-- > 0;) id[k] = tab.id_of(rows.names[k]);
    const std::vector<int64_t> len0 = tab.lengths_before();
    std::vector<uint32_t> first_line(tab.names.size(), kNoLine);
    std::vector<unsigned long long> furthest(tab.names.size(), 0ull);
    std::vector<GrowthLine> growth;
    for (size_t r = 0; r < rows.contig.size(); ++r) {
        const int32_t c = id[(size_t)rows.contig[r]];
        first_line[(size_t)c] = std::min(first_line[(size_t)c], (uint32_t)rows.line[r]);
        if (rows.stop[r] > rows.start[r]) furthest[(size_t)c] = std::max(furthest[(size_t)c], (unsigned long long)rows.stop[r]);
        if (rows.stop[r] >= len0[(size_t)c]) growth.push_back(GrowthLine{rows.stop[r], (uint32_t)rows.line[r], c});
        model.row(rows.names[(size_t)rows.contig[r]], rows.stop[r]);
    }
    std::reverse(growth.begin(), growth.end());   // (the device lists them in any order)
    for (int32_t c : tab.births(first_line)) tab.bear(c);
    tab.fold_growth(growth);
    const ContigTable before = tab;
    const StoragePlan p = tab.plan_storage(strand, furthest);
    check_plan(before, p, strand, furthest, what);
    if (p.grows) { tab.commit(p); CHECK(tab.ncells == p.total && tab.ext == p.ext && tab.cell_off == p.off, "%s: commit", what); }
    check_public(tab, model.order, model.len, what);
}

// ---------------------------------------------------------------- the golden file

struct Replay {
    int64_t min_chr = 0;
    std::map<std::string, ContigTable> tabs;
    std::map<std::string, SerialModel> models;   // (of the tables that only see declares, writes and imports)
};

static std::vector<double> cells_of(std::ifstream &in) {
    std::string line, tok;
    std::getline(in, line);
    std::vector<double> v;
    std::istringstream vs(line);
    while (vs >> tok) v.push_back(std::strtod(tok.c_str(), nullptr));
    return v;
}

static void golden(const char *path) {
    std::ifstream in(path);
    CHECK(in.good(), "cannot read %s", path);
    std::string line, name;
    Replay rp;
    std::vector<std::string> want_names;
    std::map<std::string, int64_t> want_len;
    std::vector<std::vector<double>> cells;   // export: per declared contig and strand
    int ncase = 0, nexport = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string word, target, h;
        ls >> word;
        if (word == "min_chr") ls >> rp.min_chr;
        else if (word == "case") {
            ls >> name;
            rp.tabs.clear(); rp.models.clear(); want_names.clear(); want_len.clear(); cells.clear();
            ++ncase;
        } else if (word == "new") {
            int nstrands = 2;
            ls >> target >> nstrands;
            rp.tabs[target] = ContigTable();
            rp.tabs[target].nstrands = nstrands; rp.tabs[target].min_chr_size = rp.min_chr;
            rp.models[target] = SerialModel();
            rp.models[target].min_chr = rp.min_chr;
        } else if (word == "declare") {
            long long len = 0;
            ls >> target >> h >> len;
            CHECK(rp.tabs[target].declare(unhex(h), len), "%s: %s cannot be declared", name.c_str(), unhex(h).c_str());
            CHECK(!rp.tabs[target].declare(unhex(h), len + 1), "%s: %s is declared twice", name.c_str(), unhex(h).c_str());
            rp.models[target].order.push_back(unhex(h)); rp.models[target].len[unhex(h)] = len;
        } else if (word == "add") {
            int strand = 0;
            ls >> target >> strand >> h;
            import_text(rp.tabs[target], rp.models[target], unhex(h), strand, name.c_str());
        } else if (word == "set") {
            int strand = 0;
            long long nseg = 0;
            ls >> target >> h >> strand >> nseg;
            std::vector<int64_t> start((size_t)nseg), end((size_t)nseg);
            for (long long s = 0; s < nseg; ++s) { long long a, b; ls >> a >> b; start[(size_t)s] = a; end[(size_t)s] = b; }
            ContigTable &tab = rp.tabs[target];
            SerialModel &m = rp.models[target];
            const int32_t id = tab.id_of(unhex(h));
            const int64_t furthest = tab.grow_for_set(id, start.data(), end.data(), nseg);
            int64_t far = 0;
            if (nseg == 0) m.row(unhex(h), -1);   // (born, nothing grows)
            for (long long s = 0; s < nseg; ++s) { m.row(unhex(h), end[(size_t)s]); if (end[(size_t)s] > start[(size_t)s]) far = std::max(far, end[(size_t)s]); }
            CHECK(furthest == far, "%s: furthest end %lld, not %lld", name.c_str(), (long long)furthest, (long long)far);
            if (furthest > 0) {
                const ContigTable before = tab;
                const StoragePlan p = tab.plan_storage(id, strand, furthest);
                std::vector<unsigned long long> fv((size_t)id + 1, 0ull);
                fv[(size_t)id] = (unsigned long long)furthest;
                check_plan(before, p, strand, fv, name.c_str());
                if (p.grows) tab.commit(p);
                CHECK(tab.ext[tab.slot(id, strand)] >= furthest, "%s: the slot does not reach the write", name.c_str());
            }
            check_public(tab, m.order, m.len, name.c_str());
        } else if (word == "arith") {
            std::string left, right;
            int mode_all = 0, nout = 0;
            long long pad = 0;
            ls >> target >> left >> right >> mode_all >> pad >> nout;
            std::vector<int32_t> sa((size_t)nout), sb((size_t)nout);
            for (auto &x : sa) ls >> x;
            for (auto &x : sb) ls >> x;
            ContigTable r;
            r.nstrands = nout; r.min_chr_size = rp.tabs[left].min_chr_size;
            std::vector<OpSlot> slots;
            const ContigTable *b = right == "-" ? nullptr : &rp.tabs[right];
            const int64_t total = ContigTable::combine_layout(rp.tabs[left], b, mode_all != 0, pad, sa.data(), b ? sb.data() : nullptr, r, slots);
            CHECK((int)slots.size() == r.num_public() * nout && total == r.ncells, "%s: %zu operand slots", name.c_str(), slots.size());
            int64_t at = 0;
            for (size_t k = 0; k < slots.size(); ++k) {
                const int64_t len = r.length[(size_t)r.public_id((int)(k / (size_t)nout))] - pad;
                CHECK(slots[k].out0 == at && slots[k].n >= 0 && slots[k].n <= len && (b || slots[k].n == len), "%s: operand slot %zu", name.c_str(), k);
                CHECK(r.cell_off[k] == at && r.ext[k] == slots[k].n, "%s: cells of result slot %zu", name.c_str(), k);
                at += slots[k].n;
            }
            CHECK(at == total, "%s: %lld cells of %lld", name.c_str(), (long long)at, (long long)total);
            rp.tabs[target] = r;
        } else if (word == "chrom") {
            long long len = 0;
            ls >> h >> len;
            want_names.push_back(unhex(h)); want_len[unhex(h)] = len;
        } else if (word == "expect") {
            int nstrands = 0;
            std::string left, right;
            ls >> target >> nstrands >> left >> right;
            CHECK(rp.tabs.count(target) && rp.tabs[target].nstrands == nstrands, "%s: %d strands", name.c_str(), nstrands);
            if (!left.empty()) {
                // the fixture's order comes from a set: the left operand's contigs in its order, then the right one's others in its
                std::vector<std::string> ours;
                const ContigTable &a = rp.tabs[left], &b = rp.tabs[right];
                for (int32_t id : a.order) ours.push_back(a.names[(size_t)id]);
                for (int32_t id : b.order) if (a.public_index(b.names[(size_t)id]) < 0) ours.push_back(b.names[(size_t)id]);
                std::vector<std::string> x = ours, y = want_names;
                std::sort(x.begin(), x.end()); std::sort(y.begin(), y.end());
                CHECK(x == y, "%s: the contigs of the union", name.c_str());
                want_names = ours;
            }
            check_public(rp.tabs[target], want_names, want_len, name.c_str());
        } else if (word == "cells") {
            // (declared with `new` / `declare`; both strands of every contig, in the order of the declares)
            ls >> target;
            ContigTable &tab = rp.tabs[target];
            for (int i = 0; i < tab.num_public(); ++i)
                for (int s = 0; s < tab.nstrands; ++s) {
                    cells.push_back(cells_of(in));
                    const StoragePlan p = tab.plan_storage(tab.public_id(i), s, (int64_t)cells.back().size());
                    if (p.grows) tab.commit(p);
                }
        } else if (word == "want") {
            // the contigs whose header the golden text of (strand, kind) holds, in its order
            int strand = 0, kind = 0;
            ls >> target >> strand >> kind;
            std::vector<std::string> names;
            while (ls >> h) names.push_back(unhex(h));
            const ContigTable &tab = rp.tabs[target];
            const ExportSlots x = tab.export_slots(strand);
            std::vector<SlotStat> stat;
            for (size_t k = 0; k < x.ids.size(); ++k) {
                const std::vector<double> &v = cells[(size_t)tab.rank[(size_t)x.ids[k]] * (size_t)tab.nstrands + (size_t)strand];
                CHECK(x.cells[k].n == (int64_t)v.size() && x.cells[k].cell0 == tab.cell_off[tab.slot(x.ids[k], strand)], "%s: export slot %zu", name.c_str(), k);
                CHECK(k == 0 || tab.names[(size_t)x.ids[k - 1]] < tab.names[(size_t)x.ids[k]], "%s: export slots are not sorted", name.c_str());
                SlotStat s{0.0, ~0ull, 0ull};
                for (size_t i = 0; i < v.size(); ++i) {
                    s.sum = s.sum + v[i];
                    if (v[i] != 0.0) { if (s.first == ~0ull) s.first = i; s.last1 = i + 1; }
                }
                stat.push_back(s);
            }
            const ExportRanges xr = tab.export_ranges(kind, x, stat);
            CHECK(xr.ranges.size() == (names.empty() ? 0 : names.size() + 1), "%s strand %d kind %d: %zu ranges for %zu contigs", name.c_str(), strand, kind,
                  xr.ranges.size(), names.size());
            int64_t e0 = 0;
            for (size_t k = 0; k < names.size() && k + 1 < xr.ranges.size(); ++k) {
                const ExRange &r = xr.ranges[k];
                const std::string got((const char *)xr.names.data() + r.name_off, (size_t)r.name_len);
                const int32_t id = tab.ids.at(names[k]);
                const std::vector<double> &v = cells[(size_t)tab.rank[(size_t)id] * (size_t)tab.nstrands + (size_t)strand];
                CHECK(got == names[k], "%s strand %d kind %d: contig %zu is %s, not %s", name.c_str(), strand, kind, k, got.c_str(), names[k].c_str());
                CHECK(r.e0 == e0 && r.run_base == 0, "%s: e0 of range %zu", name.c_str(), k);
                CHECK(r.cell0 == tab.cell_off[tab.slot(id, strand)] + r.pos0 && r.pos0 >= 0 && r.pos0 + r.n <= (int64_t)v.size(), "%s: cells of range %zu", name.c_str(), k);
                if (kind == 1) CHECK(r.pos0 == 0 && r.n == (int64_t)v.size(), "%s: variableStep range %zu", name.c_str(), k);
                else CHECK(r.n > 0 && v[(size_t)r.pos0] != 0.0 && v[(size_t)(r.pos0 + r.n - 1)] != 0.0, "%s: bedGraph range %zu", name.c_str(), k);
                e0 += r.n;
            }
            if (!xr.ranges.empty()) CHECK(xr.ranges.back().e0 == e0 && xr.ranges.back().n == 0 && xr.cells == e0, "%s: the sentinel", name.c_str());
            ++nexport;
        }
    }
    CHECK(ncase > 0 && nexport > 0, "no golden case in %s", path);
    printf("golden: %d cases, %d exports\n", ncase, nexport);
}

// ---------------------------------------------------------------- items

struct Cut { std::string error; std::vector<pcdense::Item> items; };

// the loop of pc_track_gather before it moved into the table (order / nstrands / cell_off / ext: the track's)
static Cut model_gather(const ContigTable &t, int64_t nseg, const int32_t *contig, const int32_t *strand_slot, const int64_t *start, const int64_t *end,
                        const int64_t *out_off, const int8_t *out_step, int64_t out_elems) {
    Cut c;
    char msg[160];
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t len = end[s] - start[s];
        if (len <= 0) continue;
        if (out_step[s] != 1 && out_step[s] != -1) { snprintf(msg, sizeof(msg), "pc_track_gather: out_step of segment %lld is not +1 / -1", (long long)s); c.error = msg; return c; }
        const int64_t first = out_off[s], last = out_off[s] + (int64_t)out_step[s] * (len - 1);
        if (first < 0 || first >= out_elems || last < 0 || last >= out_elems) {
            snprintf(msg, sizeof(msg), "pc_track_gather: segment %lld writes outside the output", (long long)s); c.error = msg; return c;
        }
        pcdense::SegIn in;
        in.out_off = out_off[s]; in.len = len; in.clip_lo = 0; in.clip_hi = len; in.start = start[s]; in.step = out_step[s];
        in.known = contig[s] >= 0 && contig[s] < (int32_t)t.order.size() && strand_slot[s] >= 0 && strand_slot[s] < t.nstrands;
        if (in.known) {
            const size_t slot = (size_t)t.order[(size_t)contig[s]] * (size_t)t.nstrands + (size_t)strand_slot[s];
            in.cell_base = t.cell_off[slot];
            in.ext = t.ext[slot];
        }
        const int64_t k_end = pcdense::items_of(len);
        for (int64_t k = 0; k < k_end; ++k) c.items.push_back(pcdense::cut_item(in, k));
    }
    return c;
}

// the two loops of pc_track_set: its checks, then (the storage grown in between) its items
static std::string model_set_checks(int64_t nseg, const int64_t *start, const int64_t *end, const int64_t *val_off, const int8_t *val_step, bool values, int64_t nvalues) {
    char msg[160];
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t len = end[s] - start[s];
        if (start[s] < 0 || len < 0 || end[s] > kMaxCoord) { snprintf(msg, sizeof(msg), "pc_track_set: segment %lld lies outside [0, 2^40]", (long long)s); return msg; }
        if (values && len > 0) {
            if (val_step[s] != 1 && val_step[s] != -1) { snprintf(msg, sizeof(msg), "pc_track_set: val_step of segment %lld is not +1 / -1", (long long)s); return msg; }
            const int64_t a = val_off[s], b = val_off[s] + (int64_t)val_step[s] * (len - 1);
            if (a < 0 || a >= nvalues || b < 0 || b >= nvalues) { snprintf(msg, sizeof(msg), "pc_track_set: segment %lld reads outside the vector", (long long)s); return msg; }
        }
    }
    return std::string();
}
static std::vector<pcdense::Item> model_set_items(const ContigTable &t, size_t slot, int64_t nseg, const int64_t *start, const int64_t *end, const int64_t *val_off,
                                                  const int8_t *val_step, bool values) {
    std::vector<pcdense::Item> items;
    for (int64_t s = 0; s < nseg; ++s) {
        pcdense::SegIn in;
        in.len = end[s] - start[s];
        if (in.len <= 0) continue;
        in.out_off = values ? val_off[s] : 0; in.step = values ? val_step[s] : 1;
        in.clip_lo = 0; in.clip_hi = in.len; in.start = start[s]; in.known = true;
        in.cell_base = t.cell_off[slot]; in.ext = t.ext[slot];
        const int64_t k_end = pcdense::items_of(in.len);
        for (int64_t k = 0; k < k_end; ++k) items.push_back(pcdense::cut_item(in, k));
    }
    return items;
}

static bool same_items(const std::vector<pcdense::Item> &a, const std::vector<pcdense::Item> &b) {
    if (a.size() != b.size()) return false;
    for (size_t k = 0; k < a.size(); ++k)
        if (a[k].out_off != b[k].out_off || a[k].cell0 != b[k].cell0 || a[k].len != b[k].len || a[k].step != b[k].step || a[k].lo != b[k].lo || a[k].hi != b[k].hi) return false;
    return true;
}

static void check_gather(const ContigTable &t, const char *what, std::vector<int32_t> contig, std::vector<int32_t> strand, std::vector<int64_t> start,
                         std::vector<int64_t> end, std::vector<int64_t> off, std::vector<int8_t> step, int64_t elems, const char *error) {
    const int64_t nseg = (int64_t)contig.size();
    const Cut want = model_gather(t, nseg, contig.data(), strand.data(), start.data(), end.data(), off.data(), step.data(), elems);
    const std::string got = check_segments(kGatherWords, nseg, start.data(), end.data(), off.data(), step.data(), elems, false);
    CHECK(got == want.error && got == error, "%s: \"%s\" for \"%s\"", what, got.c_str(), want.error.c_str());
    if (!got.empty()) return;
    std::vector<pcdense::Item> items;
    t.cut_items(nseg, start.data(), end.data(), off.data(), step.data(), [&](int64_t s) { return t.public_slot(contig[(size_t)s], strand[(size_t)s]); }, items);
    CHECK(same_items(items, want.items) && !(nseg == 1 && end[0] > start[0] && items.empty()), "%s: %zu items for %zu", what, items.size(), want.items.size());
}

static void check_set(const ContigTable &t, const char *what, std::vector<int64_t> start, std::vector<int64_t> end, std::vector<int64_t> off, std::vector<int8_t> step,
                      bool values, int64_t nvalues, const char *error) {
    const int64_t nseg = (int64_t)start.size();
    const std::string want = model_set_checks(nseg, start.data(), end.data(), off.data(), step.data(), values, nvalues);
    const std::string got = check_segments(kSetWords, nseg, start.data(), end.data(), values ? off.data() : nullptr, step.data(), nvalues, true);
    CHECK(got == want && got == error, "%s: \"%s\" for \"%s\"", what, got.c_str(), want.c_str());
    if (!got.empty()) return;
    const int64_t slot = (int64_t)t.slot(t.public_id(1), 1);
    std::vector<pcdense::Item> items;
    t.cut_items(nseg, start.data(), end.data(), values ? off.data() : nullptr, step.data(), [slot](int64_t) { return slot; }, items);
    CHECK(same_items(items, model_set_items(t, (size_t)slot, nseg, start.data(), end.data(), off.data(), step.data(), values)), "%s: %zu items", what, items.size());
}

static void items() {
    const int64_t L = pcdense::kItemLen;
    ContigTable t;
    t.min_chr_size = 100;
    t.id_of("mentioned");                      // (an internal id in front of the public contigs)
    CHECK(t.declare("a", 3 * L) && t.declare("b", 50), "declare");
    t.commit(t.plan_storage(t.ids.at("a"), 0, 2 * L + 7));
    t.commit(t.plan_storage(t.ids.at("b"), 1, 40));
    t.commit(t.plan_storage(t.ids.at("a"), 1, 5));
    check_gather(t, "length 1", {0}, {0}, {9}, {10}, {0}, {1}, 1, "");
    check_gather(t, "exactly one item", {0}, {0}, {3}, {3 + L}, {0}, {1}, L, "");
    check_gather(t, "one item plus one", {0}, {0}, {3}, {4 + L}, {0}, {1}, L + 1, "");
    check_gather(t, "step -1", {0, 1}, {0, 1}, {0, 10}, {L + 5, 30}, {L + 4, L + 24}, {-1, -1}, L + 25, "");
    check_gather(t, "past the extent", {0, 1, 0}, {0, 1, 1}, {2 * L, 35, 5}, {2 * L + 30, 60, 9}, {0, 30, 55}, {1, 1, 1}, 60, "");
    check_gather(t, "unknown contig", {-1, 2, 0, 0}, {0, 0, 2, -1}, {0, 0, 0, 0}, {4, 4, 4, 4}, {0, 4, 8, 12}, {1, 1, 1, 1}, 16, "");
    check_gather(t, "empty segments", {0, 0}, {0, 0}, {5, 9}, {5, 2}, {99, 99}, {7, 7}, 4, "");
    check_gather(t, "a wide step", {0, 0}, {0, 0}, {0, 0}, {4, 4}, {0, 4}, {1, 2}, 8, "pc_track_gather: out_step of segment 1 is not +1 / -1");
    check_gather(t, "beyond the output", {0}, {0}, {0}, {4}, {1}, {1}, 4, "pc_track_gather: segment 0 writes outside the output");
    check_gather(t, "below the output", {0, 0}, {0, 0}, {0, 0}, {4, 4}, {0, 2}, {1, -1}, 8, "pc_track_gather: segment 1 writes outside the output");
    check_set(t, "set: length 1", {39}, {40}, {0}, {1}, true, 1, "");
    check_set(t, "set: items", {0, 0}, {L, L + 1}, {0, 2 * L}, {1, -1}, true, 2 * L + 1, "");
    check_set(t, "set: a scalar", {0, 7}, {L + 1, 7}, {0, 0}, {0, 0}, false, 0, "");
    check_set(t, "set: past the extent", {30}, {45}, {0}, {1}, true, 15, "");
    check_set(t, "set: below 0", {-1}, {4}, {0}, {1}, true, 5, "pc_track_set: segment 0 lies outside [0, 2^40]");
    check_set(t, "set: backwards", {0, 9}, {4, 8}, {0, 4}, {1, 1}, true, 5, "pc_track_set: segment 1 lies outside [0, 2^40]");
    check_set(t, "set: too far", {0}, {kMaxCoord + 1}, {0}, {1}, false, 0, "pc_track_set: segment 0 lies outside [0, 2^40]");
    check_set(t, "set: a wide step", {0}, {4}, {0}, {3}, true, 4, "pc_track_set: val_step of segment 0 is not +1 / -1");
    check_set(t, "set: a short vector", {0, 4}, {4, 8}, {0, 4}, {1, 1}, true, 7, "pc_track_set: segment 1 reads outside the vector");
}

// ---------------------------------------------------------------- nonzero

static void nonzero() {
    // "late" is mentioned first (a header) and yields after "early": internal order late, early; public order early, late
    ContigTable t;
    const int32_t late = t.id_of("late"), early = t.id_of("early");
    t.bear(early); t.bear(late);
    CHECK(t.public_index("early") == 0 && t.public_index("late") == 1 && t.public_id(0) == early, "public order");
    t.commit(t.plan_storage(late, 0, 4));
    t.commit(t.plan_storage(early, 0, 3));
    t.commit(t.plan_storage(early, 1, 2));
    const std::vector<double> cells = {0, 5, 0, 6, /* early + */ 7, 0, 8, /* early - */ 0, 9};
    CHECK(t.ncells == (int64_t)cells.size() && t.cell_off[t.slot(early, 0)] == 4 && t.cell_off[t.slot(early, 1)] == 7, "layout");
    NzShares z = t.nonzero_slots();
    CHECK(z.live == std::vector<int>({(int)t.slot(late, 0), (int)t.slot(early, 0), (int)t.slot(early, 1)}) && z.at == std::vector<int64_t>({0, 4, 7, 9}), "live slots");
    // what the kernels give: non-zero cells in front of every at[], the positions on their slots in the order of the cells
    std::vector<int64_t> picked, all;
    for (int64_t at : z.at) {
        int64_t n = 0;
        for (int64_t i = 0; i < at; ++i) n += cells[(size_t)i] != 0.0;
        picked.push_back(n);
    }
    for (size_t j = 0; j + 1 < z.at.size(); ++j)
        for (int64_t i = z.at[j]; i < z.at[j + 1]; ++i) if (cells[(size_t)i] != 0.0) all.push_back(i - z.at[j]);
    std::vector<int64_t> counts(4, -1), out(all.size() + 1, -1);
    t.nonzero_counts(z, picked, counts.data());
    CHECK(counts == std::vector<int64_t>({2, 1, 2, 0}), "counts %lld %lld %lld %lld", (long long)counts[0], (long long)counts[1], (long long)counts[2], (long long)counts[3]);
    t.nonzero_regroup(z, all.data(), out.data());
    CHECK(out == std::vector<int64_t>({0, 2, 1, 1, 3, -1}), "regrouped: %lld %lld %lld %lld %lld", (long long)out[0], (long long)out[1], (long long)out[2], (long long)out[3],
          (long long)out[4]);
}

int main(int argc, char **argv) {
    items();
    nonzero();
    if (argc > 1) golden(argv[1]);
    if (g_failed) { printf("track_table_host: %d checks failed\n", g_failed); return 1; }
    printf("track_table_host: ok\n");
    return 0;
}
