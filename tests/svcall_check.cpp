// The structural-variant calling rule of flx_svcall.hpp (the one implementation that flx_svcall_host runs) on random records and
// clusters against a definition that walks every span of every cluster on its own: no sort, no
// window, no max_span. The words and the clusters live in arrays of exactly the needed size, so that a step outside them is an
// AddressSanitizer report. Then the window bound at its edges (the record that sets max_span on another sequence, hi' below max_span,
// spans that end at hi' and at hi' - 1 and start at lo' and at lo' + 1), the genotype at the defaults and the refusals of the options
// and of the clusters. Stand-alone, built with ASan + UBSan by tests/test_svcall_host.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../floxer_amd/csrc/flx_svcall.hpp"

namespace flx {
static std::string last_error;
void set_error(const std::string& m) { last_error = m; }
}

struct Span { uint32_t ref, rs, re; };

static flx_sv_cluster cluster(uint32_t type, uint32_t support, int32_t ref, uint32_t pmin, uint32_t pmax, uint32_t qmin, uint32_t qmed, uint32_t qmax) {
    flx_sv_cluster c{};
    c.type = type; c.support = support; c.ref_a = ref; c.ref_b = ref; c.pos_a_min = pmin; c.pos_a_max = pmax; c.q_min = qmin; c.q_median = qmed; c.q_max = qmax;
    return c;
}

// the definition: the count of one cluster over all spans
static uint32_t count_by_walk(std::vector<Span> const& spans, flx_sv_cluster const& c, uint64_t n_r, uint32_t flank) {
    uint64_t const lo = c.pos_a_min, hi = c.type == flx::SV_DEL ? (uint64_t)c.pos_a_max + c.q_max : (uint64_t)c.pos_a_max + 1;
    uint64_t const lo2 = lo >= flank ? lo - flank : 0, hi2 = std::min<uint64_t>(hi + flank, n_r);
    uint32_t n = 0;
    for (auto const& s : spans) n += s.ref == (uint32_t)c.ref_a && s.rs <= lo2 && s.re >= hi2;
    return n;
}

static bool rows_by_rule(std::vector<uint64_t> const& lens, std::vector<Span> const& spans, std::vector<flx_sv_cluster> const& clusters, flx_svcall_options const& o,
                         std::vector<flx_svcall_row>& rows) {
    std::vector<uint64_t> starts;
    if (!flx::coverage_lengths_valid(lens.data(), (uint32_t)lens.size(), "check", starts)) return false;
    uint64_t n_rows = 0;
    if (!flx::svcall_clusters_valid(starts, clusters.data(), clusters.size(), "check", n_rows)) return false;
    std::vector<flx::SortKey> keys;
    for (auto const& s : spans) keys.push_back(flx::svcall_span_key(s.ref, s.rs, s.re));
    flx::svcall_finish_host(starts, keys, clusters.data(), clusters.size(), flx::svcall_model(o), rows);
    return rows.size() == n_rows;
}

static int fail(const char* what, int c) { printf("case %d: %s (%s)\n", c, what, flx::last_error.c_str()); return 1; }

int main() {
    std::mt19937_64 rng(20261021);
    static const uint32_t ops[5] = {7, 8, 1, 2, 4};
    static const uint32_t flags[7] = {0, 16, 256, 272, 2048, 2064, 4};
    uint64_t n_counted = 0, n_rows = 0, n_spanned = 0, n_clamped_lo = 0, n_clamped_hi = 0, n_pass = 0, n_gt[3] = {0, 0, 0}, n_far_max = 0, n_low_hi = 0;
    int const n_cases = 1500;
    for (int c = 0; c < n_cases; ++c) {
        uint32_t const n_refs = 1 + (uint32_t)(rng() % 3);
        std::vector<uint64_t> lens(n_refs), starts;
        for (auto& l : lens) l = 2 + rng() % (c % 3 ? 400 : 40);
        if (!flx::coverage_lengths_valid(lens.data(), n_refs, "check", starts)) return fail("valid lengths were refused", c);
        flx_svcall_options o{};
        o.count_secondary = rng() % 2; o.min_mapq = rng() % 3 ? 0 : 1 + (uint32_t)(rng() % 60);
        o.flank = rng() % 3 ? (uint32_t)(rng() % 30) : 0; o.min_depth = (uint32_t)(rng() % 6); o.min_qual = rng() % 2 ? 0 : (uint32_t)(rng() % 5000);
        if (!flx::svcall_options_valid(&o)) return fail("valid options were refused", c);
        flx::SvcallModel const m = flx::svcall_model(o);
        if (m.flank != (o.flank ? o.flank : 50u) || m.v.min_depth != (o.min_depth ? o.min_depth : 4u) || m.v.min_qual != (o.min_qual ? o.min_qual : 2000u) || m.v.m != 36u ||
            m.v.x != 1574u || m.v.h != 325u || m.v.prior_het != 3000u || m.v.prior_hom != 3301u)
            return fail("the model's defaults differ", c);
        // records: a few long ones among many short, so that max_span comes from one sequence and bounds the windows of the others
        std::vector<flx_record> recs;
        std::vector<uint32_t> words;
        std::vector<Span> want;
        int const n_rec = (int)(rng() % 60);
        for (int r = 0; r < n_rec; ++r) {
            flx_record rec{};
            rec.flag = flags[rng() % 7];
            rec.reference_id = (int32_t)(rng() % n_refs);
            rec.reserved = (uint32_t)(rng() % 3 == 0 ? 0 : rng() % 61);
            uint64_t const len = lens[(size_t)rec.reference_id];
            uint32_t const T = 1 + (uint32_t)(rng() % 7);
            uint64_t const budget = rng() % 8 == 0 ? len : std::min<uint64_t>(len, 1 + rng() % 30);
            std::vector<uint32_t> w;
            uint64_t span = 0;
            for (uint32_t k = 0; k < T; ++k) {
                uint32_t const op = ops[rng() % 5];
                uint32_t l = 1 + (uint32_t)(rng() % 12);
                if (flx::svcall_op_consumes(op)) {
                    if (span >= budget) continue;
                    l = (uint32_t)std::min<uint64_t>(l, budget - span);
                    span += l;
                }
                w.push_back(l << 4 | op);
            }
            if (span == 0) { w.push_back(1u << 4 | 7u); span = 1; }
            rec.position = (int32_t)(rng() % (len - span + 1));
            if (rec.flag & 4u) { rec.reference_id = -1; rec.position = 0; w.clear(); }
            rec.cigar_offset = words.size();
            rec.cigar_length = (uint32_t)w.size();
            words.insert(words.end(), w.begin(), w.end());
            recs.push_back(rec);
            bool const counts = !(rec.flag & 4u) && (!(rec.flag & 256u) || o.count_secondary) && (o.min_mapq == 0 || rec.reserved >= o.min_mapq);
            if (counts) want.push_back(Span{(uint32_t)rec.reference_id, (uint32_t)rec.position, (uint32_t)(rec.position + span)});
        }
        std::vector<uint32_t> exact(words);                                // (exactly the needed size)
        std::vector<flx::SvcallJob> jobs;
        if (!flx::svcall_plan(starts, o, recs.data(), recs.size(), exact.data(), exact.size(), "check", jobs)) return fail("valid records were refused", c);
        if (jobs.size() != want.size()) return fail("another number of counted records", c);
        for (size_t i = 0; i < jobs.size(); ++i) {
            flx::SortKey const k = flx::svcall_job_key(jobs[i]);
            if (flx::svcall_span_ref(k) != want[i].ref || flx::svcall_span_rs(k) != want[i].rs || flx::svcall_span_re(k) != want[i].re) return fail("a span differs", c);
        }
        n_counted += want.size();
        // clusters of all types, some at position 0 and some at their sequence's end
        std::vector<flx_sv_cluster> clusters;
        int const n_cl = (int)(rng() % 25);
        for (int k = 0; k < n_cl; ++k) {
            uint32_t const type = (uint32_t)(rng() % 3);
            int32_t const ref = (int32_t)(rng() % n_refs);
            uint64_t const len = lens[(size_t)ref];
            uint32_t const qmin = 1 + (uint32_t)(rng() % 20), qmed = qmin + (uint32_t)(rng() % 5), qmax = qmed + (uint32_t)(rng() % 5);
            if (type == flx::SV_BND) { flx_sv_cluster b = cluster(2, 3, ref, 0, (uint32_t)(len - 1), 9, 2, 1); b.ref_b = (int32_t)(rng() % n_refs); b.side_a = 1; clusters.push_back(b); continue; }
            if (type == flx::SV_DEL && qmax > len) continue;
            uint64_t const room = type == flx::SV_DEL ? len - qmax : len - 1;
            uint32_t const pmax = rng() % 5 == 0 ? (uint32_t)room : (uint32_t)(rng() % (room + 1));
            uint32_t const pmin = rng() % 5 == 0 ? 0u : pmax - (uint32_t)(rng() % std::min<uint64_t>(pmax + 1, 8));
            clusters.push_back(cluster(type, (uint32_t)(rng() % 12), ref, pmin, pmax, qmin, qmed, qmax));
        }
        std::vector<flx_sv_cluster> exact_clusters(clusters);
        std::vector<flx_svcall_row> rows;
        if (!rows_by_rule(lens, want, exact_clusters, o, rows)) return fail("valid clusters were refused or rows are missing", c);
        uint32_t max_span = 0, max_ref = 0;
        for (auto const& s : want) if (s.re - s.rs > max_span) { max_span = s.re - s.rs; max_ref = s.ref; }
        size_t at = 0;
        for (size_t i = 0; i < clusters.size(); ++i) {
            flx_sv_cluster const& cl = clusters[i];
            if (cl.type == flx::SV_BND) continue;
            if (at >= rows.size()) return fail("a row is missing", c);
            flx_svcall_row const& r = rows[at++];
            uint64_t const len = lens[(size_t)cl.ref_a];
            uint32_t const span_n = count_by_walk(want, cl, len, m.flank);
            uint32_t const alt_n = cl.support, ref_n = span_n > alt_n ? span_n - alt_n : 0;
            flx::VariantGenotype const g = flx::variants_genotype(ref_n, alt_n, 0, m.v);
            uint32_t const pass = g.gt != 0 && (uint64_t)ref_n + alt_n >= m.v.min_depth && g.qual >= m.v.min_qual;
            if (r.cluster != i || r.type != cl.type || r.ref != cl.ref_a || r.pos_a_min != cl.pos_a_min || r.pos_a_max != cl.pos_a_max || r.q_min != cl.q_min ||
                r.q_median != cl.q_median || r.q_max != cl.q_max)
                return fail("a row does not repeat its cluster", c);
            if (r.span_n != span_n || r.alt_n != alt_n || r.ref_n != ref_n) { printf("span_n %u want %u\n", r.span_n, span_n); return fail("a count differs from the walk over every span", c); }
            if (r.gt != g.gt || r.gq != g.gq || r.qual != g.qual || r.pl[0] != g.pl[0] || r.pl[1] != g.pl[1] || r.pl[2] != g.pl[2] || r.pass != pass) return fail("a genotype differs", c);
            uint32_t lo2, hi2;
            flx::svcall_bounds(cl, (uint32_t)len, m.flank, lo2, hi2);
            n_rows++; n_spanned += span_n > 0; n_pass += pass; n_gt[g.gt]++;
            n_clamped_lo += cl.pos_a_min < m.flank; n_clamped_hi += hi2 == len;
            n_far_max += span_n > 0 && max_ref != (uint32_t)cl.ref_a; n_low_hi += span_n > 0 && hi2 < max_span;
        }
        if (at != rows.size()) return fail("rows without a cluster", c);
    }
    if (n_spanned < 200 || n_clamped_lo < 200 || n_clamped_hi < 200 || n_far_max < 50 || n_low_hi < 50 || !n_gt[0] || !n_gt[1] || !n_gt[2] || n_pass < 20) {
        printf("the cases miss a kind: rows %llu spanned %llu clamped %llu/%llu max_span elsewhere %llu hi' below max_span %llu gt %llu/%llu/%llu pass %llu\n", (unsigned long long)n_rows,
               (unsigned long long)n_spanned, (unsigned long long)n_clamped_lo, (unsigned long long)n_clamped_hi, (unsigned long long)n_far_max, (unsigned long long)n_low_hi,
               (unsigned long long)n_gt[0], (unsigned long long)n_gt[1], (unsigned long long)n_gt[2], (unsigned long long)n_pass);
        return 1;
    }

    // ---- the window bound at its edges: flank 10, a DEL at [100, 120) on sequence 1: lo' = 90, hi' = 130
    {
        flx_svcall_options o{};
        o.flank = 10;
        std::vector<uint64_t> const lens = {5000, 1000, 1000};
        std::vector<flx_sv_cluster> const cl = {cluster(0, 1, 1, 100, 100, 20, 20, 20)};
        struct Case { std::vector<Span> spans; uint32_t want; const char* what; };
        std::vector<Case> const cases = {
            {{{1, 90, 130}}, 1, "starts at lo' and ends at hi'"},
            {{{1, 91, 130}}, 0, "starts at lo' + 1"},
            {{{1, 90, 129}}, 0, "ends at hi' - 1"},
            {{{1, 89, 131}, {1, 90, 130}, {1, 91, 131}, {1, 0, 129}}, 2, "neighbours of the bounds"},
            {{{0, 0, 5000}, {1, 90, 130}, {1, 0, 1000}}, 2, "max_span set on another sequence, above hi'"},
            {{{0, 90, 130}, {2, 90, 130}}, 0, "the same rs and re on the neighbour sequences only"},
            {{{0, 90, 130}, {1, 90, 130}, {2, 90, 130}, {1, 90, 130}}, 2, "the reference id separates equal spans"},
            {{{1, 0, 40}, {1, 90, 130}}, 1, "max_span exactly hi' - lo'"},
            {{{1, 0, 39}, {1, 95, 134}}, 0, "no span long enough: an empty window"},
            {{}, 0, "no spans"},
        };
        for (size_t k = 0; k < cases.size(); ++k) {
            std::vector<flx_svcall_row> rows;
            if (!rows_by_rule(lens, cases[k].spans, cl, o, rows) || rows.size() != 1 || rows[0].span_n != cases[k].want || rows[0].span_n != count_by_walk(cases[k].spans, cl[0], 1000, 10)) {
                printf("window case '%s': span_n %u, want %u\n", cases[k].what, rows.empty() ? 0u : rows[0].span_n, cases[k].want);
                return 1;
            }
        }
        // lo' clamps at 0 and hi' at the sequence's end
        std::vector<flx_sv_cluster> const ends = {cluster(0, 0, 1, 5, 5, 10, 10, 10), cluster(1, 0, 1, 999, 999, 60, 60, 60), cluster(0, 0, 1, 980, 980, 20, 20, 20)};
        std::vector<Span> const spans = {{1, 0, 25}, {1, 1, 25}, {1, 0, 24}, {1, 989, 1000}, {1, 990, 1000}, {1, 970, 1000}, {1, 970, 999}};
        std::vector<flx_svcall_row> rows;
        if (!rows_by_rule(lens, spans, ends, o, rows) || rows.size() != 3 || rows[0].span_n != 1 || rows[1].span_n != 2 || rows[2].span_n != 1) { printf("the clamps differ\n"); return 1; }
    }
    // ---- the genotype at the defaults
    {
        flx_svcall_options o{};
        std::vector<uint64_t> const lens = {1000};
        auto one = [&](uint32_t carriers, uint32_t others, flx_svcall_row& r) {
            std::vector<Span> spans((size_t)carriers + others, Span{0, 0, 1000});
            std::vector<flx_svcall_row> rows;
            if (!rows_by_rule(lens, spans, {cluster(0, carriers, 0, 500, 500, 80, 80, 80)}, o, rows) || rows.size() != 1) return false;
            r = rows[0];
            return true;
        };
        flx_svcall_row r;
        if (!one(6, 6, r) || r.gt != 1 || r.qual != 2760 || !r.pass || r.ref_n != 6 || r.alt_n != 6) { printf("six and six: gt %u qual %u pass %u\n", r.gt, r.qual, r.pass); return 1; }
        if (!one(5, 5, r) || r.gt != 1 || r.qual != 1800 || r.pass) { printf("five and five: gt %u qual %u pass %u\n", r.gt, r.qual, r.pass); return 1; }
        if (!one(5, 0, r) || r.gt != 2 || r.qual != 4389 || !r.pass || r.ref_n != 0) { printf("five alone: gt %u qual %u pass %u\n", r.gt, r.qual, r.pass); return 1; }
        std::vector<flx_svcall_row> rows;                                  // ref_n clamps at 0 when alt_n > span_n
        if (!rows_by_rule(lens, {{0, 0, 1000}, {0, 0, 1000}}, {cluster(1, 7, 0, 500, 500, 60, 60, 60)}, o, rows) || rows[0].span_n != 2 || rows[0].ref_n != 0 || rows[0].alt_n != 7) { printf("the clamp of ref_n differs\n"); return 1; }
    }
    // ---- refusals: options, then clusters
    {
        auto refused = [](flx_svcall_options o, const char* part) { return !flx::svcall_options_valid(&o) && flx::last_error.find(part) != std::string::npos; };
        flx_svcall_options o{};
        if (!flx::svcall_options_valid(nullptr) || !flx::svcall_options_valid(&o)) { printf("the default options were refused\n"); return 1; }
        o = {}; o.reserved[1] = 1; if (!refused(o, "reserved")) { printf("reserved was taken\n"); return 1; }
        o = {}; o.flank = (1u << 20) + 1; if (!refused(o, "flank")) { printf("a flank above 2^20 was taken\n"); return 1; }
        o = {}; o.flank = 1u << 20; if (!flx::svcall_options_valid(&o)) { printf("a flank of 2^20 was refused\n"); return 1; }
        o = {}; o.cost_mismatch = (1u << 20) + 1; if (!refused(o, "2^20")) { printf("a cost above 2^20 was taken\n"); return 1; }
        o = {}; o.cost_het = 36; if (!refused(o, "degenerate")) { printf("cost_het == cost_match was taken\n"); return 1; }
        o = {}; o.cost_het = 1574; if (!refused(o, "degenerate")) { printf("cost_het == cost_mismatch was taken\n"); return 1; }
        std::vector<uint64_t> const lens = {100, 50};
        std::vector<uint64_t> starts;
        flx::coverage_lengths_valid(lens.data(), 2, "check", starts);
        auto bad = [&](flx_sv_cluster c, const char* part) {
            std::vector<flx_sv_cluster> two = {cluster(0, 1, 0, 10, 10, 5, 5, 5), c};
            uint64_t n = 0;
            return !flx::svcall_clusters_valid(starts, two.data(), 2, "check", n) && flx::last_error.find("cluster 1") != std::string::npos && flx::last_error.find(part) != std::string::npos;
        };
        flx_sv_cluster c;
        c = cluster(3, 1, 0, 1, 1, 1, 1, 1); if (!bad(c, "type above 2")) { printf("a type of 3 was taken\n"); return 1; }
        c = cluster(0, 1, 2, 1, 1, 1, 1, 1); if (!bad(c, "outside the lengths")) { printf("a reference id of 2 was taken\n"); return 1; }
        c = cluster(2, 1, 0, 1, 1, 1, 1, 1); c.ref_b = -1; if (!bad(c, "outside the lengths")) { printf("a ref_b of -1 was taken\n"); return 1; }
        c = cluster(1, 1, 0, 1, 1, 1, 1, 1); c.ref_b = 1; if (!bad(c, "outside the lengths")) { printf("an INS on two sequences was taken\n"); return 1; }
        c = cluster(0, 1, 0, 2, 1, 1, 1, 1); if (!bad(c, "pos_a_min above pos_a_max")) { printf("pos_a_min > pos_a_max was taken\n"); return 1; }
        c = cluster(0, 1, 0, 1, 1, 2, 1, 3); if (!bad(c, "q_min <= q_median <= q_max")) { printf("q_min > q_median was taken\n"); return 1; }
        c = cluster(1, 1, 0, 1, 1, 1, 3, 2); if (!bad(c, "q_min <= q_median <= q_max")) { printf("q_median > q_max was taken\n"); return 1; }
        c = cluster(0, 1, 1, 41, 41, 10, 10, 10); if (!bad(c, "ends behind its sequence")) { printf("a DEL past its sequence was taken\n"); return 1; }
        c = cluster(1, 1, 1, 50, 50, 10, 10, 10); if (!bad(c, "at or behind its sequence's end")) { printf("an INS at its sequence's end was taken\n"); return 1; }
        c = cluster(0, 1, 0, 1, 1, 1, 1, 1); c.reserved = 1; if (!bad(c, "reserved")) { printf("a reserved field was taken\n"); return 1; }
        uint64_t n = 0;                                                    // the last valid ones; a BND's q fields are not judged
        std::vector<flx_sv_cluster> ok = {cluster(0, 1, 1, 40, 40, 10, 10, 10), cluster(1, 1, 1, 49, 49, 10, 10, 10), cluster(2, 1, 0, 1, 1, 9, 2, 1)};
        if (!flx::svcall_clusters_valid(starts, ok.data(), 3, "check", n) || n != 2) { printf("valid clusters at the ends were refused: %s\n", flx::last_error.c_str()); return 1; }
    }
    printf("ok %d cases, %llu counted records, %llu rows (%llu spanned, %llu passing)\n", n_cases, (unsigned long long)n_counted, (unsigned long long)n_rows, (unsigned long long)n_spanned,
           (unsigned long long)n_pass);
    return 0;
}
