// The HIP-free half of the svcaller object (floxer_amd/csrc/flx_svcaller.hpp: the host table with its add, absorb, finish and copies,
// and the capacity and stretch judgements that the device path shares) on random records, against a walk over every span. The tables are
// fed in one add, in pieces cut anywhere and through an absorb; rows and spans are copied into heap buffers of exactly the needed size,
// so that a byte written past a stated capacity is an AddressSanitizer report, and the refused capacities and stretches must leave
// sentinel-filled buffers as they were. Stand-alone, built with ASan + UBSan by tests/test_svcaller_host.py; nothing is preloaded.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../floxer_amd/csrc/flx_svcaller.hpp"

namespace flx {
static std::string last_error;
void set_error(const std::string& m) { last_error = m; }
}

struct Span { uint32_t ref, rs, re; };

static uint32_t count_by_walk(std::vector<Span> const& spans, flx_sv_cluster const& c, uint64_t n_r, uint32_t flank) {
    uint64_t const lo = c.pos_a_min, hi = c.type == flx::SV_DEL ? (uint64_t)c.pos_a_max + c.q_max : (uint64_t)c.pos_a_max + 1;
    uint64_t const lo2 = lo >= flank ? lo - flank : 0, hi2 = std::min<uint64_t>(hi + flank, n_r);
    uint32_t n = 0;
    for (auto const& s : spans) n += s.ref == (uint32_t)c.ref_a && s.rs <= lo2 && s.re >= hi2;
    return n;
}

static int fail(const char* what, int c) { printf("case %d: %s (%s)\n", c, what, flx::last_error.c_str()); return 1; }
static bool said(const char* part) { return flx::last_error.find(part) != std::string::npos; }

int main() {
    std::mt19937_64 rng(20261022);
    static const uint32_t ops[5] = {7, 8, 1, 2, 4};
    static const uint32_t flags[6] = {0, 16, 256, 272, 2048, 4};
    int const n_cases = 600;
    uint64_t n_counted = 0, n_rows_all = 0, n_spanned = 0, n_absorbed = 0, n_empty_rows = 0, n_empty_spans = 0;
    for (int c = 0; c < n_cases; ++c) {
        uint32_t const n_refs = 1 + (uint32_t)(rng() % 3);
        std::vector<uint64_t> lens(n_refs), starts;
        for (auto& l : lens) l = 2 + rng() % (c % 3 ? 400 : 40);
        if (!flx::coverage_lengths_valid(lens.data(), n_refs, "check", starts)) return fail("valid lengths were refused", c);
        flx_svcall_options o{};
        o.count_secondary = rng() % 2; o.min_mapq = rng() % 3 ? 0 : 1 + (uint32_t)(rng() % 60); o.flank = rng() % 3 ? (uint32_t)(rng() % 30) : 0;
        flx::SvcallModel const m = flx::svcall_model(o);
        // records
        std::vector<flx_record> recs;
        std::vector<uint32_t> words;
        std::vector<Span> want;
        std::vector<size_t> want_upto;                                     // want.size() behind every record
        int const n_rec = c % 7 == 0 ? 0 : (int)(rng() % 60);
        for (int r = 0; r < n_rec; ++r) {
            flx_record rec{};
            rec.flag = flags[rng() % 6];
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
            want_upto.push_back(want.size());
        }
        n_counted += want.size();
        // clusters
        std::vector<flx_sv_cluster> clusters;
        int const n_cl = c % 5 == 0 ? 0 : (int)(rng() % 25);
        for (int k = 0; k < n_cl; ++k) {
            flx_sv_cluster cl{};
            cl.type = (uint32_t)(rng() % 3);
            cl.ref_a = cl.ref_b = (int32_t)(rng() % n_refs);
            cl.support = (uint32_t)(rng() % 12);
            uint64_t const len = lens[(size_t)cl.ref_a];
            cl.q_min = 1 + (uint32_t)(rng() % 20); cl.q_median = cl.q_min + (uint32_t)(rng() % 5); cl.q_max = cl.q_median + (uint32_t)(rng() % 5);
            if (cl.type == flx::SV_BND) { cl.pos_a_min = 0; cl.pos_a_max = (uint32_t)(len - 1); clusters.push_back(cl); continue; }
            if (cl.type == flx::SV_DEL && cl.q_max > len) continue;
            uint64_t const room = cl.type == flx::SV_DEL ? len - cl.q_max : len - 1;
            cl.pos_a_max = rng() % 5 == 0 ? (uint32_t)room : (uint32_t)(rng() % (room + 1));
            cl.pos_a_min = rng() % 5 == 0 ? 0u : cl.pos_a_max - (uint32_t)(rng() % std::min<uint64_t>(cl.pos_a_max + 1, 8));
            clusters.push_back(cl);
        }
        uint64_t n_rows = 0;
        if (!flx::svcall_clusters_valid(starts, clusters.data(), clusters.size(), "check", n_rows)) return fail("valid clusters were refused", c);
        std::vector<flx::u32> index;
        if (flx::svcall_row_index(clusters.data(), clusters.size(), "check", index) != FLX_OK || index.size() != n_rows) return fail("the row index differs", c);

        // the sorted spans and max_span by definition
        std::vector<Span> sorted(want);
        std::sort(sorted.begin(), sorted.end(), [](Span const& a, Span const& b) { return a.ref != b.ref ? a.ref < b.ref : a.rs != b.rs ? a.rs < b.rs : a.re < b.re; });
        uint32_t max_span = 0;
        for (auto const& s : want) max_span = std::max(max_span, s.re - s.rs);

        // three ways to the same table: one add; pieces cut anywhere; two tables and an absorb
        for (int way = 0; way < 3; ++way) {
            flx::SvcallHostTable table, other;
            auto add = [&](flx::SvcallHostTable& t, size_t from, size_t to) {
                std::vector<flx::SvcallJob> jobs;
                // the piece's records with a word pool of exactly the needed size
                std::vector<uint32_t> exact(words);
                if (!flx::svcall_plan(starts, o, recs.data() + from, to - from, exact.data(), exact.size(), "check", jobs)) return false;
                size_t const before = from ? want_upto[from - 1] : 0, after = to ? want_upto[to - 1] : 0;
                if (jobs.size() != after - before) return false;
                return t.add(jobs, "check") == FLX_OK;
            };
            if (way == 0) { if (!add(table, 0, recs.size())) return fail("one add failed", c); }
            else if (way == 1) {
                size_t at = 0;
                for (int piece = 0; piece < 5; ++piece) {
                    size_t const to = piece == 4 ? recs.size() : at + (size_t)(rng() % (recs.size() - at + 1));
                    if (!add(table, at, to)) return fail("a piece failed", c);
                    at = to;
                }
            } else {
                size_t const cut = (size_t)(rng() % (recs.size() + 1));
                if (!add(table, 0, cut) || !add(other, cut, recs.size())) return fail("an add before the absorb failed", c);
                n_absorbed += other.keys.size();
                if (table.absorb(other, "check") != FLX_OK) return fail("the absorb failed", c);
                if (!other.keys.empty() || other.max_span != 0) return fail("the absorbed table is not empty", c);
            }
            if (table.keys.size() != want.size() || table.max_span != max_span) return fail("the table's count or max_span differs", c);
            table.finish(starts, clusters.data(), clusters.size(), m);
            if (table.rows.size() != n_rows) return fail("another number of rows", c);

            // the spans, whole and in stretches, into exactly sized heap buffers
            size_t const n = sorted.size();
            {
                std::unique_ptr<flx_svcall_span[]> out(n ? new flx_svcall_span[n] : nullptr);
                if (table.copy_spans(0, n, out.get()) != FLX_OK) return fail("copy_spans of all spans failed", c);
                for (size_t i = 0; i < n; ++i)
                    if ((uint32_t)out[i].ref != sorted[i].ref || out[i].rs != sorted[i].rs || out[i].re != sorted[i].re || out[i].reserved != 0) return fail("a span differs from the sorted walk", c);
                if (n == 0) ++n_empty_spans;
                if (n) {
                    size_t const a = (size_t)(rng() % n), b = a + (size_t)(rng() % (n - a + 1));
                    std::unique_ptr<flx_svcall_span[]> part(b > a ? new flx_svcall_span[b - a] : nullptr);
                    if (table.copy_spans(a, b, part.get()) != FLX_OK) return fail("copy_spans of a stretch failed", c);
                    for (size_t i = a; i < b; ++i) if (part[i - a].rs != sorted[i].rs || part[i - a].re != sorted[i].re) return fail("a stretch differs", c);
                }
                // refused stretches leave the buffer as it was
                flx_svcall_span sentinel{-7, 7, 7, 7};
                if (table.copy_spans(0, n + 1, &sentinel) != FLX_ERR_INVALID || !said("a stretch outside the spans") || sentinel.rs != 7) return fail("a stretch past the spans was taken", c);
                if (table.copy_spans(1, 0, &sentinel) != FLX_ERR_INVALID || !said("a stretch outside the spans") || sentinel.rs != 7) return fail("a stretch from > to was taken", c);
                if (table.copy_spans(n, n, nullptr) != FLX_OK) return fail("an empty stretch was refused", c);
                if (n && (table.copy_spans(0, n, nullptr) != FLX_ERR_INVALID || !said("null argument"))) return fail("a null span buffer was taken", c);
            }
            // the rows: exactly sized, one larger with a sentinel behind, one smaller refused
            {
                std::unique_ptr<flx_svcall_row[]> out(n_rows ? new flx_svcall_row[n_rows] : nullptr);
                if (table.copy_rows(out.get(), n_rows) != FLX_OK) return fail("copy_rows into an exact buffer failed", c);
                if (n_rows == 0) ++n_empty_rows;
                size_t at = 0;
                for (size_t i = 0; i < clusters.size(); ++i) {
                    flx_sv_cluster const& cl = clusters[i];
                    if (cl.type == flx::SV_BND) continue;
                    flx_svcall_row const& r = out[at++];
                    uint32_t const span_n = count_by_walk(want, cl, lens[(size_t)cl.ref_a], m.flank);
                    flx_svcall_row const w = flx::svcall_row((uint32_t)i, cl, span_n, m);
                    if (r.cluster != i || r.span_n != span_n || r.alt_n != cl.support || r.ref_n != (span_n > cl.support ? span_n - cl.support : 0) || r.gt != w.gt || r.qual != w.qual ||
                        r.pass != w.pass || r.pos_a_min != cl.pos_a_min || r.q_max != cl.q_max)
                        return fail("a row differs from the walk over every span", c);
                    n_spanned += span_n > 0;
                }
                n_rows_all += n_rows;
                std::unique_ptr<flx_svcall_row[]> wide(new flx_svcall_row[n_rows + 1]);
                for (size_t i = 0; i <= n_rows; ++i) wide[i].cluster = 0xABCDu;
                if (table.copy_rows(wide.get(), n_rows) != FLX_OK || wide[n_rows].cluster != 0xABCDu) return fail("copy_rows wrote behind its capacity", c);
                if (table.copy_rows(wide.get(), n_rows + 1) != FLX_OK || wide[n_rows].cluster != 0xABCDu) return fail("copy_rows wrote more than num_rows rows", c);
                if (n_rows) {
                    for (size_t i = 0; i <= n_rows; ++i) wide[i].cluster = 0xABCDu;
                    if (table.copy_rows(wide.get(), n_rows - 1) != FLX_ERR_CAPACITY || !said("the row buffer is too small")) return fail("a capacity of n - 1 was taken", c);
                    for (size_t i = 0; i <= n_rows; ++i) if (wide[i].cluster != 0xABCDu) return fail("a refused copy_rows wrote", c);
                    if (table.copy_rows(nullptr, n_rows) != FLX_ERR_INVALID || !said("null argument")) return fail("a null row buffer was taken", c);
                    if (table.copy_rows(nullptr, 0) != FLX_ERR_CAPACITY) return fail("a capacity of 0 was taken", c);
                } else if (table.copy_rows(nullptr, 0) != FLX_OK) return fail("no rows into no buffer was refused", c);
            }
        }
    }
    // the judgements alone, and the room of a table
    {
        flx::u64 n = 9;
        if (flx::rows_copy_judged(3, nullptr, 2, n) != FLX_ERR_CAPACITY || n != 0) { printf("rows_copy_judged took a small capacity\n"); return 1; }
        if (flx::rows_copy_judged(3, &n, 1000, n) != FLX_OK || n != 3) { printf("rows_copy_judged does not give num_rows\n"); return 1; }
        if (flx::spans_copy_judged(10, 2, 7, &n, n) != FLX_OK || n != 5) { printf("spans_copy_judged does not give the stretch\n"); return 1; }
        if (flx::spans_room_judged(flx::SVCALL_MAX_SPANS - 1, 1, "check") != FLX_OK || flx::spans_room_judged(flx::SVCALL_MAX_SPANS - 1, 2, "check") != FLX_ERR_CAPACITY ||
            !said("more than 2^32 - 1 spans"))
            { printf("spans_room_judged differs at its limit\n"); return 1; }
        flx_svcall_options a{}, b{};
        b.flank = 50; b.min_qual = 2000; b.cost_match = 36;                 // the defaults spelled out are the defaults
        if (!flx::svcall_options_equal(a, b)) { printf("equal options differ\n"); return 1; }
        b.flank = 51;
        if (flx::svcall_options_equal(a, b)) { printf("different options are equal\n"); return 1; }
    }
    if (n_spanned < 200 || n_absorbed < 1000 || !n_empty_rows || !n_empty_spans) {
        printf("the cases miss a kind: spanned %llu absorbed %llu tables without rows %llu without spans %llu\n", (unsigned long long)n_spanned, (unsigned long long)n_absorbed,
               (unsigned long long)n_empty_rows, (unsigned long long)n_empty_spans);
        return 1;
    }
    printf("ok %d cases, %llu counted records, %llu rows (%llu spanned), %llu spans absorbed\n", n_cases, (unsigned long long)n_counted, (unsigned long long)n_rows_all,
           (unsigned long long)n_spanned, (unsigned long long)n_absorbed);
    return 0;
}
