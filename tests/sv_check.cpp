// The structural-variant rule of flx_sv.hpp (one implementation, shared by flx_sv_host, by the checks in front of every launch and, for
// the key and the junction, by the kernels) on random records against a definition that walks every word on its own into arrays of
// exactly the needed size, so that a step outside them is an AddressSanitizer report: the plan's counts and offsets, the walk, the
// junctions, the key's pack and unpack functions up to the largest reference ids, and the clustering against a definition over tuples.
// Stand-alone, built with ASan + UBSan by tests/test_sv_host.py.
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../floxer_amd/csrc/flx_sv.hpp"

namespace flx {
static std::string last_error;
void set_error(const std::string& m) { last_error = m; }
}

using Sig = std::array<uint64_t, 7>;                    // type, side_a, side_b, ref_a, ref_b, pos_a, q: the key order

static Sig sig_of(flx::SortKey const& k) {
    return Sig{flx::sv_key_type(k), flx::sv_key_side_a(k), flx::sv_key_side_b(k), flx::sv_key_ref_a(k), flx::sv_key_ref_b(k), flx::sv_key_pos_a(k), flx::sv_key_q(k)};
}

// the clusters of sorted tuples, by the rule's text: {type, side_a, side_b, support, ref_a, ref_b, pos_min, pos_max, q_min, q_median, q_max}
static std::vector<std::array<uint64_t, 11>> clusters_by_definition(std::vector<Sig> sigs, uint64_t max_distance, uint64_t min_support) {
    std::sort(sigs.begin(), sigs.end());
    std::vector<std::vector<Sig>> coarse;
    for (auto const& s : sigs) {
        bool joins = !coarse.empty();
        if (joins) {
            Sig const& p = coarse.back().back();
            for (int f = 0; f < 5; ++f) joins = joins && p[f] == s[f];
            joins = joins && s[5] - p[5] <= max_distance;
        }
        if (joins) coarse.back().push_back(s); else coarse.push_back({s});
    }
    std::vector<std::array<uint64_t, 11>> out;
    for (auto& g : coarse) {
        std::sort(g.begin(), g.end(), [](Sig const& a, Sig const& b) { return a[6] != b[6] ? a[6] < b[6] : a[5] < b[5]; });
        size_t a = 0;
        while (a < g.size()) {
            size_t b = a + 1;
            while (b < g.size() && g[b][6] - g[b - 1][6] <= max_distance) ++b;
            uint64_t lo = g[a][5], hi = g[a][5];
            for (size_t k = a; k < b; ++k) { lo = std::min(lo, g[k][5]); hi = std::max(hi, g[k][5]); }
            if (b - a >= min_support) out.push_back({g[a][0], g[a][1], g[a][2], b - a, g[a][3], g[a][4], lo, hi, g[a][6], g[a + (b - a - 1) / 2][6], g[b - 1][6]});
            a = b;
        }
    }
    return out;
}

int main() {
    std::mt19937_64 rng(20250611);
    // ---- the key: every field at its extremes, and random fields
    uint64_t n_keys = 0;
    for (int c = 0; c < 200000; ++c) {
        bool const edge = c < 4096;
        uint32_t const type = (uint32_t)(rng() % 3), sa = (uint32_t)(rng() % 2), sb = (uint32_t)(rng() % 2);
        uint32_t const ra = edge ? ((c & 1) ? (1u << 30) - 1u : (c & 2) ? 1u << 29 : 0u) : (uint32_t)(rng() % (1u << 30));
        uint32_t const rb = edge ? ((c & 4) ? (1u << 30) - 1u : (c & 8) ? 1u : 0u) : (uint32_t)(rng() % (1u << 30));
        uint32_t const pos = edge ? ((c & 16) ? 0xFFFFFFFFu : (c & 32) ? 0x7FFFFFFFu : 0u) : (uint32_t)rng();
        uint32_t const q = edge ? ((c & 64) ? 0xFFFFFFFFu : (c & 128) ? 0x80000000u : 0u) : (uint32_t)rng();
        flx::SortKey const k = flx::sv_key(type, sa, sb, ra, rb, pos, q);
        if (sig_of(k) != Sig{type, sa, sb, ra, rb, pos, q}) { printf("key %d: unpack differs from what was packed\n", c); return 1; }
        if (k.hi != ((uint64_t)type << 62 | (uint64_t)sa << 61 | (uint64_t)sb << 60 | (uint64_t)ra << 30 | rb) || k.lo != ((uint64_t)pos << 32 | q)) { printf("key %d: layout\n", c); return 1; }
        flx_sv_signature const g = flx::sv_signature_of(k);
        flx::SortKey const back = flx::sv_key_of(g);
        if (back.hi != k.hi || back.lo != k.lo || g.reserved != 0) { printf("key %d: the signature does not pack back\n", c); return 1; }
        // the key order is the tuple order
        uint32_t const type2 = (uint32_t)(rng() % 3), ra2 = rng() % 2 ? ra : (uint32_t)(rng() % (1u << 30)), pos2 = rng() % 2 ? pos : (uint32_t)rng(), q2 = (uint32_t)rng();
        flx::SortKey const k2 = flx::sv_key(type2, sa, sb, ra2, rb, pos2, q2);
        if (flx::sort_key_less(k, k2) != (sig_of(k) < sig_of(k2))) { printf("key %d: the key order is not the tuple order\n", c); return 1; }
        ++n_keys;
    }
    // ---- plan, walk and junctions on random records
    static const uint32_t ops[5] = {7, 8, 1, 2, 4};
    static const uint32_t flags[7] = {0, 16, 256, 272, 2048, 2064, 4};
    uint64_t n_counted = 0, n_del = 0, n_ins = 0, n_bnd = 0, n_first_ins = 0, n_clusters = 0;
    for (int c = 0; c < 1500; ++c) {
        uint32_t const n_refs = 1 + (uint32_t)(rng() % 4);
        std::vector<uint64_t> lens(n_refs), starts;
        for (auto& l : lens) l = 400 + rng() % 2000;                     // (a read fits every sequence)
        if (!flx::sv_lengths_valid(lens.data(), n_refs, "check", starts)) { printf("case %d: valid lengths were refused\n", c); return 1; }
        flx_sv_options o{};
        o.count_secondary = rng() % 2; o.min_mapq = rng() % 3 ? 0 : 1 + (uint32_t)(rng() % 60);
        o.min_length = rng() % 2 ? 0 : 1 + (uint32_t)(rng() % 40);
        o.max_distance = rng() % 2 ? 0 : 1 + (uint32_t)(rng() % 300);
        o.min_support = (uint32_t)(rng() % 4);
        flx::SvThresholds const t = flx::sv_thresholds(o);
        std::vector<flx_record> recs;
        std::vector<uint32_t> words;
        std::vector<uint64_t> read_lens;
        std::vector<Sig> want;
        struct Member { uint64_t q_start, index, ref, rs, re; bool reverse; };
        std::vector<Member> group;
        auto close_group = [&] {
            std::sort(group.begin(), group.end(), [](Member const& a, Member const& b) { return a.q_start != b.q_start ? a.q_start < b.q_start : a.index < b.index; });
            for (size_t k = 0; k + 1 < group.size(); ++k) {
                Member const &a = group[k], &b = group[k + 1];
                std::array<uint64_t, 3> ea = a.reverse ? std::array<uint64_t, 3>{a.ref, a.rs, 0} : std::array<uint64_t, 3>{a.ref, a.re - 1, 1};
                std::array<uint64_t, 3> eb = b.reverse ? std::array<uint64_t, 3>{b.ref, b.re - 1, 1} : std::array<uint64_t, 3>{b.ref, b.rs, 0};
                if (eb < ea) std::swap(ea, eb);
                want.push_back(Sig{2, ea[2], eb[2], ea[0], eb[0], ea[1], eb[1]});
                ++n_bnd;
            }
            group.clear();
        };
        uint64_t const n_reads = 1 + rng() % 12;
        for (uint64_t read = 0; read < n_reads; ++read) {
            uint64_t const read_len = 60 + rng() % 300;
            read_lens.push_back(read_len);
            uint32_t const n_rec = 1 + (uint32_t)(rng() % 5);
            for (uint32_t k = 0; k < n_rec; ++k) {
                flx_record rec{};
                rec.read_index = read;
                rec.flag = flags[rng() % 7];
                rec.reserved = (uint32_t)(rng() % 3 == 0 ? 0 : rng() % 61);
                if (rec.flag == 4) { rec.reference_id = -1; recs.push_back(rec); continue; }
                rec.reference_id = (int32_t)(rng() % n_refs);
                uint64_t const len = lens[(size_t)rec.reference_id];
                uint64_t const lead = rng() % 3 ? 0 : 1 + rng() % 20, trail = rng() % 3 ? 0 : 1 + rng() % 20;
                std::vector<uint32_t> w;
                if (lead) w.push_back((uint32_t)(lead << 4) | 4u);
                uint64_t left = read_len - lead - trail, span = 0;
                uint32_t const T = (uint32_t)(rng() % 10);
                for (uint32_t x = 0; x < T; ++x) {
                    uint32_t const op = ops[rng() % 4], l = rng() % 2 ? 1 + (uint32_t)(rng() % 8) : t.min_length - 1 + (uint32_t)(rng() % 3);
                    if (l == 0) continue;
                    if ((op == 7 || op == 8 || op == 1) && l + 1 > left) continue;
                    if ((op == 7 || op == 8 || op == 2) && span + l + left > len) continue;
                    if (op != 2) left -= l;
                    if (op != 1) span += l;
                    w.push_back((l << 4) | op);
                }
                w.push_back((uint32_t)(left << 4) | 7u);             // (left >= 1 and the span fits: the loop kept room for it)
                span += left;
                if (trail) w.push_back((uint32_t)(trail << 4) | 4u);
                if (span > len) { printf("case %d: the generator made a span too long\n", c); return 1; }
                rec.position = (int32_t)(rng() % 4 == 0 ? len - span : rng() % (len - span + 1));
                rec.cigar_offset = words.size();
                rec.cigar_length = (uint32_t)w.size();
                words.insert(words.end(), w.begin(), w.end());
                bool counts = true;
                if ((rec.flag & 256u) && !o.count_secondary) counts = false;
                if (o.min_mapq > 0 && rec.reserved < o.min_mapq) counts = false;
                if (counts) {
                    ++n_counted;
                    uint64_t p = (uint64_t)rec.position;
                    for (uint32_t word : w) {
                        uint32_t const op = word & 15u, l = word >> 4;
                        if (op == 2 && l >= t.min_length) { want.push_back(Sig{0, 0, 0, (uint64_t)rec.reference_id, (uint64_t)rec.reference_id, p, l}); ++n_del; }
                        if (op == 1 && l >= t.min_length) {
                            bool const preceded = p > (uint64_t)rec.position;
                            want.push_back(Sig{1, 0, 0, (uint64_t)rec.reference_id, (uint64_t)rec.reference_id, preceded ? p - 1 : p, l});
                            ++n_ins;
                            n_first_ins += preceded ? 0 : 1;
                        }
                        if (op == 7 || op == 8 || op == 2) p += l;
                    }
                    if (!(rec.flag & 256u)) group.push_back(Member{(rec.flag & 16u) ? trail : lead, recs.size(), (uint64_t)rec.reference_id, (uint64_t)rec.position, p, (rec.flag & 16u) != 0});
                }
                recs.push_back(rec);
            }
            close_group();
        }
        std::vector<uint32_t> const pool(words);                        // exactly the words: a read outside them is a report
        flx::SvPlan plan;
        if (!flx::sv_plan(starts, o, recs.data(), recs.size(), pool.data(), pool.size(), n_reads, [&](uint64_t r) { return read_lens[r]; }, "check", plan)) {
            printf("case %d: valid records were refused: %s\n", c, flx::last_error.c_str());
            return 1;
        }
        if (plan.n_keys() != want.size()) { printf("case %d: the plan counts %llu keys, the definition %zu\n", c, (unsigned long long)plan.n_keys(), want.size()); return 1; }
        uint64_t events = 0;
        for (auto const& j : plan.jobs) { if (j.key_off != events) { printf("case %d: a job's offset is not the exclusive sum\n", c); return 1; } events += j.n_events; }
        if (events != plan.n_events) { printf("case %d: the events do not sum\n", c); return 1; }
        std::vector<flx::SortKey> keys;                                 // exactly n_keys entries behind sv_keys_host's resize
        flx::sv_keys_host(plan, pool.data(), t.min_length, keys);
        std::vector<Sig> got;
        for (auto const& k : keys) got.push_back(sig_of(k));
        std::sort(got.begin(), got.end());
        std::vector<Sig> sorted_want(want);
        std::sort(sorted_want.begin(), sorted_want.end());
        if (got != sorted_want) { printf("case %d: the signatures differ from the definition\n", c); return 1; }
        // the clusters
        std::sort(keys.begin(), keys.end(), [](flx::SortKey const& a, flx::SortKey const& b) { return flx::sort_key_less(a, b); });
        std::vector<flx_sv_cluster> cl;
        flx::sv_clusters_host(keys.data(), keys.size(), t, cl);
        auto const def = clusters_by_definition(want, t.max_distance, t.min_support);
        if (cl.size() != def.size()) { printf("case %d: %zu clusters, the definition has %zu\n", c, cl.size(), def.size()); return 1; }
        for (size_t k = 0; k < cl.size(); ++k) {
            std::array<uint64_t, 11> const g{cl[k].type, cl[k].side_a, cl[k].side_b, cl[k].support, (uint64_t)cl[k].ref_a, (uint64_t)cl[k].ref_b, cl[k].pos_a_min, cl[k].pos_a_max,
                                             cl[k].q_min, cl[k].q_median, cl[k].q_max};
            if (g != def[k] || cl[k].reserved != 0) { printf("case %d: cluster %zu differs from the definition\n", c, k); return 1; }
        }
        n_clusters += cl.size();
        // one bad record behind the good ones: each of the rule's own refusals
        if (c % 10 == 0 && !recs.empty()) {
            struct Bad { std::vector<uint32_t> w; uint64_t read_len; const char* match; };
            std::vector<Bad> const bads = {{{(4u << 4) | 7u, (3u << 4) | 4u, (2u << 4) | 7u}, 9, "both sides"}, {{(4u << 4) | 7u}, 5, "sum to 4"},
                                           {{(4u << 4) | 1u, (2u << 4) | 4u}, 6, "no reference-consuming column"}};
            for (auto const& b : bads) {
                std::vector<flx_record> r2(recs);
                std::vector<uint32_t> w2(words);
                std::vector<uint64_t> l2(read_lens);
                flx_record rec{};
                rec.read_index = l2.size(); rec.reference_id = 0; rec.reserved = 60; rec.cigar_offset = w2.size(); rec.cigar_length = (uint32_t)b.w.size();
                w2.insert(w2.end(), b.w.begin(), b.w.end());
                l2.push_back(b.read_len);
                r2.push_back(rec);
                flx::SvPlan p2;
                if (flx::sv_plan(starts, o, r2.data(), r2.size(), w2.data(), w2.size(), l2.size(), [&](uint64_t r) { return l2[r]; }, "check", p2) ||
                    flx::last_error.find(b.match) == std::string::npos) {
                    printf("case %d: a bad record (%s) was not refused as such: %s\n", c, b.match, flx::last_error.c_str());
                    return 1;
                }
            }
            std::vector<flx_record> r2(recs);
            r2.back().read_index = n_reads;                             // outside the reads (the last record may not count: then it is fine)
            flx::SvPlan p2;
            bool const ok = flx::sv_plan(starts, o, r2.data(), r2.size(), pool.data(), pool.size(), n_reads, [&](uint64_t r) { return read_lens.at(r); }, "check", p2);
            flx_coverage_options const f = flx::sv_filter(o);
            if (ok == flx::coverage_record_counts(r2.back(), f)) { printf("case %d: a read_index outside the reads\n", c); return 1; }
        }
    }
    // 2^30 sequences are refused by their count, ahead of the lengths: the array of one entry is never read behind its end
    for (uint32_t n_refs : {1u << 30, (1u << 30) + 1u, 0xFFFFFFFFu}) {
        std::vector<uint64_t> const one{100};
        std::vector<uint64_t> starts{7};
        flx::last_error.clear();
        if (flx::sv_lengths_valid(one.data(), n_refs, "check", starts) || flx::last_error.find("2^30 sequences") == std::string::npos || starts != std::vector<uint64_t>{7}) {
            printf("%u sequences were not refused by their count: %s\n", n_refs, flx::last_error.c_str());
            return 1;
        }
    }
    // a group of 64 members is taken, one of 65 refused
    for (uint32_t m : {64u, 65u}) {
        std::vector<flx_record> recs(m);
        std::vector<uint32_t> const words{(5u << 4) | 7u};
        for (uint32_t k = 0; k < m; ++k) { recs[k] = flx_record{}; recs[k].flag = k ? 2048u : 0u; recs[k].cigar_length = 1; recs[k].position = (int32_t)k; }
        std::vector<uint64_t> const starts{0, 100};
        flx::SvPlan plan;
        bool const ok = flx::sv_plan(starts, flx_sv_options{}, recs.data(), recs.size(), words.data(), words.size(), 1, [](uint64_t) { return 5; }, "check", plan);
        if (ok != (m == 64) || (ok && (plan.n_junctions != 63 || plan.members.size() != 64))) { printf("a group of %u members\n", m); return 1; }
    }
    if (n_del < 1000 || n_ins < 1000 || n_bnd < 1000 || n_first_ins == 0 || n_clusters < 100) { printf("the cases are too thin: %llu %llu %llu %llu %llu\n", (unsigned long long)n_del, (unsigned long long)n_ins, (unsigned long long)n_bnd, (unsigned long long)n_first_ins, (unsigned long long)n_clusters); return 1; }
    printf("ok keys %llu counted %llu del %llu ins %llu (first %llu) bnd %llu clusters %llu\n", (unsigned long long)n_keys, (unsigned long long)n_counted, (unsigned long long)n_del,
           (unsigned long long)n_ins, (unsigned long long)n_first_ins, (unsigned long long)n_bnd, (unsigned long long)n_clusters);
    return 0;
}
