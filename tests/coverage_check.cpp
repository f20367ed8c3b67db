// The coverage rule of flx_coverage.hpp (one host implementation, shared by flx_coverage_host and by the checks in front of every launch)
// on random records against a definition that walks every column on its own, in arrays of exactly the needed size, so that a step
// outside them is an AddressSanitizer report; then every refusal on one bad record behind good ones. In front of that compact_words, the
// word pool that an add of coverage or pileup uploads. Stand-alone, built with ASan + UBSan by tests/test_coverage_host.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../floxer_amd/csrc/flx_coverage.hpp"

namespace flx {
static std::string last_error;
void set_error(const std::string& m) { last_error = m; }
}

// compact_words on spans {word_off, n_words} of a pool of n_pool words (each word holds its own index, so a word is recognised wherever
// it lands): every job reads the same words through the compacted pool as through the original, and the compacted pool holds each used
// word once. Both pools have exactly their size, so a step outside them is an AddressSanitizer report.
static bool compact_case(const char* name, uint64_t n_pool, std::vector<std::pair<uint64_t, uint32_t>> const& spans) {
    std::vector<uint32_t> original(n_pool);
    for (uint64_t i = 0; i < n_pool; ++i) original[i] = 1000u + (uint32_t)i;
    std::vector<flx::CoverageJob> jobs;
    for (auto const& s : spans) jobs.push_back(flx::CoverageJob{7 * jobs.size(), s.first, s.second, 0u});
    std::vector<uint32_t> used(n_pool, 0);
    for (auto const& s : spans)
        for (uint32_t t = 0; t < s.second; ++t) used[s.first + t] = 1;
    std::vector<uint32_t> pool{99u};                                      // (what it held before is dropped)
    flx::compact_words(jobs, original.data(), pool);
    std::vector<uint32_t> want_pool;
    for (uint64_t i = 0; i < n_pool; ++i) if (used[i]) want_pool.push_back(original[i]);
    if (pool != want_pool) { printf("compact_words, %s: the pool does not hold each used word once, in order\n", name); return false; }
    if (jobs.size() != spans.size()) { printf("compact_words, %s: the number of jobs changed\n", name); return false; }
    for (size_t k = 0; k < jobs.size(); ++k) {
        if (jobs[k].n_words != spans[k].second || jobs[k].text_off != 7 * k) { printf("compact_words, %s: job %zu changed beside its word_off\n", name, k); return false; }
        if (jobs[k].word_off > pool.size() || jobs[k].n_words > pool.size() - jobs[k].word_off) { printf("compact_words, %s: job %zu lies outside the pool\n", name, k); return false; }
        for (uint32_t t = 0; t < jobs[k].n_words; ++t)
            if (pool[jobs[k].word_off + t] != original[spans[k].first + t]) { printf("compact_words, %s: job %zu reads another word at %u\n", name, k, t); return false; }
    }
    return true;
}

static bool compact_cases() {
    std::mt19937_64 rng(7);
    std::vector<std::pair<uint64_t, uint32_t>> random;
    for (int k = 0; k < 300; ++k) { uint64_t const off = rng() % 500; random.emplace_back(off, 1 + (uint32_t)(rng() % std::min<uint64_t>(40, 500 - off))); }
    return compact_case("overlapping spans", 40, {{20, 10}, {3, 9}, {25, 10}, {8, 6}}) &&
           compact_case("nested spans", 40, {{5, 30}, {10, 4}, {12, 1}, {34, 1}, {5, 1}, {30, 9}}) &&
           compact_case("touching spans", 40, {{10, 5}, {15, 5}, {0, 10}, {21, 4}}) &&              // (and a gap of one word at 20)
           compact_case("identical spans", 40, {{17, 6}, {17, 6}, {17, 6}, {2, 3}, {2, 3}}) &&
           compact_case("a span at the pool's last word", 40, {{39, 1}, {0, 2}, {36, 4}}) &&
           compact_case("an empty job list", 40, {}) &&
           compact_case("an empty job list over no pool", 0, {}) &&
           compact_case("the whole pool, out of order", 12, {{6, 6}, {0, 6}}) &&
           compact_case("random spans", 500, random);
}

int main() {
    if (!compact_cases()) return 1;
    std::mt19937_64 rng(20240917);
    static const uint32_t ops[5] = {7, 8, 1, 2, 4};
    static const uint32_t flags[7] = {0, 16, 256, 272, 2048, 2064, 4};
    uint64_t n_counted = 0, n_left_out = 0, n_end = 0;
    int const n_cases = 3000;
    for (int c = 0; c < n_cases; ++c) {
        uint32_t const n_refs = 1 + (uint32_t)(rng() % 5);
        std::vector<uint64_t> lens(n_refs), starts;
        for (auto& l : lens) l = 1 + rng() % 400;
        if (!flx::coverage_lengths_valid(lens.data(), n_refs, "check", starts)) { printf("case %d: valid lengths were refused\n", c); return 1; }
        flx_coverage_options o{};
        o.count_deletions = rng() % 2; o.count_secondary = rng() % 2; o.min_mapq = rng() % 3 ? 0 : 1 + (uint32_t)(rng() % 60);
        std::vector<flx_record> recs;
        std::vector<uint32_t> words;
        std::vector<uint32_t> want(starts.back(), 0);
        for (int r = 0; r < 40; ++r) {
            flx_record rec{};
            rec.flag = flags[rng() % 7];
            rec.reference_id = (int32_t)(rng() % n_refs);
            rec.reserved = (uint32_t)(rng() % 3 == 0 ? 0 : rng() % 61);
            uint32_t const T = 1 + (uint32_t)(rng() % 12);
            std::vector<uint32_t> w;
            uint64_t span = 0;
            for (uint32_t t = 0; t < T; ++t) {
                uint32_t const op = ops[rng() % 5], len = 1 + (uint32_t)(rng() % 30);
                if (flx::coverage_op_consumes(op) && span + len > lens[(size_t)rec.reference_id]) continue;
                if (flx::coverage_op_consumes(op)) span += len;
                w.push_back((len << 4) | op);
            }
            if (w.empty()) w.push_back((1u << 4) | 1u);
            bool const at_end = rng() % 4 == 0;
            rec.position = (int32_t)(at_end ? lens[(size_t)rec.reference_id] - span : rng() % (lens[(size_t)rec.reference_id] - span + 1));
            rec.cigar_offset = words.size();
            rec.cigar_length = (uint32_t)w.size();
            words.insert(words.end(), w.begin(), w.end());
            recs.push_back(rec);
            bool const counts = !(rec.flag & 4u) && (!(rec.flag & 256u) || o.count_secondary) && (o.min_mapq == 0 || rec.reserved >= o.min_mapq);
            if (!counts) { ++n_left_out; continue; }
            ++n_counted;
            n_end += at_end;
            uint64_t p = starts[(size_t)rec.reference_id] + (uint64_t)rec.position;
            for (uint32_t x : w)
                for (uint32_t k = 0; k < (x >> 4); ++k) {
                    uint32_t const op = x & 15u;
                    if (op == 7u || op == 8u || (op == 2u && o.count_deletions)) ++want[p];
                    if (op == 7u || op == 8u || op == 2u) ++p;
                }
        }
        std::vector<flx::CoverageJob> jobs;
        if (!flx::coverage_plan(starts, o, recs.data(), recs.size(), words.data(), words.size(), "check", jobs)) { printf("case %d: valid records were refused: %s\n", c, flx::last_error.c_str()); return 1; }
        std::vector<uint32_t> got(starts.back(), 0);
        for (auto const& j : jobs) flx::coverage_walk(j, words.data(), o.count_deletions != 0, got.data());
        if (got != want) { printf("case %d: the depths differ\n", c); return 1; }
        // one bad record behind the good ones: refused whichever it is
        for (int bad = 0; bad < 6; ++bad) {
            std::vector<flx_record> r2 = recs;
            std::vector<uint32_t> w2 = words;
            flx_record rec{};
            rec.reference_id = 0;
            rec.cigar_offset = w2.size();
            rec.cigar_length = 1;
            w2.push_back((1u << 4) | 7u);
            if (bad == 0) rec.position = (int32_t)lens[0];                                   // ends behind its sequence
            if (bad == 1) rec.reference_id = (int32_t)n_refs;
            if (bad == 2) w2.back() = (1u << 4) | 0u;                                         // M
            if (bad == 3) w2.back() = 7u;                                                     // length 0
            if (bad == 4) rec.cigar_length = 0;
            if (bad == 5) rec.cigar_length = 2;                                               // words outside the pool
            r2.push_back(rec);
            flx_coverage_options all{};
            std::vector<flx::CoverageJob> j2;
            if (flx::coverage_plan(starts, all, r2.data(), r2.size(), w2.data(), w2.size(), "check", j2)) { printf("case %d: bad record %d was accepted\n", c, bad); return 1; }
        }
    }
    {
        std::vector<uint64_t> starts;
        uint64_t const long_one[2] = {5, 1ull << 31}, many[3] = {(1ull << 31) - 1, (1ull << 31) - 1, 2}, none[1] = {0};
        if (flx::coverage_lengths_valid(long_one, 2, "check", starts) || flx::coverage_lengths_valid(many, 3, "check", starts) || flx::coverage_lengths_valid(none, 1, "check", starts) ||
            flx::coverage_lengths_valid(many, 0, "check", starts)) { printf("lengths beyond the limits were accepted\n"); return 1; }
        if (!flx::coverage_lengths_valid(many, 2, "check", starts) || starts.back() != (1ull << 32) - 2) { printf("two sequences of 2^31 - 1 were refused\n"); return 1; }
        std::vector<uint64_t> bases;
        uint64_t const lens[3] = {10, 1, 21};
        flx::coverage_lengths_valid(lens, 3, "check", starts);
        flx::coverage_window_bases(starts, 10, bases);
        if (bases != std::vector<uint64_t>{0, 1, 2, 5}) { printf("window bases at 10\n"); return 1; }
        flx::coverage_window_bases(starts, 0, bases);
        if (bases != std::vector<uint64_t>{0, 1, 2, 3}) { printf("window bases at 0\n"); return 1; }
        flx::coverage_window_bases(starts, ~0ull, bases);
        if (bases != std::vector<uint64_t>{0, 1, 2, 3}) { printf("window bases at 2^64 - 1\n"); return 1; }
    }
    if (!n_counted || !n_left_out || !n_end) { printf("a class of cases did not occur\n"); return 1; }
    printf("ok %d cases: %llu records counted (%llu of them end with their sequence), %llu left out\n", n_cases, (unsigned long long)n_counted, (unsigned long long)n_end, (unsigned long long)n_left_out);
    return 0;
}
