// The coverage rule of flx_coverage.hpp (one host implementation, shared by flx_coverage_host and by the checks in front of every launch)
// on random records against a definition that walks every column on its own, in arrays of exactly the needed size, so that a step
// outside them is an AddressSanitizer report; then every refusal on one bad record behind good ones. Stand-alone, built with ASan +
// UBSan by tests/test_coverage_host.py.
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

int main() {
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
