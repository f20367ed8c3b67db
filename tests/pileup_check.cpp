// The pileup rule of flx_pileup.hpp (one host implementation, shared by flx_pileup_host and by the checks in front of every launch) on
// random records against a definition that walks every column on its own, in arrays of exactly the needed size, so that a step outside
// them is an AddressSanitizer report; then every refusal of its own on one bad record behind good ones, and the site test on its
// boundaries. Stand-alone, built with ASan + UBSan by tests/test_pileup_host.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../floxer_amd/csrc/flx_pileup.hpp"

namespace flx {
static std::string last_error;
void set_error(const std::string& m) { last_error = m; }
}

int main() {
    std::mt19937_64 rng(20241019);
    static const uint32_t ops[5] = {7, 8, 1, 2, 4};
    static const uint32_t flags[7] = {0, 16, 256, 272, 2048, 2064, 4};
    static const uint8_t comp[6] = {0, 4, 3, 2, 1, 5};
    uint64_t n_counted = 0, n_left_out = 0, n_leading_ins = 0, n_reverse = 0, n_letters = 0, n_not_acgt = 0;
    int const n_cases = 2000;
    for (int c = 0; c < n_cases; ++c) {
        uint32_t const n_refs = 1 + (uint32_t)(rng() % 5);
        std::vector<uint64_t> lens(n_refs), starts;
        for (auto& l : lens) l = 1 + rng() % 400;
        if (!flx::coverage_lengths_valid(lens.data(), n_refs, "check", starts)) { printf("case %d: valid lengths were refused\n", c); return 1; }
        uint64_t const total = starts.back();
        flx_pileup_options o{};
        o.count_secondary = rng() % 2; o.min_mapq = rng() % 3 ? 0 : 1 + (uint32_t)(rng() % 60);
        std::vector<flx_record> recs;
        std::vector<uint32_t> words;
        std::vector<std::vector<uint8_t>> reads;
        std::vector<uint32_t> want(7 * total, 0);
        for (int r = 0; r < 40; ++r) {
            flx_record rec{};
            rec.flag = flags[rng() % 7];
            rec.reference_id = (int32_t)(rng() % n_refs);
            rec.reserved = (uint32_t)(rng() % 3 == 0 ? 0 : rng() % 61);
            uint64_t const len = lens[(size_t)rec.reference_id];
            uint32_t const T = 1 + (uint32_t)(rng() % 12);
            std::vector<uint32_t> w;
            uint64_t span = 0, rows = 0;
            for (uint32_t t = 0; t < T; ++t) {
                uint32_t const op = ops[rng() % 5], l = 1 + (uint32_t)(rng() % 30);
                if (flx::coverage_op_consumes(op) && span + l > len) continue;
                if (flx::coverage_op_consumes(op)) span += l;
                if (flx::pileup_op_consumes_query(op)) rows += l;
                w.push_back((l << 4) | op);
            }
            if (span == 0) { w.push_back((1u << 4) | 7u); span = 1; rows += 1; }          // (every sequence has a symbol)
            rec.position = (int32_t)(rng() % 4 == 0 ? len - span : rng() % (len - span + 1));
            rec.cigar_offset = words.size();
            rec.cigar_length = (uint32_t)w.size();
            rec.read_index = reads.size();
            words.insert(words.end(), w.begin(), w.end());
            std::vector<uint8_t> read(rows);
            for (auto& x : read) x = (uint8_t)(rng() % 6);
            reads.push_back(read);
            recs.push_back(rec);
            bool const counts = !(rec.flag & 4u) && (!(rec.flag & 256u) || o.count_secondary) && (o.min_mapq == 0 || rec.reserved >= o.min_mapq);
            if (!counts) { ++n_left_out; continue; }
            ++n_counted;
            n_reverse += (rec.flag & 16u) != 0;
            n_leading_ins += (w[0] & 15u) == 1u || ((w[0] & 15u) == 4u && w.size() > 1 && (w[1] & 15u) == 1u);
            std::vector<uint8_t> seq(rows);                                                   // the oriented sequence, written out
            for (uint64_t i = 0; i < rows; ++i) seq[i] = (rec.flag & 16u) ? comp[read[rows - 1 - i]] : read[i];
            uint64_t p = starts[(size_t)rec.reference_id] + (uint64_t)rec.position, row = 0;
            bool has_last = false;
            uint64_t last = 0;                                                                // the preceding reference-consuming column
            for (uint32_t x : w) {
                uint32_t const op = x & 15u;
                if (op == 1u) ++want[6 * total + (has_last ? last : p)];
                for (uint32_t k = 0; k < (x >> 4); ++k) {
                    if (op == 7u || op == 8u) ++want[0 * total + p];
                    if (op == 2u) ++want[1 * total + p];
                    if (op == 8u) {
                        ++n_letters;
                        if (seq[row] >= 1 && seq[row] <= 4) ++want[(uint64_t)(2 + seq[row] - 1) * total + p]; else ++n_not_acgt;
                    }
                    if (op == 7u || op == 8u || op == 2u) { last = p; has_last = true; ++p; }
                    if (op == 7u || op == 8u || op == 1u || op == 4u) ++row;
                }
            }
        }
        auto read_len = [&](uint64_t i) { return (uint64_t)reads[i].size(); };
        std::vector<flx::PileupJob> jobs;
        if (!flx::pileup_plan(starts, o, recs.data(), recs.size(), words.data(), words.size(), reads.size(), read_len, "check", jobs)) { printf("case %d: valid records were refused: %s\n", c, flx::last_error.c_str()); return 1; }
        std::vector<uint32_t> got(7 * total, 0);
        for (auto const& j : jobs) flx::pileup_walk(j, words.data(), reads[j.read_index].data(), reads[j.read_index].size(), got.data(), total);
        if (got != want) { printf("case %d: the counts differ\n", c); return 1; }
        // one bad record behind the good ones: refused whichever it is
        for (int bad = 0; bad < 7; ++bad) {
            std::vector<flx_record> r2 = recs;
            std::vector<uint32_t> w2 = words;
            std::vector<std::vector<uint8_t>> reads2 = reads;
            flx_record rec{};
            rec.reference_id = 0;
            rec.cigar_offset = w2.size();
            rec.cigar_length = 1;
            rec.read_index = reads2.size();
            w2.push_back((1u << 4) | 7u);
            reads2.push_back(std::vector<uint8_t>(1, 1));
            if (bad == 0) rec.position = (int32_t)lens[0];                                   // coverage's: ends behind its sequence
            if (bad == 1) w2.back() = (1u << 4) | 0u;                                         // coverage's: M
            if (bad == 2) rec.read_index = reads2.size();                                     // a read that is not there
            if (bad == 3) reads2.back().push_back(2);                                         // the read is one letter longer
            if (bad == 4) reads2.back().clear();                                              // and one shorter
            if (bad == 5) w2.back() = (1u << 4) | 1u;                                         // I alone: no reference-consuming column
            if (bad == 6) w2.back() = (1u << 4) | 4u;                                         // S alone
            r2.push_back(rec);
            auto len2 = [&](uint64_t i) { return (uint64_t)reads2[i].size(); };
            flx_pileup_options all{};
            std::vector<flx::PileupJob> j2;
            if (flx::pileup_plan(starts, all, r2.data(), r2.size(), w2.data(), w2.size(), reads2.size(), len2, "check", j2)) { printf("case %d: bad record %d was accepted\n", c, bad); return 1; }
        }
    }
    {
        flx_pileup_options o{};
        flx::PileupThresholds const d = flx::pileup_thresholds(o);
        if (d.min_depth != 4 || d.min_count != 2 || d.min_permille != 200) { printf("the defaults\n"); return 1; }
        o.min_depth = 10; o.min_count = 3; o.min_permille = 300;
        flx::PileupThresholds const t = flx::pileup_thresholds(o);
        uint32_t const on[7] = {7, 3, 0, 3, 0, 0, 0}, below_fraction[7] = {8, 3, 0, 3, 0, 0, 0}, below_depth[7] = {6, 3, 0, 3, 0, 0, 0}, below_count[7] = {8, 2, 2, 0, 0, 0, 0};
        uint32_t const huge[7] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0, 0xFFFFFFFFu, 0};          // 64-bit products
        if (!flx::pileup_is_site(on, t) || flx::pileup_is_site(below_fraction, t) || flx::pileup_is_site(below_depth, t) || flx::pileup_is_site(below_count, t)) { printf("the site boundaries\n"); return 1; }
        o.min_permille = 500;
        if (!flx::pileup_is_site(huge, flx::pileup_thresholds(o))) { printf("the site test at 2^32 - 1\n"); return 1; }
        o.min_permille = 501;
        if (flx::pileup_is_site(huge, flx::pileup_thresholds(o))) { printf("the site test at 2^32 - 1, one permille above\n"); return 1; }
        o.min_permille = 1001;
        if (flx::pileup_options_valid(&o)) { printf("1001 permille was accepted\n"); return 1; }
        o.min_permille = 1000; o.reserved[1] = 1;
        if (flx::pileup_options_valid(&o)) { printf("a reserved field was accepted\n"); return 1; }
    }
    if (!n_counted || !n_left_out || !n_leading_ins || !n_reverse || !n_letters || !n_not_acgt) { printf("a class of cases did not occur\n"); return 1; }
    printf("ok %d cases: %llu records counted (%llu reverse, %llu with an insertion in front of every column), %llu left out, %llu X letters (%llu not ACGT)\n", n_cases,
           (unsigned long long)n_counted, (unsigned long long)n_reverse, (unsigned long long)n_leading_ins, (unsigned long long)n_left_out, (unsigned long long)n_letters,
           (unsigned long long)n_not_acgt);
    return 0;
}
