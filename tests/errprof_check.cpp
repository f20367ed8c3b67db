// The error-profile rule of flx_errprof.hpp (one host implementation, shared by flx_errprof_host, by the checks in front of every launch
// and, in its FLX_HD pieces, by the kernel) on random records against a definition that walks every column, every row and every
// position of a homopolymer run on its own. The text, the words and every read live in arrays of exactly the needed size, so that a
// step outside them (a run scanned past either end of the text, a row past a read) is an AddressSanitizer report; sequences are a few
// symbols to a few hundred long and made of runs, so records and runs touch s0 and s1 all the time. Then the refusals of its own.
// Stand-alone, built with ASan + UBSan by tests/test_errprof_host.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../floxer_amd/csrc/flx_errprof.hpp"

namespace flx {
static std::string last_error;
void set_error(const std::string& m) { last_error = m; }
}

using flx::u64;

int main() {
    std::mt19937_64 rng(20261020);
    static const uint32_t ops[5] = {7, 8, 1, 2, 4};
    static const uint32_t flags[7] = {0, 16, 256, 272, 2048, 2064, 4};
    static const uint8_t comp[6] = {0, 4, 3, 2, 1, 5};
    uint64_t n_counted = 0, n_left_out = 0, n_reverse = 0, n_at_s0 = 0, n_at_s1 = 0, n_ins_at_end = 0, n_capped = 0, n_mixed = 0, n_bin0 = 0, n_long = 0;
    int const n_cases = 1500;
    for (int c = 0; c < n_cases; ++c) {
        uint32_t const n_refs = 1 + (uint32_t)(rng() % 4);
        std::vector<uint64_t> lens(n_refs), starts;
        for (auto& l : lens) l = 1 + rng() % (c % 3 ? 300 : 12);
        if (!flx::coverage_lengths_valid(lens.data(), n_refs, "check", starts)) { printf("case %d: valid lengths were refused\n", c); return 1; }
        uint64_t const total = starts.back();
        std::vector<uint8_t> text(total);                                                         // runs of letters, the same letter across boundaries now and then
        for (uint64_t i = 0; i < total;) {
            uint8_t const a = rng() % 12 == 0 ? (uint8_t)(rng() % 2 ? 0 : 5) : (uint8_t)(1 + rng() % (c % 5 ? 4 : 1));
            static const uint32_t run_lens[8] = {1, 1, 2, 3, 7, 31, 33, 70};
            for (uint32_t k = run_lens[rng() % 8]; k && i < total; --k) text[i++] = a;
        }
        if (!flx::errprof_text_valid(text.data(), total, "check")) { printf("case %d: a valid text was refused\n", c); return 1; }
        flx_errprof_options o{};
        o.count_secondary = rng() % 2; o.min_mapq = rng() % 3 ? 0 : 1 + (uint32_t)(rng() % 60);
        std::vector<flx_record> recs;
        std::vector<uint32_t> words;
        std::vector<std::vector<uint8_t>> reads;
        std::vector<uint64_t> want(flx::ERRPROF_ENTRIES, 0);
        for (int r = 0; r < 30; ++r) {
            flx_record rec{};
            rec.flag = flags[rng() % 7];
            rec.reference_id = (int32_t)(rng() % n_refs);
            rec.reserved = (uint32_t)(rng() % 3 == 0 ? 0 : rng() % 61);
            uint64_t const len = lens[(size_t)rec.reference_id], s0 = starts[(size_t)rec.reference_id], s1 = s0 + len;
            uint32_t const T = 1 + (uint32_t)(rng() % 10);
            std::vector<uint32_t> w;
            uint64_t span = 0, rows = 0;
            for (uint32_t t = 0; t < T; ++t) {
                uint32_t const op = ops[rng() % 5], l = 1 + (uint32_t)(rng() % (rng() % 6 ? 12 : 90));
                if (flx::coverage_op_consumes(op) && span + l > len) continue;
                if (flx::coverage_op_consumes(op)) span += l;
                if (flx::pileup_op_consumes_query(op)) rows += l;
                w.push_back((l << 4) | op);
            }
            if (span == 0) { w.push_back((1u << 4) | 7u); span = 1; rows += 1; }
            rec.position = (int32_t)(rng() % 3 == 0 ? len - span : rng() % 3 == 0 ? 0 : rng() % (len - span + 1));
            rec.cigar_offset = words.size();
            rec.cigar_length = (uint32_t)w.size();
            rec.read_index = reads.size();
            words.insert(words.end(), w.begin(), w.end());
            std::vector<uint8_t> read(rows);
            uint8_t const mostly = (uint8_t)(1 + rng() % 4);
            for (auto& x : read) x = rng() % 3 ? mostly : (uint8_t)(rng() % 6);                    // (inserted runs are often uniform)
            reads.push_back(read);
            recs.push_back(rec);
            bool const counts = !(rec.flag & 4u) && (!(rec.flag & 256u) || o.count_secondary) && (o.min_mapq == 0 || rec.reserved >= o.min_mapq);
            if (!counts) { ++n_left_out; continue; }
            ++n_counted;
            bool const reverse = (rec.flag & 16u) != 0;
            n_reverse += reverse;
            std::vector<uint8_t> seq(rows);                                                       // the oriented sequence, written out
            for (uint64_t i = 0; i < rows; ++i) seq[i] = reverse ? comp[read[rows - 1 - i]] : read[i];
            auto bin = [&](uint64_t row) { return rows ? (reverse ? rows - 1 - row : row) * 100 / rows : 0; };
            auto run = [&](uint64_t at, int step, uint8_t a) {                                    // at may be s0 - 1 (wrapped) or s1: outside, no letter
                uint32_t k = 0;
                while (k < 32 && at >= s0 && at < s1 && text.at(at) == a) { ++k; at += (uint64_t)(int64_t)step; }
                return k;
            };
            uint64_t p = s0 + (uint64_t)rec.position, row = 0, m = 0, x = 0, ib = 0, db = 0;
            for (uint32_t wd : w) {
                uint32_t const op = wd & 15u, L = wd >> 4;
                n_long += L >= 64;
                if (op == 7u || op == 8u) {
                    for (uint32_t k = 0; k < L; ++k, ++p, ++row) {
                        ++want[(op == 7u ? flx::EP_PAIR_EQ : flx::EP_PAIR_X) + text.at(p) * 6u + seq.at(row)];
                        ++want[(op == 7u ? flx::EP_POS_MATCH : flx::EP_POS_MISMATCH) + bin(row)];
                    }
                    (op == 7u ? m : x) += L;
                    if (op == 7u) ++want[flx::EP_EQ_RUN + (L < 256 ? L : 256) - 1];
                } else if (op == 1u) {
                    uint8_t const a = seq.at(row);
                    bool mixed = a < 1 || a > 4;
                    for (uint32_t k = 0; k < L; ++k) mixed = mixed || seq.at(row + k) != a;
                    uint32_t const around = mixed ? 0 : run(p - 1, -1, a) + run(p, 1, a);
                    ++want[flx::EP_HP_INS + (mixed ? 33 : around < 32 ? around : 32)];
                    n_mixed += mixed; n_bin0 += !mixed && around == 0; n_ins_at_end += p == s1; n_at_s0 += p == s0;
                    for (uint32_t k = 0; k < L; ++k, ++row) { ++want[flx::EP_INS_LETTER + seq.at(row)]; ++want[flx::EP_POS_INS + bin(row)]; }
                    ++want[flx::EP_INS_LEN + (L < 64 ? L : 64) - 1];
                    ++want[flx::EP_TOTALS + flx::EP_INS_EVENTS];
                    ib += L;
                } else if (op == 2u) {
                    uint8_t const a = text.at(p);
                    bool mixed = a < 1 || a > 4;
                    for (uint32_t k = 0; k < L; ++k) { mixed = mixed || text.at(p + k) != a; ++want[flx::EP_DEL_LETTER + text.at(p + k)]; }
                    uint64_t const whole = mixed ? 0 : (uint64_t)run(p - 1, -1, a) + L + run(p + L, 1, a);
                    ++want[flx::EP_HP_DEL + (mixed ? 33 : whole < 32 ? whole : 32)];
                    n_capped += !mixed && whole >= 32; n_at_s0 += p == s0; n_at_s1 += p + L == s1;
                    ++want[flx::EP_DEL_LEN + (L < 64 ? L : 64) - 1];
                    ++want[flx::EP_POS_DEL + bin(rows ? (row < rows - 1 ? row : rows - 1) : 0)];
                    ++want[flx::EP_TOTALS + flx::EP_DEL_EVENTS];
                    p += L; db += L;
                } else {
                    for (uint32_t k = 0; k < L; ++k, ++row) ++want[flx::EP_POS_CLIP + bin(row)];
                    want[flx::EP_TOTALS + flx::EP_CLIP_BASES] += L;
                }
            }
            ++want[flx::EP_TOTALS + flx::EP_RECORDS];
            want[flx::EP_TOTALS + flx::EP_MATCHES] += m; want[flx::EP_TOTALS + flx::EP_MISMATCHES] += x;
            want[flx::EP_TOTALS + flx::EP_INS_BASES] += ib; want[flx::EP_TOTALS + flx::EP_DEL_BASES] += db;
            ++want[flx::EP_IDENTITY + m * 100 / (m + x + ib + db)];
        }
        auto read_len = [&](uint64_t i) { return (uint64_t)reads[i].size(); };
        std::vector<u64> const seq_base(starts.begin(), starts.end() - 1);
        std::vector<flx::ErrprofJob> jobs;
        if (!flx::errprof_plan(starts, seq_base, o, recs.data(), recs.size(), words.data(), words.size(), reads.size(), read_len, "check", jobs)) { printf("case %d: valid records were refused: %s\n", c, flx::last_error.c_str()); return 1; }
        std::vector<uint64_t> got(flx::ERRPROF_ENTRIES, 0);
        for (auto const& j : jobs) flx::errprof_walk(j, words.data(), text.data(), reads[j.read_index].data(), got.data());
        for (uint32_t i = 0; i < flx::ERRPROF_ENTRIES; ++i)
            if (got[i] != want[i]) { printf("case %d: entry %u differs: %llu, expected %llu\n", c, i, (unsigned long long)got[i], (unsigned long long)want[i]); return 1; }
        // one bad record behind the good ones: refused whichever it is
        for (int bad = 0; bad < 4; ++bad) {
            std::vector<flx_record> r2 = recs;
            std::vector<uint32_t> w2 = words;
            std::vector<std::vector<uint8_t>> reads2 = reads;
            flx_record rec{};
            rec.cigar_offset = w2.size();
            rec.cigar_length = 1;
            rec.read_index = reads2.size();
            w2.push_back((1u << 4) | 7u);
            reads2.push_back(std::vector<uint8_t>(1, 1));
            if (bad == 0) rec.position = (int32_t)lens[0];                                       // coverage's: ends behind its sequence
            if (bad == 1) reads2.back().push_back(2);                                             // pileup's: the read is one letter longer
            if (bad == 2) w2.back() = (1u << 4) | 1u;                                             // pileup's: no reference-consuming column
            if (bad == 3) { w2.back() = (0xFFFFFFFu << 4) | 4u; w2.push_back((1u << 4) | 7u); for (int k = 0; k < 8; ++k) w2.push_back((0xFFFFFFFu << 4) | 4u); rec.cigar_length = 10; }
            r2.push_back(rec);
            auto len2 = [&](uint64_t i) { return bad == 3 && i + 1 == reads2.size() ? (uint64_t)9 * 0xFFFFFFFu + 1 : (uint64_t)reads2[i].size(); };      // its own: 2^31 rows and more (only the length is asked for)
            flx_errprof_options all{};
            std::vector<flx::ErrprofJob> j2;
            if (flx::errprof_plan(starts, seq_base, all, r2.data(), r2.size(), w2.data(), w2.size(), reads2.size(), len2, "check", j2)) { printf("case %d: bad record %d was accepted\n", c, bad); return 1; }
            if (bad == 3 && flx::last_error.find("2^31") == std::string::npos) { printf("case %d: the long record was refused for another reason: %s\n", c, flx::last_error.c_str()); return 1; }
        }
    }
    {
        // the position bins without a division per row against one per row, at the lengths where bins are skipped, shared or uneven
        static const uint64_t read_lens[7] = {1, 2, 99, 100, 101, 250, 10007};
        for (uint64_t len : read_lens)
            for (int reverse = 0; reverse < 2; ++reverse)
                for (uint64_t row = 0; row < len; row += len < 300 ? 1 : 97)
                    for (uint64_t L : {(uint64_t)1, (uint64_t)2, (uint64_t)63, (uint64_t)64, len - row}) {
                        if (row + L > len) continue;
                        std::vector<uint64_t> a(100, 0), b(100, 0);
                        flx::errprof_pos_rows(0, row, L, len, reverse != 0, [&](uint32_t e, uint32_t k) { a.at(e) += k; });
                        for (uint64_t r = row; r < row + L; ++r) ++b.at((reverse ? len - 1 - r : r) * 100 / len);
                        if (a != b) { printf("the position bins of rows [%llu, %llu) of %llu differ\n", (unsigned long long)row, (unsigned long long)(row + L), (unsigned long long)len); return 1; }
                    }
        flx_errprof_options o{};
        o.flush_threshold = (1u << 31) + 1u;
        if (flx::errprof_options_valid(&o)) { printf("a flush threshold above 2^31 was accepted\n"); return 1; }
        o.flush_threshold = 1u << 31; o.reserved[4] = 1;
        if (flx::errprof_options_valid(&o)) { printf("a reserved field was accepted\n"); return 1; }
        uint8_t const bad_text[3] = {1, 6, 2};
        if (flx::errprof_text_valid(bad_text, 3, "check")) { printf("a rank above 5 was accepted\n"); return 1; }
    }
    if (!n_counted || !n_left_out || !n_reverse || !n_at_s0 || !n_at_s1 || !n_ins_at_end || !n_capped || !n_mixed || !n_bin0 || !n_long) { printf("a class of cases did not occur\n"); return 1; }
    printf("ok %d cases: %llu records counted (%llu reverse), %llu left out; gaps at s0 %llu, deletions that end at s1 %llu, insertions at s1 %llu, runs of 32 and more %llu, mixed %llu, insertions in bin 0 %llu, words of 64 and more %llu\n",
           n_cases, (unsigned long long)n_counted, (unsigned long long)n_reverse, (unsigned long long)n_left_out, (unsigned long long)n_at_s0, (unsigned long long)n_at_s1,
           (unsigned long long)n_ins_at_end, (unsigned long long)n_capped, (unsigned long long)n_mixed, (unsigned long long)n_bin0, (unsigned long long)n_long);
    return 0;
}
