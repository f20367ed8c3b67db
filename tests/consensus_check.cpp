// The consensus rule of flx_consensus.hpp (one host implementation, shared by flx_consensus_host and, in its FLX_HD pieces, by the
// kernels) on random records against a definition that walks every column on its own, keeps every insertion as a string of letters
// and votes position by position with no packed key anywhere. The text, the words and every read live in arrays of exactly the needed
// size, so that a step outside them is an AddressSanitizer report. Then the key's round trip and the refusals of its own.
// Stand-alone, built with ASan + UBSan by tests/test_consensus_host.py.
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../floxer_amd/csrc/flx_consensus.hpp"

namespace flx {
static std::string last_error;
void set_error(const std::string& m) { last_error = m; }
}

using flx::u64;

int main() {
    std::mt19937_64 rng(20261021);
    static const uint32_t ops[5] = {7, 8, 1, 2, 4};
    static const uint32_t flags[7] = {0, 16, 256, 272, 2048, 2064, 4};
    static const uint8_t comp[6] = {0, 4, 3, 2, 1, 5};
    uint64_t n_counted = 0, n_void_first = 0, n_void_long = 0, n_void_letter = 0, n_alleles = 0, n_sub = 0, n_del = 0, n_ins = 0, n_ins_on_del = 0, n_uncalled = 0, n_tie = 0, n_n = 0;
    int const n_cases = 1200;
    for (int c = 0; c < n_cases; ++c) {
        uint32_t const n_refs = 1 + (uint32_t)(rng() % 3);
        std::vector<uint64_t> lens(n_refs), starts;
        for (auto& l : lens) l = 1 + rng() % (c % 3 ? 40 : 6);
        if (!flx::coverage_lengths_valid(lens.data(), n_refs, "check", starts)) { printf("case %d: valid lengths were refused\n", c); return 1; }
        uint64_t const total = starts.back();
        std::vector<uint8_t> text(total);
        for (auto& x : text) x = rng() % 10 == 0 ? (uint8_t)(rng() % 2 ? 0 : 5) : (uint8_t)(1 + rng() % 4);
        flx_consensus_options o{};
        o.count_secondary = rng() % 2; o.min_mapq = rng() % 3 ? 0 : 1 + (uint32_t)(rng() % 60);
        o.min_depth = (uint32_t)(rng() % 4); o.min_count = (uint32_t)(rng() % 3); o.min_permille = rng() % 2 ? 0 : (uint32_t)(rng() % 1001); o.mask_low_depth = rng() % 2;
        flx::ConsensusThresholds const t = flx::consensus_thresholds(o);
        std::vector<flx_record> recs;
        std::vector<uint32_t> words;
        std::vector<std::vector<uint8_t>> reads;
        // the definition's sums: per position the five candidates and the insertions behind it as strings of ranks
        std::vector<uint64_t> depth(total, 0), del(total, 0);
        std::vector<std::vector<uint64_t>> x_letter(total, std::vector<uint64_t>(6, 0));
        std::vector<std::map<std::pair<size_t, std::string>, uint64_t>> ins(total);      // (length, letters) orders as the key does
        // a few insertion strings shared by the records of a case, so that alleles repeat and tie
        std::vector<std::vector<uint8_t>> shared;
        for (int k = 0; k < 4; ++k) { std::vector<uint8_t> s(1 + rng() % (rng() % 4 ? 3 : 34)); for (auto& x : s) x = rng() % 30 ? (uint8_t)(1 + rng() % 4) : (uint8_t)(rng() % 2 ? 0 : 5); shared.push_back(s); }
        for (int r = 0; r < 40; ++r) {
            flx_record rec{};
            rec.flag = flags[rng() % 7];
            rec.reference_id = (int32_t)(rng() % n_refs);
            rec.reserved = (uint32_t)(rng() % 3 == 0 ? 0 : rng() % 61);
            uint64_t const len = lens[(size_t)rec.reference_id], s0 = starts[(size_t)rec.reference_id];
            bool const reverse = (rec.flag & 16u) != 0;
            uint32_t const T = 1 + (uint32_t)(rng() % 9);
            std::vector<uint32_t> w;
            std::vector<uint8_t> seq;                                                             // the oriented sequence, written as the words are drawn
            uint64_t span = 0;
            for (uint32_t k = 0; k < T; ++k) {
                uint32_t const op = ops[rng() % 5];
                uint32_t l = 1 + (uint32_t)(rng() % 4);
                if (flx::coverage_op_consumes(op) && span + l > len) continue;
                if (op == 1u) { auto const& s = shared[rng() % shared.size()]; l = (uint32_t)s.size(); seq.insert(seq.end(), s.begin(), s.end()); }
                else if (flx::pileup_op_consumes_query(op)) for (uint32_t i = 0; i < l; ++i) seq.push_back((uint8_t)(rng() % 12 ? 1 + rng() % 2 : rng() % 6));
                if (flx::coverage_op_consumes(op)) span += l;
                w.push_back((l << 4) | op);
            }
            if (span == 0) { w.push_back((1u << 4) | 7u); span = 1; seq.push_back(1); }
            rec.position = (int32_t)(rng() % 3 == 0 ? len - span : rng() % (len - span + 1));
            rec.cigar_offset = words.size();
            rec.cigar_length = (uint32_t)w.size();
            rec.read_index = reads.size();
            words.insert(words.end(), w.begin(), w.end());
            std::vector<uint8_t> read(seq.size());                                                // the read as given
            for (size_t i = 0; i < seq.size(); ++i) read[i] = reverse ? comp[seq[seq.size() - 1 - i]] : seq[i];
            reads.push_back(read);
            recs.push_back(rec);
            bool const counts = !(rec.flag & 4u) && (!(rec.flag & 256u) || o.count_secondary) && (o.min_mapq == 0 || rec.reserved >= o.min_mapq);
            if (!counts) continue;
            ++n_counted;
            uint64_t p = s0 + (uint64_t)rec.position, row = 0;
            bool any = false;
            for (uint32_t wd : w) {
                uint32_t const op = wd & 15u, L = wd >> 4;
                if (op == 7u || op == 8u) {
                    for (uint32_t k = 0; k < L; ++k, ++p, ++row) { ++depth.at(p); if (op == 8u) ++x_letter.at(p).at(seq.at(row)); }
                    any = true;
                } else if (op == 2u) {
                    for (uint32_t k = 0; k < L; ++k, ++p) ++del.at(p);
                    any = true;
                } else if (op == 1u) {
                    std::string s;
                    bool letters_ok = true;
                    for (uint32_t k = 0; k < L; ++k) { uint8_t const x = seq.at(row + k); letters_ok = letters_ok && x >= 1 && x <= 4; s.push_back((char)('0' + x)); }
                    n_void_first += !any; n_void_long += L > 32; n_void_letter += !letters_ok;
                    if (any && L <= 32 && letters_ok) ++ins.at(p - 1)[{s.size(), s}];
                    row += L;
                } else row += L;
            }
        }
        // the definition's call
        std::vector<std::string> want_letters(n_refs);
        struct Row { uint32_t ref, pos, kind, ref_rank, alt, length; uint64_t count, cov; std::string letters; };
        std::vector<Row> want_rows;
        uint64_t want_alleles = 0;
        for (uint32_t r = 0; r < n_refs; ++r)
            for (uint64_t p = starts[r]; p < starts[r + 1]; ++p) {
                want_alleles += ins[p].size();
                uint32_t const R = text[p];
                uint64_t const cov = depth[p] + del[p];
                if (cov < t.min_depth) { want_letters[r].push_back(o.mask_low_depth || R < 1 || R > 4 ? 'N' : "ACGT"[R - 1]); ++n_uncalled; continue; }
                uint64_t n[6] = {0, x_letter[p][1], x_letter[p][2], x_letter[p][3], x_letter[p][4], del[p]};
                if (R >= 1 && R <= 4) n[R] += depth[p] - n[1] - n[2] - n[3] - n[4];
                uint64_t top = 0;
                for (int k = 1; k <= 5; ++k) top = n[k] > top ? n[k] : top;
                uint32_t best = 0, tied = 0;
                for (uint32_t k = 5; k >= 1; --k) if (n[k] == top) { best = k; ++tied; }
                if (R >= 1 && R <= 4 && n[R] == top) best = R;
                n_tie += tied > 1;
                n_n += R < 1 || R > 4;
                bool const is_r = R >= 1 && R <= 4 && best == R;                                // (R = 5 is the letter N, best = 5 the deletion)
                bool const stands = !is_r && n[best] >= t.min_count && n[best] * 1000 >= (uint64_t)t.min_permille * cov;
                if (stands) {
                    want_rows.push_back(Row{r, (uint32_t)(p - starts[r]), best == 5 ? 1u : 0u, R, best == 5 ? 0u : best, 1u, n[best], cov, ""});
                    if (best != 5) want_letters[r].push_back("ACGT"[best - 1]);
                    (best == 5 ? n_del : n_sub) += 1;
                } else want_letters[r].push_back(R < 1 || R > 4 ? 'N' : "ACGT"[R - 1]);
                const std::pair<const std::pair<size_t, std::string>, uint64_t>* win = nullptr;
                for (auto const& a : ins[p]) if (!win || a.second > win->second) win = &a;             // (map order: the smaller key keeps a tie)
                if (win && win->second >= t.min_count && win->second * 1000 >= (uint64_t)t.min_permille * cov) {
                    want_rows.push_back(Row{r, (uint32_t)(p - starts[r]), 2u, R, 0u, (uint32_t)win->first.first, win->second, cov, win->first.second});
                    for (char ch : win->first.second) want_letters[r].push_back("ACGT"[ch - '1']);
                    ++n_ins;
                    n_ins_on_del += stands && best == 5;
                }
            }
        // the header's way
        auto read_len = [&](uint64_t i) { return (uint64_t)reads[i].size(); };
        std::vector<flx::PileupJob> jobs;
        if (!flx::pileup_plan(starts, flx::consensus_filter(o), recs.data(), recs.size(), words.data(), words.size(), reads.size(), read_len, "check", jobs)) { printf("case %d: valid records were refused: %s\n", c, flx::last_error.c_str()); return 1; }
        std::vector<uint32_t> counts((size_t)flx::PILEUP_PLANES * total, 0);
        std::vector<flx::SortKey> keys;
        for (auto const& j : jobs) {
            flx::pileup_walk(j, words.data(), reads[j.read_index].data(), reads[j.read_index].size(), counts.data(), total);
            size_t const before = keys.size();
            flx::consensus_job_keys(j, words.data(), reads[j.read_index].data(), reads[j.read_index].size(), keys);
            if (keys.size() - before != flx::consensus_job_slots(j, words.data())) { printf("case %d: a record's keys are not its slots\n", c); return 1; }
        }
        flx::ConsensusResult got;
        if (!flx::consensus_finish_host(starts, text.data(), counts.data(), keys, t, got)) { printf("case %d: the finish refused\n", c); return 1; }
        n_alleles += got.alleles.size();
        if (got.alleles.size() != want_alleles) { printf("case %d: %zu alleles, expected %llu\n", c, got.alleles.size(), (unsigned long long)want_alleles); return 1; }
        for (uint32_t r = 0; r < n_refs; ++r)
            if (got.letters.substr(got.letter_offsets[r], got.letter_offsets[r + 1] - got.letter_offsets[r]) != want_letters[r]) { printf("case %d: the letters of sequence %u differ\n", c, r); return 1; }
        if (got.changes.size() != want_rows.size()) { printf("case %d: %zu changes, expected %zu\n", c, got.changes.size(), want_rows.size()); return 1; }
        for (size_t i = 0; i < want_rows.size(); ++i) {
            flx_consensus_change const& g = got.changes[i];
            Row const& w = want_rows[i];
            std::string s;
            if (g.kind == 2u) for (uint32_t k = 0; k < g.length; ++k) s.push_back((char)('0' + flx::consensus_key_letter(g.letters, k)));
            if ((uint32_t)g.reference_id != w.ref || g.position != w.pos || g.kind != w.kind || g.ref_rank != w.ref_rank || g.alt_rank != w.alt || g.length != w.length || g.count != w.count ||
                g.cov != w.cov || s != w.letters || (g.kind != 2u && g.letters != 0)) { printf("case %d: change %zu differs\n", c, i); return 1; }
        }
    }
    {
        // the key: round trip at every length, the order, the void key
        for (uint32_t len = 0; len <= 34; ++len) {
            std::vector<uint32_t> l(len);
            for (auto& x : l) x = 1 + (uint32_t)(rng() % 4);
            flx::SortKey const k = flx::consensus_key(true, 0xFFFFFFFEull, len, [&](uint32_t i) { return l[i]; });
            if ((len < 1 || len > 32) != flx::consensus_key_is_void(k)) { printf("length %u: void or not\n", len); return 1; }
            if (flx::consensus_key_is_void(k)) continue;
            if (flx::consensus_key_anchor(k) != 0xFFFFFFFEull || flx::consensus_key_length(k) != len) { printf("length %u: anchor or length\n", len); return 1; }
            for (uint32_t i = 0; i < len; ++i) if (flx::consensus_key_letter(k.lo, i) != l[i]) { printf("length %u: letter %u\n", len, i); return 1; }
            if (len < 32 && (k.lo & ((1ull << (64 - 2 * len)) - 1))) { printf("length %u: low bits set\n", len); return 1; }
            if (!flx::consensus_key_is_void(flx::consensus_key(false, 5, len, [&](uint32_t i) { return l[i]; }))) { printf("an event without a column in front yields a key\n"); return 1; }
            l[len - 1] = len % 2 ? 0 : 5;
            if (!flx::consensus_key_is_void(flx::consensus_key(true, 5, len, [&](uint32_t i) { return l[i]; }))) { printf("a letter outside A C G T yields a key\n"); return 1; }
        }
        auto key = [](u64 a, std::vector<uint32_t> l) { return flx::consensus_key(true, a, (uint32_t)l.size(), [&](uint32_t i) { return l[i]; }); };
        if (!flx::sort_key_less(key(7, {4, 4}), key(8, {1})) || !flx::sort_key_less(key(7, {4}), key(7, {1, 1})) || !flx::sort_key_less(key(7, {1, 2}), key(7, {1, 3})) ||
            !flx::sort_key_less(key(7, {1, 4}), key(7, {2, 1})) || !flx::sort_key_less(key(0xFFFFFFFEull, std::vector<uint32_t>(32, 4)), flx::consensus_void_key()))
            { printf("the key order is not (anchor, length, letters)\n"); return 1; }
        flx_consensus_options o{};
        o.min_permille = 1001;
        if (flx::consensus_options_valid(&o)) { printf("a fraction above 1000 permille was accepted\n"); return 1; }
        o.min_permille = 1000; o.reserved[1] = 1;
        if (flx::consensus_options_valid(&o)) { printf("a reserved field was accepted\n"); return 1; }
        flx::ConsensusThresholds const d = flx::consensus_thresholds(flx_consensus_options{});
        if (d.min_depth != 3 || d.min_count != 2 || d.min_permille != 500 || d.mask_low_depth != 0) { printf("the defaults are not 3 / 2 / 500\n"); return 1; }
    }
    if (!n_counted || !n_void_first || !n_void_long || !n_void_letter || !n_alleles || !n_sub || !n_del || !n_ins || !n_ins_on_del || !n_uncalled || !n_tie || !n_n) {
        printf("a class of cases did not occur: %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)n_counted, (unsigned long long)n_void_first,
               (unsigned long long)n_void_long, (unsigned long long)n_void_letter, (unsigned long long)n_alleles, (unsigned long long)n_sub, (unsigned long long)n_del,
               (unsigned long long)n_ins, (unsigned long long)n_ins_on_del, (unsigned long long)n_uncalled, (unsigned long long)n_tie, (unsigned long long)n_n);
        return 1;
    }
    printf("ok %d cases: %llu records counted, %llu alleles; events without a column in front %llu, longer than 32 %llu, with a letter outside A C G T %llu; calls SUB %llu, DEL %llu, INS %llu (%llu on a DEL), uncalled %llu, tied %llu, on N %llu\n",
           n_cases, (unsigned long long)n_counted, (unsigned long long)n_alleles, (unsigned long long)n_void_first, (unsigned long long)n_void_long, (unsigned long long)n_void_letter,
           (unsigned long long)n_sub, (unsigned long long)n_del, (unsigned long long)n_ins, (unsigned long long)n_ins_on_del, (unsigned long long)n_uncalled, (unsigned long long)n_tie,
           (unsigned long long)n_n);
    return 0;
}
