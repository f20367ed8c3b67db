// The variant-calling rule of flx_variants.hpp (one host implementation, shared by flx_variants_host and, in its FLX_HD pieces, by the
// kernels) on random records against a definition that walks every column on its own, keeps every indel as (kind, length, string of
// letters) in an ordered map per anchor with no packed key anywhere, and genotypes every candidate in 128-bit integers. The text, the
// words and every read live in arrays of exactly the needed size, so that a step outside them is an AddressSanitizer report. Then the
// key's order and round trip, the genotype at counts near 2^32 and the refusals of the options.
// Stand-alone, built with ASan + UBSan by tests/test_variants_host.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "../floxer_amd/csrc/flx_variants.hpp"

namespace flx {
static std::string last_error;
void set_error(const std::string& m) { last_error = m; }
}

using flx::u64;
typedef unsigned __int128 u128;

struct Want { uint32_t gt, gq, qual, pl[3]; };
static uint32_t sat(u128 v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }
// the genotype as the rule states it, in 128 bits
static Want genotype(u128 ref_n, u128 alt_n, u128 oth, flx::VariantsModel const& v) {
    u128 const L[3] = {ref_n * v.m + (alt_n + oth) * v.x, (ref_n + alt_n) * v.h + oth * v.x, alt_n * v.m + (ref_n + oth) * v.x};
    u128 const Q[3] = {L[0], L[1] + v.prior_het, L[2] + v.prior_hom};
    std::vector<std::pair<u128, uint32_t>> order = {{Q[0], 0u}, {Q[1], 1u}, {Q[2], 2u}};
    std::sort(order.begin(), order.end());                                                        // (the pair's order: ties go RR, RA, AA)
    Want w;
    w.gt = order[0].second;
    u128 const gq = (order[1].first - order[0].first) / 100;
    w.gq = gq > 99 ? 99u : (uint32_t)gq;
    u128 const alt_q = std::min(Q[1], Q[2]);
    w.qual = Q[0] > alt_q ? sat(Q[0] - alt_q) : 0u;
    u128 const min_l = std::min(L[0], std::min(L[1], L[2]));
    for (int g = 0; g < 3; ++g) w.pl[g] = sat((L[g] - min_l) / 100);
    return w;
}

int main() {
    std::mt19937_64 rng(20261021);
    static const uint32_t ops[5] = {7, 8, 1, 2, 4};
    static const uint32_t flags[7] = {0, 16, 256, 272, 2048, 2064, 4};
    static const uint8_t comp[6] = {0, 4, 3, 2, 1, 5};
    uint64_t n_counted = 0, n_void_first = 0, n_void_long_ins = 0, n_void_long_del = 0, n_void_letter = 0, n_alleles = 0, n_snv = 0, n_del = 0, n_ins = 0, n_het = 0, n_hom = 0,
             n_two_rows = 0, n_shared_anchor = 0, n_low = 0, n_n = 0;
    int const n_cases = 1200;
    for (int c = 0; c < n_cases; ++c) {
        uint32_t const n_refs = 1 + (uint32_t)(rng() % 3);
        std::vector<uint64_t> lens(n_refs), starts;
        for (auto& l : lens) l = 1 + rng() % (c % 3 ? 40 : 6);
        if (!flx::coverage_lengths_valid(lens.data(), n_refs, "check", starts)) { printf("case %d: valid lengths were refused\n", c); return 1; }
        uint64_t const total = starts.back();
        std::vector<uint8_t> text(total);
        for (auto& x : text) x = rng() % 10 == 0 ? (uint8_t)(rng() % 2 ? 0 : 5) : (uint8_t)(1 + rng() % 4);
        flx_variants_options o{};
        o.count_secondary = rng() % 2; o.min_mapq = rng() % 3 ? 0 : 1 + (uint32_t)(rng() % 60);
        o.min_depth = (uint32_t)(rng() % 4); o.min_qual = rng() % 2 ? 0 : 1 + (uint32_t)(rng() % 3000); o.max_del = rng() % 2 ? 0 : 1 + (uint32_t)(rng() % 4);
        if (rng() % 2) { o.cost_match = 1 + (uint32_t)(rng() % 100); o.cost_het = o.cost_match + 1 + (uint32_t)(rng() % 400); o.cost_mismatch = o.cost_het + 1 + (uint32_t)(rng() % 3000); }
        if (rng() % 2) { o.prior_het = 1 + (uint32_t)(rng() % 4000); o.prior_hom = 1 + (uint32_t)(rng() % 4000); }
        if (!flx::variants_options_valid(&o)) { printf("case %d: valid options were refused: %s\n", c, flx::last_error.c_str()); return 1; }
        flx::VariantsModel const v = flx::variants_model(o);
        std::vector<flx_record> recs;
        std::vector<uint32_t> words;
        std::vector<std::vector<uint8_t>> reads;
        // the definition's sums: per position the depth, the deletions, the X letters and the indels behind it
        std::vector<uint64_t> depth(total, 0), del(total, 0);
        std::vector<std::vector<uint64_t>> x_letter(total, std::vector<uint64_t>(6, 0));
        typedef std::tuple<int, size_t, std::string> Allele;                                       // (0 DEL | 1 INS, length, letters) orders as the key does
        std::vector<std::map<Allele, uint64_t>> indels(total);
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
                if (op == 2u && rng() % 4 == 0) l = 1 + (uint32_t)(rng() % 2);                    // short deletions repeat
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
                    n_void_first += !any; n_void_long_del += L > v.max_del;
                    if (any && L <= v.max_del) ++indels.at(p - 1)[Allele{0, L, ""}];
                    for (uint32_t k = 0; k < L; ++k, ++p) ++del.at(p);
                    any = true;
                } else if (op == 1u) {
                    std::string s;
                    bool letters_ok = true;
                    for (uint32_t k = 0; k < L; ++k) { uint8_t const x = seq.at(row + k); letters_ok = letters_ok && x >= 1 && x <= 4; s.push_back((char)('0' + x)); }
                    n_void_first += !any; n_void_long_ins += L > 32; n_void_letter += !letters_ok;
                    if (any && L <= 32 && letters_ok) ++indels.at(p - 1)[Allele{1, s.size(), s}];
                    row += L;
                } else row += L;
            }
        }
        // the definition's call
        struct Row { uint32_t ref, pos, kind, ref_rank, alt, length; uint64_t ref_n, alt_n, cov; Want g; std::string letters; };
        std::vector<Row> want_rows;
        uint64_t want_alleles = 0;
        for (uint32_t r = 0; r < n_refs; ++r)
            for (uint64_t p = starts[r]; p < starts[r + 1]; ++p) {
                want_alleles += indels[p].size();
                uint32_t const R = text[p];
                uint64_t const cov = depth[p] + del[p];
                size_t const before = want_rows.size();
                n_n += R < 1 || R > 4;
                if (R >= 1 && R <= 4) {
                    uint64_t n[5] = {0, x_letter[p][1], x_letter[p][2], x_letter[p][3], x_letter[p][4]};
                    n[R] += depth[p] - n[1] - n[2] - n[3] - n[4];
                    uint32_t alt = 0;
                    for (uint32_t k = 4; k >= 1; --k) if (k != R && (alt == 0 || n[k] >= n[alt])) alt = k;      // (downwards with >=: the smallest rank of the largest)
                    if (n[alt] > 0) {
                        Want const g = genotype(n[R], n[alt], cov - n[R] - n[alt], v);
                        n_low += g.gt != 0 && !(cov >= v.min_depth && g.qual >= v.min_qual);
                        if (g.gt != 0 && cov >= v.min_depth && g.qual >= v.min_qual) { want_rows.push_back(Row{r, (uint32_t)(p - starts[r]), 0u, R, alt, 1u, n[R], n[alt], cov, g, ""}); ++n_snv; }
                    }
                }
                if (!indels[p].empty()) {
                    const std::pair<const Allele, uint64_t>* win = nullptr;
                    uint64_t events = 0;
                    bool has_del = false, has_ins = false;
                    for (auto const& a : indels[p]) {
                        if (!win || a.second > win->second) win = &a;                            // (map order: the smaller key keeps a tie)
                        events += a.second;
                        (std::get<0>(a.first) ? has_ins : has_del) = true;
                    }
                    n_shared_anchor += has_del && has_ins;
                    uint64_t const ref_n = cov > events ? cov - events : 0;
                    Want const g = genotype(ref_n, win->second, events - win->second, v);
                    if (g.gt != 0 && cov >= v.min_depth && g.qual >= v.min_qual) {
                        bool const ins = std::get<0>(win->first) == 1;
                        want_rows.push_back(Row{r, (uint32_t)(p - starts[r]), ins ? 2u : 1u, R, 0u, (uint32_t)std::get<1>(win->first), ref_n, win->second, cov, g, std::get<2>(win->first)});
                        (ins ? n_ins : n_del) += 1;
                    }
                }
                n_two_rows += want_rows.size() - before == 2;
            }
        // the header's way
        auto read_len = [&](uint64_t i) { return (uint64_t)reads[i].size(); };
        std::vector<flx::PileupJob> jobs;
        if (!flx::pileup_plan(starts, flx::variants_filter(o), recs.data(), recs.size(), words.data(), words.size(), reads.size(), read_len, "check", jobs)) { printf("case %d: valid records were refused: %s\n", c, flx::last_error.c_str()); return 1; }
        std::vector<uint32_t> counts((size_t)flx::PILEUP_PLANES * total, 0);
        std::vector<flx::SortKey> keys;
        for (auto const& j : jobs) {
            flx::pileup_walk(j, words.data(), reads[j.read_index].data(), reads[j.read_index].size(), counts.data(), total);
            size_t const before = keys.size();
            flx::variants_job_keys(j, words.data(), reads[j.read_index].data(), reads[j.read_index].size(), v.max_del, keys);
            if (keys.size() - before != flx::variants_job_slots(j, words.data())) { printf("case %d: a record's keys are not its slots\n", c); return 1; }
        }
        flx::VariantsResult got;
        if (!flx::variants_finish_host(starts, text.data(), counts.data(), keys, v, got)) { printf("case %d: the finish refused\n", c); return 1; }
        n_alleles += got.alleles.size();
        if (got.alleles.size() != want_alleles) { printf("case %d: %zu alleles, expected %llu\n", c, got.alleles.size(), (unsigned long long)want_alleles); return 1; }
        if (got.rows.size() != want_rows.size()) { printf("case %d: %zu rows, expected %zu\n", c, got.rows.size(), want_rows.size()); return 1; }
        for (size_t i = 0; i < want_rows.size(); ++i) {
            flx_variant const& g = got.rows[i];
            Row const& w = want_rows[i];
            std::string s;
            if (g.kind == 2u) for (uint32_t k = 0; k < g.length; ++k) s.push_back((char)('0' + flx::consensus_key_letter(g.letters, k)));
            if ((uint32_t)g.reference_id != w.ref || g.position != w.pos || g.kind != w.kind || g.ref_rank != w.ref_rank || g.alt_rank != w.alt || g.length != w.length ||
                g.ref_count != w.ref_n || g.alt_count != w.alt_n || g.cov != w.cov || g.gt != w.g.gt || g.gq != w.g.gq || g.qual != w.g.qual || g.pl[0] != w.g.pl[0] ||
                g.pl[1] != w.g.pl[1] || g.pl[2] != w.g.pl[2] || g.reserved != 0 || s != w.letters || (g.kind != 2u && g.letters != 0)) { printf("case %d: row %zu differs\n", c, i); return 1; }
            (g.gt == 1 ? n_het : n_hom) += 1;
        }
    }
    {
        // the key: the fields' round trip, the order at an anchor, the void key
        auto ins = [](u64 a, std::vector<uint32_t> l) { return flx::variants_key(flx::VARIANTS_KEY_INS, true, a, (uint32_t)l.size(), 50, [&](uint32_t i) { return l[i]; }); };
        auto del = [](u64 a, uint32_t len, uint32_t max_del) { return flx::variants_key(flx::VARIANTS_KEY_DEL, true, a, len, max_del, [](uint32_t) { return 0u; }); };
        for (uint32_t len = 0; len <= 34; ++len) {
            std::vector<uint32_t> l(len);
            for (auto& x : l) x = 1 + (uint32_t)(rng() % 4);
            flx::SortKey const k = ins(0xFFFFFFFEull, l);
            if ((len < 1 || len > 32) != flx::consensus_key_is_void(k)) { printf("insertion of %u: void or not\n", len); return 1; }
            if (flx::consensus_key_is_void(k)) continue;
            if (flx::variants_key_anchor(k) != 0xFFFFFFFEull || flx::variants_key_length(k) != len || flx::variants_key_kind(k) != flx::VARIANTS_KEY_INS) { printf("insertion of %u: the key's fields\n", len); return 1; }
            for (uint32_t i = 0; i < len; ++i) if (flx::consensus_key_letter(k.lo, i) != l[i]) { printf("insertion of %u: letter %u\n", len, i); return 1; }
            l[len - 1] = len % 2 ? 0 : 5;
            if (!flx::consensus_key_is_void(ins(5, l))) { printf("a letter outside A C G T yields a key\n"); return 1; }
        }
        uint32_t const longest = flx::VARIANTS_MAX_LEN;
        for (uint32_t max_del : {1u, 50u, longest})
            for (uint32_t len : {0u, 1u, max_del - 1, max_del, max_del + 1}) {
                if (len > longest) continue;
                flx::SortKey const k = del(0xFFFFFFFEull, len, max_del);
                if ((len < 1 || len > max_del) != flx::consensus_key_is_void(k)) { printf("deletion of %u under %u: void or not\n", len, max_del); return 1; }
                if (!flx::consensus_key_is_void(k) && (flx::variants_key_anchor(k) != 0xFFFFFFFEull || flx::variants_key_length(k) != len || flx::variants_key_kind(k) != flx::VARIANTS_KEY_DEL || k.lo != 0))
                    { printf("deletion of %u: the key's fields\n", len); return 1; }
            }
        if (!flx::consensus_key_is_void(flx::variants_key(flx::VARIANTS_KEY_DEL, false, 5, 1, 50, [](uint32_t) { return 0u; })) ||
            !flx::consensus_key_is_void(flx::variants_key(flx::VARIANTS_KEY_INS, false, 5, 1, 50, [](uint32_t) { return 1u; })))
            { printf("an event without a column in front yields a key\n"); return 1; }
        if (!flx::sort_key_less(del(7, 50, 50), ins(7, {1})) || !flx::sort_key_less(del(7, 1, 50), del(7, 2, 50)) || !flx::sort_key_less(ins(7, {4}), ins(7, {1, 1})) ||
            !flx::sort_key_less(ins(7, {1, 2}), ins(7, {1, 3})) || !flx::sort_key_less(ins(7, std::vector<uint32_t>(32, 4)), del(8, 1, 50)) ||
            !flx::sort_key_less(ins(0xFFFFFFFEull, std::vector<uint32_t>(32, 4)), flx::consensus_void_key()) || !flx::sort_key_less(del(0xFFFFFFFFull, longest, longest), flx::consensus_void_key()))
            { printf("the key order is not (anchor, deletions first, length, letters), the void key last\n"); return 1; }
    }
    {
        // the genotype at counts near 2^32 and with the largest costs: the header's 64 bits against 128, and the saturation
        flx_variants_options big{};
        big.cost_match = 1; big.cost_het = (1u << 20) - 1; big.cost_mismatch = 1u << 20; big.prior_het = 1u << 20; big.prior_hom = 1u << 20;
        if (!flx::variants_options_valid(&big)) { printf("the largest costs were refused\n"); return 1; }
        uint64_t const near[6] = {0, 1, 0xFFFFFFFEull, 0xFFFFFFFFull, 0x100000000ull, 0x1FFFFFFFEull};
        uint64_t n_sat = 0;
        for (auto const* o : {(const flx_variants_options*)nullptr, (const flx_variants_options*)&big}) {
            flx::VariantsModel const v = flx::variants_model(flx::variants_options_or_default(o));
            for (uint64_t a : near) for (uint64_t b : near) for (uint64_t x : near) {
                flx::VariantGenotype const g = flx::variants_genotype(a, b, x, v);
                Want const w = genotype(a, b, x, v);
                if (g.gt != w.gt || g.gq != w.gq || g.qual != w.qual || g.pl[0] != w.pl[0] || g.pl[1] != w.pl[1] || g.pl[2] != w.pl[2]) { printf("the genotype of %llu %llu %llu differs\n", (unsigned long long)a, (unsigned long long)b, (unsigned long long)x); return 1; }
                n_sat += g.qual == 0xFFFFFFFFu || g.pl[0] == 0xFFFFFFFFu;
            }
        }
        if (!n_sat) { printf("nothing saturated\n"); return 1; }
        flx_variants_options o{};
        o.reserved[1] = 1;
        if (flx::variants_options_valid(&o)) { printf("a reserved field was accepted\n"); return 1; }
        o = flx_variants_options{}; o.cost_het = 1574;
        if (flx::variants_options_valid(&o)) { printf("cost_het = cost_mismatch was accepted\n"); return 1; }
        o = flx_variants_options{}; o.cost_match = 325;
        if (flx::variants_options_valid(&o)) { printf("cost_match = cost_het was accepted\n"); return 1; }
        o = flx_variants_options{}; o.max_del = 1u << 28;
        if (flx::variants_options_valid(&o)) { printf("max_del = 2^28 was accepted\n"); return 1; }
        o = flx_variants_options{}; o.prior_hom = (1u << 20) + 1;
        if (flx::variants_options_valid(&o)) { printf("a cost above 2^20 was accepted\n"); return 1; }
        flx::VariantsModel const d = flx::variants_model(flx_variants_options{});
        if (d.min_depth != 4 || d.min_qual != 2000 || d.max_del != 50 || d.m != 36 || d.x != 1574 || d.h != 325 || d.prior_het != 3000 || d.prior_hom != 3301) { printf("the defaults are not 4 / 2000 / 50 and 36 / 1574 / 325 / 3000 / 3301\n"); return 1; }
    }
    uint64_t const classes[15] = {n_counted, n_void_first, n_void_long_ins, n_void_long_del, n_void_letter, n_alleles, n_snv, n_del, n_ins, n_het, n_hom, n_two_rows, n_shared_anchor, n_low, n_n};
    bool all = true;
    for (uint64_t x : classes) all = all && x > 0;
    if (!all) {
        printf("a class of cases did not occur:");
        for (uint64_t x : classes) printf(" %llu", (unsigned long long)x);
        printf("\n");
        return 1;
    }
    printf("ok %d cases: %llu records counted, %llu alleles; events without a column in front %llu, insertions longer than 32 %llu, deletions longer than max_del %llu, with a letter outside A C G T %llu; rows SNV %llu, DEL %llu, INS %llu, 0/1 %llu, 1/1 %llu; positions with two rows %llu, anchors with both kinds %llu, candidates below the thresholds %llu, positions on N %llu\n",
           n_cases, (unsigned long long)n_counted, (unsigned long long)n_alleles, (unsigned long long)n_void_first, (unsigned long long)n_void_long_ins, (unsigned long long)n_void_long_del,
           (unsigned long long)n_void_letter, (unsigned long long)n_snv, (unsigned long long)n_del, (unsigned long long)n_ins, (unsigned long long)n_het, (unsigned long long)n_hom,
           (unsigned long long)n_two_rows, (unsigned long long)n_shared_anchor, (unsigned long long)n_low, (unsigned long long)n_n);
    return 0;
}
