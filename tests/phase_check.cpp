// The phasing rule of flx_phase.hpp (one host implementation, shared by flx_phase_host and, in its FLX_HD pieces, by the kernels) on
// random records against a definition that walks every column on its own: every column keeps its op, its letter and the insertions
// and deletions directly behind it as (kind, length, string of letters), with no packed key and no binary search anywhere; links,
// chain, tags and votes follow the rule's text over maps. The text, the words and every read live in arrays of exactly the needed
// size, so that a step outside them is an AddressSanitizer report. Then the refusals of the options and of the sites.
// Stand-alone, built with ASan + UBSan by tests/test_phase_host.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "../floxer_amd/csrc/flx_phase.hpp"

namespace flx {
static std::string last_error;
void set_error(const std::string& m) { last_error = m; }
}

typedef std::tuple<int, uint32_t, std::string> Event;                      // (1 DEL | 2 INS, length, letters), "" for a deletion; kind -1: no allele
struct Column { uint32_t op; uint8_t letter; std::vector<Event> behind; };

int main() {
    std::mt19937_64 rng(20261021);
    static const uint32_t ops[5] = {7, 8, 1, 2, 4};
    static const uint32_t flags[7] = {0, 16, 256, 272, 2048, 2064, 4};
    static const uint8_t comp[6] = {0, 4, 3, 2, 1, 5};
    uint64_t n_counted = 0, n_obs[3] = {0, 0, 0}, n_kind[3] = {0, 0, 0}, n_phased = 0, n_hap[3] = {0, 0, 0}, n_flipped = 0, n_sets_of_many = 0, n_shared_anchor = 0;
    int const n_cases = 800;
    for (int c = 0; c < n_cases; ++c) {
        uint32_t const n_refs = 1 + (uint32_t)(rng() % 3);
        std::vector<uint64_t> lens(n_refs), starts;
        for (auto& l : lens) l = 2 + rng() % (c % 3 ? 40 : 8);
        if (!flx::coverage_lengths_valid(lens.data(), n_refs, "check", starts)) { printf("case %d: valid lengths were refused\n", c); return 1; }
        uint64_t const total = starts.back();
        std::vector<uint8_t> text(total);
        for (auto& x : text) x = rng() % 10 == 0 ? (uint8_t)(rng() % 2 ? 0 : 5) : (uint8_t)(1 + rng() % 4);
        flx_phase_options o{};
        o.count_secondary = rng() % 2; o.min_mapq = rng() % 3 ? 0 : 1 + (uint32_t)(rng() % 60);
        o.min_link = (uint32_t)(rng() % 4); o.min_margin = (uint32_t)(rng() % 3); o.refine_rounds = (uint32_t)(rng() % 4); o.skip_refine = rng() % 4 == 0;
        if (!flx::phase_options_valid(&o)) { printf("case %d: valid options were refused: %s\n", c, flx::last_error.c_str()); return 1; }
        flx::PhaseModel const m = flx::phase_model(o);
        uint32_t const want_link = o.min_link ? o.min_link : 2, want_margin = o.min_margin ? o.min_margin : 1, want_rounds = o.skip_refine ? 0 : o.refine_rounds ? o.refine_rounds : 1;
        if (m.min_link != want_link || m.min_margin != want_margin || m.rounds != want_rounds) { printf("case %d: the model's defaults differ\n", c); return 1; }
        std::vector<flx_record> recs;
        std::vector<uint32_t> words;
        std::vector<std::vector<uint8_t>> reads;
        // the definition's view: per counted record its first position and its columns; and the alleles seen, as candidates for sites
        std::vector<uint64_t> origin;
        std::vector<std::vector<Column>> columns;
        std::map<std::tuple<uint64_t, int, uint32_t, std::string>, int> seen;   // (anchor, kind 0 SNV | 1 DEL | 2 INS, length or alt, letters)
        std::vector<std::vector<uint8_t>> shared;
        for (int k = 0; k < 3; ++k) { std::vector<uint8_t> s(1 + rng() % (rng() % 5 ? 3 : 34)); for (auto& x : s) x = rng() % 30 ? (uint8_t)(1 + rng() % 4) : (uint8_t)(rng() % 2 ? 0 : 5); shared.push_back(s); }
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
                if (op == 2u && rng() % 4 == 0) l = 1 + (uint32_t)(rng() % 2);
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
            // the columns, one by one; an I or D word joins the events of every column whose run of I and D words it continues
            std::vector<Column> cols;
            std::vector<size_t> open;
            uint64_t p = s0 + (uint64_t)rec.position, row = 0;
            for (uint32_t wd : w) {
                uint32_t const op = wd & 15u, L = wd >> 4;
                if (op == 1u || op == 2u) {
                    Event e{-1, L, ""};
                    if (op == 2u) e = Event{1, L, ""};
                    else if (L <= 32) {
                        std::string s;
                        bool ok = true;
                        for (uint32_t k = 0; k < L; ++k) { uint8_t const x = seq.at(row + k); ok = ok && x >= 1 && x <= 4; s.push_back((char)('0' + x)); }
                        if (ok) e = Event{2, L, s};
                    }
                    // (the event's own anchor is the column in front of it: only the last open column can match it)
                    for (size_t q = 0; q < open.size(); ++q) cols.at(open[q]).behind.push_back(q + 1 == open.size() ? e : Event{-1, L, ""});
                    if (!cols.empty() && std::get<0>(e) >= 0) ++seen[std::make_tuple(p - 1, std::get<0>(e), L, std::get<2>(e))];
                } else open.clear();
                if (op == 7u || op == 8u || op == 2u) {
                    for (uint32_t k = 0; k < L; ++k) {
                        uint8_t const letter = op == 2u ? (uint8_t)0 : seq.at(row + k);
                        if (op == 8u && letter >= 1 && letter <= 4 && text.at(p + k) >= 1 && text.at(p + k) <= 4 && letter != text.at(p + k)) ++seen[std::make_tuple(p + k, 0, (uint32_t)letter, "")];
                        cols.push_back(Column{op, letter, {}});
                    }
                    open.push_back(cols.size() - 1);
                    p += L;
                }
                if (op == 7u || op == 8u || op == 1u || op == 4u) row += L;
            }
            origin.push_back(s0 + (uint64_t)rec.position);
            columns.push_back(cols);
        }
        // the sites: about half of the alleles seen, one SNV per position; in (anchor, kind) order as the map has them
        std::vector<flx_phase_site> sites;
        std::vector<Event> site_event;                                                            // an indel site as the definition holds it
        std::vector<uint64_t> site_anchor;
        for (auto const& kv : seen) {
            uint64_t const a = std::get<0>(kv.first);
            int const kind = std::get<1>(kv.first);
            if (rng() % 2) continue;
            if (!sites.empty() && site_anchor.back() == a && (int)sites.back().kind == kind) continue;      // one site per (anchor, kind)
            uint32_t ref = 0;
            while (starts[ref + 1] <= a) ++ref;
            flx_phase_site s{};
            s.reference_id = (int32_t)ref; s.position = (uint32_t)(a - starts[ref]); s.kind = (uint32_t)kind;
            if (kind == 0) { s.alt_rank = std::get<2>(kv.first); s.length = 1; }
            else {
                s.length = std::get<2>(kv.first);
                if (kind == 1 && (uint64_t)s.position + s.length >= lens[ref]) continue;          // (cannot be: the records end inside their sequence)
                std::string const& letters = std::get<3>(kv.first);
                for (size_t k = 0; k < letters.size(); ++k) s.letters |= (uint64_t)(letters[k] - '1') << (62 - 2 * k);
            }
            n_shared_anchor += !sites.empty() && site_anchor.back() == a;
            sites.push_back(s);
            site_anchor.push_back(a);
            site_event.push_back(kind == 0 ? Event{0, s.alt_rank, ""} : Event{kind, s.length, std::get<3>(kv.first)});
            ++n_kind[kind];
        }
        size_t const n = sites.size();
        // ---- the header's form
        std::vector<flx::u32> anchors;
        if (flx::phase_sites_valid(starts, [&](uint64_t r, uint64_t p) { return (uint32_t)text.at(starts[r] + p); }, sites.data(), n, "check", anchors) != FLX_OK) {
            printf("case %d: valid sites were refused: %s\n", c, flx::last_error.c_str());
            return 1;
        }
        std::vector<flx::PileupJob> jobs;
        if (!flx::pileup_plan(starts, flx::phase_filter(o), recs.data(), recs.size(), words.data(), words.size(), reads.size(), [&](uint64_t r) { return reads[r].size(); }, "check", jobs)) {
            printf("case %d: valid records were refused: %s\n", c, flx::last_error.c_str());
            return 1;
        }
        if (jobs.size() != columns.size()) { printf("case %d: %zu jobs, %zu counted records\n", c, jobs.size(), columns.size()); return 1; }
        std::vector<flx::PhaseRecord> precs(jobs.size());
        uint64_t n_slots = 0;
        for (size_t j = 0; j < jobs.size(); ++j) {
            precs[j].text_end = flx::phase_job_end(jobs[j], words.data());
            flx::phase_slots(anchors, jobs[j].text_off, precs[j].text_end, precs[j].first, precs[j].n_slots);
            precs[j].obs_off = n_slots; precs[j].add = 0; precs[j].read = (uint32_t)jobs[j].read_index;
            n_slots += precs[j].n_slots;
        }
        std::vector<uint8_t> obs(n_slots, 9);                                                     // (exactly the slots: every one must be written)
        for (size_t j = 0; j < jobs.size(); ++j)
            flx::phase_job_observe(jobs[j], precs[j], words.data(), reads[jobs[j].read_index].data(), reads[jobs[j].read_index].size(), anchors.data(), sites.data(), obs.data());
        std::vector<flx_phase_result> got(n);
        std::vector<flx_phase_tag> got_tags(jobs.size());
        flx::phase_finish_host(sites.data(), n, precs, obs.data(), m, got.data(), got_tags.data());
        // ---- the definition
        std::vector<std::map<size_t, uint32_t>> mine(columns.size());                             // per record: site -> observation
        for (size_t j = 0; j < columns.size(); ++j) {
            uint64_t const end = origin[j] + columns[j].size();
            for (size_t i = 0; i < n; ++i) {
                if (site_anchor[i] < origin[j] || site_anchor[i] >= end) continue;
                Column const& col = columns[j].at(site_anchor[i] - origin[j]);
                uint32_t ob = 2;
                if (sites[i].kind == 0) ob = col.op == 7u ? 0u : col.op == 8u && col.letter == sites[i].alt_rank ? 1u : 2u;
                else if (std::find(col.behind.begin(), col.behind.end(), site_event[i]) != col.behind.end()) ob = 1;
                else if (col.behind.empty() && (col.op == 7u || col.op == 8u) && site_anchor[i] + 1 < end) ob = 0;
                mine[j][i] = ob;
                ++n_obs[ob];
            }
            if (mine[j].size() != precs[j].n_slots) { printf("case %d record %zu: %u slots, want %zu\n", c, j, precs[j].n_slots, mine[j].size()); return 1; }
            size_t k = 0;
            for (auto const& kv : mine[j]) {
                if (kv.first != precs[j].first + k || obs.at(precs[j].obs_off + k) != kv.second) {
                    printf("case %d record %zu slot %zu: site %u observation %u, want site %zu observation %u\n", c, j, k, precs[j].first + (uint32_t)k, obs.at(precs[j].obs_off + k), kv.first, kv.second);
                    return 1;
                }
                ++k;
            }
        }
        std::vector<uint64_t> cis(n, 0), trans(n, 0), keep(n, 0), swap(n, 0);
        for (auto const& rec : mine)
            for (auto const& kv : rec) {
                auto const next = rec.find(kv.first + 1);
                if (next == rec.end() || kv.second > 1 || next->second > 1) continue;
                ++(kv.second == next->second ? cis : trans)[kv.first];
            }
        std::vector<size_t> set(n);
        std::vector<uint32_t> p(n, 0);
        std::map<size_t, size_t> size;
        for (size_t i = 0; i < n; ++i) {
            uint64_t const d = i ? (cis[i - 1] > trans[i - 1] ? cis[i - 1] - trans[i - 1] : trans[i - 1] - cis[i - 1]) : 0;
            bool const joined = i > 0 && sites[i].reference_id == sites[i - 1].reference_id && d >= want_link;
            set[i] = joined ? set[i - 1] : i;
            if (joined) p[i] = p[i - 1] ^ (trans[i - 1] > cis[i - 1] ? 1u : 0u);
            ++size[set[i]];
        }
        struct Tag { uint32_t hap; size_t set; uint32_t h1, h2; };
        std::vector<Tag> tags(mine.size());
        auto tag_all = [&]() {
            for (size_t j = 0; j < mine.size(); ++j) {
                std::map<size_t, std::tuple<uint32_t, uint32_t, uint32_t>> runs;                  // set -> (observations, h1, h2)
                for (auto const& kv : mine[j]) {
                    if (size[set[kv.first]] < 2 || kv.second > 1) continue;
                    auto& r = runs[set[kv.first]];
                    ++std::get<0>(r);
                    if ((kv.second ^ p[kv.first]) == 1u) ++std::get<1>(r); else ++std::get<2>(r);
                }
                Tag t{0, (size_t)flx::PHASE_NO_SET, 0, 0};
                uint32_t best = 0;
                for (auto const& kv : runs) if (std::get<0>(kv.second) > best) { best = std::get<0>(kv.second); t.set = kv.first; t.h1 = std::get<1>(kv.second); t.h2 = std::get<2>(kv.second); }
                if ((int64_t)t.h1 - (int64_t)t.h2 >= (int64_t)want_margin) t.hap = 1;
                else if ((int64_t)t.h2 - (int64_t)t.h1 >= (int64_t)want_margin) t.hap = 2;
                tags[j] = t;
            }
        };
        tag_all();
        for (uint32_t round = 0; round < want_rounds; ++round) {
            std::fill(keep.begin(), keep.end(), 0);
            std::fill(swap.begin(), swap.end(), 0);
            for (size_t j = 0; j < mine.size(); ++j)
                for (auto const& kv : mine[j]) {
                    if (!tags[j].hap || size[set[kv.first]] < 2 || set[kv.first] != tags[j].set || kv.second > 1) continue;
                    ++((kv.second ^ p[kv.first]) == (tags[j].hap == 1 ? 1u : 0u) ? keep : swap)[kv.first];
                }
            for (size_t i = 0; i < n; ++i) if (swap[i] > keep[i]) { p[i] ^= 1u; ++n_flipped; }
            tag_all();
        }
        for (size_t i = 0; i < n; ++i) {
            flx_phase_result const& g = got[i];
            bool const phased = size[set[i]] > 1;
            n_phased += phased;
            n_sets_of_many += phased && set[i] == i;
            if (g.phase_set != set[i] || (g.phased != 0) != phased || g.phase != p[i] || g.cis != cis[i] || g.trans != trans[i] || g.keep != keep[i] || g.swap != swap[i] || g.reserved) {
                printf("case %d site %zu: set %u phased %u phase %u cis %u trans %u keep %u swap %u, want %zu %d %u %llu %llu %llu %llu\n", c, i, g.phase_set, g.phased, g.phase, g.cis, g.trans,
                       g.keep, g.swap, set[i], (int)phased, p[i], (unsigned long long)cis[i], (unsigned long long)trans[i], (unsigned long long)keep[i], (unsigned long long)swap[i]);
                return 1;
            }
        }
        for (size_t j = 0; j < mine.size(); ++j) {
            flx_phase_tag const& g = got_tags[j];
            ++n_hap[tags[j].hap];
            if (g.hap != tags[j].hap || g.phase_set != (uint32_t)tags[j].set || g.h1 != tags[j].h1 || g.h2 != tags[j].h2 || g.n_slots != mine[j].size() || g.add != 0 ||
                g.read != (uint32_t)jobs[j].read_index || g.reserved) {
                printf("case %d record %zu: hap %u set %u h1 %u h2 %u slots %u, want %u %zu %u %u %zu\n", c, j, g.hap, g.phase_set, g.h1, g.h2, g.n_slots, tags[j].hap, tags[j].set, tags[j].h1,
                       tags[j].h2, mine[j].size());
                return 1;
            }
        }
    }
    // the cases must have reached every branch of the rule
    if (!n_obs[0] || !n_obs[1] || !n_obs[2] || !n_kind[0] || !n_kind[1] || !n_kind[2] || !n_phased || !n_hap[0] || !n_hap[1] || !n_hap[2] || !n_flipped || !n_sets_of_many || !n_shared_anchor) {
        printf("a branch was never reached: obs %llu %llu %llu kinds %llu %llu %llu phased %llu hap %llu %llu %llu flipped %llu sets %llu shared %llu\n", (unsigned long long)n_obs[0],
               (unsigned long long)n_obs[1], (unsigned long long)n_obs[2], (unsigned long long)n_kind[0], (unsigned long long)n_kind[1], (unsigned long long)n_kind[2], (unsigned long long)n_phased,
               (unsigned long long)n_hap[0], (unsigned long long)n_hap[1], (unsigned long long)n_hap[2], (unsigned long long)n_flipped, (unsigned long long)n_sets_of_many,
               (unsigned long long)n_shared_anchor);
        return 1;
    }
    // the refusals of the options and of the sites
    {
        flx_phase_options o{};
        o.reserved[0] = 1;
        if (flx::phase_options_valid(&o)) { printf("a reserved option field was accepted\n"); return 1; }
        o = flx_phase_options{};
        o.refine_rounds = 9;
        if (flx::phase_options_valid(&o)) { printf("nine rounds were accepted\n"); return 1; }
        o.refine_rounds = 8;
        if (!flx::phase_options_valid(&o) || !flx::phase_options_valid(nullptr)) { printf("valid options were refused\n"); return 1; }
        std::vector<uint64_t> const starts = {0, 10, 20};
        std::vector<uint8_t> const text = {1, 2, 3, 4, 1, 2, 3, 4, 0, 5, 1, 2, 3, 4, 1, 2, 3, 4, 1, 2};
        auto rank = [&](uint64_t r, uint64_t p) { return (uint32_t)text.at(starts[r] + p); };
        std::vector<flx::u32> anchors;
        auto site = [](int32_t ref, uint32_t pos, uint32_t kind, uint32_t alt, uint32_t len, uint64_t letters) { flx_phase_site s{}; s.reference_id = ref; s.position = pos; s.kind = kind; s.alt_rank = alt; s.length = len; s.letters = letters; return s; };
        std::vector<std::vector<flx_phase_site>> const bad = {
            {site(0, 0, 0, 1, 1, 0)}, {site(0, 0, 0, 0, 1, 0)}, {site(0, 0, 0, 5, 1, 0)}, {site(0, 8, 0, 1, 1, 0)}, {site(0, 9, 0, 1, 1, 0)}, {site(0, 10, 0, 1, 1, 0)}, {site(2, 0, 0, 2, 1, 0)},
            {site(-1, 0, 0, 2, 1, 0)}, {site(0, 0, 3, 2, 1, 0)}, {site(0, 0, 0, 2, 1, 1)}, {site(0, 7, 1, 0, 3, 0)}, {site(0, 0, 1, 0, 0, 0)}, {site(0, 0, 1, 0, 1, 1)}, {site(0, 0, 2, 0, 0, 0)},
            {site(0, 0, 2, 0, 33, 0)}, {site(0, 0, 2, 0, 1, 1ull << 60)}, {site(0, 1, 0, 1, 1, 0), site(0, 0, 0, 2, 1, 0)}, {site(0, 0, 0, 2, 1, 0), site(0, 0, 0, 2, 1, 0)},
            {site(0, 0, 1, 0, 1, 0), site(0, 0, 0, 2, 1, 0)}, {site(1, 0, 0, 2, 1, 0), site(0, 0, 0, 2, 1, 0)}};
        for (size_t k = 0; k < bad.size(); ++k)
            if (flx::phase_sites_valid(starts, rank, bad[k].data(), bad[k].size(), "check", anchors) != FLX_ERR_INVALID) { printf("bad sites %zu were accepted\n", k); return 1; }
        flx_phase_site reserved = site(0, 0, 0, 2, 1, 0);
        reserved.reserved = 1;
        if (flx::phase_sites_valid(starts, rank, &reserved, 1, "check", anchors) != FLX_ERR_INVALID) { printf("a reserved site field was accepted\n"); return 1; }
        if (flx::phase_sites_valid(starts, rank, &reserved, flx::PHASE_MAX_SITES + 1, "check", anchors) != FLX_ERR_CAPACITY) { printf("2^32 - 1 sites were accepted\n"); return 1; }
        std::vector<flx_phase_site> const good = {site(0, 0, 0, 2, 1, 0), site(0, 0, 1, 0, 9, 0), site(0, 0, 2, 0, 32, ~0ull), site(0, 8, 2, 0, 1, 3ull << 62), site(1, 0, 0, 2, 1, 0), site(1, 7, 1, 0, 2, 0)};
        if (flx::phase_sites_valid(starts, rank, good.data(), good.size(), "check", anchors) != FLX_OK || anchors != std::vector<flx::u32>{0, 0, 0, 8, 10, 17}) {
            printf("valid sites were refused: %s\n", flx::last_error.c_str());
            return 1;
        }
    }
    printf("ok %d cases, %llu counted records, observations %llu %llu %llu, sites %llu %llu %llu, phased %llu in %llu sets, haps %llu %llu %llu, flips %llu\n", n_cases,
           (unsigned long long)n_counted, (unsigned long long)n_obs[0], (unsigned long long)n_obs[1], (unsigned long long)n_obs[2], (unsigned long long)n_kind[0], (unsigned long long)n_kind[1],
           (unsigned long long)n_kind[2], (unsigned long long)n_phased, (unsigned long long)n_sets_of_many, (unsigned long long)n_hap[0], (unsigned long long)n_hap[1], (unsigned long long)n_hap[2],
           (unsigned long long)n_flipped);
    return 0;
}
