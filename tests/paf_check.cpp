// The PAF rule of flx_paf.hpp (one host implementation, shared by flx_paf_summarize_host, the checks in front of every launch and the
// writer) on random records against a definition that spells every record out column by column, in arrays of exactly the needed size, so
// that a step outside them is an AddressSanitizer report; then every refusal of its own on one bad record behind good ones, and the
// divergence's rounding. Stand-alone, built with ASan + UBSan by tests/test_paf_host.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../floxer_amd/csrc/flx_paf.hpp"

namespace flx {
static std::string last_error;
void set_error(const std::string& m) { last_error = m; }
}

namespace {

// the record as one letter per column: S = X I D
std::string columns(std::vector<uint32_t> const& w) {
    static const char ops[] = "MIDNSHP=X";
    std::string s;
    for (uint32_t x : w) s.append(x >> 4, ops[x & 15u]);
    return s;
}

flx_paf_summary by_columns(std::string const& c, uint32_t flag, int32_t position) {
    uint64_t lead = 0, trail = 0, eq = 0, x = 0, ins = 0, del = 0, gaps = 0;
    while (lead < c.size() && c[lead] == 'S') ++lead;
    while (trail < c.size() - lead && c[c.size() - 1 - trail] == 'S') ++trail;
    for (size_t i = 0; i < c.size(); ++i) {
        if (c[i] == '=') ++eq;
        if (c[i] == 'X') ++x;
        if (c[i] == 'I') ++ins;
        if (c[i] == 'D') ++del;
        if ((c[i] == 'I' || c[i] == 'D') && (i == 0 || c[i - 1] != c[i])) ++gaps;
    }
    uint64_t const read_len = lead + eq + x + ins + trail;
    flx_paf_summary s;
    s.query_start = (uint32_t)((flag & 16u) ? trail : lead);
    s.query_end = (uint32_t)(read_len - ((flag & 16u) ? lead : trail));
    s.ref_end = (uint32_t)((uint64_t)position + eq + x + del);
    s.matches = (uint32_t)eq; s.mismatches = (uint32_t)x; s.ins_bases = (uint32_t)ins; s.del_bases = (uint32_t)del; s.gap_opens = (uint32_t)gaps;
    return s;
}

struct Batch {
    std::vector<flx_record> recs;
    std::vector<uint32_t> words;
    std::vector<uint64_t> offsets{0};
    void add(uint32_t flag, int32_t ref, int32_t pos, std::vector<uint32_t> const& w, int64_t read_len = -1) {
        flx_record r{};
        r.flag = flag; r.reference_id = ref; r.position = pos; r.read_index = recs.size();
        r.cigar_offset = words.size(); r.cigar_length = (uint32_t)w.size();
        words.insert(words.end(), w.begin(), w.end());
        uint64_t rows = 0;
        for (uint32_t x : w) { uint32_t const op = x & 15u; if (op == 7 || op == 8 || op == 1 || op == 4) rows += x >> 4; }
        offsets.push_back(offsets.back() + (read_len < 0 ? rows : (uint64_t)read_len));
        recs.push_back(r);
    }
};

uint32_t W(char op, uint32_t len) { return (len << 4) | (uint32_t)(strchr("MIDNSHP=X", op) - "MIDNSHP=X"); }

}  // namespace

int main() {
    std::mt19937_64 rng(20241019);
    static const uint32_t flags[7] = {0, 16, 256, 272, 2048, 2064, 4};
    static const char inner[4] = {'=', 'X', 'I', 'D'};
    uint64_t n_mapped = 0, n_unmapped = 0, n_clipped_both = 0, n_same_neighbours = 0;
    int const n_cases = 2000;
    for (int c = 0; c < n_cases; ++c) {
        uint32_t const n_refs = 1 + (uint32_t)(rng() % 5);
        std::vector<uint64_t> lens(n_refs);
        for (auto& l : lens) l = 1 + rng() % 400;
        Batch b;
        std::vector<flx_paf_summary> want;
        for (int r = 0; r < 30; ++r) {
            uint32_t const flag = flags[rng() % 7];
            if (flag == 4) { b.add(4, -1, 0, {}, (int64_t)(rng() % 50)); want.push_back(flx_paf_summary{}); ++n_unmapped; continue; }
            int32_t const ref = (int32_t)(rng() % n_refs);
            uint64_t const len = lens[(size_t)ref];
            std::vector<uint32_t> w;
            uint64_t span = 0;
            uint32_t const T = 1 + (uint32_t)(rng() % 12);
            for (uint32_t t = 0; t < T; ++t) {
                char const op = inner[rng() % 4];
                uint32_t const l = 1 + (uint32_t)(rng() % 30);
                bool const consumes = op != 'I';
                if (consumes && span + l > len) continue;
                if (consumes) span += l;
                if (!w.empty() && (w.back() & 15u) == (W(op, l) & 15u)) ++n_same_neighbours;
                w.push_back(W(op, l));
            }
            if (span == 0) { w.push_back(W('=', 1)); span = 1; }           // (every sequence has a symbol)
            bool const lead = rng() % 2, trail = rng() % 2;
            if (lead) w.insert(w.begin(), W('S', 1 + (uint32_t)(rng() % 40)));
            if (trail) w.push_back(W('S', 1 + (uint32_t)(rng() % 40)));
            n_clipped_both += lead && trail;
            int32_t const pos = (int32_t)(rng() % 4 == 0 ? len - span : rng() % (len - span + 1));
            b.add(flag, ref, pos, w);
            want.push_back(by_columns(columns(w), flag, pos));
            ++n_mapped;
        }
        std::vector<flx_paf_summary> got(b.recs.size());
        if (!flx::paf_plan(b.recs.data(), 0, b.recs.size(), b.words.data(), b.words.size(), b.offsets.data(), b.recs.size(), lens.data(), n_refs, "check", got.data())) {
            printf("case %d: valid records were refused: %s\n", c, flx::last_error.c_str());
            return 1;
        }
        for (size_t i = 0; i < got.size(); ++i)
            if (memcmp(&got[i], &want[i], sizeof(flx_paf_summary)) != 0) { printf("case %d: record %zu differs from its columns\n", c, i); return 1; }
    }
    if (!n_unmapped || !n_clipped_both || !n_same_neighbours) { printf("the random records miss a kind\n"); return 1; }

    // every refusal: one bad record behind two good ones; `out` of the bad record stays as it was
    uint64_t const lens[2] = {100, 1ull << 30};
    int n_refusals = 0;
    auto refused = [&](const char* what, const char* match, uint32_t flag, int32_t ref, int32_t pos, std::vector<uint32_t> const& w, int64_t read_len = -1, uint64_t read_index_shift = 0,
                       uint64_t words_cut = 0) {
        Batch b;
        b.add(0, 0, 10, {W('S', 3), W('=', 20), W('I', 2), W('=', 5), W('S', 4)});
        b.add(16, 1, 0, {W('D', 4), W('X', 9)});
        b.add(flag, ref, pos, w, read_len);
        b.recs.back().read_index += read_index_shift;
        std::vector<flx_paf_summary> got(3);
        memset(got.data(), 0x5A, got.size() * sizeof(flx_paf_summary));
        bool const ok = flx::paf_plan(b.recs.data(), 0, 3, b.words.data(), b.words.size() - words_cut, b.offsets.data(), 3, lens, 2, "check", got.data());
        flx_paf_summary untouched;
        memset(&untouched, 0x5A, sizeof(untouched));
        if (ok || flx::last_error.find(match) == std::string::npos || memcmp(&got[2], &untouched, sizeof(untouched)) != 0) {
            printf("refusal '%s': %s (%s)\n", what, ok ? "accepted" : "wrong message or output touched", flx::last_error.c_str());
            return false;
        }
        ++n_refusals;
        return true;
    };
    bool ok = true;
    ok = refused("no words", "no CIGAR words", 0, 0, 0, {}, 5) && ok;
    for (char op : {'M', 'N', 'H', 'P'}) ok = refused("op", "other than", 0, 0, 0, {W(op, 3)}) && ok;
    ok = refused("zero length", "length 0", 0, 0, 0, {W('=', 3), W('I', 0)}) && ok;
    ok = refused("reference", "reference_id", 0, 2, 0, {W('=', 3)}) && ok;
    ok = refused("position", "negative", 0, 0, -1, {W('=', 3)}) && ok;
    ok = refused("span", "behind its sequence", 0, 0, 98, {W('=', 3)}) && ok;
    ok = refused("span with D", "behind its sequence", 0, 0, 0, {W('=', 60), W('I', 9), W('D', 41)}) && ok;
    ok = refused("pool", "outside the pool", 0, 0, 0, {W('=', 3)}, -1, 0, 1) && ok;
    ok = refused("interior clip", "both sides", 0, 0, 0, {W('=', 3), W('S', 2), W('=', 3)}) && ok;
    ok = refused("interior clip behind a lead", "both sides", 0, 0, 0, {W('S', 1), W('X', 3), W('S', 2), W('D', 3), W('S', 2)}) && ok;
    ok = refused("read index", "read_index", 0, 0, 0, {W('=', 3)}, -1, 1) && ok;
    ok = refused("read longer", "sum to 8, its read has 9", 0, 0, 0, {W('S', 2), W('=', 3), W('I', 1), W('X', 2)}, 9) && ok;
    ok = refused("read shorter", "sum to 8, its read has 7", 0, 0, 0, {W('S', 2), W('=', 3), W('I', 1), W('X', 2)}, 7) && ok;
    ok = refused("no reference column", "no reference-consuming column", 0, 0, 0, {W('S', 4), W('I', 3), W('S', 1)}) && ok;
    ok = refused("clips only", "no reference-consuming column", 0, 0, 0, {W('S', 4)}) && ok;
    {
        std::vector<uint32_t> big(9, W('I', (1u << 28) - 1));              // nine words below 2^28 each, 2^31 and more together
        big.push_back(W('=', 1));
        ok = refused("sums", "2^31", 0, 0, 0, big) && ok;
    }
    if (!ok) return 1;
    // just below the limits: a word of 2^28 - 1 inside a sequence of 2^30, at its very end
    {
        Batch b;
        uint32_t const L = (1u << 28) - 1;
        b.add(16, 1, (int32_t)((1u << 30) - L - 2), {W('S', 7), W('=', L), W('D', 2), W('I', 5)});
        flx_paf_summary s;
        if (!flx::paf_plan(b.recs.data(), 0, 1, b.words.data(), b.words.size(), b.offsets.data(), 1, lens, 2, "check", &s)) { printf("a long word was refused: %s\n", flx::last_error.c_str()); return 1; }
        if (s.query_start != 0 || s.query_end != L + 5 || s.ref_end != (1u << 30) || s.matches != L || s.del_bases != 2 || s.ins_bases != 5 || s.gap_opens != 2) { printf("a long word is summarised wrongly\n"); return 1; }
    }
    // the divergence, rounded half up in integers
    struct { uint64_t num, den, want; } const de[] = {{0, 10, 0}, {7, 7, 10000}, {1, 3, 3333}, {2, 3, 6667}, {1, 16, 625}, {1, 32, 313}, {3, 32, 938}, {1, 20000, 1}, {1, 20001, 0}};
    for (auto const& d : de)
        if (flx::paf_divergence_e4(d.num, d.den) != d.want) { printf("divergence %llu / %llu\n", (unsigned long long)d.num, (unsigned long long)d.den); return 1; }
    printf("ok %d cases, %llu mapped records, %llu unmapped, %llu clipped on both sides, %llu neighbours with one op, %d refusals\n", n_cases, (unsigned long long)n_mapped,
           (unsigned long long)n_unmapped, (unsigned long long)n_clipped_both, (unsigned long long)n_same_neighbours, n_refusals);
    return 0;
}
