// The cs rule of flx_cs.hpp (one host implementation, shared by the C ABI, the checks of the kernel's seam and the tests) on random
// paths, against a column-by-column definition: the path is expanded into its columns (op, word, reference column, query row), and the
// string is what the columns emit one after the other, a column that opens a word first emitting what the word puts in front. Every
// string is also measured against cs_path_bytes and, where no two neighbouring words share an op, against the slab bound of
// flx_internal.hpp; the crafted paths that reach the bound must reach it exactly. Stand-alone, built with ASan + UBSan by
// tests/test_cs_host.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../floxer_amd/csrc/flx_cs.hpp"

namespace flx {
void set_error(const std::string&) {}      // (the header's checks report through it; the rule itself never does)
}

namespace {

struct Column { uint32_t op; bool first; uint32_t word_len; int64_t ref; int64_t row; };      // ref / row: -1 where the column has none

char plain_letter(uint8_t rank, bool upper) {
    const char* const lower = "?acgt";
    char const c = (rank >= 1 && rank <= 4) ? lower[rank] : 'n';
    return upper ? (char)(c - 'a' + 'A') : c;
}

std::string by_columns(std::vector<uint32_t> const& words, std::vector<uint8_t> const& ref, std::vector<uint8_t> const& qry, uint32_t begin, uint32_t form) {
    std::vector<Column> cols;
    int64_t r = begin, q = 0;
    for (uint32_t w : words) {
        uint32_t const op = w & 15u, len = w >> 4;
        for (uint32_t c = 0; c < len; ++c) {
            bool const has_ref = op != 1u, has_row = op != 2u;
            cols.push_back(Column{op, c == 0, len, has_ref ? r : -1, has_row ? q : -1});
            if (has_ref) ++r;
            if (has_row) ++q;
        }
    }
    std::string out;
    for (Column const& c : cols) {
        if (c.op == 7u) {
            if (form == 2u) { if (c.first) out += '='; out += plain_letter(ref[(size_t)c.ref], true); }
            else if (c.first) { char buf[16]; snprintf(buf, sizeof(buf), ":%u", c.word_len); out += buf; }
        } else if (c.op == 8u) {
            out += '*'; out += plain_letter(ref[(size_t)c.ref], false); out += plain_letter(qry[(size_t)c.row], false);
        } else if (c.op == 1u) {
            if (c.first) out += '+';
            out += plain_letter(qry[(size_t)c.row], false);
        } else {
            if (c.first) out += '-';
            out += plain_letter(ref[(size_t)c.ref], false);
        }
    }
    return out;
}

int failures = 0;

void check(std::vector<uint32_t> const& words, std::vector<uint8_t> const& ref, std::vector<uint8_t> const& qry, uint32_t begin, int must_reach_bound_form) {
    uint64_t nm = 0, rows = 0;
    bool neighbours_differ = true;
    for (size_t t = 0; t < words.size(); ++t) {
        uint32_t const op = words[t] & 15u, len = words[t] >> 4;
        if (op != 7u) nm += len;
        if (op != 2u) rows += len;
        if (t && (words[t - 1] & 15u) == op) neighbours_differ = false;
    }
    for (uint32_t form = 1; form <= 2; ++form) {
        std::vector<uint8_t> got{'#'};                                  // (the rule appends)
        flx::cs_path(words.data(), words.size(), ref.data(), qry.data(), begin, form, got);
        std::string const g(got.begin() + 1, got.end()), want = by_columns(words, ref, qry, begin, form);
        if (got[0] != '#' || g != want) { ++failures; fprintf(stderr, "form %u: %s != %s\n", form, g.c_str(), want.c_str()); }
        if (flx::cs_path_bytes(words.data(), words.size(), form) != g.size()) { ++failures; fprintf(stderr, "form %u: cs_path_bytes\n", form); }
        uint64_t const bound = flx::cs_slab_bytes(nm, rows, form);
        if (neighbours_differ && g.size() > bound) { ++failures; fprintf(stderr, "form %u: %zu bytes above the bound %llu\n", form, g.size(), (unsigned long long)bound); }
        if (must_reach_bound_form == (int)form && g.size() != bound) { ++failures; fprintf(stderr, "form %u: %zu bytes, bound %llu not reached\n", form, g.size(), (unsigned long long)bound); }
    }
}

}  // namespace

int main() {
    std::mt19937_64 rng(20261019);
    auto pick = [&](uint64_t n) { return (uint32_t)(rng() % n); };
    uint64_t n_paths = 0;
    // random paths over ranks 0..5 (and a few bytes beyond them), neighbouring words of one op included
    for (int it = 0; it < 4000; ++it) {
        std::vector<uint32_t> words;
        uint32_t const n_words = 1 + pick(it % 10 == 0 ? 200 : 12);
        uint64_t cols = 0, rows = 0;
        for (uint32_t t = 0; t < n_words; ++t) {
            static const uint32_t ops[4] = {7u, 8u, 1u, 2u};
            uint32_t const op = ops[pick(4)];
            static const uint32_t lens[12] = {1, 1, 2, 3, 9, 10, 63, 64, 65, 99, 100, 130};
            uint32_t const len = op == 7u && pick(20) == 0 ? 1000 + pick(3) : lens[pick(12)];
            words.push_back(len << 4 | op);
            if (op != 1u) cols += len;
            if (op != 2u) rows += len;
        }
        uint32_t const begin = pick(5);
        std::vector<uint8_t> ref(begin + cols), qry(rows);              // exactly as long as the path: one letter further is out of bounds
        for (auto& x : ref) x = (uint8_t)(pick(50) == 0 ? 6 + pick(250) : pick(6));
        for (auto& x : qry) x = (uint8_t)(pick(50) == 0 ? 6 + pick(250) : pick(6));
        check(words, ref, qry, begin, 0);
        ++n_paths;
    }
    // the bounds, reached: one '=' word of 100 000 columns and more (short), = X = X ... = with single X columns (long)
    {
        std::vector<uint32_t> const words{102400u << 4 | 7u};
        std::vector<uint8_t> const ref(102400, 1), qry(102400, 1);
        check(words, ref, qry, 0, 1);
        std::vector<uint32_t> alt;
        for (int i = 0; i < 300; ++i) { alt.push_back((1u + pick(9)) << 4 | 7u); alt.push_back(1u << 4 | 8u); }
        alt.push_back(5u << 4 | 7u);
        uint64_t len = 0;
        for (uint32_t w : alt) len += w >> 4;
        std::vector<uint8_t> r2(len, 2), q2(len, 3);
        check(alt, r2, q2, 0, 2);
        n_paths += 2;
    }
    // the empty path
    check({}, {}, {}, 0, 0);
    if (failures) { printf("FAILED %d\n", failures); return 1; }
    printf("ok %llu paths\n", (unsigned long long)n_paths + 1);
    return 0;
}
