// The realignment rule of flx_realign.hpp (one host implementation, shared by the C ABI, the checks of the kernel's seam and the tests)
// on random paths, against full (m + 1) x (n + 1) matrices in 64-bit arithmetic whose minus infinity is a flag of its own, with the
// rule's traceback spelled out over H, E and F. Every result is also replayed over its letters (= columns equal, X columns unequal,
// rows and columns kept), its score recomputed from its words and compared with the input path's, its cells checked against the band
// and its words counted against the bound. Stand-alone, built with ASan + UBSan by tests/test_realign_host.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../floxer_amd/csrc/flx_realign.hpp"

namespace flx {
void set_error(const std::string&) {}      // (the header's checks report through it; the rule itself never does)
}

namespace {

struct Val { bool inf; int64_t v; };        // inf: minus infinity
Val add(Val x, int64_t d) { return x.inf ? x : Val{false, x.v + d}; }
Val vmax(Val x, Val y) { return x.inf ? y : y.inf ? x : Val{false, std::max(x.v, y.v)}; }
bool eq(Val x, Val y) { return !x.inf && !y.inf && x.v == y.v; }

struct Ref { std::vector<uint32_t> words; int64_t score; };

Ref by_matrices(std::vector<uint32_t> const& words, std::vector<uint8_t> const& ref, std::vector<uint8_t> const& qry, uint32_t begin, flx::RealignScores const& s) {
    flx::RealignShape const p = flx::realign_shape(words.data(), words.size(), s);
    int64_t const m = p.m, n = p.n, lo = (int64_t)p.d_min - s.w, hi = (int64_t)p.d_max + s.w;
    std::vector<std::vector<Val>> H(m + 1, std::vector<Val>(n + 1, Val{true, 0})), E = H, F = H;
    for (int64_t i = 0; i <= m; ++i)
        for (int64_t j = std::max<int64_t>(0, i + lo); j <= std::min(n, i + hi); ++j) {
            if (i == 0 && j == 0) { H[0][0] = Val{false, 0}; continue; }
            if (j > 0) E[i][j] = vmax(add(H[i][j - 1], -s.o - s.e), add(E[i][j - 1], -s.e));
            if (i > 0) F[i][j] = vmax(add(H[i - 1][j], -s.o - s.e), add(F[i - 1][j], -s.e));
            Val const dg = (i > 0 && j > 0) ? add(H[i - 1][j - 1], qry[i - 1] == ref[begin + j - 1] ? s.a : -s.b) : Val{true, 0};
            H[i][j] = vmax(dg, vmax(E[i][j], F[i][j]));
        }
    std::vector<uint32_t> ops;
    int64_t i = m, j = n;
    int state = 0;
    while (i > 0 || j > 0) {
        if (state == 0) {
            if (i > 0 && eq(H[i][j], F[i][j])) state = 1;
            else if (j > 0 && eq(H[i][j], E[i][j])) state = 2;
            else { ops.push_back(qry[i - 1] == ref[begin + j - 1] ? 7u : 8u); --i; --j; }
        } else if (state == 1) {
            ops.push_back(1u);
            state = (i - 1 >= 0 && eq(F[i][j], add(F[i - 1][j], -s.e))) ? 1 : 0;
            --i;
        } else {
            ops.push_back(2u);
            state = (j - 1 >= 0 && eq(E[i][j], add(E[i][j - 1], -s.e))) ? 2 : 0;
            --j;
        }
    }
    Ref out{{}, H[m][n].v};
    for (size_t t = ops.size(); t-- > 0;) {
        if (!out.words.empty() && (out.words.back() & 15u) == ops[t]) out.words.back() += 16u;
        else out.words.push_back(16u | ops[t]);
    }
    return out;
}

}  // namespace

int main() {
    std::mt19937_64 rng(99);
    auto const below = [&](uint64_t k) { return (uint64_t)(rng() % k); };
    flx::RealignScores const sets[] = {{2, 4, 4, 2, 16}, {1, 1, 1, 1, 1}, {5, 4, 10, 1, 2}, {1, 15, 1, 1, 3}, {255, 255, 255, 255, 16}};
    uint64_t changed = 0, checked = 0;
    for (int it = 0; it < 3000; ++it) {
        flx::RealignScores const s = sets[it % 5];
        uint32_t const alphabet = it % 2 ? 4u : 2u, begin = (uint32_t)below(4);
        std::vector<uint32_t> words;
        uint64_t cols = 0, target = 1 + below(it % 3 ? 120 : 12);
        while (cols < target) {
            uint64_t const x = below(100);
            uint32_t const op = x < 4 ? 8u : x < 8 ? 1u : x < 12 ? 2u : 7u, len = (uint32_t)(1 + below(op == 7u ? 6 : 4));
            if (!words.empty() && (words.back() & 15u) == op) words.back() += len << 4;
            else words.push_back((len << 4) | op);
            cols += op == 1u ? 0 : len;
        }
        std::vector<uint8_t> ref(begin + cols + below(3)), qry;
        for (auto& c : ref) c = (uint8_t)below(alphabet);
        uint64_t r = begin;
        for (uint32_t w : words) {
            uint32_t const op = w & 15u, len = w >> 4;
            for (uint32_t i = 0; i < len; ++i) {
                if (op == 7u) qry.push_back(ref[r + i]);
                else if (op == 8u) qry.push_back((uint8_t)((ref[r + i] + 1 + below(alphabet - 1)) % alphabet));
                else if (op == 1u) qry.push_back((uint8_t)below(alphabet));
            }
            if (op != 1u) r += len;
        }
        std::vector<uint32_t> got;
        flx::RealignOut const o = flx::realign_path(words.data(), words.size(), ref.data(), qry.data(), begin, s, got);
        Ref const want = by_matrices(words, ref, qry, begin, s);
        flx::RealignShape const in = flx::realign_shape(words.data(), words.size(), s), out = flx::realign_shape(got.data(), got.size(), s);
        if (o.kept || got != want.words || o.score != want.score) { printf("FAIL %d: words or score differ\n", it); return 1; }
        if (out.m != in.m || out.n != in.n || out.score != o.score || out.score < in.score || out.nm != o.num_errors) { printf("FAIL %d: shape or score\n", it); return 1; }
        if (out.d_min < o.diag_lo || out.d_max > o.diag_hi || o.diag_lo != in.d_min - s.w || o.diag_hi != in.d_max + s.w) { printf("FAIL %d: band\n", it); return 1; }
        uint64_t not_eq_words = 0, rr = begin, qq = 0;
        for (size_t t = 0; t < got.size(); ++t) {
            uint32_t const op = got[t] & 15u, len = got[t] >> 4;
            if (len == 0 || (t && (got[t - 1] & 15u) == op)) { printf("FAIL %d: not runs\n", it); return 1; }
            not_eq_words += op != 7u;
            for (uint32_t i = 0; i < len; ++i) {
                if (op == 7u && ref[rr + i] != qry[qq + i]) { printf("FAIL %d: = over unequal letters\n", it); return 1; }
                if (op == 8u && ref[rr + i] == qry[qq + i]) { printf("FAIL %d: X over equal letters\n", it); return 1; }
            }
            if (op != 2u) qq += len;
            if (op != 1u) rr += len;
        }
        uint64_t const bound = (uint64_t)in.nm * flx::realign_c_max(s) / flx::realign_c_min(s);
        if (not_eq_words > bound || got.size() > 2 * bound + 1 || got.size() > flx::realign_cap(in.nm, words.size(), s)) { printf("FAIL %d: word bound\n", it); return 1; }
        changed += got != words;
        ++checked;
    }
    if (changed < checked / 3) { printf("FAIL: only %llu of %llu paths changed\n", (unsigned long long)changed, (unsigned long long)checked); return 1; }
    printf("ok %llu paths, %llu changed\n", (unsigned long long)checked, (unsigned long long)changed);
    return 0;
}
