// The tail rule of flx_tails.hpp (one host implementation, shared by the C ABI, the pipeline's checks and the tests) on random CIGARs
// against definitions that look at every pair of boundaries: t_R is the smallest boundary no other boundary scores above, t_L the
// largest boundary no other scores below, and, when both tails exist with t_L < t_R, the kept words (t_L, t_R] score what the best of
// all O(T^2) segments scores. Stand-alone, built with ASan + UBSan by tests/test_tails_host.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../floxer_amd/csrc/flx_tails.hpp"

namespace flx {
void set_error(const std::string&) {}      // (the header's option checks report through it; the rule itself never does)
}

int main() {
    std::mt19937_64 rng(20240611);
    uint64_t n_right = 0, n_left = 0, n_both = 0, n_none = 0, n_crossed = 0;
    int const n_cases = 20000;
    for (int c = 0; c < n_cases; ++c) {
        uint32_t const T = (uint32_t)(rng() % 120);
        uint32_t const w = 1 + (uint32_t)(rng() % 8), x_drop = (uint32_t)(rng() % 150), min_rows = 1 + (uint32_t)(rng() % 120);
        std::vector<uint32_t> words(T);
        bool const junk_left = rng() % 3 == 0, junk_right = rng() % 3 == 0;
        for (uint32_t t = 0; t < T; ++t) {
            bool const in_junk = (junk_left && t < T / 5) || (junk_right && t >= T - T / 5);
            uint32_t op, len;
            if ((t & 1u) == 0 && !in_junk) { op = 7; len = 1 + (uint32_t)(rng() % 60); }
            else { static const uint32_t ops[3] = {8, 1, 2}; op = ops[rng() % 3]; len = 1 + (uint32_t)(rng() % (in_junk ? 30 : 4)); }
            if (in_junk && rng() % 4 == 0) { op = 7; len = 1 + (uint32_t)(rng() % 3); }
            words[t] = (len << 4) | op;
        }
        flx_tail_result got;
        if (!flx::cigar_tails(words.data(), T, w, x_drop, min_rows, &got)) { printf("case %d: a valid CIGAR was refused\n", c); return 1; }
        // every boundary's sums
        std::vector<int64_t> S(T + 1, 0);
        std::vector<uint64_t> rows(T + 1, 0), cols(T + 1, 0), err(T + 1, 0);
        for (uint32_t t = 1; t <= T; ++t) {
            uint32_t const op = words[t - 1] & 15u, len = words[t - 1] >> 4;
            rows[t] = rows[t - 1] + (op != 2 ? len : 0);
            cols[t] = cols[t - 1] + (op != 1 ? len : 0);
            err[t] = err[t - 1] + (op != 7 ? len : 0);
            S[t] = (int64_t)rows[t] - (int64_t)w * (int64_t)err[t];
        }
        uint32_t tR = 0, tL = 0;
        for (uint32_t t = 0; t <= T; ++t) {                                    // the smallest t that no boundary scores above
            bool top = true;
            for (uint32_t u = 0; u <= T; ++u) top = top && S[u] <= S[t];
            if (top) { tR = t; break; }
        }
        for (uint32_t t = T + 1; t-- > 0;) {                                   // the largest t that no boundary scores below
            bool bottom = true;
            for (uint32_t u = 0; u <= T; ++u) bottom = bottom && S[u] >= S[t];
            if (bottom) { tL = t; break; }
        }
        bool right = S[tR] - S[T] > (int64_t)x_drop && rows[T] - rows[tR] >= min_rows;
        bool left = -S[tL] > (int64_t)x_drop && rows[tL] >= min_rows;
        if (left && right && tL >= tR) { left = right = false; ++n_crossed; }
        if (left && right) {
            int64_t best = 0;
            for (uint32_t a = 0; a <= T; ++a)
                for (uint32_t b = a; b <= T; ++b) best = S[b] - S[a] > best ? S[b] - S[a] : best;
            if (S[tR] - S[tL] != best) { printf("case %d: the kept words are not the maximum-scoring segment\n", c); return 1; }
        }
        flx_tail_result want{0, 0, 0, 0, 0, 0, 0, 0};
        if (left) { want.left_rows = (uint32_t)rows[tL]; want.left_cols = (uint32_t)cols[tL]; want.left_errors = (uint32_t)err[tL]; want.left_words = tL; }
        if (right) {
            want.right_rows = (uint32_t)(rows[T] - rows[tR]); want.right_cols = (uint32_t)(cols[T] - cols[tR]);
            want.right_errors = (uint32_t)(err[T] - err[tR]); want.right_words = T - tR;
        }
        const uint32_t* g = &got.left_rows;
        const uint32_t* e = &want.left_rows;
        for (int f = 0; f < 8; ++f)
            if (g[f] != e[f]) { printf("case %d field %d: got %u, want %u (T %u w %u x %u min %u)\n", c, f, g[f], e[f], T, w, x_drop, min_rows); return 1; }
        n_right += right && !left; n_left += left && !right; n_both += left && right; n_none += !left && !right;
    }
    // an op the rule does not know, and lengths that sum to 2^32
    {
        uint32_t bad[2] = {(10u << 4) | 7u, (5u << 4) | 4u};
        flx_tail_result r;
        if (flx::cigar_tails(bad, 2, 4, 100, 100, &r) || r.right_rows || r.left_rows) { printf("an S op was accepted\n"); return 1; }
        std::vector<uint32_t> big(17, (((1u << 28) - 1u) << 4) | 7u);
        if (flx::cigar_tails(big.data(), 17, 4, 100, 100, &r)) { printf("more than 2^32 rows were accepted\n"); return 1; }
        if (!flx::cigar_tails(big.data(), 16, 4, 100, 100, &r)) { printf("16 * (2^28 - 1) rows were refused\n"); return 1; }
    }
    if (!n_right || !n_left || !n_both || !n_none || !n_crossed) { printf("a class of cases did not occur: %llu %llu %llu %llu %llu\n", (unsigned long long)n_right, (unsigned long long)n_left, (unsigned long long)n_both, (unsigned long long)n_none, (unsigned long long)n_crossed); return 1; }
    printf("ok %d cases: right only %llu, left only %llu, both %llu, none %llu (of them crossed %llu)\n", n_cases, (unsigned long long)n_right,
           (unsigned long long)n_left, (unsigned long long)n_both, (unsigned long long)n_none, (unsigned long long)n_crossed);
    return 0;
}
