// The left-align rule of flx_leftalign.hpp (one host implementation, shared by the C ABI, the checks of the kernel's seam and the tests)
// on random, non-optimal paths over low-complexity sequences, against a definition that moves one gap one column at a time: the words
// are taken left to right, and a gap word is stepped left - merging with a gap of its kind that it touches - until no step is valid.
// Every result is also replayed over its letters (= columns equal, spans and NM kept), checked for normal form and for idempotence.
// Stand-alone, built with ASan + UBSan by tests/test_leftalign_host.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../floxer_amd/csrc/flx_leftalign.hpp"

namespace flx {
void set_error(const std::string&) {}      // (the header's checks report through it; the rule itself never does)
}

namespace {

struct Word { uint32_t op, len; };

// one column at a time, in left-to-right order of the words
std::vector<Word> by_steps(std::vector<Word> const& path, std::vector<uint8_t> const& ref, std::vector<uint8_t> const& qry, uint32_t begin) {
    std::vector<Word> out;
    uint64_t r = begin, q = 0;
    auto push = [&](uint32_t op, uint64_t len) {
        if (len == 0) return;
        if (!out.empty() && out.back().op == op) out.back().len += (uint32_t)len;
        else out.push_back(Word{op, (uint32_t)len});
    };
    for (Word const w : path) {
        if (w.op == 7 || w.op == 8) { push(w.op, w.len); r += w.len; q += w.len; continue; }
        std::vector<uint8_t> const& seq = w.op == 2 ? ref : qry;
        uint64_t c = w.op == 2 ? r : q, L = w.len, behind = 0;      // behind: the = columns the gap has crossed
        for (;;) {
            if (out.empty()) break;
            if (out.back().op == w.op) { L += out.back().len; c -= out.back().len; out.pop_back(); continue; }
            if (out.back().op != 7) break;
            if (out.size() == 1 && out.back().len == 1) break;      // the path's first column stays
            if (seq[c - 1] != seq[c - 1 + L]) break;
            if (--out.back().len == 0) out.pop_back();
            --c; ++behind;
        }
        out.push_back(Word{w.op, (uint32_t)L});
        push(7, behind);
        if (w.op == 2) r += w.len; else q += w.len;
    }
    return out;
}

bool replay(std::vector<Word> const& path, std::vector<uint8_t> const& ref, std::vector<uint8_t> const& qry, uint32_t begin, uint64_t sums[3]) {
    uint64_t r = begin, q = 0, nm = 0;
    for (Word const w : path) {
        if (w.len == 0) return false;
        for (uint32_t i = 0; i < w.len; ++i) {
            if (w.op == 7 && ref[r + i] != qry[q + i]) return false;
            if (w.op == 8 && ref[r + i] == qry[q + i]) return false;
        }
        if (w.op != 2) q += w.len;
        if (w.op != 1) r += w.len;
        if (w.op != 7) nm += w.len;
    }
    sums[0] = r; sums[1] = q; sums[2] = nm;
    return r <= ref.size() && q <= qry.size();
}

}  // namespace

int main() {
    std::mt19937_64 rng(20241018);
    uint64_t n_moved = 0, n_grown = 0, n_merged = 0, n_gaps = 0;
    int const n_cases = 20000;
    for (int c = 0; c < n_cases; ++c) {
        uint32_t const alphabet = 1 + (uint32_t)(rng() % 3), T = 1 + (uint32_t)(rng() % 24), max_len = 1 + (uint32_t)(rng() % 6);
        std::vector<Word> path;
        uint32_t last = 0;
        for (uint32_t t = 0; t < T; ++t) {
            static const uint32_t ops[6] = {7, 7, 7, 8, 1, 2};
            uint32_t const op = ops[rng() % 6];
            if (op == last) continue;
            path.push_back(Word{op, 1 + (uint32_t)(rng() % max_len)});
            last = op;
        }
        uint32_t const begin = (uint32_t)(rng() % 4);
        uint64_t cols = begin;
        for (Word const w : path) cols += w.op != 1 ? w.len : 0;
        std::vector<uint8_t> ref(cols + rng() % 3), qry;
        for (auto& x : ref) x = (uint8_t)(rng() % alphabet);
        uint64_t r = begin;
        for (Word const w : path) {
            for (uint32_t i = 0; i < w.len; ++i) {
                if (w.op == 7) qry.push_back(ref[r + i]);
                else if (w.op == 8) qry.push_back((uint8_t)(ref[r + i] + 1 + rng() % 2));
                else if (w.op == 1) qry.push_back((uint8_t)(rng() % alphabet));
            }
            if (w.op != 1) r += w.len;
        }
        std::vector<uint32_t> words, got;
        for (Word const w : path) words.push_back((w.len << 4) | w.op);
        flx_left_align_job const job{0, (uint32_t)words.size(), 0, 0, (uint32_t)ref.size(), begin, 0, (uint32_t)qry.size(), 0};
        if (!flx::left_align_jobs_valid(ref.size(), qry.size(), words.data(), words.size(), &job, 1, "check")) { printf("case %d: a valid job was refused\n", c); return 1; }
        // (exactly sized copies: a read outside the window or the query is the sanitizer's to find)
        std::vector<uint8_t> const ref_exact(ref.begin(), ref.end()), qry_exact(qry.begin(), qry.end());
        flx::left_align_path(words.data(), words.size(), ref_exact.data(), qry_exact.data(), begin, got);
        std::vector<Word> const want = by_steps(path, ref, qry, begin);
        bool same = got.size() == want.size();
        for (size_t t = 0; same && t < got.size(); ++t) same = got[t] == ((want[t].len << 4) | want[t].op);
        if (!same) { printf("case %d: the rule and the stepwise definition differ\n", c); return 1; }
        uint64_t a[3], b[3];
        if (!replay(path, ref, qry, begin, a) || !replay(want, ref, qry, begin, b) || a[0] != b[0] || a[1] != b[1] || a[2] != b[2]) { printf("case %d: the result does not replay\n", c); return 1; }
        for (size_t t = 1; t < want.size(); ++t) if (want[t].op == want[t - 1].op) { printf("case %d: neighbouring words share an op\n", c); return 1; }
        if (want.size() > 2 * a[2] + 1 || got.size() > flx::left_align_cap(words.data(), words.size())) { printf("case %d: too many words\n", c); return 1; }
        std::vector<uint32_t> again;
        flx::left_align_path(got.data(), got.size(), ref_exact.data(), qry_exact.data(), begin, again);
        if (again != got) { printf("case %d: not idempotent\n", c); return 1; }
        uint64_t gaps_in = 0, gaps_out = 0;
        for (Word const w : path) gaps_in += w.op == 1 || w.op == 2;
        for (Word const w : want) gaps_out += w.op == 1 || w.op == 2;
        n_gaps += gaps_in;
        n_merged += gaps_in - gaps_out;
        n_moved += got != words;
        n_grown += got.size() > words.size();
    }
    if (n_moved < 2000 || n_grown < 500 || n_merged < 200) { printf("the cases exercise too little: moved %llu grown %llu merged %llu\n", (unsigned long long)n_moved, (unsigned long long)n_grown, (unsigned long long)n_merged); return 1; }
    printf("ok %d paths, %llu gap words: %llu paths changed, %llu grew, %llu gap words merged away\n", n_cases, (unsigned long long)n_gaps, (unsigned long long)n_moved,
           (unsigned long long)n_grown, (unsigned long long)n_merged);
    return 0;
}
