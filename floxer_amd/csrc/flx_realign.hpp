// Affine-gap realignment of a traced path (flx_realign_options, include/floxer_amd.h). Host code only: the rule on one path, used by
// flx_realign (flx_capi_host.cpp), by the checks of flx_realign_batch and by the tests; the kernel cigar_realign (flx_realign.hip)
// computes the same words and numbers on the device.
//
// Every CIGAR of this project is an edit-distance path, and K5 takes the first valid move among up, left and diagonal: an indel of
// several bases often comes out scattered (1D 2= 1D 1= 1D) where a scored aligner writes 3D and an X or two. Left-alignment
// (flx_leftalign.hpp) moves a gap but never merges gaps through an X or the other gap kind. The rule here runs a banded global DP with
// affine gap costs over exactly the rows and columns the path consumes and takes its optimum:
//   - input: words over = (7) X (8) I (1) D (2), a reference window, a query and `begin`, the window column of the path's first column.
//     The path has m rows; its n columns are the reference columns it consumes. Letters are rank bytes, equal byte = match, ranks 0 and 5
//     have no special case (as in left-align and MD);
//   - scores a = match, b = mismatch, o = gap open, e = gap extend, all positive; a gap of length L costs o + e L;
//   - band: d = j - i over the cells the input path visits, (0,0) included; lo = min d - w, hi = max d + w; cells outside [lo, hi] are
//     -infinity;
//   - DP, global (both ends fixed: position, rows and columns never change): H[0][0] = 0 and nothing else is initialised,
//         E[i][j] = max(H[i][j-1] - o - e, E[i][j-1] - e)     a D column, a left move
//         F[i][j] = max(H[i-1][j] - o - e, F[i-1][j] - e)     an I row, an up move
//         H[i][j] = max(H[i-1][j-1] + (q_i == r_j ? a : -b), E[i][j], F[i][j])
//     in 32-bit signed arithmetic; -infinity is -2^30 here and every finite value stays above -2^29 (a path whose
//     (m + n + 2) * max(a, b, o + e) reaches 2^29 is not realigned: it keeps its words and is flagged `kept`), so nothing wraps and a
//     value derived from -infinity never equals a finite one;
//   - traceback from (m, n) in state H; the ties are part of the definition and follow this project's up > left > diagonal:
//       state H: H == F: go to state F; else H == E: go to state E; else emit = or X by the letters and step diagonally;
//       state F: emit one I and step up; stay in F when F[i][j] == F[i-1][j] - e (extension wins the tie; the cell above is then in
//                the band), else go to state H;
//       state E: the mirror image, with D and a step left;
//   - the result: the words (runs of equal ops, no length 0), score = H[m][n], num_errors = the X, I and D lengths of the new words
//     (it can exceed the edit distance).
// What it guarantees: score >= the input path's score under the same scores (the input path lies in the band); every = pairs equal
// letters and every X unequal ones; every cell of the result lies in the band; with c_max = max(a + b, o + e + a) and
// c_min = min(a + b, o + e) the result has at most floor(NM c_max / c_min) words that are not =, NM being the input's X + I + D lengths
// (the result's penalty against a m is <= the input's <= NM c_max, and every word that is not = costs at least c_min), so at most
// 2 floor(NM c_max / c_min) + 1 words in all: the slab of a job. The rule is NOT idempotent: the band follows the input path.
// The defaults (2, 4, 4, 2, band 16) are the first piece of minimap2's map-ont scores: conventions, fitted to nothing.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "flx_internal.hpp"
#include "flx_leftalign.hpp"

namespace flx {

constexpr int32_t REALIGN_NEG = -(1 << 30);       // -infinity of the DP
constexpr uint32_t REALIGN_MAX_SCORE = 255u, REALIGN_MAX_BAND = 1024u, REALIGN_MAX_RATIO = 8u;

// the scores and the band of a run, defaults filled in
struct RealignScores { int32_t a, b, o, e, w; };
inline RealignScores realign_scores(const flx_realign_options* O) {
    RealignScores s{2, 4, 4, 2, 16};
    if (!O) return s;
    if (O->match) s.a = (int32_t)O->match;
    if (O->mismatch) s.b = (int32_t)O->mismatch;
    if (O->gap_open) s.o = (int32_t)O->gap_open;
    if (O->gap_extend) s.e = (int32_t)O->gap_extend;
    if (O->band) s.w = (int32_t)O->band;
    return s;
}
inline uint32_t realign_c_max(RealignScores const& s) { return (uint32_t)std::max(s.a + s.b, s.o + s.e + s.a); }
inline uint32_t realign_c_min(RealignScores const& s) { return (uint32_t)std::min(s.a + s.b, s.o + s.e); }

// NULL is no options; enable must be 0 or 1, every score <= 255, band <= 1024, c_max <= 8 c_min and the reserved fields 0
inline bool realign_options_valid(const flx_realign_options* O) {
    if (!O) return true;
    if (O->enable > 1) { set_error("flx_realign_options: enable must be 0 or 1"); return false; }
    for (uint32_t r : O->reserved) if (r) { set_error("flx_realign_options: the reserved fields must be 0"); return false; }
    if (O->match > REALIGN_MAX_SCORE || O->mismatch > REALIGN_MAX_SCORE || O->gap_open > REALIGN_MAX_SCORE || O->gap_extend > REALIGN_MAX_SCORE) {
        set_error("flx_realign_options: a score above 255"); return false;
    }
    if (O->band > REALIGN_MAX_BAND) { set_error("flx_realign_options: band above 1024"); return false; }
    RealignScores const s = realign_scores(O);
    if (realign_c_max(s) > REALIGN_MAX_RATIO * realign_c_min(s)) { set_error("flx_realign_options: max(a + b, o + e + a) must not exceed 8 min(a + b, o + e)"); return false; }
    return true;
}
inline bool realign_options_active(const flx_realign_options* O) { return O && O->enable; }

// what the words say: rows, columns, the X + I + D lengths, the path's score and the diagonals it visits
struct RealignShape { uint32_t m, n, nm; int32_t d_min, d_max; int64_t score; };
inline RealignShape realign_shape(const uint32_t* words, uint64_t n_words, RealignScores const& s) {
    RealignShape p{0, 0, 0, 0, 0, 0};
    int64_t d = 0;
    for (uint64_t t = 0; t < n_words; ++t) {
        uint32_t const op = words[t] & 15u, len = words[t] >> 4;
        if (op == 7u) { p.m += len; p.n += len; p.score += (int64_t)s.a * len; }
        else if (op == 8u) { p.m += len; p.n += len; p.nm += len; p.score -= (int64_t)s.b * len; }
        else if (op == 1u) { p.m += len; p.nm += len; d -= len; p.d_min = (int32_t)std::min<int64_t>(p.d_min, d); p.score -= s.o + (int64_t)s.e * len; }
        else { p.n += len; p.nm += len; d += len; p.d_max = (int32_t)std::max<int64_t>(p.d_max, d); p.score -= s.o + (int64_t)s.e * len; }
    }
    return p;
}
// a path this long could leave the range in which no 32-bit value wraps: it keeps its words
inline bool realign_too_long(uint32_t m, uint32_t n, RealignScores const& s) {
    return ((uint64_t)m + n + 2u) * (uint64_t)std::max({s.a, s.b, s.o + s.e}) >= (1ull << 29);
}
// Words a job's result holds at most (the guarantee above), and never fewer than its input (a kept path is copied)
inline uint64_t realign_cap(uint32_t nm, uint64_t n_words, RealignScores const& s) {
    return std::max<uint64_t>(2ull * ((uint64_t)nm * realign_c_max(s) / realign_c_min(s)) + 1ull, n_words);
}
// num_errors of a realigned path at most: its penalty is <= NM c_max and every X, I or D column costs at least min(a + b, e)
inline uint64_t realign_nm_bound(uint32_t nm, RealignScores const& s) { return (uint64_t)nm * realign_c_max(s) / (uint32_t)std::min(s.a + s.b, s.e); }
// The kernel's trace of a job in 32-bit words: 4 bits per band cell, eight cells of a row in a word, [stripe of 64 rows][word][row in
// the stripe]; rows 0..m; B = hi - lo + 1 cells per row. A band wider than the hand-over row the kernel keeps in LDS adds 2 B words in
// front (H and F of a stripe's last row).
constexpr uint32_t REALIGN_LDS_BAND = 1024u;
constexpr uint32_t REALIGN_GRID_CAP = 1u << 16;            // most blocks (one wave each) of a cigar_realign launch
inline uint64_t realign_trace_words(uint32_t m, uint64_t band_cells) {
    uint64_t const stripes = ((uint64_t)m + 64u) / 64u, per_row = (band_cells + 7u) / 8u;
    return stripes * per_row * 64u + (band_cells > REALIGN_LDS_BAND ? 2u * band_cells : 0u);
}

struct RealignOut { int32_t score; uint32_t num_errors; int32_t diag_lo, diag_hi; uint32_t kept; };

// The rule on the words [words, words + n_words): ref / query point at the window's / the query's first letter. The caller has judged
// the words (left_align_jobs_valid). The result replaces *out.
inline RealignOut realign_path(const uint32_t* words, uint64_t n_words, const uint8_t* ref, const uint8_t* query, uint32_t begin, RealignScores const& s,
                               std::vector<uint32_t>& out) {
    out.clear();
    RealignShape const p = realign_shape(words, n_words, s);
    int32_t const lo = p.d_min - s.w, hi = p.d_max + s.w;
    if (realign_too_long(p.m, p.n, s)) {
        out.assign(words, words + n_words);
        return RealignOut{0, p.nm, lo, hi, 1u};
    }
    int64_t const m = p.m, n = p.n, B = (int64_t)hi - lo + 1;
    // codes[i * B + (j - i - lo)]: bits 0-1 = where H came from (0 diagonal, 1 F, 2 E), bit 2 = E extended, bit 3 = F extended
    std::vector<uint8_t> codes((size_t)((m + 1) * B), 0);
    std::vector<int32_t> H((size_t)B, REALIGN_NEG), F((size_t)B, REALIGN_NEG), Hn((size_t)B), Fn((size_t)B);      // row i - 1, then row i
    const uint8_t* const r = ref + begin;
    int32_t score = 0;
    for (int64_t i = 0; i <= m; ++i) {
        int32_t h_left = REALIGN_NEG, e_left = REALIGN_NEG;
        for (int64_t c = 0; c < B; ++c) {
            int64_t const j = i + lo + c;
            if (j < 0 || j > n) { Hn[c] = Fn[c] = REALIGN_NEG; h_left = e_left = REALIGN_NEG; continue; }
            // row i - 1 holds column j at c + 1 and column j - 1 at c
            int32_t const up_h = c + 1 < B ? H[c + 1] : REALIGN_NEG, up_f = c + 1 < B ? F[c + 1] : REALIGN_NEG, dg_h = H[c];
            int32_t const e_open = h_left - s.o - s.e, e_ext = e_left - s.e, f_open = up_h - s.o - s.e, f_ext = up_f - s.e;
            int32_t const e = std::max(e_open, e_ext), f = std::max(f_open, f_ext);
            int32_t const dg = (i > 0 && j > 0) ? dg_h + (query[i - 1] == r[j - 1] ? s.a : -s.b) : REALIGN_NEG;
            int32_t h = std::max(dg, std::max(e, f));
            uint8_t code = (uint8_t)((h == f ? 1u : h == e ? 2u : 0u) | (e_ext >= e_open ? 4u : 0u) | (f_ext >= f_open ? 8u : 0u));
            if (i == 0 && j == 0) { h = 0; code = 0; }
            codes[(size_t)(i * B + c)] = code;
            Hn[c] = h; Fn[c] = f;
            h_left = h; e_left = (i == 0 && j == 0) ? REALIGN_NEG : e;
            if (i == m && j == n) score = h;
        }
        H.swap(Hn); F.swap(Fn);
    }
    // the walk back, words right to left
    std::vector<uint32_t> rev;
    uint32_t num_errors = 0;
    auto const emit = [&](uint32_t op) {
        if (!rev.empty() && (rev.back() & 15u) == op) rev.back() += 16u;
        else rev.push_back(16u | op);
        if (op != 7u) ++num_errors;
    };
    int64_t i = m, j = n;
    int state = 0;
    while (i > 0 || j > 0) {
        uint8_t const code = codes[(size_t)(i * B + (j - i - lo))];
        if (state == 0) {
            uint32_t const src = code & 3u;
            if (src == 1u) state = 1;
            else if (src == 2u) state = 2;
            else { emit(query[i - 1] == r[j - 1] ? 7u : 8u); --i; --j; }
        } else if (state == 1) {
            emit(1u); --i;
            state = (code & 8u) ? 1 : 0;
        } else {
            emit(2u); --j;
            state = (code & 4u) ? 2 : 0;
        }
    }
    out.assign(rev.rbegin(), rev.rend());
    return RealignOut{score, num_errors, lo, hi, 0u};
}

}  // namespace flx
