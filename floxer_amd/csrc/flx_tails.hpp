// Chimeric tails of reads that are mapped in full (flx_split_options, include/floxer_amd.h). Host code only: the rule on one CIGAR, used
// by flx_cigar_tails (flx_capi_host.cpp), by the checks of flx_cigar_tails_batch and by the tests; the kernel cigar_tails (flx_tails.hip)
// computes the same numbers on the device behind the traceback, and the stage split_tails (flx_verify.cpp) acts on them.
//
// A read whose whole length fits ceil(len * p) errors is written as one record even when its last few hundred bases belong elsewhere:
// the break shows only as a run of X / I / D at one end of the CIGAR. The rule reads the extension's score (rows - w * errors, the
// score of flx_extend_options) off the path:
//   - a CIGAR core of T words, ops = X I D only (anything else: the job is invalid), the lengths summing to less than 2^32;
//   - boundary t = 0 .. T lies behind word t: rows_t = query consumed (= X I), cols_t = reference consumed (= X D), err_t = lengths of
//     X, I and D, S_t = rows_t - w * err_t as a signed 64-bit number, S_0 = 0;
//   - right tail: G = max_t S_t, t_R the smallest t with S_t = G; it exists iff G - S_T > X and rows_T - rows_{t_R} >= min_tail_rows;
//   - left tail: g = min_t S_t, t_L the largest t with S_t = g; it exists iff -g > X and rows_{t_L} >= min_tail_rows;
//   - both exist and t_L >= t_R: nothing would be kept, so neither is reported; with t_L < t_R the kept words (t_L, t_R] are the path's
//     maximum-scoring segment. Cuts fall on word boundaries;
//   - w = 4, X = 100 (the conventions of the extension) and min_tail_rows = 100 are conventions of this project, not fitted to anything.
// Reported per tail: its rows, columns, errors and words (zeros: absent).
// Limits: a tail that holds a second good region behind a second break is cut once; a structural indel inside a read whose score
// recovers afterwards is not a break.
#pragma once
#include <cstdint>
#include <string>

#include "flx_internal.hpp"

namespace flx {

constexpr uint32_t SPLIT_DEFAULT_MIN_TAIL_ROWS = 100;
constexpr uint32_t SPLIT_MAX_MIN_TAIL_ROWS = EXTEND_MAX_ROWS;      // (no read has more rows)

inline uint32_t split_weight(uint32_t v) { return v ? v : EXTEND_DEFAULT_WEIGHT; }
inline uint32_t split_x_drop(uint32_t v) { return v ? v : EXTEND_DEFAULT_XDROP; }
inline uint32_t split_min_tail_rows(uint32_t v) { return v ? v : SPLIT_DEFAULT_MIN_TAIL_ROWS; }

inline bool tail_values_valid(uint32_t error_weight, uint32_t x_drop, uint32_t min_tail_rows, const char* who) {
    if (error_weight > EXTEND_MAX_WEIGHT) { set_error(std::string(who) + ": error_weight must be at most 65535"); return false; }
    if (x_drop > EXTEND_MAX_XDROP) { set_error(std::string(who) + ": x_drop must be at most 2^30"); return false; }
    if (min_tail_rows > SPLIT_MAX_MIN_TAIL_ROWS) { set_error(std::string(who) + ": min_tail_rows must be below 2^19"); return false; }
    return true;
}
// NULL is no options; enable must be 0 or 1, the reserved fields 0 and the three values within the bounds of flx_extend_options
inline bool split_options_valid(const flx_split_options* o) {
    if (!o) return true;
    if (o->enable > 1) { set_error("flx_split_options: enable must be 0 or 1"); return false; }
    for (uint32_t r : o->reserved) if (r) { set_error("flx_split_options: the reserved fields must be 0"); return false; }
    return tail_values_valid(o->error_weight, o->x_drop, o->min_tail_rows, "flx_split_options");
}
inline bool split_options_active(const flx_split_options* o) { return o && o->enable; }

// The rule on the words [words, words + n_words) with the values as given (no defaults here). false: an op other than = X I D, or
// lengths that sum to 2^32 or more; *out is zeroed then.
inline bool cigar_tails(const uint32_t* words, uint64_t n_words, uint32_t w, uint32_t x_drop, uint32_t min_tail_rows, flx_tail_result* out) {
    *out = flx_tail_result{0, 0, 0, 0, 0, 0, 0, 0};
    struct At { uint64_t t; uint32_t rows, cols, err; };
    At first_max{0, 0, 0, 0}, last_min{0, 0, 0, 0};
    int64_t S = 0, G = 0, g = 0;
    uint64_t rows = 0, cols = 0, err = 0, total = 0;
    for (uint64_t t = 1; t <= n_words; ++t) {
        uint32_t const op = words[t - 1] & 15u, len = words[t - 1] >> 4;
        if (op != 7u && op != 8u && op != 1u && op != 2u) return false;
        total += len;
        if (total >= (1ull << 32)) return false;
        if (op != 2u) rows += len;
        if (op != 1u) cols += len;
        if (op != 7u) err += len;
        S = (int64_t)rows - (int64_t)w * (int64_t)err;
        if (S > G) { G = S; first_max = At{t, (uint32_t)rows, (uint32_t)cols, (uint32_t)err}; }
        if (S <= g) { g = S; last_min = At{t, (uint32_t)rows, (uint32_t)cols, (uint32_t)err}; }
    }
    bool const right = G - S > (int64_t)x_drop && rows - first_max.rows >= min_tail_rows;
    bool const left = -g > (int64_t)x_drop && last_min.rows >= min_tail_rows;
    if (left && right && last_min.t >= first_max.t) return true;
    if (left) { out->left_rows = last_min.rows; out->left_cols = last_min.cols; out->left_errors = last_min.err; out->left_words = (uint32_t)last_min.t; }
    if (right) {
        out->right_rows = (uint32_t)rows - first_max.rows; out->right_cols = (uint32_t)cols - first_max.cols;
        out->right_errors = (uint32_t)err - first_max.err; out->right_words = (uint32_t)(n_words - first_max.t);
    }
    return true;
}

// the jobs of flx_cigar_tails / flx_cigar_tails_batch, judged on the host: inside the pool, ops = X I D only, values within their bounds
inline bool tail_jobs_valid(const uint32_t* words, uint64_t n_words, const flx_tail_job* jobs, uint64_t n, const char* who) {
    for (uint64_t i = 0; i < n; ++i) {
        flx_tail_job const& j = jobs[i];
        if (j.cigar_offset > n_words || j.cigar_length > n_words - j.cigar_offset) { set_error(std::string(who) + ": job outside the pool"); return false; }
        if (!tail_values_valid(j.error_weight, j.x_drop, j.min_tail_rows, who)) return false;
        uint64_t total = 0;
        for (uint32_t t = 0; t < j.cigar_length; ++t) {
            uint32_t const word = words[j.cigar_offset + t], op = word & 15u;
            if (op != 7u && op != 8u && op != 1u && op != 2u) { set_error(std::string(who) + ": a CIGAR op other than = X I D"); return false; }
            total += word >> 4;
        }
        if (total >= (1ull << 32)) { set_error(std::string(who) + ": the op lengths of a job sum to 2^32 or more"); return false; }
    }
    return true;
}

}  // namespace flx
