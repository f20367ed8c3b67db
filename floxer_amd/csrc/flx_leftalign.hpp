// Left-aligned indels (flx_gap_options, include/floxer_amd.h). Host code only: the rule on one traced path, used by flx_left_align
// (flx_capi_host.cpp), by the checks of flx_left_align_batch and by the tests; the kernel cigar_left_align (flx_leftalign.hip) computes
// the same words on the device between the traceback and md_build / cigar_tails, which then read the normalised words.
//
// K5 takes an up or left move as soon as one is valid, so inside a homopolymer or a tandem repeat a gap lands on the last copy: gaps are
// right-aligned, floxer's (seqan3's) convention and this project's default. Variant callers, VCF, minimap2 and bwa put a gap on the
// first copy. The rule moves every gap as far left as it goes without changing what the path says:
//   - a path is a list of words (op, len), ops = (7) X (8) I (1) D (2), over a reference window, a query and `begin`, the window column
//     of the path's first column. A letter is the rank byte the DP compared: equal rank = equal letter, ranks 0..5, no special cases
//     (IUPAC codes collapse as they do in MD);
//   - the words are processed LEFT TO RIGHT into an output list. = and X words are appended, a word of the last output word's op
//     merging with it. A gap word of kind K (I or D) and length L starts at position c of its own sequence (the reference for D, the
//     query for I). Repeat: no previous output word: stop. The previous output word is of kind K: remove it, add its length to L, move
//     c left by it, repeat. It is X or the other gap kind: stop. It is = of length E: Emax = E, or E - 1 when that = is the path's
//     first word (a gap never becomes a path's first word by shifting: POS and the first column stay); s = the largest s <= Emax with
//     seq[c - i] == seq[c - i + L] for i = 1..s; s == 0: stop; else shorten the = by s (drop it at 0), c -= s, and stop if s < E, else
//     repeat. Then append the gap and an = of the total shift, which merges with a following = word;
//   - a gap that is a path's first word stays.
// What it guarantees: begin, the rows and columns consumed and NM do not change; every = column still pairs equal letters; no two
// neighbouring words share an op and none has length 0 (given input words of non-zero length); the word count stays <= 2 NM + 1 (it can
// grow: 5= 2D 1X becomes 2= 2D 3= 1X); the rule is idempotent; no gap of the result can move one more column left under it.
// The order is part of the definition: rewriting "one step at a time in any order" is NOT confluent once gaps merge (a merged gap has
// another length, and so another set of columns it may cross), so two orders can end in different normal forms. Left to right it is.
// Limits: a gap does not move through X or through the other gap kind, so it is not the leftmost placement over all paths of equal
// score, only over the shifts that keep every other word.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "flx_internal.hpp"

namespace flx {

// NULL is no options; left_align must be 0 or 1 and the reserved fields 0
inline bool gap_options_valid(const flx_gap_options* o) {
    if (!o) return true;
    if (o->left_align > 1) { set_error("flx_gap_options: left_align must be 0 or 1"); return false; }
    for (uint32_t r : o->reserved) if (r) { set_error("flx_gap_options: the reserved fields must be 0"); return false; }
    return true;
}
inline bool gap_options_active(const flx_gap_options* o) { return o && o->left_align; }

// The rule on the words [words, words + n_words): ref / query point at the window's / the query's first letter. The caller has judged
// the words (left_align_jobs_valid): ops = X I D, no zero length, the path inside the window and the query. The result replaces *out.
inline void left_align_path(const uint32_t* words, uint64_t n_words, const uint8_t* ref, const uint8_t* query, uint32_t begin, std::vector<uint32_t>& out) {
    out.clear();
    uint64_t r = begin, q = 0;
    for (uint64_t t = 0; t < n_words; ++t) {
        uint32_t const op = words[t] & 15u, len = words[t] >> 4;
        if (op == 7u || op == 8u) {
            if (!out.empty() && (out.back() & 15u) == op) out.back() += len << 4;
            else out.push_back(words[t]);
            r += len; q += len;
            continue;
        }
        const uint8_t* const seq = op == 2u ? ref : query;
        uint64_t c = op == 2u ? r : q, L = len, shift = 0;
        while (!out.empty()) {
            uint32_t const p_op = out.back() & 15u, p_len = out.back() >> 4;
            if (p_op == op) { out.pop_back(); L += p_len; c -= p_len; continue; }
            if (p_op != 7u) break;
            uint64_t const e_max = out.size() == 1 ? p_len - 1u : p_len;
            uint64_t s = 0;
            while (s < e_max && seq[c - s - 1] == seq[c - s - 1 + L]) ++s;
            if (s == 0) break;
            if (s == p_len) out.pop_back();
            else out.back() -= (uint32_t)s << 4;
            c -= s; shift += s;
            if (s < p_len) break;
        }
        out.push_back((uint32_t)(L << 4) | op);
        if (shift) out.push_back((uint32_t)(shift << 4) | 7u);
        if (op == 2u) r += len; else q += len;
    }
}

// Words a job's result holds at most: every gap word can add one = word behind it
inline uint64_t left_align_cap(const uint32_t* words, uint64_t n) {
    uint64_t cap = n;
    for (uint64_t t = 0; t < n; ++t) { uint32_t const op = words[t] & 15u; cap += (op == 1u || op == 2u) ? 1u : 0u; }
    return cap;
}

// the jobs of flx_left_align / flx_left_align_batch, judged on the host: inside the pools, ops = X I D only, no zero-length word, the
// columns the words consume inside [begin, ref_length) and their rows inside the query
inline bool left_align_jobs_valid(uint64_t ref_pool_len, uint64_t query_pool_len, const uint32_t* words, uint64_t n_words, const flx_left_align_job* jobs,
                                  uint64_t n, const char* who) {
    for (uint64_t i = 0; i < n; ++i) {
        flx_left_align_job const& j = jobs[i];
        if (j.reserved || j.reserved2) { set_error(std::string(who) + ": the reserved fields must be 0"); return false; }
        if (j.cigar_offset > n_words || j.cigar_length > n_words - j.cigar_offset || j.ref_offset > ref_pool_len || j.ref_length > ref_pool_len - j.ref_offset ||
            j.query_offset > query_pool_len || j.query_length > query_pool_len - j.query_offset) {
            set_error(std::string(who) + ": job outside its pools"); return false;
        }
        uint64_t rows = 0, cols = j.begin;
        for (uint32_t t = 0; t < j.cigar_length; ++t) {
            uint32_t const word = words[j.cigar_offset + t], op = word & 15u, len = word >> 4;
            if (op != 7u && op != 8u && op != 1u && op != 2u) { set_error(std::string(who) + ": a CIGAR op other than = X I D"); return false; }
            if (len == 0) { set_error(std::string(who) + ": a CIGAR word of length 0"); return false; }
            if (op != 2u) rows += len;
            if (op != 1u) cols += len;
        }
        // (below 2^28: a merged word's length fits its 28 bits)
        if (cols > j.ref_length || rows > j.query_length || cols >= (1u << 28) || rows >= (1u << 28)) { set_error(std::string(who) + ": the op lengths do not fit the window and the query"); return false; }
    }
    return true;
}

}  // namespace flx
