// The cs tag (flx_cs_options, include/floxer_amd.h): minimap2's difference string of a traced path, short and long form. Host code only:
// the rule on one path, used by flx_cs (flx_capi_host.cpp), by the checks of flx_cs_batch and by the tests; the kernel cs_build
// (flx_cs.hip) writes the same bytes on the device behind md_build, from the words K5 (or cigar_realign / cigar_left_align) left there.
//
// A path is a list of words (op, len), ops = (7) X (8) I (1) D (2), over a reference window, a query and `begin`, the window column of
// the path's first column; the query is the record's oriented sequence from its first traced row on. The walk goes left to right and
// every word emits on its own (nothing merges across words, which is where cs differs from MD):
//   = of length L   short form (1): ':' and L in decimal; long form (2): '=' and the L reference letters in upper case (they equal the
//                   query's by construction)
//   X of length L   per column '*', the reference letter, the query letter, lower case: 3 L bytes, in both forms
//   I of length L   '+' and the L query letters, lower case
//   D of length L   '-' and the L reference letters, lower case
// Letters are ranks: 1..4 give acgt / ACGT, anything else (0 and 5 included) n / N, the limit MD has: IUPAC codes and lower-case FASTA
// letters are not recoverable. Nothing is compared again: an X over equal ranks is emitted as it stands. There is no '~' (no introns).
// Soft clips are not part of a path and emit nothing. minimap2's own example has this shape: :6-ata:10+gtc:4*at:3.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "flx_internal.hpp"

namespace flx {

// NULL is no options; form must be 0, 1 or 2 and the reserved fields 0
inline bool cs_options_valid(const flx_cs_options* o) {
    if (!o) return true;
    if (o->form > 2) { set_error("flx_cs_options: form must be 0 (off), 1 (short) or 2 (long)"); return false; }
    for (uint32_t r : o->reserved) if (r) { set_error("flx_cs_options: the reserved fields must be 0"); return false; }
    return true;
}
inline uint32_t cs_options_form(const flx_cs_options* o) { return o ? o->form : 0u; }

inline uint8_t cs_letter(uint8_t rank, bool upper) {                   // 1..4 -> acgt / ACGT, else n / N
    static const char lower[4] = {'a', 'c', 'g', 't'};
    uint8_t const c = (uint8_t)(rank >= 1 && rank <= 4 ? lower[rank - 1] : 'n');
    return upper ? (uint8_t)(c - 32) : c;
}
inline uint32_t cs_dec_digits(uint32_t v) {
    uint32_t d = 1;
    while (v >= 10u) { v /= 10u; ++d; }
    return d;
}
// bytes one word emits: a function of (op, len, form) alone
inline uint64_t cs_word_bytes(uint32_t op, uint32_t len, uint32_t form) {
    if (op == 7u) return form == 2u ? 1ull + len : 1ull + cs_dec_digits(len);
    if (op == 8u) return 3ull * len;
    if (op == 1u || op == 2u) return 1ull + len;
    return 0;
}
inline uint64_t cs_path_bytes(const uint32_t* words, uint64_t n_words, uint32_t form) {
    uint64_t bytes = 0;
    for (uint64_t t = 0; t < n_words; ++t) bytes += cs_word_bytes(words[t] & 15u, words[t] >> 4, form);
    return bytes;
}

// The rule on the words [words, words + n_words): ref / query point at the window's first letter / the path's first query row. The
// caller has judged the words (left_align_jobs_valid: ops = X I D, no zero length, the path inside the window and the query). The
// string is appended to `out`.
inline void cs_path(const uint32_t* words, uint64_t n_words, const uint8_t* ref, const uint8_t* query, uint32_t begin, uint32_t form, std::vector<uint8_t>& out) {
    uint64_t r = begin, q = 0;
    for (uint64_t t = 0; t < n_words; ++t) {
        uint32_t const op = words[t] & 15u, len = words[t] >> 4;
        if (op == 7u) {
            if (form == 2u) {
                out.push_back((uint8_t)'=');
                for (uint32_t c = 0; c < len; ++c) out.push_back(cs_letter(ref[r + c], true));
            } else {
                std::string const num = std::to_string(len);
                out.push_back((uint8_t)':');
                out.insert(out.end(), num.begin(), num.end());
            }
            r += len; q += len;
        } else if (op == 8u) {
            for (uint32_t c = 0; c < len; ++c) {
                out.push_back((uint8_t)'*');
                out.push_back(cs_letter(ref[r + c], false));
                out.push_back(cs_letter(query[q + c], false));
            }
            r += len; q += len;
        } else if (op == 1u) {
            out.push_back((uint8_t)'+');
            for (uint32_t c = 0; c < len; ++c) out.push_back(cs_letter(query[q + c], false));
            q += len;
        } else if (op == 2u) {
            out.push_back((uint8_t)'-');
            for (uint32_t c = 0; c < len; ++c) out.push_back(cs_letter(ref[r + c], false));
            r += len;
        }
    }
}

}  // namespace flx
