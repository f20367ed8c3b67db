// Output options (flx_output_options, include/floxer_amd.h): which records of one read are written. Host code only; used by the
// record stage of the pipeline (keyed on the unsaturated start) and by flx_select_records (keyed on the record's position), so the
// rule has one implementation.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "flx_internal.hpp"

namespace flx {

struct SelectKey {            // one record of a read, in output order
    uint64_t start;           // start in the reference
    int32_t ref;              // -1: the unmapped record
    uint32_t flag;
    uint32_t nm;
    uint32_t cigar_len;
    const uint32_t* cigar;
};

struct SelectScratch { std::vector<uint64_t> hash; std::vector<uint32_t> order, kept; };

// NULL is no options; the reserved fields must be 0 and mapq 0 or 1 (set_error otherwise)
inline bool output_options_valid(const flx_output_options* o) {
    if (o && (o->reserved2[0] || o->reserved2[1])) { set_error("flx_output_options: the reserved fields must be 0"); return false; }
    if (o && o->mapq > 1) { set_error("flx_output_options: mapq must be 0 or 1"); return false; }
    return true;
}
inline bool output_options_active(const flx_output_options* o) { return o && (o->drop_duplicates || o->max_alignments_per_read); }
// flx_tag_options: NULL or zeroed is no tags; md must be 0 or 1 and the reserved fields 0 (set_error otherwise)
inline bool tag_options_valid(const flx_tag_options* t) {
    if (!t) return true;
    if (t->md > 1) { set_error("flx_tag_options: md must be 0 or 1"); return false; }
    for (uint32_t r : t->reserved) if (r) { set_error("flx_tag_options: the reserved fields must be 0"); return false; }
    return true;
}

// (records of one union share their CIGAR words: the same words compare equal without reading them)
inline bool select_same(SelectKey const& a, SelectKey const& b) {
    return a.ref == b.ref && (a.flag & 16u) == (b.flag & 16u) && a.start == b.start && a.nm == b.nm && a.cigar_len == b.cigar_len &&
           (a.cigar_len == 0 || a.cigar == b.cigar || memcmp(a.cigar, b.cigar, (size_t)a.cigar_len * 4) == 0);
}

// buckets for select_same: the key fields and the CIGAR's first and last four words (a 10-kb read's CIGAR is ~1600 words and a read
// has ~40 records: hashing every word cost more than the rest of the record stage; records of one bucket are compared in full)
inline uint64_t select_hash(SelectKey const& k) {
    auto mix = [](uint64_t h, uint64_t v) { h ^= v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2); return h * 0xff51afd7ed558ccdull; };
    uint64_t h = mix(mix(mix(mix(0, (uint64_t)(uint32_t)k.ref), k.flag & 16u), k.start), ((uint64_t)k.nm << 32) | k.cigar_len);
    uint32_t const head = k.cigar_len < 4 ? k.cigar_len : 4;
    for (uint32_t i = 0; i < head; ++i) h = mix(h, k.cigar[i]);
    for (uint32_t i = k.cigar_len > 8 ? k.cigar_len - 4 : head; i < k.cigar_len; ++i) h = mix(h, k.cigar[i]);
    return h;
}

// keep[i] = 1 for the records of the read that are written, 0 for the others (rules of flx_output_options)
inline void select_read_records(const SelectKey* k, size_t n, bool drop_duplicates, uint64_t max_per_read, uint8_t* keep, SelectScratch& s) {
    for (size_t i = 0; i < n; ++i) keep[i] = 1;
    // (a read with a supplementary record carries partial alignments: they are selected already, flx_partial.hpp)
    for (size_t i = 0; i < n; ++i) if (k[i].flag & 2048u) return;
    if (drop_duplicates && n > 1) {
        // records in (hash, index) order: a class of equal records lies in one run of equal hashes, its first record first
        s.hash.resize(n);
        s.order.clear();
        for (size_t i = 0; i < n; ++i)
            if (!(k[i].flag & 4u)) { s.hash[i] = select_hash(k[i]); s.order.push_back((uint32_t)i); }
        std::sort(s.order.begin(), s.order.end(), [&](uint32_t a, uint32_t b) { return s.hash[a] != s.hash[b] ? s.hash[a] < s.hash[b] : a < b; });
        for (size_t lo = 0; lo < s.order.size();) {
            size_t hi = lo + 1;
            while (hi < s.order.size() && s.hash[s.order[hi]] == s.hash[s.order[lo]]) ++hi;
            for (size_t j = lo + 1; j < hi; ++j)
                for (size_t e = lo; e < j; ++e)
                    if (keep[s.order[e]] && select_same(k[s.order[e]], k[s.order[j]])) { keep[s.order[j]] = 0; break; }
            lo = hi;
        }
    }
    if (max_per_read) {
        s.kept.clear();
        for (size_t i = 0; i < n; ++i) if (keep[i] && !(k[i].flag & 4u)) s.kept.push_back((uint32_t)i);
        if (s.kept.size() > max_per_read) {
            auto less = [&](uint32_t a, uint32_t b) { return k[a].nm != k[b].nm ? k[a].nm < k[b].nm : a < b; };
            std::nth_element(s.kept.begin(), s.kept.begin() + (long)max_per_read, s.kept.end(), less);
            for (size_t j = max_per_read; j < s.kept.size(); ++j) keep[s.kept[j]] = 0;
        }
    }
}

}  // namespace flx
