// Partial alignments of reads that would be written as unmapped (flx_partial_options, include/floxer_amd.h). Host code only; used by
// the rescue_partials stage of the pipeline (flx_verify.cpp) and by flx_choose_partials / flx_partial_mapq (flx_capi_host.cpp), so the
// rule has one implementation.
//
// floxer maps a read only when its whole length aligns within ceil(len * p) errors. A chimeric read, or one across a structural break,
// leaves verification unmapped although its anchors proved on their way up the PEX tree that a half or a quarter of it aligns: every
// node below the one an anchor failed at passed an existence test in a known window. The rule, for a read that is not skipped and has
// no mapped record:
//   1. Candidate of an anchor: the highest node on its leaf-to-root path that it passed - the child (on that path) of the node it
//      failed at, or of the root when it reached the root and the root alignment failed. A leaf counts as passed. With direct full
//      verification nothing climbs and the candidates are the leaves.
//   2. A candidate counts when its node has at least min_query_span rows (0: 1000, a convention of this project: it is not fitted to
//      anything).
//   3. It is traced in exactly the window it was tested in (no extension, k = the node's errors), so an alignment exists. Identical
//      (orientation, node, reference, window) candidates are one.
//   4. Selection (choose_partials below) on the traced candidates of a read, each with its query interval in read-forward coordinates
//      (node [from, to] of the reverse complement is [len - 1 - to, len - 1 - from]): candidates equal in (orientation, reference,
//      start, NM, CIGAR words) to an earlier one are dropped; the rest is ordered by (rows descending, NM ascending, reference id,
//      verification order) and taken greedily: the first is the primary, a later one is kept as supplementary (flag 2048) when its
//      interval overlaps no kept one, until max_records (0: 4) are kept. They are written primary first, then by forward query start.
//   5. A kept record's CIGAR is [from]S + traced words + [rows behind the node]S in the oriented sequence; NM and MD tell of the traced
//      part only.
//   6. Mapping quality (flx_output_options.mapq): read_mapq (flx_mapq.hpp) over the read's candidates (after the duplicates are dropped)
//      with exactly the kept record's forward interval, the kept record as the primary.
//
// Limits: the clip boundary is a PEX node's boundary, not the true break; a read mapped in full that also carries a chimeric tail is
// not touched; no SA tag is written.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "flx_internal.hpp"
#include "flx_mapq.hpp"

namespace flx {

constexpr uint32_t PARTIAL_DEFAULT_MIN_SPAN = 1000, PARTIAL_DEFAULT_MAX_RECORDS = 4;

// NULL is no options; enable must be 0 or 1 and the reserved fields 0 (set_error otherwise)
inline bool partial_options_valid(const flx_partial_options* o) {
    if (!o) return true;
    if (o->enable > 1) { set_error("flx_partial_options: enable must be 0 or 1"); return false; }
    for (uint32_t r : o->reserved) if (r) { set_error("flx_partial_options: the reserved fields must be 0"); return false; }
    return true;
}
inline bool partial_options_active(const flx_partial_options* o) { return o && o->enable; }
inline uint32_t partial_min_span(const flx_partial_options* o) { return o && o->min_query_span ? o->min_query_span : PARTIAL_DEFAULT_MIN_SPAN; }
inline uint32_t partial_max_records(const flx_partial_options* o) { return o && o->max_records ? o->max_records : PARTIAL_DEFAULT_MAX_RECORDS; }

struct PartialScratch { std::vector<uint32_t> order, kept; std::vector<MapqKey> keys; std::vector<uint32_t> key_of; std::vector<uint8_t> q; MapqScratch mapq; };

inline bool partial_same(flx_partial_candidate const& a, flx_partial_candidate const& b, const uint32_t* words) {
    if (a.orientation != b.orientation || a.reference_id != b.reference_id || a.start != b.start || a.nm != b.nm || a.cigar_length != b.cigar_length) return false;
    if (a.cigar_length == 0 || a.cigar_offset == b.cigar_offset) return true;
    return words && memcmp(words + a.cigar_offset, words + b.cigar_offset, (size_t)a.cigar_length * 4) == 0;
}

// flag[i] = -1 for a candidate of the read that is not written, else its SAM flag (0 / 16 the primary, 2048 / 2064 a supplementary).
// c: the read's traced candidates in verification order; s.kept receives the kept ones in the order they are written in.
inline void choose_partials(const flx_partial_candidate* c, size_t n, uint32_t max_records, const uint32_t* words, int32_t* flag, PartialScratch& s) {
    s.order.clear();
    s.kept.clear();
    for (size_t i = 0; i < n; ++i) {
        flag[i] = -1;
        bool dup = false;
        for (uint32_t e : s.order) if (partial_same(c[e], c[i], words)) { dup = true; break; }
        if (!dup && c[i].q_to >= c[i].q_from) s.order.push_back((uint32_t)i);
    }
    auto rows = [&](uint32_t i) { return c[i].q_to - c[i].q_from + 1; };
    std::sort(s.order.begin(), s.order.end(), [&](uint32_t a, uint32_t b) {
        if (rows(a) != rows(b)) return rows(a) > rows(b);
        if (c[a].nm != c[b].nm) return c[a].nm < c[b].nm;
        if (c[a].reference_id != c[b].reference_id) return c[a].reference_id < c[b].reference_id;
        return a < b;
    });
    for (uint32_t i : s.order) {
        if (s.kept.size() >= max_records) break;
        bool overlaps = false;
        for (uint32_t e : s.kept) if (c[i].q_from <= c[e].q_to && c[e].q_from <= c[i].q_to) { overlaps = true; break; }
        if (overlaps) continue;
        flag[i] = (int32_t)((s.kept.empty() ? 0u : 2048u) | (c[i].orientation ? 16u : 0u));
        s.kept.push_back(i);
    }
    if (s.kept.size() > 2) std::sort(s.kept.begin() + 1, s.kept.end(), [&](uint32_t a, uint32_t b) { return c[a].q_from < c[b].q_from; });
}

// q[i] = the mapping quality of every kept candidate (flag[i] >= 0) of the read, 0 for the others (rule 6 above)
inline void partial_mapq(const flx_partial_candidate* c, size_t n, const uint32_t* words, const int32_t* flag, uint8_t* q, PartialScratch& s) {
    for (size_t i = 0; i < n; ++i) q[i] = 0;
    for (size_t i = 0; i < n; ++i) {
        if (flag[i] < 0) continue;
        s.keys.clear();
        s.key_of.clear();
        s.mapq.spans.clear();
        size_t own = 0;
        for (size_t j = 0; j < n; ++j) {
            if (c[j].q_from != c[i].q_from || c[j].q_to != c[i].q_to) continue;
            bool dup = false;
            if (j != i) for (uint32_t e : s.key_of) if (e != i && partial_same(c[e], c[j], words)) { dup = true; break; }
            if (j != i && (dup || partial_same(c[i], c[j], words))) continue;
            uint64_t const span = c[j].cigar_length && words ? cigar_reference_span_cached(words + c[j].cigar_offset, c[j].cigar_length, s.mapq)
                                                             : (uint64_t)(c[j].q_to - c[j].q_from + 1);
            if (j == i) own = s.keys.size();
            s.keys.push_back(MapqKey{c[j].start, span, c[j].reference_id, (c[j].orientation ? 16u : 0u) | (j == i ? 0u : 256u), c[j].nm});
            s.key_of.push_back((uint32_t)j);
        }
        s.q.resize(s.keys.size());
        read_mapq(s.keys.data(), s.keys.size(), s.q.data(), s.mapq);
        q[i] = s.q[own];
    }
}

}  // namespace flx
