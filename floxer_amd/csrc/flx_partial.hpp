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
//   7. Extension to the break (flx_extend_options; the stage extend_partials of flx_verify.cpp, kernel ed_extend in flx_extend.hip),
//      after the selection, on the kept records only; all coordinates in the record's oriented sequence. Each kept record has two
//      ends, each end is one job, independent of every other:
//      - start cell: right end - the query row behind the traced part's last row and the reference symbol behind its last reference
//        column (start + the CIGAR's reference span); left end - the mirror image, both sequences walked backwards from the row and
//        the symbol in front of the traced part;
//      - limits: at most I_max rows, the rows up to the read's end, or, when another kept record of the read lies on that side
//        (forward coordinates), the rows up to that record's original node interval; at most J_max symbols, up to the end of this
//        reference sequence (never across a sequence boundary of the concatenated text). Two extensions may meet or overlap inside
//        the gap between two records (microhomology at a break); an extension never enters another kept record's node interval;
//      - score: D[i][j] = unit-cost edit distance between the first i rows and the first j symbols from the start cell, D[0][0] = 0,
//        symbols match when their ranks are equal; m(i) = min_j D[i][j] (non-decreasing, at most +1 per row);
//        R(d) = max{i <= I_max : m(i) <= d}; score(d) = R(d) - w d;
//      - scan d = 0, 1, 2, .. keeping the running maximum G and the first d that reached it; stop at the first d with
//        G - score(d) > X (x-drop), R(d) == I_max, or d == d_max;
//      - result: d* = the first d that reached G, i* = R(d*), j* = the smallest j with D[i*][j] == d*; i* == 0: the end does not move;
//      - defaults w = 4, X = 100, d_max = 1024: conventions of this project, not fitted to anything. A peak behind a valley deeper
//        than X, or behind d_max errors, is not found;
//      - a record whose ends moved by (iL, jL, dL) and (iR, jR, dR) is traced again by run_trace_jobs_union: query rows
//        [from - iL, to + iR], reference window exactly [start - jL, end + jR], k = nm + dL + dR. An alignment exists by construction
//        (FLX_ERR_INTERNAL otherwise); position, NM, the CIGAR core and the MD come from that trace (so NM <= nm + dL + dR), the soft
//        clips are what remains of the read, q_from / q_to follow the new interval. Records whose ends did not move keep their
//        words; the mapping quality keeps the value computed before the extension; flags, the order of a read's records and the
//        counters do not change.
//
// Limits: without the extension a record ends at a PEX node's boundary, not at the break. A read mapped in full that also carries a
// chimeric tail is the business of flx_split_options (flx_tails.hpp, the stage split_tails): its records come through choose_partials,
// extend_partials and the writer like the ones made here. The SA tag that ties a read's records together is the writer's (flx_sam_set_sa).
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

// flx_extend_options: NULL is no options; enable must be 0 or 1, the reserved fields 0 and the three values within what ed_extend holds
inline bool extend_options_valid(const flx_extend_options* o) {
    if (!o) return true;
    if (o->enable > 1) { set_error("flx_extend_options: enable must be 0 or 1"); return false; }
    for (uint32_t r : o->reserved) if (r) { set_error("flx_extend_options: the reserved fields must be 0"); return false; }
    if (o->max_errors > EXTEND_MAX_ERRORS) { set_error("flx_extend_options: max_errors is larger than the 4093 the extension kernel's wavefronts hold in LDS"); return false; }
    if (o->error_weight > EXTEND_MAX_WEIGHT) { set_error("flx_extend_options: error_weight must be at most 65535"); return false; }
    if (o->x_drop > EXTEND_MAX_XDROP) { set_error("flx_extend_options: x_drop must be at most 2^30"); return false; }
    return true;
}
inline bool extend_options_active(const flx_extend_options* o) { return o && o->enable; }
inline uint32_t extend_weight(uint32_t v) { return v ? v : EXTEND_DEFAULT_WEIGHT; }
inline uint32_t extend_x_drop(uint32_t v) { return v ? v : EXTEND_DEFAULT_XDROP; }
inline uint32_t extend_max_errors(uint32_t v) { return v ? v : EXTEND_DEFAULT_MAX_ERRORS; }

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
