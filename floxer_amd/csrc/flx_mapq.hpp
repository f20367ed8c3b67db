// Mapping quality from a read's distinct loci (flx_output_options.mapq, include/floxer_amd.h). Host code only, integer arithmetic
// only; used by the record stage of the pipeline (keyed on the unsaturated start) and by flx_assign_mapq (keyed on the record's
// position), so the rule has one implementation. It runs on all of a read's records, before flx_select.hpp selects among them.
//
// The rule, for the records of one read in output order:
//   1. Mapped records only. A record covers [start, start + span) on (reference id, strand), span = the reference symbols its CIGAR
//      consumes ('=', 'X', 'D'), or the read's length for a record without CIGAR; a span of 0 counts as 1.
//   2. Loci: the records sorted by (reference id, strand, start, output index) are swept with a running maximum end; a record that
//      starts below the running end of the current group on the same (reference, strand) joins it, any other opens a new locus
//      (abutting intervals are two loci). A locus' NM is the smallest NM of its records.
//   3. L0 = the locus of the primary record (neither flag bit 256 nor 4), b = its NM, n = the number of loci with NM == b,
//      s = the smallest NM above b among the loci:
//        n >= 2              q = 3, 2, 1 for n = 2, 3, 4 (-10 log10(1 - 1/n), rounded) and 0 for n >= 5
//        n == 1, one locus   q = 60
//        n == 1 otherwise    q = min(60, 10 * (s - b))
//      The factor 10 is a convention of this project: it is not fitted to anything and nobody has measured its calibration.
//   4. Every record of L0 gets q, every other record 0 (the unmapped record of a read too). Records the pipeline never forms: a read
//      without a primary record has no L0 (all 0), the first of several primaries counts, and a primary whose locus is the only one
//      of its NM while every other locus has a smaller NM gets 0.
//
// Limits: verification is exhaustive within the read's error budget, so "no other locus" means none with at most k errors and none
// lost to the hard anchor cap (-M): a locus with k + 1 errors is not seen, and a seed that the cap excluded hides the loci only it
// led to. With --interval-optimization the loci are the same, only the records per locus are fewer.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "flx_internal.hpp"

namespace flx {

struct MapqKey {              // one record of a read, in output order
    uint64_t start;           // start in the reference
    uint64_t span;            // reference symbols covered (0 counts as 1)
    int32_t ref;              // -1: the unmapped record
    uint32_t flag;
    uint32_t nm;
};

struct MapqScratch {
    std::vector<uint32_t> order, locus_of, locus_nm;
    struct Span { const uint32_t* cigar; uint32_t len; uint64_t span; };
    std::vector<Span> spans;  // of the read at hand: records of one union share their CIGAR words, so a read has a few entries
};

inline uint64_t cigar_reference_span(const uint32_t* cigar, uint32_t n) {
    // (no branch on the operation: a read's CIGAR alternates between its four operations as its errors fall, and a mispredicted
    // branch per word made this loop the option's whole cost; 0x184 has the bits of 'D' = 2, '=' = 7 and 'X' = 8)
    uint64_t span = 0;
    for (uint32_t c = 0; c < n; ++c) span += (uint64_t)(cigar[c] >> 4) * ((0x184u >> (cigar[c] & 15u)) & 1u);
    return span;
}

// the same, summed once per (words, length) of a read: call s.spans.clear() when a read begins
inline uint64_t cigar_reference_span_cached(const uint32_t* cigar, uint32_t n, MapqScratch& s) {
    for (auto const& e : s.spans) if (e.cigar == cigar && e.len == n) return e.span;
    uint64_t const span = cigar_reference_span(cigar, n);
    s.spans.push_back(MapqScratch::Span{cigar, n, span});
    return span;
}

// q[i] = the mapping quality of record i of the read (rule above)
inline void read_mapq(const MapqKey* k, size_t n, uint8_t* q, MapqScratch& s) {
    for (size_t i = 0; i < n; ++i) q[i] = 0;
    s.order.clear();
    size_t primary = n;
    for (size_t i = 0; i < n; ++i) {
        if (k[i].flag & 4u) continue;
        s.order.push_back((uint32_t)i);
        if (primary == n && !(k[i].flag & 256u)) primary = i;
    }
    if (primary == n) return;
    {
        // The common case without a sort: all records on one (reference, strand) and every interval meets the first record's. Sorted by
        // start, each of them then starts below the end of a record in front of it (the first record's, or one that reaches over the
        // first record's start), so the sweep below would make one locus of them.
        MapqKey const& f = k[s.order[0]];
        uint64_t const f_end = f.start + (f.span ? f.span : 1);
        bool one_locus = true;
        for (size_t j = 1; j < s.order.size() && one_locus; ++j) {
            MapqKey const& r = k[s.order[j]];
            one_locus = r.ref == f.ref && (r.flag & 16u) == (f.flag & 16u) && r.start < f_end && r.start + (r.span ? r.span : 1) > f.start;
        }
        if (one_locus) {
            for (uint32_t i : s.order) q[i] = 60;
            return;
        }
    }
    std::sort(s.order.begin(), s.order.end(), [&](uint32_t a, uint32_t b) {
        if (k[a].ref != k[b].ref) return k[a].ref < k[b].ref;
        if ((k[a].flag & 16u) != (k[b].flag & 16u)) return (k[a].flag & 16u) < (k[b].flag & 16u);
        if (k[a].start != k[b].start) return k[a].start < k[b].start;
        return a < b;
    });
    s.locus_of.resize(n);
    s.locus_nm.clear();
    uint64_t end = 0;
    for (size_t j = 0; j < s.order.size(); ++j) {
        MapqKey const& r = k[s.order[j]];
        uint64_t const r_end = r.start + (r.span ? r.span : 1);
        bool joins = false;
        if (j) {
            MapqKey const& p = k[s.order[j - 1]];
            joins = p.ref == r.ref && (p.flag & 16u) == (r.flag & 16u) && r.start < end;
        }
        if (joins) {
            end = std::max(end, r_end);
            s.locus_nm.back() = std::min(s.locus_nm.back(), r.nm);
        } else {
            end = r_end;
            s.locus_nm.push_back(r.nm);
        }
        s.locus_of[s.order[j]] = (uint32_t)s.locus_nm.size() - 1;
    }
    uint32_t const l0 = s.locus_of[primary], b = s.locus_nm[l0];
    uint64_t ties = 0, second = UINT64_MAX;
    for (uint32_t nm : s.locus_nm) {
        if (nm == b) ++ties;
        else if (nm > b && nm < second) second = nm;
    }
    uint8_t quality;
    if (ties >= 2) quality = ties == 2 ? 3 : ties == 3 ? 2 : ties == 4 ? 1 : 0;
    else if (s.locus_nm.size() == 1) quality = 60;
    else quality = second == UINT64_MAX ? 0 : (uint8_t)std::min<uint64_t>(60, 10 * (second - b));   // (no s: see rule 4)
    for (uint32_t i : s.order) if (s.locus_of[i] == l0) q[i] = quality;
}

}  // namespace flx
