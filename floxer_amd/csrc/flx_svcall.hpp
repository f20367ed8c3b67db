// Structural-variant calls (flx_svcall, include/floxer_amd.h): the rule, in one place. The judgement of options, records and clusters,
// the span of a record, the window of a cluster in the sorted spans, its count, its genotype and its row (FLX_HD: the kernels of
// flx_svcall.hip run them as they stand) and the whole finish on the host. The one-call C ABI, flx_svcall_host: flx_svcall_api.cpp;
// the object fed run by run, flx_svcaller: flx_svcaller_api.cpp with flx_svcaller.hpp; the tool: floxer_sv_main.cpp. Integers throughout.
//
// Positions are 0-based and local to their sequence, as flx_sv has them.
//   which records count   coverage's filter, coverage_record_counts (flx_coverage.hpp), with count_secondary and min_mapq
//   refused               all that coverage_plan refuses; 2^30 sequences or more (the clusters' keys could not hold their ids)
//   a span                one SortKey (flx_sort.hpp) per counted record: hi = ref << 32 | rs, lo = re, with rs the record's position and
//                         re = rs + the summed = X D lengths. Key order is (ref, rs, re).
//   the clusters          an array of flx_sv_cluster as flx_sv_copy_clusters returns it. Refused: a type above 2, a reference id outside
//                         the lengths (ref_a or ref_b; a DEL or INS whose ref_b is not its ref_a is refused with them), pos_a_min > pos_a_max,
//                         q_min <= q_median <= q_max not holding for a DEL or INS, a DEL with pos_a_max + q_max past its sequence, an
//                         INS with pos_a_max at or past its sequence's end, a non-zero reserved field. BND clusters get no row.
//   the count             for a DEL or INS cluster on sequence r of length n_r: lo = pos_a_min; hi = pos_a_max + q_max (DEL) or
//                         pos_a_max + 1 (INS); lo' = lo >= flank ? lo - flank : 0; hi' = min(hi + flank, n_r); span_n = the spans with
//                         ref == r, rs <= lo' and re >= hi'; alt_n = support; ref_n = span_n > alt_n ? span_n - alt_n : 0;
//                         dp = ref_n + alt_n. flank: 0 takes 50, at most 2^20.
//   the window            with max_span the largest re - rs of all spans, a spanning record has rs >= hi' - max_span (not below 0):
//                         in key order the candidates are the spans from the first with (ref, rs) >= (r, max(hi', max_span) - max_span)
//                         to the last with (ref, rs) <= (r, lo'); of these the ones with re >= hi' count. max_span is one number for
//                         all sequences: one very long record widens every window of the run.
//   the genotype          variants_genotype(ref_n, alt_n, 0, model) of flx_variants.hpp with its five costs and their defaults 36 / 1574
//                         / 325 / 3000 / 3301, the same cost_match < cost_het < cost_mismatch and 2^20 checks; pass = 1 iff gt != RR,
//                         dp >= min_depth (0 takes 4) and qual >= min_qual (0 takes 2000). Conventions of this project, fitted to nothing.
//   the rows              one per DEL / INS cluster in the input's order, failing ones included.
// Known limits: a carrier that does not span the flanks counts in alt_n and not in span_n, so ref_n errs low by at most that many; a
// record with two signatures in one cluster counts twice in alt_n; single linkage is the clusters'; no BND calls; no inserted
// sequence; an event larger than the read's error budget leaves the read unmapped and is never seen.
#pragma once
#include "flx_sv.hpp"
#include "flx_variants.hpp"

namespace flx {

constexpr u32 SVCALL_DEFAULT_FLANK = 50, SVCALL_MAX_FLANK = 1u << 20;

struct SvcallModel { u32 flank; VariantsModel v; };
inline flx_svcall_options svcall_options_or_default(const flx_svcall_options* o) { return o ? *o : flx_svcall_options{}; }
inline flx_variants_options svcall_variants_options(flx_svcall_options const& o) {
    flx_variants_options v{};
    v.count_secondary = o.count_secondary; v.min_mapq = o.min_mapq; v.min_depth = o.min_depth; v.min_qual = o.min_qual;
    v.cost_match = o.cost_match; v.cost_mismatch = o.cost_mismatch; v.cost_het = o.cost_het; v.prior_het = o.prior_het; v.prior_hom = o.prior_hom;
    return v;
}
inline SvcallModel svcall_model(flx_svcall_options const& o) { return SvcallModel{o.flank ? o.flank : SVCALL_DEFAULT_FLANK, variants_model(svcall_variants_options(o))}; }
// NULL is all zero; the reserved fields must be 0; the costs are judged with their defaults taken, as flx_variants judges them
inline bool svcall_options_valid(const flx_svcall_options* o) {
    if (!o) return true;
    for (uint32_t r : o->reserved) if (r) { set_error("flx_svcall_options: the reserved fields must be 0"); return false; }
    if (o->flank > SVCALL_MAX_FLANK) { set_error("flx_svcall_options: flank is above 2^20"); return false; }
    VariantsModel const v = svcall_model(*o).v;
    if (v.m > VARIANTS_MAX_COST || v.x > VARIANTS_MAX_COST || v.h > VARIANTS_MAX_COST || v.prior_het > VARIANTS_MAX_COST || v.prior_hom > VARIANTS_MAX_COST) {
        set_error("flx_svcall_options: a cost is above 2^20");
        return false;
    }
    if (v.h >= v.x || v.m >= v.h) { set_error("flx_svcall_options: the costs must be cost_match < cost_het < cost_mismatch, the model is degenerate otherwise"); return false; }
    return true;
}
inline flx_coverage_options svcall_filter(flx_svcall_options const& o) {
    flx_coverage_options c{};
    c.count_secondary = o.count_secondary;
    c.min_mapq = o.min_mapq;
    return c;
}

// ---- a span
FLX_HD inline SortKey svcall_span_key(u32 ref, u32 rs, u32 re) { return SortKey{(u64)ref << 32 | (u64)rs, (u64)re}; }
FLX_HD inline u32 svcall_span_ref(SortKey const& k) { return (u32)(k.hi >> 32); }
FLX_HD inline u32 svcall_span_rs(SortKey const& k) { return (u32)k.hi; }
FLX_HD inline u32 svcall_span_re(SortKey const& k) { return (u32)k.lo; }
FLX_HD inline bool svcall_op_consumes(u32 op) { return op == 7u || op == 8u || op == 2u; }

// one counted record: where its words lie in the pool it was judged against, its sequence, its position and the end the host expects
struct SvcallJob { u64 word_off; u32 n_words, ref, rs, re; };

// Judges the records (coverage_plan: its refusals, its messages) and appends one job per counted record.
inline bool svcall_plan(std::vector<u64> const& starts, flx_svcall_options const& o, const flx_record* records, uint64_t n, const uint32_t* cigar_words,
                        uint64_t n_words, const char* who, std::vector<SvcallJob>& jobs) {
    std::vector<CoverageJob> judged;
    if (!coverage_plan(starts, svcall_filter(o), records, n, cigar_words, n_words, who, judged)) return false;
    jobs.reserve(jobs.size() + judged.size());
    for (auto const& j : judged) {
        size_t const ref = (size_t)(std::upper_bound(starts.begin(), starts.end(), j.text_off) - starts.begin()) - 1;     // (text_off lies inside its sequence: position + span <= length, span >= 1)
        u64 span = 0;
        for (u32 t = 0; t < j.n_words; ++t) { uint32_t const w = cigar_words[j.word_off + t]; if (svcall_op_consumes(w & 15u)) span += w >> 4; }
        u64 const rs = j.text_off - starts[ref];
        jobs.push_back(SvcallJob{j.word_off, j.n_words, (u32)ref, (u32)rs, (u32)(rs + span)});
    }
    return true;
}
inline SortKey svcall_job_key(SvcallJob const& j) { return svcall_span_key(j.ref, j.rs, j.re); }

// ---- the clusters
inline bool svcall_clusters_valid(std::vector<u64> const& starts, const flx_sv_cluster* clusters, uint64_t n, const char* who, u64& n_rows) {
    size_t const n_refs = starts.size() - 1;
    n_rows = 0;
    for (uint64_t i = 0; i < n; ++i) {
        flx_sv_cluster const& c = clusters[i];
        std::string const cl = std::string(who) + ": cluster " + std::to_string(i);
        if (c.type > SV_BND) { set_error(cl + " has a type above 2"); return false; }
        if (c.reserved) { set_error(cl + " has a non-zero reserved field"); return false; }
        if (c.ref_a < 0 || (size_t)c.ref_a >= n_refs || c.ref_b < 0 || (size_t)c.ref_b >= n_refs) { set_error(cl + " names a reference id outside the lengths"); return false; }
        if (c.pos_a_min > c.pos_a_max) { set_error(cl + " has pos_a_min above pos_a_max"); return false; }
        if (c.type == SV_BND) continue;
        if (c.ref_b != c.ref_a) { set_error(cl + " names a reference id outside the lengths (ref_b of a DEL or INS is ref_a)"); return false; }
        if (c.q_min > c.q_median || c.q_median > c.q_max) { set_error(cl + " does not have q_min <= q_median <= q_max"); return false; }
        u64 const len = starts[(size_t)c.ref_a + 1] - starts[(size_t)c.ref_a];
        if (c.type == SV_DEL && (u64)c.pos_a_max + (u64)c.q_max > len) { set_error(cl + " is a DEL that ends behind its sequence"); return false; }
        if (c.type == SV_INS && (u64)c.pos_a_max >= len) { set_error(cl + " is an INS at or behind its sequence's end"); return false; }
        ++n_rows;
    }
    return true;
}

// ---- the count
// [lo', hi') of a valid DEL or INS cluster on a sequence of n_r symbols: hi <= n_r by the judgement, so lo' < hi' <= n_r
FLX_HD inline void svcall_bounds(flx_sv_cluster const& c, u32 n_r, u32 flank, u32& lo2, u32& hi2) {
    u64 const hi = c.type == SV_DEL ? (u64)c.pos_a_max + (u64)c.q_max : (u64)c.pos_a_max + 1ull;
    lo2 = c.pos_a_min >= flank ? c.pos_a_min - flank : 0u;
    u64 const reach = hi + (u64)flank;
    hi2 = reach < (u64)n_r ? (u32)reach : n_r;
}
// the first index in [0, n) whose key's hi is at least `target` (n when none is): hi(i) reads the hi of key i
template <class Hi>
FLX_HD inline u64 svcall_lower_bound(u64 n, u64 target, Hi&& hi) {
    u64 a = 0, b = n;
    while (a < b) {
        u64 const mid = a + (b - a) / 2;
        if (hi(mid) < target) a = mid + 1; else b = mid;
    }
    return a;
}
// the window [first, last) of the sorted spans that holds every span of sequence r with rs <= lo' that can reach hi'
template <class Hi>
FLX_HD inline void svcall_window(u64 n, u32 r, u32 lo2, u32 hi2, u32 max_span, Hi&& hi, u64& first, u64& last) {
    u32 const from = (hi2 > max_span ? hi2 : max_span) - max_span;
    first = svcall_lower_bound(n, (u64)r << 32 | (u64)from, hi);
    last = svcall_lower_bound(n, ((u64)r << 32 | (u64)lo2) + 1ull, hi);
    if (last < first) last = first;                                     // (no span is long enough to start at or before lo' and reach hi')
}
// the row of cluster `index` with span_n spanning records
FLX_HD inline flx_svcall_row svcall_row(u32 index, flx_sv_cluster const& c, u32 span_n, SvcallModel const& m) {
    u32 const alt_n = c.support, ref_n = span_n > alt_n ? span_n - alt_n : 0u;
    u64 const dp = (u64)ref_n + (u64)alt_n;
    VariantGenotype const g = variants_genotype(ref_n, alt_n, 0, m.v);
    flx_svcall_row row;
    row.cluster = index; row.type = c.type; row.ref = c.ref_a;
    row.pos_a_min = c.pos_a_min; row.pos_a_max = c.pos_a_max;
    row.q_min = c.q_min; row.q_median = c.q_median; row.q_max = c.q_max;
    row.alt_n = alt_n; row.ref_n = ref_n; row.span_n = span_n;
    row.gt = g.gt; row.gq = g.gq; row.qual = g.qual;
    row.pl[0] = g.pl[0]; row.pl[1] = g.pl[1]; row.pl[2] = g.pl[2];
    row.pass = variants_row_stands(g, dp, m.v) ? 1u : 0u;
    return row;
}

// ---- the finish on the host: spans in any order (sorted here), clusters judged by the caller
inline void svcall_finish_host(std::vector<u64> const& starts, std::vector<SortKey>& spans, const flx_sv_cluster* clusters, uint64_t n, SvcallModel const& m,
                               std::vector<flx_svcall_row>& rows) {
    std::sort(spans.begin(), spans.end(), [](SortKey const& a, SortKey const& b) { return sort_key_less(a, b); });
    u32 max_span = 0;
    for (auto const& s : spans) max_span = std::max(max_span, svcall_span_re(s) - svcall_span_rs(s));
    auto hi = [&](u64 i) { return spans[i].hi; };
    for (uint64_t i = 0; i < n; ++i) {
        flx_sv_cluster const& c = clusters[i];
        if (c.type == SV_BND) continue;
        u32 lo2, hi2;
        svcall_bounds(c, (u32)(starts[(size_t)c.ref_a + 1] - starts[(size_t)c.ref_a]), m.flank, lo2, hi2);
        u64 first, last;
        svcall_window(spans.size(), (u32)c.ref_a, lo2, hi2, max_span, hi, first, last);
        u32 span_n = 0;
        for (u64 k = first; k < last; ++k) span_n += svcall_span_re(spans[k]) >= hi2;
        rows.push_back(svcall_row((u32)i, c, span_n, m));
    }
}

}  // namespace flx
