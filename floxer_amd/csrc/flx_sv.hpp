// Structural-variant signatures (flx_sv, include/floxer_amd.h): the rule, in one place, for the host and the device. The judgement of
// options, lengths and records that flx_sv_host, flx_sv_add_records and flx_sv_add_run share, the walk and the junctions for the host
// hook, the key with its pack and unpack functions, and the clustering. The kernels (flx_sv.hip) pack keys and make junctions with the
// same functions; the object and the C ABI: flx_sv_api.cpp.
//
// Words are len << 4 | op with = 7, X 8, I 1, D 2, S 4. Positions are 0-based and local to their sequence, never in the concatenation.
//   which records count   coverage's filter, coverage_record_counts (flx_coverage.hpp), with count_secondary and min_mapq
//   a signature           type, ref_a, side_a, ref_b, side_b, pos_a, q:
//     DEL (type 0)        every D word of a counted record with len >= min_length: pos_a its first deleted column, q = len, ref_b = ref_a,
//                         both sides 0
//     INS (type 1)        every I word with len >= min_length: pos_a is pileup's anchor (the position of the record's preceding
//                         reference-consuming column, or the record's first reference-consuming column when none precedes the word),
//                         q = len, ref_b = ref_a, both sides 0
//     BND (type 2)        one per pair of query-neighbouring records of a read. A read's group is the maximal run of neighbouring records
//                         of the given array with equal read_index; its members are the group's counted records with flag & 256 clear
//                         (secondaries never form junctions); each has a query interval on the read as given (with flag & 16:
//                         [trail, read_len - lead), else [lead, read_len - trail), lead and trail the S words in front of the first and
//                         behind the last other word); members are ordered by (query_start, index in the array). Each consecutive pair
//                         (a, b) gives one junction of two ends, with rs = position and re = position + the summed = X D lengths:
//                           the end of a: (ref_a, re_a - 1, side R = 1) when a is forward, (ref_a, rs_a, side L = 0) when a is reverse
//                           the end of b: (ref_b, rs_b, L) when b is forward, (ref_b, re_b - 1, R) when b is reverse
//                         The two ends are put in ascending (ref, pos, side) order: the smaller is end a and its position pos_a, the other's
//                         position is q. A read and its reverse complement, mapped to the same places, so give equal signatures.
//   refused               all that coverage_plan refuses; a read_index outside the reads; query-consuming lengths that do not sum to the
//                         read's length (or sum to 2^31 or more); no reference-consuming column; an S word with other words on both
//                         sides; a group of more than 64 members; 2^30 sequences or more
//   the key               one SortKey (flx_sort.hpp), compared ascending as (hi, lo):
//                           hi = type << 62 | side_a << 61 | side_b << 60 | ref_a << 30 | ref_b        (the class)
//                           lo = pos_a << 32 | q
//   clusters              two levels over the signatures in key order. (1) A coarse group breaks between neighbours whose class differs
//                         or whose pos_a differ by more than max_distance. (2) Within a coarse group, in (q, pos_a) order, a cluster
//                         breaks where q differs from its predecessor by more than max_distance. A cluster reports its class, support
//                         (its members), pos_a_min, pos_a_max, q_min, q_max and q_median, the q of member (support - 1) / 2 in that order.
//                         Clusters come in the order of (2); those with support < min_support are dropped. Single linkage: a chain of
//                         close signatures can span more than max_distance end to end.
//   defaults              0 takes min_length 50, max_distance 100, min_support 2: conventions of this project, fitted to nothing.
// Equal keys are interchangeable: both tables are functions of the multiset of signatures alone.
#pragma once
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "flx_coverage.hpp"
#include "flx_paf.hpp"
#include "flx_sort.hpp"

namespace flx {

constexpr u32 SV_DEL = 0, SV_INS = 1, SV_BND = 2;
constexpr u32 SV_DEFAULT_MIN_LENGTH = 50, SV_DEFAULT_MAX_DISTANCE = 100, SV_DEFAULT_MIN_SUPPORT = 2;
constexpr u32 SV_MAX_GROUP = 64;                       // members of a read's group
constexpr u64 SV_MAX_REFS = 1ull << 30;                // reference ids lie below
constexpr u64 SV_MAX_SIGNATURES = (1ull << 32) - 1;
constexpr u32 SV_VIOLATION = 0xFFFFFFFFu;              // the kernel's mark in the `mark` field of a segment it could not make

// ---- the key
FLX_SORT_HD SortKey sv_key(uint32_t type, uint32_t side_a, uint32_t side_b, uint32_t ref_a, uint32_t ref_b, uint32_t pos_a, uint32_t q) {
    return SortKey{(uint64_t)type << 62 | (uint64_t)(side_a & 1u) << 61 | (uint64_t)(side_b & 1u) << 60 | (uint64_t)ref_a << 30 | (uint64_t)ref_b,
                   (uint64_t)pos_a << 32 | (uint64_t)q};
}
FLX_SORT_HD uint32_t sv_key_type(SortKey const& k) { return (uint32_t)(k.hi >> 62); }
FLX_SORT_HD uint32_t sv_key_side_a(SortKey const& k) { return (uint32_t)(k.hi >> 61) & 1u; }
FLX_SORT_HD uint32_t sv_key_side_b(SortKey const& k) { return (uint32_t)(k.hi >> 60) & 1u; }
FLX_SORT_HD uint32_t sv_key_ref_a(SortKey const& k) { return (uint32_t)(k.hi >> 30) & 0x3FFFFFFFu; }
FLX_SORT_HD uint32_t sv_key_ref_b(SortKey const& k) { return (uint32_t)k.hi & 0x3FFFFFFFu; }
FLX_SORT_HD uint32_t sv_key_pos_a(SortKey const& k) { return (uint32_t)(k.lo >> 32); }
FLX_SORT_HD uint32_t sv_key_q(SortKey const& k) { return (uint32_t)k.lo; }
FLX_SORT_HD flx_sv_signature sv_signature_of(SortKey const& k) {
    return flx_sv_signature{sv_key_type(k), sv_key_side_a(k), sv_key_side_b(k), 0u, (int32_t)sv_key_ref_a(k), (int32_t)sv_key_ref_b(k), sv_key_pos_a(k), sv_key_q(k)};
}
FLX_SORT_HD SortKey sv_key_of(flx_sv_signature const& s) { return sv_key(s.type, s.side_a, s.side_b, (uint32_t)s.ref_a, (uint32_t)s.ref_b, s.pos_a, s.q); }

// ---- one record as the junctions see it: its query interval on the read as given, [rs, re) on its sequence, its strand
struct SvSegment { uint32_t q_start, q_end, rs, re, ref, reverse, mark, pad; };       // 32 bytes, as the device writes them

// the junction of two query-neighbouring members a, b (a in front of b on the read)
FLX_SORT_HD SortKey sv_junction_key(SvSegment const& a, SvSegment const& b) {
    uint32_t const pa = a.reverse ? a.rs : a.re - 1u, sa = a.reverse ? 0u : 1u;
    uint32_t const pb = b.reverse ? b.re - 1u : b.rs, sb = b.reverse ? 1u : 0u;
    bool const swap = b.ref != a.ref ? b.ref < a.ref : pb != pa ? pb < pa : sb < sa;
    return swap ? sv_key(SV_BND, sb, sa, b.ref, a.ref, pb, pa) : sv_key(SV_BND, sa, sb, a.ref, b.ref, pa, pb);
}
// a in front of b in a group's order; ia, ib: their indices in the array
FLX_SORT_HD bool sv_member_less(SvSegment const& a, uint32_t ia, SvSegment const& b, uint32_t ib) { return a.q_start != b.q_start ? a.q_start < b.q_start : ia < ib; }

// ---- options
inline bool sv_options_valid(const flx_sv_options* o) {
    if (!o) return true;
    for (uint32_t r : o->reserved) if (r) { set_error("flx_sv_options: the reserved fields must be 0"); return false; }
    if (o->initial_capacity > SV_MAX_SIGNATURES) { set_error("flx_sv_options: initial_capacity above 2^32 - 1"); return false; }
    return true;
}
inline flx_sv_options sv_options_or_default(const flx_sv_options* o) { return o ? *o : flx_sv_options{}; }
struct SvThresholds { uint32_t min_length, max_distance, min_support; };
inline SvThresholds sv_thresholds(flx_sv_options const& o) {
    return SvThresholds{o.min_length ? o.min_length : SV_DEFAULT_MIN_LENGTH, o.max_distance ? o.max_distance : SV_DEFAULT_MAX_DISTANCE,
                        o.min_support ? o.min_support : SV_DEFAULT_MIN_SUPPORT};
}
inline bool sv_options_equal(flx_sv_options const& a, flx_sv_options const& b) {
    SvThresholds const x = sv_thresholds(a), y = sv_thresholds(b);
    return a.count_secondary == b.count_secondary && a.min_mapq == b.min_mapq && x.min_length == y.min_length && x.max_distance == y.max_distance &&
           x.min_support == y.min_support;
}
inline flx_coverage_options sv_filter(flx_sv_options const& o) {
    flx_coverage_options c{};
    c.count_secondary = o.count_secondary;
    c.min_mapq = o.min_mapq;
    return c;
}
inline bool sv_lengths_valid(const uint64_t* ref_lens, uint32_t n_refs, const char* who, std::vector<u64>& starts) {
    // (ahead of the lengths: nothing is read or allocated for a refused count)
    if ((u64)n_refs >= SV_MAX_REFS) { set_error(std::string(who) + ": 2^30 sequences or more: a key cannot hold their ids"); return false; }
    return coverage_lengths_valid(ref_lens, n_refs, who, starts);
}
FLX_SORT_HD bool sv_word_qualifies(uint32_t word, uint32_t min_length) { return ((word & 15u) == 1u || (word & 15u) == 2u) && (word >> 4) >= min_length; }

// ---- the plan of one array of records (one piece of a run)
// One counted record: where its words lie in the pool it was judged against, where its DEL / INS keys go (key_off, n_events of them,
// relative to the first key of the piece), and what the walk needs besides.
struct SvJob { u64 word_off; u64 key_off; u32 n_words; u32 n_events; u32 position; u32 ref; u32 read_len; u32 reverse; };
// One member of a group: its job (and segment), its group's members [group_begin, group_begin + group_size) in the member list, and the
// first key of its group's group_size - 1 junctions (relative to the first key of the piece).
struct SvMember { u32 job; u32 group_begin; u32 group_size; u32 pad; u64 key_off; };
struct SvPlan {
    std::vector<SvJob> jobs;
    std::vector<SvMember> members;
    u64 n_events = 0, n_junctions = 0, n_records = 0;  // n_events + n_junctions keys: the events first
    u64 n_keys() const { return n_events + n_junctions; }
};

// Judges the records and fills the plan. false: refused, an error is set and nothing may be added. read_len(i): the length of read i.
template <class ReadLen>
inline bool sv_plan(std::vector<u64> const& starts, flx_sv_options const& o, const flx_record* records, uint64_t n, const uint32_t* cigar_words,
                    uint64_t n_words, uint64_t n_reads, ReadLen read_len, const char* who, SvPlan& plan) {
    flx_coverage_options const filter = sv_filter(o);
    uint32_t const min_length = sv_thresholds(o).min_length;
    std::vector<CoverageJob> cov;
    if (!coverage_plan(starts, filter, records, n, cigar_words, n_words, who, cov)) return false;
    plan = SvPlan{};
    plan.n_records = n;
    PafSumsCache cache;                                                 // (a read's records at one locus share one word array)
    u32 cached_events = 0;
    size_t group_begin = 0;                                             // of the current group, in plan.members
    auto close_group = [&](size_t end) {
        u32 const m = (u32)(end - group_begin);
        for (size_t k = group_begin; k < end; ++k) { plan.members[k].group_begin = (u32)group_begin; plan.members[k].group_size = m; plan.members[k].key_off = plan.n_junctions; }
        if (m > 1) plan.n_junctions += m - 1;
        group_begin = end;
    };
    for (uint64_t i = 0; i < n; ++i) {
        flx_record const& r = records[i];
        if (i > 0 && r.read_index != records[i - 1].read_index) close_group(plan.members.size());
        if (!coverage_record_counts(r, filter)) continue;
        std::string const rec = std::string(who) + ": record " + std::to_string(i);
        if (r.read_index >= n_reads) { set_error(rec + " names a read_index outside the reads given"); return false; }
        bool const cached = cache.length == r.cigar_length && cache.offset == r.cigar_offset;      // (a counted record has words)
        if (!cached) {
            cache = PafSumsCache{r.cigar_offset, r.cigar_length, paf_reduce(cigar_words + r.cigar_offset, r.cigar_length)};
            cached_events = 0;
            for (u32 t = 0; t < r.cigar_length; ++t) cached_events += sv_word_qualifies(cigar_words[r.cigar_offset + t], min_length) ? 1u : 0u;
        }
        PafSums const& s = cache.sums;
        if (s.interior_clip) { set_error(rec + " has an S word with other words on both sides"); return false; }
        u64 const rows = s.lead + s.eq + s.x + s.ins + s.trail, len = (u64)read_len(r.read_index);
        if (rows != len) { set_error(rec + " has query-consuming CIGAR lengths that sum to " + std::to_string(rows) + ", its read has " + std::to_string(len) + " letters"); return false; }
        if (rows >= PAF_MAX_SUM) { set_error(rec + " has CIGAR lengths that sum to 2^31 or more"); return false; }
        if (s.eq + s.x + s.del == 0) { set_error(rec + " has no reference-consuming column"); return false; }
        if (plan.jobs.size() >= SV_MAX_SIGNATURES || plan.n_events + cached_events > SV_MAX_SIGNATURES) { set_error(std::string(who) + ": more than 2^32 - 1 records or signatures in one call"); return false; }
        if (!(r.flag & 256u)) {
            if (plan.members.size() - group_begin == SV_MAX_GROUP) { set_error(rec + " is member " + std::to_string(SV_MAX_GROUP + 1) + " of its read's group: more than 64 are refused"); return false; }
            plan.members.push_back(SvMember{(u32)plan.jobs.size(), 0u, 0u, 0u, 0u});
        }
        plan.jobs.push_back(SvJob{r.cigar_offset, plan.n_events, r.cigar_length, cached_events, (u32)r.position, (u32)r.reference_id, (u32)len, (r.flag & 16u) ? 1u : 0u});
        plan.n_events += cached_events;
    }
    close_group(plan.members.size());
    for (auto& m : plan.members) m.key_off += plan.n_events;             // the junctions lie behind the events
    return true;
}

// the walk of one judged job, word by word: its DEL / INS keys at keys[j.key_off ..] and its segment. Returns the keys written.
inline u32 sv_walk(SvJob const& j, const uint32_t* cigar_words, uint32_t min_length, SortKey* keys, SvSegment& seg) {
    u64 p = j.position, lead = 0, pending = 0;
    bool seen = false;
    u32 at = 0;
    for (u32 t = 0; t < j.n_words; ++t) {
        uint32_t const w = cigar_words[j.word_off + t], op = w & 15u, len = w >> 4;
        if (op == 4u) { if (seen) pending += len; else lead += len; }
        else { pending = 0; seen = true; }
        if (sv_word_qualifies(w, min_length))
            keys[j.key_off + at++] = sv_key(op == 2u ? SV_DEL : SV_INS, 0u, 0u, j.ref, j.ref, (uint32_t)(op == 1u && p > j.position ? p - 1 : p), len);
        if (coverage_op_consumes(op)) p += len;
    }
    seg = SvSegment{(uint32_t)(j.reverse ? pending : lead), (uint32_t)(j.read_len - (j.reverse ? lead : pending)), j.position, (uint32_t)p, j.ref, j.reverse, 0u, 0u};
    return at;
}

// the junctions of the plan's groups from the segments of its jobs, at keys[member.key_off ..]
inline void sv_junctions(SvPlan const& plan, const SvSegment* segments, SortKey* keys) {
    for (size_t g = 0; g < plan.members.size(); g += plan.members[g].group_size) {
        u32 const m = plan.members[g].group_size;
        std::vector<u32> order(m);
        for (u32 k = 0; k < m; ++k) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](u32 a, u32 b) { return segments[plan.members[g + a].job].q_start < segments[plan.members[g + b].job].q_start; });
        for (u32 k = 0; k + 1 < m; ++k)
            keys[plan.members[g].key_off + k] = sv_junction_key(segments[plan.members[g + order[k]].job], segments[plan.members[g + order[k + 1]].job]);
    }
}

// the keys of a judged plan, appended to `keys` in no particular order
inline void sv_keys_host(SvPlan const& plan, const uint32_t* cigar_words, uint32_t min_length, std::vector<SortKey>& keys) {
    size_t const base = keys.size();
    keys.resize(base + plan.n_keys());
    std::vector<SvSegment> segments(plan.jobs.size());
    for (size_t k = 0; k < plan.jobs.size(); ++k) sv_walk(plan.jobs[k], cigar_words, min_length, keys.data() + base, segments[k]);
    sv_junctions(plan, segments.data(), keys.data() + base);
}

// ---- clusters
// the breaks of the two levels (the kernels' tests too)
FLX_SORT_HD bool sv_coarse_break(SortKey const& prev, SortKey const& k, uint32_t max_distance) {
    return prev.hi != k.hi || sv_key_pos_a(k) - sv_key_pos_a(prev) > max_distance;       // (key order: pos_a ascends within a class)
}
FLX_SORT_HD bool sv_fine_break(uint32_t prev_group, uint32_t prev_q, uint32_t group, uint32_t q, uint32_t max_distance) {
    return prev_group != group || q - prev_q > max_distance;                               // ((group, q) order: q ascends within a group)
}
FLX_SORT_HD flx_sv_cluster sv_cluster_of(SortKey const& k, uint32_t support, uint32_t pos_a_min, uint32_t pos_a_max, uint32_t q_min, uint32_t q_median, uint32_t q_max) {
    return flx_sv_cluster{sv_key_type(k), sv_key_side_a(k), sv_key_side_b(k), support, (int32_t)sv_key_ref_a(k), (int32_t)sv_key_ref_b(k), pos_a_min, pos_a_max,
                          q_min, q_median, q_max, 0u};
}
// sorted: the signatures' keys in key order; appends the clusters with support >= min_support
inline void sv_clusters_host(const SortKey* sorted, uint64_t n, SvThresholds const& t, std::vector<flx_sv_cluster>& out) {
    uint64_t i = 0;
    while (i < n) {
        uint64_t e = i + 1;
        while (e < n && !sv_coarse_break(sorted[e - 1], sorted[e], t.max_distance)) ++e;
        std::vector<std::pair<uint32_t, uint32_t>> qp;                  // (q, pos_a) of the coarse group
        for (uint64_t k = i; k < e; ++k) qp.emplace_back(sv_key_q(sorted[k]), sv_key_pos_a(sorted[k]));
        std::sort(qp.begin(), qp.end());
        size_t a = 0;
        while (a < qp.size()) {
            size_t b = a + 1;
            while (b < qp.size() && !sv_fine_break(0u, qp[b - 1].first, 0u, qp[b].first, t.max_distance)) ++b;
            uint32_t lo = qp[a].second, hi = qp[a].second;
            for (size_t k = a; k < b; ++k) { lo = std::min(lo, qp[k].second); hi = std::max(hi, qp[k].second); }
            uint64_t const support = b - a;
            if (support >= t.min_support) out.push_back(sv_cluster_of(sorted[i], (uint32_t)support, lo, hi, qp[a].first, qp[a + (support - 1) / 2].first, qp[b - 1].first));
            a = b;
        }
        i = e;
    }
}

// ---- the launches of flx_sv.hip (each returns the hipError_t of its launch; pointers are device pointers)
struct SvDevice {
    static constexpr u32 EXTRACT_GRID_CAP = 1u << 16;  // most blocks (four waves, a job each at a time) of an sv_extract launch
    static constexpr u32 STRIDED_GRID_CAP = 1u << 14;  // most blocks of the launches with one thread per member, key or cluster: a thread strides on by the grid
    // one wave per job: its DEL / INS keys at d_keys[job.key_off ..] and d_segments[job]; *d_flag becomes nonzero when a job's words
    // disagree with the host's judgement (its segment is marked, no key is written outside its stretch)
    static int extract(void* stream, const SvJob* d_jobs, u32 n_jobs, const u32* d_words, u32 min_length, SortKey* d_keys, SvSegment* d_segments, u32* d_flag);
    // one thread per member: the junction to its successor in its group at d_keys[member.key_off + its place in the group's order]
    static int junctions(void* stream, const SvMember* d_members, u32 n_members, const SvSegment* d_segments, SortKey* d_keys, u32* d_flag);
    // flags[i] = 1 where a coarse group starts behind key i - 1 (flags[0] = 0): scanned inclusively they are the group ids
    static int coarse_flags(void* stream, const SortKey* d_sorted, u64 n, u32 max_distance, u32* d_flags);
    // keys2[i] = {group id, q << 32 | pos_a} of sorted key i
    static int regroup(void* stream, const SortKey* d_sorted, const u32* d_groups, u64 n, SortKey* d_keys2);
    // flags[i] = 1 where a cluster starts behind key2 i - 1 (flags[0] = 0): scanned inclusively they are the cluster ids
    static int fine_flags(void* stream, const SortKey* d_sorted2, u64 n, u32 max_distance, u32* d_flags);
    // the clusters in three launches: heads (a cluster's first member writes its start and clears its bounds), bounds (pos_a_min and
    // pos_a_max, reduced in the wave where it holds one cluster, then atomicMin / atomicMax) and fill (everything positional)
    static int cluster_heads(void* stream, const u32* d_ids, u64 n, u32* d_starts, flx_sv_cluster* d_clusters);
    static int cluster_bounds(void* stream, const SortKey* d_sorted2, const u32* d_ids, u64 n, flx_sv_cluster* d_clusters);
    static int cluster_fill(void* stream, const SortKey* d_sorted, const SortKey* d_sorted2, const u32* d_payload2, const u32* d_starts, u64 n, u64 n_clusters,
                            flx_sv_cluster* d_clusters);
    // mode 0: d_count[tile] = the tile's clusters with support >= min_support; mode 1: those clusters in order (d_count scanned by then)
    static int compact(void* stream, int mode, const flx_sv_cluster* d_clusters, u64 n_clusters, u32 min_support, u32* d_count, flx_sv_cluster* d_out);
    static int signatures(void* stream, const SortKey* d_sorted, u64 n, flx_sv_signature* d_out);
};

}  // namespace flx
