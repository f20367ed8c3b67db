// Depth of coverage (flx_coverage, include/floxer_amd.h): the rule, in one place. Host code only: the judgement of options, lengths and
// records that flx_coverage_host, flx_coverage_add_records and flx_coverage_add_run share, and the walk itself for the host hook; the
// kernels (flx_coverage.hip) do the same walk on the device into a difference array.
//
// Depth is a u32 per reference position, indexed by position in the unpadded concatenation of the sequences in reference-id order.
//   which records count   flag & 4: never; flag & 256: only with count_secondary; 2048 always; min_mapq > 0: only reserved >= min_mapq
//                         (samtools depth's default filters plus its -Q: a read's forty identical secondaries are not counted forty times)
//   how they add depth    walked from `position` over the CIGAR words: = (7) and X (8) columns add 1 at their reference position; I (1)
//                         and S (4) consume no reference and add nothing; D (2) columns advance and add 1 only with count_deletions
//                         (samtools depth -J)
//   refused               a counted record without CIGAR words, words outside the pool, an op other than = X I D S, a zero-length word, a
//                         reference_id outside the list, a negative position, a span that ends behind its sequence
// Records that do not count are not judged: an unmapped record has reference_id -1 and no words.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "flx_internal.hpp"

namespace flx {

constexpr u64 COVERAGE_MAX_SEQUENCE = 1ull << 31;      // flx_record.position is an int32
constexpr u64 COVERAGE_MAX_TOTAL = 1ull << 32;         // the index's own limit on its text: positions and run counts fit 32 bits

// NULL is all zero; the reserved fields must be 0
inline bool coverage_options_valid(const flx_coverage_options* o) {
    if (!o) return true;
    for (uint32_t r : o->reserved) if (r) { set_error("flx_coverage_options: the reserved fields must be 0"); return false; }
    return true;
}
inline flx_coverage_options coverage_options_or_default(const flx_coverage_options* o) { return o ? *o : flx_coverage_options{}; }
inline bool coverage_options_equal(flx_coverage_options const& a, flx_coverage_options const& b) {
    return a.count_deletions == b.count_deletions && a.count_secondary == b.count_secondary && a.min_mapq == b.min_mapq && a.report_zero == b.report_zero;
}

// starts receives n_refs + 1 entries: the first position of every sequence in the concatenation, and the total behind the last
inline bool coverage_lengths_valid(const uint64_t* ref_lens, uint32_t n_refs, const char* who, std::vector<u64>& starts) {
    if (!ref_lens || n_refs == 0) { set_error(std::string(who) + ": no reference lengths"); return false; }
    starts.assign((size_t)n_refs + 1, 0);
    for (uint32_t r = 0; r < n_refs; ++r) {
        if (ref_lens[r] == 0) { set_error(std::string(who) + ": sequence " + std::to_string(r) + " is empty"); return false; }
        if (ref_lens[r] >= COVERAGE_MAX_SEQUENCE) { set_error(std::string(who) + ": sequence " + std::to_string(r) + " has 2^31 symbols or more: flx_record.position cannot address it"); return false; }
        starts[r + 1] = starts[r] + ref_lens[r];
        if (starts[r + 1] >= COVERAGE_MAX_TOTAL) { set_error(std::string(who) + ": the sequences have 2^32 symbols or more in total"); return false; }
    }
    return true;
}

inline bool coverage_record_counts(flx_record const& r, flx_coverage_options const& o) {
    if (r.flag & 4u) return false;
    if ((r.flag & 256u) && !o.count_secondary) return false;
    if (o.min_mapq > 0 && r.reserved < o.min_mapq) return false;
    return true;
}
inline bool coverage_op_consumes(uint32_t op) { return op == 7u || op == 8u || op == 2u; }
inline bool coverage_op_counts(uint32_t op, bool count_deletions) { return op == 7u || op == 8u || (op == 2u && count_deletions); }

// one counted record: where its walk starts in the concatenation and where its words lie in the pool it was judged against
struct CoverageJob { u64 text_off; u64 word_off; u32 n_words; u32 pad; };

// Judges the records and appends one job per counted record. false: refused, an error is set and nothing may be added.
inline bool coverage_plan(std::vector<u64> const& starts, flx_coverage_options const& o, const flx_record* records, uint64_t n,
                          const uint32_t* cigar_words, uint64_t n_words, const char* who, std::vector<CoverageJob>& jobs) {
    size_t const n_refs = starts.size() - 1;
    for (uint64_t i = 0; i < n; ++i) {
        flx_record const& r = records[i];
        if (!coverage_record_counts(r, o)) continue;
        std::string const rec = std::string(who) + ": record " + std::to_string(i);
        if (r.reference_id < 0 || (size_t)r.reference_id >= n_refs) { set_error(rec + " names a reference_id outside the list"); return false; }
        if (r.position < 0) { set_error(rec + " has a negative position"); return false; }
        if (r.cigar_length == 0) { set_error(rec + " counts and has no CIGAR words (a run made with without_cigar has no depth)"); return false; }
        if (!cigar_words || r.cigar_offset > n_words || r.cigar_length > n_words - r.cigar_offset) { set_error(rec + " has CIGAR words outside the pool"); return false; }
        u64 const len = starts[(size_t)r.reference_id + 1] - starts[(size_t)r.reference_id];
        u64 span = 0;
        for (uint32_t t = 0; t < r.cigar_length; ++t) {
            uint32_t const w = cigar_words[r.cigar_offset + t], op = w & 15u;
            if (op != 7u && op != 8u && op != 1u && op != 2u && op != 4u) { set_error(rec + " has a CIGAR op other than = X I D S"); return false; }
            if ((w >> 4) == 0) { set_error(rec + " has a CIGAR word of length 0"); return false; }
            if (coverage_op_consumes(op)) span += w >> 4;
        }
        if ((u64)r.position + span > len) { set_error(rec + " ends behind its sequence"); return false; }
        jobs.push_back(CoverageJob{starts[(size_t)r.reference_id] + (u64)r.position, r.cigar_offset, r.cigar_length, 0u});
    }
    return true;
}

// Where the words of judged jobs (CoverageJob, PileupJob: word_off, n_words) lie in the pool that goes up: every word once, however many
// jobs refer to it. pool receives the words in use in the order of the original pool, every job's word_off then indexes `pool`.
template <class Job>
void compact_words(std::vector<Job>& jobs, const uint32_t* cigar_words, std::vector<u32>& pool) {
    struct Segment { u64 from, to, base; };
    std::vector<std::pair<u64, u64>> spans;
    spans.reserve(jobs.size());
    for (auto const& j : jobs) spans.emplace_back(j.word_off, j.word_off + j.n_words);
    std::sort(spans.begin(), spans.end());
    std::vector<Segment> segments;
    for (auto const& s : spans) {
        if (!segments.empty() && s.first <= segments.back().to) segments.back().to = std::max(segments.back().to, s.second);
        else segments.push_back(Segment{s.first, s.second, 0});
    }
    u64 used = 0;
    for (auto& s : segments) { s.base = used; used += s.to - s.from; }
    pool.resize(used);
    for (auto const& s : segments) memcpy(pool.data() + s.base, cigar_words + s.from, (s.to - s.from) * 4);
    for (auto& j : jobs) {
        auto it = std::upper_bound(segments.begin(), segments.end(), j.word_off, [](u64 off, Segment const& s) { return off < s.from; });
        Segment const& s = *(it - 1);
        j.word_off = s.base + (j.word_off - s.from);
    }
}

// the walk of one judged job, column by column into `depth`
inline void coverage_walk(CoverageJob const& j, const uint32_t* cigar_words, bool count_deletions, uint32_t* depth) {
    u64 p = j.text_off;
    for (u32 t = 0; t < j.n_words; ++t) {
        uint32_t const w = cigar_words[j.word_off + t], op = w & 15u, len = w >> 4;
        if (coverage_op_counts(op, count_deletions)) for (u32 c = 0; c < len; ++c) ++depth[p + c];
        if (coverage_op_consumes(op)) p += len;
    }
}

// windows of size W over the sequences (0: one per sequence): the number of windows in front of every sequence, and of all behind the last
// (a window of 2^32 or more is one per sequence too: no sequence is that long)
inline void coverage_window_bases(std::vector<u64> const& starts, u64 window, std::vector<u64>& bases) {
    size_t const n_refs = starts.size() - 1;
    if (window >= COVERAGE_MAX_TOTAL) window = 0;
    bases.assign(n_refs + 1, 0);
    for (size_t r = 0; r < n_refs; ++r) {
        u64 const len = starts[r + 1] - starts[r];
        bases[r + 1] = bases[r] + (window == 0 ? 1 : (len + window - 1) / window);
    }
}

// ---- the launches of flx_coverage.hip (each returns the hipError_t of its launch; pointers are device pointers, positions index the
// concatenation, d_starts holds the n_refs + 1 sequence starts as u32)
struct CoverageWindowAcc { unsigned long long depth_sum, covered; u32 max_depth, pad; };
struct CoverageDevice {
    static constexpr u32 ADD_GRID_CAP = 1u << 16;      // most blocks (four waves, a record each at a time) of a coverage_add launch
    static int add(void* stream, const CoverageJob* d_jobs, u32 n_jobs, const u32* d_words, u32* d_acc, u32 count_deletions);
    // mode 0: the tiles' head counts; 1: the positions of all heads; 2: the reported runs (d_count_* scanned by then)
    static int heads(void* stream, int mode, const u32* d_depth, u64 total, const u32* d_starts, u32 n_refs, u32 report_zero, u32* d_count_all,
                     u32* d_count_rep, u32* d_heads, u64 n_heads, flx_depth_run* d_out);
    static int windows(void* stream, const u32* d_depth, u64 total, const u32* d_starts, u32 n_refs, u64 window, const u64* d_bases, CoverageWindowAcc* d_out);
};

}  // namespace flx
