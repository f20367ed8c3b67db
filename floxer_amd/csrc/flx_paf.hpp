// PAF summaries (flx_paf, include/floxer_amd.h): the rule, in one place. Host code only: the reduction of one record's CIGAR words, the
// judgement of records that flx_paf_summarize_host, flx_paf_summarize (in front of its launch) and the checks share, and the integer
// form of the de:f tag for the writer. The kernel (flx_paf.hip) does the same reduction on the device, 64 words per pass.
//
// Words are len << 4 | op with = 7, X 8, I 1, D 2, S 4. For one record with flag & 4 clear and reference_id >= 0:
//   lead, trail           the summed S words in front of the first and behind the last non-S word
//   eq, x, ins, del       the summed lengths of the = X I D words
//   gap_opens             the maximal runs of neighbouring words with the same gap op: an I or D word counts when it is the record's
//                         first word or its predecessor has another op (the pipeline never writes neighbours with one op, flx_internal.hpp
//                         in front of cs_slab_bytes; the rule does not rely on that)
//   ref_end               position + eq + x + del
//   query interval        [lead, read_len - trail) on the oriented read; on the read as given, with flag & 16: query_start = trail and
//                         query_end = read_len - lead, otherwise query_start = lead and query_end = read_len - trail
//   refused               no words, an op other than = X I D S, a zero-length word, a reference_id outside the list, a negative position,
//                         a span that ends behind its sequence, words outside the pool (all as coverage refuses them); an S word with
//                         non-S words on both sides; a read_index outside the reads; lead + eq + x + ins + trail != read_len; no
//                         reference-consuming column; a sum of 2^31 or more
// A record with flag & 4 or reference_id < 0 is not judged and gets all zeros. Secondary and supplementary records are summarised like
// any other: filtering belongs to the writer.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "flx_coverage.hpp"

namespace flx {

constexpr u64 PAF_MAX_SUM = 1ull << 31;                // every sum of a summary stays below it
constexpr u32 PAF_GRID_CAP = 1u << 16;                   // most blocks (one wave, one record at a time) of a paf_summarise launch; the records behind them are taken in turns
constexpr u32 PAF_VIOLATION = 0xFFFFFFFFu;             // the kernel's mark in every field of a summary it could not make

inline bool paf_record_mapped(flx_record const& r) { return !(r.flag & 4u) && r.reference_id >= 0; }

// NULL is all zero; the switches are 0 or 1 and the reserved fields 0
inline bool paf_options_valid(const flx_paf_options* o) {
    if (!o) return true;
    for (uint32_t r : o->reserved) if (r) { set_error("flx_paf_options: the reserved fields must be 0"); return false; }
    if (o->write_cigar > 1 || o->write_unmapped > 1 || o->mapq_from_records > 1 || o->skip_secondary > 1) { set_error("flx_paf_options: the switches must be 0 or 1"); return false; }
    return true;
}

// the reduction of one record's words, whatever they are
struct PafSums {
    u64 lead = 0, trail = 0, eq = 0, x = 0, ins = 0, del = 0, gap_opens = 0;
    bool bad_op = false, zero_length = false, interior_clip = false;
};
inline PafSums paf_reduce(const uint32_t* words, u64 n) {
    PafSums s;
    bool seen = false;                                 // a non-S word lies in front
    u64 pending = 0;                                   // the S lengths since the last non-S word
    uint32_t prev = 0;                                 // (no op is 0)
    for (u64 t = 0; t < n; ++t) {
        uint32_t const op = words[t] & 15u;
        u64 const len = words[t] >> 4;
        if (len == 0) s.zero_length = true;
        if (op == 4u) {
            if (seen) pending += len; else s.lead += len;
        } else {
            if (op == 7u) s.eq += len;
            else if (op == 8u) s.x += len;
            else if (op == 1u) s.ins += len;
            else if (op == 2u) s.del += len;
            else s.bad_op = true;
            if (seen && pending) s.interior_clip = true;
            pending = 0;
            seen = true;
            if ((op == 1u || op == 2u) && prev != op) ++s.gap_opens;
        }
        prev = op;
    }
    s.trail = pending;
    return s;
}

// the summary of judged sums
inline flx_paf_summary paf_summary_of(PafSums const& s, flx_record const& r, u64 read_len) {
    flx_paf_summary o;
    bool const reverse = (r.flag & 16u) != 0;
    o.query_start = (uint32_t)(reverse ? s.trail : s.lead);
    o.query_end = (uint32_t)(read_len - (reverse ? s.lead : s.trail));
    o.ref_end = (uint32_t)((u64)r.position + s.eq + s.x + s.del);
    o.matches = (uint32_t)s.eq;
    o.mismatches = (uint32_t)s.x;
    o.ins_bases = (uint32_t)s.ins;
    o.del_bases = (uint32_t)s.del;
    o.gap_opens = (uint32_t)s.gap_opens;
    return o;
}

// the sums of the words last reduced: a read's records at one locus share one CIGAR array (forty of them at default flags), which is
// then walked once
struct PafSumsCache { u64 offset = 0; u32 length = 0; PafSums sums; };

// Judges record i and makes its summary. false: refused, an error is set, `out` is untouched.
inline bool paf_judge(flx_record const& r, uint64_t i, const uint32_t* cigar_words, uint64_t n_words, const uint64_t* read_offsets, uint64_t n_reads,
                      const uint64_t* ref_lens, uint32_t n_refs, const char* who, flx_paf_summary& out, PafSumsCache* cache = nullptr) {
    if (!paf_record_mapped(r)) { out = flx_paf_summary{}; return true; }
    auto refuse = [&](std::string const& what) { set_error(std::string(who) + ": record " + std::to_string(i) + what); return false; };
    if ((uint32_t)r.reference_id >= n_refs) return refuse(" names a reference_id outside the list");
    if (r.position < 0) return refuse(" has a negative position");
    if (r.cigar_length == 0) return refuse(" is mapped and has no CIGAR words (a run made with without_cigar has no PAF summary)");
    if (!cigar_words || r.cigar_offset > n_words || r.cigar_length > n_words - r.cigar_offset) return refuse(" has CIGAR words outside the pool");
    bool const cached = cache && cache->length == r.cigar_length && cache->offset == r.cigar_offset;      // (length 0 never gets here)
    PafSums const s = cached ? cache->sums : paf_reduce(cigar_words + r.cigar_offset, r.cigar_length);
    if (cache && !cached) *cache = PafSumsCache{r.cigar_offset, r.cigar_length, s};
    if (s.bad_op) return refuse(" has a CIGAR op other than = X I D S");
    if (s.zero_length) return refuse(" has a CIGAR word of length 0");
    if (s.interior_clip) return refuse(" has an S word with other words on both sides");
    u64 const rows = s.lead + s.eq + s.x + s.ins + s.trail;             // (a word is below 2^28 and a record has fewer than 2^32 words: no sum wraps)
    for (u64 v : {rows, s.eq + s.x + s.del, s.gap_opens})
        if (v >= PAF_MAX_SUM) return refuse(" has CIGAR lengths that sum to 2^31 or more");
    if ((u64)r.position + s.eq + s.x + s.del > ref_lens[(size_t)r.reference_id]) return refuse(" ends behind its sequence");
    if (r.read_index >= n_reads || !read_offsets) return refuse(" names a read_index outside the reads given");
    u64 const read_len = read_offsets[r.read_index + 1] - read_offsets[r.read_index];
    if (rows != read_len) return refuse(" has query-consuming CIGAR lengths that sum to " + std::to_string(rows) + ", its read has " + std::to_string(read_len) + " letters");
    if (s.eq + s.x + s.del == 0) return refuse(" has no reference-consuming column");
    out = paf_summary_of(s, r, read_len);
    return true;
}

// the sequences' lengths as coverage judges them (none empty, none of 2^31 or more)
inline bool paf_lengths_valid(const uint64_t* ref_lens, uint32_t n_refs, const char* who) {
    std::vector<u64> starts;
    return coverage_lengths_valid(ref_lens, n_refs, who, starts);
}

// The records [from, to) of a call: out[i] receives the summary of record i. false: refused, an error is set; `out` may hold summaries
// of earlier records (the callers judge into a buffer of their own).
inline bool paf_plan(const flx_record* records, uint64_t from, uint64_t to, const uint32_t* cigar_words, uint64_t n_words, const uint64_t* read_offsets,
                     uint64_t n_reads, const uint64_t* ref_lens, uint32_t n_refs, const char* who, flx_paf_summary* out) {
    PafSumsCache cache;
    for (uint64_t i = from; i < to; ++i)
        if (!paf_judge(records[i], i, cigar_words, n_words, read_offsets, n_reads, ref_lens, n_refs, who, out[i], &cache)) return false;
    return true;
}

inline bool paf_summary_is_violation(flx_paf_summary const& s) {
    return s.query_start == PAF_VIOLATION && s.query_end == PAF_VIOLATION && s.ref_end == PAF_VIOLATION && s.matches == PAF_VIOLATION &&
           s.mismatches == PAF_VIOLATION && s.ins_bases == PAF_VIOLATION && s.del_bases == PAF_VIOLATION && s.gap_opens == PAF_VIOLATION;
}

// de:f in integers: the gap-compressed divergence (mismatches + gap_opens) / (matches + mismatches + gap_opens), rounded half up to four
// decimals and returned in units of 1 / 10000. den > 0.
inline u64 paf_divergence_e4(u64 num, u64 den) { return (20000ull * num + den) / (2ull * den); }

// ---- the launch of flx_paf.hip (returns the hipError_t of its launch; pointers are device pointers). One job per record, in record
// order: where its words lie in the uploaded words, its position, its read's length and its strand; n_words 0 marks a record that gets
// all zeros.
struct PafJob { u64 word_off; u32 n_words; u32 read_len; u32 position; u32 reverse; };
struct PafDevice {
    static int summarise(void* stream, const PafJob* d_jobs, u32 n_jobs, const u32* d_words, flx_paf_summary* d_out);
};

}  // namespace flx
