// Allele pileup and variant-site table (flx_pileup, include/floxer_amd.h): the rule, in one place. Host code only: the judgement of
// options, lengths and records that flx_pileup_host, flx_pileup_add_records and flx_pileup_add_run share, the walk itself for the host
// hook, and the site predicate, which the site kernel (flx_pileup.hip) shares. The kernels do the same walk on the device.
//
// Counts are u32 per reference position, indexed by position in the unpadded concatenation of the sequences in reference-id order, in
// seven planes: DEPTH, DEL, A, C, G, T, INS.
//   which records count   coverage's filter, coverage_record_counts (flx_coverage.hpp), with count_secondary and min_mapq
//   the walk              from `position` and row 0 of the record's oriented sequence (the read for flag bit 16 clear, its reverse
//                         complement for bit 16 set, as SEQ is written), over the CIGAR words:
//                           = (7)  DEPTH + 1 on its columns
//                           X (8)  DEPTH + 1 on its columns; a column whose oriented read rank r is 1..4 adds 1 to plane A + r - 1 (rank 0
//                                  and 5 count in DEPTH only); the reference text is never read
//                           D (2)  DEL + 1 on its columns
//                           I (1)  INS + 1 at one anchor: the position of the record's preceding reference-consuming column, or the
//                                  record's first reference-consuming column when none precedes the word; one event whatever its length
//                           S (4)  rows only
//   refused               all that coverage_plan refuses; a read_index outside the reads; query-consuming lengths (= X I S) that do not
//                         sum to the read's length; a record without a reference-consuming column
//   sites                 after the sums: cov = DEPTH + DEL, best = max(A, C, G, T, DEL, INS); a site iff cov >= min_depth,
//                         best >= min_count and best * 1000 >= min_permille * cov (64-bit). 0 takes the defaults 4 / 2 / 200, which are
//                         conventions of this project and fitted to nothing.
#pragma once
#include "flx_coverage.hpp"

namespace flx {

enum PileupPlane : u32 { PILEUP_DEPTH = 0, PILEUP_DEL = 1, PILEUP_A = 2, PILEUP_C = 3, PILEUP_G = 4, PILEUP_T = 5, PILEUP_INS = 6, PILEUP_PLANES = 7 };
constexpr u32 PILEUP_DEFAULT_MIN_DEPTH = 4, PILEUP_DEFAULT_MIN_COUNT = 2, PILEUP_DEFAULT_MIN_PERMILLE = 200;

// NULL is all zero; the reserved fields must be 0; a fraction above 1000 permille is none
inline bool pileup_options_valid(const flx_pileup_options* o) {
    if (!o) return true;
    for (uint32_t r : o->reserved) if (r) { set_error("flx_pileup_options: the reserved fields must be 0"); return false; }
    if (o->min_permille > 1000u) { set_error("flx_pileup_options: min_permille is above 1000"); return false; }
    return true;
}
inline flx_pileup_options pileup_options_or_default(const flx_pileup_options* o) { return o ? *o : flx_pileup_options{}; }
inline bool pileup_options_equal(flx_pileup_options const& a, flx_pileup_options const& b) {
    return a.count_secondary == b.count_secondary && a.min_mapq == b.min_mapq && a.min_depth == b.min_depth && a.min_count == b.min_count && a.min_permille == b.min_permille;
}
// the record filter is coverage's: its options with this object's two switches
inline flx_coverage_options pileup_filter(flx_pileup_options const& o) {
    flx_coverage_options c{};
    c.count_secondary = o.count_secondary;
    c.min_mapq = o.min_mapq;
    return c;
}

// the site thresholds with the defaults taken for 0
struct PileupThresholds { u32 min_depth, min_count, min_permille; };
inline PileupThresholds pileup_thresholds(flx_pileup_options const& o) {
    return PileupThresholds{o.min_depth ? o.min_depth : PILEUP_DEFAULT_MIN_DEPTH, o.min_count ? o.min_count : PILEUP_DEFAULT_MIN_COUNT,
                            o.min_permille ? o.min_permille : PILEUP_DEFAULT_MIN_PERMILLE};
}
// one position: its DEPTH and DEL counts and the largest of its A, C, G, T, DEL and INS counts (the site kernel's test too)
FLX_HD inline bool pileup_site_test(u32 depth, u32 del, u32 best, PileupThresholds const& t) {
    u64 const cov = (u64)depth + (u64)del;
    return cov >= (u64)t.min_depth && best >= t.min_count && (u64)best * 1000ull >= (u64)t.min_permille * cov;
}
// v: the seven planes' counts of one position
inline bool pileup_is_site(const u32 (&v)[PILEUP_PLANES], PileupThresholds const& t) {
    u32 best = v[PILEUP_DEL];
    for (u32 k = PILEUP_A; k < PILEUP_PLANES; ++k) best = v[k] > best ? v[k] : best;
    return pileup_site_test(v[PILEUP_DEPTH], v[PILEUP_DEL], best, t);
}

inline bool pileup_op_consumes_query(uint32_t op) { return op == 7u || op == 8u || op == 1u || op == 4u; }

// the letter of row `row` of a read's oriented sequence (the complement table is reverse_complement's, flx_host.cpp)
inline u8 pileup_oriented_rank(const uint8_t* read, u64 len, bool reverse, u64 row) {
    constexpr u8 comp[8] = {0, 4, 3, 2, 1, 5, 5, 5};
    return reverse ? comp[read[len - 1 - row] & 7] : read[row];
}

// one counted record: where its walk starts in the concatenation, where its words lie in the pool it was judged against, its read and
// strand, and (filled when the letters are staged) where its oriented sequence lies in the letter pool the kernel reads
struct PileupJob { u64 text_off; u64 word_off; u64 seq_off; u32 n_words; u32 reverse; u64 read_index; };

// Judges the records and appends one job per counted record. false: refused, an error is set and nothing may be added.
// read_len(i): the length of read i (i < n_reads)
template <class ReadLen>
inline bool pileup_plan(std::vector<u64> const& starts, flx_pileup_options const& o, const flx_record* records, uint64_t n, const uint32_t* cigar_words,
                        uint64_t n_words, uint64_t n_reads, ReadLen read_len, const char* who, std::vector<PileupJob>& jobs) {
    flx_coverage_options const filter = pileup_filter(o);
    std::vector<CoverageJob> cov;
    if (!coverage_plan(starts, filter, records, n, cigar_words, n_words, who, cov)) return false;
    size_t at = 0;                                                      // coverage_plan made one job per counted record, in record order
    for (uint64_t i = 0; i < n; ++i) {
        flx_record const& r = records[i];
        if (!coverage_record_counts(r, filter)) continue;
        CoverageJob const& c = cov[at++];
        std::string const rec = std::string(who) + ": record " + std::to_string(i);
        if (r.read_index >= n_reads) { set_error(rec + " names a read_index outside the reads given"); return false; }
        u64 rows = 0, span = 0;
        for (u32 t = 0; t < c.n_words; ++t) {
            uint32_t const w = cigar_words[c.word_off + t], op = w & 15u;
            if (pileup_op_consumes_query(op)) rows += w >> 4;
            if (coverage_op_consumes(op)) span += w >> 4;
        }
        if (rows != (u64)read_len(r.read_index)) { set_error(rec + " has query-consuming CIGAR lengths that sum to " + std::to_string(rows) + ", its read has " + std::to_string((u64)read_len(r.read_index)) + " letters"); return false; }
        if (span == 0) { set_error(rec + " has no reference-consuming column"); return false; }
        jobs.push_back(PileupJob{c.text_off, c.word_off, 0, c.n_words, (r.flag & 16u) ? 1u : 0u, r.read_index});
    }
    return true;
}

// the walk of one judged job, column by column into the seven planes of `counts` (plane k at counts + k * plane_stride)
inline void pileup_walk(PileupJob const& j, const uint32_t* cigar_words, const uint8_t* read, u64 read_len, uint32_t* counts, u64 plane_stride) {
    u64 p = j.text_off, row = 0;
    for (u32 t = 0; t < j.n_words; ++t) {
        uint32_t const w = cigar_words[j.word_off + t], op = w & 15u, len = w >> 4;
        if (op == 7u || op == 8u) for (u32 c = 0; c < len; ++c) ++counts[PILEUP_DEPTH * plane_stride + p + c];
        if (op == 8u)
            for (u32 c = 0; c < len; ++c) {
                u8 const r = pileup_oriented_rank(read, read_len, j.reverse != 0, row + c);
                if (r >= 1 && r <= 4) ++counts[(PILEUP_A + r - 1) * plane_stride + p + c];
            }
        if (op == 2u) for (u32 c = 0; c < len; ++c) ++counts[PILEUP_DEL * plane_stride + p + c];
        if (op == 1u) ++counts[PILEUP_INS * plane_stride + (p > j.text_off ? p - 1 : p)];
        if (coverage_op_consumes(op)) p += len;
        if (pileup_op_consumes_query(op)) row += len;
    }
}

// ---- the launches of flx_pileup.hip (each returns the hipError_t of its launch; pointers are device pointers). The accumulator is seven
// planes of `stride` entries each (stride >= total + 1, a multiple of 64); DEPTH and DEL are difference arrays until the finish scan.
struct PileupDevice {
    static constexpr u32 ADD_GRID_CAP = 1u << 16;      // most blocks (four waves, a record each at a time) of a pileup_add launch
    static int add(void* stream, const PileupJob* d_jobs, u32 n_jobs, const u32* d_words, const u8* d_letters, u32* d_acc, u64 stride);
    // mode 0: d_count[tile] = the tile's sites; mode 1: the sites themselves (d_count scanned by then)
    static int sites(void* stream, int mode, const u32* d_acc, u64 stride, u64 total, const u32* d_starts, u32 n_refs, PileupThresholds t, u32* d_count,
                     flx_pileup_site* d_out);
};

}  // namespace flx
