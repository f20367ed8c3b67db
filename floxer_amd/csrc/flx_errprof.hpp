// Error profile of the alignments (flx_errprof, include/floxer_amd.h): the rule, in one place. The judgement of options, texts and records
// that flx_errprof_host, flx_errprof_add_records and flx_errprof_add_run share, the walk itself for the host hook, and, under FLX_HD, the
// pieces of the walk that the kernel (flx_errprof.hip) runs as they stand: the position bins, the homopolymer runs, what one word and
// one record add. The kernel differs from the host walk only in who walks a word (a lane, or the whole wave for a long one).
//
// All counters are u64 in one table of ERRPROF_ENTRIES entries (flx_errprof_table, the sections in the order of ErrprofSection).
//   which records count   coverage's filter, coverage_record_counts (flx_coverage.hpp), with count_secondary and min_mapq
//   the walk              from `position` and row 0 of the record's oriented sequence (pileup_oriented_rank), over the CIGAR words. t[p]:
//                         the reference rank at position p, q[r]: the oriented read rank at row r, [s0, s1): the record's sequence, len:
//                         the read's length, g(r) = reverse ? len - 1 - r : r, bin(r) = g(r) * 100 / len (64-bit; 0 for len 0).
//                           = (7)  PAIR_EQ[t][q] + 1 per column; POS_MATCH[bin(r)] + 1 per row; EQ_RUN[min(L, 256) - 1] + 1
//                           X (8)  PAIR_X[t][q] + 1 per column; POS_MISMATCH[bin(r)] + 1 per row
//                           I (1)  INS_LEN[min(L, 64) - 1] + 1; INS_LETTER[q] + 1 per letter; POS_INS[bin(r)] + 1 per row; HP_INS: p is the
//                                  position of the next reference-consuming column (the walk's cursor: `position` in front of the first
//                                  column, possibly the record's end, possibly s1), a = q[r]; a outside 1..4 or letters that differ: bin
//                                  33; else left = the run of a from p - 1 downwards within [s0, ..), right = the run of a from p upwards
//                                  within [.., s1), each stopped at 32: bin min(32, left + right)
//                           D (2)  DEL_LEN[min(L, 64) - 1] + 1; DEL_LETTER[t] + 1 per letter; POS_DEL[bin(min(r, len - 1))] + 1 per word,
//                                  r the row the walk has reached; HP_DEL: a = t[p]; a outside 1..4 or letters that differ: bin 33; else
//                                  left from p - 1 downwards, right from p + L upwards, each stopped at 32: bin min(32, left + L + right)
//                           S (4)  POS_CLIP[bin(r)] + 1 per row
//                         per record: IDENTITY[matches * 100 / (matches + mismatches + ins_bases + del_bases)] + 1 and the TOTALS
//   refused               all that pileup_plan refuses (and with it coverage_plan); a record whose reference-consuming plus query-consuming
//                         lengths reach 2^31; a reference text with a rank above 5 (at create); flush_threshold above 2^31
// A read rank above 5 is outside the contract of the read pool (flx_align_reads); it is counted as 5 and never indexes outside the table.
#pragma once
#include <cstddef>

#include "flx_pileup.hpp"

namespace flx {

enum ErrprofSection : u32 {
    EP_PAIR_EQ = 0, EP_PAIR_X = 36, EP_INS_LEN = 72, EP_DEL_LEN = 136, EP_INS_LETTER = 200, EP_DEL_LETTER = 206, EP_HP_DEL = 212, EP_HP_INS = 246,
    EP_POS_MATCH = 280, EP_POS_MISMATCH = 380, EP_POS_INS = 480, EP_POS_CLIP = 580, EP_POS_DEL = 680, EP_EQ_RUN = 780, EP_IDENTITY = 1036,
    EP_TOTALS = 1137, EP_RESERVED = 1145, ERRPROF_ENTRIES = 1152
};
enum ErrprofTotal : u32 { EP_RECORDS = 0, EP_MATCHES, EP_MISMATCHES, EP_INS_EVENTS, EP_INS_BASES, EP_DEL_EVENTS, EP_DEL_BASES, EP_CLIP_BASES, EP_N_TOTALS };
static_assert(sizeof(flx_errprof_table) == ERRPROF_ENTRIES * 8, "the table is its sections, back to back");
static_assert(offsetof(flx_errprof_table, hp_del) == EP_HP_DEL * 8 && offsetof(flx_errprof_table, pos_del) == EP_POS_DEL * 8 &&
              offsetof(flx_errprof_table, identity) == EP_IDENTITY * 8 && offsetof(flx_errprof_table, totals) == EP_TOTALS * 8 &&
              offsetof(flx_errprof_table, reserved) == EP_RESERVED * 8, "the sections' places");

constexpr u32 ERRPROF_HP_CAP = 32, ERRPROF_HP_MIXED = 33, ERRPROF_BINS = 100;
constexpr u64 ERRPROF_MAX_RECORD = 1ull << 31;         // reference-consuming plus query-consuming lengths of one record stay below
constexpr u32 ERRPROF_DEFAULT_FLUSH = 1u << 30, ERRPROF_MAX_FLUSH = 1u << 31;

// NULL is all zero; the reserved fields must be 0; a wave's u32 counters hold flush_threshold + 2^31 at most (flx_errprof.hip)
inline bool errprof_options_valid(const flx_errprof_options* o) {
    if (!o) return true;
    for (uint32_t r : o->reserved) if (r) { set_error("flx_errprof_options: the reserved fields must be 0"); return false; }
    if (o->flush_threshold > ERRPROF_MAX_FLUSH) { set_error("flx_errprof_options: flush_threshold is above 2^31"); return false; }
    return true;
}
inline flx_errprof_options errprof_options_or_default(const flx_errprof_options* o) { return o ? *o : flx_errprof_options{}; }
inline bool errprof_options_equal(flx_errprof_options const& a, flx_errprof_options const& b) {      // (the flush threshold changes no sum)
    return a.count_secondary == b.count_secondary && a.min_mapq == b.min_mapq;
}
inline flx_pileup_options errprof_filter(flx_errprof_options const& o) {
    flx_pileup_options p{};
    p.count_secondary = o.count_secondary;
    p.min_mapq = o.min_mapq;
    return p;
}
// the ranks of a reference text: 0..5
inline bool errprof_text_valid(const uint8_t* text, u64 n, const char* who) {
    u8 worst = 0;
    for (u64 i = 0; i < n; ++i) worst = text[i] > worst ? text[i] : worst;
    if (worst > 5) { set_error(std::string(who) + ": the reference text holds a rank above 5"); return false; }
    return true;
}

// one counted record: its first column, its sequence [s0, s1) and its words and letters, all as offsets into the arrays the walk reads
// (the text: the unpadded concatenation, or a context's padded text; seq_off: filled when the letters are staged)
struct ErrprofJob { u64 text_off, word_off, seq_off, s0, s1, read_index; u32 n_words, reverse, read_len, pad; };
static_assert(sizeof(ErrprofJob) == 64, "device layout");

// Judges the records and appends one job per counted record. false: refused, an error is set and nothing may be added.
// starts: the sequences in the unpadded concatenation (the judgement); seq_base[r]: where sequence r begins in the text the walk reads
template <class ReadLen>
inline bool errprof_plan(std::vector<u64> const& starts, std::vector<u64> const& seq_base, flx_errprof_options const& o, const flx_record* records, uint64_t n,
                         const uint32_t* cigar_words, uint64_t n_words, uint64_t n_reads, ReadLen read_len, const char* who, std::vector<ErrprofJob>& jobs) {
    flx_pileup_options const filter = errprof_filter(o);
    flx_coverage_options const cov = pileup_filter(filter);
    std::vector<PileupJob> pile;
    if (!pileup_plan(starts, filter, records, n, cigar_words, n_words, n_reads, read_len, who, pile)) return false;
    size_t at = 0;                                                      // pileup_plan made one job per counted record, in record order
    for (uint64_t i = 0; i < n; ++i) {
        flx_record const& r = records[i];
        if (!coverage_record_counts(r, cov)) continue;
        PileupJob const& p = pile[at++];
        u64 walked = 0;                                                 // (the rows are the read's length: pileup_plan)
        for (u32 t = 0; t < p.n_words; ++t) {
            uint32_t const w = cigar_words[p.word_off + t], op = w & 15u;
            walked += (u64)(w >> 4) * ((coverage_op_consumes(op) ? 1u : 0u) + (pileup_op_consumes_query(op) ? 1u : 0u));
        }
        if (walked >= ERRPROF_MAX_RECORD) { set_error(std::string(who) + ": record " + std::to_string(i) + " has reference-consuming plus query-consuming lengths of 2^31 or more"); return false; }
        size_t const ref = (size_t)r.reference_id;
        jobs.push_back(ErrprofJob{seq_base[ref] + (u64)r.position, p.word_off, 0, seq_base[ref], seq_base[ref] + (starts[ref + 1] - starts[ref]), r.read_index, p.n_words,
                                  p.reverse, (u32)read_len(r.read_index), 0u});
    }
    return true;
}

// ---- the pieces of the walk (host and kernel). add(entry, count) adds count (below 2^31) to a table entry.
FLX_HD inline u32 errprof_rank(u32 x) { return x < 5u ? x : 5u; }
FLX_HD inline u32 errprof_bin(u64 g, u64 len) { return len ? (u32)(g * 100u / len) : 0u; }
// the first g of bin b: the smallest g with g * 100 >= b * len
FLX_HD inline u64 errprof_bin_begin(u32 b, u64 len) { return ((u64)b * len + 99u) / 100u; }
// the rows [row, row + L) of a read of len letters as given: [ga, gb)
FLX_HD inline void errprof_given_rows(u64 row, u64 L, u64 len, bool reverse, u64& ga, u64& gb) {
    ga = reverse ? len - row - L : row;
    gb = ga + L;
}
// the part of [ga, gb) that lies in bin b
FLX_HD inline u32 errprof_rows_in_bin(u32 b, u64 ga, u64 gb, u64 len) {
    u64 const lo = errprof_bin_begin(b, len), hi = errprof_bin_begin(b + 1u, len);
    u64 const from = lo > ga ? lo : ga, to = hi < gb ? hi : gb;
    return to > from ? (u32)(to - from) : 0u;
}
// + 1 per row of [row, row + L) at section[bin(row)]: two divisions for the word, none per row
template <class Add>
FLX_HD inline void errprof_pos_rows(u32 section, u64 row, u64 L, u64 len, bool reverse, Add&& add) {
    u64 ga, gb;
    errprof_given_rows(row, L, len, reverse, ga, gb);
    u32 const last = errprof_bin(gb - 1, len);
    for (u32 b = errprof_bin(ga, len); b <= last; ++b) {
        u32 const k = errprof_rows_in_bin(b, ga, gb, len);
        if (k) add(section + b, k);
    }
}
// the run of rank a from p - 1 downwards, not below s0, and from p upwards, below s1: 32 at most (p lies in [s0, s1])
FLX_HD inline u32 errprof_run_left(const u8* text, u64 p, u64 s0, u32 a) {
    u32 k = 0;
    while (k < ERRPROF_HP_CAP && p - k > s0 && text[p - 1 - k] == a) ++k;
    return k;
}
FLX_HD inline u32 errprof_run_right(const u8* text, u64 p, u64 s1, u32 a) {
    u32 k = 0;
    while (k < ERRPROF_HP_CAP && p + k < s1 && text[p + k] == a) ++k;
    return k;
}
FLX_HD inline u32 errprof_hp_bin(u32 a, bool uniform, u64 run) {
    if (a < 1u || a > 4u || !uniform) return ERRPROF_HP_MIXED;
    return run < ERRPROF_HP_CAP ? (u32)run : ERRPROF_HP_CAP;
}

// what a word adds once, whatever its length; row: the row the walk has reached
template <class Add>
FLX_HD inline void errprof_word_events(u32 op, u32 L, u64 row, u64 len, bool reverse, Add&& add) {
    if (op == 7u) add(EP_EQ_RUN + (L < 256u ? L : 256u) - 1u, 1u);
    else if (op == 1u) add(EP_INS_LEN + (L < 64u ? L : 64u) - 1u, 1u);
    else if (op == 2u) {
        add(EP_DEL_LEN + (L < 64u ? L : 64u) - 1u, 1u);
        u64 const r = len == 0 ? 0 : row < len - 1 ? row : len - 1;
        add(EP_POS_DEL + errprof_bin(reverse && len ? len - 1 - r : r, len), 1u);
    }
}
// what a word adds per column and per row; p, row: its first position in `text` and its first row; q(r): the oriented read rank at row r
template <class Query, class Add>
FLX_HD inline void errprof_word_columns(u32 op, u32 L, u64 p, u64 row, ErrprofJob const& j, const u8* text, Query&& q, Add&& add) {
    bool const reverse = j.reverse != 0;
    if (op == 7u || op == 8u) {
        u32 const section = op == 7u ? EP_PAIR_EQ : EP_PAIR_X;
        for (u32 c = 0; c < L; ++c) add(section + errprof_rank(text[p + c]) * 6u + errprof_rank(q(row + c)), 1u);
        errprof_pos_rows(op == 7u ? EP_POS_MATCH : EP_POS_MISMATCH, row, L, j.read_len, reverse, add);
    } else if (op == 1u) {
        u32 const a = errprof_rank(q(row));
        bool uniform = true;
        for (u32 c = 0; c < L; ++c) {
            u32 const x = errprof_rank(q(row + c));
            add(EP_INS_LETTER + x, 1u);
            uniform = uniform && x == a;
        }
        bool const scan = a >= 1u && a <= 4u && uniform;
        add(EP_HP_INS + errprof_hp_bin(a, uniform, scan ? (u64)errprof_run_left(text, p, j.s0, a) + errprof_run_right(text, p, j.s1, a) : 0), 1u);
        errprof_pos_rows(EP_POS_INS, row, L, j.read_len, reverse, add);
    } else if (op == 2u) {
        u32 const a = errprof_rank(text[p]);
        bool uniform = true;
        for (u32 c = 0; c < L; ++c) {
            u32 const x = errprof_rank(text[p + c]);
            add(EP_DEL_LETTER + x, 1u);
            uniform = uniform && x == a;
        }
        bool const scan = a >= 1u && a <= 4u && uniform && L < ERRPROF_HP_CAP;      // (a longer one is bin 32 whatever stands next to it)
        add(EP_HP_DEL + errprof_hp_bin(a, uniform, (u64)L + (scan ? errprof_run_left(text, p, j.s0, a) + errprof_run_right(text, p + L, j.s1, a) : 0u)), 1u);
    } else if (op == 4u) {
        errprof_pos_rows(EP_POS_CLIP, row, L, j.read_len, reverse, add);
    }
}
// a record's own sums (each below 2^31: ERRPROF_MAX_RECORD) and what it adds at its end
struct ErrprofSums { u32 matches, mismatches, ins_events, ins_bases, del_events, del_bases, clip_bases; };
FLX_HD inline void errprof_sums_word(ErrprofSums& s, u32 op, u32 L) {
    if (op == 7u) s.matches += L;
    else if (op == 8u) s.mismatches += L;
    else if (op == 1u) { s.ins_events += 1u; s.ins_bases += L; }
    else if (op == 2u) { s.del_events += 1u; s.del_bases += L; }
    else if (op == 4u) s.clip_bases += L;
}
template <class Add>
FLX_HD inline void errprof_record_end(ErrprofSums const& s, Add&& add) {
    add(EP_TOTALS + EP_RECORDS, 1u);
    if (s.matches) add(EP_TOTALS + EP_MATCHES, s.matches);
    if (s.mismatches) add(EP_TOTALS + EP_MISMATCHES, s.mismatches);
    if (s.ins_events) add(EP_TOTALS + EP_INS_EVENTS, s.ins_events);
    if (s.ins_bases) add(EP_TOTALS + EP_INS_BASES, s.ins_bases);
    if (s.del_events) add(EP_TOTALS + EP_DEL_EVENTS, s.del_events);
    if (s.del_bases) add(EP_TOTALS + EP_DEL_BASES, s.del_bases);
    if (s.clip_bases) add(EP_TOTALS + EP_CLIP_BASES, s.clip_bases);
    u64 const columns = (u64)s.matches + s.mismatches + s.ins_bases + s.del_bases;      // (a counted record has a reference-consuming column)
    add(EP_IDENTITY + (columns ? (u32)((u64)s.matches * 100u / columns) : 0u), 1u);
}

// the walk of one judged job into `table` (ERRPROF_ENTRIES entries); read: the read as given, text: what the job's offsets refer to
inline void errprof_walk(ErrprofJob const& j, const uint32_t* cigar_words, const uint8_t* text, const uint8_t* read, uint64_t* table) {
    auto add = [&](u32 entry, u32 count) { table[entry] += count; };
    auto q = [&](u64 r) { return (u32)pileup_oriented_rank(read, j.read_len, j.reverse != 0, r); };
    ErrprofSums sums{};
    u64 p = j.text_off, row = 0;
    for (u32 t = 0; t < j.n_words; ++t) {
        uint32_t const w = cigar_words[j.word_off + t], op = w & 15u, L = w >> 4;
        errprof_word_events(op, L, row, j.read_len, j.reverse != 0, add);
        errprof_word_columns(op, L, p, row, j, text, q, add);
        errprof_sums_word(sums, op, L);
        if (coverage_op_consumes(op)) p += L;
        if (pileup_op_consumes_query(op)) row += L;
    }
    errprof_record_end(sums, add);
}

// ---- the launch of flx_errprof.hip (returns the hipError_t of its launch; pointers are device pointers)
struct ErrprofDevice {
    static constexpr u32 ADD_GRID_CAP = 1u << 11;      // most blocks (four waves, a record each at a time) of an errprof_add launch
    static int add(void* stream, const ErrprofJob* d_jobs, u32 n_jobs, const u32* d_words, const u8* d_text, const u8* d_letters, unsigned long long* d_table,
                   u32 flush_threshold);
};

}  // namespace flx
