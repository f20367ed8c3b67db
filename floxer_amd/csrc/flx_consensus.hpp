// Consensus sequence (flx_consensus, include/floxer_amd.h): the rule, in one place, for the host and the device. The judgement of options
// and records that flx_consensus_host, flx_consensus_add_records and flx_consensus_add_run share (it is pileup's), the key of an
// insertion event, the call of one position (FLX_HD: the kernels of flx_consensus.hip run it as it stands) and the whole finish on the
// host for the host hook. The object and the C ABI: flx_consensus_api.cpp.
//
//   which records count   pileup's filter (flx_pileup.hpp), with count_secondary and min_mapq
//   refused               all that pileup_plan refuses
//   the sums              pileup's seven planes by pileup's walk: DEPTH, DEL, A, C, G, T, INS (INS is not read by the call)
//   insertion events      every I word of a counted record is one event and takes one key slot, so the slots of a record are a function
//                         of its words alone. Its anchor a is the position, in the concatenation, of the record's preceding
//                         reference-consuming column. It yields an allele key when such a column precedes it in the record, its
//                         length is 1..32 and all its letters of the oriented sequence have rank 1..4; otherwise the void key
//                         {~0, ~0}, which sorts last and is dropped.
//   allele key            one SortKey: hi = a << 8 | len; lo holds the letters two bits each, letter k as (rank - 1) << (62 - 2k), the
//                         unused low bits 0. Key order is (anchor, length, letters lexicographic); equal keys are interchangeable.
//   alleles               the keys sorted: each run of equal keys is an allele with its count. The winner at an anchor is the allele
//                         with the largest count there, ties to the smaller key.
//   the call at p         R the text's rank, cov = DEPTH + DEL, n[r] = plane r + (R == r ? DEPTH - A - C - G - T : 0) for r in A, C,
//                         G, T (a rank R of 1..4 stands for its = columns), n[DEL] = DEL.
//                           cov < min_depth: uncalled: R's letter, or N under mask_low_depth; no insertion, no change row
//                           otherwise best = the largest of the five, ties to R when R is among the tied, else to the first of A, C,
//                           G, T, DEL. best != R stands only with n[best] >= min_count and n[best] * 1000 >= min_permille * cov
//                           (64-bit); otherwise R stays. A rank outside 1..4 is written N, a position called DEL emits no letter.
//                           The winning insertion behind p is applied iff cov >= min_depth and its count meets the same two
//                           thresholds, also when p itself is called DEL.
//   the outputs           out_len[p] = 0 or 1 plus the inserted length; the exclusive scan of out_len over the concatenation places
//                         every position's letters in one ASCII pool; a sequence's consensus is the slice between its first
//                         position's offset and the next sequence's (it may be empty); 2^32 letters or more in all: FLX_ERR_CAPACITY.
//                         The changes: every place the consensus departs from the text, in position order, SUB or DEL in front of the
//                         INS of the same position (a masked N is no change).
//   defaults              0 takes min_depth 3, min_count 2, min_permille 500: conventions of this project, fitted to nothing.
#pragma once
#include "flx_errprof.hpp"
#include "flx_sort.hpp"

namespace flx {

constexpr u32 CONSENSUS_DEFAULT_MIN_DEPTH = 3, CONSENSUS_DEFAULT_MIN_COUNT = 2, CONSENSUS_DEFAULT_MIN_PERMILLE = 500;
constexpr u32 CONSENSUS_MAX_INS = 32;                  // the longest allele: 64 bits of letters
constexpr u64 CONSENSUS_MAX_EVENTS = (1ull << 32) - 1;
constexpr u64 CONSENSUS_MAX_LETTERS = 1ull << 32;      // all letters together stay below
enum ConsensusKind : u32 { CONSENSUS_SUB = 0, CONSENSUS_DEL = 1, CONSENSUS_INS = 2 };
constexpr u32 CONSENSUS_CALL_DEL = 5;                  // the fifth candidate of a call, behind the ranks 1..4
constexpr u32 CONSENSUS_NO_WINNER = 0xFFFFFFFFu;       // a position without an allele

// NULL is all zero; the reserved fields must be 0; a fraction above 1000 permille is none
inline bool consensus_options_valid(const flx_consensus_options* o) {
    if (!o) return true;
    for (uint32_t r : o->reserved) if (r) { set_error("flx_consensus_options: the reserved fields must be 0"); return false; }
    if (o->min_permille > 1000u) { set_error("flx_consensus_options: min_permille is above 1000"); return false; }
    return true;
}
inline flx_consensus_options consensus_options_or_default(const flx_consensus_options* o) { return o ? *o : flx_consensus_options{}; }
// the record filter and the judgement are pileup's: its options with this object's two switches
inline flx_pileup_options consensus_filter(flx_consensus_options const& o) {
    flx_pileup_options p{};
    p.count_secondary = o.count_secondary;
    p.min_mapq = o.min_mapq;
    return p;
}
// (the text is judged as the error profile judges its own: errprof_text_valid)

// the thresholds with the defaults taken for 0, and the mask switch
struct ConsensusThresholds { u32 min_depth, min_count, min_permille, mask_low_depth; };
inline ConsensusThresholds consensus_thresholds(flx_consensus_options const& o) {
    return ConsensusThresholds{o.min_depth ? o.min_depth : CONSENSUS_DEFAULT_MIN_DEPTH, o.min_count ? o.min_count : CONSENSUS_DEFAULT_MIN_COUNT,
                               o.min_permille ? o.min_permille : CONSENSUS_DEFAULT_MIN_PERMILLE, o.mask_low_depth ? 1u : 0u};
}

// ---- the allele key
FLX_HD inline SortKey consensus_void_key() { return SortKey{~0ull, ~0ull}; }
FLX_HD inline bool consensus_key_is_void(SortKey const& k) { return k.hi == ~0ull; }       // (an anchor lies below 2^32: no allele key has it)
FLX_HD inline bool consensus_key_equal(SortKey const& a, SortKey const& b) { return a.hi == b.hi && a.lo == b.lo; }
FLX_HD inline u64 consensus_key_anchor(SortKey const& k) { return k.hi >> 8; }
FLX_HD inline u32 consensus_key_length(SortKey const& k) { return (u32)(k.hi & 255u); }
FLX_HD inline u32 consensus_key_letter(u64 lo, u32 i) { return (u32)(lo >> (62u - 2u * i) & 3u) + 1u; }      // the rank of letter i < length
// The key of one I word: preceded: a reference-consuming column lies in front of it in the record; anchor: that column's position;
// letter(i): rank i of the word's letters in the oriented sequence. Letters of a word that is void for its length are not asked for.
template <class Letter>
FLX_HD inline SortKey consensus_key(bool preceded, u64 anchor, u32 len, Letter&& letter) {
    if (!preceded || len < 1u || len > CONSENSUS_MAX_INS) return consensus_void_key();
    u64 lo = 0;
    for (u32 i = 0; i < len; ++i) {
        u32 const r = letter(i);
        if (r < 1u || r > 4u) return consensus_void_key();
        lo |= (u64)(r - 1u) << (62u - 2u * i);
    }
    return SortKey{anchor << 8 | (u64)len, lo};
}

// the key slots of a judged job: its I words
inline u64 consensus_job_slots(PileupJob const& j, const uint32_t* cigar_words) {
    u64 n = 0;
    for (u32 t = 0; t < j.n_words; ++t) n += (cigar_words[j.word_off + t] & 15u) == 1u;
    return n;
}
// the keys of one judged job in word order, appended (the host form of consensus_ins_keys)
inline void consensus_job_keys(PileupJob const& j, const uint32_t* cigar_words, const uint8_t* read, u64 read_len, std::vector<SortKey>& keys) {
    u64 p = j.text_off, row = 0;
    for (u32 t = 0; t < j.n_words; ++t) {
        uint32_t const w = cigar_words[j.word_off + t], op = w & 15u, len = w >> 4;
        if (op == 1u) keys.push_back(consensus_key(p > j.text_off, p - 1, len, [&](u32 i) { return (u32)pileup_oriented_rank(read, read_len, j.reverse != 0, row + i); }));
        if (coverage_op_consumes(op)) p += len;
        if (pileup_op_consumes_query(op)) row += len;
    }
}

// ---- the call of one position
// emit: 0 no letter (called DEL), 1..4 that rank's letter, 5 N; sub_or_del: the position departs from the text (alt: the called
// candidate, 1..4 or CONSENSUS_CALL_DEL; count: its n); called: cov >= min_depth, the position may take its winning insertion
struct ConsensusCall { u32 emit; u32 called; u32 sub_or_del; u32 alt; u32 count; u32 cov; };
FLX_HD inline bool consensus_meets(u32 count, u64 cov, ConsensusThresholds const& t) {
    return count >= t.min_count && (u64)count * 1000ull >= (u64)t.min_permille * cov;
}
// R: the text's rank (0..5); depth, del and acgt[4]: the position's counts behind the scans. (cov is u32 arithmetic modulo 2^32 nowhere:
// it is formed in 64 bits and compared there; the row's cov field saturates at 2^32 - 1.)
FLX_HD inline ConsensusCall consensus_call(u32 R, u32 depth, u32 del, u32 const (&acgt)[4], ConsensusThresholds const& t) {
    u64 const cov = (u64)depth + (u64)del;
    u32 const letter = R >= 1u && R <= 4u ? R : 5u;
    ConsensusCall c{letter, 0u, 0u, 0u, 0u, cov > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)cov};
    if (cov < (u64)t.min_depth) {
        if (t.mask_low_depth) c.emit = 5u;
        return c;
    }
    c.called = 1u;
    u32 n[6] = {0u, acgt[0], acgt[1], acgt[2], acgt[3], del};
    if (R >= 1u && R <= 4u) n[R] += depth - acgt[0] - acgt[1] - acgt[2] - acgt[3];       // (the = columns of the position; an X column adds to at most one plane)
    u32 best = 1u;
    for (u32 r = 2u; r <= CONSENSUS_CALL_DEL; ++r) if (n[r] > n[best]) best = r;
    bool const stays = R >= 1u && R <= 4u && n[R] == n[best];            // (R = 5 is the letter N, not the fifth candidate)
    if (stays || !consensus_meets(n[best], cov, t)) return c;
    c.sub_or_del = 1u;
    c.alt = best;
    c.count = n[best];
    c.emit = best == CONSENSUS_CALL_DEL ? 0u : best;
    return c;
}
FLX_HD inline char consensus_letter(u32 emit) { return emit == 1u ? 'A' : emit == 2u ? 'C' : emit == 3u ? 'G' : emit == 4u ? 'T' : 'N'; }

// the call word of a position, as consensus_call leaves it for consensus_emit: bits 0..2 emit, bits 8..13 the inserted length
FLX_HD inline u32 consensus_call_word(u32 emit, u32 ins_len) { return emit | ins_len << 8; }
FLX_HD inline u32 consensus_word_emit(u32 w) { return w & 7u; }
FLX_HD inline u32 consensus_word_ins(u32 w) { return w >> 8 & 63u; }
FLX_HD inline u32 consensus_word_len(u32 w) { return (consensus_word_emit(w) ? 1u : 0u) + consensus_word_ins(w); }

// an allele as the tables hold it, from its key and count; ref: the sequence that holds the anchor
FLX_HD inline flx_consensus_allele consensus_allele_of(SortKey const& k, u32 count, u32 ref, u64 ref_start) {
    flx_consensus_allele a;
    a.reference_id = (int32_t)ref;
    a.position = (u32)(consensus_key_anchor(k) - ref_start);
    a.length = consensus_key_length(k);
    a.count = count;
    a.letters = k.lo;
    return a;
}
FLX_HD inline flx_consensus_change consensus_change_row(u32 ref, u32 position, u32 kind, u32 ref_rank, u32 alt_rank, u32 length, u32 count, u32 cov, u64 letters) {
    flx_consensus_change c;
    c.reference_id = (int32_t)ref;
    c.position = position;
    c.kind = kind; c.ref_rank = ref_rank; c.alt_rank = alt_rank; c.length = length; c.count = count; c.cov = cov;
    c.letters = letters;
    return c;
}

// ---- the finish on the host: counts are pileup's seven planes (plane-major, `total` entries each, DEPTH and DEL summed), keys the
// events' keys in any order (sorted here). false: the letters would reach 2^32 (nothing is returned then).
struct ConsensusResult {
    std::vector<u64> letter_offsets;                   // n_refs + 1
    std::string letters;
    std::vector<flx_consensus_change> changes;
    std::vector<flx_consensus_allele> alleles;
};
inline bool consensus_finish_host(std::vector<u64> const& starts, const uint8_t* text, const uint32_t* counts, std::vector<SortKey>& keys, ConsensusThresholds const& t,
                                  ConsensusResult& out) {
    u64 const total = starts.back();
    u32 const n_refs = (u32)(starts.size() - 1);
    std::sort(keys.begin(), keys.end(), [](SortKey const& a, SortKey const& b) { return sort_key_less(a, b); });
    while (!keys.empty() && consensus_key_is_void(keys.back())) keys.pop_back();
    std::vector<u32> winner(total, CONSENSUS_NO_WINNER), allele_count;
    std::vector<SortKey> allele_key;
    for (size_t i = 0; i < keys.size();) {
        size_t e = i;
        while (e < keys.size() && consensus_key_equal(keys[e], keys[i])) ++e;
        u64 const a = consensus_key_anchor(keys[i]);
        u32 const w = winner[a];
        if (w == CONSENSUS_NO_WINNER || (u32)(e - i) > allele_count[w]) winner[a] = (u32)allele_key.size();      // (key order: an earlier allele keeps a tie)
        allele_key.push_back(keys[i]);
        allele_count.push_back((u32)(e - i));
        i = e;
    }
    u32 ref = 0;
    for (size_t j = 0; j < allele_key.size(); ++j) {
        while (starts[ref + 1] <= consensus_key_anchor(allele_key[j])) ++ref;
        out.alleles.push_back(consensus_allele_of(allele_key[j], allele_count[j], ref, starts[ref]));
    }
    // the letters are counted first: nothing is written when they would reach 2^32
    std::vector<u32> word(total);
    u64 n_letters = 0;
    ref = 0;
    out.letter_offsets.assign((size_t)n_refs + 1, 0);
    for (u64 p = 0; p < total; ++p) {
        while (starts[ref + 1] <= p) ++ref;
        if (p == starts[ref]) out.letter_offsets[ref] = n_letters;
        u32 const acgt[4] = {counts[(u64)PILEUP_A * total + p], counts[(u64)PILEUP_C * total + p], counts[(u64)PILEUP_G * total + p], counts[(u64)PILEUP_T * total + p]};
        ConsensusCall const c = consensus_call(text[p], counts[(u64)PILEUP_DEPTH * total + p], counts[(u64)PILEUP_DEL * total + p], acgt, t);
        u32 const w = winner[p];
        bool const ins = c.called && w != CONSENSUS_NO_WINNER && consensus_meets(allele_count[w], (u64)counts[(u64)PILEUP_DEPTH * total + p] + counts[(u64)PILEUP_DEL * total + p], t);
        if (c.sub_or_del)
            out.changes.push_back(consensus_change_row(ref, (u32)(p - starts[ref]), c.alt == CONSENSUS_CALL_DEL ? CONSENSUS_DEL : CONSENSUS_SUB, text[p],
                                                       c.alt == CONSENSUS_CALL_DEL ? 0u : c.alt, 1u, c.count, c.cov, 0));
        if (ins)
            out.changes.push_back(consensus_change_row(ref, (u32)(p - starts[ref]), CONSENSUS_INS, text[p], 0u, consensus_key_length(allele_key[w]), allele_count[w], c.cov,
                                                       allele_key[w].lo));
        word[p] = consensus_call_word(c.emit, ins ? consensus_key_length(allele_key[w]) : 0u);
        n_letters += consensus_word_len(word[p]);
    }
    out.letter_offsets[n_refs] = n_letters;
    if (n_letters >= CONSENSUS_MAX_LETTERS) return false;
    out.letters.reserve(n_letters);
    for (u64 p = 0; p < total; ++p) {
        if (consensus_word_emit(word[p])) out.letters.push_back(consensus_letter(consensus_word_emit(word[p])));
        for (u32 i = 0; i < consensus_word_ins(word[p]); ++i) out.letters.push_back(consensus_letter(consensus_key_letter(allele_key[winner[p]].lo, i)));
    }
    return true;
}

// ---- the launches of flx_consensus.hip (each returns the hipError_t of its launch; pointers are device pointers). The accumulator is
// pileup's: seven planes of `stride` entries each. text_delta[r]: what is added to a position of sequence r in the concatenation to
// reach its letter in d_text (0 for an unpadded text).
struct ConsensusDevice {
    static constexpr u32 KEYS_GRID_CAP = 2048;         // most blocks (four waves, a record each at a time) of a consensus_ins_keys launch
    static constexpr u32 KEYS_WAVES = 4;
    // d_keys[d_key_off[job] + slot] for every I word of every job
    static int ins_keys(void* stream, const PileupJob* d_jobs, const u64* d_key_off, u32 n_jobs, const u32* d_words, const u8* d_letters, SortKey* d_keys);
    // d_flags[i] = 1 where sorted key i starts a run of equal keys that are not void
    static int allele_heads(void* stream, const SortKey* d_sorted, u64 n, u32* d_flags);
    // d_ids: the flags inclusively scanned; run_start / run_end [allele]: the run's first key and the key behind its last
    static int allele_fill(void* stream, const SortKey* d_sorted, const u32* d_ids, u64 n, u32* d_run_start, u32* d_run_end);
    // the alleles as the tables hold them, and d_winner[anchor] = the index of the anchor's winning allele (cleared to CONSENSUS_NO_WINNER by the caller)
    static int allele_winners(void* stream, const SortKey* d_sorted, const u32* d_run_start, const u32* d_run_end, u32 n_alleles, const u32* d_starts, u32 n_refs,
                              flx_consensus_allele* d_alleles, u32* d_winner);
    // mode 0: d_count[tile] = the tile's change rows, *d_letters += the tile's letters. mode 1 (d_count scanned by then): the rows
    // themselves; out_len[p] then replaces DEPTH and the call word DEL, in place. The winners lie in the INS plane.
    static int call(void* stream, int mode, u32* d_acc, u64 stride, u64 total, const u32* d_starts, u32 n_refs, const u8* d_text, const i64* d_text_delta,
                    const flx_consensus_allele* d_alleles, ConsensusThresholds t, u32* d_count, unsigned long long* d_letters, flx_consensus_change* d_out);
    // behind the inclusive scan of out_len (in the DEPTH plane): every position's letters at its offset in d_pool
    static int emit(void* stream, const u32* d_acc, u64 stride, u64 total, const flx_consensus_allele* d_alleles, char* d_pool);
    // d_offsets[r] = the offset of sequence r's first letter, d_offsets[n_refs] = all letters
    static int offsets(void* stream, const u32* d_acc, u64 stride, u64 total, const u32* d_starts, u32 n_refs, u32* d_offsets);
};

}  // namespace flx
