// Diploid small-variant calls (flx_variants, include/floxer_amd.h): the rule, in one place, for the host and the device. The judgement of
// options and records that flx_variants_host, flx_variants_add_records and flx_variants_add_run share (it is pileup's), the key of an
// insertion or deletion event, the two candidates of a position and their genotype (FLX_HD: the kernels of flx_variants.hip run them as
// they stand) and the whole finish on the host for the host hook. The object and the C ABI: flx_variants_api.cpp.
//
//   which records count   pileup's filter (flx_pileup.hpp), with count_secondary and min_mapq
//   refused               all that pileup_plan refuses
//   the sums              pileup's seven planes by pileup's walk: DEPTH, DEL, A, C, G, T, INS (INS is not read by the call)
//   indel events          every I word and every D word of a counted record is one event and takes one key slot, so the slots of a
//                         record are a function of its words alone. Its anchor a is the position, in the concatenation, of the record's
//                         preceding reference-consuming column. An I word yields an allele key when such a column precedes it, its
//                         length is 1..32 and all its letters of the oriented sequence have rank 1..4; a D word when such a column
//                         precedes it and its length is 1..max_del (0 takes 50; longer deletions belong to the structural-variant
//                         object). Everything else gets the consensus's void key {~0, ~0}, which sorts last and is dropped.
//   allele key            one SortKey: hi = a << 32 | kind << 28 | len with kind 0 = DEL and 1 = INS (a CIGAR length has 28 bits); lo
//                         holds an insertion's letters as consensus_key packs them and is 0 for a deletion. Key order at an anchor:
//                         deletions before insertions, shorter first, then letters. kind is at most 1: no allele key is the void key.
//   alleles               the keys sorted: each run of equal keys is an allele with its count. events(a) is the sum of the counts at a,
//                         the winner the allele with the largest count there, ties to the smaller key. Insertion and deletion events
//                         share one budget of 2^32 - 1 per object.
//   costs                 centi-phred, -1000 log10 of a probability: m a read shows the allele of a homozygous genotype, x anything
//                         else, h either allele of a heterozygous genotype; prior_het, prior_hom. 0 takes 36 / 1574 / 325 / 3000 /
//                         3301 (a per-read error of 0.08, a heterozygosity of 0.001): conventions of this project, fitted to nothing.
//                         No logarithm is computed here. m < h < x is demanded (the model is degenerate otherwise) and every cost is
//                         at most 2^20, so that every sum below stays inside 64 bits (counts are below 2^34).
//   the SNV candidate     at p, only where the text's rank R is 1..4: cov = DEPTH + DEL, n[r] as consensus_call has it (the =
//                         columns are credited to R), alt the r != R with the largest n[r], ties to the smallest rank, no candidate
//                         when that count is 0; ref_n = n[R], alt_n = n[alt], oth = cov - ref_n - alt_n
//   the indel candidate   at an anchor a with an allele: cov = DEPTH[a] + DEL[a], alt_n the winner's count, oth = events(a) - alt_n,
//                         ref_n = cov - events(a), saturating at 0. A record that ends exactly on a cannot show the allele and counts
//                         towards ref all the same: a known over-count of ref_n.
//   the genotype          L_RR = ref_n m + (alt_n + oth) x, L_RA = (ref_n + alt_n) h + oth x, L_AA = alt_n m + (ref_n + oth) x;
//                         Q_RR = L_RR, Q_RA = L_RA + prior_het, Q_AA = L_AA + prior_hom. The genotype is the smallest Q, ties in the
//                         order RR, RA, AA. A row is written iff the genotype is not RR, cov >= min_depth (0 takes 4) and qual =
//                         Q_RR - min(Q_RA, Q_AA) >= min_qual (0 takes 2000). gq = (second smallest Q - smallest) / 100, at most 99;
//                         pl[g] = (L_g - min L) / 100; qual, pl and the row's counts saturate at 2^32 - 1.
//   the rows              in position order, the SNV row in front of the indel row of the same position: at most two per position
//                         (biallelic). An SNV inside a called deletion is written independently: there is no * allele. 2^32 rows or
//                         more: FLX_ERR_CAPACITY.
#pragma once
#include "flx_consensus.hpp"

namespace flx {

constexpr u32 VARIANTS_DEFAULT_MIN_DEPTH = 4, VARIANTS_DEFAULT_MIN_QUAL = 2000, VARIANTS_DEFAULT_MAX_DEL = 50;
constexpr u32 VARIANTS_DEFAULT_MATCH = 36, VARIANTS_DEFAULT_MISMATCH = 1574, VARIANTS_DEFAULT_HET = 325, VARIANTS_DEFAULT_PRIOR_HET = 3000, VARIANTS_DEFAULT_PRIOR_HOM = 3301;
constexpr u32 VARIANTS_MAX_COST = 1u << 20;
constexpr u32 VARIANTS_MAX_LEN = (1u << 28) - 1;       // the longest deletion max_del may name: a CIGAR word's length
constexpr u64 VARIANTS_MAX_EVENTS = (1ull << 32) - 1;  // I and D events together
constexpr u64 VARIANTS_MAX_ROWS = 1ull << 32;          // all rows together stay below
enum VariantKind : u32 { VARIANT_SNV = 0, VARIANT_DEL = 1, VARIANT_INS = 2 };
enum VariantKeyKind : u32 { VARIANTS_KEY_DEL = 0, VARIANTS_KEY_INS = 1 };
enum VariantGt : u32 { VARIANT_GT_RR = 0, VARIANT_GT_RA = 1, VARIANT_GT_AA = 2 };

// the options with the defaults taken for 0
struct VariantsModel { u32 min_depth, min_qual, max_del, m, x, h, prior_het, prior_hom; };
inline VariantsModel variants_model(flx_variants_options const& o) {
    return VariantsModel{o.min_depth ? o.min_depth : VARIANTS_DEFAULT_MIN_DEPTH, o.min_qual ? o.min_qual : VARIANTS_DEFAULT_MIN_QUAL, o.max_del ? o.max_del : VARIANTS_DEFAULT_MAX_DEL,
                         o.cost_match ? o.cost_match : VARIANTS_DEFAULT_MATCH, o.cost_mismatch ? o.cost_mismatch : VARIANTS_DEFAULT_MISMATCH, o.cost_het ? o.cost_het : VARIANTS_DEFAULT_HET,
                         o.prior_het ? o.prior_het : VARIANTS_DEFAULT_PRIOR_HET, o.prior_hom ? o.prior_hom : VARIANTS_DEFAULT_PRIOR_HOM};
}
inline flx_variants_options variants_options_or_default(const flx_variants_options* o) { return o ? *o : flx_variants_options{}; }
// NULL is all zero; the reserved fields must be 0; max_del is a CIGAR length; the costs are judged with their defaults taken
inline bool variants_options_valid(const flx_variants_options* o) {
    if (!o) return true;
    for (uint32_t r : o->reserved) if (r) { set_error("flx_variants_options: the reserved fields must be 0"); return false; }
    if (o->max_del > VARIANTS_MAX_LEN) { set_error("flx_variants_options: max_del is above 2^28 - 1"); return false; }
    VariantsModel const v = variants_model(*o);
    if (v.m > VARIANTS_MAX_COST || v.x > VARIANTS_MAX_COST || v.h > VARIANTS_MAX_COST || v.prior_het > VARIANTS_MAX_COST || v.prior_hom > VARIANTS_MAX_COST) {
        set_error("flx_variants_options: a cost is above 2^20");
        return false;
    }
    if (v.h >= v.x || v.m >= v.h) { set_error("flx_variants_options: the costs must be cost_match < cost_het < cost_mismatch, the model is degenerate otherwise"); return false; }
    return true;
}
// the record filter and the judgement are pileup's: its options with this object's two switches
inline flx_pileup_options variants_filter(flx_variants_options const& o) {
    flx_pileup_options p{};
    p.count_secondary = o.count_secondary;
    p.min_mapq = o.min_mapq;
    return p;
}

// ---- the allele key (void, equality: the consensus's)
FLX_HD inline u64 variants_key_anchor(SortKey const& k) { return k.hi >> 32; }
FLX_HD inline u32 variants_key_kind(SortKey const& k) { return (u32)(k.hi >> 28 & 15u); }
FLX_HD inline u32 variants_key_length(SortKey const& k) { return (u32)(k.hi & (u64)VARIANTS_MAX_LEN); }
// The key of one I or D word: preceded: a reference-consuming column lies in front of it in the record; anchor: that column's position;
// letter(i): rank i of an I word's letters in the oriented sequence. Letters are asked for only by an I word of 1..32 letters behind a
// column; a D word asks for none.
template <class Letter>
FLX_HD inline SortKey variants_key(u32 kind, bool preceded, u64 anchor, u32 len, u32 max_del, Letter&& letter) {
    if (!preceded || len < 1u) return consensus_void_key();
    if (kind == VARIANTS_KEY_DEL) return len > max_del ? consensus_void_key() : SortKey{anchor << 32 | (u64)len, 0};
    SortKey const packed = consensus_key(true, 0, len, letter);       // (void for a length above 32 or a letter outside A C G T)
    if (consensus_key_is_void(packed)) return packed;
    return SortKey{anchor << 32 | (u64)VARIANTS_KEY_INS << 28 | (u64)len, packed.lo};
}

// the key slots of a judged job: its I and D words
inline u64 variants_job_slots(PileupJob const& j, const uint32_t* cigar_words) {
    u64 n = 0;
    for (u32 t = 0; t < j.n_words; ++t) { uint32_t const op = cigar_words[j.word_off + t] & 15u; n += op == 1u || op == 2u; }
    return n;
}
// the keys of one judged job in word order, appended (the host form of variants_indel_keys)
inline void variants_job_keys(PileupJob const& j, const uint32_t* cigar_words, const uint8_t* read, u64 read_len, u32 max_del, std::vector<SortKey>& keys) {
    u64 p = j.text_off, row = 0;
    for (u32 t = 0; t < j.n_words; ++t) {
        uint32_t const w = cigar_words[j.word_off + t], op = w & 15u, len = w >> 4;
        if (op == 1u || op == 2u)
            keys.push_back(variants_key(op == 1u ? VARIANTS_KEY_INS : VARIANTS_KEY_DEL, p > j.text_off, p - 1, len, max_del,
                                        [&](u32 i) { return (u32)pileup_oriented_rank(read, read_len, j.reverse != 0, row + i); }));
        if (coverage_op_consumes(op)) p += len;
        if (pileup_op_consumes_query(op)) row += len;
    }
}

// ---- the genotype of a candidate
struct VariantGenotype { u32 gt, gq, qual, pl[3]; };
FLX_HD inline u32 variants_saturate(u64 v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)v; }
// ref_n, alt_n, oth: below 2^34 each (sums of u32 counts); the costs at most 2^20: every sum stays below 2^57
FLX_HD inline VariantGenotype variants_genotype(u64 ref_n, u64 alt_n, u64 oth, VariantsModel const& v) {
    u64 const L[3] = {ref_n * v.m + (alt_n + oth) * v.x, (ref_n + alt_n) * v.h + oth * v.x, alt_n * v.m + (ref_n + oth) * v.x};
    u64 const Q[3] = {L[0], L[1] + v.prior_het, L[2] + v.prior_hom};
    u32 gt = 0;
    if (Q[1] < Q[gt]) gt = 1;
    if (Q[2] < Q[gt]) gt = 2;                                          // (strictly smaller: ties go RR, RA, AA)
    u64 second = ~0ull, min_l = L[0];
    for (u32 g = 0; g < 3; ++g) {
        if (g != gt && Q[g] < second) second = Q[g];
        if (L[g] < min_l) min_l = L[g];
    }
    VariantGenotype out;
    out.gt = gt;
    u64 const gq = (second - Q[gt]) / 100ull;
    out.gq = gq > 99ull ? 99u : (u32)gq;
    u64 const alt_q = Q[1] < Q[2] ? Q[1] : Q[2];
    out.qual = Q[0] > alt_q ? variants_saturate(Q[0] - alt_q) : 0u;
    for (u32 g = 0; g < 3; ++g) out.pl[g] = variants_saturate((L[g] - min_l) / 100ull);
    return out;
}
// whether the candidate's genotype makes a row
FLX_HD inline bool variants_row_stands(VariantGenotype const& g, u64 cov, VariantsModel const& v) {
    return g.gt != VARIANT_GT_RR && cov >= (u64)v.min_depth && g.qual >= v.min_qual;
}
// the row of a candidate, sequence and position left to the caller
FLX_HD inline flx_variant variants_row(u32 kind, u32 ref_rank, u32 alt_rank, u32 length, u64 ref_n, u64 alt_n, u64 cov, VariantGenotype const& g, u64 letters) {
    flx_variant r;
    r.reference_id = 0; r.position = 0;
    r.kind = kind; r.ref_rank = ref_rank; r.alt_rank = alt_rank; r.length = length;
    r.ref_count = variants_saturate(ref_n); r.alt_count = variants_saturate(alt_n); r.cov = variants_saturate(cov);
    r.gt = g.gt; r.gq = g.gq; r.qual = g.qual;
    r.pl[0] = g.pl[0]; r.pl[1] = g.pl[1]; r.pl[2] = g.pl[2];
    r.reserved = 0;
    r.letters = letters;
    return r;
}

// ---- the two candidates of a position. R: the text's rank (0..5); depth, del, acgt[4]: the position's counts behind the scans.
// true: the SNV candidate exists and makes a row (its sequence and position are the caller's to fill)
FLX_HD inline bool variants_snv(u32 R, u32 depth, u32 del, u32 const (&acgt)[4], VariantsModel const& v, flx_variant& row) {
    if (R < 1u || R > 4u) return false;
    u64 const cov = (u64)depth + (u64)del;
    u32 n[5] = {0u, acgt[0], acgt[1], acgt[2], acgt[3]};
    n[R] += depth - acgt[0] - acgt[1] - acgt[2] - acgt[3];            // (the = columns of the position, as consensus_call credits them)
    u32 alt = 0;
    for (u32 r = 1u; r <= 4u; ++r) if (r != R && (alt == 0u || n[r] > n[alt])) alt = r;      // (the first of the largest)
    if (n[alt] == 0u) return false;
    u64 const ref_n = n[R], alt_n = n[alt], shown = ref_n + alt_n, oth = cov > shown ? cov - shown : 0;
    VariantGenotype const g = variants_genotype(ref_n, alt_n, oth, v);
    if (!variants_row_stands(g, cov, v)) return false;
    row = variants_row(VARIANT_SNV, R, alt, 1u, ref_n, alt_n, cov, g, 0);
    return true;
}
// the indel candidate of an anchor whose winner is the allele (key_kind, length, count, letters), with events at the anchor
FLX_HD inline bool variants_indel(u32 R, u32 depth, u32 del, u32 events, u32 key_kind, u32 length, u32 count, u64 letters, VariantsModel const& v, flx_variant& row) {
    u64 const cov = (u64)depth + (u64)del;
    u64 const alt_n = count, oth = (u64)events - alt_n, ref_n = cov > (u64)events ? cov - (u64)events : 0;      // (the winner is one of the anchor's: events >= count)
    VariantGenotype const g = variants_genotype(ref_n, alt_n, oth, v);
    if (!variants_row_stands(g, cov, v)) return false;
    row = variants_row(key_kind == VARIANTS_KEY_INS ? VARIANT_INS : VARIANT_DEL, R, 0u, length, ref_n, alt_n, cov, g, key_kind == VARIANTS_KEY_INS ? letters : 0);
    return true;
}

// an allele as the table holds it, from its key and count; ref: the sequence that holds the anchor
FLX_HD inline flx_variant_allele variants_allele_of(SortKey const& k, u32 count, u32 ref, u64 ref_start) {
    flx_variant_allele a;
    a.reference_id = (int32_t)ref;
    a.position = (u32)(variants_key_anchor(k) - ref_start);
    a.kind = variants_key_kind(k) == VARIANTS_KEY_INS ? VARIANT_INS : VARIANT_DEL;
    a.length = variants_key_length(k);
    a.count = count;
    a.reserved = 0;
    a.letters = k.lo;
    return a;
}
FLX_HD inline u32 variants_allele_key_kind(flx_variant_allele const& a) { return a.kind == VARIANT_INS ? VARIANTS_KEY_INS : VARIANTS_KEY_DEL; }

// ---- the finish on the host: counts are pileup's seven planes (plane-major, `total` entries each, DEPTH and DEL summed), keys the
// events' keys in any order (sorted here). false: the rows would reach 2^32 (nothing is returned then).
struct VariantsResult {
    std::vector<flx_variant> rows;
    std::vector<flx_variant_allele> alleles;
};
inline bool variants_finish_host(std::vector<u64> const& starts, const uint8_t* text, const uint32_t* counts, std::vector<SortKey>& keys, VariantsModel const& v, VariantsResult& out) {
    u64 const total = starts.back();
    std::sort(keys.begin(), keys.end(), [](SortKey const& a, SortKey const& b) { return sort_key_less(a, b); });
    while (!keys.empty() && consensus_key_is_void(keys.back())) keys.pop_back();
    std::vector<u32> winner(total, CONSENSUS_NO_WINNER), events(total, 0);
    u32 ref = 0;
    for (size_t i = 0; i < keys.size();) {
        size_t e = i;
        while (e < keys.size() && consensus_key_equal(keys[e], keys[i])) ++e;
        u64 const a = variants_key_anchor(keys[i]);
        u32 const w = winner[a], count = (u32)(e - i);
        if (w == CONSENSUS_NO_WINNER || count > out.alleles[w].count) winner[a] = (u32)out.alleles.size();      // (key order: an earlier allele keeps a tie)
        events[a] += count;
        while (starts[ref + 1] <= a) ++ref;
        out.alleles.push_back(variants_allele_of(keys[i], count, ref, starts[ref]));
        i = e;
    }
    ref = 0;
    for (u64 p = 0; p < total; ++p) {
        while (starts[ref + 1] <= p) ++ref;
        u32 const depth = counts[(u64)PILEUP_DEPTH * total + p], del = counts[(u64)PILEUP_DEL * total + p];
        u32 const acgt[4] = {counts[(u64)PILEUP_A * total + p], counts[(u64)PILEUP_C * total + p], counts[(u64)PILEUP_G * total + p], counts[(u64)PILEUP_T * total + p]};
        flx_variant row;
        bool made = variants_snv(text[p], depth, del, acgt, v, row);
        for (int pass = 0; pass < 2; ++pass) {
            if (made) {
                if (out.rows.size() + 1 >= VARIANTS_MAX_ROWS) return false;
                row.reference_id = (int32_t)ref;
                row.position = (u32)(p - starts[ref]);
                out.rows.push_back(row);
            }
            if (pass == 1 || winner[p] == CONSENSUS_NO_WINNER) break;
            flx_variant_allele const& al = out.alleles[winner[p]];
            made = variants_indel(text[p], depth, del, events[p], variants_allele_key_kind(al), al.length, al.count, al.letters, v, row);
        }
    }
    return true;
}

// ---- the launches of flx_variants.hip (each returns the hipError_t of its launch; pointers are device pointers). The accumulator is
// pileup's seven planes and an eighth, of `stride` entries each. text_delta[r]: what is added to a position of sequence r in the
// concatenation to reach its letter in d_text (0 for an unpadded text).
constexpr u32 VARIANTS_PLANE_EVENTS = PILEUP_PLANES;   // the eighth plane: events(a), written by variants_anchor_winners
constexpr u32 VARIANTS_PLANES = PILEUP_PLANES + 1;
struct VariantsDevice {
    static constexpr u32 KEYS_GRID_CAP = 2048;         // most blocks (four waves, a record each at a time) of a variants_indel_keys launch
    static constexpr u32 KEYS_WAVES = 4;
    // d_keys[d_key_off[job] + slot] for every I and D word of every job
    static int indel_keys(void* stream, const PileupJob* d_jobs, const u64* d_key_off, u32 n_jobs, const u32* d_words, const u8* d_letters, u32 max_del, SortKey* d_keys);
    // the alleles as the table holds them; d_winner[anchor] = the index of the anchor's winning allele (cleared to CONSENSUS_NO_WINNER by
    // the caller) and d_events[anchor] = the sum of the counts of the anchor's alleles (cleared to 0 by the caller)
    static int anchor_winners(void* stream, const SortKey* d_sorted, const u32* d_run_start, const u32* d_run_end, u32 n_alleles, const u32* d_starts, u32 n_refs,
                              flx_variant_allele* d_alleles, u32* d_winner, u32* d_events);
    // mode 0: d_count[tile] = the tile's rows, *d_rows += them (the u32 scan of the counts cannot tell 2^32 rows from none). mode 1
    // (d_count scanned by then): the rows themselves. The winners lie in the INS plane, events(a) in the eighth.
    static int call(void* stream, int mode, const u32* d_acc, u64 stride, u64 total, const u32* d_starts, u32 n_refs, const u8* d_text, const i64* d_text_delta,
                    const flx_variant_allele* d_alleles, VariantsModel v, u32* d_count, unsigned long long* d_rows, flx_variant* d_out);
};

}  // namespace flx
