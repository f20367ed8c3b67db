// Read-backed phasing of heterozygous calls (flx_phase, include/floxer_amd.h): the rule, in one place, for the host and the device. The
// judgement of options and sites, the observation of a site by a record, the link, the chain, the tag and the vote (FLX_HD: the kernels
// of flx_phase.hip run them as they stand) and the whole rule on the host for the host hook. The object and the C ABI: flx_phase_api.cpp.
//
//   sites                 given at create time, strictly increasing by (reference_id, position, kind); kind is VariantKind; position the
//                         SNV's position or the indel's anchor; letters as consensus_key packs them, 0 for an SNV or a DEL. Refused: an
//                         SNV whose text rank is outside 1..4 or equals alt_rank (or whose alt_rank is outside 1..4), a DEL that runs
//                         past its sequence, an INS of more than 32 letters (a packed letter cannot lie outside 1..4; bits behind the
//                         length are refused), a non-zero reserved, more than 2^32 - 2 sites. The site index is a u32.
//   which records count   pileup's filter and refusals (pileup_plan), with count_secondary and min_mapq. The unit is the counted record.
//   slots                 a record has one slot per site whose anchor lies in [text_off, text_end): slot k is site first + k, first and
//                         the count found by binary search over the anchors in concatenation coordinates
//   observation           one byte, REF 0, ALT 1, NONE 2. SNV: the column at the anchor is an = word: REF; an X word whose oriented
//                         letter there equals alt_rank: ALT; anything else NONE. DEL / INS: E is the run of I and D words directly
//                         behind the column at the anchor a (empty unless a is the last column of its word); the site's key is
//                         variants_key(kind, true, a, length, VARIANTS_MAX_LEN, letters); a word of E whose key, made as
//                         variants_indel_keys makes it (its own anchor, max_del = VARIANTS_MAX_LEN), equals it: ALT; otherwise E empty,
//                         the column = or X and a + 1 < text_end: REF; otherwise NONE.
//   links                 for sites i and i + 1, over every record that observes both with REF or ALT: cis(i) equal alleles, trans(i)
//                         unequal ones
//   chain                 connected(i): both in one sequence and |cis - trans| >= min_link (0 takes 2); flip(i) = trans > cis; a phase
//                         set is a maximal run of connected neighbours, its id the index of its first site; p(first) = 0,
//                         p(i + 1) = p(i) ^ flip(i); a set of one site is unphased. p = 0: ALT on haplotype 1 (1|0); p = 1: 0|1.
//   tags                  a record's slots of phased sites fall into runs of equal phase set; the record belongs to the run with the
//                         most REF/ALT observations, ties to the first, none: hap 0 and phase_set PHASE_NO_SET. In the run
//                         x = allele ^ p(site), h1 counts x == 1, h2 x == 0; hap 1 if h1 - h2 >= min_margin, 2 if h2 - h1 >= min_margin
//                         (0 takes 1), else 0.
//   refinement            refine_rounds rounds (0 takes 1, at most 8; skip_refine: none): every tagged record votes at every REF/ALT
//                         slot of its run, keep(i) counts x == (hap == 1), swap(i) the rest; where swap > keep, p flips; the tags are
//                         made again. keep and swap as reported are the last round's, before its flips.
// Known limits: links join neighbouring sites only, so a site whose observations are noise (a false 0/1) splits a set in two, and
// bridging over it is out of scope; there are no base qualities and no read-pair or supplementary linkage; the defaults 2 / 1 / 1 are
// conventions of this project, fitted to nothing.
#pragma once
#include "flx_variants.hpp"

namespace flx {

constexpr u32 PHASE_REF = 0, PHASE_ALT = 1, PHASE_NONE = 2;
constexpr u32 PHASE_DEFAULT_MIN_LINK = 2, PHASE_DEFAULT_MIN_MARGIN = 1, PHASE_DEFAULT_ROUNDS = 1, PHASE_MAX_ROUNDS = 8;
constexpr u64 PHASE_MAX_SITES = (1ull << 32) - 2;      // the site index and one past it are u32
constexpr u64 PHASE_MAX_SLOTS = (1ull << 32) - 1;      // observation slots of one object
constexpr u32 PHASE_NO_SET = 0xFFFFFFFFu;              // a tag without a run (no site index reaches it)
constexpr u32 PHASE_BIT_P = 1u, PHASE_BIT_PHASED = 2u; // a site's state word: p and whether its set has more than one site

// the options with the defaults taken for 0; rounds 0: no refinement
struct PhaseModel { u32 min_link, min_margin, rounds; };
inline PhaseModel phase_model(flx_phase_options const& o) {
    return PhaseModel{o.min_link ? o.min_link : PHASE_DEFAULT_MIN_LINK, o.min_margin ? o.min_margin : PHASE_DEFAULT_MIN_MARGIN,
                      o.skip_refine ? 0u : o.refine_rounds ? o.refine_rounds : PHASE_DEFAULT_ROUNDS};
}
inline flx_phase_options phase_options_or_default(const flx_phase_options* o) { return o ? *o : flx_phase_options{}; }
// NULL is all zero; the reserved fields must be 0; at most eight rounds
inline bool phase_options_valid(const flx_phase_options* o) {
    if (!o) return true;
    for (uint32_t r : o->reserved) if (r) { set_error("flx_phase_options: the reserved fields must be 0"); return false; }
    if (o->refine_rounds > PHASE_MAX_ROUNDS) { set_error("flx_phase_options: refine_rounds is above 8"); return false; }
    return true;
}
inline flx_pileup_options phase_filter(flx_phase_options const& o) {
    flx_pileup_options p{};
    p.count_secondary = o.count_secondary;
    p.min_mapq = o.min_mapq;
    return p;
}

// Judges the sites against the sequences and the text (rank(r, p): the text's rank at position p of sequence r) and fills anchors[s],
// the site's anchor in the unpadded concatenation. 0, or the FLX_ERR_* behind set_error.
template <class Rank>
inline int phase_sites_valid(std::vector<u64> const& starts, Rank&& rank, const flx_phase_site* sites, u64 n, const char* who, std::vector<u32>& anchors) {
    if (n > PHASE_MAX_SITES) { set_error(std::string(who) + ": more than 2^32 - 2 sites"); return FLX_ERR_CAPACITY; }
    if (n && !sites) { set_error(std::string(who) + ": null argument"); return FLX_ERR_INVALID; }
    size_t const n_refs = starts.size() - 1;
    anchors.resize(n);
    for (u64 s = 0; s < n; ++s) {
        flx_phase_site const& v = sites[s];
        std::string const site = std::string(who) + ": site " + std::to_string(s);
        if (v.reserved) { set_error(site + " has a non-zero reserved field"); return FLX_ERR_INVALID; }
        if (v.reference_id < 0 || (size_t)v.reference_id >= n_refs) { set_error(site + " names a reference_id outside the list"); return FLX_ERR_INVALID; }
        u64 const len = starts[(size_t)v.reference_id + 1] - starts[(size_t)v.reference_id];
        if (v.position >= len) { set_error(site + " lies behind its sequence"); return FLX_ERR_INVALID; }
        if (v.kind > VARIANT_INS) { set_error(site + " has a kind other than SNV 0, DEL 1, INS 2"); return FLX_ERR_INVALID; }
        if (s > 0) {
            flx_phase_site const& b = sites[s - 1];
            bool const rises = b.reference_id != v.reference_id ? b.reference_id < v.reference_id : b.position != v.position ? b.position < v.position : b.kind < v.kind;
            if (!rises) { set_error(site + " does not lie behind its predecessor: the sites must be strictly increasing by (reference_id, position, kind)"); return FLX_ERR_INVALID; }
        }
        u64 const a = starts[(size_t)v.reference_id] + v.position;
        if (v.kind != VARIANT_INS && v.letters) { set_error(site + " is no insertion and has letters"); return FLX_ERR_INVALID; }
        if (v.kind == VARIANT_SNV) {
            u32 const R = rank((u64)v.reference_id, (u64)v.position);
            if (R < 1u || R > 4u) { set_error(site + " is an SNV where the text's rank is outside 1..4"); return FLX_ERR_INVALID; }
            if (v.alt_rank < 1u || v.alt_rank > 4u) { set_error(site + " is an SNV with an alt_rank outside 1..4"); return FLX_ERR_INVALID; }
            if (v.alt_rank == R) { set_error(site + " is an SNV whose alt_rank is the text's rank"); return FLX_ERR_INVALID; }
        } else if (v.kind == VARIANT_DEL) {
            if (v.length < 1u || (u64)v.position + v.length >= len) { set_error(site + " is a deletion of no base or one that runs past its sequence"); return FLX_ERR_INVALID; }
        } else {
            if (v.length < 1u || v.length > CONSENSUS_MAX_INS) { set_error(site + " is an insertion of no letter or of more than 32"); return FLX_ERR_INVALID; }
            if (v.length < 32u && (v.letters << (2u * v.length))) { set_error(site + " is an insertion with a letter outside 1..4 behind its length"); return FLX_ERR_INVALID; }
        }
        anchors[s] = (u32)a;
    }
    return FLX_OK;
}

// the slots of a record over [text_off, text_end): first site and count
inline void phase_slots(std::vector<u32> const& anchors, u64 text_off, u64 text_end, u32& first, u32& n_slots) {
    auto const lo = std::lower_bound(anchors.begin(), anchors.end(), text_off, [](u32 a, u64 p) { return (u64)a < p; });
    auto const hi = std::lower_bound(lo, anchors.end(), text_end, [](u32 a, u64 p) { return (u64)a < p; });
    first = (u32)(lo - anchors.begin());
    n_slots = (u32)(hi - lo);
}
inline u64 phase_job_end(PileupJob const& j, const uint32_t* cigar_words) {
    u64 end = j.text_off;
    for (u32 t = 0; t < j.n_words; ++t) { uint32_t const w = cigar_words[j.word_off + t]; if (coverage_op_consumes(w & 15u)) end += w >> 4; }
    return end;
}

// ---- the observation
// an indel site's key at its anchor a in the concatenation (never void: the sites were judged)
FLX_HD inline SortKey phase_site_key(u32 kind, u64 a, u32 length, u64 letters) {
    return variants_key(kind == VARIANT_INS ? VARIANTS_KEY_INS : VARIANTS_KEY_DEL, true, a, length, VARIANTS_MAX_LEN, [&](u32 i) { return consensus_key_letter(letters, i); });
}
// the SNV: col_op the op of the word that holds the column, letter() the oriented letter of an X column
template <class Letter>
FLX_HD inline u32 phase_observe_snv(u32 col_op, u32 alt_rank, Letter&& letter) {
    if (col_op == 7u) return PHASE_REF;
    if (col_op == 8u) return (u32)letter() == alt_rank ? PHASE_ALT : PHASE_NONE;
    return PHASE_NONE;
}
// Whether an I or D word has the key `key`. anchor: the column in front of the word; letter(i): its letters in the oriented sequence.
// The word's key is variants_key's; the letters are packed only when the anchor, the kind and the length already agree.
template <class Letter>
FLX_HD inline bool phase_word_has_key(SortKey const& key, u32 op, u64 anchor, u32 len, Letter&& letter) {
    u32 const kind = op == 1u ? VARIANTS_KEY_INS : VARIANTS_KEY_DEL;
    if (key.hi != (anchor << 32 | (u64)kind << 28 | (u64)len)) return false;       // (a word's length has 28 bits)
    return consensus_key_equal(key, variants_key(kind, true, anchor, len, VARIANTS_MAX_LEN, letter));
}
// The indel: the column at the anchor a is column `a` of word t (op col_op, the last of its word iff last_col); row_behind is the row
// behind that word; word(u) is word u < n_words of the record, letter(r) row r of the oriented sequence.
template <class Word, class Letter>
FLX_HD inline u32 phase_observe_indel(SortKey const& key, u32 col_op, bool last_col, u64 a, u64 text_end, u32 t, u32 n_words, u64 row_behind, Word&& word, Letter&& letter) {
    bool empty = true;
    if (last_col) {
        u64 p = a + 1, row = row_behind;                               // the cursor behind the column and the row behind its word
        for (u32 u = t + 1u; u < n_words; ++u) {
            u32 const w = word(u), op = w & 15u, len = w >> 4;
            if (op != 1u && op != 2u) break;
            empty = false;
            if (phase_word_has_key(key, op, p - 1, len, [&](u32 i) { return (u32)letter(row + i); })) return PHASE_ALT;
            if (op == 1u) row += len; else p += len;
        }
    }
    return empty && (col_op == 7u || col_op == 8u) && a + 1 < text_end ? PHASE_REF : PHASE_NONE;
}
// every slot of one word's columns [col0, col0 + cols) (op 7, 8 or 2; row0 the word's first row): site(k), anchor(k) for slot k < n_slots,
// store(k, observation). The kernel's lane and the host walk both run this.
template <class Anchor, class Site, class Word, class Letter, class Store>
FLX_HD inline void phase_observe_word(u32 n_slots, u32 op, u32 len, u64 col0, u64 row0, u64 text_end, u32 t, u32 n_words, Anchor&& anchor, Site&& site, Word&& word, Letter&& letter,
                                      Store&& store) {
    u32 lo = 0, hi = n_slots;                                          // the first slot whose anchor is not below col0
    while (lo < hi) {
        u32 const mid = lo + (hi - lo) / 2u;
        if ((u64)anchor(mid) < col0) lo = mid + 1u; else hi = mid;
    }
    u64 const row_behind = row0 + (op == 2u ? 0u : len);
    for (u32 k = lo; k < n_slots; ++k) {
        u64 const a = anchor(k);
        if (a >= col0 + len) break;
        flx_phase_site const s = site(k);
        u32 o;
        if (s.kind == VARIANT_SNV) o = phase_observe_snv(op, s.alt_rank, [&]() { return (u32)letter(row0 + (a - col0)); });
        else o = phase_observe_indel(phase_site_key(s.kind, a, s.length, s.letters), op, a + 1 == col0 + len, a, text_end, t, n_words, row_behind, word, letter);
        store(k, o);
    }
}

// ---- links and the chain
FLX_HD inline bool phase_connected(u32 cis, u32 trans, bool same_sequence, u32 min_link) {
    return same_sequence && (cis > trans ? cis - trans : trans - cis) >= min_link;
}
FLX_HD inline bool phase_flip(u32 cis, u32 trans) { return trans > cis; }

// ---- the tag of one record: obs(k), state(k) (PHASE_BIT_*) and set(k) of slot k
template <class Obs, class State, class Set>
FLX_HD inline void phase_tag_record(u32 n_slots, u32 min_margin, Obs&& obs, State&& state, Set&& set, u32& hap, u32& phase_set, u32& h1, u32& h2) {
    u32 best_set = PHASE_NO_SET, best_n = 0, best_h1 = 0, best_h2 = 0;
    u32 cur = PHASE_NO_SET, n = 0, c1 = 0, c2 = 0;
    for (u32 k = 0; k <= n_slots; ++k) {
        u32 st = 0, sid = PHASE_NO_SET;
        if (k < n_slots) {
            st = state(k);
            if (!(st & PHASE_BIT_PHASED)) continue;                    // unphased sites are skipped
            sid = set(k);
        }
        if (sid != cur) {                                              // a run ends (set ids rise along the record)
            if (n > best_n) { best_set = cur; best_n = n; best_h1 = c1; best_h2 = c2; }
            cur = sid; n = 0; c1 = 0; c2 = 0;
        }
        if (k == n_slots) break;
        u32 const o = obs(k);
        if (o > PHASE_ALT) continue;
        ++n;
        if ((o ^ (st & PHASE_BIT_P)) == 1u) ++c1; else ++c2;
    }
    phase_set = best_set; h1 = best_h1; h2 = best_h2;
    hap = best_h1 >= best_h2 && best_h1 - best_h2 >= min_margin && best_n ? 1u : best_h2 >= best_h1 && best_h2 - best_h1 >= min_margin && best_n ? 2u : 0u;
}
// the vote of a tagged record (hap 1 or 2, its run's set) at one slot: 0 none, 1 keep, 2 swap
FLX_HD inline u32 phase_vote(u32 hap, u32 run_set, u32 obs, u32 state, u32 set) {
    if (hap == 0u || obs > PHASE_ALT || !(state & PHASE_BIT_PHASED) || set != run_set) return 0u;
    return (obs ^ (state & PHASE_BIT_P)) == (hap == 1u ? 1u : 0u) ? 1u : 2u;
}
FLX_HD inline flx_phase_result phase_result_row(u32 set, u32 state, u32 cis, u32 trans, u32 keep, u32 swap) {
    flx_phase_result r;
    r.phase_set = set; r.phased = state & PHASE_BIT_PHASED ? 1u : 0u; r.phase = state & PHASE_BIT_P;
    r.cis = cis; r.trans = trans; r.keep = keep; r.swap = swap; r.reserved = 0;
    return r;
}

// one counted record as the object keeps it: where its observations lie, where its span ends, its slots, its add and its read
struct PhaseRecord { u64 obs_off; u64 text_end; u32 first, n_slots, add, read; };
static_assert(sizeof(PhaseRecord) == 32, "PhaseRecord is 32 bytes");

// ---- the host forms
// the observations of one judged job into obs[rec.obs_off ...] (the host form of phase_observe)
inline void phase_job_observe(PileupJob const& j, PhaseRecord const& rec, const uint32_t* cigar_words, const uint8_t* read, u64 read_len, const u32* anchors,
                              const flx_phase_site* sites, u8* obs) {
    u64 p = j.text_off, row = 0;
    for (u32 t = 0; t < j.n_words; ++t) {
        uint32_t const w = cigar_words[j.word_off + t], op = w & 15u, len = w >> 4;
        if (coverage_op_consumes(op))
            phase_observe_word(rec.n_slots, op, len, p, row, rec.text_end, t, j.n_words, [&](u32 k) { return anchors[rec.first + k]; }, [&](u32 k) { return sites[rec.first + k]; },
                               [&](u32 u) { return cigar_words[j.word_off + u]; }, [&](u64 r) { return pileup_oriented_rank(read, read_len, j.reverse != 0, r); },
                               [&](u32 k, u32 o) { obs[rec.obs_off + k] = (u8)o; });
        if (coverage_op_consumes(op)) p += len;
        if (pileup_op_consumes_query(op)) row += len;
    }
}
// links, chain, tags and refinement over the records' observations; results: n_sites rows, tags: one per record
inline void phase_finish_host(const flx_phase_site* sites, u64 n_sites, std::vector<PhaseRecord> const& recs, const u8* obs, PhaseModel const& m, flx_phase_result* results,
                              flx_phase_tag* tags) {
    std::vector<u32> cis(n_sites, 0), trans(n_sites, 0), keep(n_sites, 0), swap(n_sites, 0), set(n_sites, 0), state(n_sites, 0);
    for (auto const& r : recs)
        for (u32 k = 0; k + 1 < r.n_slots; ++k) {
            u32 const a = obs[r.obs_off + k], b = obs[r.obs_off + k + 1];
            if (a > PHASE_ALT || b > PHASE_ALT) continue;
            ++(a == b ? cis : trans)[r.first + k];
        }
    for (u64 i = 0; i < n_sites; ++i) {
        bool const joined = i > 0 && phase_connected(cis[i - 1], trans[i - 1], sites[i - 1].reference_id == sites[i].reference_id, m.min_link);
        set[i] = joined ? set[i - 1] : (u32)i;
        if (joined) {
            state[i] = PHASE_BIT_PHASED | ((state[i - 1] & PHASE_BIT_P) ^ (phase_flip(cis[i - 1], trans[i - 1]) ? 1u : 0u));
            state[i - 1] |= PHASE_BIT_PHASED;
        }
    }
    auto tag_all = [&]() {
        for (size_t j = 0; j < recs.size(); ++j) {
            PhaseRecord const& r = recs[j];
            flx_phase_tag& t = tags[j];
            t.add = r.add; t.read = r.read; t.n_slots = r.n_slots; t.reserved = 0;
            phase_tag_record(r.n_slots, m.min_margin, [&](u32 k) { return (u32)obs[r.obs_off + k]; }, [&](u32 k) { return state[r.first + k]; }, [&](u32 k) { return set[r.first + k]; },
                             t.hap, t.phase_set, t.h1, t.h2);
        }
    };
    tag_all();
    for (u32 round = 0; round < m.rounds; ++round) {
        std::fill(keep.begin(), keep.end(), 0u);
        std::fill(swap.begin(), swap.end(), 0u);
        for (size_t j = 0; j < recs.size(); ++j)
            for (u32 k = 0; k < recs[j].n_slots; ++k) {
                u32 const s = recs[j].first + k, v = phase_vote(tags[j].hap, tags[j].phase_set, obs[recs[j].obs_off + k], state[s], set[s]);
                if (v == 1u) ++keep[s]; else if (v == 2u) ++swap[s];
            }
        for (u64 i = 0; i < n_sites; ++i) if (swap[i] > keep[i]) state[i] ^= PHASE_BIT_P;
        tag_all();
    }
    for (u64 i = 0; i < n_sites; ++i) results[i] = phase_result_row(set[i], state[i], cis[i], trans[i], keep[i], swap[i]);
}

// ---- the launches of flx_phase.hip (each returns the hipError_t of its launch; pointers are device pointers)
struct PhaseDevice {
    static constexpr u32 OBSERVE_GRID_CAP = 2048;      // most blocks (four waves, a record each at a time) of a phase_observe launch
    static constexpr u32 OBSERVE_WAVES = 4;
    // d_obs[rec.obs_off + k] for every slot of every record of this add (d_recs and d_jobs: the add's own, record for record)
    static int observe(void* stream, const PileupJob* d_jobs, const PhaseRecord* d_recs, u32 n_jobs, const u32* d_words, const u8* d_letters, const u32* d_anchors,
                       const flx_phase_site* d_sites, u8* d_obs);
    // slots [slot0, slot0 + n_slots) of the records d_recs[0, n_recs) (the first of them holds slot0): cis and trans
    static int links(void* stream, const PhaseRecord* d_recs, u32 n_recs, u64 slot0, u64 n_slots, const u8* d_obs, u32* d_cis, u32* d_trans);
    // step 0: d_flips[i], d_starts[i] from the links; step 1 (both scanned): the set starts scattered into d_set_start (n_sites + 1
    // entries); step 2: d_set[i], d_state[i]
    static int chain(void* stream, int step, const flx_phase_site* d_sites, u32 n_sites, const u32* d_cis, const u32* d_trans, u32 min_link, u32* d_flips, u32* d_starts,
                     u32* d_set_start, u32* d_set, u32* d_state);
    static int tags(void* stream, const PhaseRecord* d_recs, u64 n_recs, const u8* d_obs, const u32* d_set, const u32* d_state, u32 min_margin, flx_phase_tag* d_tags);
    static int votes(void* stream, const PhaseRecord* d_recs, u64 n_recs, u64 n_slots, const u8* d_obs, const u32* d_set, const u32* d_state, const flx_phase_tag* d_tags, u32* d_keep,
                     u32* d_swap);
    static int revote(void* stream, u32 n_sites, const u32* d_keep, const u32* d_swap, u32* d_state);
    static int results(void* stream, u32 n_sites, const u32* d_set, const u32* d_state, const u32* d_cis, const u32* d_trans, const u32* d_keep, const u32* d_swap,
                       flx_phase_result* d_out);
};

}  // namespace flx
