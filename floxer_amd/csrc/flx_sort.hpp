// Coordinate order of records (flx_sort, include/floxer_amd.h): the rule, in one place, for the host and the device. The kernels
// (flx_sort.hip) pack keys with the same functions; the object and the C ABI: flx_sort_api.cpp.
//
// A record's key is two u64, compared ascending as (hi, lo):
//   hi = ref << 32 | (u32)position      ref = 0xFFFFFFFF for a record with flag & 4 or reference_id < 0 (unplaced), else reference_id
//   lo = strand << 63 | ordinal         strand = (flag >> 4) & 1; the ordinal is the caller's and below 2^63
// That is samtools sort's order (reference, position, forward before reverse, unplaced records last) with ties broken by the ordinal: the
// order is total and depends on nothing but the records and their ordinals.
// A record's end: position + max(1, span) for a mapped record, span the summed lengths of its = X D words (0 for a record without
// words); position + 1 for an unplaced one. The BAM bin (reg2bin over [position, end)) and the BAI builder share it.
//   refused               a mapped record with a reference_id outside the list or a negative position, an op other than = X I D S, a
//                         zero-length word, words outside the pool, an end above 2^31 - 1, an ordinal of 2^63 or more
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FLX_SORT_HD __host__ __device__ inline
#else
#define FLX_SORT_HD inline
#endif

#include "../../include/floxer_amd.h"

namespace flx {

struct SortKey { uint64_t hi, lo; };                   // 16 bytes, as the device table holds them
struct SortMeta { uint32_t end, flag; };               // what an entry carries besides its key

constexpr uint32_t SORT_UNPLACED = 0xFFFFFFFFu;
constexpr uint64_t SORT_MAX_ORDINAL = 1ull << 63;      // ordinals lie below
constexpr uint64_t SORT_MAX_END = (1ull << 31) - 1;    // a mapped record's end lies at or below
constexpr uint64_t SORT_MAX_RECORDS = (1ull << 32) - 1;
constexpr uint32_t SORT_DIGIT_BITS = 8, SORT_DIGITS = 16, SORT_RADIX = 256;

FLX_SORT_HD bool sort_unplaced(uint32_t flag, int32_t reference_id) { return (flag & 4u) != 0u || reference_id < 0; }
FLX_SORT_HD SortKey sort_key(uint32_t flag, int32_t reference_id, int32_t position, uint64_t ordinal) {
    uint64_t const ref = sort_unplaced(flag, reference_id) ? (uint64_t)SORT_UNPLACED : (uint64_t)(uint32_t)reference_id;
    return SortKey{ref << 32 | (uint64_t)(uint32_t)position, (uint64_t)((flag >> 4) & 1u) << 63 | ordinal};
}
FLX_SORT_HD bool sort_key_less(SortKey const& a, SortKey const& b) { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; }
// digit d of a key, least significant first: 0..7 from lo, 8..15 from hi
FLX_SORT_HD uint32_t sort_digit(SortKey const& k, uint32_t d) { return (uint32_t)((d < 8u ? k.lo >> (8u * d) : k.hi >> (8u * (d - 8u))) & 255u); }
FLX_SORT_HD bool sort_op_known(uint32_t op) { return op == 7u || op == 8u || op == 1u || op == 2u || op == 4u; }
FLX_SORT_HD bool sort_op_consumes(uint32_t op) { return op == 7u || op == 8u || op == 2u; }
// span: the reference columns of a mapped record's words (0 without words); ignored for an unplaced record
FLX_SORT_HD uint64_t sort_end(bool unplaced, int32_t position, uint64_t span) {
    return unplaced ? (uint64_t)(uint32_t)position + 1u : (uint64_t)position + (span > 1u ? span : 1u);
}
// what a sorted entry says of its record, read back from the key (an unplaced record's reference_id reads -1)
FLX_SORT_HD uint64_t sort_key_ordinal(SortKey const& k) { return k.lo & (SORT_MAX_ORDINAL - 1u); }
FLX_SORT_HD int32_t sort_key_reference(SortKey const& k) { return (uint32_t)(k.hi >> 32) == SORT_UNPLACED ? -1 : (int32_t)(uint32_t)(k.hi >> 32); }
FLX_SORT_HD int32_t sort_key_position(SortKey const& k) { return (int32_t)(uint32_t)k.hi; }

// SAMv1 5.3: the smallest bin that holds [beg, end)
FLX_SORT_HD uint32_t reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// The keys one block orders per pass. The digit table of a pass has 256 entries per tile and is scanned in two levels of scan_tile
// entries: beyond scan_tile^2 / 256 tiles the tiles grow instead (in whole blocks of block_keys), so that the scan never needs a third.
inline uint64_t sort_effective_tile(uint64_t n, uint64_t tile_keys, uint64_t block_keys, uint64_t scan_tile) {
    uint64_t const max_tiles = scan_tile * scan_tile / SORT_RADIX;
    uint64_t const need = (n + max_tiles - 1) / max_tiles;
    uint64_t const grown = (need + block_keys - 1) / block_keys * block_keys;
    return grown > tile_keys ? grown : tile_keys;
}

// Judges n records against their word pool and appends their keys and {end, flag}; record i has ordinal ordinals ? ordinals[i] :
// first_ordinal + i. false: refused, *error says why, and the vectors are as they were. Templated on the record type so that the
// stand-alone check can use a record of its own; the library passes flx_record.
template <class Record>
inline bool sort_plan(uint32_t n_refs, const Record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words, uint64_t first_ordinal,
                      const uint64_t* ordinals, const char* who, std::vector<SortKey>& keys, std::vector<SortMeta>& meta, std::string* error) {
    size_t const keys_before = keys.size(), meta_before = meta.size();
    auto refuse = [&](uint64_t i, const char* what) {
        keys.resize(keys_before);
        meta.resize(meta_before);
        if (error) *error = std::string(who) + ": record " + std::to_string(i) + " " + what;
        return false;
    };
    if (!ordinals && (first_ordinal >= SORT_MAX_ORDINAL || n > SORT_MAX_ORDINAL - first_ordinal)) {
        if (error) *error = std::string(who) + ": an ordinal of 2^63 or more";
        return false;
    }
    bool have_span = false;
    uint64_t span = 0, span_offset = 0;
    uint32_t span_length = 0;
    keys.reserve(keys_before + n);
    meta.reserve(meta_before + n);
    for (uint64_t i = 0; i < n; ++i) {
        Record const& r = records[i];
        uint64_t const ordinal = ordinals ? ordinals[i] : first_ordinal + i;
        if (ordinal >= SORT_MAX_ORDINAL) return refuse(i, "has an ordinal of 2^63 or more");
        bool const unplaced = sort_unplaced(r.flag, r.reference_id);
        if (!unplaced && (uint32_t)r.reference_id >= n_refs) return refuse(i, "names a reference_id outside the list");
        if (!unplaced && r.position < 0) return refuse(i, "has a negative position");
        if (r.cigar_length != 0 && (!cigar_words || r.cigar_offset > n_words || r.cigar_length > n_words - r.cigar_offset)) return refuse(i, "has CIGAR words outside the pool");
        // (the records of one traced path share one word array: judged and summed once)
        if (!have_span || r.cigar_offset != span_offset || r.cigar_length != span_length) {
            span = 0;
            for (uint32_t t = 0; t < r.cigar_length; ++t) {
                uint32_t const w = cigar_words[r.cigar_offset + t], op = w & 15u;
                if (!sort_op_known(op)) return refuse(i, "has a CIGAR op other than = X I D S");
                if ((w >> 4) == 0) return refuse(i, "has a CIGAR word of length 0");
                if (sort_op_consumes(op)) span += w >> 4;
            }
            have_span = true; span_offset = r.cigar_offset; span_length = r.cigar_length;
        }
        uint64_t const end = sort_end(unplaced, r.position, span);
        if (!unplaced && end > SORT_MAX_END) return refuse(i, "ends above 2^31 - 1");
        keys.push_back(sort_key(r.flag, r.reference_id, r.position, ordinal));
        meta.push_back(SortMeta{(uint32_t)end, r.flag});
    }
    return true;
}

// ---- the launches of flx_sort.hip (each returns the hipError_t of its launch; pointers are device pointers)
struct SortDevice {
    static constexpr uint32_t THREADS = 256;           // a block, and the keys it takes per step of its tile
    static constexpr uint32_t TILE_KEYS = 2048;        // default keys per tile
    static constexpr uint32_t KEYS_GRID_CAP = 1u << 16;      // most blocks (four waves, a record each at a time) of a sort_keys_add launch
    static constexpr uint32_t CENSUS_GRID_CAP = 1024u;       // most blocks of a sort_census launch: a block gathers its counts over all its turns
    static constexpr uint32_t STRIDED_GRID_CAP = 1u << 14;   // most blocks of sort_iota and sort_entries: a thread strides on by the grid
    // one wave per record: keys[i], meta[i] and payload[i] = payload_base + i from records[i] (a flx_record array) and its words
    static int keys_add(void* stream, const flx_record* d_records, uint32_t n, const uint32_t* d_words, uint64_t first_ordinal, SortKey* d_keys,
                        SortMeta* d_meta);
    static int iota(void* stream, uint32_t* d_payload, uint64_t n);
    // counts[d * 256 + v]: the keys whose digit d is v (cleared by the caller)
    static int digit_census(void* stream, const SortKey* d_keys, uint64_t n, uint32_t* d_counts);
    // table[v * n_tiles + t]: the keys of tile t whose digit is v
    static int histogram(void* stream, const SortKey* d_keys, uint64_t n, uint32_t digit, uint32_t tile_keys, uint32_t* d_table);
    // table inclusively scanned; stable within and across tiles
    static int scatter(void* stream, const SortKey* d_keys, const uint32_t* d_payload, uint64_t n, uint32_t digit, uint32_t tile_keys, const uint32_t* d_table,
                       SortKey* d_keys_out, uint32_t* d_payload_out);
    // entries[i] (flx_sort_entry) from keys[i] and meta[payload[i]]
    static int entries(void* stream, const SortKey* d_keys, const uint32_t* d_payload, const SortMeta* d_meta, uint64_t n, void* d_entries);
};

// The sorted writer (flx_io.cpp) reaches the sort object through this table, which flx_sort_api.cpp fills in when the library is
// loaded: flx_io.cpp stays buildable on its own, as the host-only checks build it, and a build without the sort refuses sorted mode.
struct SortCalls {
    int (*create)(int, uint32_t, const flx_sort_options*, flx_sort**);
    void (*free)(flx_sort*);
    int (*add_records)(flx_sort*, const flx_record*, uint64_t, const uint32_t*, uint64_t, uint64_t, uint32_t*);
    int (*finish)(flx_sort*);
    uint64_t (*num_records)(const flx_sort*);
    int (*copy)(const flx_sort*, uint64_t, uint64_t, flx_sort_entry*);
};
extern const SortCalls* g_sort_calls;

}  // namespace flx
