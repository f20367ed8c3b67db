// The svcaller object (flx_svcaller, include/floxer_amd.h) without HIP: what its device path and its host form share, and the host
// form itself. The limits, the equality of two objects' options, the judgements of the two copy calls with their messages, a span as
// the copy calls give it, the host table (adds, absorb, finish, copies) and the launches of flx_svcall.hip as declarations. The rule:
// flx_svcall.hpp; the object and the C ABI: flx_svcaller_api.cpp. A host compiler takes this file alone (tests/svcaller_check.cpp).
//
// The copy contract: flx_svcaller_copy_rows writes exactly num_rows rows or nothing; a capacity below num_rows is FLX_ERR_CAPACITY.
// Both paths ask rows_copy_judged / spans_copy_judged first and move bytes only behind FLX_OK with `n` above 0, so no caller's buffer
// is written past the capacity it stated.
#pragma once
#include <cstring>

#include "flx_svcall.hpp"

namespace flx {

constexpr u64 SVCALL_MAX_SPANS = (1ull << 32) - 1;     // the sorter's payload is u32
constexpr u64 SVCALLER_DEFAULT_INITIAL_CAPACITY = 1ull << 16;

// two objects may be absorbed into one another when they count the same records and call with the same model
inline bool svcall_options_equal(flx_svcall_options const& a, flx_svcall_options const& b) {
    SvcallModel const x = svcall_model(a), y = svcall_model(b);
    return a.count_secondary == b.count_secondary && a.min_mapq == b.min_mapq && x.flank == y.flank && x.v.min_depth == y.v.min_depth && x.v.min_qual == y.v.min_qual &&
           x.v.m == y.v.m && x.v.x == y.v.x && x.v.h == y.v.h && x.v.prior_het == y.v.prior_het && x.v.prior_hom == y.v.prior_hom;
}

inline flx_svcall_span svcall_span_of(SortKey const& k) { return flx_svcall_span{(int32_t)svcall_span_ref(k), svcall_span_rs(k), svcall_span_re(k), 0u}; }

// ---- the judgements of the copy calls (behind finished_for_copy). FLX_OK with n == 0: nothing to move.
inline int rows_copy_judged(u64 n_rows, const void* out, u64 capacity, u64& n) {
    n = 0;
    if (capacity < n_rows) { set_error("flx_svcaller_copy_rows: the row buffer is too small, " + std::to_string(n_rows) + " rows"); return FLX_ERR_CAPACITY; }
    if (n_rows == 0) return FLX_OK;
    if (!out) { set_error("flx_svcaller_copy_rows: null argument"); return FLX_ERR_INVALID; }
    n = n_rows;
    return FLX_OK;
}
inline int spans_copy_judged(u64 n_spans, u64 from, u64 to, const void* out, u64& n) {
    n = 0;
    if (from > to || to > n_spans) { set_error("flx_svcaller_copy_spans: a stretch outside the spans"); return FLX_ERR_INVALID; }
    if (from == to) return FLX_OK;
    if (!out) { set_error("flx_svcaller_copy_spans: null argument"); return FLX_ERR_INVALID; }
    n = to - from;
    return FLX_OK;
}
// an add of n keys to a table of `count`
inline int spans_room_judged(u64 count, u64 n, const char* who) {
    if (n > SVCALL_MAX_SPANS - count) { set_error(std::string(who) + ": more than 2^32 - 1 spans in one svcaller object"); return FLX_ERR_CAPACITY; }
    return FLX_OK;
}
// the DEL / INS clusters' indices in input order: row w belongs to cluster index[w]
inline int svcall_row_index(const flx_sv_cluster* clusters, uint64_t n, const char* who, std::vector<u32>& index) {
    if (n > 0xFFFFFFFFull) { set_error(std::string(who) + ": more than 2^32 - 1 clusters"); return FLX_ERR_CAPACITY; }
    index.clear();
    for (uint64_t i = 0; i < n; ++i) if (clusters[i].type != SV_BND) index.push_back((u32)i);
    return FLX_OK;
}

// ---- the host form's table: the keys in adding order, then, behind finish, in key order with the rows. The object's lock is the caller's.
struct SvcallHostTable {
    std::vector<SortKey> keys;
    u32 max_span = 0;
    std::vector<flx_svcall_row> rows;                  // behind finish

    int add(std::vector<SvcallJob> const& jobs, const char* who) {
        int const rc = spans_room_judged(keys.size(), jobs.size(), who);
        if (rc) return rc;
        keys.reserve(keys.size() + jobs.size());
        for (auto const& j : jobs) { keys.push_back(svcall_job_key(j)); max_span = std::max(max_span, j.re - j.rs); }
        return FLX_OK;
    }
    // `from` is left empty with max_span 0
    int absorb(SvcallHostTable& from, const char* who) {
        int const rc = spans_room_judged(keys.size(), from.keys.size(), who);
        if (rc) return rc;
        keys.insert(keys.end(), from.keys.begin(), from.keys.end());
        max_span = std::max(max_span, from.max_span);
        from.keys.clear();
        from.max_span = 0;
        return FLX_OK;
    }
    // the clusters are judged by the caller (svcall_clusters_valid)
    void finish(std::vector<u64> const& starts, const flx_sv_cluster* clusters, uint64_t n, SvcallModel const& m) {
        rows.clear();
        svcall_finish_host(starts, keys, clusters, n, m, rows);
    }
    int copy_spans(u64 from, u64 to, flx_svcall_span* out) const {
        u64 n;
        int const rc = spans_copy_judged(keys.size(), from, to, out, n);
        if (rc) return rc;
        for (u64 i = 0; i < n; ++i) out[i] = svcall_span_of(keys[from + i]);
        return FLX_OK;
    }
    int copy_rows(flx_svcall_row* out, u64 capacity) const {
        u64 n;
        int const rc = rows_copy_judged(rows.size(), out, capacity, n);
        if (rc) return rc;
        if (n) memcpy(out, rows.data(), n * sizeof(flx_svcall_row));
        return FLX_OK;
    }
};

// ---- the launches of flx_svcall.hip (each returns the hipError_t of its launch; pointers are device pointers)
struct SvcallDevice {
    static constexpr u32 THREADS = 256, WAVES = THREADS / 64u;
    static constexpr u32 SPANS_GRID_CAP = 1u << 11;    // most blocks (four waves, a job each at a time) of an svcall_spans launch
    static constexpr u32 COUNT_GRID_CAP = 1u << 10;    // most blocks (four waves, a row each at a time) of an svcall_count launch
    // one wave per job: its span's key at d_keys[job]; d_state[0] (the object's max_span) raised to the job's span; d_state[1] (the add's
    // flag) set when a job's words do not end where the host planned
    static int spans(void* stream, const SvcallJob* d_jobs, u32 n_jobs, const u32* d_words, SortKey* d_keys, u32* d_state);
    // one wave per row: row w is the row of cluster d_index[w] over the n_spans sorted keys
    static int count(void* stream, const SortKey* d_sorted, u64 n_spans, u32 max_span, const flx_sv_cluster* d_clusters, const u32* d_index, u32 n_rows, const u32* d_lens,
                     SvcallModel model, flx_svcall_row* d_rows);
};

}  // namespace flx
