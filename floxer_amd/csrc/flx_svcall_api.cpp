// flx_svcall: the structural-variant calling rule behind the C ABI (include/floxer_amd.h). The rule and its checks: flx_svcall.hpp.
// The one-call host form: flx_svcall_host takes all records of a run and the clusters of an flx_sv object (flx_sv_copy_clusters) and
// returns one row per DEL / INS cluster. No device is touched. The object that is fed batch by batch, on a device or on the host:
// flx_svcaller_api.cpp.
#include <cstring>

#include "flx_svcall.hpp"

using namespace flx;

extern "C" int flx_svcall_host(const uint64_t* ref_lens, uint32_t n_refs, const flx_svcall_options* o, const flx_record* records, uint64_t n, const uint32_t* cigar_words,
                               uint64_t n_words, const flx_sv_cluster* clusters, uint64_t n_clusters, flx_svcall_row* rows, uint64_t* n_rows) {
    std::vector<u64> starts;
    if (!svcall_options_valid(o) || !sv_lengths_valid(ref_lens, n_refs, "flx_svcall_host", starts)) return FLX_ERR_INVALID;
    if (!n_rows || (n && !records) || (n_clusters && !clusters)) { set_error("flx_svcall_host: null argument"); return FLX_ERR_INVALID; }
    flx_svcall_options const opt = svcall_options_or_default(o);
    std::vector<SvcallJob> jobs;
    if (!svcall_plan(starts, opt, records, n, cigar_words, n_words, "flx_svcall_host", jobs)) return FLX_ERR_INVALID;
    u64 need = 0;
    if (!svcall_clusters_valid(starts, clusters, n_clusters, "flx_svcall_host", need)) return FLX_ERR_INVALID;
    u64 const capacity = *n_rows;
    *n_rows = need;
    if (need > capacity || (need && !rows)) { set_error("flx_svcall_host: the row buffer is too small, " + std::to_string(need) + " rows"); return FLX_ERR_CAPACITY; }
    std::vector<SortKey> spans;
    spans.reserve(jobs.size());
    for (auto const& j : jobs) spans.push_back(svcall_job_key(j));
    std::vector<flx_svcall_row> made;
    svcall_finish_host(starts, spans, clusters, n_clusters, svcall_model(opt), made);
    if (!made.empty()) memcpy(rows, made.data(), made.size() * sizeof(flx_svcall_row));
    return FLX_OK;
}
