// flx_sv: the object behind the structural-variant signature calls of the C ABI (include/floxer_amd.h). The rule and its checks:
// flx_sv.hpp; the kernels: flx_sv.hip; the sort's driver: flx_sort_driver.hpp; the scan: flx_scan.hip; what it shares with the other side
// objects: flx_object.hpp. The object owns one stream, the key table (one SortKey per signature, in adding order), the staging buffers
// of an add and, behind flx_sv_finish, the signatures in key order and the clusters. Adds judge their records and stage their words
// without the object's lock and take it for the upload and the launches only, so several host threads may add at once.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>

#include "flx_object.hpp"
#include "flx_sort_driver.hpp"
#include "flx_sv.hpp"

using namespace flx;

namespace {
constexpr u64 DEFAULT_INITIAL_CAPACITY = 1ull << 16;
constexpr u64 ABSORB_CHUNK = 1ull << 20;               // keys per piece of an absorb (16 MB)
}  // namespace

struct flx_sv : SideObject {             // mu: the table, staging, launches and `finished`; FLX_SV_PROFILE
    flx_sv_options opt{};
    std::vector<u64> starts;             // n_refs + 1, as coverage judges records against them
    u64 initial_capacity = DEFAULT_INITIAL_CAPACITY;
    bool finished = false;
    u64 count = 0, capacity = 0;         // signatures added; signatures the table holds
    DeviceBuffer keys;                   // the table
    DeviceBuffer jobs, members, words, segments, flag;      // an add's staging
    RadixSorter sorter;                  // finish: the two sorts
    ScanDriver scan;                     // finish: group ids, cluster ids, the compaction
    DeviceBuffer ids, cluster_starts, all_clusters, tile_counts;
    DeviceBuffer signatures, clusters;   // behind finish
    u64 n_clusters = 0;
    PinnedBuffer pinned;                 // absorb: a piece of the other object's keys on its way through the host
};

namespace {

int create(int device, std::vector<u64>&& starts, const flx_sv_options* o, flx_sv** out) {
    auto s = std::make_unique<flx_sv>();                // (an error below drops it: nothing stays allocated)
    s->opt = sv_options_or_default(o);
    if (s->opt.initial_capacity) s->initial_capacity = s->opt.initial_capacity;
    s->starts = std::move(starts);
    FLX_HIP(hipSetDevice(device));                      // (a device below 0 is refused here: the object has no host form)
    int const rc = s->open(device, "FLX_SV_PROFILE");
    if (rc) return rc;
    *out = s.release();
    return FLX_OK;
}

// the table holds at least `need` keys afterwards, its first `count` as before; a failure leaves it as it was
int grow(flx_sv* s, u64 need) {
    if (need <= s->capacity) return FLX_OK;
    u64 const cap = std::min<u64>(std::max<u64>({need, s->capacity * 2, s->initial_capacity}), SV_MAX_SIGNATURES);
    DeviceBuffer keys;
    int rc;
    if ((rc = keys.ensure(cap * sizeof(SortKey), true))) return rc;
    if (s->count) {
        FLX_HIP(hipMemcpyAsync(keys.ptr, s->keys.ptr, s->count * sizeof(SortKey), hipMemcpyDeviceToDevice, s->stream));
        FLX_HIP(hipStreamSynchronize(s->stream));
    }
    s->keys.take(keys);
    s->capacity = cap;
    return FLX_OK;
}

// the judged plan of one word pool: its words staged, then uploaded and launched under the object's lock
int commit(flx_sv* s, SvPlan& plan, const uint32_t* cigar_words, const char* who) {
    auto const t0 = std::chrono::steady_clock::now();
    std::vector<u32> pool;
    if (!plan.jobs.empty()) compact_words(plan.jobs, cigar_words, pool);
    std::lock_guard<std::mutex> g(s->mu);
    if (s->finished) { set_error(std::string(who) + ": the sv object is finished"); return FLX_ERR_INVALID; }
    if (plan.jobs.empty()) return FLX_OK;
    u64 const n_keys = plan.n_keys();
    if (n_keys > SV_MAX_SIGNATURES - s->count) { set_error(std::string(who) + ": more than 2^32 - 1 signatures in one sv object"); return FLX_ERR_CAPACITY; }
    FLX_HIP(hipSetDevice(s->device));
    int rc;
    if ((rc = grow(s, s->count + n_keys))) return rc;
    if ((rc = s->jobs.ensure(plan.jobs.size() * sizeof(SvJob))) || (rc = s->members.ensure(std::max<size_t>(plan.members.size(), 1) * sizeof(SvMember))) ||
        (rc = s->words.ensure(pool.size() * 4)) || (rc = s->segments.ensure(plan.jobs.size() * sizeof(SvSegment))) || (rc = s->flag.ensure(4)))
        return rc;
    FLX_HIP(hipMemcpyAsync(s->jobs.ptr, plan.jobs.data(), plan.jobs.size() * sizeof(SvJob), hipMemcpyHostToDevice, s->stream));
    if (!plan.members.empty()) FLX_HIP(hipMemcpyAsync(s->members.ptr, plan.members.data(), plan.members.size() * sizeof(SvMember), hipMemcpyHostToDevice, s->stream));
    FLX_HIP(hipMemcpyAsync(s->words.ptr, pool.data(), pool.size() * 4, hipMemcpyHostToDevice, s->stream));
    FLX_HIP(hipMemsetAsync(s->flag.ptr, 0, 4, s->stream));
    if ((rc = s->span_begin())) return rc;
    SortKey* const base = s->keys.as<SortKey>() + s->count;             // (room for n_keys behind it: grow saw to it)
    FLX_LAUNCH("sv_extract", SvDevice::extract(s->stream, s->jobs.as<SvJob>(), (u32)plan.jobs.size(), s->words.as<u32>(), sv_thresholds(s->opt).min_length, base,
                                               s->segments.as<SvSegment>(), s->flag.as<u32>()));
    if (plan.n_junctions)
        FLX_LAUNCH("sv_junctions", SvDevice::junctions(s->stream, s->members.as<SvMember>(), (u32)plan.members.size(), s->segments.as<SvSegment>(), base, s->flag.as<u32>()));
    if ((rc = s->span_end())) return rc;
    u32 flag = 0;
    FLX_HIP(hipMemcpyAsync(&flag, s->flag.ptr, 4, hipMemcpyDeviceToHost, s->stream));
    FLX_HIP(hipStreamSynchronize(s->stream));           // (the staging buffers are free for the next add)
    if (flag) { set_error(std::string(who) + ": a kernel found a record at odds with the host's judgement (flag " + std::to_string(flag) + ")"); return FLX_ERR_INTERNAL; }
    s->count += n_keys;
    if (s->profile) {
        float ms;
        if ((rc = s->span_ms(ms))) return rc;
        double const wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        u64 passes = 0;                                                 // the 64-word passes of sv_extract's waves
        for (auto const& j : plan.jobs) passes += (j.n_words + 63u) / 64u;
        fprintf(stderr, "[flx sv] add: records %llu counted %zu words %zu signatures %llu (junctions %llu) passes %llu device_ms %.3f wall_ms_behind_the_checks %.3f\n",
                (unsigned long long)plan.n_records, plan.jobs.size(), pool.size(), (unsigned long long)n_keys, (unsigned long long)plan.n_junctions,
                (unsigned long long)passes, (double)ms, wall);
    }
    return FLX_OK;
}

bool reads_given(const uint64_t* read_offsets, uint64_t n_reads, const char* who) {
    if (n_reads && !read_offsets) { set_error(std::string(who) + ": null argument"); return false; }
    return true;
}

bool signature_valid(flx_sv_signature const& g) {
    return g.type <= SV_BND && g.side_a <= 1u && g.side_b <= 1u && g.reserved == 0u && g.ref_a >= 0 && g.ref_b >= 0 && (u64)g.ref_a < SV_MAX_REFS && (u64)g.ref_b < SV_MAX_REFS;
}

}  // namespace

extern "C" int flx_sv_create_for_lengths(int hip_device, const uint64_t* ref_lens, uint32_t n_refs, const flx_sv_options* o, flx_sv** out) {
    if (!out) { set_error("flx_sv_create_for_lengths: null argument"); return FLX_ERR_INVALID; }
    std::vector<u64> starts;
    if (!sv_options_valid(o) || !sv_lengths_valid(ref_lens, n_refs, "flx_sv_create_for_lengths", starts)) return FLX_ERR_INVALID;
    return create(hip_device, std::move(starts), o, out);
}
extern "C" int flx_sv_create(flx_ctx* ctx, const flx_sv_options* o, flx_sv** out) {
    if (!ctx || !ctx->hidx || !out) { set_error("flx_sv_create: null argument"); return FLX_ERR_INVALID; }
    std::vector<u64> starts;
    if (!sv_options_valid(o) || !sv_lengths_valid(ctx->hidx->seq_len.data(), (uint32_t)ctx->hidx->seq_len.size(), "flx_sv_create", starts)) return FLX_ERR_INVALID;
    return create(ctx->device, std::move(starts), o, out);
}
extern "C" void flx_sv_free(flx_sv* s) { free_object(s); }

extern "C" int flx_sv_add_records(flx_sv* s, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words, const uint64_t* read_offsets,
                                  uint64_t n_reads) {
    if (!s || (n && !records) || !reads_given(read_offsets, n_reads, "flx_sv_add_records")) { set_error("flx_sv_add_records: null argument"); return FLX_ERR_INVALID; }
    SvPlan plan;
    if (!sv_plan(s->starts, s->opt, records, n, cigar_words, n_words, n_reads, [&](u64 r) { return read_offsets[r + 1] - read_offsets[r]; }, "flx_sv_add_records", plan))
        return FLX_ERR_INVALID;
    return commit(s, plan, cigar_words, "flx_sv_add_records");
}
// all pieces of a run are judged before any is added
extern "C" int flx_sv_add_run(flx_sv* s, const flx_run* run, const uint64_t* read_offsets, uint64_t n_reads) {
    const char* const who = "flx_sv_add_run";
    if (!s || !run || !reads_given(read_offsets, n_reads, who)) { set_error(std::string(who) + ": null argument"); return FLX_ERR_INVALID; }
    if (s->opt.min_mapq > 0 && !run->has_mapq) { set_error(std::string(who) + ": min_mapq needs a run made with flx_output_options.mapq"); return FLX_ERR_INVALID; }
    auto const pieces = run_pieces(run);
    std::vector<SvPlan> plans(pieces.size());
    if (!judge_in_parallel(pieces.size(), [&](size_t i) {
            return sv_plan(s->starts, s->opt, pieces[i]->records.data(), pieces[i]->records.size(), pieces[i]->cigars.data(), pieces[i]->cigars.size(), n_reads,
                           [&](u64 r) { return read_offsets[r + 1] - read_offsets[r]; }, who, plans[i]);
        }))
        return FLX_ERR_INVALID;
    for (size_t i = 0; i < pieces.size(); ++i) {
        int const rc = commit(s, plans[i], pieces[i]->cigars.data(), who);
        if (rc) return rc;
    }
    return FLX_OK;
}

extern "C" int flx_sv_absorb(flx_sv* into, flx_sv* from) {
    if (!into || !from || into == from) { set_error("flx_sv_absorb: null argument, or an object absorbed into itself"); return FLX_ERR_INVALID; }
    std::lock(into->mu, from->mu);
    std::lock_guard<std::mutex> g1(into->mu, std::adopt_lock), g2(from->mu, std::adopt_lock);
    if (into->finished || from->finished) { set_error("flx_sv_absorb: an sv object is finished"); return FLX_ERR_INVALID; }
    if (into->starts != from->starts) { set_error("flx_sv_absorb: the objects belong to different reference lengths"); return FLX_ERR_INVALID; }
    if (!sv_options_equal(into->opt, from->opt)) { set_error("flx_sv_absorb: the objects have different options"); return FLX_ERR_INVALID; }
    u64 const n = from->count;
    if (n == 0) return FLX_OK;
    if (n > SV_MAX_SIGNATURES - into->count) { set_error("flx_sv_absorb: more than 2^32 - 1 signatures in one sv object"); return FLX_ERR_CAPACITY; }
    FLX_HIP(hipSetDevice(into->device));
    int rc;
    u64 const piece = std::min(n, ABSORB_CHUNK);
    if ((rc = grow(into, into->count + n)) || (rc = into->pinned.ensure(piece * sizeof(SortKey)))) return rc;
    for (u64 at = 0; at < n; at += piece) {
        u64 const m = std::min(piece, n - at);
        FLX_HIP(hipSetDevice(from->device));
        FLX_HIP(hipMemcpyAsync(into->pinned.ptr, from->keys.as<SortKey>() + at, m * sizeof(SortKey), hipMemcpyDeviceToHost, from->stream));
        FLX_HIP(hipStreamSynchronize(from->stream));
        FLX_HIP(hipSetDevice(into->device));
        FLX_HIP(hipMemcpyAsync(into->keys.as<SortKey>() + into->count + at, into->pinned.ptr, m * sizeof(SortKey), hipMemcpyHostToDevice, into->stream));
        FLX_HIP(hipStreamSynchronize(into->stream));    // (the pinned piece is free again)
    }
    into->count += n;
    from->count = 0;
    return FLX_OK;
}

extern "C" int flx_sv_finish(flx_sv* s) {
    if (!s) { set_error("flx_sv_finish: null argument"); return FLX_ERR_INVALID; }
    std::lock_guard<std::mutex> g(s->mu);
    if (s->finished) { set_error("flx_sv_finish: the sv object is finished"); return FLX_ERR_INVALID; }
    auto const t0 = std::chrono::steady_clock::now();
    u64 const n = s->count;
    SvThresholds const t = sv_thresholds(s->opt);
    u32 passes = 0;
    u64 n_all = 0;
    float ms = 0;
    if (n) {
        FLX_HIP(hipSetDevice(s->device));
        RadixSorter& so = s->sorter;
        int rc;
        if ((rc = so.keys_a.ensure(n * sizeof(SortKey), true)) || (rc = so.keys_b.ensure(n * sizeof(SortKey), true)) || (rc = so.pay_a.ensure(n * 4, true)) ||
            (rc = so.pay_b.ensure(n * 4, true)) || (rc = s->ids.ensure(n * 4, true)) || (rc = s->scan.reserve(n)) ||
            (rc = s->signatures.ensure(n * sizeof(flx_sv_signature), true)))
            return rc;
        if ((rc = s->span_begin())) return rc;
        // (1) key order; the table itself is the first buffer: it is not read in adding order again
        SortKey *sorted, *sorted2;
        u32 *payload, *payload2, p1 = 0, p2 = 0;
        FLX_LAUNCH("sort_iota", SortDevice::iota(s->stream, so.pay_a.as<u32>(), n));
        if ((rc = so.sort(s->stream, s->keys.as<SortKey>(), so.keys_b.as<SortKey>(), so.pay_a.as<u32>(), so.pay_b.as<u32>(), n, &sorted, &payload, &p1))) return rc;
        FLX_LAUNCH("sv_signatures", SvDevice::signatures(s->stream, sorted, n, s->signatures.as<flx_sv_signature>()));
        u32* const ids = s->ids.as<u32>();
        FLX_LAUNCH("sv_coarse_flags", SvDevice::coarse_flags(s->stream, sorted, n, t.max_distance, ids));
        if ((rc = s->scan.inclusive(s->stream, ids, n))) return rc;
        // (2) (group, q, pos_a) order, in the buffer of the first sort that does not hold its result and a third one
        SortKey* const keys2 = sorted == s->keys.as<SortKey>() ? so.keys_b.as<SortKey>() : s->keys.as<SortKey>();
        struct Emptied { flx_sv* s; bool armed; ~Emptied() { if (armed) s->count = 0; } } emptied{s, true};      // the table may be written over from here on: a failure leaves the object empty
        FLX_LAUNCH("sv_regroup", SvDevice::regroup(s->stream, sorted, ids, n, keys2));
        FLX_LAUNCH("sort_iota", SortDevice::iota(s->stream, so.pay_a.as<u32>(), n));
        if ((rc = so.sort(s->stream, keys2, so.keys_a.as<SortKey>(), so.pay_a.as<u32>(), so.pay_b.as<u32>(), n, &sorted2, &payload2, &p2))) return rc;
        passes = p1 + p2;
        FLX_LAUNCH("sv_fine_flags", SvDevice::fine_flags(s->stream, sorted2, n, t.max_distance, ids));
        if ((rc = s->scan.inclusive(s->stream, ids, n))) return rc;
        u32 last = 0;
        FLX_HIP(hipMemcpyAsync(&last, ids + (n - 1), 4, hipMemcpyDeviceToHost, s->stream));
        FLX_HIP(hipStreamSynchronize(s->stream));
        n_all = (u64)last + 1;
        u64 const nt = ScanDriver::tiles(n_all);
        if ((rc = s->cluster_starts.ensure(n_all * 4, true)) || (rc = s->all_clusters.ensure(n_all * sizeof(flx_sv_cluster), true)) || (rc = s->tile_counts.ensure(nt * 4, true)))
            return rc;
        flx_sv_cluster* const all = s->all_clusters.as<flx_sv_cluster>();
        FLX_LAUNCH("sv_cluster_heads", SvDevice::cluster_heads(s->stream, ids, n, s->cluster_starts.as<u32>(), all));
        FLX_LAUNCH("sv_cluster_bounds", SvDevice::cluster_bounds(s->stream, sorted2, ids, n, all));
        FLX_LAUNCH("sv_cluster_fill", SvDevice::cluster_fill(s->stream, sorted, sorted2, payload2, s->cluster_starts.as<u32>(), n, n_all, all));
        // the clusters with enough support: count, scan, emit
        FLX_LAUNCH("sv_compact", SvDevice::compact(s->stream, 0, all, n_all, t.min_support, s->tile_counts.as<u32>(), nullptr));
        if ((rc = s->scan.inclusive(s->stream, s->tile_counts.as<u32>(), nt))) return rc;       // (nt <= n: reserved)
        FLX_HIP(hipMemcpyAsync(&last, s->tile_counts.as<u32>() + (nt - 1), 4, hipMemcpyDeviceToHost, s->stream));
        FLX_HIP(hipStreamSynchronize(s->stream));
        s->n_clusters = last;
        if (last) {
            if ((rc = s->clusters.ensure((u64)last * sizeof(flx_sv_cluster), true))) return rc;
            FLX_LAUNCH("sv_compact", SvDevice::compact(s->stream, 1, all, n_all, t.min_support, s->tile_counts.as<u32>(), s->clusters.as<flx_sv_cluster>()));
        }
        if ((rc = s->span_end())) return rc;
        FLX_HIP(hipStreamSynchronize(s->stream));
        if ((rc = s->span_ms(ms))) return rc;
        emptied.armed = false;
        s->keys.release(); so.release(); s->ids.release(); s->cluster_starts.release(); s->all_clusters.release(); s->tile_counts.release();
        s->jobs.release(); s->members.release(); s->words.release(); s->segments.release();
        s->capacity = 0;
    }
    s->finished = true;
    if (s->profile) {
        double const wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[flx sv] finish: signatures %llu passes %u clusters %llu kept %llu device_ms %.3f wall_ms %.3f\n", (unsigned long long)n, passes,
                (unsigned long long)n_all, (unsigned long long)s->n_clusters, (double)ms, wall);
    }
    return FLX_OK;
}

extern "C" uint64_t flx_sv_num_signatures(const flx_sv* s) {
    if (!s) return 0;
    std::lock_guard<std::mutex> g(const_cast<flx_sv*>(s)->mu);
    return s->finished ? s->count : 0;
}
extern "C" uint64_t flx_sv_num_clusters(const flx_sv* s) {
    if (!s) return 0;
    std::lock_guard<std::mutex> g(const_cast<flx_sv*>(s)->mu);
    return s->finished ? s->n_clusters : 0;
}
extern "C" int flx_sv_copy_signatures(const flx_sv* cs, uint64_t from, uint64_t to, flx_sv_signature* out) {
    if (!finished_for_copy(cs, "flx_sv_copy_signatures", "flx_sv_finish")) return FLX_ERR_INVALID;
    flx_sv* const s = const_cast<flx_sv*>(cs);
    std::lock_guard<std::mutex> g(s->mu);
    if (from > to || to > s->count) { set_error("flx_sv_copy_signatures: a stretch outside the signatures"); return FLX_ERR_INVALID; }
    if (from == to) return FLX_OK;
    if (!out) { set_error("flx_sv_copy_signatures: null argument"); return FLX_ERR_INVALID; }
    FLX_HIP(hipSetDevice(s->device));
    FLX_HIP(hipMemcpyAsync(out, s->signatures.as<flx_sv_signature>() + from, (to - from) * sizeof(flx_sv_signature), hipMemcpyDeviceToHost, s->stream));
    FLX_HIP(hipStreamSynchronize(s->stream));
    return FLX_OK;
}
extern "C" int flx_sv_copy_clusters(const flx_sv* cs, flx_sv_cluster* out, uint64_t capacity) {
    if (!finished_for_copy(cs, "flx_sv_copy_clusters", "flx_sv_finish")) return FLX_ERR_INVALID;
    flx_sv* const s = const_cast<flx_sv*>(cs);
    std::lock_guard<std::mutex> g(s->mu);
    if (capacity < s->n_clusters) { set_error("flx_sv_copy_clusters: the cluster buffer is too small, " + std::to_string(s->n_clusters) + " clusters"); return FLX_ERR_CAPACITY; }
    if (s->n_clusters == 0) return FLX_OK;
    if (!out) { set_error("flx_sv_copy_clusters: null argument"); return FLX_ERR_INVALID; }
    FLX_HIP(hipSetDevice(s->device));
    FLX_HIP(hipMemcpyAsync(out, s->clusters.ptr, s->n_clusters * sizeof(flx_sv_cluster), hipMemcpyDeviceToHost, s->stream));
    FLX_HIP(hipStreamSynchronize(s->stream));
    return FLX_OK;
}

extern "C" int flx_sv_host(const uint64_t* ref_lens, uint32_t n_refs, const flx_sv_options* o, const flx_record* records, uint64_t n, const uint32_t* cigar_words,
                           uint64_t n_words, const uint64_t* read_offsets, uint64_t n_reads, flx_sv_signature* out, uint64_t* n_signatures) {
    std::vector<u64> starts;
    if (!sv_options_valid(o) || !sv_lengths_valid(ref_lens, n_refs, "flx_sv_host", starts)) return FLX_ERR_INVALID;
    if (!n_signatures || (n && !records) || !reads_given(read_offsets, n_reads, "flx_sv_host")) { set_error("flx_sv_host: null argument"); return FLX_ERR_INVALID; }
    flx_sv_options const opt = sv_options_or_default(o);
    SvPlan plan;
    if (!sv_plan(starts, opt, records, n, cigar_words, n_words, n_reads, [&](u64 r) { return read_offsets[r + 1] - read_offsets[r]; }, "flx_sv_host", plan)) return FLX_ERR_INVALID;
    std::vector<SortKey> keys;
    sv_keys_host(plan, cigar_words, sv_thresholds(opt).min_length, keys);
    u64 const capacity = *n_signatures;
    *n_signatures = keys.size();
    if (keys.size() > capacity || (!keys.empty() && !out)) { set_error("flx_sv_host: the signature buffer is too small, " + std::to_string(keys.size()) + " signatures"); return FLX_ERR_CAPACITY; }
    std::sort(keys.begin(), keys.end(), [](SortKey const& a, SortKey const& b) { return sort_key_less(a, b); });
    for (size_t i = 0; i < keys.size(); ++i) out[i] = sv_signature_of(keys[i]);
    return FLX_OK;
}

extern "C" int flx_sv_clusters_host(const flx_sv_options* o, const flx_sv_signature* signatures, uint64_t n, flx_sv_cluster* out, uint64_t* n_clusters) {
    if (!sv_options_valid(o)) return FLX_ERR_INVALID;
    if (!n_clusters || (n && !signatures)) { set_error("flx_sv_clusters_host: null argument"); return FLX_ERR_INVALID; }
    std::vector<SortKey> keys(n);
    for (u64 i = 0; i < n; ++i) {
        if (!signature_valid(signatures[i])) { set_error("flx_sv_clusters_host: signature " + std::to_string(i) + " has a field outside its range"); return FLX_ERR_INVALID; }
        keys[i] = sv_key_of(signatures[i]);
    }
    std::sort(keys.begin(), keys.end(), [](SortKey const& a, SortKey const& b) { return sort_key_less(a, b); });
    std::vector<flx_sv_cluster> clusters;
    sv_clusters_host(keys.data(), n, sv_thresholds(sv_options_or_default(o)), clusters);
    u64 const capacity = *n_clusters;
    *n_clusters = clusters.size();
    if (clusters.size() > capacity || (!clusters.empty() && !out)) { set_error("flx_sv_clusters_host: the cluster buffer is too small, " + std::to_string(clusters.size()) + " clusters"); return FLX_ERR_CAPACITY; }
    if (!clusters.empty()) memcpy(out, clusters.data(), clusters.size() * sizeof(flx_sv_cluster));
    return FLX_OK;
}
