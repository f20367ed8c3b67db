// flx_svcaller: the object behind the structural-variant calling calls of the C ABI (include/floxer_amd.h). The rule and its checks:
// flx_svcall.hpp; what the device path and the host form share, and the host form's table: flx_svcaller.hpp (no HIP); the kernels:
// flx_svcall.hip; the sort's driver: flx_sort_driver.hpp; what it shares with the other side objects: flx_object.hpp. The object owns one
// stream, the key table (one SortKey per counted record's span, in adding order, growing by doubling), two state words (the largest span
// so far, which every add's kernel raises, and an add's flag), the staging buffers of an add, the sequences' lengths and, behind
// flx_svcaller_finish, the spans in key order and the rows. Adds judge their records and stage their words without the object's lock
// and take it for the upload and the launch only, so several host threads may add at once. With device -1 nothing of the device
// exists and the same calls keep the keys in a host vector (SvcallHostTable). Made for a context it is counted there
// (flx_ctx_destroy waits for it).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>

#include "flx_object.hpp"
#include "flx_sort_driver.hpp"
#include "flx_svcaller.hpp"

using namespace flx;

namespace {
constexpr u64 ABSORB_CHUNK = 1ull << 20;               // keys per piece of an absorb (16 MB)
}  // namespace

struct flx_svcaller : SideObject {       // mu: the table, staging, launches and `finished`; FLX_SVCALLER_PROFILE
    flx_svcall_options opt{};
    flx_ctx* ctx = nullptr;              // made by flx_svcaller_create: counted there
    std::vector<u64> starts;             // n_refs + 1, as coverage judges records against them
    u64 initial_capacity = SVCALLER_DEFAULT_INITIAL_CAPACITY;
    bool finished = false;
    u64 count = 0, capacity = 0;         // spans added; spans the table holds
    u32 max_span = 0;                    // the host's copy of state[0]
    DeviceBuffer keys;                   // the table; behind finish the spans in key order
    DeviceBuffer state;                  // two words: the largest span, an add's flag
    DeviceBuffer d_lens;                 // the sequences' lengths as u32
    DeviceBuffer jobs, words;            // an add's staging
    RadixSorter sorter;                  // finish
    DeviceBuffer d_clusters, d_index, rows;
    u64 n_rows = 0;
    PinnedBuffer pinned;                 // absorb: a piece of the other object's keys on its way through the host
    SvcallHostTable host;                // the host form
    ~flx_svcaller() {
        if (ctx) { std::lock_guard<std::mutex> g(ctx->spare_mu); --ctx->live_svcallers; }
    }
};

namespace {

int create(int device, std::vector<u64>&& starts, const flx_svcall_options* o, u64 initial_capacity, flx_svcaller** out) {
    auto s = std::make_unique<flx_svcaller>();          // (an error below drops it: nothing stays allocated)
    s->opt = svcall_options_or_default(o);
    if (initial_capacity) s->initial_capacity = initial_capacity;
    s->starts = std::move(starts);
    int rc = s->open(device, "FLX_SVCALLER_PROFILE");
    if (rc) return rc;
    if (device >= 0) {
        std::vector<u32> lens(s->starts.size() - 1);
        for (size_t r = 0; r < lens.size(); ++r) lens[r] = (u32)(s->starts[r + 1] - s->starts[r]);       // (below 2^31: the lengths were judged)
        if ((rc = s->d_lens.ensure(lens.size() * 4, true)) || (rc = s->state.ensure(8, true))) return rc;
        FLX_HIP(hipMemcpyAsync(s->d_lens.ptr, lens.data(), lens.size() * 4, hipMemcpyHostToDevice, s->stream));
        FLX_HIP(hipMemsetAsync(s->state.ptr, 0, 8, s->stream));
        FLX_HIP(hipStreamSynchronize(s->stream));
    }
    *out = s.release();
    return FLX_OK;
}

// the table holds at least `need` keys afterwards, its first `count` as before; a failure leaves it as it was
int grow(flx_svcaller* s, u64 need) {
    if (need <= s->capacity) return FLX_OK;
    u64 const cap = std::min<u64>(std::max<u64>({need, s->capacity * 2, s->initial_capacity}), SVCALL_MAX_SPANS);
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

// the object's max_span word on the device made equal to the host's copy
int put_max_span(flx_svcaller* s) {
    FLX_HIP(hipMemcpyAsync(s->state.ptr, &s->max_span, 4, hipMemcpyHostToDevice, s->stream));
    FLX_HIP(hipStreamSynchronize(s->stream));
    return FLX_OK;
}

// the judged jobs of one word pool: their words staged, then uploaded and launched under the object's lock
int commit(flx_svcaller* s, std::vector<SvcallJob>& jobs, u64 n_records, const uint32_t* cigar_words, const char* who) {
    auto const t0 = std::chrono::steady_clock::now();
    std::vector<u32> pool;
    if (!jobs.empty() && s->device >= 0) compact_words(jobs, cigar_words, pool);
    std::lock_guard<std::mutex> g(s->mu);
    if (s->finished) { set_error(std::string(who) + ": the svcaller object is finished"); return FLX_ERR_INVALID; }
    if (jobs.empty()) return FLX_OK;
    if (s->device < 0) return s->host.add(jobs, who);
    int rc;
    if ((rc = spans_room_judged(s->count, jobs.size(), who))) return rc;
    FLX_HIP(hipSetDevice(s->device));
    if ((rc = grow(s, s->count + jobs.size()))) return rc;
    if ((rc = s->jobs.ensure(jobs.size() * sizeof(SvcallJob))) || (rc = s->words.ensure(std::max<size_t>(pool.size(), 1) * 4))) return rc;
    FLX_HIP(hipMemcpyAsync(s->jobs.ptr, jobs.data(), jobs.size() * sizeof(SvcallJob), hipMemcpyHostToDevice, s->stream));
    FLX_HIP(hipMemcpyAsync(s->words.ptr, pool.data(), pool.size() * 4, hipMemcpyHostToDevice, s->stream));
    FLX_HIP(hipMemsetAsync(s->state.as<u32>() + 1, 0, 4, s->stream));
    if ((rc = s->span_begin())) return rc;
    // (room for the jobs' keys behind the count: grow saw to it; fewer than 2^32 jobs: the room was judged)
    FLX_LAUNCH("svcall_spans", SvcallDevice::spans(s->stream, s->jobs.as<SvcallJob>(), (u32)jobs.size(), s->words.as<u32>(), s->keys.as<SortKey>() + s->count, s->state.as<u32>()));
    if ((rc = s->span_end())) return rc;
    u32 state[2] = {0, 0};
    FLX_HIP(hipMemcpyAsync(state, s->state.ptr, 8, hipMemcpyDeviceToHost, s->stream));
    FLX_HIP(hipStreamSynchronize(s->stream));           // (the staging buffers are free for the next add)
    if (state[1]) {
        if ((rc = put_max_span(s))) return rc;          // (the add is not counted: what it raised is taken back)
        set_error(std::string(who) + ": a kernel found a record at odds with the host's judgement (flag " + std::to_string(state[1]) + ")");
        return FLX_ERR_INTERNAL;
    }
    s->count += jobs.size();
    s->max_span = state[0];
    if (s->profile) {
        float ms;
        if ((rc = s->span_ms(ms))) return rc;
        double const wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        u64 passes = 0;                                                 // the 64-word passes of svcall_spans' waves
        for (auto const& j : jobs) passes += (j.n_words + 63u) / 64u;
        fprintf(stderr, "[flx svcaller] add: records %llu counted %zu words %zu passes %llu max_span %u device_ms %.3f wall_ms_behind_the_checks %.3f\n",
                (unsigned long long)n_records, jobs.size(), pool.size(), (unsigned long long)passes, s->max_span, (double)ms, wall);
    }
    return FLX_OK;
}

}  // namespace

extern "C" int flx_svcaller_create_for_lengths(int hip_device, const uint64_t* ref_lens, uint32_t n_refs, const flx_svcall_options* o, uint64_t initial_capacity,
                                               flx_svcaller** out) {
    const char* const who = "flx_svcaller_create_for_lengths";
    if (!out) { set_error(std::string(who) + ": null argument"); return FLX_ERR_INVALID; }
    if (hip_device < -1) { set_error(std::string(who) + ": a device below -1"); return FLX_ERR_INVALID; }
    if (initial_capacity > SVCALL_MAX_SPANS) { set_error(std::string(who) + ": initial_capacity above 2^32 - 1"); return FLX_ERR_INVALID; }
    std::vector<u64> starts;
    if (!svcall_options_valid(o) || !sv_lengths_valid(ref_lens, n_refs, who, starts)) return FLX_ERR_INVALID;
    return create(hip_device, std::move(starts), o, initial_capacity, out);
}
extern "C" int flx_svcaller_create(flx_ctx* ctx, const flx_svcall_options* o, flx_svcaller** out) {
    if (!ctx || !ctx->hidx || !out) { set_error("flx_svcaller_create: null argument"); return FLX_ERR_INVALID; }
    std::vector<u64> starts;
    if (!svcall_options_valid(o) || !sv_lengths_valid(ctx->hidx->seq_len.data(), (uint32_t)ctx->hidx->seq_len.size(), "flx_svcaller_create", starts)) return FLX_ERR_INVALID;
    if (ctx->device < 0) { set_error("flx_svcaller_create: the context has no device (the host form is flx_svcaller_create_for_lengths with device -1)"); return FLX_ERR_INVALID; }
    flx_svcaller* s = nullptr;
    int const rc = create(ctx->device, std::move(starts), o, 0, &s);
    if (rc) return rc;
    { std::lock_guard<std::mutex> g(ctx->spare_mu); ++ctx->live_svcallers; }
    s->ctx = ctx;
    *out = s;
    return FLX_OK;
}
extern "C" void flx_svcaller_free(flx_svcaller* s) { free_object(s); }

extern "C" int flx_svcaller_add_records(flx_svcaller* s, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words) {
    if (!s || (n && !records)) { set_error("flx_svcaller_add_records: null argument"); return FLX_ERR_INVALID; }
    std::vector<SvcallJob> jobs;
    if (!svcall_plan(s->starts, s->opt, records, n, cigar_words, n_words, "flx_svcaller_add_records", jobs)) return FLX_ERR_INVALID;
    return commit(s, jobs, n, cigar_words, "flx_svcaller_add_records");
}
// all pieces of a run are judged before any is added
extern "C" int flx_svcaller_add_run(flx_svcaller* s, const flx_run* run) {
    const char* const who = "flx_svcaller_add_run";
    if (!s || !run) { set_error(std::string(who) + ": null argument"); return FLX_ERR_INVALID; }
    if (s->opt.min_mapq > 0 && !run->has_mapq) { set_error(std::string(who) + ": min_mapq needs a run made with flx_output_options.mapq"); return FLX_ERR_INVALID; }
    auto const pieces = run_pieces(run);
    std::vector<std::vector<SvcallJob>> plans(pieces.size());
    if (!judge_in_parallel(pieces.size(), [&](size_t i) {
            return svcall_plan(s->starts, s->opt, pieces[i]->records.data(), pieces[i]->records.size(), pieces[i]->cigars.data(), pieces[i]->cigars.size(), who, plans[i]);
        }))
        return FLX_ERR_INVALID;
    for (size_t i = 0; i < pieces.size(); ++i) {
        int const rc = commit(s, plans[i], pieces[i]->records.size(), pieces[i]->cigars.data(), who);
        if (rc) return rc;
    }
    return FLX_OK;
}

extern "C" int flx_svcaller_absorb(flx_svcaller* into, flx_svcaller* from) {
    const char* const who = "flx_svcaller_absorb";
    if (!into || !from || into == from) { set_error(std::string(who) + ": null argument, or an object absorbed into itself"); return FLX_ERR_INVALID; }
    std::lock(into->mu, from->mu);
    std::lock_guard<std::mutex> g1(into->mu, std::adopt_lock), g2(from->mu, std::adopt_lock);
    if (into->finished || from->finished) { set_error(std::string(who) + ": an svcaller object is finished"); return FLX_ERR_INVALID; }
    if (into->starts != from->starts) { set_error(std::string(who) + ": the objects belong to different reference lengths"); return FLX_ERR_INVALID; }
    if (!svcall_options_equal(into->opt, from->opt)) { set_error(std::string(who) + ": the objects have different options"); return FLX_ERR_INVALID; }
    if ((into->device < 0) != (from->device < 0)) { set_error(std::string(who) + ": a host form and a device object cannot absorb one another"); return FLX_ERR_INVALID; }
    if (into->device < 0) return into->host.absorb(from->host, who);
    u64 const n = from->count;
    if (n == 0) return FLX_OK;
    int rc;
    if ((rc = spans_room_judged(into->count, n, who))) return rc;
    FLX_HIP(hipSetDevice(into->device));
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
    into->max_span = std::max(into->max_span, from->max_span);
    if ((rc = put_max_span(into))) return rc;
    from->count = 0;
    from->max_span = 0;
    FLX_HIP(hipSetDevice(from->device));
    return put_max_span(from);
}

extern "C" int flx_svcaller_finish(flx_svcaller* s, const flx_sv_cluster* clusters, uint64_t n_clusters) {
    const char* const who = "flx_svcaller_finish";
    if (!s || (n_clusters && !clusters)) { set_error(std::string(who) + ": null argument"); return FLX_ERR_INVALID; }
    std::lock_guard<std::mutex> g(s->mu);
    if (s->finished) { set_error(std::string(who) + ": the svcaller object is finished"); return FLX_ERR_INVALID; }
    u64 n_rows = 0;
    if (!svcall_clusters_valid(s->starts, clusters, n_clusters, who, n_rows)) return FLX_ERR_INVALID;
    std::vector<u32> index;
    int rc;
    if ((rc = svcall_row_index(clusters, n_clusters, who, index))) return rc;
    SvcallModel const model = svcall_model(s->opt);
    if (s->device < 0) {
        s->host.finish(s->starts, clusters, n_clusters, model);
        s->finished = true;
        return FLX_OK;
    }
    auto const t0 = std::chrono::steady_clock::now();
    u64 const n = s->count;
    u32 passes = 0;
    float ms = 0;
    FLX_HIP(hipSetDevice(s->device));
    if (n_rows) {
        if ((rc = s->d_clusters.ensure(n_clusters * sizeof(flx_sv_cluster), true)) || (rc = s->d_index.ensure(n_rows * 4, true)) || (rc = s->rows.ensure(n_rows * sizeof(flx_svcall_row), true)))
            return rc;
    }
    RadixSorter& so = s->sorter;
    if (n > 1 && ((rc = so.keys_b.ensure(n * sizeof(SortKey), true)) || (rc = so.pay_a.ensure(n * 4, true)) || (rc = so.pay_b.ensure(n * 4, true)))) return rc;
    // the table may be written over from here on: a failure leaves the object empty
    struct Emptied { flx_svcaller* s; bool armed; ~Emptied() { if (armed) { s->count = 0; s->max_span = 0; } } } emptied{s, true};
    if ((rc = s->span_begin())) return rc;
    // (1) key order; the table itself is the first buffer: it is not read in adding order again
    SortKey* sorted = s->keys.as<SortKey>();
    if (n > 1) {
        u32* payload;
        FLX_LAUNCH("sort_iota", SortDevice::iota(s->stream, so.pay_a.as<u32>(), n));
        if ((rc = so.sort(s->stream, s->keys.as<SortKey>(), so.keys_b.as<SortKey>(), so.pay_a.as<u32>(), so.pay_b.as<u32>(), n, &sorted, &payload, &passes))) return rc;
    }
    // (2) the rows, behind the sort on the same stream
    if (n_rows) {
        FLX_HIP(hipMemcpyAsync(s->d_clusters.ptr, clusters, n_clusters * sizeof(flx_sv_cluster), hipMemcpyHostToDevice, s->stream));
        FLX_HIP(hipMemcpyAsync(s->d_index.ptr, index.data(), n_rows * 4, hipMemcpyHostToDevice, s->stream));
        FLX_LAUNCH("svcall_count", SvcallDevice::count(s->stream, sorted, n, s->max_span, s->d_clusters.as<flx_sv_cluster>(), s->d_index.as<u32>(), (u32)n_rows, s->d_lens.as<u32>(),
                                                       model, s->rows.as<flx_svcall_row>()));
    }
    if ((rc = s->span_end())) return rc;
    FLX_HIP(hipStreamSynchronize(s->stream));           // (the caller's clusters and `index` have gone up)
    if ((rc = s->span_ms(ms))) return rc;
    emptied.armed = false;
    if (n > 1 && sorted == so.keys_b.as<SortKey>()) s->keys.take(so.keys_b);       // the spans in key order stay, in whichever buffer holds them
    so.release(); s->jobs.release(); s->words.release(); s->d_clusters.release(); s->d_index.release();
    s->n_rows = n_rows;
    s->finished = true;
    if (s->profile) {
        double const wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[flx svcaller] finish: spans %llu passes %u clusters %llu rows %llu max_span %u device_ms %.3f wall_ms %.3f\n", (unsigned long long)n, passes,
                (unsigned long long)n_clusters, (unsigned long long)n_rows, s->max_span, (double)ms, wall);
    }
    return FLX_OK;
}

extern "C" uint64_t flx_svcaller_num_spans(const flx_svcaller* s) {
    if (!s) return 0;
    std::lock_guard<std::mutex> g(const_cast<flx_svcaller*>(s)->mu);
    return !s->finished ? 0 : s->device < 0 ? s->host.keys.size() : s->count;
}
extern "C" uint64_t flx_svcaller_num_rows(const flx_svcaller* s) {
    if (!s) return 0;
    std::lock_guard<std::mutex> g(const_cast<flx_svcaller*>(s)->mu);
    return !s->finished ? 0 : s->device < 0 ? s->host.rows.size() : s->n_rows;
}
extern "C" uint32_t flx_svcaller_max_span(const flx_svcaller* s) {
    if (!s) return 0;
    std::lock_guard<std::mutex> g(const_cast<flx_svcaller*>(s)->mu);
    return !s->finished ? 0 : s->device < 0 ? s->host.max_span : s->max_span;
}
extern "C" int flx_svcaller_copy_spans(const flx_svcaller* cs, uint64_t from, uint64_t to, flx_svcall_span* out) {
    if (!finished_for_copy(cs, "flx_svcaller_copy_spans", "flx_svcaller_finish")) return FLX_ERR_INVALID;
    flx_svcaller* const s = const_cast<flx_svcaller*>(cs);
    std::lock_guard<std::mutex> g(s->mu);
    if (s->device < 0) return s->host.copy_spans(from, to, out);
    u64 n;
    int const rc = spans_copy_judged(s->count, from, to, out, n);
    if (rc || n == 0) return rc;
    std::vector<SortKey> keys(n);                       // the keys come down as they are and are unpacked here
    FLX_HIP(hipSetDevice(s->device));
    FLX_HIP(hipMemcpyAsync(keys.data(), s->keys.as<SortKey>() + from, n * sizeof(SortKey), hipMemcpyDeviceToHost, s->stream));
    FLX_HIP(hipStreamSynchronize(s->stream));
    for (u64 i = 0; i < n; ++i) out[i] = svcall_span_of(keys[i]);
    return FLX_OK;
}
extern "C" int flx_svcaller_copy_rows(const flx_svcaller* cs, flx_svcall_row* out, uint64_t capacity) {
    if (!finished_for_copy(cs, "flx_svcaller_copy_rows", "flx_svcaller_finish")) return FLX_ERR_INVALID;
    flx_svcaller* const s = const_cast<flx_svcaller*>(cs);
    std::lock_guard<std::mutex> g(s->mu);
    if (s->device < 0) return s->host.copy_rows(out, capacity);
    u64 n;
    int const rc = rows_copy_judged(s->n_rows, out, capacity, n);
    if (rc || n == 0) return rc;
    FLX_HIP(hipSetDevice(s->device));
    FLX_HIP(hipMemcpyAsync(out, s->rows.ptr, n * sizeof(flx_svcall_row), hipMemcpyDeviceToHost, s->stream));      // (n <= capacity: judged)
    FLX_HIP(hipStreamSynchronize(s->stream));
    return FLX_OK;
}

extern "C" int flx_svcaller_geometry(uint32_t out[4]) {
    if (!out) { set_error("flx_svcaller_geometry: null argument"); return FLX_ERR_INVALID; }
    out[0] = SvcallDevice::SPANS_GRID_CAP; out[1] = SvcallDevice::COUNT_GRID_CAP; out[2] = SvcallDevice::WAVES; out[3] = SortDevice::TILE_KEYS;
    return FLX_OK;
}
