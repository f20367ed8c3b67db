// flx_pileup: the object behind the allele-pileup calls of the C ABI (include/floxer_amd.h). The rule and its checks: flx_pileup.hpp; the
// kernels: flx_pileup.hip, the scan and the sum: flx_scan.hip; what it shares with the other side objects: flx_object.hpp. The object owns
// one stream, the accumulator (seven planes of u32 over the concatenation; DEPTH and DEL are differences until flx_pileup_finish) and its
// staging buffers. Adds judge their records and stage their words and letters without the object's lock and take it for the upload and
// the launch only, so several host threads may add at once.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>

#include "flx_object.hpp"
#include "flx_pileup.hpp"

using namespace flx;

struct flx_pileup : PlaneObject {        // acc: PILEUP_PLANES * stride entries; FLX_PILEUP_PROFILE: every add prints its upload, its kernel's device time and its wall time
    flx_pileup_options opt{};
    u64 stride = 0;                      // entries per plane: total + 1 rounded up to 64 (every plane starts 256-byte aligned)
    DeviceBuffer jobs, words, letters;   // an add's staging: the counted records, the words and the oriented sequences they refer to
    DeviceBuffer count;                  // per tile of the accumulator: its sites, scanned by finish
    u64 n_sites = 0;
    u32* plane(u32 k) const { return acc.as<u32>() + (u64)k * stride; }
};

namespace {

int create(int device, std::vector<u64>&& starts, const flx_pileup_options* o, flx_pileup** out) {
    auto c = std::make_unique<flx_pileup>();         // (an error below drops it: nothing stays allocated)
    c->opt = pileup_options_or_default(o);
    c->stride = (starts.back() + 1 + 63) / 64 * 64;
    int const rc = c->create(device, "FLX_PILEUP_PROFILE", std::move(starts), (u64)PILEUP_PLANES * c->stride, {&c->count});
    if (rc) return rc;
    *out = c.release();
    return FLX_OK;
}

// the judged jobs of one word pool: staged, then uploaded and launched under the object's lock. resident: the letters are read from the
// batch's device pool (on this object's device); otherwise the oriented sequences in use go up from `src`.
int commit(flx_pileup* c, std::vector<PileupJob>& jobs, const uint32_t* cigar_words, Letters const& src, const flx_reads* resident, const char* who) {
    if (jobs.size() >= (1ull << 32)) { set_error(std::string(who) + ": too many records in one call"); return FLX_ERR_INVALID; }
    auto const t0 = std::chrono::steady_clock::now();
    std::vector<u32> pool;
    std::vector<u8> letters;
    if (!jobs.empty()) {
        compact_words(jobs, cigar_words, pool);
        if (resident) for (auto& j : jobs) j.seq_off = resident->pool_off[j.read_index] + (j.reverse ? resident->lens[j.read_index] : 0);
        else stage_letters(jobs, src, letters);
    }
    std::lock_guard<std::mutex> g(c->mu);
    if (c->finished) { set_error(std::string(who) + ": the pileup object is finished"); return FLX_ERR_INVALID; }
    if (jobs.empty()) return FLX_OK;
    FLX_HIP(hipSetDevice(c->device));
    int rc;
    if ((rc = c->jobs.ensure(jobs.size() * sizeof(PileupJob))) || (rc = c->words.ensure(pool.size() * 4)) || (rc = c->letters.ensure(letters.size() + 1))) return rc;
    FLX_HIP(hipMemcpyAsync(c->jobs.ptr, jobs.data(), jobs.size() * sizeof(PileupJob), hipMemcpyHostToDevice, c->stream));
    FLX_HIP(hipMemcpyAsync(c->words.ptr, pool.data(), pool.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (!letters.empty()) FLX_HIP(hipMemcpyAsync(c->letters.ptr, letters.data(), letters.size(), hipMemcpyHostToDevice, c->stream));
    if ((rc = c->span_begin())) return rc;
    FLX_LAUNCH("pileup_add", PileupDevice::add(c->stream, c->jobs.as<PileupJob>(), (u32)jobs.size(), c->words.as<u32>(),
                                               resident ? resident->d_pool.as<u8>() : c->letters.as<u8>(), c->acc.as<u32>(), c->stride));
    if ((rc = c->span_end())) return rc;
    FLX_HIP(hipStreamSynchronize(c->stream));           // (the staging buffers are free for the next add)
    if (c->profile) {
        float ms;
        if ((rc = c->span_ms(ms))) return rc;
        double const wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[flx pileup] add: records %zu words %zu letters %zu upload_bytes %zu pileup_add_ms %.3f wall_ms_behind_the_checks %.3f\n", jobs.size(), pool.size(),
                letters.size(), jobs.size() * sizeof(PileupJob) + pool.size() * 4 + letters.size(), (double)ms, wall);
    }
    return FLX_OK;
}

// all pieces of a run are judged before any is added
int add_run(flx_pileup* c, const flx_run* run, Letters const& src, const flx_reads* resident, const char* who) {
    if (c->opt.min_mapq > 0 && !run->has_mapq) { set_error(std::string(who) + ": min_mapq needs a run made with flx_output_options.mapq"); return FLX_ERR_INVALID; }
    auto const pieces = run_pieces(run);
    std::vector<std::vector<PileupJob>> jobs(pieces.size());
    if (!judge_in_parallel(pieces.size(), [&](size_t i) {
            return pileup_plan(c->starts, c->opt, pieces[i]->records.data(), pieces[i]->records.size(), pieces[i]->cigars.data(), pieces[i]->cigars.size(), src.n_reads,
                               [&](u64 r) { return src.length(r); }, who, jobs[i]);
        }))
        return FLX_ERR_INVALID;
    for (size_t i = 0; i < pieces.size(); ++i) {
        int const rc = commit(c, jobs[i], pieces[i]->cigars.data(), src, resident, who);
        if (rc) return rc;
    }
    return FLX_OK;
}

bool reads_given(const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads, const char* who) {
    if (n_reads && (!read_pool || !read_offsets)) { set_error(std::string(who) + ": null argument"); return false; }
    return true;
}

}  // namespace

extern "C" int flx_pileup_create_for_lengths(int hip_device, const uint64_t* ref_lens, uint32_t n_refs, const flx_pileup_options* o, flx_pileup** out) {
    if (!out) { set_error("flx_pileup_create_for_lengths: null argument"); return FLX_ERR_INVALID; }
    std::vector<u64> starts;
    if (!pileup_options_valid(o) || !coverage_lengths_valid(ref_lens, n_refs, "flx_pileup_create_for_lengths", starts)) return FLX_ERR_INVALID;
    return create(hip_device, std::move(starts), o, out);
}
extern "C" int flx_pileup_create(flx_ctx* ctx, const flx_pileup_options* o, flx_pileup** out) {
    if (!ctx || !ctx->hidx || !out) { set_error("flx_pileup_create: null argument"); return FLX_ERR_INVALID; }
    std::vector<u64> starts;
    if (!pileup_options_valid(o) || !coverage_lengths_valid(ctx->hidx->seq_len.data(), (uint32_t)ctx->hidx->seq_len.size(), "flx_pileup_create", starts)) return FLX_ERR_INVALID;
    return create(ctx->device, std::move(starts), o, out);
}
extern "C" void flx_pileup_free(flx_pileup* c) { free_object(c); }

extern "C" int flx_pileup_add_records(flx_pileup* c, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words,
                                      const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads) {
    if (!c || (n && !records) || !reads_given(read_pool, read_offsets, n_reads, "flx_pileup_add_records")) { set_error("flx_pileup_add_records: null argument"); return FLX_ERR_INVALID; }
    Letters src;
    src.read_pool = read_pool; src.read_offsets = read_offsets; src.n_reads = n_reads;
    std::vector<PileupJob> jobs;
    if (!pileup_plan(c->starts, c->opt, records, n, cigar_words, n_words, n_reads, [&](u64 r) { return src.length(r); }, "flx_pileup_add_records", jobs)) return FLX_ERR_INVALID;
    return commit(c, jobs, cigar_words, src, nullptr, "flx_pileup_add_records");
}
extern "C" int flx_pileup_add_run(flx_pileup* c, const flx_run* run, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads) {
    if (!c || !run || !reads_given(read_pool, read_offsets, n_reads, "flx_pileup_add_run")) { set_error("flx_pileup_add_run: null argument"); return FLX_ERR_INVALID; }
    Letters src;
    src.read_pool = read_pool; src.read_offsets = read_offsets; src.n_reads = n_reads;
    return add_run(c, run, src, nullptr, "flx_pileup_add_run");
}
extern "C" int flx_pileup_add_run_resident(flx_pileup* c, const flx_run* run, const flx_reads* reads) {
    if (!c || !run || !reads) { set_error("flx_pileup_add_run_resident: null argument"); return FLX_ERR_INVALID; }
    Letters src;
    src.batch = reads; src.n_reads = reads->n_reads;
    // the batch's device pool when it lives on this object's device, its host copy through the staged path otherwise
    bool const here = reads->ctx && reads->ctx->device == c->device && reads->d_pool.ptr;
    return add_run(c, run, src, here ? reads : nullptr, "flx_pileup_add_run_resident");
}

extern "C" int flx_pileup_absorb(flx_pileup* into, flx_pileup* from) {
    if (!into || !from || into == from) { set_error("flx_pileup_absorb: null argument, or an object absorbed into itself"); return FLX_ERR_INVALID; }
    std::lock(into->mu, from->mu);
    std::lock_guard<std::mutex> g1(into->mu, std::adopt_lock), g2(from->mu, std::adopt_lock);
    if (into->finished || from->finished) { set_error("flx_pileup_absorb: a pileup object is finished"); return FLX_ERR_INVALID; }
    if (into->starts != from->starts) { set_error("flx_pileup_absorb: the objects belong to different reference lengths"); return FLX_ERR_INVALID; }
    if (!pileup_options_equal(into->opt, from->opt)) { set_error("flx_pileup_absorb: the objects have different options"); return FLX_ERR_INVALID; }
    for (u32 k = 0; k < PILEUP_PLANES; ++k) {
        int const rc = absorb_plane(into, from, into->plane(k), from->plane(k), into->total + 1);
        if (rc) return rc;
    }
    return from->clear();
}

extern "C" int flx_pileup_finish(flx_pileup* c) {
    if (!c) { set_error("flx_pileup_finish: null argument"); return FLX_ERR_INVALID; }
    std::lock_guard<std::mutex> g(c->mu);
    if (c->finished) { set_error("flx_pileup_finish: the pileup object is finished"); return FLX_ERR_INVALID; }
    auto const t0 = std::chrono::steady_clock::now();
    FLX_HIP(hipSetDevice(c->device));
    int rc;
    if ((rc = c->scan.inclusive(c->stream, c->plane(PILEUP_DEPTH), c->total)) || (rc = c->scan.inclusive(c->stream, c->plane(PILEUP_DEL), c->total))) return rc;
    u64 const nt = c->n_tiles();
    FLX_LAUNCH("pileup_sites", PileupDevice::sites(c->stream, 0, c->acc.as<u32>(), c->stride, c->total, c->d_starts.as<u32>(), c->n_refs(), pileup_thresholds(c->opt),
                                                   c->count.as<u32>(), nullptr));
    if ((rc = c->scan.inclusive(c->stream, c->count.as<u32>(), nt))) return rc;
    u32 last = 0;
    FLX_HIP(hipMemcpyAsync(&last, c->count.as<u32>() + (nt - 1), 4, hipMemcpyDeviceToHost, c->stream));
    FLX_HIP(hipStreamSynchronize(c->stream));
    c->n_sites = last;
    c->finished = true;
    if (c->profile)
        fprintf(stderr, "[flx pileup] finish: positions %llu sites %llu wall_ms %.3f\n", (unsigned long long)c->total, (unsigned long long)c->n_sites,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return FLX_OK;
}

extern "C" uint64_t flx_pileup_num_sites(const flx_pileup* c) {
    if (!c) return 0;
    std::lock_guard<std::mutex> g(const_cast<flx_pileup*>(c)->mu);
    return c->finished ? c->n_sites : 0;
}
extern "C" int flx_pileup_copy_sites(const flx_pileup* cc, flx_pileup_site* out, uint64_t capacity) {
    if (!finished_for_copy(cc, "flx_pileup_copy_sites", "flx_pileup_finish")) return FLX_ERR_INVALID;
    flx_pileup* const c = const_cast<flx_pileup*>(cc);
    if (capacity < c->n_sites) { set_error("flx_pileup_copy_sites: the site buffer is too small, " + std::to_string(c->n_sites) + " sites"); return FLX_ERR_CAPACITY; }
    if (c->n_sites == 0) return FLX_OK;
    if (!out) { set_error("flx_pileup_copy_sites: null argument"); return FLX_ERR_INVALID; }
    std::lock_guard<std::mutex> g(c->mu);
    auto const t0 = std::chrono::steady_clock::now();
    FLX_HIP(hipSetDevice(c->device));
    DeviceBuffer sites;                               // (made per call: as many entries as the table has sites)
    int rc;
    if ((rc = sites.ensure(c->n_sites * sizeof(flx_pileup_site), true))) return rc;
    FLX_LAUNCH("pileup_sites", PileupDevice::sites(c->stream, 1, c->acc.as<u32>(), c->stride, c->total, c->d_starts.as<u32>(), c->n_refs(), pileup_thresholds(c->opt),
                                                   c->count.as<u32>(), sites.as<flx_pileup_site>()));
    FLX_HIP(hipMemcpyAsync(out, sites.ptr, c->n_sites * sizeof(flx_pileup_site), hipMemcpyDeviceToHost, c->stream));
    FLX_HIP(hipStreamSynchronize(c->stream));
    if (c->profile)
        fprintf(stderr, "[flx pileup] copy_sites: sites %llu wall_ms %.3f\n", (unsigned long long)c->n_sites,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return FLX_OK;
}

extern "C" int flx_pileup_copy_counts(const flx_pileup* cc, uint32_t reference_id, uint64_t from, uint64_t to, uint32_t* out) {
    if (!finished_for_copy(cc, "flx_pileup_copy_counts", "flx_pileup_finish")) return FLX_ERR_INVALID;
    flx_pileup* const c = const_cast<flx_pileup*>(cc);
    if (reference_id >= c->n_refs() || from > to || to > c->starts[reference_id + 1] - c->starts[reference_id]) { set_error("flx_pileup_copy_counts: a stretch outside the sequences"); return FLX_ERR_INVALID; }
    if (from == to) return FLX_OK;
    if (!out) { set_error("flx_pileup_copy_counts: null argument"); return FLX_ERR_INVALID; }
    std::lock_guard<std::mutex> g(c->mu);
    FLX_HIP(hipSetDevice(c->device));
    for (u32 k = 0; k < PILEUP_PLANES; ++k)
        FLX_HIP(hipMemcpyAsync(out + (u64)k * (to - from), c->plane(k) + c->starts[reference_id] + from, (to - from) * 4, hipMemcpyDeviceToHost, c->stream));
    FLX_HIP(hipStreamSynchronize(c->stream));
    return FLX_OK;
}

extern "C" int flx_pileup_host(const uint64_t* ref_lens, uint32_t n_refs, const flx_pileup_options* o, const flx_record* records, uint64_t n,
                               const uint32_t* cigar_words, uint64_t n_words, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads,
                               uint32_t* counts) {
    std::vector<u64> starts;
    if (!pileup_options_valid(o) || !coverage_lengths_valid(ref_lens, n_refs, "flx_pileup_host", starts)) return FLX_ERR_INVALID;
    if (!counts || (n && !records) || !reads_given(read_pool, read_offsets, n_reads, "flx_pileup_host")) { set_error("flx_pileup_host: null argument"); return FLX_ERR_INVALID; }
    flx_pileup_options const opt = pileup_options_or_default(o);
    std::vector<PileupJob> jobs;
    if (!pileup_plan(starts, opt, records, n, cigar_words, n_words, n_reads, [&](u64 r) { return read_offsets[r + 1] - read_offsets[r]; }, "flx_pileup_host", jobs)) return FLX_ERR_INVALID;
    for (auto const& j : jobs) pileup_walk(j, cigar_words, read_pool + read_offsets[j.read_index], read_offsets[j.read_index + 1] - read_offsets[j.read_index], counts, starts.back());
    return FLX_OK;
}

extern "C" int flx_pileup_sites_host(const uint64_t* ref_lens, uint32_t n_refs, const flx_pileup_options* o, const uint32_t* counts, flx_pileup_site* out,
                                     uint64_t* n_sites) {
    std::vector<u64> starts;
    if (!pileup_options_valid(o) || !coverage_lengths_valid(ref_lens, n_refs, "flx_pileup_sites_host", starts)) return FLX_ERR_INVALID;
    if (!counts || !n_sites) { set_error("flx_pileup_sites_host: null argument"); return FLX_ERR_INVALID; }
    PileupThresholds const t = pileup_thresholds(pileup_options_or_default(o));
    u64 const total = starts.back(), capacity = *n_sites;
    u64 found = 0;
    for (u32 r = 0; r < n_refs; ++r)
        for (u64 p = starts[r]; p < starts[r + 1]; ++p) {
            u32 v[PILEUP_PLANES];
            for (u32 k = 0; k < PILEUP_PLANES; ++k) v[k] = counts[(u64)k * total + p];
            if (!pileup_is_site(v, t)) continue;
            if (found < capacity && out)
                out[found] = flx_pileup_site{(int32_t)r, (uint32_t)(p - starts[r]), v[PILEUP_DEPTH], v[PILEUP_DEL], v[PILEUP_INS], {v[PILEUP_A], v[PILEUP_C], v[PILEUP_G], v[PILEUP_T]}, 0u};
            ++found;
        }
    *n_sites = found;
    if (found > capacity) { set_error("flx_pileup_sites_host: the site buffer is too small, " + std::to_string(found) + " sites"); return FLX_ERR_CAPACITY; }
    return FLX_OK;
}
