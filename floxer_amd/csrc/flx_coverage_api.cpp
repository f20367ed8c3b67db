// flx_coverage: the object behind the depth-of-coverage calls of the C ABI (include/floxer_amd.h). The rule and its checks:
// flx_coverage.hpp; the kernels: flx_coverage.hip, the scan and the sum: flx_scan.hip; what it shares with the other side objects:
// flx_object.hpp. The object owns one stream, the accumulator (a u32 per position of the concatenation plus one, differences until
// flx_coverage_finish, depths behind it) and its staging buffers. Adds judge their records without the object's lock and take it for the
// staging and the launch only, so several host threads may add at once.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <memory>
#include <mutex>

#include "flx_coverage.hpp"
#include "flx_object.hpp"

using namespace flx;

struct flx_coverage : PlaneObject {      // acc: total + 1 entries; FLX_COVERAGE_PROFILE: every add prints its upload, its kernel's device time and its wall time
    flx_coverage_options opt{};
    DeviceBuffer jobs, words;            // an add's staging: the counted records and the words they refer to
    DeviceBuffer count_all, count_rep;   // per tile of the accumulator: heads / reported heads, scanned by finish
    u64 n_heads = 0, n_runs = 0;
};

namespace {

int create(int device, std::vector<u64>&& starts, const flx_coverage_options* o, flx_coverage** out) {
    auto c = std::make_unique<flx_coverage>();       // (an error below drops it: nothing stays allocated)
    c->opt = coverage_options_or_default(o);
    u64 const entries = starts.back() + 1;
    int const rc = c->create(device, "FLX_COVERAGE_PROFILE", std::move(starts), entries, {&c->count_all, &c->count_rep});
    if (rc) return rc;
    *out = c.release();
    return FLX_OK;
}

// the judged jobs of one word pool: staged and launched under the object's lock
int commit(flx_coverage* c, std::vector<CoverageJob>& jobs, const uint32_t* cigar_words, const char* who) {
    if (jobs.size() >= (1ull << 32)) { set_error(std::string(who) + ": too many records in one call"); return FLX_ERR_INVALID; }
    auto const t0 = std::chrono::steady_clock::now();
    std::vector<u32> pool;
    if (!jobs.empty()) compact_words(jobs, cigar_words, pool);
    std::lock_guard<std::mutex> g(c->mu);
    if (c->finished) { set_error(std::string(who) + ": the coverage object is finished"); return FLX_ERR_INVALID; }
    if (jobs.empty()) return FLX_OK;
    FLX_HIP(hipSetDevice(c->device));
    int rc;
    if ((rc = c->jobs.ensure(jobs.size() * sizeof(CoverageJob))) || (rc = c->words.ensure(pool.size() * 4))) return rc;
    FLX_HIP(hipMemcpyAsync(c->jobs.ptr, jobs.data(), jobs.size() * sizeof(CoverageJob), hipMemcpyHostToDevice, c->stream));
    FLX_HIP(hipMemcpyAsync(c->words.ptr, pool.data(), pool.size() * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = c->span_begin())) return rc;
    FLX_LAUNCH("coverage_add", CoverageDevice::add(c->stream, c->jobs.as<CoverageJob>(), (u32)jobs.size(), c->words.as<u32>(), c->acc.as<u32>(), c->opt.count_deletions));
    if ((rc = c->span_end())) return rc;
    FLX_HIP(hipStreamSynchronize(c->stream));           // (the staging buffers are free for the next add)
    if (c->profile) {
        float ms;
        if ((rc = c->span_ms(ms))) return rc;
        double const wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[flx coverage] add: records %zu words %zu upload_bytes %zu coverage_add_ms %.3f wall_ms_behind_the_checks %.3f\n", jobs.size(), pool.size(),
                jobs.size() * sizeof(CoverageJob) + pool.size() * 4, (double)ms, wall);
    }
    return FLX_OK;
}

}  // namespace

extern "C" int flx_coverage_create_for_lengths(int hip_device, const uint64_t* ref_lens, uint32_t n_refs, const flx_coverage_options* o, flx_coverage** out) {
    if (!out) { set_error("flx_coverage_create_for_lengths: null argument"); return FLX_ERR_INVALID; }
    std::vector<u64> starts;
    if (!coverage_options_valid(o) || !coverage_lengths_valid(ref_lens, n_refs, "flx_coverage_create_for_lengths", starts)) return FLX_ERR_INVALID;
    return create(hip_device, std::move(starts), o, out);
}
extern "C" int flx_coverage_create(flx_ctx* ctx, const flx_coverage_options* o, flx_coverage** out) {
    if (!ctx || !ctx->hidx || !out) { set_error("flx_coverage_create: null argument"); return FLX_ERR_INVALID; }
    std::vector<u64> starts;
    if (!coverage_options_valid(o) || !coverage_lengths_valid(ctx->hidx->seq_len.data(), (uint32_t)ctx->hidx->seq_len.size(), "flx_coverage_create", starts)) return FLX_ERR_INVALID;
    return create(ctx->device, std::move(starts), o, out);
}
extern "C" void flx_coverage_free(flx_coverage* c) { free_object(c); }

extern "C" int flx_coverage_add_records(flx_coverage* c, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words) {
    if (!c || (n && !records)) { set_error("flx_coverage_add_records: null argument"); return FLX_ERR_INVALID; }
    std::vector<CoverageJob> jobs;
    if (!coverage_plan(c->starts, c->opt, records, n, cigar_words, n_words, "flx_coverage_add_records", jobs)) return FLX_ERR_INVALID;
    return commit(c, jobs, cigar_words, "flx_coverage_add_records");
}
extern "C" int flx_coverage_add_run(flx_coverage* c, const flx_run* run) {
    if (!c || !run) { set_error("flx_coverage_add_run: null argument"); return FLX_ERR_INVALID; }
    if (c->opt.min_mapq > 0 && !run->has_mapq) { set_error("flx_coverage_add_run: min_mapq needs a run made with flx_output_options.mapq"); return FLX_ERR_INVALID; }
    // all pieces are judged before any is added
    auto const pieces = run_pieces(run);
    std::vector<std::vector<CoverageJob>> jobs(pieces.size());
    if (!judge_in_parallel(pieces.size(), [&](size_t i) {
            return coverage_plan(c->starts, c->opt, pieces[i]->records.data(), pieces[i]->records.size(), pieces[i]->cigars.data(), pieces[i]->cigars.size(), "flx_coverage_add_run", jobs[i]);
        }))
        return FLX_ERR_INVALID;
    for (size_t i = 0; i < pieces.size(); ++i) {
        int const rc = commit(c, jobs[i], pieces[i]->cigars.data(), "flx_coverage_add_run");
        if (rc) return rc;
    }
    return FLX_OK;
}

extern "C" int flx_coverage_absorb(flx_coverage* into, flx_coverage* from) {
    if (!into || !from || into == from) { set_error("flx_coverage_absorb: null argument, or an object absorbed into itself"); return FLX_ERR_INVALID; }
    std::lock(into->mu, from->mu);
    std::lock_guard<std::mutex> g1(into->mu, std::adopt_lock), g2(from->mu, std::adopt_lock);
    if (into->finished || from->finished) { set_error("flx_coverage_absorb: a coverage object is finished"); return FLX_ERR_INVALID; }
    if (into->starts != from->starts) { set_error("flx_coverage_absorb: the objects belong to different reference lengths"); return FLX_ERR_INVALID; }
    if (!coverage_options_equal(into->opt, from->opt)) { set_error("flx_coverage_absorb: the objects have different options"); return FLX_ERR_INVALID; }
    int const rc = absorb_plane(into, from, into->acc.as<u32>(), from->acc.as<u32>(), into->total + 1);
    return rc ? rc : from->clear();
}

extern "C" int flx_coverage_finish(flx_coverage* c) {
    if (!c) { set_error("flx_coverage_finish: null argument"); return FLX_ERR_INVALID; }
    std::lock_guard<std::mutex> g(c->mu);
    if (c->finished) { set_error("flx_coverage_finish: the coverage object is finished"); return FLX_ERR_INVALID; }
    FLX_HIP(hipSetDevice(c->device));
    int rc = c->scan.inclusive(c->stream, c->acc.as<u32>(), c->total);
    if (rc) return rc;
    u64 const nt = c->n_tiles();
    FLX_LAUNCH("coverage_heads", CoverageDevice::heads(c->stream, 0, c->acc.as<u32>(), c->total, c->d_starts.as<u32>(), c->n_refs(), c->opt.report_zero,
                                                       c->count_all.as<u32>(), c->count_rep.as<u32>(), nullptr, 0, nullptr));
    if ((rc = c->scan.inclusive(c->stream, c->count_all.as<u32>(), nt)) || (rc = c->scan.inclusive(c->stream, c->count_rep.as<u32>(), nt))) return rc;
    u32 last[2] = {0, 0};
    FLX_HIP(hipMemcpyAsync(&last[0], c->count_all.as<u32>() + (nt - 1), 4, hipMemcpyDeviceToHost, c->stream));
    FLX_HIP(hipMemcpyAsync(&last[1], c->count_rep.as<u32>() + (nt - 1), 4, hipMemcpyDeviceToHost, c->stream));
    FLX_HIP(hipStreamSynchronize(c->stream));
    c->n_heads = last[0];
    c->n_runs = last[1];
    c->finished = true;
    return FLX_OK;
}

extern "C" uint64_t flx_coverage_num_runs(const flx_coverage* c) {
    if (!c) return 0;
    std::lock_guard<std::mutex> g(const_cast<flx_coverage*>(c)->mu);
    return c->finished ? c->n_runs : 0;
}
extern "C" int flx_coverage_copy_runs(const flx_coverage* cc, flx_depth_run* out, uint64_t capacity) {
    if (!finished_for_copy(cc, "flx_coverage_copy_runs", "flx_coverage_finish")) return FLX_ERR_INVALID;
    flx_coverage* const c = const_cast<flx_coverage*>(cc);
    if (capacity < c->n_runs) { set_error("flx_coverage_copy_runs: the run buffer is too small, " + std::to_string(c->n_runs) + " runs"); return FLX_ERR_CAPACITY; }
    if (c->n_runs == 0) return FLX_OK;
    if (!out) { set_error("flx_coverage_copy_runs: null argument"); return FLX_ERR_INVALID; }
    std::lock_guard<std::mutex> g(c->mu);
    FLX_HIP(hipSetDevice(c->device));
    DeviceBuffer heads, runs;                         // (made per call: as many entries as the track has heads)
    int rc;
    if ((rc = heads.ensure(c->n_heads * 4, true)) || (rc = runs.ensure(c->n_runs * sizeof(flx_depth_run), true))) return rc;
    for (int mode = 1; mode <= 2; ++mode)
        FLX_LAUNCH("coverage_heads", CoverageDevice::heads(c->stream, mode, c->acc.as<u32>(), c->total, c->d_starts.as<u32>(), c->n_refs(), c->opt.report_zero,
                                                          c->count_all.as<u32>(), c->count_rep.as<u32>(), heads.as<u32>(), c->n_heads, runs.as<flx_depth_run>()));
    FLX_HIP(hipMemcpyAsync(out, runs.ptr, c->n_runs * sizeof(flx_depth_run), hipMemcpyDeviceToHost, c->stream));
    FLX_HIP(hipStreamSynchronize(c->stream));
    return FLX_OK;
}

extern "C" uint64_t flx_coverage_num_windows(const flx_coverage* c, uint64_t window) {
    if (!c) return 0;
    std::vector<u64> bases;
    coverage_window_bases(c->starts, window, bases);
    return bases.back();
}
extern "C" int flx_coverage_copy_windows(flx_coverage* c, uint64_t window, flx_depth_window* out, uint64_t capacity) {
    if (!finished_for_copy(c, "flx_coverage_copy_windows", "flx_coverage_finish")) return FLX_ERR_INVALID;
    if (window >= COVERAGE_MAX_TOTAL) window = 0;
    std::vector<u64> bases;
    coverage_window_bases(c->starts, window, bases);
    u64 const n = bases.back();
    if (capacity < n) { set_error("flx_coverage_copy_windows: the window buffer is too small, " + std::to_string(n) + " windows"); return FLX_ERR_CAPACITY; }
    if (!out) { set_error("flx_coverage_copy_windows: null argument"); return FLX_ERR_INVALID; }
    std::vector<CoverageWindowAcc> acc(n);
    {
        std::lock_guard<std::mutex> g(c->mu);
        FLX_HIP(hipSetDevice(c->device));
        DeviceBuffer d_bases, d_acc;
        int rc;
        if ((rc = d_bases.ensure(bases.size() * 8, true)) || (rc = d_acc.ensure(n * sizeof(CoverageWindowAcc), true))) return rc;
        FLX_HIP(hipMemcpyAsync(d_bases.ptr, bases.data(), bases.size() * 8, hipMemcpyHostToDevice, c->stream));
        FLX_HIP(hipMemsetAsync(d_acc.ptr, 0, n * sizeof(CoverageWindowAcc), c->stream));
        FLX_LAUNCH("coverage_windows", CoverageDevice::windows(c->stream, c->acc.as<u32>(), c->total, c->d_starts.as<u32>(), c->n_refs(), window, d_bases.as<u64>(), d_acc.as<CoverageWindowAcc>()));
        FLX_HIP(hipMemcpyAsync(acc.data(), d_acc.ptr, n * sizeof(CoverageWindowAcc), hipMemcpyDeviceToHost, c->stream));
        FLX_HIP(hipStreamSynchronize(c->stream));
    }
    for (size_t r = 0; r + 1 < c->starts.size(); ++r) {
        u64 const len = c->starts[r + 1] - c->starts[r], w = window == 0 ? len : window;
        for (u64 k = 0; k < bases[r + 1] - bases[r]; ++k) {
            CoverageWindowAcc const& a = acc[bases[r] + k];
            out[bases[r] + k] = flx_depth_window{(int32_t)r, a.max_depth, k * w, std::min((k + 1) * w, len), a.depth_sum, a.covered};
        }
    }
    return FLX_OK;
}

extern "C" int flx_coverage_copy_depth(const flx_coverage* cc, uint32_t reference_id, uint64_t from, uint64_t to, uint32_t* out) {
    if (!finished_for_copy(cc, "flx_coverage_copy_depth", "flx_coverage_finish")) return FLX_ERR_INVALID;
    flx_coverage* const c = const_cast<flx_coverage*>(cc);
    if (reference_id >= c->n_refs() || from > to || to > c->starts[reference_id + 1] - c->starts[reference_id]) { set_error("flx_coverage_copy_depth: a stretch outside the sequences"); return FLX_ERR_INVALID; }
    if (from == to) return FLX_OK;
    if (!out) { set_error("flx_coverage_copy_depth: null argument"); return FLX_ERR_INVALID; }
    std::lock_guard<std::mutex> g(c->mu);
    FLX_HIP(hipSetDevice(c->device));
    FLX_HIP(hipMemcpyAsync(out, c->acc.as<u32>() + c->starts[reference_id] + from, (to - from) * 4, hipMemcpyDeviceToHost, c->stream));
    FLX_HIP(hipStreamSynchronize(c->stream));
    return FLX_OK;
}

extern "C" int flx_coverage_geometry(uint32_t out[2]) {
    if (!out) { set_error("flx_coverage_geometry: null argument"); return FLX_ERR_INVALID; }
    out[0] = ScanDevice::SCAN_TILE;
    out[1] = ScanDevice::SCAN_TILE;
    return FLX_OK;
}

extern "C" int flx_coverage_host(const uint64_t* ref_lens, uint32_t n_refs, const flx_coverage_options* o, const flx_record* records, uint64_t n,
                                 const uint32_t* cigar_words, uint64_t n_words, uint32_t* depth) {
    std::vector<u64> starts;
    if (!coverage_options_valid(o) || !coverage_lengths_valid(ref_lens, n_refs, "flx_coverage_host", starts)) return FLX_ERR_INVALID;
    if (!depth || (n && !records)) { set_error("flx_coverage_host: null argument"); return FLX_ERR_INVALID; }
    flx_coverage_options const opt = coverage_options_or_default(o);
    std::vector<CoverageJob> jobs;
    if (!coverage_plan(starts, opt, records, n, cigar_words, n_words, "flx_coverage_host", jobs)) return FLX_ERR_INVALID;
    for (auto const& j : jobs) coverage_walk(j, cigar_words, opt.count_deletions != 0, depth);
    return FLX_OK;
}
