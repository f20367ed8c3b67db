// flx_coverage: the object behind the depth-of-coverage calls of the C ABI (include/floxer_amd.h). The rule and its checks:
// flx_coverage.hpp; the kernels: flx_coverage.hip. The object owns one stream, the accumulator (a u32 per position of the concatenation
// plus one, differences until flx_coverage_finish, depths behind it) and its staging buffers. Adds judge their records without the
// object's lock and take it for the staging and the launch only, so several host threads may add at once.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>

#include "flx_coverage.hpp"
#include "flx_pipeline.hpp"

using namespace flx;

struct flx_coverage {
    int device = 0;
    flx_coverage_options opt{};
    std::vector<u64> starts;             // n_refs + 1
    u64 total = 0;
    hipStream_t stream = nullptr;
    DeviceBuffer acc, d_starts;          // total + 1 entries; the starts as u32
    DeviceBuffer jobs, words;            // an add's staging: the counted records and the words they refer to
    DeviceBuffer levels;                 // the scan's tile sums, one array per level (level_off, in entries)
    std::vector<u64> level_off;
    DeviceBuffer count_all, count_rep;   // per tile of the accumulator: heads / reported heads, scanned by finish
    DeviceBuffer chunk;                  // absorb: a piece of the other object's accumulator on this device
    PinnedBuffer pinned;                 // absorb: the same piece on its way through the host
    std::mutex mu;                       // staging, launches and `finished`
    bool finished = false;
    u64 n_heads = 0, n_runs = 0;
    bool profile = false;                // FLX_COVERAGE_PROFILE set (and not 0): every add prints its upload, its kernel's device time and its wall time to stderr
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    ~flx_coverage() {
        if (ev_a) (void)hipEventDestroy(ev_a);
        if (ev_b) (void)hipEventDestroy(ev_b);
        if (stream) (void)hipStreamDestroy(stream);
    }
    u32 n_refs() const { return (u32)(starts.size() - 1); }
};

namespace {

constexpr u64 TILE = CoverageDevice::SCAN_TILE;
constexpr u64 ABSORB_CHUNK = 4ull << 20;             // entries per piece (16 MB)

#define COV_LAUNCH(name, expr)                                                                                                     \
    do {                                                                                                                           \
        int const e__ = (expr);                                                                                                    \
        if (e__ != 0) { set_error(std::string(name) + ": launch failed: " + hipGetErrorString((hipError_t)e__)); return FLX_ERR_NO_DEVICE; } \
    } while (0)

u64 tiles_of(u64 n) { return (n + TILE - 1) / TILE; }

// inclusive prefix sum of a[0, n) in place; the tile sums of this level live in levels[level]
int scan_in_place(flx_coverage* c, u32* a, u64 n, size_t level) {
    u64 const nt = tiles_of(n);
    if (nt <= 1) { COV_LAUNCH("coverage_scan_apply", CoverageDevice::scan_apply(c->stream, a, n, nullptr)); return FLX_OK; }
    u32* const sums = c->levels.as<u32>() + c->level_off[level];
    COV_LAUNCH("coverage_scan_sums", CoverageDevice::scan_sums(c->stream, a, n, sums));
    int const rc = scan_in_place(c, sums, nt, level + 1);
    if (rc) return rc;
    COV_LAUNCH("coverage_scan_apply", CoverageDevice::scan_apply(c->stream, a, n, sums));
    return FLX_OK;
}

int create(int device, std::vector<u64>&& starts, const flx_coverage_options* o, flx_coverage** out) {
    FLX_HIP(hipSetDevice(device));
    auto c = std::make_unique<flx_coverage>();       // (an error below drops it: nothing stays allocated)
    c->device = device;
    c->opt = coverage_options_or_default(o);
    c->starts = std::move(starts);
    c->total = c->starts.back();
    if (const char* env = getenv("FLX_COVERAGE_PROFILE")) c->profile = strtol(env, nullptr, 10) != 0 || env[0] == '\0';
    FLX_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    int rc = c->acc.ensure((c->total + 1) * 4, true);
    if (rc) return rc;
    FLX_HIP(hipMemsetAsync(c->acc.ptr, 0, (c->total + 1) * 4, c->stream));
    std::vector<u32> starts32(c->starts.begin(), c->starts.end());
    if ((rc = c->d_starts.ensure(starts32.size() * 4, true))) return rc;
    FLX_HIP(hipMemcpyAsync(c->d_starts.ptr, starts32.data(), starts32.size() * 4, hipMemcpyHostToDevice, c->stream));
    u64 entries = 0;
    for (u64 nt = tiles_of(c->total); nt > 1; nt = tiles_of(nt)) { c->level_off.push_back(entries); entries += (nt + 63) / 64 * 64; }
    if (entries && (rc = c->levels.ensure(entries * 4, true))) return rc;
    u64 const nt = tiles_of(c->total);
    if ((rc = c->count_all.ensure(nt * 4, true)) || (rc = c->count_rep.ensure(nt * 4, true))) return rc;
    FLX_HIP(hipStreamSynchronize(c->stream));
    *out = c.release();
    return FLX_OK;
}

// where the words of the counted records lie in the pool that goes up: every word once, however many records refer to it
void compact_words(std::vector<CoverageJob>& jobs, const uint32_t* cigar_words, std::vector<u32>& pool) {
    struct Segment { u64 from, to, base; };
    std::vector<std::pair<u64, u64>> spans;
    spans.reserve(jobs.size());
    for (auto const& j : jobs) spans.emplace_back(j.word_off, j.word_off + j.n_words);
    std::sort(spans.begin(), spans.end());
    std::vector<Segment> segments;
    for (auto const& s : spans) {
        if (!segments.empty() && s.first <= segments.back().to) segments.back().to = std::max(segments.back().to, s.second);
        else segments.push_back(Segment{s.first, s.second, 0});
    }
    u64 used = 0;
    for (auto& s : segments) { s.base = used; used += s.to - s.from; }
    pool.resize(used);
    for (auto const& s : segments) memcpy(pool.data() + s.base, cigar_words + s.from, (s.to - s.from) * 4);
    for (auto& j : jobs) {
        auto it = std::upper_bound(segments.begin(), segments.end(), j.word_off, [](u64 off, Segment const& s) { return off < s.from; });
        Segment const& s = *(it - 1);
        j.word_off = s.base + (j.word_off - s.from);
    }
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
    if (c->profile) {
        if (!c->ev_a) { FLX_HIP(hipEventCreate(&c->ev_a)); FLX_HIP(hipEventCreate(&c->ev_b)); }
        FLX_HIP(hipEventRecord(c->ev_a, c->stream));
    }
    COV_LAUNCH("coverage_add", CoverageDevice::add(c->stream, c->jobs.as<CoverageJob>(), (u32)jobs.size(), c->words.as<u32>(), c->acc.as<u32>(), c->opt.count_deletions));
    if (c->profile) FLX_HIP(hipEventRecord(c->ev_b, c->stream));
    FLX_HIP(hipStreamSynchronize(c->stream));           // (the staging buffers are free for the next add)
    if (c->profile) {
        float ms = 0;
        FLX_HIP(hipEventElapsedTime(&ms, c->ev_a, c->ev_b));
        double const wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[flx coverage] add: records %zu words %zu upload_bytes %zu coverage_add_ms %.3f wall_ms_behind_the_checks %.3f\n", jobs.size(), pool.size(),
                jobs.size() * sizeof(CoverageJob) + pool.size() * 4, (double)ms, wall);
    }
    return FLX_OK;
}

bool finished_for_copy(const flx_coverage* c, const char* who) {
    if (!c) { set_error(std::string(who) + ": null argument"); return false; }
    std::lock_guard<std::mutex> g(const_cast<flx_coverage*>(c)->mu);
    if (!c->finished) { set_error(std::string(who) + ": call flx_coverage_finish first"); return false; }
    return true;
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
extern "C" void flx_coverage_free(flx_coverage* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

extern "C" int flx_coverage_add_records(flx_coverage* c, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words) {
    if (!c || (n && !records)) { set_error("flx_coverage_add_records: null argument"); return FLX_ERR_INVALID; }
    std::vector<CoverageJob> jobs;
    if (!coverage_plan(c->starts, c->opt, records, n, cigar_words, n_words, "flx_coverage_add_records", jobs)) return FLX_ERR_INVALID;
    return commit(c, jobs, cigar_words, "flx_coverage_add_records");
}
extern "C" int flx_coverage_add_run(flx_coverage* c, const flx_run* run) {
    if (!c || !run) { set_error("flx_coverage_add_run: null argument"); return FLX_ERR_INVALID; }
    if (c->opt.min_mapq > 0 && !run->has_mapq) { set_error("flx_coverage_add_run: min_mapq needs a run made with flx_output_options.mapq"); return FLX_ERR_INVALID; }
    // a run is its own records plus its per-lane parts, each over its own word pool: all are judged before any is added
    std::vector<const flx_run*> pieces{run};
    for (auto const& p : run->parts) pieces.push_back(&p);
    // (the parts are independent: each is judged by a thread of its own, up to eight at a time; the first refusal in part order is reported)
    std::vector<std::vector<CoverageJob>> jobs(pieces.size());
    std::vector<std::string> refusals(pieces.size());
    std::vector<char> refused(pieces.size(), 0);
    auto judge = [&](size_t i) {
        if (!coverage_plan(c->starts, c->opt, pieces[i]->records.data(), pieces[i]->records.size(), pieces[i]->cigars.data(), pieces[i]->cigars.size(), "flx_coverage_add_run", jobs[i])) {
            refused[i] = 1;
            refusals[i] = flx_last_error();      // (the message is the judging thread's own)
        }
    };
    size_t const n_threads = std::min<size_t>(8, pieces.size());
    if (n_threads <= 1) for (size_t i = 0; i < pieces.size(); ++i) judge(i);
    else {
        std::vector<std::thread> threads;
        for (size_t t = 0; t < n_threads; ++t)
            threads.emplace_back([&, t] { for (size_t i = t; i < pieces.size(); i += n_threads) judge(i); });
        for (auto& t : threads) t.join();
    }
    for (size_t i = 0; i < pieces.size(); ++i)
        if (refused[i]) { set_error(refusals[i]); return FLX_ERR_INVALID; }
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
    u64 const n = into->total + 1, piece = std::min(n, ABSORB_CHUNK);
    FLX_HIP(hipSetDevice(into->device));
    int rc;
    if ((rc = into->pinned.ensure(piece * 4)) || (rc = into->chunk.ensure(piece * 4, true))) return rc;
    for (u64 at = 0; at < n; at += piece) {
        u64 const m = std::min(piece, n - at);
        FLX_HIP(hipSetDevice(from->device));
        FLX_HIP(hipMemcpyAsync(into->pinned.ptr, from->acc.as<u32>() + at, m * 4, hipMemcpyDeviceToHost, from->stream));
        FLX_HIP(hipStreamSynchronize(from->stream));
        FLX_HIP(hipSetDevice(into->device));
        FLX_HIP(hipMemcpyAsync(into->chunk.ptr, into->pinned.ptr, m * 4, hipMemcpyHostToDevice, into->stream));
        COV_LAUNCH("coverage_sum", CoverageDevice::sum(into->stream, into->acc.as<u32>() + at, into->chunk.as<u32>(), m));
        FLX_HIP(hipStreamSynchronize(into->stream));    // (the piece's buffers are free again)
    }
    FLX_HIP(hipSetDevice(from->device));
    FLX_HIP(hipMemsetAsync(from->acc.ptr, 0, n * 4, from->stream));
    FLX_HIP(hipStreamSynchronize(from->stream));
    return FLX_OK;
}

extern "C" int flx_coverage_finish(flx_coverage* c) {
    if (!c) { set_error("flx_coverage_finish: null argument"); return FLX_ERR_INVALID; }
    std::lock_guard<std::mutex> g(c->mu);
    if (c->finished) { set_error("flx_coverage_finish: the coverage object is finished"); return FLX_ERR_INVALID; }
    FLX_HIP(hipSetDevice(c->device));
    int rc = scan_in_place(c, c->acc.as<u32>(), c->total, 0);
    if (rc) return rc;
    u64 const nt = tiles_of(c->total);
    COV_LAUNCH("coverage_heads", CoverageDevice::heads(c->stream, 0, c->acc.as<u32>(), c->total, c->d_starts.as<u32>(), c->n_refs(), c->opt.report_zero,
                                                      c->count_all.as<u32>(), c->count_rep.as<u32>(), nullptr, 0, nullptr));
    if ((rc = scan_in_place(c, c->count_all.as<u32>(), nt, 1)) || (rc = scan_in_place(c, c->count_rep.as<u32>(), nt, 1))) return rc;
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
    if (!finished_for_copy(cc, "flx_coverage_copy_runs")) return FLX_ERR_INVALID;
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
        COV_LAUNCH("coverage_heads", CoverageDevice::heads(c->stream, mode, c->acc.as<u32>(), c->total, c->d_starts.as<u32>(), c->n_refs(), c->opt.report_zero,
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
    if (!finished_for_copy(c, "flx_coverage_copy_windows")) return FLX_ERR_INVALID;
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
        COV_LAUNCH("coverage_windows", CoverageDevice::windows(c->stream, c->acc.as<u32>(), c->total, c->d_starts.as<u32>(), c->n_refs(), window, d_bases.as<u64>(), d_acc.as<CoverageWindowAcc>()));
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
    if (!finished_for_copy(cc, "flx_coverage_copy_depth")) return FLX_ERR_INVALID;
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
    out[0] = CoverageDevice::SCAN_TILE;
    out[1] = CoverageDevice::SCAN_TILE;
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
