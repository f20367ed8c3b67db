// flx_pileup: the object behind the allele-pileup calls of the C ABI (include/floxer_amd.h). The rule and its checks: flx_pileup.hpp; the
// kernels: flx_pileup.hip, and coverage's scan and sum launches (flx_coverage.hip). The object owns one stream, the accumulator (seven
// planes of u32 over the concatenation; DEPTH and DEL are differences until flx_pileup_finish) and its staging buffers. Adds judge their
// records and stage their words and letters without the object's lock and take it for the upload and the launch only, so several host
// threads may add at once.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>

#include "flx_pileup.hpp"
#include "flx_pipeline.hpp"

using namespace flx;

struct flx_pileup {
    int device = 0;
    flx_pileup_options opt{};
    std::vector<u64> starts;             // n_refs + 1
    u64 total = 0, stride = 0;           // entries per plane: total + 1 rounded up to 64 (every plane starts 256-byte aligned)
    hipStream_t stream = nullptr;
    DeviceBuffer acc, d_starts;          // PILEUP_PLANES * stride entries; the starts as u32
    DeviceBuffer jobs, words, letters;   // an add's staging: the counted records, the words and the oriented sequences they refer to
    DeviceBuffer levels;                 // the scan's tile sums, one array per level (level_off, in entries)
    std::vector<u64> level_off;
    DeviceBuffer count;                  // per tile of the accumulator: its sites, scanned by finish
    DeviceBuffer chunk;                  // absorb: a piece of the other object's accumulator on this device
    PinnedBuffer pinned;                 // absorb: the same piece on its way through the host
    std::mutex mu;                       // staging buffers, launches and `finished`
    bool finished = false;
    u64 n_sites = 0;
    bool profile = false;                // FLX_PILEUP_PROFILE set (and not 0): every add prints its upload, its kernel's device time and its wall time to stderr
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    ~flx_pileup() {
        if (ev_a) (void)hipEventDestroy(ev_a);
        if (ev_b) (void)hipEventDestroy(ev_b);
        if (stream) (void)hipStreamDestroy(stream);
    }
    u32 n_refs() const { return (u32)(starts.size() - 1); }
    u32* plane(u32 k) const { return acc.as<u32>() + (u64)k * stride; }
};

namespace {

constexpr u64 TILE = CoverageDevice::SCAN_TILE;
constexpr u64 ABSORB_CHUNK = 4ull << 20;             // entries per piece (16 MB)

#define PILEUP_LAUNCH(name, expr)                                                                                                  \
    do {                                                                                                                           \
        int const e__ = (expr);                                                                                                    \
        if (e__ != 0) { set_error(std::string(name) + ": launch failed: " + hipGetErrorString((hipError_t)e__)); return FLX_ERR_NO_DEVICE; } \
    } while (0)

u64 tiles_of(u64 n) { return (n + TILE - 1) / TILE; }

// inclusive prefix sum of a[0, n) in place with coverage's launches; the tile sums of this level live in levels[level]
int scan_in_place(flx_pileup* c, u32* a, u64 n, size_t level) {
    u64 const nt = tiles_of(n);
    if (nt <= 1) { PILEUP_LAUNCH("coverage_scan_apply", CoverageDevice::scan_apply(c->stream, a, n, nullptr)); return FLX_OK; }
    u32* const sums = c->levels.as<u32>() + c->level_off[level];
    PILEUP_LAUNCH("coverage_scan_sums", CoverageDevice::scan_sums(c->stream, a, n, sums));
    int const rc = scan_in_place(c, sums, nt, level + 1);
    if (rc) return rc;
    PILEUP_LAUNCH("coverage_scan_apply", CoverageDevice::scan_apply(c->stream, a, n, sums));
    return FLX_OK;
}

int create(int device, std::vector<u64>&& starts, const flx_pileup_options* o, flx_pileup** out) {
    FLX_HIP(hipSetDevice(device));
    auto c = std::make_unique<flx_pileup>();         // (an error below drops it: nothing stays allocated)
    c->device = device;
    c->opt = pileup_options_or_default(o);
    c->starts = std::move(starts);
    c->total = c->starts.back();
    c->stride = (c->total + 1 + 63) / 64 * 64;
    if (const char* env = getenv("FLX_PILEUP_PROFILE")) c->profile = strtol(env, nullptr, 10) != 0 || env[0] == '\0';
    FLX_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    size_t const bytes = (size_t)PILEUP_PLANES * c->stride * 4;
    int rc = c->acc.ensure(bytes, true);
    if (rc) return rc;
    FLX_HIP(hipMemsetAsync(c->acc.ptr, 0, bytes, c->stream));
    std::vector<u32> starts32(c->starts.begin(), c->starts.end());
    if ((rc = c->d_starts.ensure(starts32.size() * 4, true))) return rc;
    FLX_HIP(hipMemcpyAsync(c->d_starts.ptr, starts32.data(), starts32.size() * 4, hipMemcpyHostToDevice, c->stream));
    u64 entries = 0;
    for (u64 nt = tiles_of(c->total); nt > 1; nt = tiles_of(nt)) { c->level_off.push_back(entries); entries += (nt + 63) / 64 * 64; }
    if (entries && (rc = c->levels.ensure(entries * 4, true))) return rc;
    if ((rc = c->count.ensure(tiles_of(c->total) * 4, true))) return rc;
    FLX_HIP(hipStreamSynchronize(c->stream));
    *out = c.release();
    return FLX_OK;
}

// where the words of the counted records lie in the pool that goes up: every word once, however many records refer to it
void compact_words(std::vector<PileupJob>& jobs, const uint32_t* cigar_words, std::vector<u32>& pool) {
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

// Where the letters of the reads come from: the caller's rank pool (forward sequences: a reverse complement is made here with the
// rank routine) or a batch's host copy (both orientations, flx_reads::pool).
struct Letters {
    const uint8_t* read_pool = nullptr;
    const uint64_t* read_offsets = nullptr;
    const flx_reads* batch = nullptr;
    uint64_t n_reads = 0;
    u64 length(u64 i) const { return batch ? batch->lens[i] : read_offsets[i + 1] - read_offsets[i]; }
    void oriented(u64 i, bool reverse, u8* out) const {
        u64 const len = length(i);
        if (batch) memcpy(out, batch->pool.data() + batch->pool_off[i] + (reverse ? len : 0), len);
        else if (reverse) reverse_complement(read_pool + read_offsets[i], len, out);
        else memcpy(out, read_pool + read_offsets[i], len);
    }
};

// the oriented sequences the jobs refer to, each once per orientation used, and every job's seq_off into them
void stage_letters(std::vector<PileupJob>& jobs, Letters const& src, std::vector<u8>& pool) {
    std::vector<u64> keys;
    keys.reserve(jobs.size());
    for (auto const& j : jobs) keys.push_back(j.read_index * 2 + j.reverse);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    std::vector<u64> off(keys.size() + 1, 0);
    for (size_t k = 0; k < keys.size(); ++k) off[k + 1] = off[k] + src.length(keys[k] >> 1);
    pool.resize(off.back());
    for (size_t k = 0; k < keys.size(); ++k) src.oriented(keys[k] >> 1, (keys[k] & 1) != 0, pool.data() + off[k]);
    for (auto& j : jobs) j.seq_off = off[(size_t)(std::lower_bound(keys.begin(), keys.end(), j.read_index * 2 + j.reverse) - keys.begin())];
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
    if (c->profile) {
        if (!c->ev_a) { FLX_HIP(hipEventCreate(&c->ev_a)); FLX_HIP(hipEventCreate(&c->ev_b)); }
        FLX_HIP(hipEventRecord(c->ev_a, c->stream));
    }
    PILEUP_LAUNCH("pileup_add", PileupDevice::add(c->stream, c->jobs.as<PileupJob>(), (u32)jobs.size(), c->words.as<u32>(),
                                                  resident ? resident->d_pool.as<u8>() : c->letters.as<u8>(), c->acc.as<u32>(), c->stride));
    if (c->profile) FLX_HIP(hipEventRecord(c->ev_b, c->stream));
    FLX_HIP(hipStreamSynchronize(c->stream));           // (the staging buffers are free for the next add)
    if (c->profile) {
        float ms = 0;
        FLX_HIP(hipEventElapsedTime(&ms, c->ev_a, c->ev_b));
        double const wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[flx pileup] add: records %zu words %zu letters %zu upload_bytes %zu pileup_add_ms %.3f wall_ms_behind_the_checks %.3f\n", jobs.size(), pool.size(),
                letters.size(), jobs.size() * sizeof(PileupJob) + pool.size() * 4 + letters.size(), (double)ms, wall);
    }
    return FLX_OK;
}

bool finished_for_copy(const flx_pileup* c, const char* who) {
    if (!c) { set_error(std::string(who) + ": null argument"); return false; }
    std::lock_guard<std::mutex> g(const_cast<flx_pileup*>(c)->mu);
    if (!c->finished) { set_error(std::string(who) + ": call flx_pileup_finish first"); return false; }
    return true;
}

// a run is its own records plus its per-lane parts, each over its own word pool: all are judged before any is added
int add_run(flx_pileup* c, const flx_run* run, Letters const& src, const flx_reads* resident, const char* who) {
    if (c->opt.min_mapq > 0 && !run->has_mapq) { set_error(std::string(who) + ": min_mapq needs a run made with flx_output_options.mapq"); return FLX_ERR_INVALID; }
    std::vector<const flx_run*> pieces{run};
    for (auto const& p : run->parts) pieces.push_back(&p);
    // (the parts are independent: each is judged by a thread of its own, up to eight at a time; the first refusal in part order is reported)
    std::vector<std::vector<PileupJob>> jobs(pieces.size());
    std::vector<std::string> refusals(pieces.size());
    std::vector<char> refused(pieces.size(), 0);
    auto judge = [&](size_t i) {
        if (!pileup_plan(c->starts, c->opt, pieces[i]->records.data(), pieces[i]->records.size(), pieces[i]->cigars.data(), pieces[i]->cigars.size(), src.n_reads,
                         [&](u64 r) { return src.length(r); }, who, jobs[i])) {
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
extern "C" void flx_pileup_free(flx_pileup* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

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
    u64 const n = into->total + 1, piece = std::min(n, ABSORB_CHUNK);
    FLX_HIP(hipSetDevice(into->device));
    int rc;
    if ((rc = into->pinned.ensure(piece * 4)) || (rc = into->chunk.ensure(piece * 4, true))) return rc;
    for (u32 k = 0; k < PILEUP_PLANES; ++k)
        for (u64 at = 0; at < n; at += piece) {
            u64 const m = std::min(piece, n - at);
            FLX_HIP(hipSetDevice(from->device));
            FLX_HIP(hipMemcpyAsync(into->pinned.ptr, from->plane(k) + at, m * 4, hipMemcpyDeviceToHost, from->stream));
            FLX_HIP(hipStreamSynchronize(from->stream));
            FLX_HIP(hipSetDevice(into->device));
            FLX_HIP(hipMemcpyAsync(into->chunk.ptr, into->pinned.ptr, m * 4, hipMemcpyHostToDevice, into->stream));
            PILEUP_LAUNCH("coverage_sum", CoverageDevice::sum(into->stream, into->plane(k) + at, into->chunk.as<u32>(), m));
            FLX_HIP(hipStreamSynchronize(into->stream));    // (the piece's buffers are free again)
        }
    FLX_HIP(hipSetDevice(from->device));
    FLX_HIP(hipMemsetAsync(from->acc.ptr, 0, (size_t)PILEUP_PLANES * from->stride * 4, from->stream));
    FLX_HIP(hipStreamSynchronize(from->stream));
    return FLX_OK;
}

extern "C" int flx_pileup_finish(flx_pileup* c) {
    if (!c) { set_error("flx_pileup_finish: null argument"); return FLX_ERR_INVALID; }
    std::lock_guard<std::mutex> g(c->mu);
    if (c->finished) { set_error("flx_pileup_finish: the pileup object is finished"); return FLX_ERR_INVALID; }
    auto const t0 = std::chrono::steady_clock::now();
    FLX_HIP(hipSetDevice(c->device));
    int rc;
    if ((rc = scan_in_place(c, c->plane(PILEUP_DEPTH), c->total, 0)) || (rc = scan_in_place(c, c->plane(PILEUP_DEL), c->total, 0))) return rc;
    u64 const nt = tiles_of(c->total);
    PILEUP_LAUNCH("pileup_sites", PileupDevice::sites(c->stream, 0, c->acc.as<u32>(), c->stride, c->total, c->d_starts.as<u32>(), c->n_refs(), pileup_thresholds(c->opt),
                                                      c->count.as<u32>(), nullptr));
    if ((rc = scan_in_place(c, c->count.as<u32>(), nt, 1))) return rc;
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
    if (!finished_for_copy(cc, "flx_pileup_copy_sites")) return FLX_ERR_INVALID;
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
    PILEUP_LAUNCH("pileup_sites", PileupDevice::sites(c->stream, 1, c->acc.as<u32>(), c->stride, c->total, c->d_starts.as<u32>(), c->n_refs(), pileup_thresholds(c->opt),
                                                      c->count.as<u32>(), sites.as<flx_pileup_site>()));
    FLX_HIP(hipMemcpyAsync(out, sites.ptr, c->n_sites * sizeof(flx_pileup_site), hipMemcpyDeviceToHost, c->stream));
    FLX_HIP(hipStreamSynchronize(c->stream));
    if (c->profile)
        fprintf(stderr, "[flx pileup] copy_sites: sites %llu wall_ms %.3f\n", (unsigned long long)c->n_sites,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return FLX_OK;
}

extern "C" int flx_pileup_copy_counts(const flx_pileup* cc, uint32_t reference_id, uint64_t from, uint64_t to, uint32_t* out) {
    if (!finished_for_copy(cc, "flx_pileup_copy_counts")) return FLX_ERR_INVALID;
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
