// flx_phase: the object behind the phasing calls of the C ABI (include/floxer_amd.h). The rule and its checks: flx_phase.hpp; the
// kernels: flx_phase.hip and the scan (flx_scan.hip); what it shares with the other side objects: flx_object.hpp. The object holds its
// sites and their anchors, the links (cis and trans per site, added to by every add), one observation byte per slot and one PhaseRecord
// per counted record, both in counting order and growing by doubling, and, behind flx_phase_finish, the results and the tags. It never
// reads the reference text on the device: the text judges the sites at create time, on the host. Made for a context it is counted
// there (flx_ctx_destroy waits for it). An add judges its records and stages their words and letters without the object's lock and
// takes it once for all pieces of its run, for the uploads and the launches only, so several host threads may add at once and the tags
// of one add stay together.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>

#include "flx_phase.hpp"
#include "flx_object.hpp"

using namespace flx;

namespace {
constexpr u64 INITIAL_OBS_CAPACITY = 1ull << 20, INITIAL_RECORD_CAPACITY = 1ull << 14;
}  // namespace

struct flx_phase : SideObject {          // FLX_PHASE_PROFILE: every add and the finish print their device and wall time
    flx_phase_options opt{};
    flx_ctx* ctx = nullptr;              // made by flx_phase_create: counted there
    std::vector<u64> starts;             // n_refs + 1
    std::vector<u32> anchors;            // every site's anchor in the concatenation
    u64 n_sites = 0;
    DeviceBuffer d_anchors, d_sites, cis, trans;
    u64 n_recs = 0, rec_capacity = 0, n_obs = 0, obs_capacity = 0;       // counted records and slots added; what the tables hold
    u32 n_adds = 0;                      // add calls that took the lock
    DeviceBuffer recs, obs;              // the tables
    DeviceBuffer jobs, words, letters;   // an add's staging
    ScanDriver scan;                     // finish
    DeviceBuffer flips, breaks, set_start, set, state, keep, swap;
    DeviceBuffer results, tags;          // behind finish
    bool finished = false;
    ~flx_phase() {
        if (ctx) { std::lock_guard<std::mutex> g(ctx->spare_mu); --ctx->live_phases; }
    }
};

namespace {

// the common part of a create, behind the judgement of the sites
int open_sites(flx_phase* c, int device, std::vector<u64>&& starts, std::vector<u32>&& anchors, const flx_phase_options* o, const flx_phase_site* sites) {
    c->opt = phase_options_or_default(o);
    c->starts = std::move(starts);
    c->anchors = std::move(anchors);
    c->n_sites = c->anchors.size();
    if (device < 0) { set_error("flx_phase: no device given (the host form is flx_phase_host)"); return FLX_ERR_INVALID; }
    FLX_HIP(hipSetDevice(device));
    int rc = c->open(device, "FLX_PHASE_PROFILE");
    if (rc) return rc;
    u64 const n = std::max<u64>(c->n_sites, 1);
    if ((rc = c->d_anchors.ensure(n * 4, true)) || (rc = c->d_sites.ensure(n * sizeof(flx_phase_site), true)) || (rc = c->cis.ensure(n * 4, true)) || (rc = c->trans.ensure(n * 4, true)))
        return rc;
    if (c->n_sites) {
        FLX_HIP(hipMemcpyAsync(c->d_anchors.ptr, c->anchors.data(), c->n_sites * 4, hipMemcpyHostToDevice, c->stream));
        FLX_HIP(hipMemcpyAsync(c->d_sites.ptr, sites, c->n_sites * sizeof(flx_phase_site), hipMemcpyHostToDevice, c->stream));
    }
    FLX_HIP(hipMemsetAsync(c->cis.ptr, 0, n * 4, c->stream));
    FLX_HIP(hipMemsetAsync(c->trans.ptr, 0, n * 4, c->stream));
    FLX_HIP(hipStreamSynchronize(c->stream));
    return FLX_OK;
}

// the table holds at least `need` elements of `size` bytes afterwards, its first `used` as before; a failure leaves it as it was
int grow(flx_phase* c, DeviceBuffer& table, u64& capacity, u64 used, u64 need, u64 initial, u64 most, size_t size) {
    if (need <= capacity) return FLX_OK;
    u64 const cap = std::min<u64>(std::max<u64>({need, capacity * 2, initial}), most);
    DeviceBuffer bigger;
    int rc;
    if ((rc = bigger.ensure(cap * size, true))) return rc;
    if (used) {
        FLX_HIP(hipMemcpyAsync(bigger.ptr, table.ptr, used * size, hipMemcpyDeviceToDevice, c->stream));
        FLX_HIP(hipStreamSynchronize(c->stream));
    }
    table.take(bigger);
    capacity = cap;
    return FLX_OK;
}

// the judged jobs of one word pool, staged without the object's lock: the compacted words, the letters, and every job's record with
// its slots (obs_off counts from the piece's first slot until the commit moves it)
struct Staged {
    std::vector<PileupJob> jobs;
    std::vector<PhaseRecord> recs;
    std::vector<u32> pool;
    std::vector<u8> letters;
    u64 n_slots = 0;
};
void stage(flx_phase const* c, Staged& s, const uint32_t* cigar_words, Letters const& src, const flx_reads* resident) {
    if (s.jobs.empty()) return;
    s.recs.resize(s.jobs.size());
    for (size_t i = 0; i < s.jobs.size(); ++i) {
        PhaseRecord& r = s.recs[i];
        r.text_end = phase_job_end(s.jobs[i], cigar_words);
        phase_slots(c->anchors, s.jobs[i].text_off, r.text_end, r.first, r.n_slots);
        r.obs_off = s.n_slots;
        r.add = 0;
        r.read = (u32)s.jobs[i].read_index;
        s.n_slots += r.n_slots;
    }
    compact_words(s.jobs, cigar_words, s.pool);
    if (resident) for (auto& j : s.jobs) j.seq_off = resident->pool_off[j.read_index] + (j.reverse ? resident->lens[j.read_index] : 0);
    else stage_letters(s.jobs, src, s.letters);
}

// all pieces of one add under one hold of the lock: uploaded and launched piece by piece
int commit(flx_phase* c, std::vector<Staged>& pieces, const flx_reads* resident, const char* who) {
    auto const t0 = std::chrono::steady_clock::now();
    u64 n_recs = 0, n_slots = 0, n_words = 0, n_letters = 0;
    for (auto const& s : pieces) {
        if (s.jobs.size() >= (1ull << 32)) { set_error(std::string(who) + ": too many records in one call"); return FLX_ERR_INVALID; }
        n_recs += s.jobs.size(); n_slots += s.n_slots; n_words += s.pool.size(); n_letters += s.letters.size();
    }
    std::lock_guard<std::mutex> g(c->mu);
    if (c->finished) { set_error(std::string(who) + ": the phase object is finished"); return FLX_ERR_INVALID; }
    if (n_slots > PHASE_MAX_SLOTS - c->n_obs) { set_error(std::string(who) + ": more than 2^32 - 1 observation slots in one phase object"); return FLX_ERR_CAPACITY; }
    u32 const serial = c->n_adds++;
    if (n_recs == 0) return FLX_OK;
    FLX_HIP(hipSetDevice(c->device));
    int rc;
    if ((rc = grow(c, c->recs, c->rec_capacity, c->n_recs, c->n_recs + n_recs, INITIAL_RECORD_CAPACITY, ~0ull, sizeof(PhaseRecord))) ||
        (rc = grow(c, c->obs, c->obs_capacity, c->n_obs, c->n_obs + n_slots, INITIAL_OBS_CAPACITY, PHASE_MAX_SLOTS, 1)))
        return rc;
    float device_ms = 0;                                 // the launches' spans, piece by piece (the uploads lie outside them, as in the other objects)
    for (auto& s : pieces) {
        if (s.jobs.empty()) continue;
        for (auto& r : s.recs) { r.obs_off += c->n_obs; r.add = serial; }
        if ((rc = c->jobs.ensure(s.jobs.size() * sizeof(PileupJob))) || (rc = c->words.ensure(s.pool.size() * 4)) || (rc = c->letters.ensure(s.letters.size() + 1))) return rc;
        PhaseRecord* const d_recs = c->recs.as<PhaseRecord>() + c->n_recs;      // (room for the piece's records and slots: grow saw to it)
        FLX_HIP(hipMemcpyAsync(c->jobs.ptr, s.jobs.data(), s.jobs.size() * sizeof(PileupJob), hipMemcpyHostToDevice, c->stream));
        FLX_HIP(hipMemcpyAsync(d_recs, s.recs.data(), s.recs.size() * sizeof(PhaseRecord), hipMemcpyHostToDevice, c->stream));
        FLX_HIP(hipMemcpyAsync(c->words.ptr, s.pool.data(), s.pool.size() * 4, hipMemcpyHostToDevice, c->stream));
        if (!s.letters.empty()) FLX_HIP(hipMemcpyAsync(c->letters.ptr, s.letters.data(), s.letters.size(), hipMemcpyHostToDevice, c->stream));
        const u8* const d_letters = resident ? resident->d_pool.as<u8>() : c->letters.as<u8>();
        if ((rc = c->span_begin())) return rc;
        if (s.n_slots) {
            FLX_LAUNCH("phase_observe", PhaseDevice::observe(c->stream, c->jobs.as<PileupJob>(), d_recs, (u32)s.jobs.size(), c->words.as<u32>(), d_letters, c->d_anchors.as<u32>(),
                                                             c->d_sites.as<flx_phase_site>(), c->obs.as<u8>()));
            FLX_LAUNCH("phase_links", PhaseDevice::links(c->stream, d_recs, (u32)s.jobs.size(), c->n_obs, s.n_slots, c->obs.as<u8>(), c->cis.as<u32>(), c->trans.as<u32>()));
        }
        if ((rc = c->span_end())) return rc;
        FLX_HIP(hipStreamSynchronize(c->stream));       // (the staging buffers are free for the next piece)
        float ms;
        if ((rc = c->span_ms(ms))) return rc;
        device_ms += ms;
        c->n_recs += s.jobs.size();
        c->n_obs += s.n_slots;
    }
    if (c->profile) {
        double const wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[flx phase] add %u: records %llu words %llu letters %llu slots %llu upload_bytes %llu add_device_ms %.3f wall_ms_behind_the_checks %.3f\n", serial,
                (unsigned long long)n_recs, (unsigned long long)n_words, (unsigned long long)n_letters, (unsigned long long)n_slots,
                (unsigned long long)(n_recs * (sizeof(PileupJob) + sizeof(PhaseRecord)) + n_words * 4 + n_letters), (double)device_ms, wall);
    }
    return FLX_OK;
}

template <class ReadLen>
bool plan(flx_phase* c, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words, uint64_t n_reads, ReadLen read_len, const char* who,
          std::vector<PileupJob>& jobs) {
    return pileup_plan(c->starts, phase_filter(c->opt), records, n, cigar_words, n_words, n_reads, read_len, who, jobs);
}

// all pieces of a run are judged and staged before any is added
int add_run(flx_phase* c, const flx_run* run, Letters const& src, const flx_reads* resident, const char* who) {
    if (c->opt.min_mapq > 0 && !run->has_mapq) { set_error(std::string(who) + ": min_mapq needs a run made with flx_output_options.mapq"); return FLX_ERR_INVALID; }
    auto const parts = run_pieces(run);
    std::vector<Staged> pieces(parts.size());
    if (!judge_in_parallel(parts.size(), [&](size_t i) {
            if (!plan(c, parts[i]->records.data(), parts[i]->records.size(), parts[i]->cigars.data(), parts[i]->cigars.size(), src.n_reads, [&](u64 r) { return src.length(r); }, who,
                      pieces[i].jobs))
                return false;
            stage(c, pieces[i], parts[i]->cigars.data(), src, resident);
            return true;
        }))
        return FLX_ERR_INVALID;
    return commit(c, pieces, resident, who);
}

bool reads_given(const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads) { return n_reads == 0 || (read_pool && read_offsets); }

// a finished table of `n` rows of `row` bytes into the caller's buffer
int copy_table(flx_phase* c, const DeviceBuffer& table, u64 n, size_t row, void* out, uint64_t capacity, const char* who, const char* what) {
    if (capacity < n) { set_error(std::string(who) + ": the buffer is too small, " + std::to_string(n) + " " + what); return FLX_ERR_CAPACITY; }
    if (n == 0) return FLX_OK;
    if (!out) { set_error(std::string(who) + ": null argument"); return FLX_ERR_INVALID; }
    std::lock_guard<std::mutex> g(c->mu);
    FLX_HIP(hipSetDevice(c->device));
    FLX_HIP(hipMemcpyAsync(out, table.ptr, n * row, hipMemcpyDeviceToHost, c->stream));
    FLX_HIP(hipStreamSynchronize(c->stream));
    return FLX_OK;
}

}  // namespace

extern "C" int flx_phase_create_for_text(int hip_device, const uint8_t* ref_ranks_concat, const uint64_t* ref_lens, uint32_t n_refs, const flx_phase_options* o,
                                         const flx_phase_site* sites, uint64_t n_sites, flx_phase** out) {
    if (!out || !ref_ranks_concat) { set_error("flx_phase_create_for_text: null argument"); return FLX_ERR_INVALID; }
    std::vector<u64> starts;
    if (!phase_options_valid(o) || !coverage_lengths_valid(ref_lens, n_refs, "flx_phase_create_for_text", starts)) return FLX_ERR_INVALID;
    if (!errprof_text_valid(ref_ranks_concat, starts.back(), "flx_phase_create_for_text")) return FLX_ERR_INVALID;
    if (hip_device < 0) { set_error("flx_phase_create_for_text: no device given (the host form is flx_phase_host)"); return FLX_ERR_INVALID; }
    std::vector<u32> anchors;
    int rc = phase_sites_valid(starts, [&](u64 r, u64 p) { return (u32)ref_ranks_concat[starts[r] + p]; }, sites, n_sites, "flx_phase_create_for_text", anchors);
    if (rc) return rc;
    auto c = std::make_unique<flx_phase>();          // (an error below drops it: nothing stays allocated)
    if ((rc = open_sites(c.get(), hip_device, std::move(starts), std::move(anchors), o, sites))) return rc;
    *out = c.release();
    return FLX_OK;
}
extern "C" int flx_phase_create(flx_ctx* ctx, const flx_phase_options* o, const flx_phase_site* sites, uint64_t n_sites, flx_phase** out) {
    if (!ctx || !ctx->hidx || !out) { set_error("flx_phase_create: null argument"); return FLX_ERR_INVALID; }
    HostIndex const& H = *ctx->hidx;
    std::vector<u64> starts;
    if (!phase_options_valid(o) || !coverage_lengths_valid(H.seq_len.data(), (uint32_t)H.seq_len.size(), "flx_phase_create", starts)) return FLX_ERR_INVALID;
    if (!ctx->didx.text) { set_error("flx_phase_create: the context holds no text"); return FLX_ERR_INVALID; }
    // the text judges the sites: the index's host copy, or, for an index without its host arrays, the device's
    std::vector<u8> fetched;
    const u8* text = H.text.data();
    if (H.text.size() != H.n) {
        fetched.resize(H.n);
        FLX_HIP(hipSetDevice(ctx->device));
        FLX_HIP(hipMemcpy(fetched.data(), ctx->didx.text, H.n, hipMemcpyDeviceToHost));
        text = fetched.data();
    }
    std::vector<u32> anchors;
    int rc = phase_sites_valid(starts, [&](u64 r, u64 p) { return (u32)text[H.seq_start[r] + p]; }, sites, n_sites, "flx_phase_create", anchors);      // (positions through the padded starts)
    if (rc) return rc;
    auto c = std::make_unique<flx_phase>();
    if ((rc = open_sites(c.get(), ctx->device, std::move(starts), std::move(anchors), o, sites))) return rc;
    { std::lock_guard<std::mutex> g(ctx->spare_mu); ++ctx->live_phases; }
    c->ctx = ctx;
    *out = c.release();
    return FLX_OK;
}
extern "C" void flx_phase_free(flx_phase* c) { free_object(c); }

extern "C" int flx_phase_add_records(flx_phase* c, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words, const uint8_t* read_pool,
                                     const uint64_t* read_offsets, uint64_t n_reads) {
    if (!c || (n && !records) || !reads_given(read_pool, read_offsets, n_reads)) { set_error("flx_phase_add_records: null argument"); return FLX_ERR_INVALID; }
    Letters src;
    src.read_pool = read_pool; src.read_offsets = read_offsets; src.n_reads = n_reads;
    std::vector<Staged> pieces(1);
    if (!plan(c, records, n, cigar_words, n_words, n_reads, [&](u64 r) { return src.length(r); }, "flx_phase_add_records", pieces[0].jobs)) return FLX_ERR_INVALID;
    stage(c, pieces[0], cigar_words, src, nullptr);
    return commit(c, pieces, nullptr, "flx_phase_add_records");
}
extern "C" int flx_phase_add_run(flx_phase* c, const flx_run* run, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads) {
    if (!c || !run || !reads_given(read_pool, read_offsets, n_reads)) { set_error("flx_phase_add_run: null argument"); return FLX_ERR_INVALID; }
    Letters src;
    src.read_pool = read_pool; src.read_offsets = read_offsets; src.n_reads = n_reads;
    return add_run(c, run, src, nullptr, "flx_phase_add_run");
}
extern "C" int flx_phase_add_run_resident(flx_phase* c, const flx_run* run, const flx_reads* reads) {
    if (!c || !run || !reads) { set_error("flx_phase_add_run_resident: null argument"); return FLX_ERR_INVALID; }
    Letters src;
    src.batch = reads; src.n_reads = reads->n_reads;
    // the batch's device pool when it lives on this object's device, its host copy through the staged path otherwise
    bool const here = reads->ctx && reads->ctx->device == c->device && reads->d_pool.ptr;
    return add_run(c, run, src, here ? reads : nullptr, "flx_phase_add_run_resident");
}

extern "C" int flx_phase_finish(flx_phase* c) {
    if (!c) { set_error("flx_phase_finish: null argument"); return FLX_ERR_INVALID; }
    std::lock_guard<std::mutex> g(c->mu);
    if (c->finished) { set_error("flx_phase_finish: the phase object is finished"); return FLX_ERR_INVALID; }
    auto const t0 = std::chrono::steady_clock::now();
    FLX_HIP(hipSetDevice(c->device));
    PhaseModel const m = phase_model(c->opt);
    u32 const n = (u32)c->n_sites;
    u64 const ns = std::max<u64>(n, 1);
    int rc;
    if ((rc = c->flips.ensure(ns * 4, true)) || (rc = c->breaks.ensure(ns * 4, true)) || (rc = c->set_start.ensure((ns + 1) * 4, true)) || (rc = c->set.ensure(ns * 4, true)) ||
        (rc = c->state.ensure(ns * 4, true)) || (rc = c->keep.ensure(ns * 4, true)) || (rc = c->swap.ensure(ns * 4, true)) || (rc = c->results.ensure(ns * sizeof(flx_phase_result), true)) ||
        (rc = c->tags.ensure(std::max<u64>(c->n_recs, 1) * sizeof(flx_phase_tag), true)) || (rc = c->scan.reserve(ns)))
        return rc;
    const PhaseRecord* const recs = c->recs.as<PhaseRecord>();
    const u8* const obs = c->obs.as<u8>();
    u32 *const set = c->set.as<u32>(), *const state = c->state.as<u32>(), *const keep = c->keep.as<u32>(), *const swap = c->swap.as<u32>();
    if ((rc = c->span_begin())) return rc;
    // (a) the chain: flags, their two scans, the set starts, the phase
    FLX_LAUNCH("phase_chain", PhaseDevice::chain(c->stream, 0, c->d_sites.as<flx_phase_site>(), n, c->cis.as<u32>(), c->trans.as<u32>(), m.min_link, c->flips.as<u32>(),
                                                 c->breaks.as<u32>(), nullptr, nullptr, nullptr));
    if (n && ((rc = c->scan.inclusive(c->stream, c->flips.as<u32>(), n)) || (rc = c->scan.inclusive(c->stream, c->breaks.as<u32>(), n)))) return rc;
    FLX_LAUNCH("phase_chain", PhaseDevice::chain(c->stream, 1, nullptr, n, nullptr, nullptr, 0, nullptr, c->breaks.as<u32>(), c->set_start.as<u32>(), nullptr, nullptr));
    FLX_LAUNCH("phase_chain", PhaseDevice::chain(c->stream, 2, nullptr, n, nullptr, nullptr, 0, c->flips.as<u32>(), c->breaks.as<u32>(), c->set_start.as<u32>(), set, state));
    // (b) the tags, then the rounds: votes, flips, the tags again
    FLX_LAUNCH("phase_tags", PhaseDevice::tags(c->stream, recs, c->n_recs, obs, set, state, m.min_margin, c->tags.as<flx_phase_tag>()));
    FLX_HIP(hipMemsetAsync(keep, 0, ns * 4, c->stream));
    FLX_HIP(hipMemsetAsync(swap, 0, ns * 4, c->stream));
    for (u32 round = 0; round < m.rounds; ++round) {
        if (round) {
            FLX_HIP(hipMemsetAsync(keep, 0, ns * 4, c->stream));
            FLX_HIP(hipMemsetAsync(swap, 0, ns * 4, c->stream));
        }
        FLX_LAUNCH("phase_votes", PhaseDevice::votes(c->stream, recs, c->n_recs, c->n_obs, obs, set, state, c->tags.as<flx_phase_tag>(), keep, swap));
        FLX_LAUNCH("phase_revote", PhaseDevice::revote(c->stream, n, keep, swap, state));
        FLX_LAUNCH("phase_tags", PhaseDevice::tags(c->stream, recs, c->n_recs, obs, set, state, m.min_margin, c->tags.as<flx_phase_tag>()));
    }
    FLX_LAUNCH("phase_results", PhaseDevice::results(c->stream, n, set, state, c->cis.as<u32>(), c->trans.as<u32>(), keep, swap, c->results.as<flx_phase_result>()));
    if ((rc = c->span_end())) return rc;
    FLX_HIP(hipStreamSynchronize(c->stream));
    c->finished = true;
    // what only the adds and the finish needed
    c->obs.release(); c->recs.release(); c->jobs.release(); c->words.release(); c->letters.release(); c->cis.release(); c->trans.release(); c->flips.release();
    c->breaks.release(); c->set_start.release(); c->set.release(); c->state.release(); c->keep.release(); c->swap.release(); c->d_anchors.release(); c->d_sites.release();
    c->obs_capacity = c->rec_capacity = 0;
    if (c->profile) {
        float ms;
        if ((rc = c->span_ms(ms))) return rc;
        fprintf(stderr, "[flx phase] finish: sites %llu records %llu slots %llu rounds %u finish_device_ms %.3f wall_ms %.3f\n", (unsigned long long)c->n_sites,
                (unsigned long long)c->n_recs, (unsigned long long)c->n_obs, m.rounds, (double)ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    return FLX_OK;
}

extern "C" uint64_t flx_phase_num_sites(const flx_phase* c) { return c ? c->n_sites : 0; }
extern "C" int flx_phase_copy_results(const flx_phase* cc, flx_phase_result* out, uint64_t capacity) {
    if (!finished_for_copy(cc, "flx_phase_copy_results", "flx_phase_finish")) return FLX_ERR_INVALID;
    flx_phase* const c = const_cast<flx_phase*>(cc);
    return copy_table(c, c->results, c->n_sites, sizeof(flx_phase_result), out, capacity, "flx_phase_copy_results", "sites");
}
extern "C" uint64_t flx_phase_num_tags(const flx_phase* c) {
    if (!c) return 0;
    std::lock_guard<std::mutex> g(const_cast<flx_phase*>(c)->mu);
    return c->finished ? c->n_recs : 0;
}
extern "C" int flx_phase_copy_tags(const flx_phase* cc, flx_phase_tag* out, uint64_t capacity) {
    if (!finished_for_copy(cc, "flx_phase_copy_tags", "flx_phase_finish")) return FLX_ERR_INVALID;
    flx_phase* const c = const_cast<flx_phase*>(cc);
    return copy_table(c, c->tags, c->n_recs, sizeof(flx_phase_tag), out, capacity, "flx_phase_copy_tags", "tags");
}

extern "C" int flx_phase_geometry(uint32_t out[4]) {
    if (!out) { set_error("flx_phase_geometry: null argument"); return FLX_ERR_INVALID; }
    out[0] = PhaseDevice::OBSERVE_GRID_CAP; out[1] = PhaseDevice::OBSERVE_WAVES; out[2] = ScanDevice::SCAN_TILE; out[3] = CONSENSUS_MAX_INS;
    return FLX_OK;
}

extern "C" int flx_phase_host(const uint8_t* ref_ranks_concat, const uint64_t* ref_lens, uint32_t n_refs, const flx_phase_options* o, const flx_phase_site* sites, uint64_t n_sites,
                              const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words, const uint8_t* read_pool, const uint64_t* read_offsets,
                              uint64_t n_reads, flx_phase_result* results, flx_phase_tag* tags, uint64_t* n_tags) {
    std::vector<u64> starts;
    if (!phase_options_valid(o) || !coverage_lengths_valid(ref_lens, n_refs, "flx_phase_host", starts)) return FLX_ERR_INVALID;
    if (!ref_ranks_concat || !n_tags || (n && !records) || !reads_given(read_pool, read_offsets, n_reads)) { set_error("flx_phase_host: null argument"); return FLX_ERR_INVALID; }
    if (!errprof_text_valid(ref_ranks_concat, starts.back(), "flx_phase_host")) return FLX_ERR_INVALID;
    std::vector<u32> anchors;
    int const rc = phase_sites_valid(starts, [&](u64 r, u64 p) { return (u32)ref_ranks_concat[starts[r] + p]; }, sites, n_sites, "flx_phase_host", anchors);
    if (rc) return rc;
    flx_phase_options const opt = phase_options_or_default(o);
    std::vector<PileupJob> jobs;
    if (!pileup_plan(starts, phase_filter(opt), records, n, cigar_words, n_words, n_reads, [&](u64 r) { return read_offsets[r + 1] - read_offsets[r]; }, "flx_phase_host", jobs))
        return FLX_ERR_INVALID;
    std::vector<PhaseRecord> recs(jobs.size());
    u64 n_slots = 0;
    for (size_t i = 0; i < jobs.size(); ++i) {
        PhaseRecord& r = recs[i];
        r.text_end = phase_job_end(jobs[i], cigar_words);
        phase_slots(anchors, jobs[i].text_off, r.text_end, r.first, r.n_slots);
        r.obs_off = n_slots; r.add = 0; r.read = (u32)jobs[i].read_index;
        n_slots += r.n_slots;
    }
    if (n_slots > PHASE_MAX_SLOTS) { set_error("flx_phase_host: more than 2^32 - 1 observation slots"); return FLX_ERR_CAPACITY; }
    u64 const cap_tags = *n_tags;
    *n_tags = jobs.size();
    if (jobs.size() > cap_tags || (!jobs.empty() && !tags)) { set_error("flx_phase_host: the tag buffer is too small: " + std::to_string(jobs.size()) + " tags"); return FLX_ERR_CAPACITY; }
    if (n_sites && !results) { set_error("flx_phase_host: null argument"); return FLX_ERR_INVALID; }
    std::vector<u8> obs(n_slots, (u8)PHASE_NONE);
    for (size_t i = 0; i < jobs.size(); ++i) {
        const uint8_t* const read = read_pool + read_offsets[jobs[i].read_index];
        phase_job_observe(jobs[i], recs[i], cigar_words, read, read_offsets[jobs[i].read_index + 1] - read_offsets[jobs[i].read_index], anchors.data(), sites, obs.data());
    }
    phase_finish_host(sites, n_sites, recs, obs.data(), phase_model(opt), results, tags);
    return FLX_OK;
}
