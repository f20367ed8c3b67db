// flx_errprof: the object behind the error-profile calls of the C ABI (include/floxer_amd.h). The rule and its checks: flx_errprof.hpp; the
// kernel: flx_errprof.hip; what it shares with the other side objects: flx_object.hpp. The object owns one stream, the table of u64
// counters in HBM, its staging buffers and, when it was made for a text of its own, that text; made for a context it reads the context's
// text where it lies and is counted there (flx_ctx_destroy waits for it). Adds judge their records and stage their words and letters
// without the object's lock and take it for the upload and the launch only, so several host threads may add at once.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>

#include "flx_errprof.hpp"
#include "flx_object.hpp"

using namespace flx;

struct flx_errprof : SideObject {        // FLX_ERRPROF_PROFILE: every add prints its upload, its kernel's device time and its wall time
    flx_errprof_options opt{};
    flx_ctx* ctx = nullptr;              // made by flx_errprof_create: the text is the context's
    std::vector<u64> starts;             // n_refs + 1: the sequences in the unpadded concatenation (the judgement)
    std::vector<u64> seq_base;           // n_refs: where each begins in the text the kernel reads
    const u8* d_text = nullptr;
    DeviceBuffer own_text, table;        // table: ERRPROF_ENTRIES u64
    DeviceBuffer jobs, words, letters;   // an add's staging: the counted records, the words and the oriented sequences they refer to
    u32 flush_threshold() const { return opt.flush_threshold ? opt.flush_threshold : ERRPROF_DEFAULT_FLUSH; }
    ~flx_errprof() {
        if (ctx) { std::lock_guard<std::mutex> g(ctx->spare_mu); --ctx->live_errprofs; }
    }
};

namespace {

// the common part of a create: the stream and the cleared table
int open_table(flx_errprof* c, int device) {
    FLX_HIP(hipSetDevice(device));                  // (a device below 0 is refused here: the host form is flx_errprof_host)
    int rc = c->open(device, "FLX_ERRPROF_PROFILE");
    if (rc) return rc;
    if ((rc = c->table.ensure(sizeof(flx_errprof_table), true))) return rc;
    FLX_HIP(hipMemsetAsync(c->table.ptr, 0, sizeof(flx_errprof_table), c->stream));
    return FLX_OK;
}

// the judged jobs of one word pool: staged, then uploaded and launched under the object's lock. resident: the letters are read from the
// batch's device pool (on this object's device); otherwise the oriented sequences in use go up from `src`.
int commit(flx_errprof* c, std::vector<ErrprofJob>& jobs, const uint32_t* cigar_words, Letters const& src, const flx_reads* resident, const char* who) {
    if (jobs.size() >= (1ull << 32)) { set_error(std::string(who) + ": too many records in one call"); return FLX_ERR_INVALID; }
    if (jobs.empty()) return FLX_OK;
    auto const t0 = std::chrono::steady_clock::now();
    std::vector<u32> pool;
    std::vector<u8> letters;
    compact_words(jobs, cigar_words, pool);
    if (resident) for (auto& j : jobs) j.seq_off = resident->pool_off[j.read_index] + (j.reverse ? resident->lens[j.read_index] : 0);
    else stage_letters(jobs, src, letters);
    std::lock_guard<std::mutex> g(c->mu);
    FLX_HIP(hipSetDevice(c->device));
    int rc;
    if ((rc = c->jobs.ensure(jobs.size() * sizeof(ErrprofJob))) || (rc = c->words.ensure(pool.size() * 4)) || (rc = c->letters.ensure(letters.size() + 1))) return rc;
    FLX_HIP(hipMemcpyAsync(c->jobs.ptr, jobs.data(), jobs.size() * sizeof(ErrprofJob), hipMemcpyHostToDevice, c->stream));
    FLX_HIP(hipMemcpyAsync(c->words.ptr, pool.data(), pool.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (!letters.empty()) FLX_HIP(hipMemcpyAsync(c->letters.ptr, letters.data(), letters.size(), hipMemcpyHostToDevice, c->stream));
    if ((rc = c->span_begin())) return rc;
    FLX_LAUNCH("errprof_add", ErrprofDevice::add(c->stream, c->jobs.as<ErrprofJob>(), (u32)jobs.size(), c->words.as<u32>(), c->d_text,
                                                 resident ? resident->d_pool.as<u8>() : c->letters.as<u8>(), c->table.as<unsigned long long>(), c->flush_threshold()));
    if ((rc = c->span_end())) return rc;
    FLX_HIP(hipStreamSynchronize(c->stream));           // (the staging buffers are free for the next add)
    if (c->profile) {
        float ms;
        if ((rc = c->span_ms(ms))) return rc;
        double const wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[flx errprof] add: records %zu words %zu letters %zu upload_bytes %zu errprof_add_ms %.3f wall_ms_behind_the_checks %.3f\n", jobs.size(), pool.size(),
                letters.size(), jobs.size() * sizeof(ErrprofJob) + pool.size() * 4 + letters.size(), (double)ms, wall);
    }
    return FLX_OK;
}

// all pieces of a run are judged before any is added
int add_run(flx_errprof* c, const flx_run* run, Letters const& src, const flx_reads* resident, const char* who) {
    if (c->opt.min_mapq > 0 && !run->has_mapq) { set_error(std::string(who) + ": min_mapq needs a run made with flx_output_options.mapq"); return FLX_ERR_INVALID; }
    auto const pieces = run_pieces(run);
    std::vector<std::vector<ErrprofJob>> jobs(pieces.size());
    if (!judge_in_parallel(pieces.size(), [&](size_t i) {
            return errprof_plan(c->starts, c->seq_base, c->opt, pieces[i]->records.data(), pieces[i]->records.size(), pieces[i]->cigars.data(), pieces[i]->cigars.size(),
                                src.n_reads, [&](u64 r) { return src.length(r); }, who, jobs[i]);
        }))
        return FLX_ERR_INVALID;
    for (size_t i = 0; i < pieces.size(); ++i) {
        int const rc = commit(c, jobs[i], pieces[i]->cigars.data(), src, resident, who);
        if (rc) return rc;
    }
    return FLX_OK;
}

bool reads_given(const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads) { return n_reads == 0 || (read_pool && read_offsets); }

// the table on the host, the stream idle; the object's lock is held
int fetch(flx_errprof* c, flx_errprof_table* out) {
    FLX_HIP(hipSetDevice(c->device));
    FLX_HIP(hipMemcpyAsync(out, c->table.ptr, sizeof(flx_errprof_table), hipMemcpyDeviceToHost, c->stream));
    FLX_HIP(hipStreamSynchronize(c->stream));
    return FLX_OK;
}

}  // namespace

extern "C" int flx_errprof_create_for_text(int hip_device, const uint8_t* ref_ranks_concat, const uint64_t* ref_lens, uint32_t n_refs, const flx_errprof_options* o,
                                           flx_errprof** out) {
    if (!out || !ref_ranks_concat) { set_error("flx_errprof_create_for_text: null argument"); return FLX_ERR_INVALID; }
    std::vector<u64> starts;
    if (!errprof_options_valid(o) || !coverage_lengths_valid(ref_lens, n_refs, "flx_errprof_create_for_text", starts)) return FLX_ERR_INVALID;
    if (!errprof_text_valid(ref_ranks_concat, starts.back(), "flx_errprof_create_for_text")) return FLX_ERR_INVALID;
    if (hip_device < 0) { set_error("flx_errprof_create_for_text: no device given (the host form is flx_errprof_host)"); return FLX_ERR_INVALID; }
    auto c = std::make_unique<flx_errprof>();        // (an error below drops it: nothing stays allocated)
    c->opt = errprof_options_or_default(o);
    int rc = open_table(c.get(), hip_device);
    if (rc) return rc;
    u64 const total = starts.back();
    if ((rc = c->own_text.ensure(total, true))) return rc;
    FLX_HIP(hipMemcpyAsync(c->own_text.ptr, ref_ranks_concat, total, hipMemcpyHostToDevice, c->stream));
    FLX_HIP(hipStreamSynchronize(c->stream));
    c->d_text = c->own_text.as<u8>();
    c->seq_base.assign(starts.begin(), starts.end() - 1);
    c->starts = std::move(starts);
    *out = c.release();
    return FLX_OK;
}
extern "C" int flx_errprof_create(flx_ctx* ctx, const flx_errprof_options* o, flx_errprof** out) {
    if (!ctx || !ctx->hidx || !out) { set_error("flx_errprof_create: null argument"); return FLX_ERR_INVALID; }
    HostIndex const& H = *ctx->hidx;
    std::vector<u64> starts;
    if (!errprof_options_valid(o) || !coverage_lengths_valid(H.seq_len.data(), (uint32_t)H.seq_len.size(), "flx_errprof_create", starts)) return FLX_ERR_INVALID;
    if (!ctx->didx.text) { set_error("flx_errprof_create: the context holds no text"); return FLX_ERR_INVALID; }
    if (H.text.size() == H.n && !errprof_text_valid(H.text.data(), H.n, "flx_errprof_create")) return FLX_ERR_INVALID;      // (an index without its host arrays was checked when it was built)
    auto c = std::make_unique<flx_errprof>();
    c->opt = errprof_options_or_default(o);
    int const rc = open_table(c.get(), ctx->device);
    if (rc) return rc;
    FLX_HIP(hipStreamSynchronize(c->stream));
    c->d_text = ctx->didx.text;                      // positions are addressed through the padded starts, as the MD and cs jobs do
    c->seq_base.assign(H.seq_start.begin(), H.seq_start.end());
    c->starts = std::move(starts);
    { std::lock_guard<std::mutex> g(ctx->spare_mu); ++ctx->live_errprofs; }
    c->ctx = ctx;
    *out = c.release();
    return FLX_OK;
}
extern "C" void flx_errprof_free(flx_errprof* c) { free_object(c); }

extern "C" int flx_errprof_add_records(flx_errprof* c, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words,
                                       const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads) {
    if (!c || (n && !records) || !reads_given(read_pool, read_offsets, n_reads)) { set_error("flx_errprof_add_records: null argument"); return FLX_ERR_INVALID; }
    Letters src;
    src.read_pool = read_pool; src.read_offsets = read_offsets; src.n_reads = n_reads;
    std::vector<ErrprofJob> jobs;
    if (!errprof_plan(c->starts, c->seq_base, c->opt, records, n, cigar_words, n_words, n_reads, [&](u64 r) { return src.length(r); }, "flx_errprof_add_records", jobs)) return FLX_ERR_INVALID;
    return commit(c, jobs, cigar_words, src, nullptr, "flx_errprof_add_records");
}
extern "C" int flx_errprof_add_run(flx_errprof* c, const flx_run* run, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads) {
    if (!c || !run || !reads_given(read_pool, read_offsets, n_reads)) { set_error("flx_errprof_add_run: null argument"); return FLX_ERR_INVALID; }
    Letters src;
    src.read_pool = read_pool; src.read_offsets = read_offsets; src.n_reads = n_reads;
    return add_run(c, run, src, nullptr, "flx_errprof_add_run");
}
extern "C" int flx_errprof_add_run_resident(flx_errprof* c, const flx_run* run, const flx_reads* reads) {
    if (!c || !run || !reads) { set_error("flx_errprof_add_run_resident: null argument"); return FLX_ERR_INVALID; }
    Letters src;
    src.batch = reads; src.n_reads = reads->n_reads;
    // the batch's device pool when it lives on this object's device, its host copy through the staged path otherwise
    bool const here = reads->ctx && reads->ctx->device == c->device && reads->d_pool.ptr;
    return add_run(c, run, src, here ? reads : nullptr, "flx_errprof_add_run_resident");
}

extern "C" int flx_errprof_absorb(flx_errprof* into, flx_errprof* from) {
    if (!into || !from || into == from) { set_error("flx_errprof_absorb: null argument, or an object absorbed into itself"); return FLX_ERR_INVALID; }
    std::lock(into->mu, from->mu);
    std::lock_guard<std::mutex> g1(into->mu, std::adopt_lock), g2(from->mu, std::adopt_lock);
    if (into->starts != from->starts) { set_error("flx_errprof_absorb: the objects belong to different reference lengths"); return FLX_ERR_INVALID; }
    if (!errprof_options_equal(into->opt, from->opt)) { set_error("flx_errprof_absorb: the objects have different options"); return FLX_ERR_INVALID; }
    // 9 KB: both tables come to the host, their sum goes back to `into`, zeros to `from`
    auto a = std::make_unique<flx_errprof_table>(), b = std::make_unique<flx_errprof_table>();
    int rc;
    if ((rc = fetch(into, a.get())) || (rc = fetch(from, b.get()))) return rc;
    uint64_t* const x = reinterpret_cast<uint64_t*>(a.get());
    const uint64_t* const y = reinterpret_cast<const uint64_t*>(b.get());
    for (u32 i = 0; i < ERRPROF_ENTRIES; ++i) x[i] += y[i];
    FLX_HIP(hipSetDevice(into->device));
    FLX_HIP(hipMemcpyAsync(into->table.ptr, a.get(), sizeof(flx_errprof_table), hipMemcpyHostToDevice, into->stream));
    FLX_HIP(hipStreamSynchronize(into->stream));
    FLX_HIP(hipSetDevice(from->device));
    FLX_HIP(hipMemsetAsync(from->table.ptr, 0, sizeof(flx_errprof_table), from->stream));
    FLX_HIP(hipStreamSynchronize(from->stream));
    return FLX_OK;
}

extern "C" int flx_errprof_copy(const flx_errprof* cc, flx_errprof_table* out) {
    if (!cc || !out) { set_error("flx_errprof_copy: null argument"); return FLX_ERR_INVALID; }
    flx_errprof* const c = const_cast<flx_errprof*>(cc);
    std::lock_guard<std::mutex> g(c->mu);
    return fetch(c, out);
}

extern "C" int flx_errprof_host(const uint8_t* ref_ranks_concat, const uint64_t* ref_lens, uint32_t n_refs, const flx_errprof_options* o, const flx_record* records,
                                uint64_t n, const uint32_t* cigar_words, uint64_t n_words, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads,
                                flx_errprof_table* table) {
    std::vector<u64> starts;
    if (!errprof_options_valid(o) || !coverage_lengths_valid(ref_lens, n_refs, "flx_errprof_host", starts)) return FLX_ERR_INVALID;
    if (!table || !ref_ranks_concat || (n && !records) || !reads_given(read_pool, read_offsets, n_reads)) { set_error("flx_errprof_host: null argument"); return FLX_ERR_INVALID; }
    if (!errprof_text_valid(ref_ranks_concat, starts.back(), "flx_errprof_host")) return FLX_ERR_INVALID;
    flx_errprof_options const opt = errprof_options_or_default(o);
    std::vector<u64> const seq_base(starts.begin(), starts.end() - 1);
    std::vector<ErrprofJob> jobs;
    if (!errprof_plan(starts, seq_base, opt, records, n, cigar_words, n_words, n_reads, [&](u64 r) { return read_offsets[r + 1] - read_offsets[r]; }, "flx_errprof_host", jobs)) return FLX_ERR_INVALID;
    for (auto const& j : jobs) errprof_walk(j, cigar_words, ref_ranks_concat, read_pool + read_offsets[j.read_index], reinterpret_cast<uint64_t*>(table));
    return FLX_OK;
}
