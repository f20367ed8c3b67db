// flx_variants: the object behind the variant calls of the C ABI (include/floxer_amd.h). The rule and its checks: flx_variants.hpp; the
// kernels: flx_variants.hip, pileup_add (flx_pileup.hip), consensus_allele_heads and consensus_allele_fill (flx_consensus.hip), the
// sort's driver (flx_sort_driver.hpp) and the scan (flx_scan.hip); what it shares with the other side objects: flx_object.hpp. The
// object is a PlaneObject with pileup's seven planes and an eighth (events per anchor, written at the finish) plus the key table (one
// SortKey per insertion or deletion event, in adding order) and, behind flx_variants_finish, the rows and the alleles. Made for a
// context it reads the context's text where it lies and is counted there (flx_ctx_destroy waits for it). Adds judge their records and
// stage their words and letters without the object's lock and take it for the upload and the launches only, so several host threads may
// add at once.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>

#include "flx_variants.hpp"
#include "flx_object.hpp"
#include "flx_sort_driver.hpp"

using namespace flx;

namespace {
constexpr u64 INITIAL_KEY_CAPACITY = 1ull << 16;
}  // namespace

struct flx_variants : PlaneObject {      // acc: VARIANTS_PLANES * stride entries; FLX_VARIANTS_PROFILE: every add and the finish print their device and wall time
    flx_variants_options opt{};
    flx_ctx* ctx = nullptr;              // made by flx_variants_create: the text is the context's
    u64 stride = 0;                      // entries per plane: total + 1 rounded up to 64 (every plane starts 256-byte aligned)
    const u8* d_text = nullptr;
    DeviceBuffer own_text, text_delta;   // text_delta: per sequence, what leads from a position in the concatenation to its letter in d_text
    u64 n_keys = 0, key_capacity = 0;    // events added; events the table holds
    DeviceBuffer keys;                   // the table
    DeviceBuffer jobs, key_off, words, letters;      // an add's staging
    RadixSorter sorter;                  // finish
    ScanDriver key_scan;
    DeviceBuffer ids, run_start, run_end, count, d_n_rows;
    DeviceBuffer alleles, rows;          // behind finish
    bool failed = false;                 // finish found 2^32 rows or more: the object holds no result
    u64 n_alleles = 0, n_rows = 0;
    u32* plane(u32 k) const { return acc.as<u32>() + (u64)k * stride; }
    ~flx_variants() {
        if (ctx) { std::lock_guard<std::mutex> g(ctx->spare_mu); --ctx->live_variants; }
    }
};

namespace {

// the common part of a create: the planes, the tile counts and the per-sequence deltas (seq_base[r]: where sequence r begins in the text)
int open_planes(flx_variants* c, int device, std::vector<u64>&& starts, std::vector<u64> const& seq_base, const flx_variants_options* o) {
    c->opt = variants_options_or_default(o);
    c->stride = (starts.back() + 1 + 63) / 64 * 64;
    std::vector<i64> delta(seq_base.size());
    for (size_t r = 0; r < seq_base.size(); ++r) delta[r] = (i64)seq_base[r] - (i64)starts[r];
    int rc = c->create(device, "FLX_VARIANTS_PROFILE", std::move(starts), (u64)VARIANTS_PLANES * c->stride, {&c->count});
    if (rc) return rc;
    if ((rc = c->text_delta.ensure(delta.size() * 8, true)) || (rc = c->d_n_rows.ensure(8, true))) return rc;
    FLX_HIP(hipMemcpyAsync(c->text_delta.ptr, delta.data(), delta.size() * 8, hipMemcpyHostToDevice, c->stream));
    FLX_HIP(hipStreamSynchronize(c->stream));
    return FLX_OK;
}

// the table holds at least `need` keys afterwards, its first n_keys as before; a failure leaves it as it was
int grow(flx_variants* c, u64 need) {
    if (need <= c->key_capacity) return FLX_OK;
    u64 const cap = std::min<u64>(std::max<u64>({need, c->key_capacity * 2, INITIAL_KEY_CAPACITY}), VARIANTS_MAX_EVENTS);
    DeviceBuffer keys;
    int rc;
    if ((rc = keys.ensure(cap * sizeof(SortKey), true))) return rc;
    if (c->n_keys) {
        FLX_HIP(hipMemcpyAsync(keys.ptr, c->keys.ptr, c->n_keys * sizeof(SortKey), hipMemcpyDeviceToDevice, c->stream));
        FLX_HIP(hipStreamSynchronize(c->stream));
    }
    c->keys.take(keys);
    c->key_capacity = cap;
    return FLX_OK;
}

// the judged jobs of one word pool: staged, then uploaded and launched under the object's lock. resident: the letters are read from the
// batch's device pool (on this object's device); otherwise the oriented sequences in use go up from `src`.
int commit(flx_variants* c, std::vector<PileupJob>& jobs, const uint32_t* cigar_words, Letters const& src, const flx_reads* resident, const char* who) {
    if (jobs.size() >= (1ull << 32)) { set_error(std::string(who) + ": too many records in one call"); return FLX_ERR_INVALID; }
    auto const t0 = std::chrono::steady_clock::now();
    std::vector<u32> pool;
    std::vector<u8> letters;
    std::vector<u64> key_off(jobs.size());               // every job's first key slot among this add's
    u64 n_keys = 0;
    if (!jobs.empty()) {
        for (size_t i = 0; i < jobs.size(); ++i) { key_off[i] = n_keys; n_keys += variants_job_slots(jobs[i], cigar_words); }
        compact_words(jobs, cigar_words, pool);
        if (resident) for (auto& j : jobs) j.seq_off = resident->pool_off[j.read_index] + (j.reverse ? resident->lens[j.read_index] : 0);
        else stage_letters(jobs, src, letters);
    }
    std::lock_guard<std::mutex> g(c->mu);
    if (c->finished) { set_error(std::string(who) + ": the variants object is finished"); return FLX_ERR_INVALID; }
    if (jobs.empty()) return FLX_OK;
    if (n_keys > VARIANTS_MAX_EVENTS - c->n_keys) { set_error(std::string(who) + ": more than 2^32 - 1 insertion and deletion events in one variants object"); return FLX_ERR_CAPACITY; }
    FLX_HIP(hipSetDevice(c->device));
    int rc;
    if ((rc = grow(c, c->n_keys + n_keys))) return rc;
    if ((rc = c->jobs.ensure(jobs.size() * sizeof(PileupJob))) || (rc = c->key_off.ensure(jobs.size() * 8)) || (rc = c->words.ensure(pool.size() * 4)) ||
        (rc = c->letters.ensure(letters.size() + 1)))
        return rc;
    FLX_HIP(hipMemcpyAsync(c->jobs.ptr, jobs.data(), jobs.size() * sizeof(PileupJob), hipMemcpyHostToDevice, c->stream));
    FLX_HIP(hipMemcpyAsync(c->key_off.ptr, key_off.data(), key_off.size() * 8, hipMemcpyHostToDevice, c->stream));
    FLX_HIP(hipMemcpyAsync(c->words.ptr, pool.data(), pool.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (!letters.empty()) FLX_HIP(hipMemcpyAsync(c->letters.ptr, letters.data(), letters.size(), hipMemcpyHostToDevice, c->stream));
    const u8* const d_letters = resident ? resident->d_pool.as<u8>() : c->letters.as<u8>();
    if ((rc = c->span_begin())) return rc;
    FLX_LAUNCH("pileup_add", PileupDevice::add(c->stream, c->jobs.as<PileupJob>(), (u32)jobs.size(), c->words.as<u32>(), d_letters, c->acc.as<u32>(), c->stride));
    if (n_keys)                                          // (room for n_keys behind the table's n_keys: grow saw to it)
        FLX_LAUNCH("variants_indel_keys", VariantsDevice::indel_keys(c->stream, c->jobs.as<PileupJob>(), c->key_off.as<u64>(), (u32)jobs.size(), c->words.as<u32>(), d_letters,
                                                                     variants_model(c->opt).max_del, c->keys.as<SortKey>() + c->n_keys));
    if ((rc = c->span_end())) return rc;
    FLX_HIP(hipStreamSynchronize(c->stream));           // (the staging buffers are free for the next add)
    c->n_keys += n_keys;
    if (c->profile) {
        float ms;
        if ((rc = c->span_ms(ms))) return rc;
        double const wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[flx variants] add: records %zu words %zu letters %zu events %llu upload_bytes %zu add_device_ms %.3f wall_ms_behind_the_checks %.3f\n", jobs.size(),
                pool.size(), letters.size(), (unsigned long long)n_keys, jobs.size() * (sizeof(PileupJob) + 8) + pool.size() * 4 + letters.size(), (double)ms, wall);
    }
    return FLX_OK;
}

template <class ReadLen>
bool plan(flx_variants* c, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words, uint64_t n_reads, ReadLen read_len, const char* who,
          std::vector<PileupJob>& jobs) {
    return pileup_plan(c->starts, variants_filter(c->opt), records, n, cigar_words, n_words, n_reads, read_len, who, jobs);
}

// all pieces of a run are judged before any is added
int add_run(flx_variants* c, const flx_run* run, Letters const& src, const flx_reads* resident, const char* who) {
    if (c->opt.min_mapq > 0 && !run->has_mapq) { set_error(std::string(who) + ": min_mapq needs a run made with flx_output_options.mapq"); return FLX_ERR_INVALID; }
    auto const pieces = run_pieces(run);
    std::vector<std::vector<PileupJob>> jobs(pieces.size());
    if (!judge_in_parallel(pieces.size(), [&](size_t i) {
            return plan(c, pieces[i]->records.data(), pieces[i]->records.size(), pieces[i]->cigars.data(), pieces[i]->cigars.size(), src.n_reads,
                        [&](u64 r) { return src.length(r); }, who, jobs[i]);
        }))
        return FLX_ERR_INVALID;
    for (size_t i = 0; i < pieces.size(); ++i) {
        int const rc = commit(c, jobs[i], pieces[i]->cigars.data(), src, resident, who);
        if (rc) return rc;
    }
    return FLX_OK;
}

bool reads_given(const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads) { return n_reads == 0 || (read_pool && read_offsets); }

// the copy calls: the object finished and holding a result; the object's lock is taken by the caller afterwards
bool ready_for_copy(const flx_variants* c, const char* who) {
    if (!finished_for_copy(c, who, "flx_variants_finish")) return false;
    if (c->failed) { set_error(std::string(who) + ": flx_variants_finish found 2^32 rows or more: the object holds no result"); return false; }
    return true;
}

// a finished table of `n` rows of `row` bytes into the caller's buffer
int copy_table(flx_variants* c, const DeviceBuffer& table, u64 n, size_t row, void* out, uint64_t capacity, const char* who, const char* what) {
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

extern "C" int flx_variants_create_for_text(int hip_device, const uint8_t* ref_ranks_concat, const uint64_t* ref_lens, uint32_t n_refs, const flx_variants_options* o,
                                            flx_variants** out) {
    if (!out || !ref_ranks_concat) { set_error("flx_variants_create_for_text: null argument"); return FLX_ERR_INVALID; }
    std::vector<u64> starts;
    if (!variants_options_valid(o) || !coverage_lengths_valid(ref_lens, n_refs, "flx_variants_create_for_text", starts)) return FLX_ERR_INVALID;
    if (!errprof_text_valid(ref_ranks_concat, starts.back(), "flx_variants_create_for_text")) return FLX_ERR_INVALID;
    if (hip_device < 0) { set_error("flx_variants_create_for_text: no device given (the host form is flx_variants_host)"); return FLX_ERR_INVALID; }
    auto c = std::make_unique<flx_variants>();       // (an error below drops it: nothing stays allocated)
    u64 const total = starts.back();
    std::vector<u64> const seq_base(starts.begin(), starts.end() - 1);
    int rc = open_planes(c.get(), hip_device, std::move(starts), seq_base, o);
    if (rc) return rc;
    if ((rc = c->own_text.ensure(total, true))) return rc;
    FLX_HIP(hipMemcpyAsync(c->own_text.ptr, ref_ranks_concat, total, hipMemcpyHostToDevice, c->stream));
    FLX_HIP(hipStreamSynchronize(c->stream));
    c->d_text = c->own_text.as<u8>();
    *out = c.release();
    return FLX_OK;
}
extern "C" int flx_variants_create(flx_ctx* ctx, const flx_variants_options* o, flx_variants** out) {
    if (!ctx || !ctx->hidx || !out) { set_error("flx_variants_create: null argument"); return FLX_ERR_INVALID; }
    HostIndex const& H = *ctx->hidx;
    std::vector<u64> starts;
    if (!variants_options_valid(o) || !coverage_lengths_valid(H.seq_len.data(), (uint32_t)H.seq_len.size(), "flx_variants_create", starts)) return FLX_ERR_INVALID;
    if (!ctx->didx.text) { set_error("flx_variants_create: the context holds no text"); return FLX_ERR_INVALID; }
    if (H.text.size() == H.n && !errprof_text_valid(H.text.data(), H.n, "flx_variants_create")) return FLX_ERR_INVALID;      // (an index without its host arrays was checked when it was built)
    auto c = std::make_unique<flx_variants>();
    std::vector<u64> const seq_base(H.seq_start.begin(), H.seq_start.end());     // positions are addressed through the padded starts, as the MD and cs jobs do
    int const rc = open_planes(c.get(), ctx->device, std::move(starts), seq_base, o);
    if (rc) return rc;
    c->d_text = ctx->didx.text;
    { std::lock_guard<std::mutex> g(ctx->spare_mu); ++ctx->live_variants; }
    c->ctx = ctx;
    *out = c.release();
    return FLX_OK;
}
extern "C" void flx_variants_free(flx_variants* c) { free_object(c); }

extern "C" int flx_variants_add_records(flx_variants* c, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words,
                                        const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads) {
    if (!c || (n && !records) || !reads_given(read_pool, read_offsets, n_reads)) { set_error("flx_variants_add_records: null argument"); return FLX_ERR_INVALID; }
    Letters src;
    src.read_pool = read_pool; src.read_offsets = read_offsets; src.n_reads = n_reads;
    std::vector<PileupJob> jobs;
    if (!plan(c, records, n, cigar_words, n_words, n_reads, [&](u64 r) { return src.length(r); }, "flx_variants_add_records", jobs)) return FLX_ERR_INVALID;
    return commit(c, jobs, cigar_words, src, nullptr, "flx_variants_add_records");
}
extern "C" int flx_variants_add_run(flx_variants* c, const flx_run* run, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads) {
    if (!c || !run || !reads_given(read_pool, read_offsets, n_reads)) { set_error("flx_variants_add_run: null argument"); return FLX_ERR_INVALID; }
    Letters src;
    src.read_pool = read_pool; src.read_offsets = read_offsets; src.n_reads = n_reads;
    return add_run(c, run, src, nullptr, "flx_variants_add_run");
}
extern "C" int flx_variants_add_run_resident(flx_variants* c, const flx_run* run, const flx_reads* reads) {
    if (!c || !run || !reads) { set_error("flx_variants_add_run_resident: null argument"); return FLX_ERR_INVALID; }
    Letters src;
    src.batch = reads; src.n_reads = reads->n_reads;
    // the batch's device pool when it lives on this object's device, its host copy through the staged path otherwise
    bool const here = reads->ctx && reads->ctx->device == c->device && reads->d_pool.ptr;
    return add_run(c, run, src, here ? reads : nullptr, "flx_variants_add_run_resident");
}

extern "C" int flx_variants_finish(flx_variants* c) {
    if (!c) { set_error("flx_variants_finish: null argument"); return FLX_ERR_INVALID; }
    std::lock_guard<std::mutex> g(c->mu);
    if (c->finished) { set_error("flx_variants_finish: the variants object is finished"); return FLX_ERR_INVALID; }
    auto const t0 = std::chrono::steady_clock::now();
    FLX_HIP(hipSetDevice(c->device));
    VariantsModel const v = variants_model(c->opt);
    u64 const n = c->n_keys, nt = c->n_tiles();
    u32 passes = 0;
    int rc;
    if ((rc = c->span_begin())) return rc;
    // (a) the sums
    if ((rc = c->scan.inclusive(c->stream, c->plane(PILEUP_DEPTH), c->total)) || (rc = c->scan.inclusive(c->stream, c->plane(PILEUP_DEL), c->total))) return rc;
    // (b) the alleles and, in the INS plane's storage, every anchor's winner; in the eighth plane, every anchor's events
    FLX_HIP(hipMemsetAsync(c->plane(PILEUP_INS), 0xFF, c->stride * 4, c->stream));
    FLX_HIP(hipMemsetAsync(c->plane(VARIANTS_PLANE_EVENTS), 0, c->stride * 4, c->stream));
    if (n) {
        RadixSorter& so = c->sorter;
        if ((rc = so.keys_b.ensure(n * sizeof(SortKey), true)) || (rc = so.pay_a.ensure(n * 4, true)) || (rc = so.pay_b.ensure(n * 4, true)) || (rc = c->ids.ensure(n * 4, true)) ||
            (rc = c->run_start.ensure(n * 4, true)) || (rc = c->run_end.ensure(n * 4, true)) || (rc = c->key_scan.reserve(n)))
            return rc;
        SortKey* sorted;
        u32* payload;
        FLX_LAUNCH("sort_iota", SortDevice::iota(c->stream, so.pay_a.as<u32>(), n));
        if ((rc = so.sort(c->stream, c->keys.as<SortKey>(), so.keys_b.as<SortKey>(), so.pay_a.as<u32>(), so.pay_b.as<u32>(), n, &sorted, &payload, &passes))) return rc;
        u32* const ids = c->ids.as<u32>();
        FLX_LAUNCH("consensus_allele_heads", ConsensusDevice::allele_heads(c->stream, sorted, n, ids));
        if ((rc = c->key_scan.inclusive(c->stream, ids, n))) return rc;
        FLX_LAUNCH("consensus_allele_fill", ConsensusDevice::allele_fill(c->stream, sorted, ids, n, c->run_start.as<u32>(), c->run_end.as<u32>()));
        u32 last = 0;
        FLX_HIP(hipMemcpyAsync(&last, ids + (n - 1), 4, hipMemcpyDeviceToHost, c->stream));
        FLX_HIP(hipStreamSynchronize(c->stream));
        c->n_alleles = last;
        if (last) {
            if ((rc = c->alleles.ensure((u64)last * sizeof(flx_variant_allele), true))) return rc;
            FLX_LAUNCH("variants_anchor_winners", VariantsDevice::anchor_winners(c->stream, sorted, c->run_start.as<u32>(), c->run_end.as<u32>(), last, c->d_starts.as<u32>(),
                                                                                 c->n_refs(), c->alleles.as<flx_variant_allele>(), c->plane(PILEUP_INS), c->plane(VARIANTS_PLANE_EVENTS)));
        }
    }
    // (c) the call: the rows per tile and all rows, then the rows themselves
    FLX_HIP(hipMemsetAsync(c->d_n_rows.ptr, 0, 8, c->stream));
    FLX_LAUNCH("variants_call", VariantsDevice::call(c->stream, 0, c->acc.as<u32>(), c->stride, c->total, c->d_starts.as<u32>(), c->n_refs(), c->d_text, c->text_delta.as<i64>(),
                                                     c->alleles.as<flx_variant_allele>(), v, c->count.as<u32>(), c->d_n_rows.as<unsigned long long>(), nullptr));
    if ((rc = c->scan.inclusive(c->stream, c->count.as<u32>(), nt))) return rc;
    u32 last = 0;
    unsigned long long n_rows = 0;
    FLX_HIP(hipMemcpyAsync(&last, c->count.as<u32>() + (nt - 1), 4, hipMemcpyDeviceToHost, c->stream));
    FLX_HIP(hipMemcpyAsync(&n_rows, c->d_n_rows.ptr, 8, hipMemcpyDeviceToHost, c->stream));
    FLX_HIP(hipStreamSynchronize(c->stream));
    c->finished = true;                                  // (the planes are scanned: there is no way back to adding)
    c->failed = true;                                    // (until the rows stand)
    if (n_rows >= VARIANTS_MAX_ROWS) {
        set_error("flx_variants_finish: " + std::to_string(n_rows) + " rows, 2^32 or more");
        return FLX_ERR_CAPACITY;
    }
    if (n_rows != last) { set_error("flx_variants_finish: the rows' scan and their count disagree"); return FLX_ERR_INTERNAL; }
    c->n_rows = n_rows;
    if ((rc = c->rows.ensure(std::max<u64>(n_rows, 1) * sizeof(flx_variant), true))) return rc;
    if (n_rows)
        FLX_LAUNCH("variants_call", VariantsDevice::call(c->stream, 1, c->acc.as<u32>(), c->stride, c->total, c->d_starts.as<u32>(), c->n_refs(), c->d_text, c->text_delta.as<i64>(),
                                                         c->alleles.as<flx_variant_allele>(), v, c->count.as<u32>(), c->d_n_rows.as<unsigned long long>(), c->rows.as<flx_variant>()));
    if ((rc = c->span_end())) return rc;
    FLX_HIP(hipStreamSynchronize(c->stream));
    c->failed = false;
    // what only the finish needed
    c->keys.release(); c->sorter.release(); c->ids.release(); c->run_start.release(); c->run_end.release();
    c->jobs.release(); c->key_off.release(); c->words.release(); c->letters.release(); c->acc.release();
    c->key_capacity = 0;
    if (c->profile) {
        float ms;
        if ((rc = c->span_ms(ms))) return rc;
        fprintf(stderr, "[flx variants] finish: positions %llu events %llu passes %u alleles %llu rows %llu finish_device_ms %.3f wall_ms %.3f\n", (unsigned long long)c->total,
                (unsigned long long)n, passes, (unsigned long long)c->n_alleles, (unsigned long long)c->n_rows, (double)ms,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    return FLX_OK;
}

extern "C" uint64_t flx_variants_num_rows(const flx_variants* c) {
    if (!c) return 0;
    std::lock_guard<std::mutex> g(const_cast<flx_variants*>(c)->mu);
    return c->finished && !c->failed ? c->n_rows : 0;
}
extern "C" int flx_variants_copy_rows(const flx_variants* cc, flx_variant* out, uint64_t capacity) {
    if (!ready_for_copy(cc, "flx_variants_copy_rows")) return FLX_ERR_INVALID;
    flx_variants* const c = const_cast<flx_variants*>(cc);
    return copy_table(c, c->rows, c->n_rows, sizeof(flx_variant), out, capacity, "flx_variants_copy_rows", "rows");
}
extern "C" uint64_t flx_variants_num_alleles(const flx_variants* c) {
    if (!c) return 0;
    std::lock_guard<std::mutex> g(const_cast<flx_variants*>(c)->mu);
    return c->finished && !c->failed ? c->n_alleles : 0;
}
extern "C" int flx_variants_copy_alleles(const flx_variants* cc, flx_variant_allele* out, uint64_t capacity) {
    if (!ready_for_copy(cc, "flx_variants_copy_alleles")) return FLX_ERR_INVALID;
    flx_variants* const c = const_cast<flx_variants*>(cc);
    return copy_table(c, c->alleles, c->n_alleles, sizeof(flx_variant_allele), out, capacity, "flx_variants_copy_alleles", "alleles");
}

extern "C" int flx_variants_geometry(uint32_t out[4]) {
    if (!out) { set_error("flx_variants_geometry: null argument"); return FLX_ERR_INVALID; }
    out[0] = VariantsDevice::KEYS_GRID_CAP; out[1] = VariantsDevice::KEYS_WAVES; out[2] = CONSENSUS_MAX_INS; out[3] = VARIANTS_DEFAULT_MAX_DEL;
    return FLX_OK;
}

extern "C" int flx_variants_genotype(const flx_variants_options* o, uint64_t ref_n, uint64_t alt_n, uint64_t oth, uint32_t out[8]) {
    if (!out) { set_error("flx_variants_genotype: null argument"); return FLX_ERR_INVALID; }
    if (!variants_options_valid(o)) return FLX_ERR_INVALID;
    if (ref_n >> 34 || alt_n >> 34 || oth >> 34) { set_error("flx_variants_genotype: a count of 2^34 or more"); return FLX_ERR_INVALID; }
    VariantsModel const v = variants_model(variants_options_or_default(o));
    VariantGenotype const g = variants_genotype(ref_n, alt_n, oth, v);
    out[0] = g.gt; out[1] = g.gq; out[2] = g.qual; out[3] = g.pl[0]; out[4] = g.pl[1]; out[5] = g.pl[2];
    out[6] = variants_row_stands(g, ref_n + alt_n + oth, v) ? 1u : 0u;
    out[7] = 0;
    return FLX_OK;
}

extern "C" int flx_variants_host(const uint8_t* ref_ranks_concat, const uint64_t* ref_lens, uint32_t n_refs, const flx_variants_options* o, const flx_record* records,
                                 uint64_t n, const uint32_t* cigar_words, uint64_t n_words, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads,
                                 flx_variant* rows, uint64_t* n_rows, flx_variant_allele* alleles, uint64_t* n_alleles) {
    std::vector<u64> starts;
    if (!variants_options_valid(o) || !coverage_lengths_valid(ref_lens, n_refs, "flx_variants_host", starts)) return FLX_ERR_INVALID;
    if (!ref_ranks_concat || !n_rows || !n_alleles || (n && !records) || !reads_given(read_pool, read_offsets, n_reads)) {
        set_error("flx_variants_host: null argument");
        return FLX_ERR_INVALID;
    }
    if (!errprof_text_valid(ref_ranks_concat, starts.back(), "flx_variants_host")) return FLX_ERR_INVALID;
    flx_variants_options const opt = variants_options_or_default(o);
    VariantsModel const v = variants_model(opt);
    std::vector<PileupJob> jobs;
    if (!pileup_plan(starts, variants_filter(opt), records, n, cigar_words, n_words, n_reads, [&](u64 r) { return read_offsets[r + 1] - read_offsets[r]; }, "flx_variants_host", jobs))
        return FLX_ERR_INVALID;
    u64 const total = starts.back();
    std::vector<uint32_t> counts((size_t)PILEUP_PLANES * total, 0);
    std::vector<SortKey> keys;
    for (auto const& j : jobs) {
        const uint8_t* const read = read_pool + read_offsets[j.read_index];
        u64 const len = read_offsets[j.read_index + 1] - read_offsets[j.read_index];
        pileup_walk(j, cigar_words, read, len, counts.data(), total);
        variants_job_keys(j, cigar_words, read, len, v.max_del, keys);
    }
    if (keys.size() > VARIANTS_MAX_EVENTS) { set_error("flx_variants_host: more than 2^32 - 1 insertion and deletion events"); return FLX_ERR_CAPACITY; }
    VariantsResult res;
    if (!variants_finish_host(starts, ref_ranks_concat, counts.data(), keys, v, res)) {
        set_error("flx_variants_host: 2^32 rows or more");
        return FLX_ERR_CAPACITY;
    }
    u64 const cap_rows = *n_rows, cap_alleles = *n_alleles;
    *n_rows = res.rows.size(); *n_alleles = res.alleles.size();
    if (res.rows.size() > cap_rows || res.alleles.size() > cap_alleles || (!res.rows.empty() && !rows) || (!res.alleles.empty() && !alleles)) {
        set_error("flx_variants_host: a buffer is too small: " + std::to_string(res.rows.size()) + " rows, " + std::to_string(res.alleles.size()) + " alleles");
        return FLX_ERR_CAPACITY;
    }
    if (!res.rows.empty()) memcpy(rows, res.rows.data(), res.rows.size() * sizeof(flx_variant));
    if (!res.alleles.empty()) memcpy(alleles, res.alleles.data(), res.alleles.size() * sizeof(flx_variant_allele));
    return FLX_OK;
}
