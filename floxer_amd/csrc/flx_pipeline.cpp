// Read batches and whole runs behind the C ABI (seam 3): upload of a batch, the cut of a batch into chunks that the context's lanes
// align (flx_verify.cpp) with --threads 1 record order (parallelization.cpp:14-43, 230-276; output.cpp:49-108), and the result object.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>

#include "flx_fm_core.hpp"
#include "flx_partial.hpp"
#include "flx_pipeline.hpp"
#include "flx_select.hpp"
#include "flx_tails.hpp"
#include "flx_leftalign.hpp"
#include "flx_realign.hpp"
#include "flx_cs.hpp"

using namespace flx;

extern "C" void flx_params_default(flx_params* p) {
    memset(p, 0, sizeof(*p));
    p->query_error_probability = -1.0;
    p->pex_seed_num_errors = 2;
    p->search.max_num_anchors_hard = 500;
    p->search.max_num_anchors_soft = 50;
    p->search.anchor_group_order = FLX_ORDER_COUNT_FIRST;
    p->search.anchor_choice_strategy = FLX_CHOICE_ROUND_ROBIN;
    p->search.erase_useless_anchors = 1;
    p->seed_sampling_step_size = 1;
    p->extra_verification_ratio = 0.05;
    p->num_anchors_per_verification_task = 3000;
}

namespace flx {
void take_spare_read_buffer(flx_ctx* ctx, int role, DeviceBuffer& buf) {
    if (buf.ptr) return;
    std::lock_guard<std::mutex> g(ctx->spare_mu);
    auto& v = ctx->spare_read_buffers[role];
    if (v.empty()) return;
    size_t best = 0;
    for (size_t i = 1; i < v.size(); ++i) if (v[i]->cap > v[best]->cap) best = i;
    buf.take(*v[best]);
    v.erase(v.begin() + (long)best);
}
void keep_spare_read_buffer(flx_ctx* ctx, int role, DeviceBuffer& buf) {
    if (!buf.ptr) return;
    {
        std::lock_guard<std::mutex> g(ctx->spare_mu);
        auto& v = ctx->spare_read_buffers[role];
        if (v.size() < 6) {                               // (as many batches as a caller keeps in flight, and a few)
            v.emplace_back(new DeviceBuffer());
            v.back()->take(buf);
            return;
        }
    }
    buf.release();
}
}  // namespace flx

extern "C" int flx_reads_upload(flx_ctx* ctx, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads, flx_reads** out) {
    if (!ctx || !out || (n_reads && (!read_pool || !read_offsets))) { set_error("flx_reads_upload: null argument"); return FLX_ERR_INVALID; }
    FLX_HIP(hipSetDevice(ctx->device));
    auto rd = std::make_unique<flx_reads>();
    rd->ctx = ctx;
    rd->n_reads = n_reads;
    rd->lens.resize(n_reads);
    rd->pool_off.resize(n_reads);
    rd->flags.assign(n_reads, 0);
    u64 total = 0;
    for (u64 i = 0; i < n_reads; ++i) {
        if (read_offsets[i + 1] < read_offsets[i]) { set_error("read offsets must be non-decreasing"); return FLX_ERR_INVALID; }
        rd->lens[i] = read_offsets[i + 1] - read_offsets[i];
        total += 2 * rd->lens[i];
    }
    rd->pool.resize(total);
    {
        u64 off = 0;
        for (u64 i = 0; i < n_reads; ++i) { rd->pool_off[i] = off; off += 2 * rd->lens[i]; }
    }
    // forward copy, reverse complement and symbol classes of every read, on several threads for large batches (a 16384-read batch is
    // 330 MB of pool: 80 ms on one thread, inside the clock of a caller that hands reads over in host memory)
    std::atomic<bool> bad_rank{false};
    auto fill = [&](u64 r0, u64 r1) {
        for (u64 i = r0; i < r1; ++i) {
            u64 const len = rd->lens[i], off = rd->pool_off[i];
            const u8* src = read_pool + read_offsets[i];
            u8 seen = 0;                                   // bit r: rank r occurs
            for (u64 b = 0; b < len; ++b) seen |= (u8)(1u << (src[b] < 6 ? src[b] : 7));
            if (seen & 0x80) { bad_rank = true; return; }
            rd->flags[i] = (u8)(((seen & 1) ? SEED_HAS_DELIM : 0) | ((seen & 0x21) ? SEED_NOT_ACGT : 0));
            memcpy(rd->pool.data() + off, src, len);
            reverse_complement(src, len, rd->pool.data() + off + len);
        }
    };
    unsigned const n_threads = total >= (8u << 20) ? std::min<unsigned>(8u, std::max(1u, std::thread::hardware_concurrency() / 2)) : 1u;
    if (n_threads <= 1) fill(0, n_reads);
    else {
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < n_threads; ++t) pool.emplace_back(fill, n_reads * t / n_threads, n_reads * (t + 1) / n_threads);
        for (auto& th : pool) th.join();
    }
    if (bad_rank) { set_error("read rank > 5"); return FLX_ERR_INVALID; }
    take_spare_read_buffer(ctx, 0, rd->d_pool);
    int rc = rd->d_pool.ensure(total + 256);
    if (rc) return rc;
    hipStream_t const s0 = ctx->external_stream ? ctx->lane0()->stream : ctx->upload_stream;
    if (total) FLX_HIP(hipMemcpyAsync(rd->d_pool.ptr, rd->pool.data(), total, hipMemcpyHostToDevice, s0));
    FLX_HIP(hipMemsetAsync((char*)rd->d_pool.ptr + total, 0, 192, s0));
    FLX_HIP(hipStreamSynchronize(s0));
    { std::lock_guard<std::mutex> g(ctx->spare_mu); ++ctx->live_reads; }
    *out = rd.release();
    return FLX_OK;
}

// (the batch's device buffers go back to the context for the next batch without a device-wide wait: every run on the batch must have
// returned before it is freed, and the context outlives it - flx_ctx_destroy refuses while a batch is alive)
extern "C" void flx_reads_free(flx_reads* reads) {
    if (!reads) return;
    if (reads->ctx) (void)hipSetDevice(reads->ctx->device);
    if (reads->ctx) {
        { std::lock_guard<std::mutex> g(reads->ctx->spare_mu); --reads->ctx->live_reads; }
        keep_spare_read_buffer(reads->ctx, 0, reads->d_pool);
        keep_spare_read_buffer(reads->ctx, 1, reads->d_pack);
        keep_spare_read_buffer(reads->ctx, 2, reads->d_peq);
        keep_spare_read_buffer(reads->ctx, 3, reads->d_pool_rev);
        keep_spare_read_buffer(reads->ctx, 4, reads->d_peq_rev);
    }
    reads->d_pool.release();
    reads->d_pack.release();
    reads->d_peq.release();
    reads->d_pool_rev.release();
    reads->d_peq_rev.release();
    if (reads->peq_event) (void)hipEventDestroy(reads->peq_event);
    if (reads->rev_event) (void)hipEventDestroy(reads->rev_event);
    delete reads;
}

extern "C" int flx_align_reads(flx_ctx* ctx, const flx_params* P, const uint8_t* read_pool, const uint64_t* read_offsets,
                               uint64_t n_reads, flx_run** out) {
    return flx_align_reads_with_options(ctx, P, read_pool, read_offsets, n_reads, nullptr, out);
}
extern "C" int flx_align_reads_with_options(flx_ctx* ctx, const flx_params* P, const uint8_t* read_pool, const uint64_t* read_offsets,
                                            uint64_t n_reads, const flx_output_options* O, flx_run** out) {
    return flx_align_reads_with_tags(ctx, P, read_pool, read_offsets, n_reads, O, nullptr, out);
}
// md and the partial alignments need the trace: refused together with without_cigar, before any work
static bool run_options_valid(const flx_params* P, const flx_run_options* R, const flx_split_options* S, const flx_gap_options* G, const flx_realign_options* A,
                              const flx_cs_options* C) {
    if (!cs_options_valid(C) || !gap_options_valid(G) || !realign_options_valid(A)) return false;
    if (cs_options_form(C) && P && P->without_cigar) { set_error("flx_cs_options.form needs the CIGAR's trace: it cannot be combined with without_cigar"); return false; }
    if (realign_options_active(A) && P && P->without_cigar) { set_error("flx_realign_options.enable needs the CIGAR's trace: it cannot be combined with without_cigar"); return false; }
    if (gap_options_active(G) && P && P->without_cigar) { set_error("flx_gap_options.left_align needs the CIGAR's trace: it cannot be combined with without_cigar"); return false; }
    if (!split_options_valid(S)) return false;
    if (split_options_active(S)) {
        if (P && P->without_cigar) { set_error("flx_split_options.enable needs the CIGAR's trace: it cannot be combined with without_cigar"); return false; }
        if (!R || !partial_options_active(R->partial)) { set_error("flx_split_options.enable writes partial records: it needs flx_partial_options.enable"); return false; }
        if (!R->output || R->output->max_alignments_per_read != 1) { set_error("flx_split_options.enable judges the primary: it needs flx_output_options.max_alignments_per_read == 1"); return false; }
    }
    if (!R) return true;
    for (const void* r : R->reserved) if (r) { set_error("flx_run_options: the reserved pointers must be NULL"); return false; }
    if (!output_options_valid(R->output) || !tag_options_valid(R->tags) || !partial_options_valid(R->partial) || !extend_options_valid(R->extend)) return false;
    if (R->tags && R->tags->md && P && P->without_cigar) { set_error("flx_tag_options.md needs the CIGAR's trace: it cannot be combined with without_cigar"); return false; }
    if (partial_options_active(R->partial) && P && P->without_cigar) { set_error("flx_partial_options.enable needs the CIGAR's trace: it cannot be combined with without_cigar"); return false; }
    if (extend_options_active(R->extend) && !partial_options_active(R->partial)) { set_error("flx_extend_options.enable extends partial records: it needs flx_partial_options.enable"); return false; }
    return true;
}
extern "C" int flx_align_reads_with_tags(flx_ctx* ctx, const flx_params* P, const uint8_t* read_pool, const uint64_t* read_offsets,
                                         uint64_t n_reads, const flx_output_options* O, const flx_tag_options* T, flx_run** out) {
    flx_run_options const R{O, T, nullptr, nullptr, {}};
    return flx_align_reads_opt(ctx, P, read_pool, read_offsets, n_reads, &R, out);
}
extern "C" int flx_align_reads_opt(flx_ctx* ctx, const flx_params* P, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads,
                                   const flx_run_options* R, flx_run** out) {
    return flx_align_reads_split(ctx, P, read_pool, read_offsets, n_reads, R, nullptr, out);
}
extern "C" int flx_align_reads_split(flx_ctx* ctx, const flx_params* P, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads,
                                     const flx_run_options* R, const flx_split_options* S, flx_run** out) {
    return flx_align_reads_gaps(ctx, P, read_pool, read_offsets, n_reads, R, S, nullptr, out);
}
extern "C" int flx_align_reads_gaps(flx_ctx* ctx, const flx_params* P, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads,
                                    const flx_run_options* R, const flx_split_options* S, const flx_gap_options* G, flx_run** out) {
    return flx_align_reads_realign(ctx, P, read_pool, read_offsets, n_reads, R, S, G, nullptr, out);
}
extern "C" int flx_align_reads_realign(flx_ctx* ctx, const flx_params* P, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads,
                                       const flx_run_options* R, const flx_split_options* S, const flx_gap_options* G, const flx_realign_options* A,
                                       flx_run** out) {
    return flx_align_reads_cs(ctx, P, read_pool, read_offsets, n_reads, R, S, G, A, nullptr, out);
}
extern "C" int flx_align_reads_cs(flx_ctx* ctx, const flx_params* P, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads,
                                  const flx_run_options* R, const flx_split_options* S, const flx_gap_options* G, const flx_realign_options* A,
                                  const flx_cs_options* C, flx_run** out) {
    if (!run_options_valid(P, R, S, G, A, C)) return FLX_ERR_INVALID;
    flx_reads* rd = nullptr;
    int rc = flx_reads_upload(ctx, read_pool, read_offsets, n_reads, &rd);
    if (rc) return rc;
    rc = flx_align_reads_resident_cs(ctx, P, rd, R, S, G, A, C, out);
    flx_reads_free(rd);
    return rc;
}

extern "C" int flx_align_reads_resident(flx_ctx* ctx, const flx_params* P, const flx_reads* RD, flx_run** out) {
    return flx_align_reads_resident_with_options(ctx, P, RD, nullptr, out);
}
extern "C" int flx_align_reads_resident_with_options(flx_ctx* ctx, const flx_params* P, const flx_reads* RD, const flx_output_options* O,
                                                     flx_run** out) {
    return flx_align_reads_resident_with_tags(ctx, P, RD, O, nullptr, out);
}
extern "C" int flx_align_reads_resident_with_tags(flx_ctx* ctx, const flx_params* P, const flx_reads* RD, const flx_output_options* O,
                                                  const flx_tag_options* T, flx_run** out) {
    flx_run_options const R{O, T, nullptr, nullptr, {}};
    return flx_align_reads_resident_opt(ctx, P, RD, &R, out);
}
extern "C" int flx_align_reads_resident_opt(flx_ctx* ctx, const flx_params* P, const flx_reads* RD, const flx_run_options* R, flx_run** out) {
    return flx_align_reads_resident_split(ctx, P, RD, R, nullptr, out);
}
extern "C" int flx_align_reads_resident_split(flx_ctx* ctx, const flx_params* P, const flx_reads* RD, const flx_run_options* R,
                                              const flx_split_options* S, flx_run** out) {
    return flx_align_reads_resident_gaps(ctx, P, RD, R, S, nullptr, out);
}
extern "C" int flx_align_reads_resident_gaps(flx_ctx* ctx, const flx_params* P, const flx_reads* RD, const flx_run_options* R,
                                             const flx_split_options* S, const flx_gap_options* G, flx_run** out) {
    return flx_align_reads_resident_realign(ctx, P, RD, R, S, G, nullptr, out);
}
extern "C" int flx_align_reads_resident_realign(flx_ctx* ctx, const flx_params* P, const flx_reads* RD, const flx_run_options* R,
                                                const flx_split_options* S, const flx_gap_options* G, const flx_realign_options* A, flx_run** out) {
    return flx_align_reads_resident_cs(ctx, P, RD, R, S, G, A, nullptr, out);
}
extern "C" int flx_align_reads_resident_cs(flx_ctx* ctx, const flx_params* P, const flx_reads* RD, const flx_run_options* R, const flx_split_options* S,
                                           const flx_gap_options* G, const flx_realign_options* A, const flx_cs_options* C, flx_run** out) {
    if (!run_options_valid(P, R, S, G, A, C)) return FLX_ERR_INVALID;
    RunOptions opt{};                            // (a NULL bundle, a NULL member and a zeroed struct are the same: that option is off)
    if (R && R->output) opt.output = *R->output;
    if (R && R->tags) opt.tags = *R->tags;
    if (R && R->partial) opt.partial = *R->partial;
    if (R && R->extend) opt.extend = *R->extend;
    if (S) opt.split = *S;
    if (G) opt.gaps = *G;
    if (realign_options_active(A)) opt.realign = *A;
    if (C) opt.cs = *C;
    if (!ctx || !P || !out || !RD || RD->ctx != ctx) { set_error("flx_align_reads_resident: null argument or reads of another context"); return FLX_ERR_INVALID; }
    FLX_HIP(hipSetDevice(ctx->device));
    if (P->query_error_probability < 0 && P->query_num_errors < P->pex_seed_num_errors) { set_error("query errors must be >= seed errors (floxer_cli.cpp:180)"); return FLX_ERR_INVALID; }
    if (P->pex_seed_num_errors > 3 || P->seed_sampling_step_size == 0 || P->num_anchors_per_verification_task == 0) { set_error("invalid parameters"); return FLX_ERR_INVALID; }
    if (P->search.max_num_anchors_hard < P->search.max_num_anchors_soft) { set_error("max-anchors-hard must not be smaller than max-anchors-soft"); return FLX_ERR_INVALID; }
    u64 const n_reads = RD->n_reads;
    PhaseTimer dprof("dispatch");
    auto run = std::make_unique<flx_run>();
    run->skipped.assign(n_reads, 0);
    run->has_md = opt.tags.md;
    run->has_scores = opt.realign.enable != 0;
    run->realign = opt.realign;
    run->has_cs = opt.cs.form != 0;
    run->has_mapq = opt.output.mapq != 0;
    if (n_reads == 0) { *out = run.release(); return FLX_OK; }       // an empty batch is an empty run
    // reads are independent units (parallelization.cpp:77-87): the batch is cut into contiguous chunks and every lane (a host
    // thread with its own stream and workspaces) takes the next chunk when it is done with its last one.
    size_t n_lanes = ctx->external_stream ? 1 : ctx->lanes.size();
    n_lanes = std::max<size_t>(1, std::min<size_t>(n_lanes, (n_reads + 63) / 64));
    // a chunk's kernels last as long as their longest job whatever the number of jobs, and a launch is the more efficient the
    // more jobs it has, so chunks are large: one per lane up to 2048 reads, more than one per lane beyond that
    // (a batch that gives every lane 1024 reads or more is cut into 2048-read chunks, batches overlap, see acquire_lane; with the
    // interval optimisation 1024-read chunks were better while the rounds' bookkeeping was host work: 2048 now, 78 k -> 83 k reads/s)
    u64 const big_chunk = 2048;
    u64 chunk_reads = n_reads >= 1024 * n_lanes ? big_chunk : std::max<u64>(64, (n_reads + n_lanes - 1) / n_lanes);
    if (const char* env = getenv("FLX_CHUNK_READS")) { u64 const v = strtoull(env, nullptr, 10); if (v >= 1) chunk_reads = v; }
    if (n_lanes == 1) chunk_reads = std::max<u64>(n_reads, 1);
    // A chunk's workspaces grow with its bases, not its reads (seeds, hits, requests, trace arena; with first_reported also the DFS
    // stacks of the ordered K1, ~100 bytes per read base): chunks are also cut at FLX_CHUNK_BASES read bases (default 48 M), so a
    // batch of 100-kb reads gets more, smaller chunks instead of workspaces of tens of GB per lane.
    u64 chunk_bases = 48ull << 20;
    if (const char* env = getenv("FLX_CHUNK_BASES")) { u64 const v = strtoull(env, nullptr, 10); if (v >= 1) chunk_bases = v; }
    hvec<u64> chunk_first{0};                                // chunk c = reads [chunk_first[c], chunk_first[c + 1])
    {
        u64 reads_in = 0, bases_in = 0;
        for (u64 i = 0; i < n_reads; ++i) {
            u64 const len = RD->lens[i];
            if (reads_in > 0 && (reads_in >= chunk_reads || bases_in + len > chunk_bases)) { chunk_first.push_back(i); reads_in = 0; bases_in = 0; }
            ++reads_in;
            bases_in += len;
        }
        chunk_first.push_back(n_reads);
    }
    size_t const n_chunks = chunk_first.size() - 1;
    run->parts.resize(n_chunks);
    hvec<flx_run>& parts = run->parts;
    hvec<int> rcs(n_chunks, FLX_OK);
    std::vector<std::string> errs(n_chunks);
    {
        std::lock_guard<std::mutex> g(RD->peq_mu);
        if (!RD->peq_built && n_reads) {
            LaneLease lease(ctx, ctx->external_stream ? 0 : -1);
            take_spare_read_buffer(ctx, 2, RD->d_peq);
            take_spare_read_buffer(ctx, 1, RD->d_pack);
            int const rc = build_peq(lease.lane, RD->d_pool.as<u8>(), RD->pool.size(), RD->d_peq);
            if (rc) return rc;
            if (ctx->didx.filter) {
                int const rc2 = RD->d_pack.ensure(pack_words_for(RD->pool.size()) * 4 + 64);
                if (rc2) return rc2;
                int const e = DeviceApi::pack_pool(lease.lane->stream, RD->d_pool.as<u8>(), RD->pool.size(), RD->d_pack.as<u32>());
                if (e) { set_error(std::string("pack_pool: ") + hipGetErrorString((hipError_t)e)); return FLX_ERR_NO_DEVICE; }
            }
            if (!RD->peq_event) FLX_HIP(hipEventCreateWithFlags(&RD->peq_event, hipEventDisableTiming));
            FLX_HIP(hipEventRecord(RD->peq_event, lease.lane->stream));
            RD->peq_built = true;
        }
    }
    std::atomic<size_t> next_chunk{0};
    std::atomic<bool> failed{false};
    auto work = [&]() {
        for (size_t c; (c = next_chunk.fetch_add(1)) < n_chunks && !failed.load();) {
            u64 const a = chunk_first[c], b = chunk_first[c + 1];
            parts[c].skipped.assign(n_reads, 0);
            LaneLease lease(ctx, ctx->external_stream ? 0 : -1);      // waits while other calls on this context hold all lanes
            rcs[c] = align_slice(lease.lane, P, opt, RD, a, b, &parts[c]);
            if (rcs[c]) { errs[c] = flx_last_error(); failed.store(true); }
            else { lease.lane->has_run = true; if (!ctx->external_stream) ctx->warm_one_cold_lane(lease.lane); }
        }
    };
    size_t const n_workers = std::min(n_lanes, n_chunks);
    if (n_workers == 1) work();
    else {
        std::vector<std::thread> threads;
        for (size_t l = 0; l < n_workers; ++l) threads.emplace_back(work);
        for (auto& t : threads) t.join();
    }
    dprof.mark("lanes");
    for (size_t c = 0; c < n_chunks; ++c)
        if (rcs[c]) { set_error(errs[c]); return rcs[c]; }
    for (auto& p : parts)
        for (u64 i = 0; i < n_reads; ++i) run->skipped[i] |= p.skipped[i];
    *out = run.release();
    dprof.mark("merge");
    return FLX_OK;
}

extern "C" uint64_t flx_run_num_records(const flx_run* run) {
    if (!run) return 0;
    uint64_t n = run->records.size();
    for (auto const& p : run->parts) n += p.records.size();
    return n;
}
extern "C" uint64_t flx_run_num_cigar_words(const flx_run* run) {
    if (!run) return 0;
    uint64_t n = run->cigars.size();
    for (auto const& p : run->parts) n += p.cigars.size();
    return n;
}
extern "C" int flx_run_copy(const flx_run* run, flx_record* records, uint32_t* cigar_words, uint8_t* skipped) {
    if (!run) { set_error("null run"); return FLX_ERR_INVALID; }
    PhaseTimer cprof("run_copy");
    // the run itself plus its per-lane parts, each copied by its own thread (the CIGAR pools are tens of MB per part)
    hvec<const flx_run*> pieces{run};
    for (auto const& p : run->parts) pieces.push_back(&p);
    hvec<uint64_t> rec_base(pieces.size()), cig_base(pieces.size());
    uint64_t rb = 0, cb = 0;
    for (size_t i = 0; i < pieces.size(); ++i) { rec_base[i] = rb; cig_base[i] = cb; rb += pieces[i]->records.size(); cb += pieces[i]->cigars.size(); }
    auto emit = [&](size_t i) {
        flx_run const& part = *pieces[i];
        if (records) for (size_t r = 0; r < part.records.size(); ++r) { records[rec_base[i] + r] = part.records[r]; records[rec_base[i] + r].cigar_offset += cig_base[i]; }
        if (cigar_words && !part.cigars.empty()) memcpy(cigar_words + cig_base[i], part.cigars.data(), part.cigars.size() * 4);
    };
    if (pieces.size() <= 2) for (size_t i = 0; i < pieces.size(); ++i) emit(i);
    else {
        size_t const n_threads = std::min<size_t>(8, pieces.size());
        std::vector<std::thread> threads;
        for (size_t t = 0; t < n_threads; ++t)
            threads.emplace_back([&, t] { for (size_t i = t; i < pieces.size(); i += n_threads) emit(i); });
        for (auto& t : threads) t.join();
    }
    if (skipped && !run->skipped.empty()) memcpy(skipped, run->skipped.data(), run->skipped.size());
    cprof.mark("copy");
    return FLX_OK;
}
extern "C" uint64_t flx_run_num_md_bytes(const flx_run* run) {
    if (!run) return 0;
    uint64_t n = run->md.size();
    for (auto const& p : run->parts) n += p.md.size();
    return n;
}
// the parts' MD offsets are rebased onto the concatenation of their pools, as flx_run_copy rebases the CIGAR offsets
extern "C" int flx_run_copy_md(const flx_run* run, flx_md_ref* refs, uint8_t* md_bytes) {
    if (!run) { set_error("null run"); return FLX_ERR_INVALID; }
    if (!run->has_md) { set_error("flx_run_copy_md: the run was made without flx_tag_options.md"); return FLX_ERR_INVALID; }
    uint64_t rb = 0, mb = 0;
    auto emit = [&](flx_run const& part) {
        if (refs) for (size_t r = 0; r < part.md_refs.size(); ++r) { refs[rb + r] = part.md_refs[r]; if (part.md_refs[r].length) refs[rb + r].offset += mb; }
        if (md_bytes && !part.md.empty()) memcpy(md_bytes + mb, part.md.data(), part.md.size());
        rb += part.records.size();
        mb += part.md.size();
    };
    emit(*run);
    for (auto const& p : run->parts) emit(p);
    return FLX_OK;
}
extern "C" uint64_t flx_run_num_cs_bytes(const flx_run* run) {
    if (!run) return 0;
    uint64_t n = run->cs.size();
    for (auto const& p : run->parts) n += p.cs.size();
    return n;
}
// the parts' cs offsets are rebased onto the concatenation of their pools, as flx_run_copy_md rebases the MD offsets
extern "C" int flx_run_copy_cs(const flx_run* run, flx_md_ref* refs, uint8_t* bytes) {
    if (!run) { set_error("null run"); return FLX_ERR_INVALID; }
    if (!run->has_cs) { set_error("flx_run_copy_cs: the run was made without flx_cs_options.form"); return FLX_ERR_INVALID; }
    uint64_t rb = 0, cb = 0;
    auto emit = [&](flx_run const& part) {
        if (refs) for (size_t r = 0; r < part.cs_refs.size(); ++r) { refs[rb + r] = part.cs_refs[r]; if (part.cs_refs[r].length) refs[rb + r].offset += cb; }
        if (bytes && !part.cs.empty()) memcpy(bytes + cb, part.cs.data(), part.cs.size());
        rb += part.records.size();
        cb += part.cs.size();
    };
    emit(*run);
    for (auto const& p : run->parts) emit(p);
    return FLX_OK;
}
// a record's score is read off its written words: the realigned path's H[m][n] is the score of its own words, and left-alignment, clips
// and the extension of a partial record leave words whose score is again their own
extern "C" int flx_run_copy_scores(const flx_run* run, int32_t* scores) {
    if (!run) { set_error("null run"); return FLX_ERR_INVALID; }
    if (!run->has_scores) { set_error("flx_run_copy_scores: the run was made without flx_realign_options.enable"); return FLX_ERR_INVALID; }
    if (!scores) return FLX_OK;
    RealignScores const s = realign_scores(&run->realign);
    uint64_t rb = 0;
    auto emit = [&](flx_run const& part) {
        for (size_t r = 0; r < part.records.size(); ++r) {
            flx_record const& rec = part.records[r];
            int64_t score = 0;
            if (!(rec.flag & 4u))
                for (uint32_t t = 0; t < rec.cigar_length; ++t) {
                    uint32_t const w = part.cigars[rec.cigar_offset + t], op = w & 15u, len = w >> 4;
                    if (op == 7u) score += (int64_t)s.a * len;
                    else if (op == 8u) score -= (int64_t)s.b * len;
                    else if (op == 1u || op == 2u) score -= s.o + (int64_t)s.e * len;
                }
            scores[rb + r] = (int32_t)std::max<int64_t>(INT32_MIN, std::min<int64_t>(INT32_MAX, score));
        }
        rb += part.records.size();
    };
    emit(*run);
    for (auto const& p : run->parts) emit(p);
    return FLX_OK;
}
extern "C" void flx_run_free(flx_run* run) {
    PhaseTimer fprof("run_free");
    delete run;
    fprof.mark("free");
}
