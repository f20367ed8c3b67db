// What the pieces of the host pipeline share: flx_lane.cpp (buffers, lanes, copies), flx_seeding.cpp (K1/K2 + anchor selection),
// flx_align_jobs.cpp (K0/K3/K4 job batches), flx_traceback.cpp with flx_traceback.hpp (K5 and the passes behind it),
// flx_align_capi.cpp (the C ABI of job batches and of a kernel alone), flx_verify.cpp (one chunk of reads: align_slice and its stages)
// and flx_pipeline.cpp (read batches, chunking over lanes, the C ABI of runs).
#pragma once

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <map>
#include <memory>
#include <mutex>
#include <utility>

#include "flx_context.hpp"
#include "flx_stats.hpp"

// ---- the objects behind the C ABI's opaque handles
struct flx_run {
    flx::hvec<flx_record> records;     // cigar_offset relative to this object's `cigars`
    flx::hvec<flx::u32> cigars;
    flx::hvec<flx::u8> skipped;
    bool has_md = false;               // made with flx_tag_options.md: md_refs is parallel to records, offsets relative to this object's `md`
    flx::hvec<flx_md_ref> md_refs;
    flx::hvec<flx::u8> md;
    bool has_scores = false;           // made with flx_realign_options.enable: `realign` holds the options the records' scores are taken under
    flx_realign_options realign{};
    bool has_cs = false;               // made with flx_cs_options.form != 0: cs_refs is parallel to records, offsets relative to this object's `cs`
    flx::hvec<flx_md_ref> cs_refs;
    flx::hvec<flx::u8> cs;
    bool has_mapq = false;             // made with flx_output_options.mapq: the records' `reserved` holds their mapping quality
    flx::hvec<flx_run> parts;          // a batch result is the in-order list of its slices (no concatenation on the host)
};

struct flx_reads {
    flx_ctx* ctx = nullptr;
    uint64_t n_reads = 0;
    flx::hvec<flx::u64> lens;            // per read
    flx::hvec<flx::u64> pool_off;        // per read: offset of the forward sequence; reverse complement follows at +len
    flx::hvec<flx::u8> pool;             // host copy (forward + reverse complement per read)
    flx::hvec<flx::u8> flags;            // per read: SEED_HAS_DELIM | SEED_NOT_ACGT (flx_fm_core.hpp) when it holds such symbols
    flx::DeviceBuffer d_pool;         // HBM-resident copy
    mutable flx::DeviceBuffer d_pack; // its 2-bit form (K1's presence filter), built with the Peq planes
    // Peq planes of the whole pool (K0), built by the first flx_align_reads_resident call on these reads and shared by all
    // lanes and later calls (they depend on the pool only)
    mutable std::mutex peq_mu;
    mutable bool peq_built = false;
    mutable flx::DeviceBuffer d_peq;
    mutable hipEvent_t peq_event = nullptr;      // recorded behind K0; every lane's stream waits for it before its first DP launch
    // --without-cigar aligns the reversed sequences (alignment.cpp:115-145): the reversed pool and its Peq planes, made by the first
    // chunk that needs them and shared like d_peq
    mutable bool rev_built = false;
    mutable flx::DeviceBuffer d_pool_rev, d_peq_rev;
    mutable hipEvent_t rev_event = nullptr;
};

namespace flx {

// FLX_HOST_PROFILE=1 prints wall-clock milliseconds of the host phases of flx_align_reads_resident to stderr
struct PhaseTimer {
    struct Row { const char* name; double wall, cpu; };
    bool on;
    std::chrono::steady_clock::time_point t;
    double cpu_t = 0;
    hvec<Row> rows;
    const char* what;
    static double thread_cpu_ms() {
        timespec ts{};
        clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
        return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
    }
    explicit PhaseTimer(const char* what_ = "slice") : on(getenv("FLX_HOST_PROFILE") != nullptr), t(std::chrono::steady_clock::now()), what(what_) {
        if (on) cpu_t = thread_cpu_ms();
    }
    void mark(const char* name) {
        if (!on) return;
        auto const now = std::chrono::steady_clock::now();
        double const cpu_now = thread_cpu_ms();
        rows.push_back({name, std::chrono::duration<double, std::milli>(now - t).count(), cpu_now - cpu_t});
        t = now;
        cpu_t = cpu_now;
    }
    ~PhaseTimer() {                                  // name=wall/cpu of the calling thread, milliseconds
        if (!on) return;
        double total = 0, cpu = 0;
        for (auto& r : rows) { total += r.wall; cpu += r.cpu; }
        fprintf(stderr, "[flx host profile] %s total %.2f/%.2f ms:", what, total, cpu);
        for (auto& r : rows) fprintf(stderr, " %s=%.2f/%.2f", r.name, r.wall, r.cpu);
        fprintf(stderr, "\n");
    }
};

// ---- flx_lane.cpp
int h2d(Lane* lane, DeviceBuffer& buf, const void* src, size_t bytes, size_t extra_zero_tail = 0);
int d2h(Lane* lane, void* dst, const void* src, size_t bytes);      // waits for the stream first (the thread sleeps meanwhile)
// upload a byte sequence with TEXT_PAD zero bytes in front and behind; returns pointer to element 0
int upload_padded(Lane* lane, DeviceBuffer& buf, const u8* src, u64 len, const u8** d_first);
// FLX_ALLOC_DEBUG: the address ranges of a lane's workspaces (a GPU memory fault reports an address)
void dump_lane_buffers(Lane& l, const char* when);

// ---- flx_seeding.cpp
struct HostAnchor { u32 seed_index, leaf, ref_id, errors; u64 pos; };
struct SeedStats { u32 useful, raw, excluded_soft, fully_excluded; };

// d_seq_pool_or_null: the pool is resident (then d_qpack_or_null may be its 2-bit form); seed_flags (per seed, SEED_* of
// flx_fm_core.hpp) may be null when the host pool is given (they are read off it)
int search_seeds_device(Lane* lane, const u8* d_seq_pool_or_null, const u8* h_seq_pool, u64 pool_len, const flx_seed* seeds,
                        u64 n_seeds, const flx_search_config& cfg, hvec<HostAnchor>& anchors, hvec<SeedStats>& stats,
                        hvec<DevHit>* raw_hits, u64 raw_max_hits, const u32* d_qpack_or_null = nullptr, const u8* seed_flags = nullptr,
                        const SeedGen* gen = nullptr);
// gen: `seeds` is null and the chunk's seeds are written on the device from this description (their ids = the order the caller would have
// listed them in: read by read, forward then reverse complement, leaf by leaf); the anchors' leaf is left to the caller; returns
// SEARCH_NEEDS_HOST_SEEDS (nothing done that counts) for the forms that read the list (ordered walk, host-side grouping): call again with it.
constexpr int SEARCH_NEEDS_HOST_SEEDS = 1;

// ---- flx_align_jobs.cpp
struct AlignRequest { u64 ref_off, q_off; u32 n, m, k; };
struct TraceResult {
    bool exists = false; u32 nm = 0; u32 begin = 0; u64 cigar_off = 0; u32 cigar_len = 0; u64 md_off = 0; u32 md_len = 0; DevTailOut tail{};
    int32_t score = 0;          // a realigned path (flx_realign.hip): its score; nm is then its num_errors and
    u32 ed = 0;                 // ed the edit distance K4 found (nm without the option)
    u64 cs_off = 0; u32 cs_len = 0;      // its cs string (flx_cs.hip) in the caller's cs pool, when wanted
};
// the values of the tail rule (flx_tails.hpp) for the traces that want it, defaults resolved
struct TailParams { u32 w, x_drop, min_rows; };
// What a trace wants beyond score, begin and CIGAR (default: nothing). Every pass runs behind K5 on each traced path (flx_traceback.hpp).
struct RealignScores;
struct TraceWants {
    hvec<u8>* md_pool = nullptr;             // the MD strings (flx_md.hip), their bytes into this pool (shared by duplicates like the CIGAR words)
    const TailParams* tails = nullptr;       // the paths' tails (flx_tails.hip), in TraceResult::tail
    bool left_align = false;                 // gaps left-aligned (flx_leftalign.hip) before the MD string, cs string and tails are read off them
    const RealignScores* realign = nullptr;  // the paths realigned under these scores (flx_realign.hip) before all of that
    u32 cs_form = 0;                         // the cs strings (flx_cs.hip), form 1 (short) or 2 (long), read off the final words,
    hvec<u8>* cs_pool = nullptr;             // their bytes into this pool
    const u8* d_query = nullptr;             // the device query pool's letters (q_off addresses them as it does the Peq planes): left-align, realign and cs read them
};
// host milliseconds of the host-rounds form, summed over a chunk's rounds (FLX_HOST_PROFILE); owned by the chunk
struct ExistsTimes { double ms[4] = {0, 0, 0, 0}; double build_requests = 0; };      // ms: dedup, cluster, GPU round trip, scatter

u64 round_span_percent();       // a round tests the nodes of [smallest, smallest * span / 100] rows (FLX_ROUND_SPAN overrides the percentage)
u64 align_few_waves();          // FLX_ALIGN_FEW_WAVES overrides the threshold (tests force either form)
// score + end column for every request (no trace)
int run_score_jobs(Lane* lane, const u8* d_text, const u64* d_peq, hvec<AlignRequest> const& reqs, hvec<DevAlignOut>& outs, const char* kernel_name);
// score, begin position and CIGAR for every request (alignment.cpp:147-180); CIGAR words land in cigar_pool (shared by duplicates)
int run_trace_jobs(Lane* lane, const u8* d_text, const u64* d_peq, hvec<AlignRequest> const& reqs, hvec<TraceResult>& results, hvec<u32>& cigar_pool,
                   TraceWants const& wants);
// the same for root windows: anchors of one locus share one DP over the union of their windows
int run_trace_jobs_union(Lane* lane, const u8* d_text, const u64* d_peq, hvec<AlignRequest> const& reqs, hvec<TraceResult>& results, hvec<u32>& cigar_pool,
                         TraceWants const& wants);
// the distinct requests of `reqs` and every request's index among them; the launch shape of every request of one call
void dedup_requests(hvec<AlignRequest> const& reqs, hvec<AlignRequest>& uniq, hvec<u32>& uniq_of);
int choose_shapes(hvec<AlignRequest> const& reqs, hvec<AlignShape>& shapes);
// existence tests of one round: outs[i].score is 0xFFFFFFFF for "no alignment within k"
int run_exists_jobs(Lane* lane, const u8* d_text, const u64* d_peq, hvec<AlignRequest> const& reqs, hvec<DevAlignOut>& outs, ExistsTimes& times);
// extension jobs of partial records' ends (ed_extend, flx_extend.hip): one launch, outs[i] for jobs[i] (out_index is set here)
int run_extend_jobs(Lane* lane, const u8* d_text, const u8* d_query, hvec<DevExtendJob>& jobs, hvec<DevExtendOut>& outs);
int build_peq(Lane* lane, const u8* d_seq, u64 len, DeviceBuffer& peq);
int ensure_reversed_text(Lane* lane);

// ---- flx_pipeline.cpp: device buffers of freed read batches, by role (flx_ctx::spare_read_buffers)
void take_spare_read_buffer(flx_ctx* ctx, int role, DeviceBuffer& buf);      // buf owns the largest kept one afterwards, if there is one
void keep_spare_read_buffer(flx_ctx* ctx, int role, DeviceBuffer& buf);

// ---- flx_verify.cpp: one contiguous slice of a batch on one lane. What the slice carries from stage to stage:
struct ReadState {
    u64 read_index;
    u32 len, k;
    u64 pool_off[2];            // forward, reverse complement
    const PexTree* tree_ptr = nullptr;      // reads of one length share one tree (it depends on (length, errors) only)
    PexTree const& tree_ref() const { return *tree_ptr; }
    hvec<u32> anchor_ids[2];
};

struct AnchorState {
    u32 read;                   // index into kept reads
    u8 orientation;
    u32 leaf, ref_id;
    u64 pos;
    u32 node;                   // inner node under test
    bool alive = true, at_root = false, wants_root = false;
};

struct Span { u64 offset, length, extra; };
// (ed: the edit distance verification found, what the statistics count; nm differs from it on a realigned path only)
struct RootAlignment { bool exists = false; u64 start = 0; u32 nm = 0; u64 cigar_off = 0; u32 cigar_len = 0; u64 md_off = 0; u32 md_len = 0; DevTailOut tail{}; u32 ed = 0; u64 cs_off = 0; u32 cs_len = 0; };

// a record rescue_partials (flx_partial.hpp: a soft-clipped part of a read without a mapped record) or split_tails (flx_tails.hpp: the
// kept part and the tails of a read mapped in full) leaves for write_records
struct PartialRecord {
    u32 read; u32 flag; u32 ref_id; u64 start; u32 nm; u64 cigar_off; u32 cigar_len; u64 md_off; u32 md_len; u32 q_from, q_to; u32 mapq;
    u32 o_from, o_to;           // the traced rows in the oriented sequence (the node, before extend_partials moves them)
    u64 core_off; u32 core_len; // the traced words without the clips
    bool split = false;         // a record of a split read: written instead of the read's root records
    u64 cs_off = 0; u32 cs_len = 0;      // the cs string of the traced words (flx_cs_options)
};

struct Slice {
    // plan_reads
    hvec<ReadState> reads;                                                    // the reads that are not skipped
    std::map<std::pair<u64, u64>, std::unique_ptr<PexTree>> tree_cache;       // (length, errors) -> tree
    // plan_seeds: seed s of the chunk = (read, orientation, leaf) by the reads' seed ranges seed_first[r] .. seed_first[r + 1]
    u64 step = 1;
    hvec<u32> seed_first;
    bool use_gen = false;
    SeedGen gen;                                                              // the seeds as a description the device writes them from, or
    hvec<flx_seed> seeds;                                                     // as a list (the host's selection, statistics, FLX_HOST_SEEDS=1)
    hvec<u8> seed_flags;
    // search_seeds
    hvec<HostAnchor> anchors;                                                 // in seed order
    hvec<SeedStats> sstats;                                                   // per seed
    // anchors_to_reads, verification_order, the climb
    hvec<AnchorState> A;                                                      // one per anchor
    hvec<hvec<u32>> exec_order;                                               // per read: its anchors in verification order
    u64 n_inner_requested = 0;
    // interval_pass: the anchors that align the root, in verification order
    hvec<AlignRequest> root_reqs;
    hvec<u32> root_anchor;
    hvec<Span> root_spans;
    // align_roots
    hvec<RootAlignment> root_res;
    hvec<u32> cig;                                                            // CIGAR pool of root_res
    bool want_md = false;                                                     // flx_tag_options.md: the traced paths' MD strings as well
    bool want_left_align = false;                                             // flx_gap_options.left_align: every traced path's gaps left-aligned
    const RealignScores* realign = nullptr;                                   // flx_realign_options.enable: every traced path realigned under these scores
    hvec<u8> md;                                                              // MD pool of root_res
    u32 cs_form = 0;                                                          // flx_cs_options.form: the traced paths' cs strings as well
    hvec<u8> cs;                                                              // cs pool of root_res
    // split_tails, rescue_partials: the records of the reads they split / rescued, read by read in the order they are written in;
    // {q_from, q_to} read-forward
    hvec<PartialRecord> partials;
    // statistics in the reference's form (flx_stats.cpp), when the context has a statistics object attached, and their clock
    std::unique_ptr<Stats> st_local;
    std::chrono::steady_clock::time_point t_slice;
    double search_ms = 0;

    u32 n_sampled(ReadState const& r) const { return (u32)((r.tree_ref().leaves.size() + step - 1) / step); }      // seeds per orientation
    // traces windows of the slice's reads (root windows, partial records): CIGAR words into cig, MD strings into md when wanted
    // tails: the paths' tails as well (align_roots alone asks for them)
    int trace_windows(Lane* lane, const flx_reads* RD, hvec<AlignRequest> const& reqs, hvec<TraceResult>& tres, const TailParams* tails = nullptr) {
        TraceWants wants;
        wants.md_pool = want_md ? &md : nullptr;
        wants.tails = tails;
        wants.left_align = want_left_align;
        wants.realign = realign;             // (null unless the option is active)
        wants.cs_form = cs_form;
        wants.cs_pool = &cs;
        wants.d_query = RD->d_pool.as<u8>();
        return run_trace_jobs_union(lane, lane->ctx->didx.text, RD->d_peq.as<u64>(), reqs, tres, cig, wants);
    }
};

// the options of a run by value (flx_run_options, validated): an option that is off is a zeroed member
struct RunOptions { flx_output_options output; flx_tag_options tags; flx_partial_options partial; flx_extend_options extend; flx_split_options split; flx_gap_options gaps; flx_realign_options realign; flx_cs_options cs; };

// produces the slice's records (read_index relative to the whole batch)
int align_slice(Lane* lane, const flx_params* P, RunOptions const& R, const flx_reads* RD, u64 first_read, u64 end_read, flx_run* run);

}  // namespace flx
