// Device context: HBM-resident index, grow-only workspaces, stream, per-kernel accounting.
#pragma once

#include <hip/hip_runtime.h>

#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "flx_internal.hpp"

namespace flx {

#define FLX_HIP(expr)                                                                                   \
    do {                                                                                                \
        hipError_t const e__ = (expr);                                                                  \
        if (e__ != hipSuccess) {                                                                        \
            set_error(std::string(#expr) + ": " + hipGetErrorString(e__));                              \
            return FLX_ERR_NO_DEVICE;                                                                   \
        }                                                                                               \
    } while (0)

// the one check of a launch: rc is the hipError_t that a launch function returned
#define FLX_LAUNCH(name, rc)                                                                            \
    do {                                                                                                \
        int const e__ = (rc);                                                                           \
        if (e__ != 0) {                                                                                 \
            set_error(std::string(name) + ": launch failed: " + hipGetErrorString((hipError_t)e__));    \
            return FLX_ERR_NO_DEVICE;                                                                   \
        }                                                                                               \
    } while (0)

struct DeviceBuffer {
    void* ptr = nullptr;
    size_t cap = 0;
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer const&) = delete;
    DeviceBuffer& operator=(DeviceBuffer const&) = delete;
    ~DeviceBuffer() { release(); }   // (error paths drop half-made owners: nothing stays allocated)
    int ensure(size_t bytes, bool exact = false);      // grow-only; contents are NOT preserved; exact: no growth slack
    void release();
    void take(DeviceBuffer& other) { release(); ptr = other.ptr; cap = other.cap; other.ptr = nullptr; other.cap = 0; }      // this one owns other's memory now
    template <class T> T* as() const { return reinterpret_cast<T*>(ptr); }
};

// Page-locked host memory that the device reads and writes in place (mapped), grow-only.
struct PinnedBuffer {
    void* ptr = nullptr;
    size_t cap = 0;
    PinnedBuffer() = default;
    PinnedBuffer(PinnedBuffer const&) = delete;
    PinnedBuffer& operator=(PinnedBuffer const&) = delete;
    ~PinnedBuffer() { release(); }
    int ensure(size_t bytes);        // contents are NOT preserved; the caller makes sure the device is done with the old block
    void release();
};

struct PendingTiming { std::string name; hipEvent_t start, stop; u64 bytes, units; };

}  // namespace flx


struct flx_ctx;
struct flx_stats;

namespace flx {
// One execution lane: a HIP stream with its own grow-only workspaces. A context runs the slices of a read batch on several
// lanes concurrently (one host thread each) so that the host-side phases of one slice overlap the kernels of the others.
struct Lane {
    flx_ctx* ctx = nullptr;
    int id = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    DeviceBuffer seq, seq_rev, peq, peq_rev, scheme, seeds, stack, hits, counters, rows, rows_out, qpack, items;
    DeviceBuffer jobs, job_out, trace, tjobs, tjob_out, cigar, md, md_out, user_text, user_text_rev, lastrow, row_windows, row_out,
        seed_cnt, hit_off, grouped, sel_stat, sel_n, sel_off, sel_out, sel_tmp, sel_rows, sel_row_off, sel_sparse, sel_lists, vr, seed_gen, mailboxes, ext_jobs, ext_out, tail_jobs, tail_out, cigar_la, la_jobs, la_stat, cigar_ra, ra_jobs, ra_stat, cs, cs_jobs, cs_out;
    size_t trace_budget_bytes = 0;
    std::vector<PendingTiming> pending;
    std::vector<hipEvent_t> event_pool;
    hipEvent_t sync_event = nullptr;
    u32* vr_host_scalars = nullptr;  // page-locked, mapped: a round's scalars, written by the device (flx_rounds.hip)
    // A stage's small tables go up packed: built in place in `staging`, one copy per stage (or read in place by a kernel that reads a
    // table once). stage_begin returns the block for the stage that starts now: every stage ends with a wait for the stream before its
    // host code goes on, so the previous stage's copies have left the block. Null: out of page-locked memory (an error is set).
    PinnedBuffer staging;
    void* stage_begin(size_t bytes);
    // Small per-chunk results (counters, job counts, result tables of a few KB) come back without a copy: the producing kernel stores
    // them into this mapped block and the host reads them after the stream wait it makes anyway. Every use takes its own range
    // (result_slot), written in full by its producer: nothing is ever cleared. A ResultScope gives the ranges taken inside it back.
    PinnedBuffer results;
    size_t results_used = 0;
    static constexpr size_t RESULT_BLOCK_BYTES = 1u << 20;
    // the bytes result_slot hands out at most: RESULT_BLOCK_BYTES, or less under FLX_RESULT_BLOCK_BYTES (a test hook, read when the block
    // is first made; 0: no block at all, every table takes its copy path)
    size_t results_limit = RESULT_BLOCK_BYTES;
    bool results_limit_read = false;
    void* result_slot(size_t bytes); // null: no room (the caller copies instead)
    bool has_run = false;            // a chunk has run here (its workspaces have their working sizes)
    double hits_per_seed = 0, items_per_seed = 0, sel_rows_per_seed = 0;      // of the last search here: the next one's buffers are sized for that and a margin
    int wait_idle();                 // the stream has drained (the thread sleeps on a blocking event unless FLX_SPIN_SYNC is set)
    int sync();                      // wait_idle + fold pending timings into the context's statistics
    std::vector<DeviceBuffer*> workspaces();
    int size_like(Lane& other);      // grow this lane's workspaces to the other lane's capacities
    hipEvent_t get_event();
    void release_all();
};
}  // namespace flx

struct flx_ctx {
    ~flx_ctx();                      // releases streams, workspaces and the index image it owns (also on a half-made context)
    int device = 0;
    const flx::HostIndex* hidx = nullptr;
    flx::DevIndex didx{};
    flx::DeviceBuffer occ0, occ1, sa, text, text_rev, kmer, seq_start;
    flx::DeviceBuffer isa, filter, filter_m;   // derived from text and suffix array when the context is made (flx_search.hip)
    bool text_rev_ready = false;
    std::mutex mu;                   // guards text_rev upload and the statistics
    std::vector<std::unique_ptr<flx::Lane>> lanes;
    hipStream_t upload_stream = nullptr;   // flx_reads_upload copies here, so that it can run while the lanes are busy
    // Device buffers of read batches that have been freed (flx_reads_free), by role (pool, 2-bit form, Peq planes, reversed pool, its Peq
    // planes): the next batch takes them instead of allocating. hipFree waits for the whole device, so a caller that hands batches over in
    // host memory (flx_align_reads: three buffers made and freed per batch) used to stall every lane three times per batch.
    std::mutex spare_mu;
    std::vector<std::unique_ptr<flx::DeviceBuffer>> spare_read_buffers[5];
    int live_reads = 0;              // read batches made on this context and not yet freed (guarded by spare_mu): flx_ctx_destroy refuses while > 0
    int live_errprofs = 0;           // error-profile objects that read this context's text (flx_errprof_create) and are not yet freed (guarded by spare_mu): the same
    int live_consensus = 0;          // consensus objects that read this context's text (flx_consensus_create) and are not yet freed (guarded by spare_mu): the same
    int live_variants = 0;           // variants objects that read this context's text (flx_variants_create) and are not yet freed (guarded by spare_mu): the same
    int live_phases = 0;             // phase objects made on this context (flx_phase_create) and not yet freed (guarded by spare_mu): the same
    int live_svcallers = 0;          // svcaller objects made on this context (flx_svcaller_create) and not yet freed (guarded by spare_mu): the same
    bool external_stream = false;    // a caller-owned stream is installed on lane 0: run on that lane only
    // accounting
    bool timing = false;
    std::map<std::string, flx_kernel_stat> stats;
    std::vector<std::string> stat_order;
    flx_path_counters path{};        // guarded by mu
    flx_realign_counters realign{};  // guarded by mu
    flx_search_counters search{};    // guarded by mu; reset with `path`
    flx_stats* read_stats = nullptr; // flx_ctx_set_stats: every batch adds its reads (flx_stats.cpp); not owned

    // lanes are handed out one holder at a time, so calls on one context may overlap (each waits for a free lane)
    std::mutex lane_mu;
    std::condition_variable lane_cv;
    std::vector<int> free_lanes;     // indices into `lanes`
    flx::Lane* acquire_lane(int wanted = -1);   // blocks; wanted >= 0: that lane. Prefers the lane released last.
    void release_lane(flx::Lane* lane);
    void warm_one_cold_lane(flx::Lane* like);   // gives one lane that never ran the workspace sizes of `like` (still held)

    // K1 launches in flight at a time (see search_seeds_device): a counting semaphore
    int k1_tokens = 0;               // guarded by lane_mu; 0 = unlimited
    int k1_running = 0;
    void k1_acquire();
    void k1_release();

    flx::Lane* lane0() { return lanes[0].get(); }
    int sync_all();
    void account(const char* name, flx::u64 bytes, flx::u64 units, hipEvent_t start, hipEvent_t stop);   // caller holds mu
    // bytes and units of launches already accounted that were only known once their results were back (takes mu; nothing when timing is off
    // or the kernel has no entry)
    void account_more(const char* name, flx::u64 bytes, flx::u64 units);
};

namespace flx {

struct LaneLease {
    flx_ctx* ctx;
    Lane* lane;
    explicit LaneLease(flx_ctx* c, int wanted = -1) : ctx(c), lane(c->acquire_lane(wanted)) {}
    ~LaneLease() { ctx->release_lane(lane); }
    LaneLease(LaneLease const&) = delete;
    LaneLease& operator=(LaneLease const&) = delete;
};

struct ResultScope {
    Lane* lane;
    size_t mark;
    explicit ResultScope(Lane* l) : lane(l), mark(l->results_used) {}
    ~ResultScope() { lane->results_used = mark; }
    ResultScope(ResultScope const&) = delete;
    ResultScope& operator=(ResultScope const&) = delete;
};

// brackets a launch with events when timing is enabled
template <class F>
int timed_launch(Lane* lane, const char* name, u64 bytes, u64 units, F&& launch) {
    if (!lane->ctx->timing) {
        FLX_LAUNCH(name, launch());
        return FLX_OK;
    }
    hipEvent_t const a = lane->get_event(), b = lane->get_event();
    FLX_HIP(hipEventRecord(a, lane->stream));
    int const rc = launch();
    FLX_HIP(hipEventRecord(b, lane->stream));
    FLX_LAUNCH(name, rc);
    lane->pending.push_back(PendingTiming{name, a, b, bytes, units});
    return FLX_OK;
}

}  // namespace flx
