// The traceback stage behind K4 (flx_traceback.cpp): K5 over the paths of one arena chunk and the five passes queued behind it on the
// lane's stream, each written once. A pass owns its job and result vectors, `add` for one trace job, `launch` (the timed launch under
// the kernel's name with its launch-time bytes and units, on device pointers it is given) and `judge` (the overflow test, and the
// bytes and units that depend on what K5 and the pass found: they are known once the results are back). The chain (Traceback::run)
// and the runners of a kernel alone (run_*_jobs, behind flx_*_batch of flx_align_capi.cpp) call the same launch and judge: a kernel's
// accounting does not depend on the door it was launched through.
#pragma once

#include <cstring>

#include "flx_pipeline.hpp"
#include "flx_realign.hpp"

namespace flx {

// the names the kernels are accounted under
extern const char MD_BUILD[], CIGAR_TAILS[], CIGAR_LEFT_ALIGN[], CIGAR_REALIGN[], CS_BUILD[];

// One small result table of a stage (a row per job) on its way back. It has a range of the lane's mapped result block when the block
// had room (slot) and a lane buffer on the device. A table that a later pass reads on the device is written to the lane buffer and
// handed over by the stage's one publish_stage launch, and only when every such table has its range (they are published together or
// not at all); a table nothing on the device reads is stored into its range by its own kernel, whatever became of the others. Not in
// the block: copied behind the stage.
struct ResultTable {
    DeviceBuffer* buf = nullptr;       // null: not wanted
    void* host = nullptr;
    size_t bytes = 0;
    bool read_on_device = false;
    void* slot = nullptr;
    bool in_block = false;
    template <class Row> void want(DeviceBuffer& lane_buf, hvec<Row>& rows, size_t n, bool read_on_device_) {
        rows.resize(n);
        buf = &lane_buf; host = rows.data(); bytes = n * sizeof(Row); read_on_device = read_on_device_;
    }
    void ask(Lane* lane) { slot = lane->result_slot(bytes); }
    int settle(bool published) {       // in_block, and the lane buffer when the kernel writes there
        in_block = slot && (published || !read_on_device);
        return in_block && !read_on_device ? FLX_OK : buf->ensure(bytes);
    }
    // a table on its own that nothing on the device reads: all of the above
    template <class Row> int place(Lane* lane, DeviceBuffer& lane_buf, hvec<Row>& rows, size_t n) { want(lane_buf, rows, n, false); ask(lane); return settle(false); }
    template <class Row> Row* dev() const { return in_block && !read_on_device ? (Row*)slot : buf->as<Row>(); }      // where its kernel stores it
    void publish(PublishList& pub) const { if (buf && in_block && read_on_device) pub.add(buf->ptr, slot, bytes / 4); }
    int fetch(Lane* lane) const { return buf && !in_block ? d2h(lane, host, buf->ptr, bytes) : FLX_OK; }
    void land() const { if (buf && in_block) memcpy(host, slot, bytes); }    // after the stream wait
};

inline bool any_overflow(hvec<DevTraceOut> const& touts, const char* message) {
    for (auto const& t : touts)
        if (t.cigar_len == 0xFFFFFFFFu) { set_error(message); return true; }
    return false;
}

// ---- md_build (flx_md.hip): a slab of md_slab_bytes per job
struct MdPass {
    hvec<DevMdJob> jobs;
    hvec<DevMdOut> outs;
    ResultTable table;
    u64 slab_bytes = 0;
    void add(AlignRequest const& r, u64 cigar_off, u32 nm, u32 j) {
        u64 const slab = md_slab_bytes(nm);
        jobs.push_back(DevMdJob{r.ref_off, cigar_off, slab_bytes, r.n, (u32)slab, j, 0});
        slab_bytes += slab;
    }
    int launch(Lane* lane, const u8* d_text, const u32* d_words, const DevTraceOut* d_touts, const DevMdJob* d_jobs, u8* d_md, DevMdOut* d_outs) const {
        return timed_launch(lane, MD_BUILD, 0, jobs.size(), [&] { return DeviceApi::md_build(lane->stream, d_text, d_words, d_touts, d_jobs, (u32)jobs.size(), d_md, d_outs); });
    }
    int judge(Lane* lane, hvec<DevTraceOut> const& touts) const {
        // CIGAR words read + reference letters read (one per X / D column: at most NM) + MD bytes written
        u64 bytes = 0;
        for (size_t j = 0; j < jobs.size(); ++j) {
            if (outs[j].len == 0xFFFFFFFFu) { set_error("md_build: MD slab overflow, or a path that leaves its window"); return FLX_ERR_INTERNAL; }
            bytes += 4ull * touts[j].cigar_len + outs[j].len + (jobs[j].md_cap - 6u) / 8u;
        }
        lane->ctx->account_more(MD_BUILD, bytes, 0);
        return FLX_OK;
    }
};

// ---- cigar_tails (flx_tails.hip)
struct TailPass {
    hvec<DevTailJob> jobs;
    hvec<DevTailOut> outs;
    ResultTable table;
    void add(TailParams const& p, u64 cigar_off, u32 j) { jobs.push_back(DevTailJob{cigar_off, j, p.w, p.x_drop, p.min_rows}); }
    int launch(Lane* lane, const u32* d_words, const DevTraceOut* d_touts, const DevTailJob* d_jobs, DevTailOut* d_outs) const {
        return timed_launch(lane, CIGAR_TAILS, jobs.size() * (sizeof(DevTailJob) + sizeof(DevTraceOut) + sizeof(DevTailOut)), jobs.size(),
                            [&] { return DeviceApi::cigar_tails(lane->stream, d_words, d_touts, d_jobs, (u32)jobs.size(), d_outs); });
    }
    int judge(Lane* lane, hvec<DevTraceOut> const& touts) const {
        u64 bytes = 0;
        for (auto const& t : touts) bytes += 4ull * t.cigar_len;
        lane->ctx->account_more(CIGAR_TAILS, bytes, 0);
        return FLX_OK;
    }
};

// ---- cigar_left_align (flx_leftalign.hip): the normalised words go to a second slab buffer, the DevTraceOuts are rewritten
struct LeftAlignPass {
    hvec<DevLeftAlignJob> jobs;
    hvec<DevLeftAlignStat> stats;
    ResultTable table;
    void add(AlignRequest const& r, u64 cigar_off, u32 cap, u32 j) { jobs.push_back(DevLeftAlignJob{r.ref_off, r.q_off, cigar_off, cigar_off, r.n, r.m, cap, j}); }
    int launch(Lane* lane, const u8* d_text, const u8* d_query, const u32* d_words, DevTraceOut* d_touts, const DevLeftAlignJob* d_jobs, u32* d_words_out,
               DevLeftAlignStat* d_stats) const {
        return timed_launch(lane, CIGAR_LEFT_ALIGN, jobs.size() * (sizeof(DevLeftAlignJob) + 2 * sizeof(DevTraceOut) + sizeof(DevLeftAlignStat)), 0, [&] {
            return DeviceApi::cigar_left_align(lane->stream, d_text, d_query, d_words, d_touts, d_jobs, (u32)jobs.size(), d_words_out, d_stats);
        });
    }
    int judge(Lane* lane, hvec<DevTraceOut> const& touts, const char* overflow) const {      // touts: as they are behind the stage
        if (any_overflow(touts, overflow)) return FLX_ERR_INTERNAL;
        // CIGAR words read and written + letters compared (both sides of every comparison); units: the gap words that moved or merged
        u64 bytes = 0, moved = 0;
        for (size_t j = 0; j < jobs.size(); ++j) { bytes += 4ull * stats[j].words_in + 4ull * touts[j].cigar_len + 2ull * stats[j].letters; moved += stats[j].moved; }
        lane->ctx->account_more(CIGAR_LEFT_ALIGN, bytes, moved);
        return FLX_OK;
    }
};

// ---- cigar_realign (flx_realign.hip): launches whose traces lie in the lane's arena together (`cut`)
enum class OversizeTrace { KEEP_PATH, CLAMP_TO_ARENA };
struct RealignPass {
    hvec<DevRealignJob> jobs;
    hvec<DevRealignStat> stats;
    ResultTable table;
    hvec<size_t> cuts;                 // launch c runs jobs [cuts[c], cuts[c + 1])
    // (the diagonals of an edit path of NM errors span at most NM: the trace of a band of NM + 2 w + 1 cells always suffices)
    void add(AlignRequest const& r, u64 cigar_off, u32 cap, u32 j, u32 nm, RealignScores const& s) {
        jobs.push_back(DevRealignJob{r.ref_off, r.q_off, cigar_off, cigar_off, 0, r.n, r.m, cap, j,
                                     (u32)std::min<u64>(realign_trace_words(r.m, (u64)nm + 2u * (u64)s.w + 1u), 0xFFFFFFFFull), 0});
    }
    // sets the cuts and every job's trace_off (jobs[i].trace_cap: the trace words job i asks for); returns the words the largest launch needs
    u64 cut(u64 arena_words, OversizeTrace oversize);
    int launch(Lane* lane, const u8* d_text, const u8* d_query, const u32* d_words, DevTraceOut* d_touts, const DevRealignJob* d_jobs, RealignScores const& scores,
               u32* d_words_out, DevRealignStat* d_stats) const {
        for (size_t c = 0; c + 1 < cuts.size(); ++c) {
            size_t const first = cuts[c], count = cuts[c + 1] - first;
            int const rc = timed_launch(lane, CIGAR_REALIGN, count * (sizeof(DevRealignJob) + 2 * sizeof(DevTraceOut) + sizeof(DevRealignStat)), 0, [&] {
                return DeviceApi::cigar_realign(lane->stream, d_text, d_query, d_words, d_touts, d_jobs + first, (u32)count, scores, lane->trace.as<u32>(), d_words_out, d_stats);
            });
            if (rc) return rc;
        }
        return FLX_OK;
    }
    int judge(Lane* lane, hvec<DevTraceOut> const& touts, const char* overflow) const {      // touts: as they are behind the stage
        if (any_overflow(touts, overflow)) return FLX_ERR_INTERNAL;
        // the trace is written once and read along the path + the words written; units: DP cells
        u64 bytes = 0, cells = 0, changed = 0, kept = 0;
        for (size_t j = 0; j < jobs.size(); ++j) {
            bytes += stats[j].cells / 2 + 4ull * touts[j].cigar_len;
            cells += stats[j].cells; changed += stats[j].changed; kept += stats[j].kept;
        }
        lane->ctx->account_more(CIGAR_REALIGN, bytes, cells);
        std::lock_guard<std::mutex> g(lane->ctx->mu);
        lane->ctx->realign.paths_realigned += jobs.size() - kept;
        lane->ctx->realign.paths_changed += changed;
        lane->ctx->realign.paths_kept += kept;
        return FLX_OK;
    }
};

// ---- cs_build (flx_cs.hip): a slab of cs_slab_bytes per job
struct CsPass {
    hvec<DevCsJob> jobs;
    hvec<DevCsOut> outs;
    ResultTable table;
    u64 slab_bytes = 0;
    void add(AlignRequest const& r, u64 cigar_off, u32 nm, u32 form, u32 j) {
        u64 const slab = cs_slab_bytes(nm, r.m, form);
        jobs.push_back(DevCsJob{r.ref_off, r.q_off, cigar_off, slab_bytes, r.n, r.m, (u32)slab, j});
        slab_bytes += slab;
    }
    int launch(Lane* lane, const u8* d_text, const u8* d_query, const u32* d_words, const DevTraceOut* d_touts, const DevCsJob* d_jobs, u32 form, u8* d_cs,
               DevCsOut* d_outs) const {
        return timed_launch(lane, CS_BUILD, 0, 0, [&] { return DeviceApi::cs_build(lane->stream, d_text, d_query, d_words, d_touts, d_jobs, (u32)jobs.size(), form, d_cs, d_outs); });
    }
    int judge(Lane* lane, hvec<DevTraceOut> const& touts) const {
        // CIGAR words read + the string written + a letter read per letter written (at most the string again); units: output bytes
        u64 bytes = 0, written = 0;
        for (size_t j = 0; j < jobs.size(); ++j) {
            if (outs[j].len == 0xFFFFFFFFu) { set_error("cs_build: cs slab overflow, or a path that leaves its window or its query"); return FLX_ERR_INTERNAL; }
            bytes += 4ull * touts[j].cigar_len + 2ull * outs[j].len;
            written += outs[j].len;
        }
        lane->ctx->account_more(CS_BUILD, bytes, written);
        return FLX_OK;
    }
};

// K5 over the paths of one arena chunk and what the wants add: one job of every wanted pass per trace job. The job tables go up with
// the trace jobs in one copy; the passes are queued behind K5 without a host synchronisation in between, in this order:
// cigar_realign, cigar_left_align (each writes its words into a second slab buffer of K5's layout and rewrites K5's DevTraceOuts:
// everything behind it reads that buffer), md_build, cs_build, cigar_tails. A job's CIGAR slab holds 2 NM + 2 words (more under
// realign_cap), its MD slab md_slab_bytes(NM) and its cs slab cs_slab_bytes bytes, NM being what K4 returned for it; the slabs come
// back as they are (gaps included): no host repacking.
struct Traceback {
    TraceWants const& wants;
    PhaseTimer* const prof;
    hvec<DevTraceJob> jobs;
    hvec<DevTraceOut> outs;
    ResultTable table;
    MdPass md;
    TailPass tails;
    LeftAlignPass la;
    RealignPass ra;
    CsPass cs;
    u64 cigar_words = 0, path_steps = 0;
    size_t cigar_base = 0, md_base = 0, cs_base = 0;           // where this batch's slabs start in the host pools
    explicit Traceback(TraceWants const& wants_, PhaseTimer* prof_ = nullptr) : wants(wants_), prof(prof_) {}
    // the path that ends at end_col of the last row of r's DP, whose trace planes lie at trace_off; returns the trace job's index
    u32 add(AlignRequest const& r, u64 trace_off, AlignShape sh, u32 end_col, u32 nm);
    int run(Lane* lane, const u8* d_text, const u64* d_peq, hvec<u32>& cigar_pool);
    // trace job j as the result of a request whose K4 score was nm (begin: relative to the job's window)
    TraceResult result(u32 j, u32 nm) const;
};

// ---- a kernel alone, over CIGAR words and DevTraceOuts made on the host (the pipeline queues it behind K5): pass.jobs on entry
int run_tail_jobs(Lane* lane, const u32* words, u64 n_words, hvec<DevTraceOut> const& touts, TailPass& pass);
// out_words receives the second buffer (words_out words), touts the rewritten DevTraceOuts
int run_left_align_jobs(Lane* lane, const u8* d_text, const u8* d_query, const u32* words, u64 n_words, hvec<DevTraceOut>& touts, LeftAlignPass& pass,
                        u64 words_out, hvec<u32>& out_words);
// the same; pass.jobs[i].trace_cap = the trace words job i needs on entry
int run_realign_jobs(Lane* lane, const u8* d_text, const u8* d_query, const u32* words, u64 n_words, hvec<DevTraceOut>& touts, RealignPass& pass,
                     RealignScores const& scores, u64 words_out, hvec<u32>& out_words);
// slabs receives the jobs' slabs (pass.slab_bytes bytes)
int run_cs_jobs(Lane* lane, const u8* d_text, const u8* d_query, const u32* words, u64 n_words, hvec<DevTraceOut> const& touts, CsPass& pass, u32 form,
                hvec<u8>& slabs);

}  // namespace flx
