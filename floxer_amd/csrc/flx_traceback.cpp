// The traceback stage behind K4: K5, the five passes behind it (launch and judge of each, once), their result tables on the way back,
// and the runners of a pass alone.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "flx_traceback.hpp"

namespace flx {

extern const char MD_BUILD[] = "md_build", CIGAR_TAILS[] = "cigar_tails", CIGAR_LEFT_ALIGN[] = "cigar_left_align", CIGAR_REALIGN[] = "cigar_realign",
                  CS_BUILD[] = "cs_build";

// cigar_realign's launches: at most REALIGN_LAUNCH_JOBS jobs each, their traces together inside the arena. A job that asks for more
// trace than the arena holds: the door of the kernel alone sizes trace_cap from the words themselves, the band the kernel will really
// use, so such a path cannot be realigned on this lane; it keeps its words (trace_cap 0) and takes no room in a launch. The chain
// sizes it from K4's NM, an upper bound of that band: the job gets the whole arena and the kernel, which sees the path, decides.
u64 RealignPass::cut(u64 arena_words, OversizeTrace oversize) {
    constexpr size_t REALIGN_LAUNCH_JOBS = 4096;
    cuts.assign(1, 0);
    u64 used = 0, largest = 0;
    for (size_t k = 0; k < jobs.size(); ++k) {
        if (jobs[k].trace_cap > arena_words) jobs[k].trace_cap = oversize == OversizeTrace::KEEP_PATH ? 0u : (u32)std::min<u64>(arena_words, 0xFFFFFFFFull);
        if (k - cuts.back() == REALIGN_LAUNCH_JOBS || used + jobs[k].trace_cap > arena_words) { cuts.push_back(k); used = 0; }
        jobs[k].trace_off = used;
        used += jobs[k].trace_cap;
        largest = std::max(largest, used);
    }
    cuts.push_back(jobs.size());
    return largest;
}

// ================================================================================================ the chain
u32 Traceback::add(AlignRequest const& r, u64 trace_off, AlignShape sh, u32 end_col, u32 nm) {
    // runs <= 2*NM + 1; a realigned path has at most realign_cap words (left-aligned too: gaps only merge there) and its NM stays
    // below realign_nm_bound, which sizes its MD and cs slabs
    const RealignScores* const rs = wants.realign;
    u32 const j = (u32)jobs.size(), cap = rs ? (u32)std::max<u64>(2 * nm + 2, realign_cap(nm, 0, *rs)) : 2 * nm + 2;
    u32 const nm_slab = rs ? (u32)realign_nm_bound(nm, *rs) : nm;
    jobs.push_back(DevTraceJob{r.ref_off, r.q_off, trace_off, cigar_words, r.n, r.m, sh.lanes_per_job, sh.words_per_lane, end_col, cap, j, r.k});
    if (wants.md_pool) md.add(r, cigar_words, nm_slab, j);
    if (wants.tails) tails.add(*wants.tails, cigar_words, j);
    if (wants.left_align) la.add(r, cigar_words, cap, j);      // (<= 2 NM + 1 words after it too)
    if (rs) ra.add(r, cigar_words, cap, j, nm, *rs);
    if (wants.cs_form) cs.add(r, cigar_words, nm_slab, wants.cs_form, j);
    cigar_words += cap;
    path_steps += (u64)r.m + nm;
    return j;
}

int Traceback::run(Lane* lane, const u8* d_text, const u64* d_peq, hvec<u32>& cigar_pool) {
    cigar_base = cigar_pool.size();
    if (jobs.empty()) return FLX_OK;
    int rc;
    const RealignScores* const realign = wants.realign;
    bool const want_md = wants.md_pool != nullptr, want_tails = wants.tails != nullptr, want_la = wants.left_align, want_cs = wants.cs_form != 0;
    // the job tables (all but cigar_realign's: its trace_off is only known below) up in one copy, 256-byte-aligned sections packed in the
    // lane's staging block
    struct Section { const void* src; size_t bytes, off; };
    Section sec[5] = {{jobs.data(), jobs.size() * sizeof(DevTraceJob), 0}, {md.jobs.data(), md.jobs.size() * sizeof(DevMdJob), 0},
                      {tails.jobs.data(), tails.jobs.size() * sizeof(DevTailJob), 0}, {la.jobs.data(), la.jobs.size() * sizeof(DevLeftAlignJob), 0},
                      {cs.jobs.data(), cs.jobs.size() * sizeof(DevCsJob), 0}};
    size_t b_tables = 0;
    for (Section& s : sec)
        if (s.bytes) { s.off = b_tables; b_tables += (s.bytes + 255) & ~(size_t)255; }
    if ((rc = lane->tjobs.ensure(b_tables + 16))) return rc;
    char* const h = (char*)lane->stage_begin(b_tables);
    if (!h) return FLX_ERR_NO_DEVICE;
    for (Section const& s : sec)
        if (s.bytes) memcpy(h + s.off, s.src, s.bytes);
    FLX_HIP(hipMemcpyAsync(lane->tjobs.ptr, h, b_tables, hipMemcpyHostToDevice, lane->stream));
    auto const d_section = [&](int i) { return (const void*)((char*)lane->tjobs.ptr + sec[i].off); };
    if ((rc = lane->tjob_out.ensure(jobs.size() * sizeof(DevTraceOut)))) return rc;
    if ((rc = lane->cigar.ensure(cigar_words * 4 + 16))) return rc;
    if (want_md && (rc = lane->md.ensure(md.slab_bytes + 16))) return rc;
    if (want_cs && (rc = lane->cs.ensure(cs.slab_bytes + 16))) return rc;
    if (want_la && (rc = lane->cigar_la.ensure(cigar_words * 4 + 16))) return rc;
    if (realign) {
        // (the arena as it stands: K4's planes lie there until K5 has read them, it is not grown here)
        ra.cut(lane->trace.cap / 4, OversizeTrace::CLAMP_TO_ARENA);
        if ((rc = h2d(lane, lane->ra_jobs, ra.jobs.data(), ra.jobs.size() * sizeof(DevRealignJob)))) return rc;
        if ((rc = lane->cigar_ra.ensure(cigar_words * 4 + 16))) return rc;
    }
    // the words everything behind K5 reads: K5's, the realigned or the normalised ones
    u32* const d_ra_words = realign ? lane->cigar_ra.as<u32>() : lane->cigar.as<u32>();
    u32* const d_words = want_la ? lane->cigar_la.as<u32>() : d_ra_words;
    // The result tables ask the lane's mapped block for room in this order. Every pass reads K5's DevTraceOuts on the device; md_build's,
    // cigar_tails' and cigar_left_align's tables are handed over with them; nothing reads cigar_realign's statistics or cs_build's lengths.
    size_t const n = jobs.size();
    table.want(lane->tjob_out, outs, n, want_md || want_tails || want_la || realign || want_cs);
    if (want_md) md.table.want(lane->md_out, md.outs, n, true);
    if (want_tails) tails.table.want(lane->tail_out, tails.outs, n, true);
    if (want_la) la.table.want(lane->la_stat, la.stats, n, true);
    if (realign) ra.table.want(lane->ra_stat, ra.stats, n, false);
    if (want_cs) cs.table.want(lane->cs_out, cs.outs, n, false);
    ResultTable* const tables[6] = {&table, &md.table, &tails.table, &la.table, &ra.table, &cs.table};
    size_t asked = 0;
    bool published = true;
    for (ResultTable* t : tables) {
        if (!t->buf) continue;
        t->ask(lane);
        asked += (t->bytes + 63) & ~(size_t)63;
        if (t->read_on_device && !t->slot) published = false;
    }
    for (ResultTable* t : tables)
        if (t->buf && (rc = t->settle(published))) return rc;
    if (getenv("FLX_ALIGN_DEBUG")) {
        // 1: the table has its range of the block, 0: it has none and is copied, -: not wanted (outs, md, tails and la come back through
        // the block only when each of them that is wanted shows 1)
        char b[6];
        for (int i = 0; i < 6; ++i) b[i] = !tables[i]->buf ? '-' : tables[i]->slot ? '1' : '0';
        fprintf(stderr, "[traceback] jobs %zu block: outs md tails la ra cs = %c %c %c %c %c %c asked %zu\n", n, b[0], b[1], b[2], b[3], b[4], b[5], asked);
    }
    DevTraceOut* const d_outs = table.dev<DevTraceOut>();
    rc = timed_launch(lane, "ed_traceback", path_steps * 18, path_steps, [&] {
        return DeviceApi::traceback(lane->stream, d_text, d_peq, lane->trace.as<u64>(), (const DevTraceJob*)d_section(0), (u32)n, lane->cigar.as<u32>(), d_outs);
    });
    if (rc) return rc;
    if (realign && (rc = ra.launch(lane, d_text, wants.d_query, lane->cigar.as<u32>(), d_outs, lane->ra_jobs.as<DevRealignJob>(), *realign, d_ra_words,
                                   ra.table.dev<DevRealignStat>()))) return rc;
    if (want_la && (rc = la.launch(lane, d_text, wants.d_query, d_ra_words, d_outs, (const DevLeftAlignJob*)d_section(3), d_words, la.table.dev<DevLeftAlignStat>()))) return rc;
    if (want_md && (rc = md.launch(lane, d_text, d_words, d_outs, (const DevMdJob*)d_section(1), lane->md.as<u8>(), md.table.dev<DevMdOut>()))) return rc;
    if (want_cs && (rc = cs.launch(lane, d_text, wants.d_query, d_words, d_outs, (const DevCsJob*)d_section(4), wants.cs_form, lane->cs.as<u8>(), cs.table.dev<DevCsOut>()))) return rc;
    if (want_tails && (rc = tails.launch(lane, d_words, d_outs, (const DevTailJob*)d_section(2), tails.table.dev<DevTailOut>()))) return rc;
    PublishList pub;
    for (ResultTable* t : tables) t->publish(pub);
    if (pub.n) {
        int const e = DeviceApi::publish_stage(lane->stream, pub);
        if (e) { set_error(std::string("publish_stage: ") + hipGetErrorString((hipError_t)e)); return FLX_ERR_NO_DEVICE; }
    }
    if (prof) prof->mark("tb-prep");
    cigar_pool.resize(cigar_base + cigar_words);
    if (prof) prof->mark("pool-resize");
    // what is not in the block is copied, the tables next to their slabs
    if ((rc = table.fetch(lane))) return rc;
    if ((rc = d2h(lane, cigar_pool.data() + cigar_base, d_words, cigar_words * 4))) return rc;
    if (want_md) {
        md_base = wants.md_pool->size();
        wants.md_pool->resize(md_base + md.slab_bytes);
        if ((rc = md.table.fetch(lane))) return rc;
        if ((rc = d2h(lane, wants.md_pool->data() + md_base, lane->md.ptr, md.slab_bytes))) return rc;
    }
    if (want_cs) {
        cs_base = wants.cs_pool->size();
        wants.cs_pool->resize(cs_base + cs.slab_bytes);
        if ((rc = cs.table.fetch(lane))) return rc;
        if ((rc = d2h(lane, wants.cs_pool->data() + cs_base, lane->cs.ptr, cs.slab_bytes))) return rc;
    }
    if ((rc = tails.table.fetch(lane)) || (rc = la.table.fetch(lane)) || (rc = ra.table.fetch(lane))) return rc;
    if ((rc = lane->sync())) return rc;
    for (ResultTable* t : tables) t->land();
    if (prof) prof->mark("K5+d2h");
    const char* const overflow = want_la || realign ? "ed_traceback / cigar_realign / cigar_left_align: CIGAR slab overflow" : "ed_traceback: CIGAR slab overflow";
    if (any_overflow(outs, overflow)) return FLX_ERR_INTERNAL;
    if (realign && (rc = ra.judge(lane, outs, overflow))) return rc;
    if (want_la && (rc = la.judge(lane, outs, overflow))) return rc;
    if (want_md && (rc = md.judge(lane, outs))) return rc;
    if (want_cs && (rc = cs.judge(lane, outs))) return rc;
    if (want_tails && (rc = tails.judge(lane, outs))) return rc;
    return FLX_OK;
}

TraceResult Traceback::result(u32 j, u32 nm) const {
    TraceResult res;
    res.exists = true;
    res.nm = res.ed = nm;
    res.begin = outs[j].begin;
    res.cigar_off = cigar_base + jobs[j].cigar_off + outs[j].cigar_start;
    res.cigar_len = outs[j].cigar_len;
    if (wants.md_pool) { res.md_off = md_base + md.jobs[j].md_off; res.md_len = md.outs[j].len; }
    if (wants.cs_form) { res.cs_off = cs_base + cs.jobs[j].cs_off; res.cs_len = cs.outs[j].len; }
    if (wants.tails) res.tail = tails.outs[j];
    if (wants.realign) { res.nm = ra.stats[j].num_errors; res.score = ra.stats[j].score; }      // (a kept path: NM is K4's)
    return res;
}

// ================================================================================================ a pass alone
namespace {
// what every runner of a pass alone sends up: the words, the DevTraceOuts and its job table
template <class Job>
int upload_alone(Lane* lane, const u32* words, u64 n_words, hvec<DevTraceOut> const& touts, DeviceBuffer& job_buf, hvec<Job> const& jobs) {
    int rc;
    if ((rc = h2d(lane, lane->cigar, words, n_words * 4))) return rc;
    if ((rc = h2d(lane, lane->tjob_out, touts.data(), touts.size() * sizeof(DevTraceOut)))) return rc;
    return h2d(lane, job_buf, jobs.data(), jobs.size() * sizeof(Job));
}
}  // namespace

int run_tail_jobs(Lane* lane, const u32* words, u64 n_words, hvec<DevTraceOut> const& touts, TailPass& pass) {
    pass.outs.assign(pass.jobs.size(), DevTailOut{});
    if (pass.jobs.empty()) return FLX_OK;
    int rc;
    if ((rc = upload_alone(lane, words, n_words, touts, lane->tail_jobs, pass.jobs))) return rc;
    if ((rc = lane->tail_out.ensure(pass.jobs.size() * sizeof(DevTailOut)))) return rc;
    if ((rc = pass.launch(lane, lane->cigar.as<u32>(), lane->tjob_out.as<DevTraceOut>(), lane->tail_jobs.as<DevTailJob>(), lane->tail_out.as<DevTailOut>()))) return rc;
    if ((rc = d2h(lane, pass.outs.data(), lane->tail_out.ptr, pass.outs.size() * sizeof(DevTailOut)))) return rc;
    if ((rc = lane->sync())) return rc;
    return pass.judge(lane, touts);
}

int run_left_align_jobs(Lane* lane, const u8* d_text, const u8* d_query, const u32* words, u64 n_words, hvec<DevTraceOut>& touts, LeftAlignPass& pass,
                        u64 words_out, hvec<u32>& out_words) {
    out_words.assign(words_out, 0u);
    pass.stats.resize(pass.jobs.size());
    if (pass.jobs.empty()) return FLX_OK;
    int rc;
    if ((rc = upload_alone(lane, words, n_words, touts, lane->la_jobs, pass.jobs))) return rc;
    if ((rc = lane->cigar_la.ensure(words_out * 4 + 16))) return rc;
    if ((rc = lane->la_stat.ensure(pass.jobs.size() * sizeof(DevLeftAlignStat)))) return rc;
    if ((rc = pass.launch(lane, d_text, d_query, lane->cigar.as<u32>(), lane->tjob_out.as<DevTraceOut>(), lane->la_jobs.as<DevLeftAlignJob>(), lane->cigar_la.as<u32>(),
                          lane->la_stat.as<DevLeftAlignStat>()))) return rc;
    if ((rc = d2h(lane, touts.data(), lane->tjob_out.ptr, touts.size() * sizeof(DevTraceOut)))) return rc;
    if ((rc = d2h(lane, out_words.data(), lane->cigar_la.ptr, words_out * 4))) return rc;
    if ((rc = d2h(lane, pass.stats.data(), lane->la_stat.ptr, pass.stats.size() * sizeof(DevLeftAlignStat)))) return rc;
    if ((rc = lane->sync())) return rc;
    return pass.judge(lane, touts, "cigar_left_align: CIGAR slab overflow, or a path that leaves its window or its query");
}

int run_realign_jobs(Lane* lane, const u8* d_text, const u8* d_query, const u32* words, u64 n_words, hvec<DevTraceOut>& touts, RealignPass& pass,
                     RealignScores const& scores, u64 words_out, hvec<u32>& out_words) {
    out_words.assign(words_out, 0u);
    pass.stats.assign(pass.jobs.size(), DevRealignStat{0, 0u, 0, 0, 0u, 0u, 0ull});
    if (pass.jobs.empty()) return FLX_OK;
    int rc;
    u64 const largest = pass.cut(std::max<u64>(lane->trace_budget_bytes / 4, 1), OversizeTrace::KEEP_PATH);
    if ((rc = upload_alone(lane, words, n_words, touts, lane->ra_jobs, pass.jobs))) return rc;
    if ((rc = lane->cigar_ra.ensure(words_out * 4 + 16))) return rc;
    if ((rc = lane->ra_stat.ensure(pass.jobs.size() * sizeof(DevRealignStat)))) return rc;
    // (the arena is taken as the traceback stage takes it on first use: no reallocation when that stage runs later)
    if ((rc = lane->trace.ensure(std::max<size_t>(largest * 4 + 64, lane->trace.ptr ? 0 : lane->trace_budget_bytes / 3 * 2)))) return rc;
    if ((rc = pass.launch(lane, d_text, d_query, lane->cigar.as<u32>(), lane->tjob_out.as<DevTraceOut>(), lane->ra_jobs.as<DevRealignJob>(), scores,
                          lane->cigar_ra.as<u32>(), lane->ra_stat.as<DevRealignStat>()))) return rc;
    if ((rc = d2h(lane, touts.data(), lane->tjob_out.ptr, touts.size() * sizeof(DevTraceOut)))) return rc;
    if ((rc = d2h(lane, out_words.data(), lane->cigar_ra.ptr, words_out * 4))) return rc;
    if ((rc = d2h(lane, pass.stats.data(), lane->ra_stat.ptr, pass.stats.size() * sizeof(DevRealignStat)))) return rc;
    if ((rc = lane->sync())) return rc;
    return pass.judge(lane, touts, "cigar_realign: CIGAR slab overflow, or a path that leaves its window or its query");
}

int run_cs_jobs(Lane* lane, const u8* d_text, const u8* d_query, const u32* words, u64 n_words, hvec<DevTraceOut> const& touts, CsPass& pass, u32 form,
                hvec<u8>& slabs) {
    slabs.assign(pass.slab_bytes, (u8)0);
    pass.outs.assign(pass.jobs.size(), DevCsOut{0, 0});
    if (pass.jobs.empty()) return FLX_OK;
    int rc;
    if ((rc = upload_alone(lane, words, n_words, touts, lane->cs_jobs, pass.jobs))) return rc;
    if ((rc = lane->cs.ensure(pass.slab_bytes + 16))) return rc;
    if ((rc = lane->cs_out.ensure(pass.jobs.size() * sizeof(DevCsOut)))) return rc;
    if ((rc = pass.launch(lane, d_text, d_query, lane->cigar.as<u32>(), lane->tjob_out.as<DevTraceOut>(), lane->cs_jobs.as<DevCsJob>(), form, lane->cs.as<u8>(),
                          lane->cs_out.as<DevCsOut>()))) return rc;
    if ((rc = d2h(lane, pass.outs.data(), lane->cs_out.ptr, pass.outs.size() * sizeof(DevCsOut)))) return rc;
    if (pass.slab_bytes && (rc = d2h(lane, slabs.data(), lane->cs.ptr, pass.slab_bytes))) return rc;
    if ((rc = lane->sync())) return rc;
    return pass.judge(lane, touts);
}

}  // namespace flx
