// Alignment job batches (K0/K3/K4/K5, alignment.cpp:83-181): de-duplication, launch shapes, one launch per shape class, and the score,
// trace, root-union and existence forms built on them; the C ABI of seam 2.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <numeric>
#include <string>

#include "flx_partial.hpp"
#include "flx_pipeline.hpp"
#include "flx_tails.hpp"
#include "flx_leftalign.hpp"
#include "flx_realign.hpp"
#include "flx_cs.hpp"

namespace flx {

u64 round_span_percent() {
    static u64 const v = getenv("FLX_ROUND_SPAN") ? std::max<u64>(100, strtoull(getenv("FLX_ROUND_SPAN"), nullptr, 10)) : 150;
    return v;
}
u64 align_few_waves() {
    const char* env = getenv("FLX_ALIGN_FEW_WAVES");
    return env ? strtoull(env, nullptr, 10) : 512;
}

namespace {

// word-steps the launch really performs for one job: only the band -k <= col-row <= n-m+k
u64 job_word_steps(u32 n, u32 m, u32 k, AlignShape sh) {
    u64 const nw = (m + 63) / 64;
    i64 const W = sh.words_per_lane, band_hi = (i64)n - (i64)m + (i64)k;
    u64 total = 0;
    for (i64 g = 0; g * W < (i64)nw; ++g) {
        i64 const r0 = 64 * W * g, r1 = std::min<i64>(m, r0 + 64 * W);
        i64 const lo = std::max<i64>(0, r0 - (i64)k), hi = std::min<i64>((i64)n - 1, r1 - 1 + band_hi);
        if (hi >= lo) total += (u64)(hi - lo + 1) * (u64)std::min<i64>(W, (i64)nw - g * W);
    }
    return total;
}

struct ShapeKey {
    u32 w, g;
    bool operator<(ShapeKey const& o) const { return w != o.w ? w < o.w : g < o.g; }
};

// Anchors of one locus produce many identical (window, node) jobs (sibling leaves share their parent's window, anchors with the
// same indel drift share the root window). Identical inputs give identical outputs, so each distinct job runs once.
bool same_request(AlignRequest const& a, AlignRequest const& b) { return a.ref_off == b.ref_off && a.q_off == b.q_off && a.n == b.n && a.m == b.m && a.k == b.k; }
size_t request_hash(AlignRequest const& r) {
    u64 h = r.ref_off * 0x9E3779B97F4A7C15ull ^ (r.q_off + 0x7F4A7C15ull) * 0xC2B2AE3D27D4EB4Full;
    h ^= ((u64)r.n << 40) ^ ((u64)r.m << 20) ^ r.k;
    h ^= h >> 29;
    return (size_t)(h * 0xBF58476D1CE4E5B9ull);
}
void dedup_requests(hvec<AlignRequest> const& reqs, hvec<AlignRequest>& uniq, hvec<u32>& uniq_of) {
    // open-addressing table of indices into `uniq` (power-of-two size, linear probing)
    size_t cap = 16;
    while (cap < reqs.size() * 2 + 1) cap <<= 1;
    hvec<u32> table(cap, 0xFFFFFFFFu);
    uniq.clear();
    uniq.reserve(reqs.size());
    uniq_of.resize(reqs.size());
    for (size_t i = 0; i < reqs.size(); ++i) {
        size_t h = request_hash(reqs[i]) & (cap - 1);
        while (table[h] != 0xFFFFFFFFu && !same_request(uniq[table[h]], reqs[i])) h = (h + 1) & (cap - 1);
        if (table[h] == 0xFFFFFFFFu) { table[h] = (u32)uniq.size(); uniq.push_back(reqs[i]); }
        uniq_of[i] = table[h];
    }
}
// a form for distinct requests, run over the distinct ones of `reqs`: every request gets the result of its like
template <class Out, class RunUnique>
int run_deduplicated(hvec<AlignRequest> const& reqs, hvec<Out>& outs, RunUnique&& run_unique) {
    hvec<AlignRequest> uniq;
    hvec<u32> uniq_of;
    dedup_requests(reqs, uniq, uniq_of);
    hvec<Out> uouts;
    if (int const rc = run_unique(uniq, uouts)) return rc;
    outs.resize(reqs.size());
    for (size_t i = 0; i < reqs.size(); ++i) outs[i] = uouts[uniq_of[i]];
    return FLX_OK;
}

// Shapes for the jobs of one call. Many jobs: each gets the shape that costs the fewest wave slots. Few jobs (they would leave
// most SIMDs without a wave): all get one common shape with the fewest words per lane, i.e. more, shorter-running waves and a
// single launch.
int choose_shapes(hvec<AlignRequest> const& reqs, hvec<AlignShape>& shapes) {
    shapes.resize(reqs.size());
    u64 lanes = 0;
    for (size_t i = 0; i < reqs.size(); ++i) {
        shapes[i] = choose_align_shape(reqs[i].n, reqs[i].m, reqs[i].k);
        if (shapes[i].words_per_lane == 0) { set_error("query longer than the supported maximum"); return FLX_ERR_UNSUPPORTED; }
        lanes += shapes[i].lanes_per_job;
    }
    auto fits = [](AlignRequest const& r, AlignShape const& sh) {
        u32 const nw = (r.m + 63) / 64, W = sh.words_per_lane, R = sh.lanes_per_job;
        i64 const width = (i64)r.n - (i64)r.m + 2 * (i64)r.k;
        if ((nw + W - 1) / W <= R || (i64)64 * W * (R - 1) + R + 1 > width) return true;
        return sh.queue != 0 && ring_delay(r.n, r.m, r.k, W, R) + 1u <= RING_QUEUE_MAX;      // (a ring that waits: DeviceApi::align gives it the largest queue)
    };
    if (!reqs.empty() && lanes / 64 >= align_few_waves()) {
        // A launch lasts at least as long as its longest job, and the jobs of a batch differ by a few columns (unions of a locus' windows): the
        // shape is chosen per class of query words, for the class's widest band - a ring's delay is the job's own (ring_delay), so the narrower
        // jobs of the class lose nothing on it. (Per job, 10-kb root alignments over a repeat-rich reference fell into a dozen launches of two
        // shapes and took 171 ms per 16384 reads instead of 46.)
        std::map<u32, size_t> widest;                        // query words -> request with the widest band
        auto width_of = [](AlignRequest const& r) { return (i64)r.n - (i64)r.m + 2 * (i64)r.k; };
        for (size_t i = 0; i < reqs.size(); ++i) {
            u32 const nw = (reqs[i].m + 63) / 64;
            auto it = widest.find(nw);
            if (it == widest.end() || width_of(reqs[i]) > width_of(reqs[it->second])) widest[nw] = i;
        }
        for (size_t i = 0; i < reqs.size(); ++i) {
            AlignShape const cand = shapes[widest[(reqs[i].m + 63) / 64]];
            if (fits(reqs[i], cand)) shapes[i] = cand;
        }
        // a handful of jobs with a shape of their own join the most common shape that can hold them instead of getting a launch
        std::map<ShapeKey, std::pair<u32, u32>> count;       // jobs, queue
        for (auto const& sh : shapes) { auto& c = count[ShapeKey{sh.words_per_lane, sh.lanes_per_job}]; c.first++; c.second = std::max(c.second, sh.queue); }
        if (count.size() > 1) {
            for (size_t i = 0; i < reqs.size(); ++i) {
                ShapeKey const mine{shapes[i].words_per_lane, shapes[i].lanes_per_job};
                if (count[mine].first >= 64) continue;
                u32 best_n = 0;
                AlignShape best = shapes[i];
                for (auto const& kv : count) {
                    AlignShape const cand{kv.first.w, kv.first.g, kv.second.second};
                    if (kv.second.first >= 64 && kv.second.first > best_n && fits(reqs[i], cand)) { best_n = kv.second.first; best = cand; }
                }
                shapes[i] = best;
            }
        }
        return FLX_OK;
    }
    if (reqs.empty()) return FLX_OK;
    AlignShape common{0, 0};
    for (size_t i = 0; i < reqs.size(); ++i) {
        AlignShape const p = choose_align_shape(reqs[i].n, reqs[i].m, reqs[i].k, true);
        if (p.words_per_lane > common.words_per_lane) common.words_per_lane = p.words_per_lane;
    }
    // lanes each job needs at the common words per lane
    for (size_t i = 0; i < reqs.size(); ++i) {
        u32 const nw = (reqs[i].m + 63) / 64, W = common.words_per_lane;
        i64 const width = (i64)reqs[i].n - (i64)reqs[i].m + 2 * (i64)reqs[i].k;
        u32 r = 1;
        while (r < 64 && !((nw + W - 1) / W <= r || (i64)64 * W * (r - 1) + r + 1 > width)) r *= 2;
        if (r > common.lanes_per_job) common.lanes_per_job = r;
    }
    for (auto& sh : shapes) sh = common;
    return FLX_OK;
}

// K3 / K4 over the requests [begin, end) of one call: one launch per shape class, the classes in ShapeKey order, the jobs of a class in
// request order (TRACE launches: widest window first, equal widths in request order). A job writes to out_index = its request - begin.
// per_job(request, job) sets what the caller's form adds to the job (trace arena and last-row offsets: it is called in job order) and
// returns the bytes the job moves beyond its n + m sequence symbols (the launch's accounting).
struct ShapeLaunch { ShapeKey key; u32 first, count; u64 word_steps, bytes; };
template <class PerJob>
int launch_by_shape(Lane* ctx, const u8* d_text, const u64* d_peq, hvec<AlignRequest> const& reqs, hvec<AlignShape> const& shapes, size_t begin, size_t end,
                    const char* kernel_name, const char* what, bool trace, u16* d_lastrow, DevAlignOut** d_out, PerJob&& per_job) {
    std::map<ShapeKey, hvec<u32>> by_shape;
    for (size_t i = begin; i < end; ++i) by_shape[ShapeKey{shapes[i].words_per_lane, shapes[i].lanes_per_job}].push_back((u32)i);
    hvec<DevAlignJob> jobs;
    jobs.reserve(end - begin);
    hvec<ShapeLaunch> launches;
    for (auto& kv : by_shape) {
        auto& ids = kv.second;
        if (trace) std::stable_sort(ids.begin(), ids.end(), [&](u32 a, u32 b) { return reqs[a].n > reqs[b].n; });
        ShapeLaunch l{kv.first, (u32)jobs.size(), (u32)ids.size(), 0, 0};
        for (u32 id : ids) {
            AlignRequest const& r = reqs[id];
            jobs.push_back(DevAlignJob{r.ref_off, r.q_off, 0, r.n, r.m, r.k, (u32)(id - begin), 0});
            l.word_steps += job_word_steps(r.n, r.m, r.k, shapes[id]);
            l.bytes += (u64)r.n + r.m + per_job(id, jobs.back());
        }
        launches.push_back(l);
    }
    int rc;
    if ((rc = h2d(ctx, ctx->jobs, jobs.data(), jobs.size() * sizeof(DevAlignJob)))) return rc;
    // the results: into the lane's mapped result block when it has room (read in place after the stream wait), else on the device
    // (*d_out tells the caller where)
    *d_out = (DevAlignOut*)ctx->result_slot((end - begin) * sizeof(DevAlignOut));
    if (!*d_out) {
        if ((rc = ctx->job_out.ensure((end - begin) * sizeof(DevAlignOut)))) return rc;
        *d_out = ctx->job_out.as<DevAlignOut>();
    }
    DevAlignOut* const out = *d_out;
    for (auto const& l : launches) {
        if (getenv("FLX_ALIGN_DEBUG")) fprintf(stderr, "[%s]%s W %u R %u jobs %u word-steps %llu n0 %u m0 %u k0 %u\n", kernel_name, what, l.key.w, l.key.g, l.count, (unsigned long long)l.word_steps, jobs[l.first].n, jobs[l.first].m, jobs[l.first].k);
        rc = timed_launch(ctx, kernel_name, l.bytes, l.word_steps, [&] {
            return DeviceApi::align(ctx->stream, d_text, d_peq, ctx->jobs.as<DevAlignJob>() + l.first, l.count, AlignShape{l.key.w, l.key.g}, trace,
                                    trace ? ctx->trace.as<u64>() : nullptr, out, d_lastrow);
        });
        if (rc) return rc;
    }
    return FLX_OK;
}

// a result table that a launch left at `src`: read in place when it is in the lane's mapped block (after the wait the caller makes
// next), copied when it is on the device
template <class T>
int fetch_results(Lane* lane, hvec<T>& dst, const T* src, bool& in_place) {
    char const* const lo = (char const*)lane->results.ptr;
    in_place = lo && (char const*)src >= lo && (char const*)src < lo + lane->results.cap;
    return in_place ? FLX_OK : d2h(lane, dst.data(), src, dst.size() * sizeof(T));
}

// score + end column for every (distinct) request (no trace)
int run_score_jobs_unique(Lane* ctx, const u8* d_text, const u64* d_peq, hvec<AlignRequest> const& reqs,
                          hvec<DevAlignOut>& outs, const char* kernel_name) {
    outs.assign(reqs.size(), DevAlignOut{0xFFFFFFFFu, 0});
    if (reqs.empty()) return FLX_OK;
    PhaseTimer jprof("score-jobs");
    hvec<AlignShape> shapes;
    int rc;
    if ((rc = choose_shapes(reqs, shapes))) return rc;
    jprof.mark("shapes");
    ResultScope const scope(ctx);
    DevAlignOut* d_out = nullptr;
    bool in_place = false;
    if ((rc = launch_by_shape(ctx, d_text, d_peq, reqs, shapes, 0, reqs.size(), kernel_name, "", false, nullptr, &d_out, [](u32, DevAlignJob&) { return (u64)0; }))) return rc;
    if ((rc = fetch_results(ctx, outs, d_out, in_place))) return rc;
    jprof.mark("launch");
    rc = ctx->sync();
    if (!rc && in_place) memcpy(outs.data(), d_out, outs.size() * sizeof(DevAlignOut));
    jprof.mark("wait");
    return rc;
}

// The trace arena of one call: the launch shape and the trace slots (16 bytes each) of every request, and the cut of the requests into
// chunks whose trace planes fit the lane's budget together.
struct TracePlan {
    hvec<AlignShape> shapes;
    hvec<u64> slots;
    u64 budget_slots = 0;
    size_t next = 0;                                           // the first request of the next chunk
    int make(Lane* lane, hvec<AlignRequest> const& reqs) {
        if (int const rc = choose_shapes(reqs, shapes)) return rc;
        slots.resize(reqs.size());
        budget_slots = std::max<u64>(lane->trace_budget_bytes / 16, 1);
        for (size_t i = 0; i < reqs.size(); ++i) {
            slots[i] = align_trace_slots(reqs[i].n, reqs[i].m, reqs[i].k, shapes[i]);
            if (slots[i] > budget_slots) { set_error("one alignment needs more trace memory than the configured budget (FLX_TRACE_ARENA_MB)"); return FLX_ERR_CAPACITY; }
        }
        return FLX_OK;
    }
    bool done() const { return next == slots.size(); }
    // the next chunk [begin, end); the lane's arena holds its planes afterwards
    int next_chunk(Lane* lane, size_t& begin, size_t& end) {
        begin = next;
        u64 used = 0;
        while (next < slots.size() && used + slots[next] <= budget_slots) { used += slots[next]; ++next; }
        end = next;
        // the arena is taken whole on first use (its size is the configured budget): no reallocation between batches
        return lane->trace.ensure(std::max<size_t>(used * 16 + 64, lane->trace.ptr ? 0 : std::min<size_t>(lane->trace_budget_bytes, (size_t)budget_slots * 16) / 3 * 2));
    }
};

constexpr size_t REALIGN_LAUNCH_JOBS = 4096;      // jobs of one cigar_realign launch at most

// K5 over the paths of one arena chunk, and their MD strings (flx_md.hip) when wanted: one MD job per trace job. The MD jobs go up with
// the trace jobs, md_build is queued directly behind K5 (it reads K5's DevTraceOut and CIGAR words on the device: no host synchronisation
// in between), and the bytes come back with the CIGAR words. A job's CIGAR slab holds 2 NM + 2 words and its MD slab md_slab_bytes(NM)
// bytes, NM being what K4 returned for it; the slabs are kept as they are (gaps included): no host repacking. The paths' tails
// (flx_tails.hip) when wanted: one tail job per trace job as well, cigar_tails queued behind K5 (behind md_build if both are on), its
// 32-byte results back with the CIGAR words. Left-aligned gaps (flx_leftalign.hip) when wanted: one job per trace job again,
// cigar_left_align queued between K5 and md_build; it writes the normalised words into a second slab buffer of the same layout and
// rewrites K5's DevTraceOuts, and everything behind it (md_build, cigar_tails, the copy back) takes that buffer instead of K5's. The cs
// strings (flx_cs.hip) when wanted: one job per trace job once more, cs_build queued behind md_build's place on the same words and
// DevTraceOuts, a slab of cs_slab_bytes per job under the NM that sizes the MD slab, its bytes back with the CIGAR words.
struct Traceback {
    bool const want_md;
    const TailParams* const want_tails;
    const u8* const d_la_query;                                // null: gaps stay where K5 put them
    bool const want_left_align;
    const RealignScores* const realign;                        // null: the paths stay edit-distance paths
    const u8* const d_ra_query;                                // the device query pool's letters for cigar_realign
    const CsWant* const cs;                                    // null: no cs strings
    PhaseTimer* const prof;
    hvec<DevTraceJob> jobs;
    hvec<DevTraceOut> outs;
    hvec<DevMdJob> md_jobs;
    hvec<DevMdOut> md_outs;
    hvec<DevTailJob> tail_jobs;
    hvec<DevTailOut> tail_outs;
    hvec<DevLeftAlignJob> la_jobs;
    hvec<DevLeftAlignStat> la_stats;
    hvec<DevRealignJob> ra_jobs;
    hvec<DevRealignStat> ra_stats;
    hvec<DevCsJob> cs_jobs;
    hvec<DevCsOut> cs_outs;
    u64 cigar_words = 0, path_steps = 0, md_bytes = 0, cs_bytes = 0;
    size_t cigar_base = 0, md_base = 0, cs_base = 0;           // where this batch's slabs start in the host pools
    explicit Traceback(bool md, const TailParams* tails, const u8* d_la_query_, PhaseTimer* prof_ = nullptr, const RealignScores* realign_ = nullptr,
                       const u8* d_ra_query_ = nullptr, const CsWant* cs_ = nullptr)
        : want_md(md), want_tails(tails), d_la_query(d_la_query_), want_left_align(d_la_query_ != nullptr), realign(d_ra_query_ ? realign_ : nullptr),
          d_ra_query(d_ra_query_), cs(cs_), prof(prof_) {}
    // the path that ends at end_col of the last row of r's DP, whose trace planes lie at trace_off; returns the trace job's index
    u32 add(AlignRequest const& r, u64 trace_off, AlignShape sh, u32 end_col, u32 nm) {
        // runs <= 2*NM + 1; a realigned path has at most realign_cap words (left-aligned too: gaps only merge there) and its NM stays
        // below realign_nm_bound, which sizes its MD slab
        u32 const j = (u32)jobs.size(), cap = realign ? (u32)std::max<u64>(2 * nm + 2, realign_cap(nm, 0, *realign)) : 2 * nm + 2;
        u32 const nm_md = realign ? (u32)realign_nm_bound(nm, *realign) : nm;
        jobs.push_back(DevTraceJob{r.ref_off, r.q_off, trace_off, cigar_words, r.n, r.m, sh.lanes_per_job, sh.words_per_lane, end_col, cap, j, r.k});
        if (want_md) {
            u64 const slab = md_slab_bytes(nm_md);
            md_jobs.push_back(DevMdJob{r.ref_off, cigar_words, md_bytes, r.n, (u32)slab, j, 0});
            md_bytes += slab;
        }
        if (want_tails) tail_jobs.push_back(DevTailJob{cigar_words, j, want_tails->w, want_tails->x_drop, want_tails->min_rows});
        if (want_left_align) la_jobs.push_back(DevLeftAlignJob{r.ref_off, r.q_off, cigar_words, cigar_words, r.n, r.m, cap, j});      // (<= 2 NM + 1 words after it too)
        // (the diagonals of an edit path of NM errors span at most NM: the trace of a band of NM + 2 w + 1 cells always suffices)
        if (realign)
            ra_jobs.push_back(DevRealignJob{r.ref_off, r.q_off, cigar_words, cigar_words, 0, r.n, r.m, cap, j,
                                            (u32)std::min<u64>(realign_trace_words(r.m, (u64)nm + 2u * (u64)realign->w + 1u), 0xFFFFFFFFull), 0});
        if (cs) {
            u64 const slab = cs_slab_bytes(nm_md, r.m, cs->form);
            cs_jobs.push_back(DevCsJob{r.ref_off, r.q_off, cigar_words, cs_bytes, r.n, r.m, (u32)slab, j});
            cs_bytes += slab;
        }
        cigar_words += cap;
        path_steps += (u64)r.m + nm;
        return j;
    }
    int run(Lane* lane, const u8* d_text, const u64* d_peq, hvec<u32>& cigar_pool, hvec<u8>* md_pool) {
        cigar_base = cigar_pool.size();
        if (jobs.empty()) return FLX_OK;
        int rc;
        // the job tables (trace, MD, tails, left-align) up in one copy, packed in the lane's staging block
        auto const up = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
        size_t const b_jobs = jobs.size() * sizeof(DevTraceJob), b_md = md_jobs.size() * sizeof(DevMdJob), b_tail = tail_jobs.size() * sizeof(DevTailJob),
                     b_la = la_jobs.size() * sizeof(DevLeftAlignJob), b_cs = cs_jobs.size() * sizeof(DevCsJob);
        size_t const o_md = up(b_jobs), o_tail = o_md + up(b_md), o_la = o_tail + up(b_tail), o_cs = o_la + up(b_la),
                     b_tables = b_cs ? o_cs + b_cs : b_la ? o_la + b_la : o_tail + b_tail;
        if ((rc = lane->tjobs.ensure(b_tables + 16))) return rc;
        char* const h = (char*)lane->stage_begin(b_tables);
        if (!h) return FLX_ERR_NO_DEVICE;
        memcpy(h, jobs.data(), b_jobs);
        if (b_md) memcpy(h + o_md, md_jobs.data(), b_md);
        if (b_tail) memcpy(h + o_tail, tail_jobs.data(), b_tail);
        if (b_la) memcpy(h + o_la, la_jobs.data(), b_la);
        if (b_cs) memcpy(h + o_cs, cs_jobs.data(), b_cs);
        FLX_HIP(hipMemcpyAsync(lane->tjobs.ptr, h, b_tables, hipMemcpyHostToDevice, lane->stream));
        const DevTraceJob* const d_jobs = lane->tjobs.as<DevTraceJob>();
        const DevMdJob* const d_md_jobs = (const DevMdJob*)((char*)lane->tjobs.ptr + o_md);
        const DevTailJob* const d_tail_jobs = (const DevTailJob*)((char*)lane->tjobs.ptr + o_tail);
        const DevLeftAlignJob* const d_la_jobs = (const DevLeftAlignJob*)((char*)lane->tjobs.ptr + o_la);
        const DevCsJob* const d_cs_jobs = (const DevCsJob*)((char*)lane->tjobs.ptr + o_cs);
        if ((rc = lane->tjob_out.ensure(jobs.size() * sizeof(DevTraceOut)))) return rc;
        if ((rc = lane->cigar.ensure(cigar_words * 4 + 16))) return rc;
        if (want_md) {
            if ((rc = lane->md_out.ensure(md_jobs.size() * sizeof(DevMdOut)))) return rc;
            if ((rc = lane->md.ensure(md_bytes + 16))) return rc;
        }
        if (want_tails && (rc = lane->tail_out.ensure(tail_jobs.size() * sizeof(DevTailOut)))) return rc;
        if (cs && (rc = lane->cs.ensure(cs_bytes + 16))) return rc;
        if (want_left_align) {
            if ((rc = lane->cigar_la.ensure(cigar_words * 4 + 16))) return rc;
            if ((rc = lane->la_stat.ensure(la_jobs.size() * sizeof(DevLeftAlignStat)))) return rc;
        }
        // cigar_realign's launches: at most REALIGN_LAUNCH_JOBS jobs each, their traces together inside the arena as it stands (K4's
        // planes lie there until K5 has read them: it is not grown here)
        hvec<size_t> ra_cuts{0};
        if (realign) {
            u64 const arena_words = lane->trace.cap / 4;
            u64 used = 0;
            for (size_t k = 0; k < ra_jobs.size(); ++k) {
                if (ra_jobs[k].trace_cap > arena_words) ra_jobs[k].trace_cap = (u32)std::min<u64>(arena_words, 0xFFFFFFFFull);
                if (k - ra_cuts.back() == REALIGN_LAUNCH_JOBS || used + ra_jobs[k].trace_cap > arena_words) { ra_cuts.push_back(k); used = 0; }
                ra_jobs[k].trace_off = used;
                used += ra_jobs[k].trace_cap;
            }
            ra_cuts.push_back(ra_jobs.size());
            if ((rc = h2d(lane, lane->ra_jobs, ra_jobs.data(), ra_jobs.size() * sizeof(DevRealignJob)))) return rc;
            if ((rc = lane->cigar_ra.ensure(cigar_words * 4 + 16))) return rc;
        }
        // the words everything behind K5 reads: K5's, the realigned or the normalised ones
        u32* const d_ra_words = realign ? lane->cigar_ra.as<u32>() : lane->cigar.as<u32>();
        u32* const d_words = want_left_align ? lane->cigar_la.as<u32>() : d_ra_words;
        // The small result tables (16 bytes per path, MD lengths, tails) come back through the lane's mapped result block when it holds them
        // all: K5 stores its DevTraceOuts there itself when nothing on the device reads them; md_build, cigar_tails and cigar_left_align read them, so with
        // any of them they stay on the device and one publish_stage launch behind the stage hands all the tables over.
        outs.resize(jobs.size());
        md_outs.resize(md_jobs.size());
        tail_outs.resize(tail_jobs.size());
        la_stats.resize(la_jobs.size());
        ra_stats.resize(ra_jobs.size());
        cs_outs.resize(cs_jobs.size());
        DevTraceOut* r_outs = (DevTraceOut*)lane->result_slot(outs.size() * sizeof(DevTraceOut));
        DevMdOut* r_md = want_md ? (DevMdOut*)lane->result_slot(md_outs.size() * sizeof(DevMdOut)) : nullptr;
        DevTailOut* r_tail = want_tails ? (DevTailOut*)lane->result_slot(tail_outs.size() * sizeof(DevTailOut)) : nullptr;
        DevLeftAlignStat* r_la = want_left_align ? (DevLeftAlignStat*)lane->result_slot(la_stats.size() * sizeof(DevLeftAlignStat)) : nullptr;
        DevRealignStat* r_ra = realign ? (DevRealignStat*)lane->result_slot(ra_stats.size() * sizeof(DevRealignStat)) : nullptr;
        bool const mapped = r_outs && (!want_md || r_md) && (!want_tails || r_tail) && (!want_left_align || r_la);
        // (nothing on the device reads cigar_realign's statistics: the kernel stores them in the block itself when it has room)
        if (realign && !r_ra && (rc = lane->ra_stat.ensure(ra_jobs.size() * sizeof(DevRealignStat)))) return rc;
        DevRealignStat* const d_ra_stats = r_ra ? r_ra : lane->ra_stat.as<DevRealignStat>();
        // (nor cs_build's lengths)
        DevCsOut* const r_cs = cs ? (DevCsOut*)lane->result_slot(cs_outs.size() * sizeof(DevCsOut)) : nullptr;
        if (cs && !r_cs && (rc = lane->cs_out.ensure(cs_jobs.size() * sizeof(DevCsOut)))) return rc;
        DevCsOut* const d_cs_outs = r_cs ? r_cs : lane->cs_out.as<DevCsOut>();
        bool const direct = mapped && !want_md && !want_tails && !want_left_align && !realign && !cs;
        DevTraceOut* const d_outs = direct ? r_outs : lane->tjob_out.as<DevTraceOut>();
        rc = timed_launch(lane, "ed_traceback", path_steps * 18, path_steps, [&] {
            return DeviceApi::traceback(lane->stream, d_text, d_peq, lane->trace.as<u64>(), d_jobs, (u32)jobs.size(), lane->cigar.as<u32>(), d_outs);
        });
        if (rc) return rc;
        for (size_t c = 0; realign && c + 1 < ra_cuts.size(); ++c) {
            size_t const first = ra_cuts[c], count = ra_cuts[c + 1] - first;
            // (the cells it computes are known once its results are back: they are added below)
            rc = timed_launch(lane, "cigar_realign", count * (sizeof(DevRealignJob) + 2 * sizeof(DevTraceOut) + sizeof(DevRealignStat)), 0, [&] {
                return DeviceApi::cigar_realign(lane->stream, d_text, d_ra_query, lane->cigar.as<u32>(), d_outs, lane->ra_jobs.as<DevRealignJob>() + first,
                                                (u32)count, *realign, lane->trace.as<u32>(), d_ra_words, d_ra_stats);
            });
            if (rc) return rc;
        }
        if (want_left_align) {
            // (the words it reads and writes and the letters it compares are known once its results are back: they are added below)
            rc = timed_launch(lane, "cigar_left_align", la_jobs.size() * (sizeof(DevLeftAlignJob) + 2 * sizeof(DevTraceOut) + sizeof(DevLeftAlignStat)), 0, [&] {
                return DeviceApi::cigar_left_align(lane->stream, d_text, d_la_query, d_ra_words, d_outs, d_la_jobs, (u32)la_jobs.size(), d_words,
                                                   lane->la_stat.as<DevLeftAlignStat>());
            });
            if (rc) return rc;
        }
        if (want_md) {
            // (its algorithmic bytes depend on what K5 finds: they are added below once the lengths are back)
            rc = timed_launch(lane, "md_build", 0, md_jobs.size(), [&] {
                return DeviceApi::md_build(lane->stream, d_text, d_words, d_outs, d_md_jobs, (u32)md_jobs.size(), lane->md.as<u8>(), lane->md_out.as<DevMdOut>());
            });
            if (rc) return rc;
        }
        if (cs) {
            // (what it reads and writes is known once the lengths are back: added below)
            rc = timed_launch(lane, "cs_build", 0, 0, [&] {
                return DeviceApi::cs_build(lane->stream, d_text, cs->d_query, d_words, d_outs, d_cs_jobs, (u32)cs_jobs.size(), cs->form, lane->cs.as<u8>(), d_cs_outs);
            });
            if (rc) return rc;
        }
        if (want_tails) {
            // (the CIGAR words it reads are known once K5's lengths are back: they are added below)
            rc = timed_launch(lane, "cigar_tails", tail_jobs.size() * (sizeof(DevTailJob) + sizeof(DevTraceOut) + sizeof(DevTailOut)), tail_jobs.size(), [&] {
                return DeviceApi::cigar_tails(lane->stream, d_words, d_outs, d_tail_jobs, (u32)tail_jobs.size(), lane->tail_out.as<DevTailOut>());
            });
            if (rc) return rc;
        }
        if (mapped && !direct) {
            PublishList pub;
            pub.add(lane->tjob_out.ptr, r_outs, outs.size() * sizeof(DevTraceOut) / 4);
            if (want_md) pub.add(lane->md_out.ptr, r_md, md_outs.size() * sizeof(DevMdOut) / 4);
            if (want_tails) pub.add(lane->tail_out.ptr, r_tail, tail_outs.size() * sizeof(DevTailOut) / 4);
            if (want_left_align) pub.add(lane->la_stat.ptr, r_la, la_stats.size() * sizeof(DevLeftAlignStat) / 4);
            int const e = DeviceApi::publish_stage(lane->stream, pub);
            if (e) { set_error(std::string("publish_stage: ") + hipGetErrorString((hipError_t)e)); return FLX_ERR_NO_DEVICE; }
        }
        if (prof) prof->mark("tb-prep");
        cigar_pool.resize(cigar_base + cigar_words);
        if (prof) prof->mark("pool-resize");
        if (!mapped && (rc = d2h(lane, outs.data(), lane->tjob_out.ptr, outs.size() * sizeof(DevTraceOut)))) return rc;
        if ((rc = d2h(lane, cigar_pool.data() + cigar_base, d_words, cigar_words * 4))) return rc;
        if (want_md) {
            md_base = md_pool->size();
            md_pool->resize(md_base + md_bytes);
            if (!mapped && (rc = d2h(lane, md_outs.data(), lane->md_out.ptr, md_outs.size() * sizeof(DevMdOut)))) return rc;
            if ((rc = d2h(lane, md_pool->data() + md_base, lane->md.ptr, md_bytes))) return rc;
        }
        if (cs) {
            cs_base = cs->pool->size();
            cs->pool->resize(cs_base + cs_bytes);
            if (!r_cs && (rc = d2h(lane, cs_outs.data(), lane->cs_out.ptr, cs_outs.size() * sizeof(DevCsOut)))) return rc;
            if ((rc = d2h(lane, cs->pool->data() + cs_base, lane->cs.ptr, cs_bytes))) return rc;
        }
        if (want_tails && !mapped && (rc = d2h(lane, tail_outs.data(), lane->tail_out.ptr, tail_outs.size() * sizeof(DevTailOut)))) return rc;
        if (want_left_align && !mapped && (rc = d2h(lane, la_stats.data(), lane->la_stat.ptr, la_stats.size() * sizeof(DevLeftAlignStat)))) return rc;
        if (realign && !r_ra && (rc = d2h(lane, ra_stats.data(), lane->ra_stat.ptr, ra_stats.size() * sizeof(DevRealignStat)))) return rc;
        if ((rc = lane->sync())) return rc;
        if (r_ra) memcpy(ra_stats.data(), r_ra, ra_stats.size() * sizeof(DevRealignStat));
        if (r_cs) memcpy(cs_outs.data(), r_cs, cs_outs.size() * sizeof(DevCsOut));
        if (mapped) {
            memcpy(outs.data(), r_outs, outs.size() * sizeof(DevTraceOut));
            if (want_left_align) memcpy(la_stats.data(), r_la, la_stats.size() * sizeof(DevLeftAlignStat));
            if (want_md) memcpy(md_outs.data(), r_md, md_outs.size() * sizeof(DevMdOut));
            if (want_tails) memcpy(tail_outs.data(), r_tail, tail_outs.size() * sizeof(DevTailOut));
        }
        if (prof) prof->mark("K5+d2h");
        for (auto const& t : outs)
            if (t.cigar_len == 0xFFFFFFFFu) { set_error(want_left_align || realign ? "ed_traceback / cigar_realign / cigar_left_align: CIGAR slab overflow" : "ed_traceback: CIGAR slab overflow"); return FLX_ERR_INTERNAL; }
        if (realign) {
            // the trace is written once and read along the path + the words written; units: DP cells
            u64 bytes = 0, cells = 0, changed = 0, kept = 0;
            for (size_t j = 0; j < ra_jobs.size(); ++j) {
                bytes += ra_stats[j].cells / 2 + 4ull * outs[j].cigar_len;
                cells += ra_stats[j].cells; changed += ra_stats[j].changed; kept += ra_stats[j].kept;
            }
            lane->ctx->account_more("cigar_realign", bytes, cells);
            std::lock_guard<std::mutex> g(lane->ctx->mu);
            lane->ctx->realign.paths_realigned += ra_jobs.size() - kept;
            lane->ctx->realign.paths_changed += changed;
            lane->ctx->realign.paths_kept += kept;
        }
        if (want_left_align) {
            // CIGAR words read and written + letters compared (both sides of every comparison); units: the gap words that moved or merged
            u64 bytes = 0, moved = 0;
            for (size_t j = 0; j < la_jobs.size(); ++j) { bytes += 4ull * la_stats[j].words_in + 4ull * outs[j].cigar_len + 2ull * la_stats[j].letters; moved += la_stats[j].moved; }
            lane->ctx->account_more("cigar_left_align", bytes, moved);
        }
        if (want_md) {
            // CIGAR words read + reference letters read (one per X / D column: at most NM) + MD bytes written
            u64 bytes = 0;
            for (size_t j = 0; j < md_jobs.size(); ++j) {
                if (md_outs[j].len == 0xFFFFFFFFu) { set_error("md_build: MD slab overflow, or a path that leaves its window"); return FLX_ERR_INTERNAL; }
                bytes += 4ull * outs[j].cigar_len + md_outs[j].len + (md_jobs[j].md_cap - 6u) / 8u;
            }
            lane->ctx->account_more("md_build", bytes, 0);
        }
        if (cs) {
            // CIGAR words read + the string written + a letter read per letter written (at most the string again); units: output bytes
            u64 bytes = 0, written = 0;
            for (size_t j = 0; j < cs_jobs.size(); ++j) {
                if (cs_outs[j].len == 0xFFFFFFFFu) { set_error("cs_build: cs slab overflow, or a path that leaves its window or its query"); return FLX_ERR_INTERNAL; }
                bytes += 4ull * outs[j].cigar_len + 2ull * cs_outs[j].len;
                written += cs_outs[j].len;
            }
            lane->ctx->account_more("cs_build", bytes, written);
        }
        if (want_tails) {
            u64 bytes = 0;
            for (auto const& t : outs) bytes += 4ull * t.cigar_len;
            lane->ctx->account_more("cigar_tails", bytes, 0);
        }
        return FLX_OK;
    }
    // trace job j as the result of a request whose K4 score was nm (begin: relative to the job's window)
    TraceResult result(u32 j, u32 nm) const {
        TraceResult res;
        res.exists = true;
        res.nm = res.ed = nm;
        res.begin = outs[j].begin;
        res.cigar_off = cigar_base + jobs[j].cigar_off + outs[j].cigar_start;
        res.cigar_len = outs[j].cigar_len;
        if (want_md) { res.md_off = md_base + md_jobs[j].md_off; res.md_len = md_outs[j].len; }
        if (cs) { res.cs_off = cs_base + cs_jobs[j].cs_off; res.cs_len = cs_outs[j].len; }
        if (want_tails) res.tail = tail_outs[j];
        if (realign) { res.nm = ra_stats[j].num_errors; res.score = ra_stats[j].score; }      // (a kept path: NM is K4's)
        return res;
    }
};

// score, begin position and CIGAR (and MD string, when md_pool is given) for every (distinct) request
int run_trace_jobs_unique(Lane* ctx, const u8* d_text, const u64* d_peq, hvec<AlignRequest> const& reqs,
                          hvec<TraceResult>& results, hvec<u32>& cigar_pool, hvec<u8>* md_pool, const TailParams* tails, const u8* d_la_query,
                          const RealignScores* realign, const u8* d_ra_query, const CsWant* cs) {
    results.assign(reqs.size(), TraceResult{});
    if (reqs.empty()) return FLX_OK;
    PhaseTimer tprof("trace-jobs");
    TracePlan plan;
    int rc;
    if ((rc = plan.make(ctx, reqs))) return rc;
    while (!plan.done()) {
        size_t begin, end;
        if ((rc = plan.next_chunk(ctx, begin, end))) return rc;
        size_t const count = end - begin;
        hvec<u64> trace_off(count);
        u64 off = 0;
        // (bytes: reference + query symbols read; trace written: the checkpointed trace's carry and checkpoint regions)
        ResultScope const scope(ctx);
        DevAlignOut* d_out = nullptr;
        bool in_place = false;
        rc = launch_by_shape(ctx, d_text, d_peq, reqs, plan.shapes, begin, end, "ed_align_trace", "", true, nullptr, &d_out, [&](u32 id, DevAlignJob& job) {
            AlignRequest const& r = reqs[id];
            job.trace_off = trace_off[id - begin] = off;
            off += plan.slots[id];
            TraceLayout const tl = ckpt_trace_layout(r.n, r.m, r.k, plan.shapes[id].words_per_lane, plan.shapes[id].lanes_per_job);
            return (tl.carry_slots + tl.ckpt_slots) * 16;
        });
        if (rc) return rc;
        hvec<DevAlignOut> outs(count);
        if ((rc = fetch_results(ctx, outs, d_out, in_place))) return rc;
        if ((rc = ctx->sync())) return rc;
        if (in_place) memcpy(outs.data(), d_out, count * sizeof(DevAlignOut));
        tprof.mark("K4");

        // ---- traceback for the jobs that have an alignment within k
        Traceback tb(md_pool != nullptr, tails, d_la_query, &tprof, realign, d_ra_query, cs);
        hvec<u32> tjob_req;
        for (size_t c = 0; c < count; ++c) {
            if (outs[c].score == 0xFFFFFFFFu) continue;
            tb.add(reqs[begin + c], trace_off[c], plan.shapes[begin + c], outs[c].end_col, outs[c].score);
            tjob_req.push_back((u32)(begin + c));
        }
        if ((rc = tb.run(ctx, d_text, d_peq, cigar_pool, md_pool))) return rc;
        for (u32 j = 0; j < tjob_req.size(); ++j) results[tjob_req[j]] = tb.result(j, outs[tjob_req[j] - begin].score);
    }
    return FLX_OK;
}

}  // namespace

int run_score_jobs(Lane* ctx, const u8* d_text, const u64* d_peq, hvec<AlignRequest> const& reqs,
                   hvec<DevAlignOut>& outs, const char* kernel_name) {
    return run_deduplicated(reqs, outs, [&](hvec<AlignRequest> const& uniq, hvec<DevAlignOut>& uouts) {
        return run_score_jobs_unique(ctx, d_text, d_peq, uniq, uouts, kernel_name);
    });
}

// score, begin position and CIGAR for every request (alignment.cpp:147-180); CIGAR words land in cigar_pool (shared by duplicates)
int run_trace_jobs(Lane* ctx, const u8* d_text, const u64* d_peq, hvec<AlignRequest> const& reqs,
                   hvec<TraceResult>& results, hvec<u32>& cigar_pool, hvec<u8>* md_pool, const TailParams* tails, const u8* d_la_query,
                   const RealignScores* realign, const u8* d_ra_query, const CsWant* cs) {
    return run_deduplicated(reqs, results, [&](hvec<AlignRequest> const& uniq, hvec<TraceResult>& ures) {
        return run_trace_jobs_unique(ctx, d_text, d_peq, uniq, ures, cigar_pool, md_pool, tails, d_la_query, realign, d_ra_query, cs);
    });
}

// Existence tests of one locus. Anchors of the same read at the same locus test the same node in windows shifted by their indel
// drift. Existence is monotone in the window: an alignment inside the intersection I of such windows lies inside every one of them,
// and if their union U holds none then neither does any of them. So a cluster first tests I (one job instead of one per member);
// only if that fails it tests U, and only if U holds an alignment that I does not are the members tested one by one.
// outs[i].score is 0xFFFFFFFF for "no alignment within k" and some score <= k of a contained alignment otherwise (callers of
// this function only look at that distinction); outs[i].end_col is not meaningful.
int run_exists_jobs(Lane* ctx, const u8* d_text, const u64* d_peq, hvec<AlignRequest> const& reqs, hvec<DevAlignOut>& outs, ExistsTimes& times) {
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](int slot) { auto const t1 = std::chrono::steady_clock::now(); times.ms[slot] += std::chrono::duration<double, std::milli>(t1 - t0).count(); t0 = t1; };
    // The requests come in anchor order, and the anchors of a read and orientation are in leaf order: all requests for one node
    // (the leaves below it are a contiguous range) form one run of equal (query rows, errors). Sorting a run by reference
    // position puts equal windows and the windows of one locus next to each other: no hash table, no sort of the whole round.
    // (Requests for one node that are not adjacent would only be tested more than once.)
    static int const disabled = (getenv("FLX_NO_UNION") || getenv("FLX_NO_EXISTS_CLUSTERS")) ? 1 : 0;
    hvec<AlignRequest> uniq;
    hvec<u32> uniq_of(reqs.size());
    struct Cluster { u32 first, count; u64 lo_start, hi_start, lo_end, hi_end; };     // members = uniq[first .. first+count)
    hvec<Cluster> clusters;
    uniq.reserve(reqs.size());
    hvec<u32> run;
    for (size_t i0 = 0; i0 < reqs.size();) {
        size_t i1 = i0 + 1;
        while (i1 < reqs.size() && reqs[i1].q_off == reqs[i0].q_off && reqs[i1].m == reqs[i0].m && reqs[i1].k == reqs[i0].k) ++i1;
        run.resize(i1 - i0);
        for (size_t j = 0; j < run.size(); ++j) run[j] = (u32)(i0 + j);
        if (run.size() > 1)
            std::sort(run.begin(), run.end(), [&](u32 x, u32 y) { return reqs[x].ref_off != reqs[y].ref_off ? reqs[x].ref_off < reqs[y].ref_off : reqs[x].n < reqs[y].n; });
        bool first_of_run = true;
        for (u32 idx : run) {
            AlignRequest const& r = reqs[idx];
            if (!first_of_run && uniq.back().ref_off == r.ref_off && uniq.back().n == r.n) { uniq_of[idx] = (u32)uniq.size() - 1; continue; }
            uniq_of[idx] = (u32)uniq.size();
            if (!first_of_run && !disabled) {
                Cluster& c = clusters.back();
                if (r.ref_off <= uniq[c.first].ref_off + std::max<u64>(8, r.m / 8)) {
                    c.count++;
                    c.hi_start = std::max(c.hi_start, r.ref_off);
                    c.lo_end = std::min(c.lo_end, r.ref_off + r.n);
                    c.hi_end = std::max(c.hi_end, r.ref_off + r.n);
                    uniq.push_back(r);
                    continue;
                }
            }
            clusters.push_back(Cluster{(u32)uniq.size(), 1, r.ref_off, r.ref_off, r.ref_off + r.n, r.ref_off + r.n});
            uniq.push_back(r);
            first_of_run = false;
        }
        i0 = i1;
    }
    lap(0);
    hvec<DevAlignOut> uouts(uniq.size(), DevAlignOut{0xFFFFFFFFu, 0});
    // ---- one launch: single windows on their own, clusters on their intersection and (speculatively: a separate round trip
    //      to the GPU costs a chunk more than the extra jobs) on their union
    hvec<AlignRequest> jobs;
    hvec<u32> job_cluster;                                   // cluster index, bit 31 set for the union job
    for (u32 ci = 0; ci < clusters.size(); ++ci) {
        Cluster const& c = clusters[ci];
        AlignRequest r = uniq[c.first];
        if (c.count == 1) { jobs.push_back(r); job_cluster.push_back(ci); continue; }
        if (c.lo_end > c.hi_start) {                         // the common columns (none: straight to the union and the members)
            AlignRequest i = r;
            i.ref_off = c.hi_start;
            i.n = (u32)(c.lo_end - c.hi_start);
            jobs.push_back(i);
            job_cluster.push_back(ci);
        }
        r.ref_off = c.lo_start;
        r.n = (u32)(c.hi_end - c.lo_start);
        jobs.push_back(r);
        job_cluster.push_back(ci | 0x80000000u);
    }
    hvec<DevAlignOut> jouts;
    lap(1);
    int rc = run_score_jobs_unique(ctx, d_text, d_peq, jobs, jouts, "ed_align_exists");
    if (rc) return rc;
    lap(2);
    hvec<u8> state(clusters.size(), 0);                      // 0 undecided, 1 all pass, 2 all fail
    hvec<u32> pass_score(clusters.size(), 0);
    for (size_t j = 0; j < jobs.size(); ++j) {
        u32 const ci = job_cluster[j] & 0x7FFFFFFFu;
        bool const is_union = job_cluster[j] >> 31;
        bool const found = jouts[j].score != 0xFFFFFFFFu;
        if (!is_union) {
            if (found) { state[ci] = 1; pass_score[ci] = jouts[j].score; }
            else if (clusters[ci].count == 1) state[ci] = 2;
        } else if (!found) state[ci] = 2;                   // (an intersection cannot hold an alignment the union does not)
    }
    // ---- phase C: members of the clusters that are still undecided, one by one
    jobs.clear();
    hvec<u32> job_member;
    for (u32 ci = 0; ci < clusters.size(); ++ci) {
        Cluster const& c = clusters[ci];
        if (state[ci] != 0) continue;
        for (u32 j = 0; j < c.count; ++j) { jobs.push_back(uniq[c.first + j]); job_member.push_back(c.first + j); }
    }
    if (!jobs.empty()) {
        if ((rc = run_score_jobs_unique(ctx, d_text, d_peq, jobs, jouts, "ed_align_exists"))) return rc;
        for (size_t j = 0; j < jobs.size(); ++j) uouts[job_member[j]] = jouts[j];
    }
    for (u32 ci = 0; ci < clusters.size(); ++ci) {
        if (state[ci] == 0) continue;
        Cluster const& c = clusters[ci];
        for (u32 j = 0; j < c.count; ++j) uouts[c.first + j] = DevAlignOut{state[ci] == 1 ? pass_score[ci] : 0xFFFFFFFFu, 0};
    }
    if (getenv("FLX_ALIGN_DEBUG")) {
        size_t multi = 0, decided_a = 0;
        for (u32 ci = 0; ci < clusters.size(); ++ci) if (clusters[ci].count > 1) { ++multi; if (state[ci] == 1) ++decided_a; }
        fprintf(stderr, "[exists clusters] requests %zu distinct %zu clusters %zu (of several windows %zu, passed on the intersection %zu) one by one %zu\n",
                reqs.size(), uniq.size(), clusters.size(), multi, decided_a, jobs.size());
    }
    outs.resize(reqs.size());
    for (size_t i = 0; i < reqs.size(); ++i) outs[i] = uouts[uniq_of[i]];
    lap(3);
    return FLX_OK;
}

// Root alignments of one locus. Anchors of the same read at the same locus ask for windows that differ by a few columns (their
// indel drift), ten per read with floxer's defaults, and nearly always get the same alignment. One DP over the union U of such
// windows serves them all, exactly:
//   * a window w is a column range of U, and D_U <= D_w cell by cell (U only adds start columns), with equality on every cell of
//     a D_U-optimal path that starts inside w;
//   * let j be the rightmost column of w with the minimal D_U[m][.] = v over w. If the path traced back from (m, j) in D_U starts at
//     a column of w, then D_w = D_U along it, so min D_w = v, j is also the rightmost minimum of D_w (right of j D_w >= D_U > v), and
//     the trace decisions along the path agree (a move D_U rejects is rejected by D_w as well, a move D_U takes leads to a cell of
//     the path): score, end, begin and CIGAR of w are those read off U;
//   * v > k: no alignment in w either; the path starts left of w (rare): w is aligned on its own as before.
// The band of U contains the band of every member, and a banded value is exact whenever it is <= k.
constexpr u64 UNION_MAX_SHIFT = 256;      // members start within this many columns of the first member of their union

namespace {

// the union form over distinct requests (n_requests: with their duplicates, for the debug line)
int run_trace_jobs_union_unique(Lane* ctx, const u8* d_text, const u64* d_peq, hvec<AlignRequest> const& uniq, size_t n_requests,
                                hvec<TraceResult>& ures, hvec<u32>& cigar_pool, hvec<u8>* md_pool, const TailParams* tails, const u8* d_la_query,
                                const RealignScores* realign, const u8* d_ra_query, const CsWant* cs) {
    bool usable = !uniq.empty() && !getenv("FLX_NO_UNION");
    for (auto const& r : uniq) usable = usable && r.k < 0xFFFFu;
    // ---- unions: same query rows, starts within UNION_MAX_SHIFT of the first member
    struct Union { AlignRequest req; u32 first_member, n_members; };
    hvec<u32> order(uniq.size());
    hvec<Union> unions;
    hvec<u32> members;                       // indices into uniq, grouped by union
    if (usable) {
        std::iota(order.begin(), order.end(), 0u);
        std::sort(order.begin(), order.end(), [&](u32 a, u32 b) {
            AlignRequest const &x = uniq[a], &y = uniq[b];
            if (x.q_off != y.q_off) return x.q_off < y.q_off;
            if (x.m != y.m) return x.m < y.m;
            if (x.k != y.k) return x.k < y.k;
            return x.ref_off < y.ref_off;
        });
        for (u32 id : order) {
            AlignRequest const& r = uniq[id];
            if (!unions.empty()) {
                Union& u = unions.back();
                if (u.req.q_off == r.q_off && u.req.m == r.m && u.req.k == r.k && r.ref_off <= u.req.ref_off + UNION_MAX_SHIFT) {
                    u64 const end = std::max<u64>(u.req.ref_off + u.req.n, r.ref_off + r.n);
                    u.req.n = (u32)(end - u.req.ref_off);
                    u.n_members++;
                    members.push_back(id);
                    continue;
                }
            }
            unions.push_back(Union{r, (u32)members.size(), 1});
            members.push_back(id);
        }
    }
    if (!usable || unions.size() == uniq.size()) return run_trace_jobs_unique(ctx, d_text, d_peq, uniq, ures, cigar_pool, md_pool, tails, d_la_query, realign, d_ra_query, cs);      // nothing to share: the plain path

    ures.assign(uniq.size(), TraceResult{});
    hvec<AlignRequest> ureqs(unions.size());
    for (size_t i = 0; i < unions.size(); ++i) ureqs[i] = unions[i].req;
    TracePlan plan;
    int rc;
    if ((rc = plan.make(ctx, ureqs))) return rc;
    hvec<AlignRequest> fallback;
    hvec<u32> fallback_of;                   // uniq index of each fallback request
    size_t n_tjobs = 0, n_unions_several_jobs = 0;      // (FLX_ALIGN_DEBUG: traceback jobs, unions whose members end at more than one column)
    while (!plan.done()) {
        size_t begin, next;
        if ((rc = plan.next_chunk(ctx, begin, next))) return rc;
        size_t const count = next - begin;

        // ---- K4 over the unions of this arena chunk, with their last rows
        hvec<u64> trace_off(count), row_off(count);
        u64 off = 0, rows = 0;
        for (size_t i = begin; i < next; ++i) rows += ((u64)ureqs[i].n + 15) / 16 * 16;      // K4 stores a block's 16 last-row values as two 16-byte words
        if ((rc = ctx->lastrow.ensure(rows * 2 + 64))) return rc;
        // (No fill of the last-row region: K4's last group writes whole blocks from the job's block b_lo to its last, 0xFFFF past column n,
        // and lastrow_min does not read a window's columns in front of that - lastrow_first_written, proved from enter_group's b_lo / b_hi of
        // the last group: DevRowWindow::skip below.)
        rows = 0;
        ResultScope const scope(ctx);
        DevAlignOut* d_union_out = nullptr;      // (the unions' own scores are not read: every member's comes from its window of the last row)
        rc = launch_by_shape(ctx, d_text, d_peq, ureqs, plan.shapes, begin, next, "ed_align_trace", " unions", true, ctx->lastrow.as<u16>(), &d_union_out, [&](u32 id, DevAlignJob& job) {
            AlignRequest const& r = ureqs[id];
            job.trace_off = trace_off[id - begin] = off;
            job.lastrow_off = row_off[id - begin] = rows;
            off += plan.slots[id];
            rows += ((u64)r.n + 15) / 16 * 16;
            TraceLayout const tl = ckpt_trace_layout(r.n, r.m, r.k, plan.shapes[id].words_per_lane, plan.shapes[id].lanes_per_job);
            return (tl.carry_slots + tl.ckpt_slots) * 16 + 2ull * r.n;
        });
        if (rc) return rc;
        // ---- every member's rightmost minimum over its own columns
        // (the window table is read once, by one wave per window: lastrow_min reads it where the host builds it, in the lane's staging
        // block, and leaves its results in the lane's mapped result block; a copy each way when the block has no room)
        size_t n_wins = 0;
        for (size_t ui = begin; ui < next; ++ui) n_wins += unions[ui].n_members;
        DevRowWindow* const wins = (DevRowWindow*)ctx->stage_begin(n_wins * sizeof(DevRowWindow));
        if (!wins) return FLX_ERR_NO_DEVICE;
        hvec<u32> win_member;                // uniq index per window
        hvec<u32> win_union;                 // union index (absolute) per window
        for (size_t ui = begin; ui < next; ++ui) {
            AlignRequest const& u = ureqs[ui];
            u64 const first_written = lastrow_first_written(u.n, u.m, u.k, plan.shapes[ui].words_per_lane);
            for (u32 j = 0; j < unions[ui].n_members; ++j) {
                u32 const id = members[unions[ui].first_member + j];
                AlignRequest const& r = uniq[id];
                u64 const shift = r.ref_off - u.ref_off;
                u32 const skip = (u32)std::min<u64>(first_written > shift ? first_written - shift : 0, r.n);
                wins[win_member.size()] = DevRowWindow{row_off[ui - begin] + shift, r.n, r.k, (u32)win_member.size(), skip};
                win_member.push_back(id);
                win_union.push_back((u32)ui);
            }
        }
        hvec<DevAlignOut> wouts(n_wins);
        DevAlignOut* d_wouts = (DevAlignOut*)ctx->result_slot(n_wins * sizeof(DevAlignOut));
        bool const wouts_in_place = d_wouts != nullptr;
        if (!wouts_in_place) {
            if ((rc = ctx->row_out.ensure(n_wins * sizeof(DevAlignOut)))) return rc;
            d_wouts = ctx->row_out.as<DevAlignOut>();
        }
        rc = timed_launch(ctx, "ed_lastrow_min", rows * 2, n_wins, [&] {
            return DeviceApi::lastrow_min(ctx->stream, ctx->lastrow.as<u16>(), wins, (u32)n_wins, d_wouts);
        });
        if (rc) return rc;
        if (!wouts_in_place && (rc = d2h(ctx, wouts.data(), d_wouts, n_wins * sizeof(DevAlignOut)))) return rc;
        if ((rc = ctx->sync())) return rc;
        if (wouts_in_place) memcpy(wouts.data(), d_wouts, n_wins * sizeof(DevAlignOut));

        // ---- one traceback per distinct (union, end column); the members of a union share its trace job's CIGAR words and MD string
        Traceback tb(md_pool != nullptr, tails, d_la_query, nullptr, realign, d_ra_query, cs);
        hvec<u32> win_tjob(n_wins, 0xFFFFFFFFu);
        for (size_t w0 = 0; w0 < n_wins;) {                     // windows of one union are consecutive
            size_t w1 = w0;
            while (w1 < n_wins && win_union[w1] == win_union[w0]) ++w1;
            u32 const ui = win_union[w0];
            size_t const jobs_before = tb.jobs.size();
            for (size_t w = w0; w < w1; ++w) {
                if (wouts[w].score == 0xFFFFFFFFu) continue;
                u32 const end_in_union = (u32)(uniq[win_member[w]].ref_off - ureqs[ui].ref_off) + wouts[w].end_col;
                for (size_t v = w0; v < w; ++v)
                    if (win_tjob[v] != 0xFFFFFFFFu && tb.jobs[win_tjob[v]].end_col == end_in_union) { win_tjob[w] = win_tjob[v]; break; }
                if (win_tjob[w] == 0xFFFFFFFFu) win_tjob[w] = tb.add(ureqs[ui], trace_off[ui - begin], plan.shapes[ui], end_in_union, wouts[w].score);
            }
            n_unions_several_jobs += tb.jobs.size() - jobs_before > 1;
            w0 = w1;
        }
        n_tjobs += tb.jobs.size();
        if ((rc = tb.run(ctx, d_text, d_peq, cigar_pool, md_pool))) return rc;
        // ---- members take the union's alignment when its path starts inside their window
        for (size_t w = 0; w < n_wins; ++w) {
            u32 const id = win_member[w];
            if (wouts[w].score == 0xFFFFFFFFu) continue;                       // no alignment within k in this window
            TraceResult res = tb.result(win_tjob[w], wouts[w].score);
            u64 const shift = uniq[id].ref_off - ureqs[win_union[w]].ref_off;
            static int const force_own = getenv("FLX_UNION_ALIGN_OWN") ? 1 : 0;        // test hook: as if every path left its window
            if (res.begin < shift || force_own) { fallback_of.push_back(id); fallback.push_back(uniq[id]); continue; }
            res.begin = (u32)(res.begin - shift);
            ures[id] = res;
        }
    }
    if (!fallback.empty()) {
        hvec<TraceResult> fres;
        if ((rc = run_trace_jobs_unique(ctx, d_text, d_peq, fallback, fres, cigar_pool, md_pool, tails, d_la_query, realign, d_ra_query, cs))) return rc;
        for (size_t i = 0; i < fallback.size(); ++i) ures[fallback_of[i]] = fres[i];
    }
    if (getenv("FLX_ALIGN_DEBUG")) fprintf(stderr, "[root unions] requests %zu distinct %zu unions %zu aligned on their own %zu traceback jobs %zu unions with several jobs %zu\n", n_requests, uniq.size(), unions.size(), fallback.size(), n_tjobs, n_unions_several_jobs);
    return FLX_OK;
}

}  // namespace

int run_trace_jobs_union(Lane* ctx, const u8* d_text, const u64* d_peq, hvec<AlignRequest> const& reqs,
                         hvec<TraceResult>& results, hvec<u32>& cigar_pool, hvec<u8>* md_pool, const TailParams* tails, const u8* d_la_query,
                         const RealignScores* realign, const u8* d_ra_query, const CsWant* cs) {
    return run_deduplicated(reqs, results, [&](hvec<AlignRequest> const& uniq, hvec<TraceResult>& ures) {
        return run_trace_jobs_union_unique(ctx, d_text, d_peq, uniq, reqs.size(), ures, cigar_pool, md_pool, tails, d_la_query, realign, d_ra_query, cs);
    });
}

// One ed_extend launch over all jobs; the wavefront cells and the symbols walked are known once the results are back.
int run_extend_jobs(Lane* lane, const u8* d_text, const u8* d_query, hvec<DevExtendJob>& jobs, hvec<DevExtendOut>& outs) {
    outs.assign(jobs.size(), DevExtendOut{});
    if (jobs.empty()) return FLX_OK;
    u32 lds_d = 0;
    for (size_t i = 0; i < jobs.size(); ++i) {
        jobs[i].out_index = (u32)i;
        if (jobs[i].d_max > EXTEND_MAX_ERRORS || jobs[i].row_limit > EXTEND_MAX_ROWS) { set_error("ed_extend: a job is larger than the kernel holds"); return FLX_ERR_INTERNAL; }
        lds_d = std::max(lds_d, std::min(jobs[i].d_max, jobs[i].row_limit));
    }
    int rc;
    if ((rc = h2d(lane, lane->ext_jobs, jobs.data(), jobs.size() * sizeof(DevExtendJob)))) return rc;
    if ((rc = lane->ext_out.ensure(jobs.size() * sizeof(DevExtendOut)))) return rc;
    rc = timed_launch(lane, "ed_extend", jobs.size() * (sizeof(DevExtendJob) + sizeof(DevExtendOut)), 0, [&] {
        return DeviceApi::extend(lane->stream, d_text, d_query, lane->ext_jobs.as<DevExtendJob>(), (u32)jobs.size(), lds_d, lane->ext_out.as<DevExtendOut>());
    });
    if (rc) return rc;
    if ((rc = d2h(lane, outs.data(), lane->ext_out.ptr, outs.size() * sizeof(DevExtendOut)))) return rc;
    if ((rc = lane->sync())) return rc;
    u64 cells = 0, symbols = 0;
    for (auto const& o : outs) { cells += ((u64)o.last_d + 1) * ((u64)o.last_d + 1); symbols += (u64)o.rows + o.cols; }
    lane->ctx->account_more("ed_extend", symbols, cells);
    return FLX_OK;
}

// One cigar_tails launch over CIGAR words and DevTraceOuts made on the host: the kernel alone (the pipeline queues it behind K5).
int run_tail_jobs(Lane* lane, const u32* words, u64 n_words, hvec<DevTraceOut> const& touts, hvec<DevTailJob> const& jobs, hvec<DevTailOut>& outs) {
    outs.assign(jobs.size(), DevTailOut{});
    if (jobs.empty()) return FLX_OK;
    int rc;
    if ((rc = h2d(lane, lane->cigar, words, n_words * 4))) return rc;
    if ((rc = h2d(lane, lane->tjob_out, touts.data(), touts.size() * sizeof(DevTraceOut)))) return rc;
    if ((rc = h2d(lane, lane->tail_jobs, jobs.data(), jobs.size() * sizeof(DevTailJob)))) return rc;
    if ((rc = lane->tail_out.ensure(jobs.size() * sizeof(DevTailOut)))) return rc;
    u64 bytes = jobs.size() * (sizeof(DevTailJob) + sizeof(DevTraceOut) + sizeof(DevTailOut));
    for (auto const& t : touts) bytes += 4ull * t.cigar_len;
    rc = timed_launch(lane, "cigar_tails", bytes, jobs.size(), [&] {
        return DeviceApi::cigar_tails(lane->stream, lane->cigar.as<u32>(), lane->tjob_out.as<DevTraceOut>(), lane->tail_jobs.as<DevTailJob>(), (u32)jobs.size(),
                                      lane->tail_out.as<DevTailOut>());
    });
    if (rc) return rc;
    if ((rc = d2h(lane, outs.data(), lane->tail_out.ptr, outs.size() * sizeof(DevTailOut)))) return rc;
    return lane->sync();
}

// One cigar_left_align launch over CIGAR words and DevTraceOuts made on the host: the kernel alone (the pipeline queues it behind K5).
int run_left_align_jobs(Lane* lane, const u8* d_text, const u8* d_query, const u32* words, u64 n_words, hvec<DevTraceOut>& touts,
                        hvec<DevLeftAlignJob> const& jobs, u64 words_out, hvec<u32>& out_words) {
    out_words.assign(words_out, 0u);
    if (jobs.empty()) return FLX_OK;
    int rc;
    if ((rc = h2d(lane, lane->cigar, words, n_words * 4))) return rc;
    if ((rc = h2d(lane, lane->tjob_out, touts.data(), touts.size() * sizeof(DevTraceOut)))) return rc;
    if ((rc = h2d(lane, lane->la_jobs, jobs.data(), jobs.size() * sizeof(DevLeftAlignJob)))) return rc;
    if ((rc = lane->cigar_la.ensure(words_out * 4 + 16))) return rc;
    if ((rc = lane->la_stat.ensure(jobs.size() * sizeof(DevLeftAlignStat)))) return rc;
    rc = timed_launch(lane, "cigar_left_align", jobs.size() * (sizeof(DevLeftAlignJob) + 2 * sizeof(DevTraceOut) + sizeof(DevLeftAlignStat)), 0, [&] {
        return DeviceApi::cigar_left_align(lane->stream, d_text, d_query, lane->cigar.as<u32>(), lane->tjob_out.as<DevTraceOut>(), lane->la_jobs.as<DevLeftAlignJob>(),
                                           (u32)jobs.size(), lane->cigar_la.as<u32>(), lane->la_stat.as<DevLeftAlignStat>());
    });
    if (rc) return rc;
    hvec<DevLeftAlignStat> stats(jobs.size());
    if ((rc = d2h(lane, touts.data(), lane->tjob_out.ptr, touts.size() * sizeof(DevTraceOut)))) return rc;
    if ((rc = d2h(lane, out_words.data(), lane->cigar_la.ptr, words_out * 4))) return rc;
    if ((rc = d2h(lane, stats.data(), lane->la_stat.ptr, stats.size() * sizeof(DevLeftAlignStat)))) return rc;
    if ((rc = lane->sync())) return rc;
    u64 bytes = 0, moved = 0;
    for (size_t j = 0; j < jobs.size(); ++j) {
        if (touts[j].cigar_len == 0xFFFFFFFFu) { set_error("cigar_left_align: CIGAR slab overflow, or a path that leaves its window or its query"); return FLX_ERR_INTERNAL; }
        bytes += 4ull * stats[j].words_in + 4ull * touts[j].cigar_len + 2ull * stats[j].letters;
        moved += stats[j].moved;
    }
    lane->ctx->account_more("cigar_left_align", bytes, moved);
    return FLX_OK;
}

// One cs_build launch over CIGAR words and DevTraceOuts made on the host: the kernel alone (the pipeline queues it behind md_build).
int run_cs_jobs(Lane* lane, const u8* d_text, const u8* d_query, const u32* words, u64 n_words, hvec<DevTraceOut> const& touts, hvec<DevCsJob> const& jobs,
                u32 form, u64 slab_bytes, hvec<u8>& slabs, hvec<u32>& lens) {
    slabs.assign(slab_bytes, (u8)0);
    lens.assign(jobs.size(), 0u);
    if (jobs.empty()) return FLX_OK;
    int rc;
    if ((rc = h2d(lane, lane->cigar, words, n_words * 4))) return rc;
    if ((rc = h2d(lane, lane->tjob_out, touts.data(), touts.size() * sizeof(DevTraceOut)))) return rc;
    if ((rc = h2d(lane, lane->cs_jobs, jobs.data(), jobs.size() * sizeof(DevCsJob)))) return rc;
    if ((rc = lane->cs.ensure(slab_bytes + 16))) return rc;
    if ((rc = lane->cs_out.ensure(jobs.size() * sizeof(DevCsOut)))) return rc;
    rc = timed_launch(lane, "cs_build", 0, 0, [&] {
        return DeviceApi::cs_build(lane->stream, d_text, d_query, lane->cigar.as<u32>(), lane->tjob_out.as<DevTraceOut>(), lane->cs_jobs.as<DevCsJob>(),
                                   (u32)jobs.size(), form, lane->cs.as<u8>(), lane->cs_out.as<DevCsOut>());
    });
    if (rc) return rc;
    hvec<DevCsOut> outs(jobs.size());
    if ((rc = d2h(lane, outs.data(), lane->cs_out.ptr, outs.size() * sizeof(DevCsOut)))) return rc;
    if (slab_bytes && (rc = d2h(lane, slabs.data(), lane->cs.ptr, slab_bytes))) return rc;
    if ((rc = lane->sync())) return rc;
    u64 bytes = 0, written = 0;
    for (size_t j = 0; j < jobs.size(); ++j) {
        if (outs[j].len == 0xFFFFFFFFu) { set_error("cs_build: cs slab overflow, or a path that leaves its window or its query"); return FLX_ERR_INTERNAL; }
        lens[j] = outs[j].len;
        bytes += 4ull * touts[j].cigar_len + 2ull * outs[j].len;
        written += outs[j].len;
    }
    lane->ctx->account_more("cs_build", bytes, written);
    return FLX_OK;
}

// cigar_realign over CIGAR words and DevTraceOuts made on the host: the kernel alone. jobs[i].trace_cap holds the words of trace job i
// needs (0: it does not fit the lane's arena and keeps its path); the jobs are cut into launches of at most REALIGN_LAUNCH_JOBS jobs
// whose traces fit the arena together, and trace_off is set here.
int run_realign_jobs(Lane* lane, const u8* d_text, const u8* d_query, const u32* words, u64 n_words, hvec<DevTraceOut>& touts, hvec<DevRealignJob>& jobs,
                     RealignScores const& scores, u64 words_out, hvec<u32>& out_words, hvec<DevRealignStat>& stats) {
    out_words.assign(words_out, 0u);
    stats.assign(jobs.size(), DevRealignStat{0, 0u, 0, 0, 0u, 0u, 0ull});
    if (jobs.empty()) return FLX_OK;
    int rc;
    u64 const arena_words = std::max<u64>(lane->trace_budget_bytes / 4, 1);
    hvec<size_t> cuts{0};
    u64 used = 0, largest = 0;
    for (size_t j = 0; j < jobs.size(); ++j) {
        if (jobs[j].trace_cap > arena_words) jobs[j].trace_cap = 0;
        if (j - cuts.back() == REALIGN_LAUNCH_JOBS || used + jobs[j].trace_cap > arena_words) { cuts.push_back(j); used = 0; }
        jobs[j].trace_off = used;
        used += jobs[j].trace_cap;
        largest = std::max(largest, used);
    }
    cuts.push_back(jobs.size());
    if ((rc = h2d(lane, lane->cigar, words, n_words * 4))) return rc;
    if ((rc = h2d(lane, lane->tjob_out, touts.data(), touts.size() * sizeof(DevTraceOut)))) return rc;
    if ((rc = h2d(lane, lane->ra_jobs, jobs.data(), jobs.size() * sizeof(DevRealignJob)))) return rc;
    if ((rc = lane->cigar_ra.ensure(words_out * 4 + 16))) return rc;
    if ((rc = lane->ra_stat.ensure(jobs.size() * sizeof(DevRealignStat)))) return rc;
    // (the arena is taken as the traceback stage takes it on first use: no reallocation when that stage runs later)
    if ((rc = lane->trace.ensure(std::max<size_t>(largest * 4 + 64, lane->trace.ptr ? 0 : lane->trace_budget_bytes / 3 * 2)))) return rc;
    for (size_t k = 0; k + 1 < cuts.size(); ++k) {
        size_t const first = cuts[k], count = cuts[k + 1] - first;
        // (the cells it computes are known once its results are back: they are added below)
        rc = timed_launch(lane, "cigar_realign", count * (sizeof(DevRealignJob) + 2 * sizeof(DevTraceOut) + sizeof(DevRealignStat)), 0, [&] {
            return DeviceApi::cigar_realign(lane->stream, d_text, d_query, lane->cigar.as<u32>(), lane->tjob_out.as<DevTraceOut>(),
                                            lane->ra_jobs.as<DevRealignJob>() + first, (u32)count, scores, lane->trace.as<u32>(), lane->cigar_ra.as<u32>(),
                                            lane->ra_stat.as<DevRealignStat>());
        });
        if (rc) return rc;
    }
    if ((rc = d2h(lane, touts.data(), lane->tjob_out.ptr, touts.size() * sizeof(DevTraceOut)))) return rc;
    if ((rc = d2h(lane, out_words.data(), lane->cigar_ra.ptr, words_out * 4))) return rc;
    if ((rc = d2h(lane, stats.data(), lane->ra_stat.ptr, stats.size() * sizeof(DevRealignStat)))) return rc;
    if ((rc = lane->sync())) return rc;
    // the trace is written once and read once along the path; work units: DP cells
    u64 bytes = 0, cells = 0, changed = 0, kept = 0;
    for (size_t j = 0; j < jobs.size(); ++j) {
        if (touts[j].cigar_len == 0xFFFFFFFFu) { set_error("cigar_realign: CIGAR slab overflow, or a path that leaves its window or its query"); return FLX_ERR_INTERNAL; }
        bytes += stats[j].cells / 2 + 4ull * touts[j].cigar_len;
        cells += stats[j].cells; changed += stats[j].changed; kept += stats[j].kept;
    }
    lane->ctx->account_more("cigar_realign", bytes, cells);
    {
        std::lock_guard<std::mutex> g(lane->ctx->mu);
        lane->ctx->realign.paths_realigned += jobs.size() - kept;
        lane->ctx->realign.paths_changed += changed;
        lane->ctx->realign.paths_kept += kept;
    }
    return FLX_OK;
}

int build_peq(Lane* ctx, const u8* d_seq, u64 len, DeviceBuffer& peq) {
    u64 const n_words = len / 64 + 2;
    int rc = peq.ensure(n_words * 6 * 8 + 64);
    if (rc) return rc;
    return timed_launch(ctx, "peq_build", len + n_words * 48, n_words, [&] { return DeviceApi::build_peq(ctx->stream, d_seq, len, peq.as<u64>()); });
}

int ensure_reversed_text(Lane* lane) {
    flx_ctx* ctx = lane->ctx;
    std::lock_guard<std::mutex> g(ctx->mu);
    if (ctx->text_rev_ready) return FLX_OK;
    HostIndex const& H = *ctx->hidx;
    hvec<u8> rev(H.n);
    if (H.text.size() == H.n) std::reverse_copy(H.text.begin(), H.text.end(), rev.begin());
    else {                                       // a context on a received image: the text is in HBM only
        FLX_HIP(hipMemcpy(rev.data(), ctx->didx.text, H.n, hipMemcpyDeviceToHost));
        std::reverse(rev.begin(), rev.end());
    }
    const u8* first = nullptr;
    int rc = upload_padded(lane, ctx->text_rev, rev.data(), rev.size(), &first);
    if (rc) return rc;
    FLX_HIP(hipStreamSynchronize(lane->stream));
    ctx->text_rev_ready = true;
    return FLX_OK;
}

}  // namespace flx

using namespace flx;

// ================================================================================================ C ABI: seam 2
// The jobs of one flx_align_batch call as the three request lists it runs, by mode (ids: the job of every request). WITHOUT_CIGAR jobs
// run on the reversed pools: their offsets are mirrored in text_len / query_pool_len.
struct BatchRequests { hvec<AlignRequest> reqs[3]; hvec<u32> ids[3]; };
static void split_batch_jobs(const flx_align_job* jobs, uint64_t n_jobs, u64 text_len, u64 query_pool_len, BatchRequests& B) {
    for (uint64_t i = 0; i < n_jobs; ++i) {
        flx_align_job const& j = jobs[i];
        if (j.mode == FLX_MODE_WITHOUT_CIGAR) B.reqs[j.mode].push_back({text_len - j.ref_offset - j.ref_length, query_pool_len - j.query_offset - j.query_length, j.ref_length, j.query_length, j.num_allowed_errors});
        else B.reqs[j.mode].push_back({j.ref_offset, j.query_offset, j.ref_length, j.query_length, j.num_allowed_errors});
        B.ids[j.mode].push_back((u32)i);
    }
}

// The launch shape flx_align_batch gives every job: the same three lists, their distinct requests (run_deduplicated) and choose_shapes on
// each. queue: the hand-over slots the job's own ring occupies in that shape (0: it never waits; more than RING_QUEUE_MAX would mean a
// shape that does not hold the job). Host arithmetic only: no context, no device.
extern "C" int flx_align_shapes(const flx_align_job* jobs, uint64_t n_jobs, flx_align_shape* out) {
    if (n_jobs && (!jobs || !out)) { set_error("flx_align_shapes: null argument"); return FLX_ERR_INVALID; }
    if (n_jobs >= (1ull << 31)) { set_error("too many jobs in one call"); return FLX_ERR_INVALID; }
    u64 text_len = 0, query_pool_len = 0;                 // (any pool that holds every job mirrors the offsets one to one)
    for (uint64_t i = 0; i < n_jobs; ++i) {
        flx_align_job const& j = jobs[i];
        if (j.query_length == 0 || j.mode > 2) { set_error("flx_align_shapes: job without query rows, or of an unknown mode"); return FLX_ERR_INVALID; }
        if (j.query_length > align_supported_max_query()) { set_error("query longer than the supported maximum"); return FLX_ERR_UNSUPPORTED; }
        text_len = std::max<u64>(text_len, j.ref_offset + j.ref_length);
        query_pool_len = std::max<u64>(query_pool_len, j.query_offset + j.query_length);
    }
    BatchRequests B;
    split_batch_jobs(jobs, n_jobs, text_len, query_pool_len, B);
    for (int mode = 0; mode < 3; ++mode) {
        hvec<AlignRequest> uniq;
        hvec<u32> uniq_of;
        hvec<AlignShape> shapes;
        dedup_requests(B.reqs[mode], uniq, uniq_of);
        if (int const rc = choose_shapes(uniq, shapes)) return rc;
        for (size_t i = 0; i < B.reqs[mode].size(); ++i) {
            AlignRequest const& r = B.reqs[mode][i];
            AlignShape const sh = shapes[uniq_of[i]];
            out[B.ids[mode][i]] = flx_align_shape{sh.words_per_lane, sh.lanes_per_job, ring_queue_for(ring_delay(r.n, r.m, r.k, sh.words_per_lane, sh.lanes_per_job))};
        }
    }
    return FLX_OK;
}

extern "C" int flx_align_batch(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool,
                               uint64_t query_pool_len, const flx_align_job* jobs, uint64_t n_jobs, flx_align_result* out,
                               uint32_t* cigar_pool, uint64_t* cigar_pool_words) {
    return flx_align_batch_gaps(ctx, ref_pool, ref_pool_len, query_pool, query_pool_len, jobs, n_jobs, out, cigar_pool, cigar_pool_words, nullptr, nullptr, nullptr, nullptr);
}
extern "C" int flx_align_batch_md(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool,
                                  uint64_t query_pool_len, const flx_align_job* jobs, uint64_t n_jobs, flx_align_result* out,
                                  uint32_t* cigar_pool, uint64_t* cigar_pool_words, flx_md_ref* out_md, uint8_t* md_pool, uint64_t* md_pool_bytes) {
    return flx_align_batch_gaps(ctx, ref_pool, ref_pool_len, query_pool, query_pool_len, jobs, n_jobs, out, cigar_pool, cigar_pool_words, out_md, md_pool, md_pool_bytes, nullptr);
}
extern "C" int flx_align_batch_gaps(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool,
                                    uint64_t query_pool_len, const flx_align_job* jobs, uint64_t n_jobs, flx_align_result* out,
                                    uint32_t* cigar_pool, uint64_t* cigar_pool_words, flx_md_ref* out_md, uint8_t* md_pool, uint64_t* md_pool_bytes,
                                    const flx_gap_options* gaps) {
    return flx_align_batch_realign(ctx, ref_pool, ref_pool_len, query_pool, query_pool_len, jobs, n_jobs, out, cigar_pool, cigar_pool_words, out_md, md_pool,
                                   md_pool_bytes, gaps, nullptr, nullptr);
}
// out_md == NULL: no MD strings (flx_align_batch); gaps NULL or zeroed: the gaps stay where K5 put them (flx_align_batch_md); realign
// NULL or zeroed: the paths stay edit-distance paths (flx_align_batch_gaps)
extern "C" int flx_align_batch_realign(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool,
                                       uint64_t query_pool_len, const flx_align_job* jobs, uint64_t n_jobs, flx_align_result* out,
                                       uint32_t* cigar_pool, uint64_t* cigar_pool_words, flx_md_ref* out_md, uint8_t* md_pool, uint64_t* md_pool_bytes,
                                       const flx_gap_options* gaps, const flx_realign_options* realign, int32_t* out_scores) {
    return flx_align_batch_cs(ctx, ref_pool, ref_pool_len, query_pool, query_pool_len, jobs, n_jobs, out, cigar_pool, cigar_pool_words, out_md, md_pool, md_pool_bytes,
                              gaps, realign, out_scores, nullptr, nullptr, nullptr, nullptr);
}
// cs NULL or zeroed: no cs strings (flx_align_batch_realign)
extern "C" int flx_align_batch_cs(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool,
                                  uint64_t query_pool_len, const flx_align_job* jobs, uint64_t n_jobs, flx_align_result* out,
                                  uint32_t* cigar_pool, uint64_t* cigar_pool_words, flx_md_ref* out_md, uint8_t* md_pool, uint64_t* md_pool_bytes,
                                  const flx_gap_options* gaps, const flx_realign_options* realign, int32_t* out_scores, const flx_cs_options* cs,
                                  flx_md_ref* out_cs, uint8_t* cs_pool, uint64_t* cs_pool_bytes) {
    if (!cs_options_valid(cs)) return FLX_ERR_INVALID;                                 // (before the context is looked at)
    uint32_t const cs_form = cs_options_form(cs);
    std::string const fn = cs_form ? "flx_align_batch_cs" : realign_options_active(realign) ? "flx_align_batch_realign" : gap_options_active(gaps) ? "flx_align_batch_gaps" : out_md ? "flx_align_batch_md" : "flx_align_batch";        // (all forward here)
    if (!gap_options_valid(gaps) || !realign_options_valid(realign)) return FLX_ERR_INVALID;
    RealignScores const ra_scores = realign_scores(realign);
    if (cs_form && (!out_cs || !cs_pool_bytes)) { set_error(fn + ": null argument"); return FLX_ERR_INVALID; }
    uint64_t const cs_pool_cap = cs_pool_bytes ? *cs_pool_bytes : 0;
    if (cs_pool_bytes) *cs_pool_bytes = 0;                                            // (out: bytes used, also on an early return)
    if (out_md && !md_pool_bytes) { set_error(fn + ": null argument"); return FLX_ERR_INVALID; }
    uint64_t const md_pool_cap = md_pool_bytes ? *md_pool_bytes : 0;
    if (md_pool_bytes) *md_pool_bytes = 0;                                            // (out: bytes used, also on an early return)
    if (!ctx || (n_jobs && (!jobs || !out || !query_pool))) { set_error(fn + ": null argument"); return FLX_ERR_INVALID; }
    FLX_HIP(hipSetDevice(ctx->device));
    if (n_jobs >= (1ull << 31)) { set_error("too many jobs in one call"); return FLX_ERR_INVALID; }
    u64 const text_len = ref_pool ? ref_pool_len : ctx->hidx->n;
    bool any_rev = false, any_trace = false;
    for (uint64_t i = 0; i < n_jobs; ++i) {
        flx_align_job const& j = jobs[i];
        if (j.query_length == 0 || j.query_offset + j.query_length > query_pool_len || j.ref_offset + j.ref_length > text_len || j.mode > 2) {
            set_error(fn + ": job outside its pools"); return FLX_ERR_INVALID;
        }
        if (j.query_length > align_supported_max_query()) { set_error("query longer than the supported maximum"); return FLX_ERR_UNSUPPORTED; }
        any_rev |= j.mode == FLX_MODE_WITHOUT_CIGAR;
        any_trace |= j.mode == FLX_MODE_WITH_CIGAR;
    }
    int rc;
    LaneLease lease(ctx, ctx->external_stream ? 0 : -1);
    Lane* L = lease.lane;
    const u8* d_text = ctx->didx.text;
    const u8* d_text_rev = nullptr;
    hvec<u8> tmp;
    if (ref_pool) {
        if ((rc = upload_padded(L, L->user_text, ref_pool, ref_pool_len, &d_text))) return rc;
        if (any_rev) {
            tmp.assign(ref_pool, ref_pool + ref_pool_len);
            std::reverse(tmp.begin(), tmp.end());
            if ((rc = upload_padded(L, L->user_text_rev, tmp.data(), tmp.size(), &d_text_rev))) return rc;
            if ((rc = L->sync())) return rc;
        }
    } else if (any_rev) {
        if ((rc = ensure_reversed_text(L))) return rc;
        d_text_rev = ctx->text_rev.as<u8>() + TEXT_PAD;
    }
    if ((rc = h2d(L, L->seq, query_pool, query_pool_len, 192))) return rc;
    if ((rc = build_peq(L, L->seq.as<u8>(), query_pool_len, L->peq))) return rc;
    hvec<u8> qrev;
    if (any_rev) {
        qrev.assign(query_pool, query_pool + query_pool_len);
        std::reverse(qrev.begin(), qrev.end());
        if ((rc = h2d(L, L->seq_rev, qrev.data(), qrev.size(), 64))) return rc;
        if ((rc = build_peq(L, L->seq_rev.as<u8>(), query_pool_len, L->peq_rev))) return rc;
    }
    BatchRequests B;
    split_batch_jobs(jobs, n_jobs, text_len, query_pool_len, B);
    hvec<AlignRequest> const &score_reqs = B.reqs[FLX_MODE_EXISTS], &rev_reqs = B.reqs[FLX_MODE_WITHOUT_CIGAR], &trace_reqs = B.reqs[FLX_MODE_WITH_CIGAR];
    hvec<u32> const &score_ids = B.ids[FLX_MODE_EXISTS], &rev_ids = B.ids[FLX_MODE_WITHOUT_CIGAR], &trace_ids = B.ids[FLX_MODE_WITH_CIGAR];
    for (uint64_t i = 0; i < n_jobs; ++i) out[i] = flx_align_result{0, 0, 0, 0, 0, 0};
    if (out_md) for (uint64_t i = 0; i < n_jobs; ++i) out_md[i] = flx_md_ref{0, 0, 0};
    if (out_scores) for (uint64_t i = 0; i < n_jobs; ++i) out_scores[i] = 0;
    if (cs_form) for (uint64_t i = 0; i < n_jobs; ++i) out_cs[i] = flx_md_ref{0, 0, 0};
    hvec<DevAlignOut> outs;
    if ((rc = run_score_jobs(L, d_text, L->peq.as<u64>(), score_reqs, outs, "ed_align_exists"))) return rc;
    for (size_t i = 0; i < outs.size(); ++i)
        if (outs[i].score != 0xFFFFFFFFu) { out[score_ids[i]].exists = 1; out[score_ids[i]].num_errors = outs[i].score; }
    if ((rc = run_score_jobs(L, d_text_rev, L->peq_rev.as<u64>(), rev_reqs, outs, "ed_align_exists"))) return rc;
    for (size_t i = 0; i < outs.size(); ++i)
        if (outs[i].score != 0xFFFFFFFFu) {
            flx_align_result& r = out[rev_ids[i]];
            r.exists = 1; r.num_errors = outs[i].score; r.begin = rev_reqs[i].n - outs[i].end_col;      // alignment.cpp:135
        }
    hvec<TraceResult> tres;
    hvec<u32> cig;
    hvec<u8> mdp, csp;
    CsWant const want_cs{cs_form, L->seq.as<u8>(), &csp};
    if ((rc = run_trace_jobs(L, d_text, L->peq.as<u64>(), trace_reqs, tres, cig, out_md ? &mdp : nullptr, nullptr, gap_options_active(gaps) ? L->seq.as<u8>() : nullptr,
                             &ra_scores, realign_options_active(realign) ? L->seq.as<u8>() : nullptr, cs_form ? &want_cs : nullptr))) return rc;
    uint64_t const cap = cigar_pool_words ? *cigar_pool_words : 0;
    if (cigar_pool_words) *cigar_pool_words = cig.size();
    if (any_trace && (!cigar_pool || cig.size() > cap)) { set_error("cigar pool too small"); return FLX_ERR_CAPACITY; }
    if (!cig.empty()) memcpy(cigar_pool, cig.data(), cig.size() * 4);
    if (out_md) {
        *md_pool_bytes = mdp.size();
        if (!mdp.empty() && (!md_pool || mdp.size() > md_pool_cap)) { set_error("md pool too small"); return FLX_ERR_CAPACITY; }
        if (!mdp.empty()) memcpy(md_pool, mdp.data(), mdp.size());
    }
    if (cs_form) {
        *cs_pool_bytes = csp.size();
        if (!csp.empty() && (!cs_pool || csp.size() > cs_pool_cap)) { set_error("cs pool too small"); return FLX_ERR_CAPACITY; }
        if (!csp.empty()) memcpy(cs_pool, csp.data(), csp.size());
    }
    for (size_t i = 0; i < tres.size(); ++i)
        if (tres[i].exists) {
            flx_align_result& r = out[trace_ids[i]];
            r.exists = 1; r.num_errors = tres[i].nm; r.begin = tres[i].begin; r.cigar_offset = tres[i].cigar_off; r.cigar_length = tres[i].cigar_len;
            if (out_md) out_md[trace_ids[i]] = flx_md_ref{tres[i].md_off, tres[i].md_len, 0};
            if (out_scores) out_scores[trace_ids[i]] = tres[i].score;
            if (cs_form) out_cs[trace_ids[i]] = flx_md_ref{tres[i].cs_off, tres[i].cs_len, 0};
        }
    return FLX_OK;
}

// ================================================================================================ C ABI: the extension kernel alone
extern "C" int flx_extend_batch(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len,
                                const flx_extend_job* jobs, uint64_t n_jobs, flx_extend_result* out) {
    if (!ctx || (n_jobs && (!jobs || !out || !query_pool))) { set_error("flx_extend_batch: null argument"); return FLX_ERR_INVALID; }
    if (n_jobs >= (1ull << 31)) { set_error("too many jobs in one call"); return FLX_ERR_INVALID; }
    u64 const text_len = ref_pool ? ref_pool_len : ctx->hidx->n;
    hvec<DevExtendJob> dj(n_jobs);
    for (uint64_t i = 0; i < n_jobs; ++i) {
        flx_extend_job const& j = jobs[i];
        flx_extend_options const as_options{0, j.error_weight, j.x_drop, j.max_errors, {}};
        if (!extend_options_valid(&as_options)) return FLX_ERR_INVALID;
        if (j.direction != 1 && j.direction != -1) { set_error("flx_extend_batch: direction must be +1 or -1"); return FLX_ERR_INVALID; }
        if (j.row_limit > EXTEND_MAX_ROWS || j.ref_limit >= (1u << 31)) { set_error("flx_extend_batch: row_limit must be below 2^19 and ref_limit below 2^31"); return FLX_ERR_INVALID; }
        bool const inside = j.direction > 0 ? (j.text_pos <= text_len && j.ref_limit <= text_len - j.text_pos && j.q_pos <= query_pool_len && j.row_limit <= query_pool_len - j.q_pos)
                                            : ((j.ref_limit == 0 || (j.text_pos < text_len && j.ref_limit <= j.text_pos + 1)) &&
                                               (j.row_limit == 0 || (j.q_pos < query_pool_len && j.row_limit <= j.q_pos + 1)));
        if (!inside) { set_error("flx_extend_batch: job outside its pools"); return FLX_ERR_INVALID; }
        dj[i] = DevExtendJob{j.text_pos, j.q_pos, j.ref_limit, j.row_limit, j.direction, extend_weight(j.error_weight), extend_x_drop(j.x_drop),
                             extend_max_errors(j.max_errors), (u32)i, 0};
        if (j.ref_limit == 0 || j.row_limit == 0) { dj[i].text_pos = 0; dj[i].q_pos = 0; dj[i].ref_limit = 0; }      // nothing is read: R(0) = 0 (row_limit 0), or only D[i][0] = i (ref_limit 0)
    }
    FLX_HIP(hipSetDevice(ctx->device));
    int rc;
    LaneLease lease(ctx, ctx->external_stream ? 0 : -1);
    Lane* L = lease.lane;
    const u8* d_text = ctx->didx.text;
    if (ref_pool && (rc = upload_padded(L, L->user_text, ref_pool, ref_pool_len, &d_text))) return rc;
    if ((rc = h2d(L, L->seq, query_pool, query_pool_len, 192))) return rc;
    hvec<DevExtendOut> outs;
    if ((rc = run_extend_jobs(L, d_text, L->seq.as<u8>(), dj, outs))) return rc;
    for (uint64_t i = 0; i < n_jobs; ++i) out[i] = flx_extend_result{outs[i].rows, outs[i].cols, outs[i].errors, outs[i].reason};
    return FLX_OK;
}

// ================================================================================================ C ABI: the tail kernel alone
extern "C" int flx_cigar_tails_batch(flx_ctx* ctx, const uint32_t* cigar_words, uint64_t n_words, const flx_tail_job* jobs, uint64_t n_jobs, flx_tail_result* out) {
    if (!ctx || (n_jobs && (!jobs || !out)) || (n_words && !cigar_words)) { set_error("flx_cigar_tails_batch: null argument"); return FLX_ERR_INVALID; }
    if (n_jobs >= (1ull << 31)) { set_error("too many jobs in one call"); return FLX_ERR_INVALID; }
    if (!tail_jobs_valid(cigar_words, n_words, jobs, n_jobs, "flx_cigar_tails_batch")) return FLX_ERR_INVALID;      // (before any launch)
    hvec<DevTraceOut> touts(n_jobs);
    hvec<DevTailJob> dj(n_jobs);
    for (uint64_t i = 0; i < n_jobs; ++i) {
        flx_tail_job const& j = jobs[i];
        touts[i] = DevTraceOut{0, 0, j.cigar_length, 0};
        dj[i] = DevTailJob{j.cigar_offset, (u32)i, split_weight(j.error_weight), split_x_drop(j.x_drop), split_min_tail_rows(j.min_tail_rows)};
    }
    FLX_HIP(hipSetDevice(ctx->device));
    LaneLease lease(ctx, ctx->external_stream ? 0 : -1);
    hvec<DevTailOut> outs;
    if (int const rc = run_tail_jobs(lease.lane, cigar_words, n_words, touts, dj, outs)) return rc;
    for (uint64_t i = 0; i < n_jobs; ++i) memcpy(&out[i], &outs[i], sizeof(flx_tail_result));
    return FLX_OK;
}

// ================================================================================================ C ABI: the left-align kernel alone
extern "C" int flx_left_align_batch(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len,
                                    const uint32_t* cigar_words, uint64_t n_words, const flx_left_align_job* jobs, uint64_t n_jobs, uint32_t* out_words,
                                    uint64_t* out_n_words, flx_cigar_ref* out) {
    if (!ctx || !out_n_words || (n_jobs && (!jobs || !out)) || (n_words && !cigar_words) || (query_pool_len && !query_pool)) {
        set_error("flx_left_align_batch: null argument"); return FLX_ERR_INVALID;
    }
    uint64_t const out_cap = *out_n_words;
    *out_n_words = 0;
    if (n_jobs >= (1ull << 31)) { set_error("too many jobs in one call"); return FLX_ERR_INVALID; }
    u64 const text_len = ref_pool ? ref_pool_len : ctx->hidx->n;
    if (!left_align_jobs_valid(text_len, query_pool_len, cigar_words, n_words, jobs, n_jobs, "flx_left_align_batch")) return FLX_ERR_INVALID;      // (before any launch)
    hvec<DevTraceOut> touts(n_jobs);
    hvec<DevLeftAlignJob> dj(n_jobs);
    u64 slab_words = 0;
    for (uint64_t i = 0; i < n_jobs; ++i) {
        flx_left_align_job const& j = jobs[i];
        u64 const cap = left_align_cap(cigar_words + j.cigar_offset, j.cigar_length);
        touts[i] = DevTraceOut{j.begin, 0, j.cigar_length, 0};
        dj[i] = DevLeftAlignJob{j.ref_offset, j.query_offset, j.cigar_offset, slab_words, j.ref_length, j.query_length, (u32)cap, (u32)i};
        slab_words += cap;
    }
    FLX_HIP(hipSetDevice(ctx->device));
    int rc;
    LaneLease lease(ctx, ctx->external_stream ? 0 : -1);
    Lane* L = lease.lane;
    hvec<u32> slabs;
    if (n_jobs) {
        const u8* d_text = ctx->didx.text;
        if (ref_pool && (rc = upload_padded(L, L->user_text, ref_pool, ref_pool_len, &d_text))) return rc;
        if ((rc = h2d(L, L->seq, query_pool, query_pool_len, 192))) return rc;
        if ((rc = run_left_align_jobs(L, d_text, L->seq.as<u8>(), cigar_words, n_words, touts, dj, slab_words, slabs))) return rc;
    }
    u64 used = 0;
    for (uint64_t i = 0; i < n_jobs; ++i) used += touts[i].cigar_len;
    *out_n_words = used;
    if (used > out_cap || (used && !out_words)) { set_error("flx_left_align_batch: the output word pool is too small"); return FLX_ERR_CAPACITY; }
    used = 0;
    for (uint64_t i = 0; i < n_jobs; ++i) {                   // the slabs packed in job order
        if (touts[i].cigar_len) memcpy(out_words + used, slabs.data() + dj[i].out_off + touts[i].cigar_start, 4ull * touts[i].cigar_len);
        out[i] = flx_cigar_ref{used, touts[i].cigar_len, 0};
        used += touts[i].cigar_len;
    }
    return FLX_OK;
}

// ================================================================================================ C ABI: the realign kernel alone
extern "C" int flx_realign_batch(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len,
                                 const uint32_t* cigar_words, uint64_t n_words, const flx_realign_job* jobs, uint64_t n_jobs,
                                 const flx_realign_options* options, uint32_t* out_words, uint64_t* out_n_words, flx_realign_result* out) {
    if (!realign_options_valid(options)) return FLX_ERR_INVALID;
    if (!ctx || !out_n_words || (n_jobs && (!jobs || !out)) || (n_words && !cigar_words) || (query_pool_len && !query_pool)) {
        set_error("flx_realign_batch: null argument"); return FLX_ERR_INVALID;
    }
    uint64_t const out_cap = *out_n_words;
    *out_n_words = 0;
    if (n_jobs >= (1ull << 31)) { set_error("too many jobs in one call"); return FLX_ERR_INVALID; }
    u64 const text_len = ref_pool ? ref_pool_len : ctx->hidx->n;
    if (!left_align_jobs_valid(text_len, query_pool_len, cigar_words, n_words, jobs, n_jobs, "flx_realign_batch")) return FLX_ERR_INVALID;      // (before any launch)
    RealignScores const scores = realign_scores(options);
    hvec<DevTraceOut> touts(n_jobs);
    hvec<DevRealignJob> dj(n_jobs);
    u64 slab_words = 0;
    for (uint64_t i = 0; i < n_jobs; ++i) {
        flx_realign_job const& j = jobs[i];
        RealignShape const p = realign_shape(cigar_words + j.cigar_offset, j.cigar_length, scores);
        u64 const cap = realign_cap(p.nm, j.cigar_length, scores);
        u64 const need = realign_trace_words(p.m, (u64)((int64_t)p.d_max - p.d_min + 2 * (int64_t)scores.w + 1));
        if (cap >= (1ull << 32)) { set_error("flx_realign_batch: a job's result could exceed 2^32 words"); return FLX_ERR_INVALID; }
        touts[i] = DevTraceOut{j.begin, 0, j.cigar_length, 0};
        // (a need beyond 32 bits is beyond every arena: 0 words, the path is kept)
        dj[i] = DevRealignJob{j.ref_offset, j.query_offset, j.cigar_offset, slab_words, 0, j.ref_length, j.query_length, (u32)cap, (u32)i,
                              need > 0xFFFFFFFFull ? 0u : (u32)need, 0};
        slab_words += cap;
    }
    FLX_HIP(hipSetDevice(ctx->device));
    int rc;
    LaneLease lease(ctx, ctx->external_stream ? 0 : -1);
    Lane* L = lease.lane;
    hvec<u32> slabs;
    hvec<DevRealignStat> stats;
    if (n_jobs) {
        const u8* d_text = ctx->didx.text;
        if (ref_pool && (rc = upload_padded(L, L->user_text, ref_pool, ref_pool_len, &d_text))) return rc;
        if ((rc = h2d(L, L->seq, query_pool, query_pool_len, 192))) return rc;
        if ((rc = run_realign_jobs(L, d_text, L->seq.as<u8>(), cigar_words, n_words, touts, dj, scores, slab_words, slabs, stats))) return rc;
    }
    u64 used = 0;
    for (uint64_t i = 0; i < n_jobs; ++i) used += touts[i].cigar_len;
    *out_n_words = used;
    if (used > out_cap || (used && !out_words)) { set_error("flx_realign_batch: the output word pool is too small"); return FLX_ERR_CAPACITY; }
    used = 0;
    for (uint64_t i = 0; i < n_jobs; ++i) {                   // the slabs packed in job order
        if (touts[i].cigar_len) memcpy(out_words + used, slabs.data() + dj[i].out_off + touts[i].cigar_start, 4ull * touts[i].cigar_len);
        out[i] = flx_realign_result{used, touts[i].cigar_len, stats[i].num_errors, stats[i].score, stats[i].diag_lo, stats[i].diag_hi, stats[i].kept};
        used += touts[i].cigar_len;
    }
    return FLX_OK;
}

// ================================================================================================ C ABI: the cs kernel alone
extern "C" int flx_cs_batch(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len,
                            const uint32_t* cigar_words, uint64_t n_words, const flx_cs_job* jobs, uint64_t n_jobs, const flx_cs_options* options,
                            uint8_t* out_bytes, uint64_t* out_n_bytes, flx_md_ref* out) {
    if (!cs_options_valid(options)) return FLX_ERR_INVALID;
    if (cs_options_form(options) == 0) { set_error("flx_cs_batch: form must be 1 (short) or 2 (long)"); return FLX_ERR_INVALID; }
    if (!ctx || !out_n_bytes || (n_jobs && (!jobs || !out)) || (n_words && !cigar_words) || (query_pool_len && !query_pool)) {
        set_error("flx_cs_batch: null argument"); return FLX_ERR_INVALID;
    }
    uint64_t const out_cap = *out_n_bytes;
    *out_n_bytes = 0;
    if (n_jobs >= (1ull << 31)) { set_error("too many jobs in one call"); return FLX_ERR_INVALID; }
    u64 const text_len = ref_pool ? ref_pool_len : ctx->hidx->n;
    if (!left_align_jobs_valid(text_len, query_pool_len, cigar_words, n_words, jobs, n_jobs, "flx_cs_batch")) return FLX_ERR_INVALID;      // (before any launch)
    u32 const form = cs_options_form(options);
    hvec<DevTraceOut> touts(n_jobs);
    hvec<DevCsJob> dj(n_jobs);
    u64 slab_bytes = 0;
    for (uint64_t i = 0; i < n_jobs; ++i) {
        flx_cs_job const& j = jobs[i];
        u64 const need = cs_path_bytes(cigar_words + j.cigar_offset, j.cigar_length, form);      // (below 2^30: rows and columns are below 2^28)
        touts[i] = DevTraceOut{j.begin, 0, j.cigar_length, 0};
        dj[i] = DevCsJob{j.ref_offset, j.query_offset, j.cigar_offset, slab_bytes, j.ref_length, j.query_length, (u32)need, (u32)i};
        slab_bytes += need;
    }
    FLX_HIP(hipSetDevice(ctx->device));
    int rc;
    LaneLease lease(ctx, ctx->external_stream ? 0 : -1);
    Lane* L = lease.lane;
    hvec<u8> slabs;
    hvec<u32> lens;
    if (n_jobs) {
        const u8* d_text = ctx->didx.text;
        if (ref_pool && (rc = upload_padded(L, L->user_text, ref_pool, ref_pool_len, &d_text))) return rc;
        if ((rc = h2d(L, L->seq, query_pool, query_pool_len, 192))) return rc;
        if ((rc = run_cs_jobs(L, d_text, L->seq.as<u8>(), cigar_words, n_words, touts, dj, form, slab_bytes, slabs, lens))) return rc;
    }
    u64 used = 0;
    for (uint64_t i = 0; i < n_jobs; ++i) used += lens[i];
    *out_n_bytes = used;
    if (used > out_cap || (used && !out_bytes)) { set_error("flx_cs_batch: the output byte pool is too small"); return FLX_ERR_CAPACITY; }
    used = 0;
    for (uint64_t i = 0; i < n_jobs; ++i) {                   // the strings packed in job order
        if (lens[i]) memcpy(out_bytes + used, slabs.data() + dj[i].cs_off, lens[i]);
        out[i] = flx_md_ref{used, lens[i], 0};
        used += lens[i];
    }
    return FLX_OK;
}
