// Alignment job batches (K0/K3/K4, alignment.cpp:83-181): de-duplication, launch shapes, one launch per shape class, and the score,
// trace, root-union and existence forms built on them (the traceback stage behind K4: flx_traceback.cpp; the C ABI of seam 2:
// flx_align_capi.cpp).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <numeric>
#include <string>

#include "flx_traceback.hpp"

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
}  // namespace
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
namespace {
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
}  // namespace

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

namespace {
// K3 / K4 over the requests [begin, end) of one call: one launch per shape class, the classes in ShapeKey order, the jobs of a class in
// request order (TRACE launches: widest window first, equal widths in request order). A job writes to out_index = its request - begin.
// per_job(request, job) sets what the caller's form adds to the job (trace arena and last-row offsets: it is called in job order) and
// returns the bytes the job moves beyond its n + m sequence symbols (the launch's accounting). The results: `table` over `outs`, in the
// lane's mapped result block when it has room, else on the device (the caller fetches it, waits and lands it).
struct ShapeLaunch { ShapeKey key; u32 first, count; u64 word_steps, bytes; };
template <class PerJob>
int launch_by_shape(Lane* ctx, const u8* d_text, const u64* d_peq, hvec<AlignRequest> const& reqs, hvec<AlignShape> const& shapes, size_t begin, size_t end,
                    const char* kernel_name, const char* what, bool trace, u16* d_lastrow, ResultTable& table, hvec<DevAlignOut>& outs, PerJob&& per_job) {
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
    if ((rc = table.place(ctx, ctx->job_out, outs, end - begin))) return rc;
    DevAlignOut* const out = table.dev<DevAlignOut>();
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
    ResultTable table;
    if ((rc = launch_by_shape(ctx, d_text, d_peq, reqs, shapes, 0, reqs.size(), kernel_name, "", false, nullptr, table, outs, [](u32, DevAlignJob&) { return (u64)0; }))) return rc;
    if ((rc = table.fetch(ctx))) return rc;
    jprof.mark("launch");
    rc = ctx->sync();
    if (!rc) table.land();
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

// score, begin position and CIGAR, and what `wants` adds, for every (distinct) request
int run_trace_jobs_unique(Lane* ctx, const u8* d_text, const u64* d_peq, hvec<AlignRequest> const& reqs,
                          hvec<TraceResult>& results, hvec<u32>& cigar_pool, TraceWants const& wants) {
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
        ResultTable table;
        hvec<DevAlignOut> outs;
        rc = launch_by_shape(ctx, d_text, d_peq, reqs, plan.shapes, begin, end, "ed_align_trace", "", true, nullptr, table, outs, [&](u32 id, DevAlignJob& job) {
            AlignRequest const& r = reqs[id];
            job.trace_off = trace_off[id - begin] = off;
            off += plan.slots[id];
            TraceLayout const tl = ckpt_trace_layout(r.n, r.m, r.k, plan.shapes[id].words_per_lane, plan.shapes[id].lanes_per_job);
            return (tl.carry_slots + tl.ckpt_slots) * 16;
        });
        if (rc) return rc;
        if ((rc = table.fetch(ctx))) return rc;
        if ((rc = ctx->sync())) return rc;
        table.land();
        tprof.mark("K4");

        // ---- traceback for the jobs that have an alignment within k
        Traceback tb(wants, &tprof);
        hvec<u32> tjob_req;
        for (size_t c = 0; c < count; ++c) {
            if (outs[c].score == 0xFFFFFFFFu) continue;
            tb.add(reqs[begin + c], trace_off[c], plan.shapes[begin + c], outs[c].end_col, outs[c].score);
            tjob_req.push_back((u32)(begin + c));
        }
        if ((rc = tb.run(ctx, d_text, d_peq, cigar_pool))) return rc;
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
                   hvec<TraceResult>& results, hvec<u32>& cigar_pool, TraceWants const& wants) {
    return run_deduplicated(reqs, results, [&](hvec<AlignRequest> const& uniq, hvec<TraceResult>& ures) {
        return run_trace_jobs_unique(ctx, d_text, d_peq, uniq, ures, cigar_pool, wants);
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
                                hvec<TraceResult>& ures, hvec<u32>& cigar_pool, TraceWants const& wants) {
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
    if (!usable || unions.size() == uniq.size()) return run_trace_jobs_unique(ctx, d_text, d_peq, uniq, ures, cigar_pool, wants);      // nothing to share: the plain path

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
        ResultTable union_table, win_table;
        hvec<DevAlignOut> union_outs;            // (the unions' own scores are not read: every member's comes from its window of the last row)
        rc = launch_by_shape(ctx, d_text, d_peq, ureqs, plan.shapes, begin, next, "ed_align_trace", " unions", true, ctx->lastrow.as<u16>(), union_table, union_outs, [&](u32 id, DevAlignJob& job) {
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
        hvec<DevAlignOut> wouts;
        if ((rc = win_table.place(ctx, ctx->row_out, wouts, n_wins))) return rc;
        rc = timed_launch(ctx, "ed_lastrow_min", rows * 2, n_wins, [&] {
            return DeviceApi::lastrow_min(ctx->stream, ctx->lastrow.as<u16>(), wins, (u32)n_wins, win_table.dev<DevAlignOut>());
        });
        if (rc) return rc;
        if ((rc = win_table.fetch(ctx))) return rc;
        if ((rc = ctx->sync())) return rc;
        win_table.land();

        // ---- one traceback per distinct (union, end column); the members of a union share its trace job's CIGAR words and MD string
        Traceback tb(wants);
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
        if ((rc = tb.run(ctx, d_text, d_peq, cigar_pool))) return rc;
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
        if ((rc = run_trace_jobs_unique(ctx, d_text, d_peq, fallback, fres, cigar_pool, wants))) return rc;
        for (size_t i = 0; i < fallback.size(); ++i) ures[fallback_of[i]] = fres[i];
    }
    if (getenv("FLX_ALIGN_DEBUG")) fprintf(stderr, "[root unions] requests %zu distinct %zu unions %zu aligned on their own %zu traceback jobs %zu unions with several jobs %zu\n", n_requests, uniq.size(), unions.size(), fallback.size(), n_tjobs, n_unions_several_jobs);
    return FLX_OK;
}

}  // namespace

int run_trace_jobs_union(Lane* ctx, const u8* d_text, const u64* d_peq, hvec<AlignRequest> const& reqs,
                         hvec<TraceResult>& results, hvec<u32>& cigar_pool, TraceWants const& wants) {
    return run_deduplicated(reqs, results, [&](hvec<AlignRequest> const& uniq, hvec<TraceResult>& ures) {
        return run_trace_jobs_union_unique(ctx, d_text, d_peq, uniq, reqs.size(), ures, cigar_pool, wants);
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
