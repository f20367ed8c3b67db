// One chunk of reads on one lane: the level-synchronous PEX verification driver (verification.cpp:8-245) as a list of stages.
// align_slice at the end of the file calls them in order; what a stage leaves for the later ones is in the Slice (flx_pipeline.hpp).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <string>
#include <tuple>
#include <vector>

#include "flx_fm_core.hpp"
#include "flx_mapq.hpp"
#include "flx_partial.hpp"
#include "flx_pipeline.hpp"
#include "flx_realign.hpp"
#include "flx_select.hpp"
#include "flx_tails.hpp"

namespace flx {

namespace {

struct half_open { u64 start, end; };
half_open trim_both(half_open a, u64 amount) {                                                  // intervals.cpp:48-58
    u64 const new_end = std::max(a.start + 1, amount > a.end ? 0 : a.end - amount);
    u64 const new_start = std::min(new_end - 1, a.start + amount);
    return {new_start, new_end};
}
struct VerifiedIntervals {                                                                     // intervals.cpp:84-127
    hvec<half_open> ivs;
    bool contains(half_open t) const {
        for (auto const& e : ivs) if (e.start <= t.start && e.end >= t.end) return true;      // equal or contains
        return false;
    }
    void insert(half_open t) { if (!contains(t)) ivs.push_back(t); }
};

Span compute_span(u64 anchor_pos, flx_pex_node const& node, u64 leaf_from, u64 reflen, double ratio) {   // verification.cpp:157-184
    u64 const base = (u64)(node.to - node.from + 1) + 2ull * node.num_errors + 1;
    u64 const extra = ratio == 0.0 ? 0 : fp_aware_ceil(base * ratio);        // (inner nodes: no extension, fp_aware_ceil(0) = 0)
    i64 const start_signed = (i64)anchor_pos - (i64)(leaf_from - node.from) - (i64)node.num_errors - (i64)extra;
    u64 const start = start_signed >= 0 ? (u64)start_signed : 0;
    u64 const length = std::min(base + 2 * extra, reflen - start);
    return {start, length, extra};
}

struct pr_task { int priority; int id; bool operator<(pr_task const& o) const { return priority < o.priority; } };
// order in which one worker runs the verification packages of a read (BS::thread_pool's priority queue), parallelization.cpp:131-148
hvec<int> package_order(int n) {
    std::priority_queue<pr_task> q;
    for (int i = 0; i < n; ++i) q.push(pr_task{16383, i});
    q.push(pr_task{-16384, -1});
    hvec<int> order;
    while (!q.empty()) { pr_task t = q.top(); q.pop(); if (t.id < 0) break; order.push_back(t.id); }
    return order;
}

// the window in which an anchor tests (or aligns) a node of its read's tree
AlignRequest window_request(Slice const& S, HostIndex const& H, AnchorState const& a, flx_pex_node const& node, double ratio, Span* span_out) {
    ReadState const& rs = S.reads[a.read];
    flx_pex_node const& leaf = rs.tree_ref().leaves[a.leaf];
    Span const sp = compute_span(a.pos, node, leaf.from, H.seq_len[a.ref_id], ratio);
    if (span_out) *span_out = sp;
    return AlignRequest{H.seq_start[a.ref_id] + sp.offset, rs.pool_off[a.orientation] + node.from, (u32)sp.length,
                        node.to - node.from + 1, node.num_errors};
}

// ---- 1. reads -> PEX trees (parallelization.cpp:77-98); the reads that the input rules skip are marked in run->skipped
int plan_reads(Slice& S, const flx_params* P, const flx_reads* RD, u64 first_read, u64 end_read, flx_run* run) {
    hvec<ReadState>& reads = S.reads;
    auto& tree_cache = S.tree_cache;
    reads.reserve(end_read - first_read);
    for (u64 i = first_read; i < end_read; ++i) {
        u64 const len = RD->lens[i];
        if (len == 0 || len > 100000) { run->skipped[i] = 1; continue; }                       // input.cpp:95-110
        u64 const k = P->query_error_probability >= 0 ? fp_aware_ceil(len * P->query_error_probability) : P->query_num_errors;
        if (len <= k || k < P->pex_seed_num_errors) { run->skipped[i] = 1; continue; }         // input.cpp:115-129
        if (len > align_supported_max_query()) { set_error("read longer than the supported maximum"); return FLX_ERR_UNSUPPORTED; }
        ReadState rs;
        rs.read_index = i;
        rs.len = (u32)len;
        rs.k = (u32)k;
        {
            auto it = tree_cache.find(std::make_pair(len, k));
            if (it == tree_cache.end())
                it = tree_cache.emplace(std::make_pair(len, k), std::make_unique<PexTree>(build_pex_tree(len, k, P->pex_seed_num_errors, P->bottom_up_pex_tree_building != 0))).first;
            rs.tree_ptr = it->second.get();
        }
        rs.pool_off[0] = RD->pool_off[i];
        rs.pool_off[1] = RD->pool_off[i] + len;
        reads.push_back(std::move(rs));
    }
    return FLX_OK;
}

// the seeds as a list (the host's selection, statistics, FLX_HOST_SEEDS=1)
void build_host_seeds(Slice& S, const flx_reads* RD) {
    hvec<ReadState> const& reads = S.reads;
    hvec<flx_seed>& seeds = S.seeds;
    hvec<u8>& seed_flags = S.seed_flags;
    u64 const step = S.step, n_seeds_total = S.seed_first[reads.size()];
    seeds.clear(); seed_flags.clear();
    seeds.reserve(n_seeds_total); seed_flags.reserve(n_seeds_total);
    for (size_t r = 0; r < reads.size(); ++r)
        for (int o = 0; o < 2; ++o)
            for (u64 l = 0; l < reads[r].tree_ref().leaves.size(); l += step) {
                flx_pex_node const& leaf = reads[r].tree_ref().leaves[l];
                seeds.push_back(flx_seed{reads[r].pool_off[o] + leaf.from, leaf.to - leaf.from + 1, leaf.num_errors, (u32)l, 0});
                seed_flags.push_back(RD->flags[reads[r].read_index]);
            }
}

// ---- 2. the seeds: every step-th leaf of a read's tree, forward then reverse complement (pex.cpp:258-277). Seed s of the chunk =
//      (read, orientation, leaf) by the reads' seed ranges: seed_first[r] .. seed_first[r + 1], n_sampled(r) per orientation.
int plan_seeds(Slice& S, const flx_params* P, const flx_reads* RD) {
    hvec<ReadState> const& reads = S.reads;
    u64 const step = S.step = std::max<u64>(1, P->seed_sampling_step_size);
    auto n_sampled = [&](ReadState const& r) { return S.n_sampled(r); };
    hvec<u32>& seed_first = S.seed_first;
    seed_first.assign(reads.size() + 1, 0);
    for (size_t r = 0; r < reads.size(); ++r) seed_first[r + 1] = seed_first[r] + 2u * n_sampled(reads[r]);
    u64 const n_seeds_total = seed_first[reads.size()];
    // the same as a description the device writes the seeds from: per tree its sampled leaves with their class (errors, length) and rank
    // within the class, per read where its seeds of each class start in launch order (heaviest class first: more errors, then shorter)
    SeedGen& gen = S.gen;
    bool const use_gen = S.use_gen = !getenv("FLX_HOST_SEEDS") && n_seeds_total > 0 && n_seeds_total < (1ull << 31);
    if (use_gen) {
        struct TreePlan { u32 leaf_first; hvec<u32> class_key, class_count; };
        std::map<const PexTree*, TreePlan> plans;
        struct GlobalClass { u64 pos = 0; u32 scheme_off = 0, nsearch = 0; };
        std::map<u32, GlobalClass> global;                             // class key -> seeds of the class in the chunk, then its next launch position; its scheme
        for (auto const& rs : reads) {
            auto it = plans.find(rs.tree_ptr);
            if (it == plans.end()) {
                TreePlan tp;
                tp.leaf_first = (u32)gen.leaves.size();
                for (u64 l = 0; l < rs.tree_ref().leaves.size(); l += step) {
                    flx_pex_node const& leaf = rs.tree_ref().leaves[l];
                    u32 const length = leaf.to - leaf.from + 1, key = ((3u - std::min<u32>(leaf.num_errors, 3u)) << 24) | length;
                    size_t c = 0;
                    while (c < tp.class_key.size() && tp.class_key[c] != key) ++c;
                    if (c == tp.class_key.size()) { tp.class_key.push_back(key); tp.class_count.push_back(0); }
                    gen.leaves.push_back(DevSeedLeaf{leaf.from, length, (u32)c, tp.class_count[c]++});
                    gen.max_errors = std::max(gen.max_errors, leaf.num_errors);
                    gen.max_length = std::max(gen.max_length, length);
                }
                it = plans.emplace(rs.tree_ptr, std::move(tp)).first;
            }
            for (size_t c = 0; c < it->second.class_key.size(); ++c) global[it->second.class_key[c]].pos += 2ull * it->second.class_count[c];
        }
        if (gen.max_errors > 3) { set_error("seed errors must be in [0,3] (floxer_cli.cpp:299)"); return FLX_ERR_INVALID; }
        u64 pos = 0;
        for (auto& kv : global) {                                      // ascending key = heaviest class first
            u32 const errors = 3u - (kv.first >> 24), length = kv.first & 0xFFFFFFu;
            auto const e = expanded_scheme(errors, length);
            kv.second.scheme_off = (u32)gen.scheme_table.size();
            kv.second.nsearch = e.empty() ? 0 : (u32)(e.size() / length);
            gen.scheme_table.insert(gen.scheme_table.end(), e.begin(), e.end());
            u64 const n = kv.second.pos;
            kv.second.pos = pos;
            pos += n;
        }
        gen.reads.reserve(reads.size());
        for (size_t r = 0; r < reads.size(); ++r) {
            ReadState const& rs = reads[r];
            TreePlan const& tp = plans.find(rs.tree_ptr)->second;
            gen.reads.push_back(DevSeedRead{rs.pool_off[0], rs.pool_off[1], tp.leaf_first, n_sampled(rs), seed_first[r], (u32)gen.classes.size(), RD->flags[rs.read_index], 0});
            for (size_t c = 0; c < tp.class_key.size(); ++c) {
                auto& g = global[tp.class_key[c]];
                u32 const errors = 3u - (tp.class_key[c] >> 24), length = tp.class_key[c] & 0xFFFFFFu;
                gen.classes.push_back(DevSeedClass{(u32)g.pos, tp.class_count[c], g.scheme_off, (length + errors + 3) | (g.nsearch << 24)});
                g.pos += 2ull * tp.class_count[c];
            }
        }
        gen.n_seeds = n_seeds_total;
    } else build_host_seeds(S, RD);
    return FLX_OK;
}

// ---- 3. seeding: the anchors of the chunk's seeds, in seed order
int search_seeds(Slice& S, Lane* lane, const flx_params* P, const flx_reads* RD) {
    hvec<u8> const& pool = RD->pool;
    const u8* d_pool = RD->d_pool.as<u8>();
    hvec<HostAnchor>& anchors = S.anchors;
    hvec<SeedStats>& sstats = S.sstats;
    // statistics in the reference's form (flx_stats.cpp), when the context has a statistics object attached
    if (lane->ctx->read_stats) S.st_local = std::make_unique<Stats>(stats_simulated(lane->ctx->read_stats));
    S.t_slice = std::chrono::steady_clock::now();
    // (K1 starts behind K0 and the pool's 2-bit form: the event is recorded when the first call on these reads has queued both)
    FLX_HIP(hipStreamWaitEvent(lane->stream, RD->peq_event, 0));
    int rc = S.use_gen ? search_seeds_device(lane, d_pool, pool.data(), pool.size(), nullptr, 0, P->search, anchors, sstats, nullptr, 0,
                                       RD->d_pack.ptr ? RD->d_pack.as<u32>() : nullptr, nullptr, &S.gen)
                 : SEARCH_NEEDS_HOST_SEEDS;
    if (rc == SEARCH_NEEDS_HOST_SEEDS) {
        if (S.use_gen) build_host_seeds(S, RD);
        rc = search_seeds_device(lane, d_pool, pool.data(), pool.size(), S.seeds.data(), S.seeds.size(), P->search, anchors, sstats, nullptr, 0,
                                 RD->d_pack.ptr ? RD->d_pack.as<u32>() : nullptr, S.seed_flags.data());
    }
    return rc;
}

// per-query seed statistics, and every anchor's seed -> (read, orientation, leaf)
void anchors_to_reads(Slice& S) {
    hvec<ReadState>& reads = S.reads;
    hvec<u32> const& seed_first = S.seed_first;
    hvec<HostAnchor> const& anchors = S.anchors;
    hvec<SeedStats> const& sstats = S.sstats;
    u64 const step = S.step;
    auto n_sampled = [&](ReadState const& r) { return S.n_sampled(r); };
    Stats* const st_local = S.st_local.get();
    double const search_ms = S.search_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - S.t_slice).count();
    if (st_local) {
        // per query: its length, its seeds (forward then reverse complement: one contiguous run of the seed list) and their
        // selection counters (statistics.cpp:283-295, 367-419)
        hvec<SeedStatRow> rows;
        for (size_t r = 0; r < reads.size(); ++r) {
            st_local->at(Stats::QUERY_LENGTHS).add(reads[r].len);
            rows.clear();
            u32 const nl = n_sampled(reads[r]);
            for (u32 si = seed_first[r]; si < seed_first[r + 1]; ++si) {
                flx_pex_node const& leaf = reads[r].tree_ref().leaves[(u64)((si - seed_first[r]) % nl) * step];
                st_local->at(Stats::ERRORS_PER_SEED).add(leaf.num_errors);
                st_local->at(Stats::SEED_LENGTHS).add(leaf.to - leaf.from + 1);
                rows.push_back(SeedStatRow{sstats[si].useful, sstats[si].raw, sstats[si].excluded_soft});
            }
            st_local->at(Stats::SEEDS_PER_QUERY).add(rows.size());
            st_local->add_search_result(rows.data(), rows.size());
            st_local->at(Stats::MS_SEARCH).add((u64)(search_ms / (double)std::max<size_t>(1, reads.size())));
        }
    }
    hvec<AnchorState>& A = S.A;
    A.assign(anchors.size(), AnchorState{});
    u32 rd_i = 0;
    for (size_t a = 0; a < anchors.size(); ++a) {
        // the anchor's seed -> (read, orientation, leaf); the anchors come seed by seed, so the read mostly stays or moves on by one
        u32 const si = anchors[a].seed_index;
        if (si < seed_first[rd_i] || si >= seed_first[rd_i + 1]) {
            if (si >= seed_first[rd_i + 1] && rd_i + 2 < seed_first.size() && si < seed_first[rd_i + 2]) ++rd_i;
            else rd_i = (u32)(std::upper_bound(seed_first.begin(), seed_first.end(), si) - seed_first.begin() - 1);
        }
        u32 const nl = n_sampled(reads[rd_i]), local = si - seed_first[rd_i];
        u8 const orientation = local >= nl ? 1 : 0;
        A[a].read = rd_i;
        A[a].orientation = orientation;
        A[a].leaf = (u32)((u64)(local - (orientation ? nl : 0u)) * step);
        A[a].ref_id = anchors[a].ref_id;
        A[a].pos = anchors[a].pos;
        reads[rd_i].anchor_ids[orientation].push_back((u32)a);
    }
}

// ---- 4. verification order of each read: packages (forward then reverse complement, <= N anchors each) in the order one
//      worker would run them (parallelization.cpp:14-43, 230)
void verification_order(Slice& S, const flx_params* P) {
    hvec<ReadState> const& reads = S.reads;
    hvec<hvec<u32>>& exec_order = S.exec_order;
    exec_order.assign(reads.size(), hvec<u32>{});
    for (size_t r = 0; r < reads.size(); ++r) {
        hvec<std::pair<u32, u32>> pkgs;          // (first, count) into a concatenated list
        hvec<u32> concat;
        for (int o = 0; o < 2; ++o) {
            auto const& ids = reads[r].anchor_ids[o];
            for (size_t i = 0; i < ids.size(); i += P->num_anchors_per_verification_task) {
                u32 const cnt = (u32)std::min<size_t>(P->num_anchors_per_verification_task, ids.size() - i);
                pkgs.emplace_back((u32)concat.size(), cnt);
                concat.insert(concat.end(), ids.begin() + i, ids.begin() + i + cnt);
            }
        }
        for (int pid : package_order((int)pkgs.size()))
            for (u32 j = 0; j < pkgs[pid].second; ++j) exec_order[r].push_back(concat[pkgs[pid].first + j]);
    }
}

// ---- 5. hierarchical verification, level-synchronous (verification.cpp:44-117): inner nodes only test existence and do
//      not depend on the interval cache, so all anchors climb together; an anchor stops at its first failing node.
// every anchor's first inner node; returns how many anchors have one to test
u32 start_climb(Slice& S, const flx_params* P) {
    u32 n_climbing = 0;
    for (auto& a : S.A) {
        ReadState const& rs = S.reads[a.read];
        flx_pex_node const& leaf = rs.tree_ref().leaves[a.leaf];
        if (P->direct_full_verification || leaf.parent_id == FLX_NULL_ID) { a.at_root = true; continue; }   // verification.cpp:23-42, 52-72
        a.node = leaf.parent_id;
        if (rs.tree_ref().inner[a.node].parent_id == FLX_NULL_ID) a.at_root = true;
        n_climbing += !a.at_root;
    }
    return n_climbing;
}

// Anchors do not wait for each other and their tests do not depend on any order, so a round tests the anchors whose
// current node is in the smallest size class still pending (PEX trees are unbalanced: the same node is reached after a
// different number of steps from different leaves). All tests of a node size then share one launch, and identical
// (window, node) tests requested by anchors that started at different depths are found by the de-duplication.
// The rounds run with the anchors' state resident on the device (requests, de-duplication, clusters and the moves up the trees
// are kernels; the host launches K3 on each round's job list and decides per cluster). FLX_HOST_ROUNDS=1, or a statistics
// object on the context (it wants every request's window), selects climb_on_host instead; both give the same records.
int climb_on_device(Slice& S, Lane* lane, const flx_reads* RD) {
    flx_ctx* ctx = lane->ctx;
    HostIndex const& H = *ctx->hidx;
    hvec<ReadState> const& reads = S.reads;
    hvec<AnchorState>& A = S.A;
    const u8* d_text = ctx->didx.text;
    const u64* const d_peq = RD->d_peq.as<u64>();              // built once per resident read set (flx_align_reads_resident)
    int rc;
    u32 const n = (u32)A.size();
    PhaseTimer vprof("rounds");
    // ---- node table of the chunk's trees, anchors, the anchors of every query (read x orientation: contiguous, the anchors are in
    //      seed order)
    std::map<const PexTree*, u32> tree_base;
    hvec<DevVrNode> nodes;
    for (auto const& kv : S.tree_cache) {
        PexTree const& t = *kv.second;
        tree_base[&t] = (u32)nodes.size();
        for (auto const& nd : t.inner) nodes.push_back(DevVrNode{nd.parent_id, nd.from, nd.to - nd.from + 1, nd.num_errors});
    }
    if (nodes.empty()) nodes.push_back(DevVrNode{0xFFFFFFFFu, 0, 1, 0});
    u32 const n_queries = (u32)(2 * reads.size());
    // ---- one device buffer cut into the arrays of Vr2Buffers. What the host fills (anchors, nodes, the queries' first anchors, every
    //      anchor's node and status) and what starts from a constant (the job slots: ~0, the scalars: 0) lie in front, in one image that is
    //      built in the lane's staging block and goes up in one copy; node and status, next to each other, come back in one
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t const at = off; off += (bytes + 255) & ~(size_t)255; return at; };
    size_t const o_anchors = take((size_t)n * sizeof(DevVrAnchor)), o_nodes = take(nodes.size() * sizeof(DevVrNode)), o_qfirst = take(((size_t)n_queries + 1) * 4),
                 o_node = take((size_t)n * 4), o_status = take(n), o_slot = take((size_t)n * 4), o_scalars = take(VR2_SCALARS * 4), image_bytes = off,
                 o_jobs = take((size_t)n * 2 * sizeof(DevAlignJob)), o_outs = take((size_t)n * 2 * sizeof(DevAlignOut));
    if ((rc = lane->vr.ensure(off))) return rc;
    char* const image = (char*)lane->stage_begin(image_bytes);
    if (!image) return FLX_ERR_NO_DEVICE;
    memset(image, 0, image_bytes);                              // (the gaps between the arrays as well)
    DevVrAnchor* const da = (DevVrAnchor*)(image + o_anchors);
    u32* const q_first = (u32*)(image + o_qfirst);
    u32* const h_node = (u32*)(image + o_node);
    u8* const h_status = (u8*)(image + o_status);
    memcpy(image + o_nodes, nodes.data(), nodes.size() * sizeof(DevVrNode));
    memset(image + o_slot, 0xFF, (size_t)n * 4);
    u32 n_climbing = 0, smallest = 0xFFFFFFFFu;
    for (u32 i = 0; i < n; ++i) {
        AnchorState const& a = A[i];
        ReadState const& rs = reads[a.read];
        flx_pex_node const& leaf = rs.tree_ref().leaves[a.leaf];
        u32 const tb = tree_base[rs.tree_ptr];
        u32 const query = 2u * a.read + a.orientation;
        q_first[query + 1]++;
        da[i] = DevVrAnchor{(i64)a.pos - (i64)leaf.from, H.seq_start[a.ref_id], H.seq_len[a.ref_id], rs.pool_off[a.orientation], tb, query};
        bool const climbs = a.alive && !a.at_root;
        h_node[i] = climbs ? a.node : 0u;
        h_status[i] = climbs ? VR_CLIMBING : a.at_root ? VR_AT_ROOT : VR_DEAD;
        if (climbs) { ++n_climbing; smallest = std::min(smallest, nodes[tb + a.node].rows); }
        if (i > 0 && 2u * A[i - 1].read + A[i - 1].orientation > query) { set_error("verification rounds: anchors out of query order"); return FLX_ERR_INTERNAL; }
    }
    for (u32 qi = 0; qi < n_queries; ++qi) q_first[qi + 1] += q_first[qi];
    vprof.mark("anchor-table");
    char* const base = (char*)lane->vr.ptr;
    Vr2Buffers B{};
    B.anchors = (const DevVrAnchor*)(base + o_anchors); B.nodes = (const DevVrNode*)(base + o_nodes); B.q_first = (const u32*)(base + o_qfirst);
    B.node = (u32*)(base + o_node); B.status = (u8*)(base + o_status); B.a_slot = (u32*)(base + o_slot);
    B.jobs = (DevAlignJob*)(base + o_jobs); B.outs = (DevAlignOut*)(base + o_outs); B.scalars = (u32*)(base + o_scalars);
    FLX_HIP(hipMemcpyAsync(base, image, image_bytes, hipMemcpyHostToDevice, lane->stream));
    if (!lane->vr_host_scalars) FLX_HIP(hipHostMalloc((void**)&lane->vr_host_scalars, VR2_SCALARS * 4, hipHostMallocMapped));
    vprof.mark("upload");
    u64 const few_waves = align_few_waves();
    u64 prev_jobs = n_climbing / 2, acc_steps = 0, acc_bytes = 0, acc_req = 0;
    for (u32 round = 0; n_climbing > 0; ++round) {
        u64 const limit = (u64)smallest * round_span_percent() / 100;
        // One launch shape for the round: the cheapest that holds the window of every node in the round's size class, or the one
        // with the fewest words per lane when the round has few jobs (they would leave most SIMDs without a wave; the last round's
        // job count is the estimate: either shape holds every job)
        u32 nw_max = 0;
        i64 width_max = 0;
        for (auto const& nd : nodes)
            if (nd.rows >= smallest && nd.rows <= limit) {
                nw_max = std::max(nw_max, (nd.rows + 63u) / 64u);
                width_max = std::max<i64>(width_max, 4 * (i64)nd.errors + 1);            // a window of its own: n - m + 2k = (2e + 1) + 2e
            }
        AlignShape const shape_t = DeviceApi::shape_holding(nw_max, width_max, false), shape_p = DeviceApi::shape_holding(nw_max, width_max, true);
        if (shape_t.words_per_lane == 0 || shape_p.words_per_lane == 0) { set_error("query longer than the supported maximum"); return FLX_ERR_UNSUPPORTED; }
        AlignShape const shape = prev_jobs * shape_t.lanes_per_job / 64 >= few_waves ? shape_t : shape_p;
        // what the shape holds beyond that goes to the clusters' union windows (a shape holds a job when every word group has a lane of
        // its own, when the ring's lanes are free again before their next group starts: 64 W (R - 1) + R + 1 > diagonals, or when the
        // steps a revolution of the ring has to wait fit the launch's hand-over slots: flx_internal.hpp, ring_delay)
        u64 const width_cap = DeviceApi::shape_width_cap(nw_max, shape);
        u32 const max_jobs = (u32)std::min<u64>(2ull * n_climbing, 2ull * n);
        int const e1 = DeviceApi::vr2_request(lane->stream, B, n_queries, (u32)std::min<u64>(limit, 0xFFFFFFFFu), shape.words_per_lane,
                                              (u32)std::min<u64>(width_cap, 0xFFFFFFFFull), round);
        if (e1) { set_error(std::string("verification round: ") + hipGetErrorString((hipError_t)e1)); return FLX_ERR_NO_DEVICE; }
        rc = timed_launch(lane, "ed_align_exists", 0, 0, [&] {
            // (a fixed grid of at most this many waves takes the round's job groups in turn; FLX_EXISTS_MAX_WAVES: how much of the chip one
            // round's launch may hold while the other lanes' kernels want room)
            static u32 const exists_waves = [] { const char* e = getenv("FLX_EXISTS_MAX_WAVES"); return (u32)(e ? std::max(64, atoi(e)) : 8192); }();
            return DeviceApi::align_exists_counted(lane->stream, d_text, d_peq, B.jobs, max_jobs, B.scalars + VR2_N_JOBS + (round & 1u), shape, exists_waves, B.outs, B.scalars + VR2_QUEUE_ERR);
        });
        if (rc) return rc;
        int const e2 = DeviceApi::vr2_apply(lane->stream, B, n, lane->vr_host_scalars);
        if (e2) { set_error(std::string("verification round: ") + hipGetErrorString((hipError_t)e2)); return FLX_ERR_NO_DEVICE; }
        if ((rc = lane->sync())) return rc;
        u32 sc[VR2_SCALARS];
        memcpy(sc, lane->vr_host_scalars, sizeof(sc));            // (left there by the last block of vr2_apply)
        if (sc[VR2_QUEUE_ERR]) { set_error("existence tests: a window did not fit the row buffers"); return FLX_ERR_INTERNAL; }
        u64 ws, by;
        memcpy(&ws, &sc[VR2_WORD_STEPS], 8);
        memcpy(&by, &sc[VR2_BYTES], 8);
        if (ctx->timing) {        // the round's word-steps and sequence bytes were counted on the device: fold them into the kernel's accounting
            std::lock_guard<std::mutex> g(ctx->mu);
            auto it = ctx->stats.find("ed_align_exists");
            if (it != ctx->stats.end()) { it->second.algorithmic_bytes += by - acc_bytes; it->second.work_units += ws - acc_steps; }
        }
        u64 const round_req = sc[VR2_N_REQ] - acc_req;
        acc_steps = ws; acc_bytes = by; acc_req = sc[VR2_N_REQ];
        S.n_inner_requested += round_req;
        if (round_req == 0 && sc[VR2_N_CLIMBING] >= n_climbing) { set_error("verification rounds do not advance"); return FLX_ERR_INTERNAL; }
        prev_jobs = sc[VR2_N_JOBS + (round & 1u)];
        n_climbing = sc[VR2_N_CLIMBING];
        smallest = sc[VR2_SMALLEST];
        vprof.mark("round");
    }
    // (node and status back in one copy, over the image's own copy of them: the rounds' last wait is long past the upload)
    if ((rc = lane->wait_idle())) return rc;
    if (n) FLX_HIP(hipMemcpyAsync(image + o_node, base + o_node, o_status + n - o_node, hipMemcpyDeviceToHost, lane->stream));
    if ((rc = lane->sync())) return rc;
    for (u32 i = 0; i < n; ++i) {
        AnchorState& a = A[i];
        if (h_status[i] == VR_DEAD && a.alive && !a.at_root) { a.alive = false; a.node = h_node[i]; }      // (the node it failed at, as climb_on_host leaves it)
        else if (h_status[i] == VR_AT_ROOT && !a.at_root) { a.at_root = true; a.node = h_node[i]; }
    }
    vprof.mark("read-back");
    return FLX_OK;
}

int climb_on_host(Slice& S, Lane* lane, const flx_reads* RD, ExistsTimes& times) {
    flx_ctx* ctx = lane->ctx;
    HostIndex const& H = *ctx->hidx;
    hvec<ReadState> const& reads = S.reads;
    hvec<AnchorState>& A = S.A;
    const u8* d_text = ctx->didx.text;
    const u64* const d_peq = RD->d_peq.as<u64>();
    int rc;
    hvec<u32> climbing;                 // anchors that still have an inner node to test (in anchor order)
    for (u32 ai = 0; ai < A.size(); ++ai) if (A[ai].alive && !A[ai].at_root) climbing.push_back(ai);
    hvec<AlignRequest> reqs;
    hvec<DevAlignOut> outs;
    auto rows_of = [&](AnchorState const& a) { flx_pex_node const& nd = reads[a.read].tree_ref().inner[a.node]; return nd.to - nd.from + 1; };
    // `climbing` carries each anchor's node size next to its index (the rounds scan it): {anchor, rows}
    struct Climber { u32 anchor, rows; };
    hvec<Climber> climbers, sel, wait, surv;
    u32 smallest = 0xFFFFFFFFu;
    climbers.reserve(climbing.size());
    for (u32 ai : climbing) { u32 const r = rows_of(A[ai]); climbers.push_back(Climber{ai, r}); smallest = std::min(smallest, r); }
    while (!climbers.empty()) {
        u64 const limit = (u64)smallest * round_span_percent() / 100;
        auto const tb0 = std::chrono::steady_clock::now();
        sel.clear();
        wait.clear();
        surv.clear();
        reqs.clear();
        u32 next_smallest = 0xFFFFFFFFu;
        for (Climber const& c : climbers) {                  // both parts stay in anchor order
            if (c.rows <= limit) {
                sel.push_back(c);
                reqs.push_back(window_request(S, H, A[c.anchor], reads[A[c.anchor].read].tree_ref().inner[A[c.anchor].node], 0.0, nullptr));
            } else { wait.push_back(c); next_smallest = std::min(next_smallest, c.rows); }
        }
        times.build_requests += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count();
        S.n_inner_requested += reqs.size();
        // (statistics: the inner tests are counted per anchor in the interval pass below - under -I the reference never starts on an
        // anchor whose root window is already verified, verification.cpp:45)
        if ((rc = run_exists_jobs(lane, d_text, d_peq, reqs, outs, times))) return rc;
        for (size_t i = 0; i < outs.size(); ++i) {
            AnchorState& a = A[sel[i].anchor];
            if (outs[i].score == 0xFFFFFFFFu) { a.alive = false; continue; }
            a.node = reads[a.read].tree_ref().inner[a.node].parent_id;
            if (reads[a.read].tree_ref().inner[a.node].parent_id == FLX_NULL_ID) a.at_root = true;
            else { u32 const r = rows_of(a); surv.push_back(Climber{sel[i].anchor, r}); next_smallest = std::min(next_smallest, r); }
        }
        climbers.resize(wait.size() + surv.size());
        std::merge(wait.begin(), wait.end(), surv.begin(), surv.end(), climbers.begin(), [](Climber const& x, Climber const& y) { return x.anchor < y.anchor; });
        smallest = next_smallest;
    }
    return FLX_OK;
}

// ---- 6. interval pass in verification order (verification.cpp:45, 106-109, 119-136): decides which anchors align the root
void interval_pass(Slice& S, const flx_params* P, HostIndex const& H) {
    hvec<ReadState> const& reads = S.reads;
    hvec<AnchorState>& A = S.A;
    hvec<hvec<u32>> const& exec_order = S.exec_order;
    Stats* const st_local = S.st_local.get();
    hvec<AlignRequest>& root_reqs = S.root_reqs;
    hvec<u32>& root_anchor = S.root_anchor;
    hvec<Span>& root_spans = S.root_spans;
    // statistics: the inner nodes an anchor tested (verification.cpp:241) - its leaf's parent, upwards, to the node it failed at or to
    // the node below the root
    auto add_inner_spans = [&](AnchorState const& a) {
        auto const& tree = reads[a.read].tree_ref();
        flx_pex_node const& leaf = tree.leaves[a.leaf];
        if (P->direct_full_verification || leaf.parent_id == FLX_NULL_ID) return;
        for (u32 nd = leaf.parent_id; tree.inner[nd].parent_id != FLX_NULL_ID; nd = tree.inner[nd].parent_id) {
            st_local->at(Stats::SPAN_INNER).add(window_request(S, H, a, tree.inner[nd], 0.0, nullptr).n);
            if (!a.alive && nd == a.node) break;
        }
    };
    for (size_t r = 0; r < reads.size(); ++r) {
        hvec<VerifiedIntervals> cache[2];
        if (P->use_interval_optimization) { cache[0].resize(H.seq_len.size()); cache[1].resize(H.seq_len.size()); }
        for (u32 ai : exec_order[r]) {
            AnchorState& a = A[ai];
            ReadState const& rs = reads[a.read];
            Span sp;
            AlignRequest const req = window_request(S, H, a, rs.tree_ref().root(), P->extra_verification_ratio, &sp);
            if (P->use_interval_optimization) {
                auto& ivs = cache[a.orientation][a.ref_id];
                if (ivs.contains(trim_both({sp.offset, sp.offset + sp.length}, sp.extra))) {           // root_was_already_verified
                    if (st_local) st_local->at(Stats::SPAN_ROOT_AVOIDED).add(sp.length);                // verification.cpp:130
                    continue;
                }
                if (st_local) add_inner_spans(a);
                if (!(a.alive && a.at_root)) continue;
                ivs.insert({sp.offset, sp.offset + sp.length});
            } else {
                if (st_local) add_inner_spans(a);
                if (!(a.alive && a.at_root)) continue;
            }
            a.wants_root = true;
            if (st_local) st_local->at(Stats::SPAN_ROOT).add(sp.length);                               // verification.cpp:239
            root_reqs.push_back(req);
            root_anchor.push_back(ai);
            root_spans.push_back(sp);
        }
    }
}

// ---- 7. root alignments (alignment.cpp:115-180)
int align_roots(Slice& S, Lane* lane, const flx_params* P, RunOptions const& R, const flx_reads* RD) {
    flx_ctx* ctx = lane->ctx;
    HostIndex const& H = *ctx->hidx;
    hvec<u8> const& pool = RD->pool;
    hvec<AlignRequest> const& root_reqs = S.root_reqs;
    hvec<Span> const& root_spans = S.root_spans;
    hvec<RootAlignment>& root_res = S.root_res;
    root_res.assign(root_reqs.size(), RootAlignment{});
    int rc;
    if (P->without_cigar) {
        if ((rc = ensure_reversed_text(lane))) return rc;
        {
            std::lock_guard<std::mutex> g(RD->peq_mu);
            if (!RD->rev_built) {
                hvec<u8> qrev(pool.rbegin(), pool.rend());
                take_spare_read_buffer(ctx, 3, RD->d_pool_rev);
                take_spare_read_buffer(ctx, 4, RD->d_peq_rev);
                if ((rc = RD->d_pool_rev.ensure(qrev.size() + 256))) return rc;
                FLX_HIP(hipMemcpyAsync(RD->d_pool_rev.ptr, qrev.data(), qrev.size(), hipMemcpyHostToDevice, lane->stream));
                FLX_HIP(hipMemsetAsync((char*)RD->d_pool_rev.ptr + qrev.size(), 0, 192, lane->stream));
                if ((rc = build_peq(lane, RD->d_pool_rev.as<u8>(), qrev.size(), RD->d_peq_rev))) return rc;
                if (!RD->rev_event) FLX_HIP(hipEventCreateWithFlags(&RD->rev_event, hipEventDisableTiming));
                FLX_HIP(hipEventRecord(RD->rev_event, lane->stream));
                FLX_HIP(hipStreamSynchronize(lane->stream));        // qrev leaves scope
                RD->rev_built = true;
            }
        }
        FLX_HIP(hipStreamWaitEvent(lane->stream, RD->rev_event, 0));
        hvec<AlignRequest> rev(root_reqs.size());
        for (size_t i = 0; i < rev.size(); ++i)
            rev[i] = AlignRequest{H.n - root_reqs[i].ref_off - root_reqs[i].n, pool.size() - root_reqs[i].q_off - root_reqs[i].m,
                                  root_reqs[i].n, root_reqs[i].m, root_reqs[i].k};
        hvec<DevAlignOut> outs;
        if ((rc = run_score_jobs(lane, ctx->text_rev.as<u8>() + TEXT_PAD, RD->d_peq_rev.as<u64>(), rev, outs, "ed_align_exists"))) return rc;
        for (size_t i = 0; i < outs.size(); ++i)
            if (outs[i].score != 0xFFFFFFFFu) { root_res[i].exists = true; root_res[i].nm = root_res[i].ed = outs[i].score; root_res[i].start = root_spans[i].offset + (root_reqs[i].n - outs[i].end_col); }
    } else {
        hvec<TraceResult> tres;
        // (flx_split_options: the tails of every root path come back with its CIGAR words; no other trace of the slice asks for them)
        TailParams const tails{split_weight(R.split.error_weight), split_x_drop(R.split.x_drop), split_min_tail_rows(R.split.min_tail_rows)};
        if ((rc = S.trace_windows(lane, RD, root_reqs, tres, R.split.enable ? &tails : nullptr))) return rc;
        for (size_t i = 0; i < tres.size(); ++i)
            if (tres[i].exists)
                root_res[i] = RootAlignment{true, root_spans[i].offset + tres[i].begin, tres[i].nm, tres[i].cigar_off, tres[i].cigar_len, tres[i].md_off, tres[i].md_len, tres[i].tail, tres[i].ed, tres[i].cs_off, tres[i].cs_len};
    }
    return FLX_OK;
}

// [left]S + the core words + [right]S as new words behind the pool's (the core's words may be shared with other records); {offset, length}
std::pair<u64, u32> append_clipped(hvec<u32>& cig, u32 left, u64 core_off, u32 core_len, u32 right) {
    u64 const off = cig.size();
    auto clip = [&](u32 rows) { if (rows) cig.push_back((rows << 4) | 4u); };
    clip(left);
    size_t const at = cig.size();
    cig.resize(at + core_len);                             // (grown first: the source lies in the same pool)
    std::copy(cig.begin() + (long)core_off, cig.begin() + (long)(core_off + core_len), cig.begin() + (long)at);
    clip(right);
    return {off, (u32)(cig.size() - off)};
}

// ---- 7b. reads mapped in full whose primary carries a chimeric tail (flx_split_options; the rule: flx_tails.hpp, its numbers came back
//      with the root CIGARs): the primary is traced again over the kept part, and the nodes that the read's anchors passed inside a
//      tail are traced as rescue_partials traces them; one trace over both for the whole slice. Does nothing, and launches nothing,
//      when the option is off or no primary has a tail
int split_tails(Slice& S, Lane* lane, const flx_params* P, RunOptions const& R, const flx_reads* RD) {
    if (!R.split.enable) return FLX_OK;
    HostIndex const& H = *lane->ctx->hidx;
    hvec<ReadState> const& reads = S.reads;
    hvec<AnchorState> const& A = S.A;
    hvec<RootAlignment> const& root_res = S.root_res;
    hvec<hvec<u32>> roots_of_read(reads.size());
    for (u32 i = 0; i < S.root_anchor.size(); ++i) roots_of_read[A[S.root_anchor[i]].read].push_back(i);
    u32 const min_span = partial_min_span(&R.partial), max_records = partial_max_records(&R.partial);
    struct Split { u32 read, root, req; u32 cand_first, cand_end; };
    struct Candidate { u8 orientation; u32 ref_id; flx_pex_node node; Span span; };
    hvec<Split> splits;
    hvec<Candidate> cands;
    hvec<AlignRequest> reqs;
    hvec<u32> cand_req;
    std::map<std::tuple<u64, u32, u32, u64, u32>, u32> seen;
    for (size_t r = 0; r < reads.size(); ++r) {
        // the primary, as write_records finds it: the first record with the best NM, references in id order
        bool have = false;
        u32 best = 0, prim = 0;
        for (u32 i : roots_of_read[r]) if (root_res[i].exists && (!have || root_res[i].nm < best)) { best = root_res[i].nm; have = true; }
        if (!have) continue;
        have = false;
        for (u32 ref = 0; ref < H.seq_len.size() && !have; ++ref)
            for (u32 i : roots_of_read[r])
                if (A[S.root_anchor[i]].ref_id == ref && root_res[i].exists && root_res[i].nm == best) { prim = i; have = true; break; }
        RootAlignment const& pr = root_res[prim];
        DevTailOut const& t = pr.tail;
        if (!t.left_rows && !t.right_rows) continue;
        ReadState const& rs = reads[r];
        AnchorState const& pa = A[S.root_anchor[prim]];
        u32 const len = rs.len;
        u64 const span = cigar_reference_span(S.cig.data() + pr.cigar_off, pr.cigar_len);
        if ((u64)t.left_rows + t.right_rows >= len) continue;             // (error rates beyond 1 / w: the score never rises, nothing would be kept)
        if ((u64)t.left_cols + t.right_cols > span || (u64)t.left_errors + t.right_errors > pr.nm) {
            set_error("split tails: a tail larger than its alignment"); return FLX_ERR_INTERNAL;
        }
        Split sp{(u32)r, prim, (u32)reqs.size(), (u32)cands.size(), 0};
        reqs.push_back(AlignRequest{H.seq_start[pa.ref_id] + pr.start + t.left_cols, rs.pool_off[pa.orientation] + t.left_rows,
                                    (u32)(span - t.left_cols - t.right_cols), len - t.left_rows - t.right_rows, pr.nm - t.left_errors - t.right_errors});
        // the tails' read-forward intervals, half-open: [0] the oriented left tail, [1] the right one
        u32 tail_lo[2] = {0, len - t.right_rows}, tail_hi[2] = {t.left_rows, len};
        if (pa.orientation) { tail_lo[0] = len - t.left_rows; tail_hi[0] = len; tail_lo[1] = 0; tail_hi[1] = t.right_rows; }
        PexTree const& tree = rs.tree_ref();
        seen.clear();
        for (u32 ai : S.exec_order[r]) {
            AnchorState const& a = A[ai];
            flx_pex_node const* node = &tree.leaves[a.leaf];
            if (node->parent_id == FLX_NULL_ID) continue;                                        // a tree of one node: the leaf is the root
            auto inside = [&](flx_pex_node const& nd) {
                u32 const f = a.orientation ? len - 1 - nd.to : nd.from, e = (a.orientation ? len - 1 - nd.from : nd.to) + 1;
                return (tail_lo[0] < tail_hi[0] && f >= tail_lo[0] && e <= tail_hi[0]) || (tail_lo[1] < tail_hi[1] && f >= tail_lo[1] && e <= tail_hi[1]);
            };
            if (!inside(*node)) continue;
            if (!P->direct_full_verification) {
                if (a.alive && !a.at_root) { set_error("split tails: an anchor neither failed nor reached the root"); return FLX_ERR_INTERNAL; }
                // upwards over the nodes it passed (those below a.node: the node it failed at, or the root) while they stay inside the tail
                u32 guard = 0;
                for (u32 up = node->parent_id; up != a.node; up = node->parent_id) {
                    if (up == FLX_NULL_ID || ++guard > tree.inner.size()) { set_error("split tails: an anchor's node is not on its path"); return FLX_ERR_INTERNAL; }
                    if (!inside(tree.inner[up])) break;
                    node = &tree.inner[up];
                }
            }
            if (node->to - node->from + 1 < min_span) continue;
            Span wsp;
            AlignRequest const req = window_request(S, H, a, *node, 0.0, &wsp);
            if (!seen.emplace(std::make_tuple(req.q_off, req.m, req.k, req.ref_off, req.n), 0u).second) continue;
            cands.push_back(Candidate{a.orientation, a.ref_id, *node, wsp});
            cand_req.push_back((u32)reqs.size());
            reqs.push_back(req);
        }
        sp.cand_end = (u32)cands.size();
        splits.push_back(sp);
    }
    if (splits.empty()) return FLX_OK;
    hvec<TraceResult> tres;
    if (int const rc = S.trace_windows(lane, RD, reqs, tres)) return rc;
    std::vector<flx_partial_candidate> pc;
    std::vector<int32_t> flags;
    std::vector<u8> quality;
    PartialScratch scratch;
    for (Split const& sp : splits) {
        ReadState const& rs = reads[sp.read];
        RootAlignment const& pr = root_res[sp.root];
        AnchorState const& pa = A[S.root_anchor[sp.root]];
        DevTailOut const& t = pr.tail;
        u32 const len = rs.len, o_from = t.left_rows, o_to = len - 1 - t.right_rows;
        TraceResult const& kt = tres[sp.req];
        if (!kt.exists) { set_error("split tails: no alignment over the kept part of a path"); return FLX_ERR_INTERNAL; }
        auto const clipped = append_clipped(S.cig, o_from, kt.cigar_off, kt.cigar_len, len - 1 - o_to);
        u32 const q_from = pa.orientation ? len - 1 - o_to : o_from, q_to = pa.orientation ? len - 1 - o_from : o_to;
        PartialRecord kept{sp.read, pa.orientation ? 16u : 0u, pa.ref_id, pr.start + t.left_cols + kt.begin, kt.nm, clipped.first, clipped.second, kt.md_off, kt.md_len,
                           q_from, q_to, 0, o_from, o_to, kt.cigar_off, kt.cigar_len};
        kept.split = true;
        kept.cs_off = kt.cs_off; kept.cs_len = kt.cs_len;
        S.partials.push_back(kept);
        // the supplementaries: choose_partials over the tail candidates
        pc.clear();
        for (u32 c = sp.cand_first; c < sp.cand_end; ++c) {
            TraceResult const& ct = tres[cand_req[c]];
            if (!ct.exists) { set_error("split tails: no alignment in a window that verification passed"); return FLX_ERR_INTERNAL; }
            flx_pex_node const& nd = cands[c].node;
            u32 const f = cands[c].orientation ? len - 1 - nd.to : nd.from, e = cands[c].orientation ? len - 1 - nd.from : nd.to;
            pc.push_back(flx_partial_candidate{rs.read_index, f, e, cands[c].orientation, (int32_t)cands[c].ref_id, cands[c].span.offset + ct.begin, ct.nm, ct.cigar_len, ct.cigar_off});
        }
        if (pc.empty() || max_records < 2) continue;
        flags.resize(pc.size());
        choose_partials(pc.data(), pc.size(), max_records - 1, S.cig.data(), flags.data(), scratch);
        quality.assign(pc.size(), 0);
        if (R.output.mapq) partial_mapq(pc.data(), pc.size(), S.cig.data(), flags.data(), quality.data(), scratch);
        std::vector<uint32_t> order(scratch.kept);
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return pc[x].q_from < pc[y].q_from; });
        for (u32 j : order) {
            u32 const c = sp.cand_first + j;
            flx_pex_node const& nd = cands[c].node;
            TraceResult const& ct = tres[cand_req[c]];
            auto const cl = append_clipped(S.cig, nd.from, ct.cigar_off, ct.cigar_len, len - 1 - nd.to);
            PartialRecord sup{sp.read, 2048u | (cands[c].orientation ? 16u : 0u), cands[c].ref_id, pc[j].start, ct.nm, cl.first, cl.second, ct.md_off, ct.md_len,
                              pc[j].q_from, pc[j].q_to, quality[j], nd.from, nd.to, ct.cigar_off, ct.cigar_len};
            sup.split = true;
            sup.cs_off = ct.cs_off; sup.cs_len = ct.cs_len;
            S.partials.push_back(sup);
        }
    }
    return FLX_OK;
}

// ---- 8. partial alignments of the reads that would be written as unmapped (flx_partial.hpp): every anchor's highest passed node,
//      traced in the window it was tested in; does nothing, and launches nothing, when the option is off or no read is eligible
int rescue_partials(Slice& S, Lane* lane, const flx_params* P, RunOptions const& R, const flx_reads* RD) {
    if (!R.partial.enable) return FLX_OK;
    HostIndex const& H = *lane->ctx->hidx;
    hvec<ReadState> const& reads = S.reads;
    hvec<AnchorState> const& A = S.A;
    hvec<u8> mapped(reads.size(), 0);
    for (u32 i = 0; i < S.root_anchor.size(); ++i) if (S.root_res[i].exists) mapped[A[S.root_anchor[i]].read] = 1;
    u32 const min_span = partial_min_span(&R.partial), max_records = partial_max_records(&R.partial);
    // ---- candidates, read by read in verification order; identical (orientation, node, reference, window) ones are one
    struct Candidate { u32 read; u8 orientation; u32 ref_id; flx_pex_node node; Span span; };
    hvec<Candidate> cands;
    hvec<AlignRequest> reqs;
    hvec<u32> read_first(reads.size() + 1, 0);
    std::map<std::tuple<u64, u32, u32, u64, u32>, u32> seen;
    for (size_t r = 0; r < reads.size(); ++r) {
        read_first[r] = (u32)cands.size();
        if (mapped[r]) continue;
        PexTree const& tree = reads[r].tree_ref();
        seen.clear();
        for (u32 ai : S.exec_order[r]) {
            AnchorState const& a = A[ai];
            flx_pex_node const* node = &tree.leaves[a.leaf];
            if (node->parent_id == FLX_NULL_ID) continue;                                        // a tree of one node: the leaf is the root
            if (!P->direct_full_verification) {
                if (a.alive && !a.at_root) { set_error("partial alignments: an anchor neither failed nor reached the root"); return FLX_ERR_INTERNAL; }
                // the child of a.node (the node it failed at, or the root) on the anchor's path
                u32 guard = 0;
                for (u32 up = node->parent_id; up != a.node; up = node->parent_id) {
                    if (up == FLX_NULL_ID || ++guard > tree.inner.size()) { set_error("partial alignments: an anchor's node is not on its path"); return FLX_ERR_INTERNAL; }
                    node = &tree.inner[up];
                }
            }
            if (node->to - node->from + 1 < min_span) continue;
            Span sp;
            AlignRequest const req = window_request(S, H, a, *node, 0.0, &sp);
            if (!seen.emplace(std::make_tuple(req.q_off, req.m, req.k, req.ref_off, req.n), 0u).second) continue;
            cands.push_back(Candidate{(u32)r, a.orientation, a.ref_id, *node, sp});
            reqs.push_back(req);
        }
    }
    read_first[reads.size()] = (u32)cands.size();
    if (cands.empty()) return FLX_OK;
    hvec<TraceResult> tres;
    if (int const rc = S.trace_windows(lane, RD, reqs, tres)) return rc;
    // ---- selection per read, and the kept records with their clips
    std::vector<flx_partial_candidate> pc;
    std::vector<int32_t> flags;
    std::vector<u8> quality;
    PartialScratch scratch;
    bool const mapq = R.output.mapq;
    for (size_t r = 0; r < reads.size(); ++r) {
        u32 const c0 = read_first[r], c1 = read_first[r + 1];
        if (c0 == c1) continue;
        u32 const len = reads[r].len;
        pc.clear();
        for (u32 c = c0; c < c1; ++c) {
            if (!tres[c].exists) { set_error("partial alignments: no alignment in a window that verification passed"); return FLX_ERR_INTERNAL; }
            flx_pex_node const& nd = cands[c].node;
            u32 const q_from = cands[c].orientation ? len - 1 - nd.to : nd.from, q_to = cands[c].orientation ? len - 1 - nd.from : nd.to;
            pc.push_back(flx_partial_candidate{reads[r].read_index, q_from, q_to, cands[c].orientation, (int32_t)cands[c].ref_id,
                                               cands[c].span.offset + tres[c].begin, tres[c].nm, tres[c].cigar_len, tres[c].cigar_off});
        }
        flags.resize(pc.size());
        choose_partials(pc.data(), pc.size(), max_records, S.cig.data(), flags.data(), scratch);
        quality.assign(pc.size(), 0);
        if (mapq) partial_mapq(pc.data(), pc.size(), S.cig.data(), flags.data(), quality.data(), scratch);
        for (u32 j : scratch.kept) {
            u32 const c = c0 + j;
            flx_pex_node const& nd = cands[c].node;
            auto const clipped = append_clipped(S.cig, nd.from, tres[c].cigar_off, tres[c].cigar_len, len - 1 - nd.to);
            S.partials.push_back(PartialRecord{(u32)r, (u32)flags[j], cands[c].ref_id, pc[j].start, tres[c].nm, clipped.first, clipped.second, tres[c].md_off,
                                               tres[c].md_len, pc[j].q_from, pc[j].q_to, quality[j], nd.from, nd.to, tres[c].cigar_off, tres[c].cigar_len});
            S.partials.back().cs_off = tres[c].cs_off;
            S.partials.back().cs_len = tres[c].cs_len;
        }
    }
    // (split_tails has left its records in front of these: read by read again, a read's records in the order they were made in)
    if (R.split.enable) std::stable_sort(S.partials.begin(), S.partials.end(), [](PartialRecord const& x, PartialRecord const& y) { return x.read < y.read; });
    return FLX_OK;
}

// ---- 8b. the kept partial records' ends extended to the break (flx_extend_options; the rule: flx_partial.hpp): one ed_extend launch
//      over both ends of every kept record of the slice, then one trace of the records that moved; does nothing, and launches nothing,
//      when the option is off or no record is kept
int extend_partials(Slice& S, Lane* lane, RunOptions const& R, const flx_reads* RD) {
    flx_extend_options const& EO = R.extend;
    if (!EO.enable || S.partials.empty()) return FLX_OK;
    HostIndex const& H = *lane->ctx->hidx;
    u32 const w = extend_weight(EO.error_weight), x_drop = extend_x_drop(EO.x_drop), d_max = extend_max_errors(EO.max_errors);
    struct End { u32 record; bool right; };
    hvec<DevExtendJob> jobs;
    hvec<End> ends;
    hvec<u64> spans(S.partials.size());
    for (size_t p0 = 0; p0 < S.partials.size();) {
        size_t p1 = p0;
        while (p1 < S.partials.size() && S.partials[p1].read == S.partials[p0].read) ++p1;
        ReadState const& rs = S.reads[S.partials[p0].read];
        for (size_t i = p0; i < p1; ++i) {
            PartialRecord const& p = S.partials[i];
            // rows free on either side in forward coordinates: up to the read's end, or to the nearest kept record's node interval
            u32 fwd_left = p.q_from, fwd_right = rs.len - 1 - p.q_to;
            for (size_t j = p0; j < p1; ++j) {
                PartialRecord const& o = S.partials[j];
                if (j == i) continue;
                if (o.q_to < p.q_from) fwd_left = std::min(fwd_left, p.q_from - 1 - o.q_to);
                else if (o.q_from > p.q_to) fwd_right = std::min(fwd_right, o.q_from - 1 - p.q_to);
            }
            bool const rc_strand = (p.flag & 16u) != 0;
            u32 const rows_right = rc_strand ? fwd_left : fwd_right, rows_left = rc_strand ? fwd_right : fwd_left;
            u64 const span = spans[i] = cigar_reference_span(S.cig.data() + p.core_off, p.core_len);
            u64 const seq_start = H.seq_start[p.ref_id], seq_len = H.seq_len[p.ref_id], q_base = rs.pool_off[rc_strand ? 1 : 0];
            u64 const cols_right = seq_len - std::min(seq_len, p.start + span), cols_left = p.start;
            if (rows_right && cols_right) {
                jobs.push_back(DevExtendJob{seq_start + p.start + span, q_base + p.o_to + 1, (u32)std::min<u64>(cols_right, 0x7FFFFFFFu), rows_right, 1, w, x_drop, d_max, 0, 0});
                ends.push_back(End{(u32)i, true});
            }
            if (rows_left && cols_left) {
                jobs.push_back(DevExtendJob{seq_start + p.start - 1, q_base + p.o_from - 1, (u32)std::min<u64>(cols_left, 0x7FFFFFFFu), rows_left, -1, w, x_drop, d_max, 0, 0});
                ends.push_back(End{(u32)i, false});
            }
        }
        p0 = p1;
    }
    hvec<DevExtendOut> outs;
    int rc;
    if ((rc = run_extend_jobs(lane, lane->ctx->didx.text, RD->d_pool.as<u8>(), jobs, outs))) return rc;
    // ---- the records that moved, traced again over exactly the longer interval
    struct Move { u32 rows[2] = {0, 0}, cols[2] = {0, 0}, errors[2] = {0, 0}; };      // [0] left, [1] right
    hvec<Move> moves(S.partials.size());
    for (size_t e = 0; e < ends.size(); ++e) {
        if (outs[e].rows == 0) continue;
        Move& m = moves[ends[e].record];
        int const side = ends[e].right ? 1 : 0;
        m.rows[side] = outs[e].rows; m.cols[side] = outs[e].cols; m.errors[side] = outs[e].errors;
    }
    hvec<AlignRequest> reqs;
    hvec<u32> req_record;
    for (size_t i = 0; i < S.partials.size(); ++i) {
        Move const& m = moves[i];
        if (!m.rows[0] && !m.rows[1]) continue;
        PartialRecord const& p = S.partials[i];
        ReadState const& rs = S.reads[p.read];
        reqs.push_back(AlignRequest{H.seq_start[p.ref_id] + p.start - m.cols[0], rs.pool_off[(p.flag & 16u) ? 1 : 0] + p.o_from - m.rows[0],
                                    (u32)(spans[i] + m.cols[0] + m.cols[1]), p.o_to - p.o_from + 1 + m.rows[0] + m.rows[1], p.nm + m.errors[0] + m.errors[1]});
        req_record.push_back((u32)i);
    }
    if (reqs.empty()) return FLX_OK;
    hvec<TraceResult> tres;
    if ((rc = S.trace_windows(lane, RD, reqs, tres))) return rc;
    for (size_t j = 0; j < reqs.size(); ++j) {
        if (!tres[j].exists) { set_error("partial extension: no alignment over an interval the extension reached"); return FLX_ERR_INTERNAL; }
        PartialRecord& p = S.partials[req_record[j]];
        Move const& m = moves[req_record[j]];
        u32 const len = S.reads[p.read].len;
        p.o_from -= m.rows[0];
        p.o_to += m.rows[1];
        if (p.flag & 16u) { p.q_from -= m.rows[1]; p.q_to += m.rows[0]; }
        else { p.q_from -= m.rows[0]; p.q_to += m.rows[1]; }
        p.start = p.start - m.cols[0] + tres[j].begin;
        p.nm = tres[j].nm;
        p.core_off = tres[j].cigar_off;
        p.core_len = tres[j].cigar_len;
        p.md_off = tres[j].md_off;
        p.md_len = tres[j].md_len;
        p.cs_off = tres[j].cs_off;
        p.cs_len = tres[j].cs_len;
        std::tie(p.cigar_off, p.cigar_len) = append_clipped(S.cig, p.o_from, p.core_off, p.core_len, len - 1 - p.o_to);
    }
    return FLX_OK;
}

// the CIGAR words of the kept records only: records that shared (or overlapped in) words before share them afterwards
void compact_cigars(flx_run* run, hvec<u32>& cig) {
    hvec<u32> order;
    for (u32 j = 0; j < run->records.size(); ++j) {
        if (run->records[j].cigar_length) order.push_back(j);
        else run->records[j].cigar_offset = 0;
    }
    std::sort(order.begin(), order.end(), [&](u32 a, u32 b) { return run->records[a].cigar_offset < run->records[b].cigar_offset; });
    hvec<u32> kept_words;
    u64 seg_start = 0, seg_end = 0, seg_base = 0;
    for (u32 j : order) {
        flx_record& rec = run->records[j];
        u64 const off = rec.cigar_offset, end = off + rec.cigar_length;
        if (kept_words.empty() || off >= seg_end) {
            seg_start = off; seg_end = end; seg_base = kept_words.size();
            kept_words.insert(kept_words.end(), cig.begin() + (long)off, cig.begin() + (long)end);
        } else if (end > seg_end) {
            kept_words.insert(kept_words.end(), cig.begin() + (long)seg_end, cig.begin() + (long)end);
            seg_end = end;
        }
        rec.cigar_offset = seg_base + (off - seg_start);
    }
    cig.swap(kept_words);
}

// ---- 9. records (alignment.cpp:37-79, output.cpp:49-108): per reference in id order, alignments in verification order
void write_records(Slice& S, flx_ctx* ctx, RunOptions const& R, u64 n_slice_reads, flx_run* run) {
    flx_output_options const& O = R.output;
    HostIndex const& H = *ctx->hidx;
    hvec<ReadState> const& reads = S.reads;
    hvec<AnchorState> const& A = S.A;
    hvec<u32> const& root_anchor = S.root_anchor;
    hvec<RootAlignment> const& root_res = S.root_res;
    hvec<u32>& cig = S.cig;
    Stats* const st_local = S.st_local.get();
    hvec<hvec<u32>> roots_of_read(reads.size());
    for (u32 i = 0; i < root_anchor.size(); ++i) roots_of_read[A[root_anchor[i]].read].push_back(i);   // already in verification order
    // output options (flx_select.hpp): a read's records are selected once they are formed and its statistics are taken
    bool const select = output_options_active(&O);
    u64 n_dropped = 0;
    std::vector<SelectKey> sel_keys;
    std::vector<u8> sel_keep;
    SelectScratch sel_scratch;
    // mapping quality (flx_mapq.hpp): from all of a read's records, before any of them is dropped
    bool const mapq = O.mapq;
    std::vector<MapqKey> mq_keys;
    std::vector<u8> mq_q;
    MapqScratch mq_scratch;
    // MD (flx_tag_options.md): one {offset, length} per record, parallel to run->records; the selection moves it with the records it keeps
    bool const md = S.want_md;
    run->has_md = md;
    // cs (flx_cs_options.form): the same, parallel to run->records
    bool const cs = S.cs_form != 0;
    run->has_cs = cs;
    size_t next_partial = 0;
    u64 n_partial_records = 0, n_rescued = 0, n_split = 0;
    for (size_t r = 0; r < reads.size(); ++r) {
        size_t const rec0 = run->records.size();
        bool have_best = false;
        u32 best = 0;
        for (u32 i : roots_of_read[r]) if (root_res[i].exists && (!have_best || root_res[i].nm < best)) { best = root_res[i].nm; have_best = true; }
        bool primary_written = false;
        for (u32 ref = 0; ref < H.seq_len.size(); ++ref)
            for (u32 i : roots_of_read[r]) {
                AnchorState const& a = A[root_anchor[i]];
                if (a.ref_id != ref || !root_res[i].exists) continue;
                u32 flag = a.orientation ? 16u : 0u;
                bool const primary = !primary_written && root_res[i].nm == best;
                if (primary) primary_written = true;
                else flag |= 256u;
                run->records.push_back(flx_record{reads[r].read_index, flag, (int32_t)ref, saturate_i32(root_res[i].start), root_res[i].nm,
                                                  root_res[i].cigar_off, root_res[i].cigar_len, 0});
                if (md) run->md_refs.push_back(flx_md_ref{root_res[i].md_off, root_res[i].md_len, 0});
                if (cs) run->cs_refs.push_back(flx_md_ref{root_res[i].cs_off, root_res[i].cs_len, 0});
                if (mapq) {
                    if (mq_keys.empty()) mq_scratch.spans.clear();
                    u64 const span = root_res[i].cigar_len ? cigar_reference_span_cached(cig.data() + root_res[i].cigar_off, root_res[i].cigar_len, mq_scratch)
                                                           : reads[r].len;
                    mq_keys.push_back(MapqKey{root_res[i].start, span, (int32_t)ref, flag, root_res[i].nm});
                }
            }
        bool const rescued = next_partial < S.partials.size() && S.partials[next_partial].read == r;
        bool const split = rescued && S.partials[next_partial].split;
        u32 split_mapq = 0;
        if (split) {
            // a split read's partial records are written instead of its root records; with -Q its primary keeps their value
            if (mapq && !mq_keys.empty()) {
                mq_q.resize(mq_keys.size());
                read_mapq(mq_keys.data(), mq_keys.size(), mq_q.data(), mq_scratch);
                for (size_t j = 0; j < mq_keys.size(); ++j) if (!(mq_keys[j].flag & 256u)) split_mapq = mq_q[j];
                mq_keys.clear();
            }
            n_dropped += run->records.size() - rec0;
            run->records.resize(rec0);
            if (md) run->md_refs.resize(rec0);
            if (cs) run->cs_refs.resize(rec0);
        }
        if (rescued) {                                           // (a read without a mapped record, or a split one)
            for (; next_partial < S.partials.size() && S.partials[next_partial].read == r; ++next_partial) {
                PartialRecord const& p = S.partials[next_partial];
                run->records.push_back(flx_record{reads[r].read_index, p.flag, (int32_t)p.ref_id, saturate_i32(p.start), p.nm, p.cigar_off, p.cigar_len,
                                                  split && !(p.flag & 2048u) ? split_mapq : p.mapq});
                if (md) run->md_refs.push_back(flx_md_ref{p.md_off, p.md_len, 0});
                if (cs) run->cs_refs.push_back(flx_md_ref{p.cs_off, p.cs_len, 0});
                ++n_partial_records;
            }
            if (split) ++n_split; else ++n_rescued;
        } else if (!primary_written) {
            run->records.push_back(flx_record{reads[r].read_index, 4u, -1, 0, 0, 0, 0, 0});
            if (md) run->md_refs.push_back(flx_md_ref{0, 0, 0});
            if (cs) run->cs_refs.push_back(flx_md_ref{0, 0, 0});
        }
        if (mapq && !mq_keys.empty()) {
            mq_q.resize(mq_keys.size());
            read_mapq(mq_keys.data(), mq_keys.size(), mq_q.data(), mq_scratch);
            for (size_t j = 0; j < mq_keys.size(); ++j) run->records[rec0 + j].reserved = mq_q[j];
            mq_keys.clear();
        }
        if (select && !rescued && run->records.size() - rec0 > 1) {
            // (records in the loop's order: the read's mapped roots by reference, the start key unsaturated)
            size_t const n = run->records.size() - rec0;
            sel_keys.clear();
            for (u32 ref = 0; ref < H.seq_len.size(); ++ref)
                for (u32 i : roots_of_read[r]) {
                    if (A[root_anchor[i]].ref_id != ref || !root_res[i].exists) continue;
                    flx_record const& rec = run->records[rec0 + sel_keys.size()];
                    sel_keys.push_back(SelectKey{root_res[i].start, rec.reference_id, rec.flag, rec.num_errors, rec.cigar_length,
                                                 rec.cigar_length ? cig.data() + rec.cigar_offset : nullptr});
                }
            sel_keep.resize(n);
            select_read_records(sel_keys.data(), n, O.drop_duplicates != 0, O.max_alignments_per_read, sel_keep.data(), sel_scratch);
            size_t w = rec0;
            for (size_t j = 0; j < n; ++j)
                if (sel_keep[j]) {
                    if (md) run->md_refs[w] = run->md_refs[rec0 + j];
                    if (cs) run->cs_refs[w] = run->cs_refs[rec0 + j];
                    run->records[w++] = run->records[rec0 + j];
                }
            n_dropped += run->records.size() - w;
            run->records.resize(w);
            if (md) run->md_refs.resize(w);
            if (cs) run->cs_refs.resize(w);
        }
        if (st_local) {                                                                                  // parallelization.cpp:262-268
            u64 n_al = 0;
            for (u32 i : roots_of_read[r]) if (root_res[i].exists) { ++n_al; st_local->at(Stats::EDIT_DISTANCE).add(root_res[i].ed); }      // (what verification found: a realigned NM is not one)
            st_local->at(Stats::ALIGNMENTS_PER_QUERY).add(n_al);
        }
    }
    if (st_local) {
        double const total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - S.t_slice).count();
        for (size_t r = 0; r < reads.size(); ++r) st_local->at(Stats::MS_VERIFICATION).add((u64)((total_ms - S.search_ms) / (double)std::max<size_t>(1, reads.size())));
        stats_merge_locked(ctx->read_stats, *st_local);
    }
    if (select) compact_cigars(run, cig);
    run->cigars = std::move(cig);
    if (md) run->md = std::move(S.md);              // (not compacted under -D / -N: the dropped records' bytes stay, unreferenced)
    if (cs) run->cs = std::move(S.cs);              // (nor this pool)
    {
        u64 found = 0;
        for (auto const& rr : root_res) found += rr.exists;
        std::lock_guard<std::mutex> g(ctx->mu);
        flx_path_counters& pc = ctx->path;
        pc.inner_tests_requested += S.n_inner_requested; pc.root_alignments_requested += S.root_reqs.size(); pc.root_alignments_found += found;
        pc.records += run->records.size(); pc.reads += n_slice_reads; pc.reserved[0] += n_dropped;
        pc.reserved[1] += n_partial_records; pc.reserved[2] += n_rescued; pc.reserved[3] += n_split;
    }
}

}  // namespace

int align_slice(Lane* lane, const flx_params* P, RunOptions const& R, const flx_reads* RD, u64 first_read, u64 end_read, flx_run* run) {
    flx_ctx* ctx = lane->ctx;
    FLX_HIP(hipSetDevice(ctx->device));
    HostIndex const& H = *ctx->hidx;
    PhaseTimer prof;
    Slice S;
    S.want_md = R.tags.md;
    S.cs_form = R.cs.form;
    S.want_left_align = R.gaps.left_align != 0;
    RealignScores const realign = realign_scores(&R.realign);
    if (R.realign.enable) S.realign = &realign;
    int rc;
    if ((rc = plan_reads(S, P, RD, first_read, end_read, run))) return rc;
    if ((rc = plan_seeds(S, P, RD))) return rc;
    prof.mark("pex+seeds");
    if ((rc = search_seeds(S, lane, P, RD))) return rc;
    prof.mark("search");
    anchors_to_reads(S);
    verification_order(S, P);
    prof.mark("anchors+order");
    FLX_HIP(hipStreamWaitEvent(lane->stream, RD->peq_event, 0));      // the DP launches start behind the Peq planes of the whole pool
    u32 const n_climbing = start_climb(S, P);
    static int const host_rounds = getenv("FLX_HOST_ROUNDS") ? 1 : 0;
    ExistsTimes times;
    if (!host_rounds && !S.st_local && n_climbing) rc = climb_on_device(S, lane, RD);
    else rc = climb_on_host(S, lane, RD, times);
    if (rc) return rc;
    prof.mark("inner-levels");
    if (prof.on)
        fprintf(stderr, "[flx host profile] exists rounds: dedup=%.2f cluster=%.2f gpu-round-trip=%.2f scatter=%.2f build-requests=%.2f ms\n",
                times.ms[0], times.ms[1], times.ms[2], times.ms[3], times.build_requests);
    interval_pass(S, P, H);
    prof.mark("interval-pass");
    if ((rc = align_roots(S, lane, P, R, RD))) return rc;
    prof.mark("root-align");
    if ((rc = split_tails(S, lane, P, R, RD))) return rc;
    if (R.split.enable) prof.mark("split-tails");
    if ((rc = rescue_partials(S, lane, P, R, RD))) return rc;
    prof.mark("partials");
    if ((rc = extend_partials(S, lane, R, RD))) return rc;
    if (R.extend.enable) prof.mark("extend");
    write_records(S, ctx, R, end_read - first_read, run);
    prof.mark("records");
    return FLX_OK;
}

}  // namespace flx

// ---- the climb alone (flx_climb_anchors, include/floxer_amd.h): a test hook. plan_reads, the caller's anchors in place of
//      anchors_to_reads, start_climb and one of the two drivers, as align_slice calls them; nothing of a run's path is changed for it.
namespace {
// the Peq planes and the 2-bit form of the batch's pool, as the first flx_align_reads_resident call on the batch builds them
int climb_read_planes(flx_ctx* ctx, const flx_reads* RD) {
    using namespace flx;
    std::lock_guard<std::mutex> g(RD->peq_mu);
    if (RD->peq_built || !RD->n_reads) return FLX_OK;
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
    return FLX_OK;
}
}  // namespace

extern "C" int flx_climb_anchors(flx_ctx* ctx, const flx_params* P, const flx_reads* RD, const flx_climb_anchor* anchors, uint64_t n_anchors,
                                 const flx_climb_options* O, uint8_t* out_status, uint32_t* out_node, uint64_t* out_requests) {
    using namespace flx;
    if (!ctx || !P || !RD || RD->ctx != ctx || (n_anchors && (!anchors || !out_status || !out_node))) {
        set_error("flx_climb_anchors: null argument or reads of another context"); return FLX_ERR_INVALID;
    }
    if (O && (O->driver > 1 || O->reserved[0] || O->reserved[1] || O->reserved[2])) { set_error("flx_climb_anchors: unknown driver, or reserved options set"); return FLX_ERR_INVALID; }
    if (P->query_error_probability < 0 && P->query_num_errors < P->pex_seed_num_errors) { set_error("query errors must be >= seed errors (floxer_cli.cpp:180)"); return FLX_ERR_INVALID; }
    if (P->pex_seed_num_errors > 3) { set_error("invalid parameters"); return FLX_ERR_INVALID; }
    if (n_anchors >= (1ull << 31)) { set_error("flx_climb_anchors: too many anchors"); return FLX_ERR_INVALID; }
    if (out_requests) *out_requests = 0;
    FLX_HIP(hipSetDevice(ctx->device));
    HostIndex const& H = *ctx->hidx;
    Slice S;
    flx_run run;
    run.skipped.assign(RD->n_reads, 0);
    int rc;
    if ((rc = plan_reads(S, P, RD, 0, RD->n_reads, &run))) return rc;
    hvec<u32> kept_of(RD->n_reads, 0xFFFFFFFFu);
    for (size_t r = 0; r < S.reads.size(); ++r) kept_of[S.reads[r].read_index] = (u32)r;
    S.A.reserve(n_anchors);
    u64 prev_query = 0;
    for (u64 i = 0; i < n_anchors; ++i) {
        flx_climb_anchor const& in = anchors[i];
        if (in.read >= RD->n_reads || in.orientation > 1 || kept_of[in.read] == 0xFFFFFFFFu) { set_error("flx_climb_anchors: an anchor of no read, of a read the input rules skip, or of no orientation"); return FLX_ERR_INVALID; }
        u64 const query = 2ull * kept_of[in.read] + in.orientation;
        if (query < prev_query) { set_error("flx_climb_anchors: anchors out of (read, orientation) order"); return FLX_ERR_INVALID; }
        prev_query = query;
        PexTree const& tree = S.reads[kept_of[in.read]].tree_ref();
        if (in.leaf >= tree.leaves.size()) { set_error("flx_climb_anchors: a leaf outside the read's tree"); return FLX_ERR_INVALID; }
        if (in.reference_id >= H.seq_len.size()) { set_error("flx_climb_anchors: a reference outside the index"); return FLX_ERR_INVALID; }
        flx_pex_node const& leaf = tree.leaves[in.leaf];
        u64 const rows = leaf.to - leaf.from + 1;
        if (in.position >= H.seq_len[in.reference_id] || in.position + rows > H.seq_len[in.reference_id] + leaf.num_errors) {
            set_error("flx_climb_anchors: a position whose leaf does not lie inside the reference sequence"); return FLX_ERR_INVALID;
        }
        AnchorState a{};
        a.read = kept_of[in.read]; a.orientation = (u8)in.orientation; a.leaf = in.leaf; a.ref_id = in.reference_id; a.pos = in.position;
        a.node = FLX_NULL_ID;
        S.A.push_back(a);
    }
    if (n_anchors == 0) return FLX_OK;
    if ((rc = climb_read_planes(ctx, RD))) return rc;
    {
        LaneLease lease(ctx, ctx->external_stream ? 0 : -1);
        Lane* const lane = lease.lane;
        FLX_HIP(hipStreamWaitEvent(lane->stream, RD->peq_event, 0));
        u32 const n_climbing = start_climb(S, P);
        ExistsTimes times;
        if (O && O->driver == 1) rc = climb_on_host(S, lane, RD, times);
        else rc = n_climbing ? climb_on_device(S, lane, RD) : FLX_OK;
        if (rc) return rc;
    }
    for (u64 i = 0; i < n_anchors; ++i) {
        AnchorState const& a = S.A[i];
        if (a.alive && !a.at_root) { set_error("flx_climb_anchors: an anchor neither failed nor reached the root"); return FLX_ERR_INTERNAL; }
        out_status[i] = a.alive ? 1 : 0;
        out_node[i] = a.node;
    }
    if (out_requests) *out_requests = S.n_inner_requested;
    return FLX_OK;
}
