// Seeding on the device: the FM-index search of a chunk's seeds (K1/K2) and the anchor selection behind it (search.cpp:143-324),
// and the C ABI of seam 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <numeric>
#include <string>

#include "flx_fm_core.hpp"
#include "flx_pipeline.hpp"

namespace flx {

namespace {

struct Group { u32 lb, len, errors; };

bool anchor_better(u64 pos_a, u64 err_a, u64 pos_b, u64 err_b) {                         // search.cpp:38-44
    u64 const d = pos_a < pos_b ? pos_b - pos_a : pos_a - pos_b;
    return err_a <= err_b && d <= err_b - err_a;
}

constexpr u64 ERASED = ~0ull;
struct RefAnchor { u64 pos; u64 errors; };

// search.cpp:352-389 for one (seed, reference) bucket
void erase_useless(hvec<RefAnchor>& v) {
    if (v.empty()) return;
    std::sort(v.begin(), v.end(), [](RefAnchor const& a, RefAnchor const& b) { return a.pos < b.pos; });
    for (size_t cur = 0; cur + 1 < v.size();) {
        size_t other = cur + 1;
        while (other < v.size() && anchor_better(v[cur].pos, v[cur].errors, v[other].pos, v[other].errors)) {
            v[other].errors = ERASED;
            ++other;
        }
        if (other < v.size() && anchor_better(v[other].pos, v[other].errors, v[cur].pos, v[cur].errors)) v[cur].errors = ERASED;
        cur = other;
    }
    v.erase(std::remove_if(v.begin(), v.end(), [](RefAnchor const& a) { return a.errors == ERASED; }), v.end());
}

}  // namespace

int search_seeds_device(Lane* ctx, const u8* d_seq_pool_or_null, const u8* h_seq_pool, u64 pool_len, const flx_seed* seeds,
                        u64 n_seeds, const flx_search_config& cfg, hvec<HostAnchor>& anchors, hvec<SeedStats>& stats,
                        hvec<DevHit>* raw_hits, u64 raw_max_hits, const u32* d_qpack_or_null, const u8* seed_flags, const SeedGen* gen) {
    anchors.clear();
    if (gen) n_seeds = gen->n_seeds;
    stats.assign(n_seeds, SeedStats{0, 0, 0, 0});
    if (n_seeds == 0) return FLX_OK;
    if (n_seeds >= (1ull << 31)) { set_error("too many seeds in one call"); return FLX_ERR_INVALID; }
    HostIndex const& H = *ctx->ctx->hidx;
    PhaseTimer sprof("search");

    // ---- expanded schemes (search_scheme_cache, search.cpp:328-350), DFS stack reservations and the launch order
    // Launch order = expected cost, heaviest class first (more errors, then shorter): the work of a seed grows steeply with its
    // errors (k = 2 leaves of a 5-kb read cost 4x the k = 1 leaves), and what a wave still holds when the seed queue runs dry
    // is the tail of the kernel. Within a class the caller's order is kept. Hits carry the seed's id, not its launch position.
    // Two passes over the caller's seeds (a chunk of 10-kb reads has a million of them): classes and their sizes, then every DevSeed
    // written once, at its launch position.
    struct SeedClass { u32 scheme_off, frames_searches, count, next; };
    std::map<u32, SeedClass> classes;                                   // key: (3 - errors) << 24 | length -> heaviest first
    hvec<u64> scheme_table;
    u64 frames = 0;
    u32 max_errors = 0, max_length = 0;
    auto class_key = [](flx_seed const& s) { return ((3u - s.num_errors) << 24) | s.length; };
    if (gen) { scheme_table = gen->scheme_table; max_errors = gen->max_errors; max_length = gen->max_length; }
    else {
        u32 last = 0xFFFFFFFFu;
        SeedClass* slot = nullptr;                                      // consecutive seeds are mostly of one class
        for (u64 i = 0; i < n_seeds; ++i) {
            flx_seed const& s = seeds[i];
            if (s.num_errors > 3) { set_error("seed errors must be in [0,3] (floxer_cli.cpp:299)"); return FLX_ERR_INVALID; }
            if (s.length == 0 || s.length > SCH_POS_MASK || s.seq_offset + s.length > pool_len) { set_error("seed outside the sequence pool"); return FLX_ERR_INVALID; }
            u32 const key = class_key(s);
            if (key != last) {
                auto it = classes.find(key);
                if (it == classes.end()) {
                    auto const e = expanded_scheme(s.num_errors, s.length);
                    u32 const nsearch = e.empty() ? 0 : (u32)(e.size() / s.length);
                    it = classes.emplace(key, SeedClass{(u32)scheme_table.size(), (s.length + s.num_errors + 3) | (nsearch << 24), 0, 0}).first;
                    scheme_table.insert(scheme_table.end(), e.begin(), e.end());
                    max_errors = std::max(max_errors, s.num_errors);
                    max_length = std::max(max_length, s.length);
                }
                slot = &it->second;
                last = key;
            }
            ++slot->count;
        }
        u32 pos = 0;
        for (auto& kv : classes) { kv.second.next = pos; pos += kv.second.count; }
    }
    hvec<DevSeed> dseeds(gen ? 0 : n_seeds);
    // what a seed's symbols may be (SEED_* of flx_fm_core.hpp): given by the caller per seed, or read off the host pool
    auto flags_of = [&](u64 i) -> u32 {
        if (seed_flags) return seed_flags[i];
        if (!h_seq_pool) return SEED_HAS_DELIM | SEED_NOT_ACGT;
        u32 f = 0;
        const u8* p = h_seq_pool + seeds[i].seq_offset;
        for (u32 j = 0; j < seeds[i].length; ++j) { if (p[j] == 0) f |= SEED_HAS_DELIM; if (p[j] - 1u > 3u) f |= SEED_NOT_ACGT; }
        return f;
    };
    if (!gen) {
        u32 last = 0xFFFFFFFFu;
        SeedClass* slot = nullptr;
        for (u64 i = 0; i < n_seeds; ++i) {
            flx_seed const& s = seeds[i];
            u32 const key = class_key(s);
            if (key != last) { slot = &classes.find(key)->second; last = key; }
            DevSeed& d = dseeds[slot->next++];
            d.seq_off = s.seq_offset;
            d.length = s.length;
            d.scheme_off = slot->scheme_off;
            d.frames_searches = slot->frames_searches;
            d.stack_off = frames;                                       // (reserved in the caller's order: only the ordered walk uses it)
            d.id = (u32)i;
            d.flags = flags_of(i);
            d.pad = 0;
            frames += slot->frames_searches & 0xFFFFFFu;
        }
    }
    if (scheme_table.empty()) scheme_table.push_back(0);
    // most seeds longer than 64 symbols (20-kb reads at 2 %: leaves of 98 .. 147)? The text walk then takes its larger LDS windows.
    bool long_seeds = false;
    {
        u64 n_long = 0, n_all = 0;
        if (gen) { for (auto const& lf : gen->leaves) { n_long += lf.length > 64u; ++n_all; } }
        else for (u64 i = 0; i < n_seeds; ++i) { n_long += seeds[i].length > 64u; ++n_all; }
        long_seeds = 2 * n_long > n_all;
    }

    sprof.mark("prep");
    int rc;
    const u8* d_seq = d_seq_pool_or_null;
    if (!d_seq) {
        if ((rc = h2d(ctx, ctx->seq, h_seq_pool, pool_len, 64))) return rc;
        d_seq = ctx->seq.as<u8>();
    }
    const u64* d_scheme = nullptr;
    if (!gen) {
        if ((rc = h2d(ctx, ctx->scheme, scheme_table.data(), scheme_table.size() * 8))) return rc;
        d_scheme = ctx->scheme.as<u64>();
        if ((rc = h2d(ctx, ctx->seeds, dseeds.data(), dseeds.size() * sizeof(DevSeed)))) return rc;
    } else {
        // the chunk's description (a few hundred KB) and the scheme table up in one copy, packed in the lane's staging block; the DevSeeds
        // written where the search reads them
        size_t const b_reads = gen->reads.size() * sizeof(DevSeedRead), b_leaves = gen->leaves.size() * sizeof(DevSeedLeaf), b_classes = gen->classes.size() * sizeof(DevSeedClass),
                     b_scheme = scheme_table.size() * 8;
        auto const up = [](size_t b) { return (b + 255) / 256 * 256; };
        size_t const o_leaves = up(b_reads), o_classes = o_leaves + up(b_leaves), o_scheme = o_classes + up(b_classes), total = o_scheme + b_scheme;
        if ((rc = ctx->seed_gen.ensure(total + 256))) return rc;
        if ((rc = ctx->seeds.ensure(n_seeds * sizeof(DevSeed)))) return rc;
        char* const h = (char*)ctx->stage_begin(total);
        if (!h) return FLX_ERR_NO_DEVICE;
        memcpy(h, gen->reads.data(), b_reads);
        memcpy(h + o_leaves, gen->leaves.data(), b_leaves);
        memcpy(h + o_classes, gen->classes.data(), b_classes);
        memcpy(h + o_scheme, scheme_table.data(), b_scheme);
        char* const g = (char*)ctx->seed_gen.ptr;
        FLX_HIP(hipMemcpyAsync(g, h, total, hipMemcpyHostToDevice, ctx->stream));
        d_scheme = (const u64*)(g + o_scheme);
        int const e = DeviceApi::build_seeds(ctx->stream, (const DevSeedRead*)g, (u32)gen->reads.size(), (const DevSeedLeaf*)(g + o_leaves), (const DevSeedClass*)(g + o_classes),
                                             ctx->seeds.as<DevSeed>());
        if (e) { set_error(std::string("seed_build: ") + hipGetErrorString((hipError_t)e)); return FLX_ERR_NO_DEVICE; }
    }
    // The DFS in the reference's order (frames on a per-seed stack in HBM) where the order of discovery matters: the raw-emission
    // hook and first_reported, which want the first n rows; everywhere else the walk with its stack in LDS, whose hits carry keys
    // that restore the emission order.
    bool const ordered = (raw_hits && !getenv("FLX_FM_KEYED_RAW")) || cfg.anchor_choice_strategy == FLX_CHOICE_FIRST_REPORTED || max_length > fm_search_max_keyed_length() ||
                         max_errors > 3 || getenv("FLX_FM_ORDERED");      // (FLX_FM_ORDERED=1: the ordered walk for everything, for comparisons)
    if (ordered && (rc = ctx->stack.ensure(frames * sizeof(DevFrame)))) return rc;
    if ((rc = ctx->counters.ensure(128))) return rc;
    // the walk of flx_search.hip (presence filter, one-row subtrees against the text) unless the order of discovery matters
    bool const filtered = !ordered;
    const u32* d_qpack = d_qpack_or_null;
    if (filtered && !d_qpack && ctx->ctx->didx.filter) {
        if ((rc = ctx->qpack.ensure(pack_words_for(pool_len) * 4 + 64))) return rc;
        int const e = DeviceApi::pack_pool(ctx->stream, d_seq, pool_len, ctx->qpack.as<u32>());
        if (e) { set_error(std::string("pack_pool: ") + hipGetErrorString((hipError_t)e)); return FLX_ERR_NO_DEVICE; }
        d_qpack = ctx->qpack.as<u32>();
    }
    // (10-kb reads at 8 % on a random text: 6.3 one-row subtrees and 0.4 hits per seed; on a repeat-rich text several times that: what the
    // last search on this lane needed, and a quarter more, is the starting size; a search that outgrows its buffers runs again)
    u64 item_cap = filtered && ctx->ctx->didx.isa ? std::max<u64>(n_seeds * 8, (u64)(ctx->items_per_seed * 1.25 * (double)n_seeds)) + 4096 * 64 : 0;

    u32 const max_hits = raw_hits ? (u32)std::min<u64>(raw_max_hits, 0xFFFFFFF0u)
                                  : (cfg.anchor_choice_strategy == FLX_CHOICE_FIRST_REPORTED
                                         ? (u32)cfg.max_num_anchors_soft
                                         : (u32)std::max(cfg.max_num_anchors_hard, cfg.max_num_anchors_hard + 1));
    u64 const hit_slack = 4096 * 64;            // unused ends of the per-wave slot ranges (FM_MAX_WAVES x FM_HIT_GRAB)
    u64 hit_cap = std::max<u64>(n_seeds * 6, (u64)(ctx->hits_per_seed * 1.25 * (double)n_seeds)) + hit_slack;
    // Anchor selection on the device (K1b) for the default group order and anchor choice; seeds it does not handle come back
    // flagged and go through the host code below.
    bool const device_select = !raw_hits && cfg.anchor_group_order == FLX_ORDER_COUNT_FIRST && cfg.anchor_choice_strategy == FLX_CHOICE_ROUND_ROBIN &&
                               cfg.max_num_anchors_soft >= 1 && !getenv("FLX_HOST_SELECT");
    if (gen && (!device_select || ordered)) return SEARCH_NEEDS_HOST_SEEDS;      // (those paths read the seed list)
    size_t const scan_bytes = device_select ? DeviceApi::select_scan_bytes((u32)n_seeds) : 0;
    hvec<DevSelStat> sel_stat;                // per seed
    u32 sel_total = 0, sel_rows_total = 0;
    if (device_select) {
        if ((rc = ctx->seed_cnt.ensure((n_seeds + 1) * 4))) return rc;
        if ((rc = ctx->hit_off.ensure((n_seeds + 1) * 4))) return rc;
        if ((rc = ctx->sel_stat.ensure(n_seeds * sizeof(DevSelStat) + 16))) return rc;
        if ((rc = ctx->sel_n.ensure((n_seeds + 1) * 4))) return rc;
        if ((rc = ctx->sel_off.ensure((n_seeds + 1) * 4))) return rc;
        if ((rc = ctx->sel_rows.ensure((n_seeds + 1) * 4))) return rc;
        if ((rc = ctx->sel_row_off.ensure((n_seeds + 1) * 4))) return rc;
        if ((rc = ctx->sel_tmp.ensure(scan_bytes + 64))) return rc;
        if ((rc = ctx->sel_lists.ensure((3 * n_seeds + 3) * 4))) return rc;
        sel_stat.resize(n_seeds);
    }
    // the mailboxes through which the waves of a search launch hand subtrees to each other (at most 4096 waves per launch, 6 KB each)
    u32 const mailbox_waves = device_select ? 4096u : 0u;
    if (mailbox_waves && (rc = ctx->mailboxes.ensure(DeviceApi::mailbox_bytes(mailbox_waves)))) return rc;
    u32 counters[32];
    u64 sel_cap = (u64)(ctx->sel_rows_per_seed * 1.25 * (double)n_seeds);      // entries of the selected-anchor list (at least hit_cap, below)
    struct K1Token { flx_ctx* c; explicit K1Token(flx_ctx* c_) : c(c_) { c->k1_acquire(); } ~K1Token() { c->k1_release(); } };
    for (int attempt = 0;; ++attempt) {
        K1Token const token(ctx->ctx);           // (held until this attempt's kernels have finished)
        static int const alloc_debug = getenv("FLX_ALLOC_DEBUG") ? 1 : 0;
        sel_cap = std::max(sel_cap, hit_cap);
        if ((rc = ctx->hits.ensure(hit_cap * sizeof(DevHit)))) return rc;
        if (item_cap && (rc = ctx->items.ensure(item_cap * sizeof(DevHit)))) return rc;
        // what the stage's kernels want zeroed, in one clear_stage launch in front of the walk
        ClearList clears;
        clears.add(ctx->counters.ptr, 32);
        if (device_select) {
            // one selected anchor per hit row at most; rows <= hits * SEL_MAX would be the hard bound, the seeds the device
            // handles have at most soft-cap rows each and nearly all hits have one row: hit_cap entries, checked after the run
            if ((rc = ctx->grouped.ensure(hit_cap * sizeof(DevHit)))) return rc;
            if ((rc = ctx->sel_out.ensure(sel_cap * sizeof(DevOutAnchor)))) return rc;
            if ((rc = ctx->sel_sparse.ensure(sel_cap * sizeof(DevOutAnchor)))) return rc;
            // (the search counts a seed's rows here while it runs; seed_rows_kernel then writes every entry but the last)
            clears.add(ctx->sel_rows.ptr, n_seeds + 1);
            clears.add(ctx->seed_cnt.ptr, n_seeds + 1);
            clears.add(ctx->sel_n.as<u32>() + n_seeds, 1);
            clears.add(ctx->sel_lists.as<u32>() + 3 * n_seeds, 3);      // (the lengths of the selection's three seed lists)
        }
        if (alloc_debug) { dump_lane_buffers(*ctx, "search"); fprintf(stderr, "[flx alloc] lane %d search: seeds %llu hit_cap %llu item_cap %llu pool %p qpack %p\n", ctx->id, (unsigned long long)n_seeds, (unsigned long long)hit_cap, (unsigned long long)item_cap, (const void*)d_seq, (const void*)d_qpack); }
        rc = timed_launch(ctx, "fm_search", 0, n_seeds, [&] {
            u32 const concurrent = ctx->ctx->external_stream ? 1u : (u32)ctx->ctx->lanes.size();
            if (filtered)
                return DeviceApi::search_filtered(ctx->stream, ctx->ctx->didx, d_seq, d_qpack, d_scheme, ctx->seeds.as<DevSeed>(), (u32)n_seeds,
                                                  max_hits, max_errors, ctx->hits.as<DevHit>(), (u32)std::min<u64>(hit_cap, 0xFFFFFFFFu),
                                                  item_cap ? ctx->items.as<DevHit>() : nullptr, (u32)std::min<u64>(item_cap, 0xFFFFFFFFu),
                                                  ctx->counters.as<u32>(), device_select ? ctx->seed_cnt.as<u32>() : nullptr,
                                                  device_select ? ctx->sel_rows.as<u32>() : nullptr, device_select ? ctx->mailboxes.ptr : nullptr, mailbox_waves, concurrent, long_seeds, clears);
            if (int const e = DeviceApi::clear_stage(ctx->stream, clears)) return e;
            return DeviceApi::search(ctx->stream, ctx->ctx->didx, d_seq, d_scheme, ctx->seeds.as<DevSeed>(), (u32)n_seeds,
                                     max_hits, ctx->stack.as<DevFrame>(), ctx->hits.as<DevHit>(), (u32)std::min<u64>(hit_cap, 0xFFFFFFFFu),
                                     ctx->counters.as<u32>(), device_select ? ctx->seed_cnt.as<u32>() : nullptr);
        });
        if (rc) return rc;
        if (device_select) {
            rc = timed_launch(ctx, "fm_select", n_seeds * 5, n_seeds, [&] {
                return DeviceApi::select(ctx->stream, ctx->hits.as<DevHit>(), ctx->counters.as<u32>(), (u32)std::min<u64>(hit_cap, 0xFFFFFFFFu),
                                         ctx->seed_cnt.as<u32>(), ctx->hit_off.as<u32>(), ctx->grouped.as<DevHit>(), (u32)n_seeds, ctx->ctx->didx,
                                         ctx->ctx->seq_start.as<u64>(), (u32)H.seq_start.size(), (u32)std::min<u64>(cfg.max_num_anchors_hard, 0xFFFFFFFFu),
                                         (u32)std::min<u64>(cfg.max_num_anchors_soft, 0xFFFFFFFFu), cfg.erase_useless_anchors != 0, ctx->sel_stat.ptr,
                                         ctx->sel_n.as<u32>(), ctx->sel_off.as<u32>(), ctx->sel_out.as<DevOutAnchor>(), (u32)std::min<u64>(sel_cap, 0xFFFFFFFFu),
                                         ctx->sel_rows.as<u32>(), ctx->sel_row_off.as<u32>(), ctx->sel_sparse.as<DevOutAnchor>(),
                                         (u32)std::min<u64>(sel_cap, 0xFFFFFFFFu), ctx->sel_tmp.ptr, scan_bytes, ctx->sel_lists.as<u32>());
            });
            if (rc) return rc;
        }
        // the counters and the selection's two totals come back through the lane's mapped result block: one publish_stage launch behind the
        // stage's kernels, read after the stream wait (a copy each when the block has no room)
        ResultScope const scope(ctx);
        u32* const r_small = (u32*)ctx->result_slot(34 * 4);
        if (r_small) {
            PublishList pub;
            pub.add(ctx->counters.ptr, r_small, 32);
            if (device_select) {
                pub.add(ctx->sel_off.as<u32>() + n_seeds, r_small + 32, 1);
                pub.add(ctx->sel_row_off.as<u32>() + n_seeds, r_small + 33, 1);
            }
            int const e = DeviceApi::publish_stage(ctx->stream, pub);
            if (e) { set_error(std::string("publish_stage: ") + hipGetErrorString((hipError_t)e)); return FLX_ERR_NO_DEVICE; }
        } else {
            if ((rc = d2h(ctx, counters, ctx->counters.ptr, 128))) return rc;
            if (device_select) {
                if ((rc = d2h(ctx, &sel_total, (char*)ctx->sel_off.ptr + n_seeds * 4, 4))) return rc;
                if ((rc = d2h(ctx, &sel_rows_total, (char*)ctx->sel_row_off.ptr + n_seeds * 4, 4))) return rc;
            }
        }
        if (device_select && (rc = d2h(ctx, sel_stat.data(), ctx->sel_stat.ptr, n_seeds * sizeof(DevSelStat)))) return rc;
        if ((rc = ctx->sync())) return rc;
        if (r_small) {
            memcpy(counters, r_small, 128);
            if (device_select) { sel_total = r_small[32]; sel_rows_total = r_small[33]; }
        }
        if (getenv("FLX_SEARCH_DEBUG")) fprintf(stderr, "[fm_search] seeds %llu ext %u (of single-row intervals %u) wave-iterations %u (max per wave %u) busy pair-iterations %u, after the queue ran dry %u (max %u), subtrees handed over %u, from wave to wave %u, walks abandoned over the cap %u\n", (unsigned long long)n_seeds, counters[2], counters[3], counters[4], counters[5], counters[6], counters[8], counters[9], counters[14], counters[15], counters[20]);
        if (getenv("FLX_SEARCH_DEBUG") && filtered) fprintf(stderr, "[fm_search filtered] subtrees queued %u (slots %u of %llu), filter words asked %u, children dropped %u, searches ended by the prefix lookup %u; text walk: lane-steps %u, wave-iterations %u in %u waves (longest %u)\n", counters[3], counters[16], (unsigned long long)item_cap, counters[10], counters[11], counters[12], counters[18], counters[19], counters[22], counters[21]);
        if (counters[1]) { set_error(counters[1] & 2u ? "fm_search: a subtree handed between waves was not taken" : "fm_search: DFS stack reservation exceeded"); return FLX_ERR_INTERNAL; }
        bool const items_fit = !item_cap || counters[16] <= item_cap;
        bool const fits = items_fit && counters[0] <= hit_cap && (!device_select || sel_rows_total <= sel_cap);      // (selected anchors <= rows)
        if (!fits && attempt >= 3) { set_error("fm_search: hit buffer could not be sized"); return FLX_ERR_INTERNAL; }
        {
            // what this launch's work sharing did (flx_search_counters), and the launch repeated when its buffers were outgrown
            std::lock_guard<std::mutex> g(ctx->ctx->mu);
            flx_search_counters& sc = ctx->ctx->search;
            ++sc.launches;
            if (filtered) { sc.subtrees_queued += counters[3]; sc.lane_handovers += counters[14]; sc.wave_handovers += counters[15]; sc.walks_abandoned += counters[20]; }
            if (!fits) ++ctx->ctx->path.search_reruns;
        }
        if (fits) break;
        // (a wave reserves 64 slots at a time and leaves the rest of a range unused when a ballot's records do not fit into it: the slots
        // reserved are at most twice the records written plus one range per wave of both kernels, however the waves were scheduled)
        u64 const wave_ranges = (u64)(4096 + 8192 + 64) * 64;
        if (!items_fit) item_cap = std::max<u64>((u64)counters[16], 2 * (u64)counters[3]) + wave_ranges;      // queued subtrees were dropped: run again with room for all
        else if (counters[0] > hit_cap) hit_cap = std::max<u64>((u64)counters[0], 2 * (u64)counters[13]) + wave_ranges;      // the number of hits is known now; run again
        else sel_cap = (u64)sel_rows_total + 1024;
    }
    // The kernel's accounting: the bytes THIS walk has to touch, from its own device counters (work units = rank pairs). Random accesses
    // count at the 64-B size the memory system fetches them in; records that stream count at their size:
    //   rank pair                2 x 64 B   (a 32-B block at either end of the interval; both ends in one block still count twice)
    //   filter lookup            64 B       (one 64-bit word of the presence table)
    //   queued one-row subtree   24 B written + 24 B read (the record) + 64 B (SA[row]) + 64 B (the text next to it) + 64 B (its seed's record)
    //   hit                      24 B written; a hit of the text walk reads ISA[position] (64 B): charged for every hit
    //   seed                     40 B (its record) + 64 B (its symbols) + 64 B (their 2-bit form, filter walk only)
    // The ordered walk (no filter, no text walk) prices its rank pairs and its 64-B frames written and read back.
    // SURVEY.md 8(d)'s figure - 128 B per cursor extension of the REFERENCE's walk - is computed by bench.py from the oracle's count and
    // reported beside this one; it is not a fraction of the HBM peak for a walk that answers with fewer rank queries.
    if (ctx->ctx->timing) {
        u64 bytes = (u64)counters[2] * 128;
        if (filtered) bytes += (u64)counters[10] * 64 + (u64)counters[3] * (24 + 24 + 64 + 64 + 64) + (u64)counters[13] * (24 + 64) + n_seeds * (u64)(40 + 64 + (d_qpack ? 64 : 0));
        else bytes += (u64)counters[2] * 128 + n_seeds * (u64)(40 + 64);
        std::lock_guard<std::mutex> g(ctx->ctx->mu);
        auto it = ctx->ctx->stats.find("fm_search");
        if (it != ctx->ctx->stats.end()) { it->second.algorithmic_bytes += bytes; it->second.work_units += counters[2]; }
    }
    ctx->hits_per_seed = (double)counters[0] / (double)n_seeds;
    ctx->items_per_seed = (double)counters[16] / (double)n_seeds;
    ctx->sel_rows_per_seed = (double)sel_rows_total / (double)n_seeds;
    sprof.mark("kernel");
    // path counters of this call (folded into the context's at every way out of the selection below)
    u64 const n_extensions = counters[2];
    auto count_path = [&](u64 on_host) {
        u64 with = 0, excl = 0;
        for (auto const& st : stats) { with += st.useful != 0; excl += st.fully_excluded != 0; }
        std::lock_guard<std::mutex> g(ctx->ctx->mu);
        flx_path_counters& pc = ctx->ctx->path;
        pc.seeds += n_seeds; pc.seeds_with_anchors += with; pc.seeds_excluded_by_hard_cap += excl; pc.seeds_selected_on_host += on_host;
        pc.anchors += anchors.size(); pc.cursor_extensions += n_extensions;
    };
    // ---- what the device selected; host_seed[si] != 0: this seed still goes through the host code
    hvec<HostAnchor> dev_anchors;
    hvec<u8> host_seed;
    if (device_select) {
        static_assert(sizeof(HostAnchor) == sizeof(DevOutAnchor), "the compact list is read as HostAnchor");
        dev_anchors.resize(sel_total);
        if (sel_total) {
            if ((rc = d2h(ctx, dev_anchors.data(), ctx->sel_out.ptr, (size_t)sel_total * sizeof(HostAnchor)))) return rc;
            if ((rc = ctx->sync())) return rc;
        }
        if (seeds) for (auto& a : dev_anchors) a.leaf = seeds[a.seed_index].pex_leaf_index;
        host_seed.assign(n_seeds, 0);
        bool any = false;
        for (u64 si = 0; si < n_seeds; ++si) {
            DevSelStat const st = sel_stat[si];
            if (st.flag) { host_seed[si] = 1; any = true; }
            else stats[si] = SeedStats{st.useful, st.raw, st.excluded_soft, st.excluded};
        }
        sprof.mark("device-select");
        if (getenv("FLX_SEARCH_DEBUG")) {
            u64 flagged = 0, with_anchors = 0, excl = 0;
            for (u64 si = 0; si < n_seeds; ++si) { DevSelStat const st = sel_stat[si]; flagged += st.flag; with_anchors += st.useful != 0; excl += st.excluded; }
            fprintf(stderr, "[fm_select] seeds %llu: with anchors %llu, excluded %llu, left to the host %llu; anchors %u\n", (unsigned long long)n_seeds,
                    (unsigned long long)with_anchors, (unsigned long long)excl, (unsigned long long)flagged, sel_total);
        }
        if (!any) { anchors.swap(dev_anchors); count_path(0); return FLX_OK; }
    }
    // ---- the hits per seed in emission order: `by_seed`, seed si owns [first[si], first[si+1]). With device-side selection the
    //      device has grouped them already (only the seeds left to the host are looked at below); else the host groups them.
    hvec<u32> first(n_seeds + 1, 0);
    hvec<DevHit> by_seed;
    if (device_select) {
        if ((rc = d2h(ctx, first.data(), ctx->hit_off.ptr, (n_seeds + 1) * 4))) return rc;
        if ((rc = ctx->sync())) return rc;
        by_seed.resize(first[n_seeds]);
        if ((rc = d2h(ctx, by_seed.data(), ctx->grouped.ptr, (size_t)first[n_seeds] * sizeof(DevHit)))) return rc;
        if ((rc = ctx->sync())) return rc;
        // the segments the host is going to look at, into emission order (the device sorts its own seeds' hits where it reads them)
        if (!ordered)
            for (u64 si = 0; si < n_seeds; ++si)
                if (host_seed[si] && first[si + 1] - first[si] > 1)
                    std::stable_sort(by_seed.begin() + first[si], by_seed.begin() + first[si + 1], [](DevHit const& a, DevHit const& b) { return a.key < b.key; });
        sprof.mark("d2h-hits");
    } else {
        u32 const n_slots = counters[0];      // reserved slots; unused ones carry seed 0xFFFFFFFF
        hvec<DevHit> hits(n_slots);
        if ((rc = d2h(ctx, hits.data(), ctx->hits.ptr, (size_t)n_slots * sizeof(DevHit)))) return rc;
        if ((rc = ctx->sync())) return rc;
        sprof.mark("d2h-hits");
        // a seed stays on one wave, whose slot ranges and slots within a range are handed out in increasing order
        for (auto const& h : hits) if (h.seed != 0xFFFFFFFFu) first[h.seed + 1]++;
        for (u64 i = 0; i < n_seeds; ++i) first[i + 1] += first[i];
        by_seed.resize(first[n_seeds]);
        hvec<u32> cursor(first.begin(), first.end() - 1);
        for (auto const& h : hits) if (h.seed != 0xFFFFFFFFu) by_seed[cursor[h.seed]++] = h;
        // into the reference's emission order (the keys of the walk with its stack in LDS; the ordered walk's hits are in it already)
        if (!ordered)
            for (u64 si = 0; si < n_seeds; ++si)
                if (first[si + 1] - first[si] > 1)
                    std::stable_sort(by_seed.begin() + first[si], by_seed.begin() + first[si + 1], [](DevHit const& a, DevHit const& b) { return a.key < b.key; });
    }
    if (raw_hits) { *raw_hits = std::move(by_seed); return FLX_OK; }
    hvec<u32> todo;                           // the seeds the host selects for, ascending
    if (host_seed.empty()) { todo.resize(n_seeds); std::iota(todo.begin(), todo.end(), 0u); }
    else for (u64 si = 0; si < n_seeds; ++si) if (host_seed[si]) todo.push_back((u32)si);

    sprof.mark("group");
    // ---- hard cap, group order, anchor choice (search.cpp:190-302)
    struct RowReq { u32 seed, errors, row; };
    hvec<RowReq> reqs;
    hvec<u64> total_raw(n_seeds, 0);
    hvec<u8> excluded(n_seeds, 0);
    hvec<Group> groups;
    hvec<u32> alive;
    for (u32 const si : todo) {
        if (first[si] == first[si + 1]) continue;               // no hit at all: nothing to select
        if (first[si] + 1 == first[si + 1] && by_seed[first[si]].len == 1 && cfg.max_num_anchors_hard >= 1 && cfg.max_num_anchors_soft >= 1) {
            // one group of one row (most seeds of a read that has a single locus): every order and strategy keeps exactly it
            total_raw[si] = 1;
            reqs.push_back(RowReq{(u32)si, by_seed[first[si]].errors, by_seed[first[si]].lb});
            continue;
        }
        groups.clear();
        u64 total = 0;
        for (u32 h = first[si]; h < first[si + 1]; ++h) { groups.push_back(Group{by_seed[h].lb, by_seed[h].len, by_seed[h].errors}); total += by_seed[h].len; }
        total_raw[si] = total;
        if (total > cfg.max_num_anchors_hard && cfg.anchor_choice_strategy != FLX_CHOICE_FIRST_REPORTED) { excluded[si] = 1; continue; }
        switch (cfg.anchor_group_order) {
            case FLX_ORDER_COUNT_FIRST:
                std::sort(groups.begin(), groups.end(), [](Group const& a, Group const& b) {
                    if (a.len != b.len) return a.len < b.len;
                    return a.errors < b.errors;
                });
                break;
            case FLX_ORDER_ERRORS_FIRST:     // literally as written in search.cpp:215-222
                std::sort(groups.begin(), groups.end(), [](Group const& a, Group const& b) {
                    if (a.errors != b.errors) return a.len < b.len;
                    return a.errors < b.errors;
                });
                break;
            default: break;
        }
        u64 kept = 0;
        if (cfg.anchor_choice_strategy == FLX_CHOICE_ROUND_ROBIN) {
            // search.cpp:239-272: cycle through the groups that still have rows, taking row lb + round from each; a group leaves
            // the cycle after its last row. (The reference keeps the remaining indices in a std::set; a compacting vector visits
            // them in the same ascending order.)
            alive.resize(groups.size());
            for (size_t g = 0; g < groups.size(); ++g) alive[g] = (u32)g;
            u64 round = 0;
            while (kept != cfg.max_num_anchors_soft && !alive.empty()) {
                size_t w = 0;
                for (size_t a = 0; a < alive.size(); ++a) {
                    if (kept == cfg.max_num_anchors_soft) { alive[w++] = alive[a]; continue; }
                    Group const& g = groups[alive[a]];
                    reqs.push_back(RowReq{(u32)si, g.errors, (u32)(g.lb + round)});
                    ++kept;
                    if (g.len != round + 1) alive[w++] = alive[a];
                }
                alive.resize(w);
                ++round;
            }
        } else {
            size_t gi = 0;
            while (kept != cfg.max_num_anchors_soft && gi < groups.size()) {
                Group const& g = groups[gi];
                for (u32 r = 0; r < g.len; ++r) {
                    reqs.push_back(RowReq{(u32)si, g.errors, g.lb + r});
                    if (++kept == cfg.max_num_anchors_soft) break;
                }
                ++gi;
            }
        }
    }

    sprof.mark("select");
    // ---- locate (search.cpp:253, 284) as one SA gather
    hvec<u32> rows(reqs.size()), textpos(reqs.size());
    for (size_t i = 0; i < reqs.size(); ++i) rows[i] = reqs[i].row;
    if (!reqs.empty()) {
        if ((rc = h2d(ctx, ctx->rows, rows.data(), rows.size() * 4))) return rc;
        if ((rc = ctx->rows_out.ensure(rows.size() * 4))) return rc;
        rc = timed_launch(ctx, "fm_locate", rows.size() * 8, rows.size(), [&] {
            return DeviceApi::locate(ctx->stream, ctx->ctx->didx, ctx->rows.as<u32>(), (u32)rows.size(), ctx->rows_out.as<u32>());
        });
        if (rc) return rc;
        if ((rc = d2h(ctx, textpos.data(), ctx->rows_out.ptr, rows.size() * 4))) return rc;
        if ((rc = ctx->sync())) return rc;
    }

    sprof.mark("locate");
    // ---- per seed: bucket per reference, erase useless anchors, flatten (search.cpp:78-100, 304-318)
    size_t const nref = H.seq_len.size();
    hvec<hvec<RefAnchor>> by_ref(nref);
    hvec<u32> touched;                    // references that received an anchor of the current seed
    size_t ri = 0;
    for (u32 const si : todo) {
        if (excluded[si]) { stats[si] = SeedStats{0, 0, 0, 1}; continue; }
        if (ri >= reqs.size() || reqs[ri].seed != si) continue;      // nothing kept: stats stay zero
        if (ri + 1 == reqs.size() || reqs[ri + 1].seed != si) {
            // a single anchor: its bucket holds nothing that could make it useless
            u64 const p = textpos[ri];
            if (p >= H.n) { set_error("fm_locate returned a position outside the text"); return FLX_ERR_INTERNAL; }
            size_t const s = nref == 1 ? 0 : std::upper_bound(H.seq_start.begin(), H.seq_start.end(), p) - H.seq_start.begin() - 1;
            stats[si] = SeedStats{1, 1, (u32)(total_raw[si] - 1), 0};
            anchors.push_back(HostAnchor{(u32)si, (seeds ? seeds[si].pex_leaf_index : 0u), (u32)s, reqs[ri].errors, p - H.seq_start[s]});
            ++ri;
            continue;
        }
        touched.clear();
        u32 raw = 0;
        while (ri < reqs.size() && reqs[ri].seed == si) {
            u64 const p = textpos[ri];
            if (p >= H.n) { set_error("fm_locate returned a position outside the text"); return FLX_ERR_INTERNAL; }
            size_t const s = nref == 1 ? 0 : std::upper_bound(H.seq_start.begin(), H.seq_start.end(), p) - H.seq_start.begin() - 1;
            if (by_ref[s].empty()) touched.push_back((u32)s);
            by_ref[s].push_back(RefAnchor{p - H.seq_start[s], reqs[ri].errors});
            ++raw;
            ++ri;
        }
        std::sort(touched.begin(), touched.end());                   // anchors are reported by reference id (search.cpp:78-100)
        u32 useful = raw;
        if (cfg.erase_useless_anchors) {
            useful = 0;
            for (u32 r : touched) { erase_useless(by_ref[r]); useful += (u32)by_ref[r].size(); }
        }
        stats[si] = SeedStats{useful, raw, (u32)(total_raw[si] - raw), 0};
        for (u32 r : touched) {
            for (auto const& a : by_ref[r]) anchors.push_back(HostAnchor{(u32)si, (seeds ? seeds[si].pex_leaf_index : 0u), r, (u32)a.errors, a.pos});
            by_ref[r].clear();
        }
    }
    sprof.mark("erase+flatten");
    if (!dev_anchors.empty()) {               // both lists are in seed order
        hvec<HostAnchor> merged(anchors.size() + dev_anchors.size());
        std::merge(anchors.begin(), anchors.end(), dev_anchors.begin(), dev_anchors.end(), merged.begin(),
                   [](HostAnchor const& a, HostAnchor const& b) { return a.seed_index < b.seed_index; });
        anchors.swap(merged);
    }
    count_path(todo.size());
    return FLX_OK;
}
}  // namespace flx

using namespace flx;

// ================================================================================================ C ABI: seam 1
extern "C" int flx_search_seeds(flx_ctx* ctx, const uint8_t* seq_pool, uint64_t seq_pool_len, const flx_seed* seeds, uint64_t n_seeds,
                                const flx_search_config* cfg, flx_anchor* out_anchors, uint64_t* n_anchors, flx_seed_stats* out_stats) {
    if (!ctx || !cfg || !n_anchors || (n_seeds && (!seeds || !seq_pool))) { set_error("flx_search_seeds: null argument"); return FLX_ERR_INVALID; }
    if (cfg->max_num_anchors_hard < cfg->max_num_anchors_soft) { set_error("max-anchors-hard must not be smaller than max-anchors-soft (floxer_cli.cpp:194)"); return FLX_ERR_INVALID; }
    FLX_HIP(hipSetDevice(ctx->device));
    hvec<HostAnchor> anchors;
    hvec<SeedStats> stats;
    LaneLease lease(ctx, ctx->external_stream ? 0 : -1);
    int rc = search_seeds_device(lease.lane, nullptr, seq_pool, seq_pool_len, seeds, n_seeds, *cfg, anchors, stats, nullptr, 0);
    if (rc) return rc;
    uint64_t const cap = *n_anchors;
    *n_anchors = anchors.size();
    if (out_stats) for (uint64_t i = 0; i < n_seeds; ++i) out_stats[i] = flx_seed_stats{stats[i].useful, stats[i].raw, stats[i].excluded_soft, stats[i].fully_excluded};
    if (anchors.size() > cap) { set_error("anchor buffer too small"); return FLX_ERR_CAPACITY; }
    for (size_t i = 0; i < anchors.size(); ++i)
        out_anchors[i] = flx_anchor{anchors[i].seed_index, anchors[i].leaf, anchors[i].ref_id, anchors[i].errors, anchors[i].pos};
    return FLX_OK;
}

extern "C" int flx_search_groups(flx_ctx* ctx, const uint8_t* seq_pool, uint64_t seq_pool_len, const flx_seed* seeds, uint64_t n_seeds,
                                 uint64_t max_hits_per_seed, flx_hit_group* out, uint64_t* n_out) {
    if (!ctx || !n_out || (n_seeds && (!seeds || !seq_pool))) { set_error("flx_search_groups: null argument"); return FLX_ERR_INVALID; }
    FLX_HIP(hipSetDevice(ctx->device));
    hvec<HostAnchor> anchors;
    hvec<SeedStats> stats;
    hvec<DevHit> hits;
    flx_search_config cfg{};
    LaneLease lease(ctx, ctx->external_stream ? 0 : -1);
    int rc = search_seeds_device(lease.lane, nullptr, seq_pool, seq_pool_len, seeds, n_seeds, cfg, anchors, stats, &hits, max_hits_per_seed);
    if (rc) return rc;
    uint64_t const cap = *n_out;
    *n_out = hits.size();
    if (hits.size() > cap) { set_error("hit buffer too small"); return FLX_ERR_CAPACITY; }
    for (size_t i = 0; i < hits.size(); ++i) out[i] = flx_hit_group{hits[i].seed, hits[i].lb, hits[i].len, hits[i].errors};
    return FLX_OK;
}
