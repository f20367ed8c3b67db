// K1b and K2 for gfx950: the scans of the anchor selection's count arrays, the selection itself (hits -> located, ordered, pruned
// anchors per seed) and the plain locate gather.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_internal.hpp"
#include "flx_stdsort.hpp"
#include "flx_wave.hpp"

namespace flx {

// Scans (exclusive sums) of the anchor selection's count arrays in two launches without any waiting between blocks: every block reduces
// its tile, then every block scans its tile again behind the reduction of the tiles before it (a few hundred words it adds up
// itself). The library scans are single-pass with decoupled look-back: their blocks spin on their predecessors' results, which on a
// GPU filled with other lanes' kernels made a 1.2 M-element scan take a millisecond and burn issue slots meanwhile (11 % of the
// kernel time of a run went into them); an onesweep radix sort in place of rocprim's merge sort for the same reason cost 10 % of the
// throughput.
constexpr u32 SCAN_ITEMS = 8, SCAN_TILE = 256 * SCAN_ITEMS;
template <bool MAX> __device__ __forceinline__ u32 scan_op(u32 a, u32 b) { return MAX ? max(a, b) : a + b; }
template <bool MAX>
__device__ __forceinline__ u32 block_reduce_256(u32 v, u32* __restrict__ lds4) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = scan_op<MAX>(v, (u32)__shfl_xor((int)v, off));
    if (lane_id() == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    u32 const r = scan_op<MAX>(scan_op<MAX>(lds4[0], lds4[1]), scan_op<MAX>(lds4[2], lds4[3]));
    __syncthreads();
    return r;
}
template <bool MAX>
__global__ void __launch_bounds__(256) vr_scan_reduce_kernel(const u32* __restrict__ in, u32 n, u32* __restrict__ tile_total) {
    __shared__ u32 lds4[4];
    u32 const base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    u32 v = 0;
#pragma unroll
    for (u32 j = 0; j < SCAN_ITEMS; ++j) if (base + j < n) v = scan_op<MAX>(v, in[base + j]);
    u32 const total = block_reduce_256<MAX>(v, lds4);
    if (threadIdx.x == 0) tile_total[blockIdx.x] = total;
}
template <bool MAX, bool EXCLUSIVE = false>
__global__ void __launch_bounds__(256) vr_scan_apply_kernel(const u32* __restrict__ in, u32 n, const u32* __restrict__ tile_total, u32* __restrict__ out) {
    __shared__ u32 lds4[4];
    __shared__ u32 wave_total[4];
    u32 before = 0;                                       // the tiles before this one
    for (u32 t = threadIdx.x; t < blockIdx.x; t += 256u) before = scan_op<MAX>(before, tile_total[t]);
    before = block_reduce_256<MAX>(before, lds4);
    u32 const base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    u32 item[SCAN_ITEMS];
    u32 run = 0;
#pragma unroll
    for (u32 j = 0; j < SCAN_ITEMS; ++j) {
        if (EXCLUSIVE) item[j] = run;
        run = scan_op<MAX>(run, base + j < n ? in[base + j] : 0u);
        if (!EXCLUSIVE) item[j] = run;
    }
    // exclusive scan of the threads' totals: within the wave by shuffles, across the four waves through LDS
    u32 incl = run;
#pragma unroll
    for (u32 off = 1; off < 64u; off <<= 1) {
        u32 const up = (u32)__shfl_up((int)incl, off);
        if (lane_id() >= off) incl = scan_op<MAX>(incl, up);
    }
    if (lane_id() == 63u) wave_total[threadIdx.x >> 6] = incl;
    __syncthreads();
    u32 prefix = before;
    for (u32 w = 0; w < (threadIdx.x >> 6); ++w) prefix = scan_op<MAX>(prefix, wave_total[w]);
    u32 const excl = (u32)__shfl_up((int)incl, 1);
    if (lane_id() > 0) prefix = scan_op<MAX>(prefix, excl);
#pragma unroll
    for (u32 j = 0; j < SCAN_ITEMS; ++j) if (base + j < n) out[base + j] = scan_op<MAX>(prefix, item[j]);
}
static void exclusive_sum(hipStream_t s, const u32* in, u32* out, u32 n, u32* tile_total) {
    unsigned const tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    hipLaunchKernelGGL((vr_scan_reduce_kernel<false>), dim3(tiles), dim3(256), 0, s, in, n, tile_total);
    hipLaunchKernelGGL((vr_scan_apply_kernel<false, true>), dim3(tiles), dim3(256), 0, s, in, n, tile_total, out);
}

// ================================================================================================ K1b: anchor selection
// hits -> per-seed segments in emission order (a scan over the seeds' hit counts + a scatter by the ordinal each hit carries),
// then one thread per seed does what search.cpp:190-318 does with the seed's groups: hard cap, group order, rows round robin,
// locate through the suffix array, buckets per reference sorted by position, useless anchors erased (search.cpp:352-389).
// Handled here: seeds with at most SEL_MAX groups whose rows all fit under the soft cap and SEL_MAX. The two std::sort calls of
// the reference (groups by (count, errors), a bucket's anchors by position) are reproduced step for step (std_sort_emulated):
// their comparators tie (the same row reached through two groups gives two anchors of equal position) and the order of equal
// elements shows in the result. Every seed not handled is flagged and goes through the host code.
constexpr u32 SEL_MAX = 64;
struct SelStat { u8 useful, raw, flag, excluded; u32 excluded_soft; };      // flag 1: the host selects this seed's anchors; = DevSelStat

// A search that outgrew the hit buffer (more slots asked for, counters[0], than it has) counted hits in seed_cnt that have no slot:
// the offsets then run past `grouped`. Such a pass is repeated with a larger buffer; nothing of it is scattered and nothing selected.
// With every hit in its slot the last offset is at most counters[0] <= hit_cap.
__device__ __forceinline__ bool hits_fit(const u32* __restrict__ counters, u32 hit_cap) { return counters[0] <= hit_cap; }

__global__ void __launch_bounds__(256) hit_scatter_kernel(const DevHit* __restrict__ hits, const u32* __restrict__ counters, u32 hit_cap,
                                                          const u32* __restrict__ offset, DevHit* __restrict__ grouped) {
    u32 const n_slots = hits_fit(counters, hit_cap) ? counters[0] : 0u;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += gridDim.x * blockDim.x) {
        DevHit h = hits[i];
        if (h.seed == 0xFFFFFFFFu) continue;
        u32 const ordinal = h.errors >> 8;
        h.errors &= 0xFFu;
        grouped[offset[h.seed] + ordinal] = h;
    }
}

struct SelGroup { u32 lb, len, errors; };
struct SelAnchor { u32 pos; u32 ref; u32 errors; };           // pos within its reference sequence (the text has fewer than 2^32 symbols)
struct SelKey { u32 lo, hi; };
__device__ __forceinline__ bool sel_key_less(u64 k, SelKey const& o) { return k < ((u64)o.lo | ((u64)o.hi << 32)); }

// the selection of one seed whose groups (cnt <= CAP) hold `total` <= CAP rows; returns false when the seed has to go to the host.
// Working storage from the caller (a thread's indexed private arrays would live in scratch memory: round 3 had 720 B per lane there):
// g: CAP groups; w: CAP SelKeys while the groups are put into emission order, CAP SelAnchors afterwards (the two do not overlap in
// time); stacks: 48 ints when CAP > 16 (std::sort's partitions)
template <u32 CAP, bool WRITE>
__device__ __forceinline__ bool select_seed(const DevHit* __restrict__ groups, u32 cnt, u32 total, const u32* __restrict__ sa, u32 n_text,
                                            const u64* __restrict__ seq_start, u32 n_ref, u32 erase, u32 sid, SelStat& st, u32& produced,
                                            DevOutAnchor* __restrict__ out, u32 at, u32 out_cap, SelGroup* g, void* w, int* stacks) {
    // the groups in search_n's emission order (the keys of fm_search_kernel; all 0 from the ordered kernel, whose hits are in it already:
    // the insertion sort is stable), then ordered by (count, errors) (search.cpp:200-212)
    {
        SelKey* const key = static_cast<SelKey*>(w);
        for (u32 i = 0; i < cnt; ++i) {
            DevHit const h = groups[i];
            u32 j = i;
            while (j > 0 && sel_key_less(h.key, key[j - 1])) { key[j] = key[j - 1]; g[j] = g[j - 1]; --j; }
            key[j] = SelKey{(u32)h.key, (u32)(h.key >> 32)};
            g[j] = SelGroup{h.lb, h.len, h.errors};
        }
    }
    auto less_g = [](SelGroup const& x, SelGroup const& y) { return x.len != y.len ? x.len < y.len : x.errors < y.errors; };
    if (CAP <= 16u) insertion_sort_emulated(g, (int)cnt, less_g);
    else if (!std_sort_emulated(g, (int)cnt, less_g, stacks)) return false;
    // rows round robin over the groups (search.cpp:239-272), located
    SelAnchor* const an = static_cast<SelAnchor*>(w);
    u32 kept = 0;
    bool bad = false;
    // (`total` = the rows to keep: all of them, or the soft cap when the seed has more: the cycle then stops in the middle of a round)
    for (u32 round = 0; kept < total; ++round)
        for (u32 gi = 0; gi < cnt && kept < total; ++gi) {
            if (g[gi].len <= round) continue;
            u32 const row = g[gi].lb + round;
            u64 const p = row < n_text ? sa[row] : 0xFFFFFFFFull;
            if (p >= n_text) bad = true;
            u32 r = 0;
            if (n_ref > 1) {                                   // last sequence that starts at or before p
                u32 lo = 0, hi = n_ref;
                while (hi - lo > 1) { u32 const mid = (lo + hi) >> 1; if (seq_start[mid] <= p) lo = mid; else hi = mid; }
                r = lo;
            }
            an[kept++] = SelAnchor{(u32)(p - seq_start[r]), r, g[gi].errors};
        }
    if (bad) return false;                                  // the host reports the error
    // buckets per reference in id order, each keeping the order of selection (search.cpp:78-100, 304-318)
    for (u32 i = 1; i < kept; ++i) {
        SelAnchor const v = an[i];
        u32 j = i;
        while (j > 0 && v.ref < an[j - 1].ref) { an[j] = an[j - 1]; --j; }
        an[j] = v;
    }
    u64 gone = 0;                                           // bit i: anchor i erased
    if (erase) {
        u32 b0 = 0;
        while (b0 < kept) {                                 // one bucket = one reference (search.cpp:352-389)
            u32 b1 = b0;
            while (b1 < kept && an[b1].ref == an[b0].ref) ++b1;
            auto less_p = [](SelAnchor const& x, SelAnchor const& y) { return x.pos < y.pos; };
            if (CAP <= 16u) insertion_sort_emulated(an + b0, (int)(b1 - b0), less_p);
            else if (!std_sort_emulated(an + b0, (int)(b1 - b0), less_p, stacks)) return false;
            // an erased anchor compares with "infinitely many" errors
            auto better = [&](u32 a, u32 b) {
                u64 const ea = (gone >> a) & 1 ? ~0ull : (u64)an[a].errors, eb = (gone >> b) & 1 ? ~0ull : (u64)an[b].errors;
                u64 const d = an[a].pos < an[b].pos ? an[b].pos - an[a].pos : an[a].pos - an[b].pos;
                return ea <= eb && d <= eb - ea;
            };
            for (u32 cur = b0; cur + 1 < b1;) {
                u32 other = cur + 1;
                while (other < b1 && better(cur, other)) { gone |= 1ull << other; ++other; }
                if (other < b1 && better(other, cur)) gone |= 1ull << cur;
                cur = other;
            }
            b0 = b1;
        }
    }
    st.raw = (u8)kept;
    for (u32 i = 0; i < kept; ++i)
        if (!((gone >> i) & 1)) {
            if (WRITE && at + produced < out_cap) out[at + produced] = DevOutAnchor{sid, 0u, an[i].ref, an[i].errors, (u64)an[i].pos};
            ++produced;
        }
    st.useful = (u8)produced;
    return true;
}

// Every seed's class: nothing to select (no hit / over the hard cap / left to the host: its statistics are final here), light (at
// most SEL_LIGHT groups and rows: one thread per seed, seed_select_kernel) or heavy (up to SELW_MAX_GROUPS groups, any number of
// rows up to the hard cap of which the soft cap's worth, at most SEL_MAX, is kept: one wave per seed, seed_select_wave_kernel).
// rows[sid] = the slots the seed gets in the sparse anchor list. Light and heavy seeds go on two lists (wave-aggregated appends;
// the order of a list does not matter, every seed writes to its own slots).
constexpr u32 SEL_LIGHT = 8;
constexpr u32 SELW_MAX_GROUPS = 512, SELW_FEW_GROUPS = 64;
__global__ void __launch_bounds__(256) seed_rows_kernel(const DevHit* __restrict__ grouped, const u32* __restrict__ hit_offset, u32 n_seeds,
                                                        const u32* __restrict__ counters, u32 hit_cap, u32 hard_cap, u32 soft_cap,
                                                        u32* __restrict__ rows, SelStat* __restrict__ stat, u32* __restrict__ n_out,
                                                        u32* __restrict__ lists, u32* __restrict__ list_counts) {
    u32 const sid = blockIdx.x * blockDim.x + threadIdx.x;
    u32 cls = 0;                                             // 1 light, 2 heavy (a wave, up to SELW_FEW_GROUPS groups), 3 heavy with more groups
    if (sid < n_seeds) {
        // (a pass whose hits did not fit: every seed counts as one without hits, so no kernel behind this one reads `grouped`)
        u32 const g0 = hit_offset[sid], cnt = hits_fit(counters, hit_cap) ? hit_offset[sid + 1] - g0 : 0u;
        SelStat st{0, 0, 0, 0, 0};
        u32 total = 0;
        if (cnt > hard_cap) st.excluded = 1;                // every group has at least one row: over the hard cap whatever the rows are
        else if (cnt > SELW_MAX_GROUPS) st.flag = 1;        // more groups than the wave kernel's arrays hold: the host
        else if (cnt > 0) {
            u32 all = 0;
            for (u32 i = 0; i < cnt; ++i) all += min(grouped[g0 + i].len, 0x1000000u);
            total = min(all, soft_cap);                      // rows kept (search.cpp:239-272 stops at the soft cap)
            if (all > hard_cap) st.excluded = 1;
            else if (total > SEL_MAX) st.flag = 1;           // a soft cap beyond the anchor arrays: the host
            else { cls = (cnt <= SEL_LIGHT && total <= SEL_LIGHT) ? 1u : cnt <= SELW_FEW_GROUPS ? 2u : 3u; st.excluded_soft = all - total; }
        }
        rows[sid] = cls ? total : 0u;
        if (!cls) { stat[sid] = st; n_out[sid] = 0; }
        else stat[sid].excluded_soft = st.excluded_soft;     // (the select kernels fill in the rest)
    }
#pragma unroll
    for (u32 c = 1; c <= 3; ++c) {
        u64 const m = __ballot(cls == c);
        if (!m) continue;
        u32 base = 0;
        if (lane_id() == 0) base = atomicAdd(&list_counts[c - 1], (u32)__popcll(m));
        base = (u32)__builtin_amdgcn_readfirstlane((int)base);
        if (cls == c) lists[(c - 1) * n_seeds + base + (u32)__popcll(m & ((1ull << lane_id()) - 1ull))] = sid;
    }
}

// the seeds of one list: their anchors to their slots of the sparse list (row_offset), n_out says how many. A thread's arrays are in LDS
// for the light seeds (CAP groups + CAP keys / anchors, 12 B each, a word of padding per thread against bank conflicts); a seed with one
// group of one row - most seeds of a read with one locus - takes neither.
template <u32 CAP>
__global__ void __launch_bounds__(64, 4) seed_select_kernel(const u32* __restrict__ list, const u32* __restrict__ list_count,
                                                         const DevHit* __restrict__ grouped, const u32* __restrict__ hit_offset,
                                                         const u32* __restrict__ sa, u32 n_text, const u64* __restrict__ seq_start, u32 n_ref,
                                                         u32 erase, SelStat* __restrict__ stat, u32* __restrict__ n_out,
                                                         const u32* __restrict__ row_offset, const u32* __restrict__ rows,
                                                         DevOutAnchor* __restrict__ sparse, u32 sparse_cap) {
    constexpr u32 IN_LDS = CAP <= 16u ? 1u : 0u;
    constexpr u32 STRIDE = 6u * CAP + 1u;                       // words per thread
    __shared__ u32 s_pool[IN_LDS ? 64u * STRIDE : 1u];
    SelGroup g_priv[IN_LDS ? 1u : CAP];
    SelAnchor w_priv[IN_LDS ? 1u : CAP];
    int stacks_priv[IN_LDS ? 1 : 48];
    SelGroup* const g = IN_LDS ? reinterpret_cast<SelGroup*>(s_pool + threadIdx.x * STRIDE) : g_priv;
    void* const w = IN_LDS ? static_cast<void*>(s_pool + threadIdx.x * STRIDE + 3u * CAP) : static_cast<void*>(w_priv);
    u32 const n = *list_count;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        u32 const sid = list[i];
        u32 const g0 = hit_offset[sid], cnt = hit_offset[sid + 1] - g0;
        SelStat st{0, 0, 0, 0, stat[sid].excluded_soft};
        u32 produced = 0;
        bool ok;
        if (cnt == 1u && rows[sid] == 1u) {
            // one group, one row: every order and strategy keeps exactly it
            DevHit const h = grouped[g0];
            u64 const p = h.lb < n_text ? sa[h.lb] : 0xFFFFFFFFull;
            ok = p < n_text;
            if (ok) {
                u32 r = 0;
                if (n_ref > 1) { u32 lo = 0, hi = n_ref; while (hi - lo > 1) { u32 const mid = (lo + hi) >> 1; if (seq_start[mid] <= p) lo = mid; else hi = mid; } r = lo; }
                u32 const at = row_offset[sid];
                if (at < sparse_cap) sparse[at] = DevOutAnchor{sid, 0u, r, h.errors, p - seq_start[r]};
                produced = 1; st.raw = 1; st.useful = 1;
            }
        } else ok = select_seed<CAP, true>(grouped + g0, cnt, rows[sid], sa, n_text, seq_start, n_ref, erase, sid, st, produced, sparse, row_offset[sid], sparse_cap, g, w, stacks_priv);
        if (!ok) {
            st = SelStat{0, 0, 1, 0, 0};
            produced = 0;
        }
        stat[sid] = st;
        n_out[sid] = st.flag ? 0u : produced;
    }
}

// One wave per heavy seed: what select_seed does, with the parts that parallelise spread over the lanes - the emission order and
// the stable orders as ranks (element i goes to the number of elements in front of it), the rows' round robin as one ballot per
// round, SA and reference lookups one per lane - and the parts that are std::sort's own (more than 16 elements: introsort, whose
// order of equal elements has to be reproduced step by step) and the erase sweep on one lane over LDS arrays. A round-2 profile had
// the thread-per-seed form of this at 3 ms per launch on 2.3 KB of scratch per thread (profiles/r03_k1v2_kernel_stats.csv).
// (MAXG: groups a seed of the list may have; 64 groups keep the block at 2.7 KB of LDS, which finds room on a CU next to the DP
// kernels of other lanes; the few seeds with up to 512 groups take the 17-KB form)
template <u32 MAXG>
__global__ void __launch_bounds__(64, MAXG <= 64 ? 4 : 2) seed_select_wave_kernel(const u32* __restrict__ list, const u32* __restrict__ list_count,
                                                              const DevHit* __restrict__ grouped, const u32* __restrict__ hit_offset,
                                                              const u32* __restrict__ sa, u32 n_text, const u64* __restrict__ seq_start, u32 n_ref,
                                                              u32 erase, SelStat* __restrict__ stat, u32* __restrict__ n_out,
                                                              const u32* __restrict__ row_offset, const u32* __restrict__ rows,
                                                              DevOutAnchor* __restrict__ sparse, u32 sparse_cap) {
    __shared__ u64 s_key[MAXG];
    __shared__ SelGroup s_a[MAXG], s_b[MAXG];
    __shared__ u32 s_row[SEL_MAX], s_err[SEL_MAX];
    __shared__ SelAnchor s_an[SEL_MAX];
    __shared__ u32 s_flag[4];                 // [0] a sort gave up (host), [1..2] erased anchors (bits)
    __shared__ int s_stacks[48];              // std::sort's partitions still to do (one lane sorts)
    u32 const lane = lane_id();
    u64 const below = (1ull << lane) - 1ull;
    u32 const n = *list_count;
    for (u32 li = blockIdx.x; li < n; li += gridDim.x) {
        u32 const sid = list[li];
        u32 const g0 = hit_offset[sid], cnt = hit_offset[sid + 1] - g0, total = rows[sid];
        __syncthreads();
        for (u32 i = lane; i < cnt; i += 64u) { DevHit const h = grouped[g0 + i]; s_key[i] = h.key; s_a[i] = SelGroup{h.lb, h.len, h.errors}; }
        if (lane < 4u) s_flag[lane] = 0u;
        __syncthreads();
        // ---- emission order (the keys of fm_search; equal keys keep their order), then std::sort by (count, errors): up to 16
        //      elements that is an insertion sort, i.e. stable
        for (u32 i = lane; i < cnt; i += 64u) {
            u64 const k = s_key[i];
            u32 r = 0;
            for (u32 j = 0; j < cnt; ++j) { u64 const kj = s_key[j]; r += (kj < k || (kj == k && j < i)) ? 1u : 0u; }
            s_b[r] = s_a[i];
        }
        __syncthreads();
        auto less_g = [](SelGroup const& x, SelGroup const& y) { return x.len != y.len ? x.len < y.len : x.errors < y.errors; };
        if (cnt <= 16u) {
            if (lane < cnt) {
                SelGroup const me = s_b[lane];
                u32 r = 0;
                for (u32 j = 0; j < cnt; ++j) { SelGroup const o = s_b[j]; r += (less_g(o, me) || (!less_g(me, o) && j < lane)) ? 1u : 0u; }
                s_a[r] = me;
            }
        } else {
            if (lane == 0u && !std_sort_emulated(s_b, (int)cnt, less_g, s_stacks)) s_flag[0] = 1u;
            __syncthreads();
            for (u32 i = lane; i < cnt; i += 64u) s_a[i] = s_b[i];
        }
        __syncthreads();
        // ---- rows round robin over the groups (search.cpp:239-272): row lb + round of every group that still has one, until
        //      `total` are kept
        //      (with more than 64 groups round 0 ends at its first ballot: all 64 lanes are alive and total <= SEL_MAX = 64 rows are
        //      kept, so the later bases only ever run with 64 groups or fewer, where there are none)
        u32 kept = 0;
        for (u32 round = 0; kept < total; ++round) {
            bool any = false;
            for (u32 base = 0; base < cnt && kept < total; base += 64u) {
                u32 const i = base + lane;
                bool const alive = i < cnt && s_a[i].len > round;
                u64 const m = __ballot(alive);
                if (!m) continue;
                any = true;
                u32 const slot = kept + (u32)__popcll(m & below);
                if (alive && slot < total) { s_row[slot] = s_a[i].lb + round; s_err[slot] = s_a[i].errors; }
                kept = min(total, kept + (u32)__popcll(m));
            }
            if (!any) break;
        }
        __syncthreads();
        // ---- locate, reference, position; buckets per reference in id order, each keeping the order of selection
        bool const mine = lane < kept;
        u64 p = 0;
        u32 ref = 0, err = 0;
        bool bad = false;
        if (mine) {
            u32 const row = s_row[lane];
            err = s_err[lane];
            p = row < n_text ? sa[row] : 0xFFFFFFFFull;
            bad = p >= n_text;
            if (!bad && n_ref > 1) {
                u32 lo = 0, hi = n_ref;
                while (hi - lo > 1) { u32 const mid = (lo + hi) >> 1; if (seq_start[mid] <= p) lo = mid; else hi = mid; }
                ref = lo;
            }
        }
        if (__any(bad)) s_flag[0] = 1u;
        u32 r3 = 0;
        for (u32 j = 0; j < kept; ++j) { u32 const rj = (u32)__shfl((int)ref, (int)j); r3 += (rj < ref || (rj == ref && j < lane)) ? 1u : 0u; }
        if (mine && !bad) s_an[r3] = SelAnchor{(u32)(p - seq_start[ref]), ref, err};
        __syncthreads();
        // ---- erase_useless_anchors (search.cpp:352-389) bucket by bucket: std::sort by position, then the sweep
        if (erase && lane == 0u && s_flag[0] == 0u) {
            u64 gone = 0;
            u32 b0 = 0;
            while (b0 < kept) {
                u32 b1 = b0;
                while (b1 < kept && s_an[b1].ref == s_an[b0].ref) ++b1;
                if (!std_sort_emulated(s_an + b0, (int)(b1 - b0), [](SelAnchor const& x, SelAnchor const& y) { return x.pos < y.pos; }, s_stacks)) { s_flag[0] = 1u; break; }
                auto better = [&](u32 a, u32 b) {          // an erased anchor compares with "infinitely many" errors
                    u64 const ea = (gone >> a) & 1 ? ~0ull : (u64)s_an[a].errors, eb = (gone >> b) & 1 ? ~0ull : (u64)s_an[b].errors;
                    u64 const d = s_an[a].pos < s_an[b].pos ? s_an[b].pos - s_an[a].pos : s_an[a].pos - s_an[b].pos;
                    return ea <= eb && d <= eb - ea;
                };
                for (u32 cur = b0; cur + 1 < b1;) {
                    u32 other = cur + 1;
                    while (other < b1 && better(cur, other)) { gone |= 1ull << other; ++other; }
                    if (other < b1 && better(other, cur)) gone |= 1ull << cur;
                    cur = other;
                }
                b0 = b1;
            }
            s_flag[1] = (u32)gone;
            s_flag[2] = (u32)(gone >> 32);
        }
        __syncthreads();
        bool const to_host = s_flag[0] != 0u;
        u64 const gone = (u64)s_flag[1] | ((u64)s_flag[2] << 32);
        bool const keep = mine && !to_host && !((gone >> lane) & 1ull);
        u64 const km = __ballot(keep);
        u32 const produced = (u32)__popcll(km);
        if (keep) {
            u32 const at = row_offset[sid] + (u32)__popcll(km & below);
            SelAnchor const a = s_an[lane];
            if (at < sparse_cap) sparse[at] = DevOutAnchor{sid, 0u, a.ref, a.errors, (u64)a.pos};
        }
        if (lane == 0u) {
            SelStat st{(u8)produced, (u8)kept, 0, 0, stat[sid].excluded_soft};
            if (to_host) st = SelStat{0, 0, 1, 0, 0};
            stat[sid] = st;
            n_out[sid] = to_host ? 0u : produced;
        }
    }
}

__global__ void __launch_bounds__(256) seed_compact_kernel(const DevOutAnchor* __restrict__ sparse, const u32* __restrict__ row_offset,
                                                           const u32* __restrict__ n_out, const u32* __restrict__ out_offset, u32 n_seeds,
                                                           DevOutAnchor* __restrict__ out, u32 out_cap, u32 sparse_cap) {
    u32 const sid = blockIdx.x * blockDim.x + threadIdx.x;
    if (sid >= n_seeds) return;
    u32 const n = n_out[sid], from = row_offset[sid], to = out_offset[sid];
    // (a seed's slots of the sparse list lie past its end when the list was outgrown: those anchors were never stored, and the pass
    // is repeated)
    for (u32 i = 0; i < n; ++i) if (from + i < sparse_cap && to + i < out_cap) out[to + i] = sparse[from + i];
}

size_t DeviceApi::select_scan_bytes(u32 n_seeds) {
    return ((size_t)(n_seeds + 1) / SCAN_TILE + 1) * sizeof(u32);        // tile totals of exclusive_sum
}

int DeviceApi::select(void* stream, const DevHit* d_hits, const u32* d_counters, u32 hit_cap, u32* d_seed_cnt, u32* d_hit_offset,
                      DevHit* d_grouped, u32 n_seeds, const DevIndex& idx, const u64* d_seq_start, u32 n_ref, u32 hard_cap, u32 soft_cap,
                      bool erase, void* d_stat, u32* d_n_out, u32* d_out_offset, DevOutAnchor* d_out, u32 out_cap, u32* d_rows,
                      u32* d_row_offset, DevOutAnchor* d_sparse, u32 sparse_cap, void* d_scan_tmp, size_t scan_bytes, u32* d_lists) {
    if (n_seeds == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    // d_seed_cnt, d_rows and d_n_out have n_seeds + 1 entries, the last one zero: the scans end with the totals
    hipError_t e = hipSuccess;
    exclusive_sum(s, d_seed_cnt, d_hit_offset, n_seeds + 1, (u32*)d_scan_tmp);
    hipLaunchKernelGGL(hit_scatter_kernel, dim3(2048), dim3(256), 0, s, d_hits, d_counters, hit_cap, d_hit_offset, d_grouped);
    SelStat* const stat = reinterpret_cast<SelStat*>(d_stat);
    u32* const list_counts = d_lists + 3 * (size_t)n_seeds;
    hipLaunchKernelGGL(seed_rows_kernel, dim3((n_seeds + 255) / 256), dim3(256), 0, s, d_grouped, d_hit_offset, n_seeds, d_counters, hit_cap,
                       hard_cap, soft_cap, d_rows, stat, d_n_out, d_lists, list_counts);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    exclusive_sum(s, d_rows, d_row_offset, n_seeds + 1, (u32*)d_scan_tmp);
    // grids sized for the usual shares (a quarter of the seeds light, a per cent heavy); the kernels loop over their lists
    hipLaunchKernelGGL((seed_select_kernel<SEL_LIGHT>), dim3(std::max(1u, (n_seeds / 4 + 63) / 64)), dim3(64), 0, s, d_lists, list_counts, d_grouped, d_hit_offset,
                       idx.sa, idx.n, d_seq_start, n_ref, erase ? 1u : 0u, stat, d_n_out, d_row_offset, d_rows, d_sparse, sparse_cap);
    // (one wave per heavy seed)
    hipLaunchKernelGGL((seed_select_wave_kernel<SELW_FEW_GROUPS>), dim3(std::max(1u, std::min(n_seeds / 8u + 1u, 16384u))), dim3(64), 0, s, d_lists + n_seeds, list_counts + 1, d_grouped,
                       d_hit_offset, idx.sa, idx.n, d_seq_start, n_ref, erase ? 1u : 0u, stat, d_n_out, d_row_offset, d_rows, d_sparse, sparse_cap);
    hipLaunchKernelGGL((seed_select_wave_kernel<SELW_MAX_GROUPS>), dim3(std::max(1u, std::min(n_seeds / 256u + 1u, 2048u))), dim3(64), 0, s, d_lists + 2 * (size_t)n_seeds, list_counts + 2, d_grouped,
                       d_hit_offset, idx.sa, idx.n, d_seq_start, n_ref, erase ? 1u : 0u, stat, d_n_out, d_row_offset, d_rows, d_sparse, sparse_cap);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    exclusive_sum(s, d_n_out, d_out_offset, n_seeds + 1, (u32*)d_scan_tmp);
    hipLaunchKernelGGL(seed_compact_kernel, dim3((n_seeds + 255) / 256), dim3(256), 0, s, d_sparse, d_row_offset, d_n_out, d_out_offset, n_seeds,
                       d_out, out_cap, sparse_cap);
    return (int)hipGetLastError();
}

// ================================================================================================ K2: locate
__global__ void __launch_bounds__(256) fm_locate_kernel(const u32* __restrict__ sa, u32 n_text, const u32* __restrict__ rows, u32 n,
                                                        u32* __restrict__ out) {
    u32 const i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 const r = rows[i];
    out[i] = r < n_text ? sa[r] : 0xFFFFFFFFu;
}

int DeviceApi::locate(void* stream, const DevIndex& idx, const u32* d_rows, u32 n, u32* d_out) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(fm_locate_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, idx.sa, idx.n, d_rows, n, d_out);
    return (int)hipGetLastError();
}

}  // namespace flx
