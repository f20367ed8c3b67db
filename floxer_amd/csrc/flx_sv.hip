// Structural-variant signatures on the device (the rule: flx_sv.hpp; the object and the C ABI: flx_sv_api.cpp). Wave64 integer work:
//   sv_extract        one wave per counted record, 64 CIGAR words per pass. A wave prefix sum over the reference-consuming lengths with
//                     a wave-uniform carry gives every word its first column; a second carry says whether a reference-consuming column
//                     lies in front of the pass (the insertion anchor, as pileup_add has it). A ballot over the qualifying D / I words
//                     gives each its place behind the keys of the earlier passes (a third carry), at the offset the host computed. Soft
//                     clips as paf_summarise takes them: S lanes below the pass's first other word add to `lead` while no other word
//                     has been seen, S lanes above its last become the pending length, which is `trail` at the end. Lanes 0..7 store
//                     the record's segment, one plain 32-byte stretch. A record whose words disagree with the host's judgement (another
//                     number of qualifying words, an interior clip, rows that do not sum to the read's length) gets a marked segment and
//                     raises the flag; no key is ever written outside the record's own stretch.
//   sv_junctions      one thread per group member: it reads the at most 64 segments of its group, counts those in front of it in
//                     (query_start, index) order and finds its successor, and writes the canonical key of that junction at its place.
//   sv_coarse_flags, sv_regroup, sv_fine_flags      the break flags of the two clustering levels over sorted keys (scanned by the shared
//                     scan, flx_scan.hip) and the keys of the second sort, {group id, q << 32 | pos_a}.
//   sv_cluster_heads, sv_cluster_bounds, sv_cluster_fill      a cluster's first member stores its start; pos_a_min / pos_a_max are
//                     reduced in the wave where the wave holds one cluster (one atomicMin and one atomicMax per wave) and per lane
//                     otherwise; support and the three q values are positional. No thread walks a cluster.
//   sv_compact        over SCAN_TILE clusters per block: mode 0 counts those with enough support, mode 1 (behind the scan of the counts)
//                     writes them in order, as pileup_sites does.
// All stores are plain C++ vector stores, all atomics device-scope integer atomics.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_scan_dev.hpp"
#include "flx_sv.hpp"

namespace flx {

namespace {
__device__ __forceinline__ SortKey sv_load_key(const SortKey* __restrict__ keys, u64 i) {
    ulonglong2 const x = reinterpret_cast<const ulonglong2*>(keys)[i];      // one 16-byte load
    return SortKey{x.x, x.y};
}
__device__ __forceinline__ void sv_store_key(SortKey* __restrict__ keys, u64 i, SortKey const& k) {
    reinterpret_cast<ulonglong2*>(keys)[i] = make_ulonglong2(k.hi, k.lo);
}
__device__ __forceinline__ SvSegment sv_load_segment(const SvSegment* __restrict__ segments, u32 i) {
    const uint4* __restrict__ p = reinterpret_cast<const uint4*>(segments + i);
    uint4 const a = p[0], b = p[1];
    return SvSegment{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}
inline u32 strided_blocks(u64 n, u32 cap) { return (u32)std::min<u64>((n + THREADS - 1) / THREADS, cap); }
}  // namespace

// ------------------------------------------------------------------------------------------------ sv_extract
__global__ void __launch_bounds__(THREADS) sv_extract_kernel(const SvJob* __restrict__ jobs, u32 n_jobs, const u32* __restrict__ words, u32 min_length,
                                                             SortKey* __restrict__ keys, u32* __restrict__ segments, u32* __restrict__ flag) {
    u32 const lane = lane_id();
    u32 const waves = gridDim.x * (THREADS / 64u);
    for (u32 id = blockIdx.x * (THREADS / 64u) + (threadIdx.x >> 6); id < n_jobs; id += waves) {       // (id is wave-uniform)
        SvJob const job = jobs[id];
        u64 pos = job.position, rows = 0, lead = 0, pending = 0;        // the wave-uniform carries
        bool any_before = false, seen = false, violation = false;
        u32 emitted = 0;
        for (u32 base = 0; base < job.n_words; base += 64u) {
            bool const valid = base + lane < job.n_words;
            u32 const word = valid ? words[job.word_off + base + lane] : 0u;                          // (op 0 consumes and counts nothing)
            u32 const op = word & 15u, len = word >> 4;
            u32 const cols = (op == 7u || op == 8u || op == 2u) ? len : 0u;
            u32 const incl = wave_inclusive_scan(cols);
            u64 const first = pos + incl - cols;
            rows += wave_sum((op == 7u || op == 8u || op == 1u || op == 4u) ? (u64)len : 0ull);
            bool const qualifies = valid && sv_word_qualifies(word, min_length);
            unsigned long long const q_mask = __ballot(qualifies);
            if (qualifies) {
                u32 const at = emitted + (u32)__popcll(q_mask & ((1ull << lane) - 1ull));
                bool const preceded = any_before || incl - cols > 0u;
                u32 const pos_a = (u32)(op == 1u && preceded ? first - 1 : first);
                if (at < job.n_events) sv_store_key(keys, job.key_off + at, sv_key(op == 2u ? SV_DEL : SV_INS, 0u, 0u, job.ref, job.ref, pos_a, len));
            }
            emitted += (u32)__popcll(q_mask);
            u32 const pass_cols = __shfl(incl, 63);
            pos += pass_cols;
            any_before = any_before || pass_cols > 0u;
            bool const is_s = valid && op == 4u, non_s = valid && op != 4u;
            unsigned long long const s_mask = __ballot(is_s), n_mask = __ballot(non_s);
            if (n_mask == 0ull) {                                        // S words only
                u64 const s = wave_sum(is_s ? (u64)len : 0ull);
                if (seen) pending += s; else lead += s;
            } else {
                u32 const first_n = (u32)__ffsll((long long)n_mask) - 1u, last_n = 63u - (u32)__clzll((long long)n_mask);
                unsigned long long const below = (1ull << first_n) - 1ull, above = last_n == 63u ? 0ull : ~0ull << (last_n + 1u);
                u64 const head = wave_sum(is_s && lane < first_n ? (u64)len : 0ull), tail = wave_sum(is_s && lane > last_n ? (u64)len : 0ull);
                if ((s_mask & ~below & ~above) != 0ull) violation = true;
                if (seen && (pending != 0 || head != 0)) violation = true;
                if (!seen) lead += head;
                pending = tail;
                seen = true;
            }
        }
        u64 const trail = pending;
        if (emitted != job.n_events || rows != (u64)job.read_len || pos == (u64)job.position || lead + trail > (u64)job.read_len) violation = true;
        u32 const q_start = (u32)(job.reverse ? trail : lead), q_end = job.read_len - (u32)(job.reverse ? lead : trail);
        u32 const v = lane == 0u ? q_start : lane == 1u ? q_end : lane == 2u ? job.position : lane == 3u ? (u32)pos : lane == 4u ? job.ref : lane == 5u ? job.reverse
                    : lane == 6u ? (violation ? SV_VIOLATION : 0u) : 0u;
        if (lane < 8u) segments[(u64)id * 8u + lane] = v;
        if (violation && lane == 0u) atomicOr(flag, 1u);
    }
}

// ------------------------------------------------------------------------------------------------ sv_junctions
__global__ void __launch_bounds__(THREADS) sv_junctions_kernel(const SvMember* __restrict__ members, u32 n_members, const SvSegment* __restrict__ segments,
                                                               SortKey* __restrict__ keys, u32* __restrict__ flag) {
    for (u32 i = blockIdx.x * THREADS + threadIdx.x; i < n_members; i += gridDim.x * THREADS) {
        SvMember const me = members[i];
        if (me.group_size < 2u) continue;
        if (me.group_size > SV_MAX_GROUP || me.group_begin > i || i - me.group_begin >= me.group_size || me.group_size > n_members - me.group_begin) { atomicOr(flag, 2u); continue; }   // (the host refused such a plan)
        SvSegment const mine = sv_load_segment(segments, me.job);
        u32 rank = 0, next = 0;                                         // the members in front of this one; its successor
        bool have_next = false, marked = mine.mark != 0u;
        SvSegment succ = mine;
        for (u32 k = 0; k < me.group_size; ++k) {
            u32 const j = me.group_begin + k;
            if (j == i) continue;
            SvSegment const other = sv_load_segment(segments, members[j].job);
            marked = marked || other.mark != 0u;
            if (sv_member_less(other, j, mine, i)) ++rank;
            else if (!have_next || sv_member_less(other, j, succ, next)) { succ = other; next = j; have_next = true; }
        }
        if (marked || !have_next) continue;                             // (a marked segment raised the flag in sv_extract; the last member has no successor)
        sv_store_key(keys, me.key_off + rank, sv_junction_key(mine, succ));      // (rank < group_size - 1: a successor exists)
    }
}

// ------------------------------------------------------------------------------------------------ the break flags and the second keys
__global__ void __launch_bounds__(THREADS) sv_coarse_flags_kernel(const SortKey* __restrict__ sorted, u64 n, u32 max_distance, u32* __restrict__ flags) {
    for (u64 i = (u64)blockIdx.x * THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * THREADS)
        flags[i] = i > 0 && sv_coarse_break(sv_load_key(sorted, i - 1), sv_load_key(sorted, i), max_distance) ? 1u : 0u;
}
__global__ void __launch_bounds__(THREADS) sv_regroup_kernel(const SortKey* __restrict__ sorted, const u32* __restrict__ groups, u64 n, SortKey* __restrict__ keys2) {
    for (u64 i = (u64)blockIdx.x * THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * THREADS) {
        SortKey const k = sv_load_key(sorted, i);
        sv_store_key(keys2, i, SortKey{(u64)groups[i], (u64)sv_key_q(k) << 32 | (u64)sv_key_pos_a(k)});
    }
}
__global__ void __launch_bounds__(THREADS) sv_fine_flags_kernel(const SortKey* __restrict__ sorted2, u64 n, u32 max_distance, u32* __restrict__ flags) {
    for (u64 i = (u64)blockIdx.x * THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * THREADS) {
        u32 f = 0;
        if (i > 0) {
            SortKey const p = sv_load_key(sorted2, i - 1), k = sv_load_key(sorted2, i);
            f = sv_fine_break((u32)p.hi, (u32)(p.lo >> 32), (u32)k.hi, (u32)(k.lo >> 32), max_distance) ? 1u : 0u;
        }
        flags[i] = f;
    }
}

// ------------------------------------------------------------------------------------------------ the clusters
// ids: the inclusive scan of the fine flags, the cluster of every key of the second order
__global__ void __launch_bounds__(THREADS) sv_cluster_heads_kernel(const u32* __restrict__ ids, u64 n, u32* __restrict__ starts, flx_sv_cluster* __restrict__ clusters) {
    for (u64 i = (u64)blockIdx.x * THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * THREADS) {
        u32 const c = ids[i];
        if (i > 0 && ids[i - 1] == c) continue;
        starts[c] = (u32)i;                                             // (c <= i < n: the ids start at 0 and rise by at most 1)
        clusters[c].pos_a_min = 0xFFFFFFFFu;
        clusters[c].pos_a_max = 0u;
    }
}
__global__ void __launch_bounds__(THREADS) sv_cluster_bounds_kernel(const SortKey* __restrict__ sorted2, const u32* __restrict__ ids, u64 n,
                                                                    flx_sv_cluster* __restrict__ clusters) {
    u64 const rounds = (n + (u64)gridDim.x * THREADS - 1) / ((u64)gridDim.x * THREADS);      // (every lane of a wave takes every round: the shuffles read all)
    for (u64 r = 0; r < rounds; ++r) {
        u64 const i = (r * gridDim.x + blockIdx.x) * THREADS + threadIdx.x;
        bool const valid = i < n;
        u32 const c = valid ? ids[i] : 0xFFFFFFFFu;
        u32 const p = valid ? (u32)sv_load_key(sorted2, i).lo : 0u;
        u32 lo = valid ? p : 0xFFFFFFFFu, hi = p;
        u32 const c0 = (u32)__shfl((int)c, 0);
        if (__all(!valid || c == c0)) {                                 // one cluster in the wave's valid lanes (they are its low lanes)
#pragma unroll
            for (u32 d = 1; d < 64u; d <<= 1) {
                lo = std::min(lo, (u32)__shfl_xor((int)lo, (int)d));
                hi = std::max(hi, (u32)__shfl_xor((int)hi, (int)d));
            }
            if (lane_id() == 0u && valid) { atomicMin(&clusters[c].pos_a_min, lo); atomicMax(&clusters[c].pos_a_max, hi); }
        } else if (valid) {
            atomicMin(&clusters[c].pos_a_min, p);
            atomicMax(&clusters[c].pos_a_max, p);
        }
    }
}
__global__ void __launch_bounds__(THREADS) sv_cluster_fill_kernel(const SortKey* __restrict__ sorted, const SortKey* __restrict__ sorted2,
                                                                  const u32* __restrict__ payload2, const u32* __restrict__ starts, u64 n, u64 n_clusters,
                                                                  flx_sv_cluster* __restrict__ clusters) {
    for (u64 c = (u64)blockIdx.x * THREADS + threadIdx.x; c < n_clusters; c += (u64)gridDim.x * THREADS) {
        u64 const first = starts[c], last = (c + 1 < n_clusters ? (u64)starts[c + 1] : n) - 1;
        u32 const support = (u32)(last - first + 1);
        flx_sv_cluster const bounds = clusters[c];
        SortKey const k = sv_load_key(sorted, payload2[first]);         // (the class is the same in all of a cluster)
        clusters[c] = sv_cluster_of(k, support, bounds.pos_a_min, bounds.pos_a_max, (u32)(sv_load_key(sorted2, first).lo >> 32),
                                    (u32)(sv_load_key(sorted2, first + (support - 1u) / 2u).lo >> 32), (u32)(sv_load_key(sorted2, last).lo >> 32));
    }
}

// MODE 0: count[tile] = the tile's kept clusters. MODE 1: out[index among all kept] = the cluster; count is then the inclusive scan of mode 0's.
template <int MODE>
__global__ void __launch_bounds__(THREADS) sv_compact_kernel(const flx_sv_cluster* __restrict__ clusters, u64 n_clusters, u32 min_support, u32* __restrict__ count,
                                                             flx_sv_cluster* __restrict__ out) {
    __shared__ u32 lds[THREADS / 64u];
    u64 const c0 = (u64)blockIdx.x * TILE + (u64)threadIdx.x * STRIP;
    u32 mask = 0;                                                      // bit i: cluster c0 + i is kept
#pragma unroll
    for (u32 i = 0; i < STRIP; ++i)
        if (c0 + i < n_clusters && clusters[c0 + i].support >= min_support) mask |= 1u << i;
    u32 tile_total;
    u32 const before = block_exclusive_scan((u32)__popc(mask), lds, tile_total);
    if (MODE == 0) {
        if (threadIdx.x == 0) count[blockIdx.x] = tile_total;
        return;
    }
    u64 index = (u64)before + (blockIdx.x > 0 ? count[blockIdx.x - 1] : 0u);
#pragma unroll
    for (u32 i = 0; i < STRIP; ++i)
        if (mask >> i & 1u) out[index++] = clusters[c0 + i];
}

__global__ void __launch_bounds__(THREADS) sv_signatures_kernel(const SortKey* __restrict__ sorted, u64 n, flx_sv_signature* __restrict__ out) {
    for (u64 i = (u64)blockIdx.x * THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * THREADS) out[i] = sv_signature_of(sv_load_key(sorted, i));
}

// ------------------------------------------------------------------------------------------------ launches (each one checked)
int SvDevice::extract(void* stream, const SvJob* d_jobs, u32 n_jobs, const u32* d_words, u32 min_length, SortKey* d_keys, SvSegment* d_segments, u32* d_flag) {
    if (n_jobs == 0) return 0;
    static_assert(sizeof(SvSegment) == 32, "eight u32 fields");
    u32 const blocks = std::min<u32>((n_jobs + THREADS / 64u - 1) / (THREADS / 64u), EXTRACT_GRID_CAP);
    hipLaunchKernelGGL(sv_extract_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, d_jobs, n_jobs, d_words, min_length, d_keys,
                       reinterpret_cast<u32*>(d_segments), d_flag);
    return (int)hipGetLastError();
}
int SvDevice::junctions(void* stream, const SvMember* d_members, u32 n_members, const SvSegment* d_segments, SortKey* d_keys, u32* d_flag) {
    if (n_members == 0) return 0;
    hipLaunchKernelGGL(sv_junctions_kernel, dim3(strided_blocks(n_members, STRIDED_GRID_CAP)), dim3(THREADS), 0, (hipStream_t)stream, d_members, n_members, d_segments, d_keys, d_flag);
    return (int)hipGetLastError();
}
int SvDevice::coarse_flags(void* stream, const SortKey* d_sorted, u64 n, u32 max_distance, u32* d_flags) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(sv_coarse_flags_kernel, dim3(strided_blocks(n, STRIDED_GRID_CAP)), dim3(THREADS), 0, (hipStream_t)stream, d_sorted, n, max_distance, d_flags);
    return (int)hipGetLastError();
}
int SvDevice::regroup(void* stream, const SortKey* d_sorted, const u32* d_groups, u64 n, SortKey* d_keys2) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(sv_regroup_kernel, dim3(strided_blocks(n, STRIDED_GRID_CAP)), dim3(THREADS), 0, (hipStream_t)stream, d_sorted, d_groups, n, d_keys2);
    return (int)hipGetLastError();
}
int SvDevice::fine_flags(void* stream, const SortKey* d_sorted2, u64 n, u32 max_distance, u32* d_flags) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(sv_fine_flags_kernel, dim3(strided_blocks(n, STRIDED_GRID_CAP)), dim3(THREADS), 0, (hipStream_t)stream, d_sorted2, n, max_distance, d_flags);
    return (int)hipGetLastError();
}
int SvDevice::cluster_heads(void* stream, const u32* d_ids, u64 n, u32* d_starts, flx_sv_cluster* d_clusters) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(sv_cluster_heads_kernel, dim3(strided_blocks(n, STRIDED_GRID_CAP)), dim3(THREADS), 0, (hipStream_t)stream, d_ids, n, d_starts, d_clusters);
    return (int)hipGetLastError();
}
int SvDevice::cluster_bounds(void* stream, const SortKey* d_sorted2, const u32* d_ids, u64 n, flx_sv_cluster* d_clusters) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(sv_cluster_bounds_kernel, dim3(strided_blocks(n, STRIDED_GRID_CAP)), dim3(THREADS), 0, (hipStream_t)stream, d_sorted2, d_ids, n, d_clusters);
    return (int)hipGetLastError();
}
int SvDevice::cluster_fill(void* stream, const SortKey* d_sorted, const SortKey* d_sorted2, const u32* d_payload2, const u32* d_starts, u64 n, u64 n_clusters,
                           flx_sv_cluster* d_clusters) {
    if (n_clusters == 0) return 0;
    hipLaunchKernelGGL(sv_cluster_fill_kernel, dim3(strided_blocks(n_clusters, STRIDED_GRID_CAP)), dim3(THREADS), 0, (hipStream_t)stream, d_sorted, d_sorted2, d_payload2, d_starts,
                       n, n_clusters, d_clusters);
    return (int)hipGetLastError();
}
int SvDevice::compact(void* stream, int mode, const flx_sv_cluster* d_clusters, u64 n_clusters, u32 min_support, u32* d_count, flx_sv_cluster* d_out) {
    if (n_clusters == 0) return 0;
    dim3 const grid((u32)((n_clusters + TILE - 1) / TILE)), block(THREADS);
    if (mode == 0) hipLaunchKernelGGL(sv_compact_kernel<0>, grid, block, 0, (hipStream_t)stream, d_clusters, n_clusters, min_support, d_count, d_out);
    else hipLaunchKernelGGL(sv_compact_kernel<1>, grid, block, 0, (hipStream_t)stream, d_clusters, n_clusters, min_support, d_count, d_out);
    return (int)hipGetLastError();
}
int SvDevice::signatures(void* stream, const SortKey* d_sorted, u64 n, flx_sv_signature* d_out) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(sv_signatures_kernel, dim3(strided_blocks(n, STRIDED_GRID_CAP)), dim3(THREADS), 0, (hipStream_t)stream, d_sorted, n, d_out);
    return (int)hipGetLastError();
}

}  // namespace flx
