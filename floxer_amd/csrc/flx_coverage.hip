// Depth of coverage on the device (the rule: flx_coverage.hpp; the object and the C ABI: flx_coverage_api.cpp). Everything is wave64 integer
// work on one u32 array of (total + 1) entries over the unpadded concatenation of the sequences:
//   coverage_add      one wave per counted record, 64 CIGAR words per pass: a wave prefix sum over the reference-consuming lengths, with a
//                     wave-uniform carry between passes, gives every word its first position; a counted word adds +1 there and -1 behind
//                     its last column (device-scope integer atomicAdd). Neighbouring counted words of a pass (= then X) share a
//                     boundary whose +1 and -1 cancel: neither is issued.
//   (the scan)        the inclusive prefix sum that turns the differences into depths, in place: flx_scan.hip.
//   coverage_heads    a position is a run head when it is the first of a sequence or its depth differs from its predecessor's. Mode 0
//                     counts the heads per tile (all of them, and those that are reported), the counts are scanned with the same scan,
//                     mode 1 writes the positions of all heads, mode 2 writes the reported runs: a run ends where the next head starts.
//   coverage_windows  one segmented reduction for every window size: a lane folds a strip of 16 positions, flushing when a window ends
//                     inside the strip, the wave folds its lanes by window with a segmented scan, the last lane of a window adds the
//                     wave's part to the window (64-bit atomicAdd, atomicMax).
// flx_coverage_absorb adds another object's array with flx_scan.hip's sum.
// All stores are plain C++ vector stores; arithmetic on depths is modulo 2^32 (the differences are i32, their prefix sums never negative).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_coverage.hpp"
#include "flx_scan_dev.hpp"
#include "flx_wave.hpp"

namespace flx {

// ------------------------------------------------------------------------------------------------ coverage_add
__global__ void __launch_bounds__(THREADS) coverage_add_kernel(const CoverageJob* __restrict__ jobs, u32 n_jobs, const u32* __restrict__ words,
                                                               int* __restrict__ acc, u32 count_deletions) {
    u32 const lane = lane_id();
    u32 const waves = gridDim.x * (THREADS / 64u);
    for (u32 id = blockIdx.x * (THREADS / 64u) + (threadIdx.x >> 6); id < n_jobs; id += waves) {       // (id is wave-uniform)
        CoverageJob const job = jobs[id];
        u64 pos = job.text_off;                                        // the wave-uniform carry: the position behind the last pass
        for (u32 base = 0; base < job.n_words; base += 64u) {
            u32 const word = base + lane < job.n_words ? words[job.word_off + base + lane] : 0u;      // (op 0 neither consumes nor counts)
            u32 const op = word & 15u, len = word >> 4;
            u32 const cols = (op == 7u || op == 8u || op == 2u) ? len : 0u;
            bool const counts = op == 7u || op == 8u || (op == 2u && count_deletions != 0u);
            u32 const incl = wave_inclusive_scan(cols);
            bool const left = __shfl_up((int)counts, 1) != 0 && lane > 0u, right = __shfl_down((int)counts, 1) != 0 && lane < 63u;
            if (counts) {
                u64 const first = pos + incl - cols;
                if (!left) atomicAdd(&acc[first], 1);
                if (!right) atomicAdd(&acc[first + len], -1);           // (the host judged the span: at most index `total`)
            }
            pos += __shfl(incl, 63);
        }
    }
}

// ------------------------------------------------------------------------------------------------ run heads
// MODE 0: count_all[tile], count_rep[tile]. MODE 1: heads[index among all heads] = position. MODE 2: out[index among the reported heads]
// = the run that starts there. count_all / count_rep are then the inclusive scans of mode 0's counts.
template <int MODE>
__global__ void __launch_bounds__(THREADS) coverage_heads_kernel(const u32* __restrict__ depth, u64 total, const u32* __restrict__ starts, u32 n_refs,
                                                                 u32 report_zero, u32* __restrict__ count_all, u32* __restrict__ count_rep,
                                                                 u32* __restrict__ heads, u64 n_heads, flx_depth_run* __restrict__ out) {
    __shared__ u32 lds[THREADS / 64u];
    u64 const p0 = (u64)blockIdx.x * TILE + (u64)threadIdx.x * STRIP;
    u32 v[STRIP];
    load_strip(depth, total, p0, v);
    u32 head_mask = 0, rep_mask = 0;                                   // bit i: position p0 + i is a head / a reported head
    u32 first_ref = 0;
    if (p0 < total) {
        u32 ref = find_ref(starts, n_refs, p0);
        first_ref = ref;
        u64 next_start = starts[ref + 1];
        bool at_start = p0 == (u64)starts[ref];
        u32 prev = p0 > 0 ? depth[p0 - 1] : 0u;
#pragma unroll
        for (u32 i = 0; i < STRIP; ++i) {
            u64 const p = p0 + i;
            if (p < total) {
                if (p == next_start) { ++ref; next_start = starts[ref + 1]; at_start = true; }
                if (at_start || v[i] != prev) {
                    head_mask |= 1u << i;
                    if (v[i] != 0u || report_zero != 0u) rep_mask |= 1u << i;
                }
                at_start = false;
                prev = v[i];
            }
        }
    }
    u32 total_all, total_rep;
    u32 const before_all = block_exclusive_scan((u32)__popc(head_mask), lds, total_all);
    u32 const before_rep = block_exclusive_scan((u32)__popc(rep_mask), lds, total_rep);
    if (MODE == 0) {
        if (threadIdx.x == 0) { count_all[blockIdx.x] = total_all; count_rep[blockIdx.x] = total_rep; }
        return;
    }
    u64 index_all = (u64)before_all + (blockIdx.x > 0 ? count_all[blockIdx.x - 1] : 0u);
    u64 index_rep = (u64)before_rep + (blockIdx.x > 0 ? count_rep[blockIdx.x - 1] : 0u);
    u32 ref = first_ref;
#pragma unroll
    for (u32 i = 0; i < STRIP; ++i) {
        if (!(head_mask >> i & 1u)) continue;
        u64 const p = p0 + i;
        if (MODE == 1) heads[index_all] = (u32)p;
        else if (rep_mask >> i & 1u) {
            while ((u64)starts[ref + 1] <= p) ++ref;                   // (p < total = starts[n_refs]: ref stays below n_refs)
            u64 const end = index_all + 1 < n_heads ? (u64)heads[index_all + 1] : total;      // the next sequence's first position is a head
            flx_depth_run run;
            run.reference_id = (int32_t)ref;
            run.depth = v[i];
            run.start = p - starts[ref];
            run.end = end - starts[ref];
            out[index_rep++] = run;
        }
        ++index_all;
    }
}

// ------------------------------------------------------------------------------------------------ windows
namespace {
struct WindowPart { u64 key; unsigned long long sum, covered; u32 max_depth; };

__device__ __forceinline__ void window_flush(CoverageWindowAcc* __restrict__ out, WindowPart const& part) {
    if (part.sum == 0ull) return;                                       // nothing covered: the cleared entry stands
    atomicAdd(&out[part.key].depth_sum, part.sum);
    atomicAdd(&out[part.key].covered, part.covered);
    atomicMax(&out[part.key].max_depth, part.max_depth);
}
}  // namespace

// window: the size, 2^32 for one window per sequence; bases[r]: the windows in front of sequence r
__global__ void __launch_bounds__(THREADS) coverage_windows_kernel(const u32* __restrict__ depth, u64 total, const u32* __restrict__ starts, u32 n_refs,
                                                                   u64 window, const u64* __restrict__ bases, CoverageWindowAcc* __restrict__ out) {
    u32 const lane = lane_id();
    u64 const p0 = (u64)blockIdx.x * TILE + (u64)threadIdx.x * STRIP;  // (a wave's strips are 1024 contiguous positions)
    u32 v[STRIP];
    load_strip(depth, total, p0, v);
    WindowPart part{~0ull, 0ull, 0ull, 0u};
    if (p0 < total) {
        u32 ref = find_ref(starts, n_refs, p0);
        u64 seq_start = starts[ref], seq_end = starts[ref + 1];
        u64 k = (p0 - seq_start) / window;
        part.key = bases[ref] + k;
        u64 window_end = std::min(seq_start + (k + 1) * window, seq_end);
#pragma unroll
        for (u32 i = 0; i < STRIP; ++i) {
            u64 const p = p0 + i;
            if (p < total) {
                if (p == window_end) {                                  // the strip crosses into the next window: hand the finished one over
                    window_flush(out, part);
                    if (p == seq_end) { ++ref; seq_start = seq_end; seq_end = starts[ref + 1]; k = 0; part.key = bases[ref]; }
                    else { ++k; ++part.key; }
                    window_end = std::min(seq_start + (k + 1) * window, seq_end);
                    part.sum = 0; part.covered = 0; part.max_depth = 0;
                }
                part.sum += v[i];
                part.covered += v[i] != 0u ? 1u : 0u;
                part.max_depth = std::max(part.max_depth, v[i]);
            }
        }
    }
    // the lanes' last windows ascend with the lane: a segmented inclusive scan by key, the last lane of a key holds the wave's part
#pragma unroll
    for (u32 d = 1; d < 64u; d <<= 1) {
        u64 const key = __shfl_up(part.key, d);
        unsigned long long const sum = __shfl_up(part.sum, d), covered = __shfl_up(part.covered, d);
        u32 const max_depth = __shfl_up(part.max_depth, d);
        if (lane >= d && key == part.key) { part.sum += sum; part.covered += covered; part.max_depth = std::max(part.max_depth, max_depth); }
    }
    u64 const next_key = __shfl_down(part.key, 1);
    if (part.key != ~0ull && (lane == 63u || next_key != part.key)) window_flush(out, part);
}

// ------------------------------------------------------------------------------------------------ launches (each one checked)
static inline u32 tiles_of(u64 n) { return (u32)((n + TILE - 1) / TILE); }

int CoverageDevice::add(void* stream, const CoverageJob* d_jobs, u32 n_jobs, const u32* d_words, u32* d_acc, u32 count_deletions) {
    if (n_jobs == 0) return 0;
    u32 const blocks = std::min<u32>((n_jobs + THREADS / 64u - 1) / (THREADS / 64u), ADD_GRID_CAP);
    hipLaunchKernelGGL(coverage_add_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, d_jobs, n_jobs, d_words, reinterpret_cast<int*>(d_acc), count_deletions);
    return (int)hipGetLastError();
}
int CoverageDevice::heads(void* stream, int mode, const u32* d_depth, u64 total, const u32* d_starts, u32 n_refs, u32 report_zero, u32* d_count_all,
                          u32* d_count_rep, u32* d_heads, u64 n_heads, flx_depth_run* d_out) {
    dim3 const grid(tiles_of(total)), block(THREADS);
    if (mode == 0) hipLaunchKernelGGL(coverage_heads_kernel<0>, grid, block, 0, (hipStream_t)stream, d_depth, total, d_starts, n_refs, report_zero, d_count_all, d_count_rep, d_heads, n_heads, d_out);
    else if (mode == 1) hipLaunchKernelGGL(coverage_heads_kernel<1>, grid, block, 0, (hipStream_t)stream, d_depth, total, d_starts, n_refs, report_zero, d_count_all, d_count_rep, d_heads, n_heads, d_out);
    else hipLaunchKernelGGL(coverage_heads_kernel<2>, grid, block, 0, (hipStream_t)stream, d_depth, total, d_starts, n_refs, report_zero, d_count_all, d_count_rep, d_heads, n_heads, d_out);
    return (int)hipGetLastError();
}
int CoverageDevice::windows(void* stream, const u32* d_depth, u64 total, const u32* d_starts, u32 n_refs, u64 window, const u64* d_bases, CoverageWindowAcc* d_out) {
    hipLaunchKernelGGL(coverage_windows_kernel, dim3(tiles_of(total)), dim3(THREADS), 0, (hipStream_t)stream, d_depth, total, d_starts, n_refs,
                       window == 0 || window >= COVERAGE_MAX_TOTAL ? COVERAGE_MAX_TOTAL : window, d_bases, d_out);
    return (int)hipGetLastError();
}

}  // namespace flx
