// Device helpers of the tile kernels over position arrays, shared by flx_scan.hip, flx_coverage.hip and flx_pileup.hip: a block of 256
// threads takes one tile of ScanDevice::SCAN_TILE positions, a thread a strip of 16.
#pragma once
#include <hip/hip_runtime.h>

#include "flx_scan.hpp"
#include "flx_wave.hpp"

namespace flx {
namespace {

constexpr u32 TILE = ScanDevice::SCAN_TILE;            // elements per block
constexpr u32 THREADS = 256;
constexpr u32 STRIP = TILE / THREADS;                  // contiguous elements per thread
static_assert(STRIP == 16, "a thread's strip is four 16-byte loads");

// a thread's strip [p0, p0 + 16) of a[0, n): elements past n read as 0
__device__ __forceinline__ void load_strip(const u32* __restrict__ a, u64 n, u64 p0, u32 (&v)[STRIP]) {
    if (p0 + STRIP <= n) {
        const uint4* __restrict__ a4 = reinterpret_cast<const uint4*>(a + p0);      // (p0 is a multiple of 16 elements, the array 256-byte aligned)
#pragma unroll
        for (u32 k = 0; k < STRIP / 4; ++k) { uint4 const x = a4[k]; v[4 * k] = x.x; v[4 * k + 1] = x.y; v[4 * k + 2] = x.z; v[4 * k + 3] = x.w; }
    } else {
#pragma unroll
        for (u32 i = 0; i < STRIP; ++i) v[i] = p0 + i < n ? a[p0 + i] : 0u;
    }
}
__device__ __forceinline__ void store_strip(u32* __restrict__ a, u64 n, u64 p0, u32 const (&v)[STRIP]) {
    if (p0 + STRIP <= n) {
        uint4* __restrict__ a4 = reinterpret_cast<uint4*>(a + p0);
#pragma unroll
        for (u32 k = 0; k < STRIP / 4; ++k) a4[k] = make_uint4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    } else {
#pragma unroll
        for (u32 i = 0; i < STRIP; ++i) if (p0 + i < n) a[p0 + i] = v[i];
    }
}

// exclusive prefix sum over the block's 256 threads; total receives the block's sum. Every thread of the block calls it.
__device__ __forceinline__ u32 block_exclusive_scan(u32 v, u32* lds, u32& total) {
    u32 const incl = wave_inclusive_scan(v), wave = threadIdx.x >> 6;
    if (lane_id() == 63u) lds[wave] = incl;
    __syncthreads();
    u32 base = 0;
    total = 0;
#pragma unroll
    for (u32 w = 0; w < THREADS / 64u; ++w) { u32 const x = lds[w]; if (w < wave) base += x; total += x; }
    __syncthreads();
    return base + incl - v;
}

// the sequence that holds position p: starts[r] <= p < starts[r + 1] (starts has n_refs + 1 entries, p < starts[n_refs])
__device__ __forceinline__ u32 find_ref(const u32* __restrict__ starts, u32 n_refs, u64 p) {
    u32 lo = 0, hi = n_refs;                                           // the answer lies in [lo, hi)
    while (hi - lo > 1u) {
        u32 const mid = lo + (hi - lo) / 2u;
        if ((u64)starts[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace
}  // namespace flx
