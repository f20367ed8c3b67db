// Wave64 helpers that more than one kernel file uses.
#pragma once
#include <hip/hip_runtime.h>

#include "flx_internal.hpp"

namespace flx {

__device__ __forceinline__ u32 lane_id() { return threadIdx.x & 63u; }

// Inclusive prefix sum over the 64 lanes of a wave: lane l receives v[0] + ... + v[l]. Six __shfl_up steps, no LDS; every lane of the
// wave must call it (the shuffles read inactive lanes otherwise). The wave's total is the value of lane 63.
__device__ __forceinline__ u32 wave_inclusive_scan(u32 v) {
    u32 const lane = lane_id();
#pragma unroll
    for (u32 d = 1; d < 64u; d <<= 1) {
        u32 const below = __shfl_up(v, d);
        if (lane >= d) v += below;
    }
    return v;
}
// the same over signed 64-bit values (every shuffle moves two words)
__device__ __forceinline__ i64 wave_inclusive_scan(i64 v) {
    u32 const lane = lane_id();
#pragma unroll
    for (u32 d = 1; d < 64u; d <<= 1) {
        i64 const below = __shfl_up(v, d);
        if (lane >= d) v += below;
    }
    return v;
}
// The sum of v over the 64 lanes of a wave, in every lane: six __shfl_xor steps over 64-bit values, no LDS; every lane of the wave must
// call it.
__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (u32 d = 1; d < 64u; d <<= 1) v += (u64)__shfl_xor((unsigned long long)v, (int)d);
    return v;
}

}  // namespace flx
