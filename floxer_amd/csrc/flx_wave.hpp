// Wave64 helpers that more than one kernel file uses.
#pragma once
#include <hip/hip_runtime.h>

#include "flx_internal.hpp"

namespace flx {

__device__ __forceinline__ u32 lane_id() { return threadIdx.x & 63u; }

}  // namespace flx
