// What a stage of the pipeline wants done to its small buffers, as one launch each: clear_stage_kernel in front of a stage sets a short
// list of (pointer, words, value) taken from its kernel arguments (instead of one fill per buffer), publish_stage_kernel behind a stage
// copies a short list of small device arrays into the lane's page-locked mapped result block (instead of one device-to-host copy per
// result and a host wake-up behind each). Both write with ordinary vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_internal.hpp"

namespace flx {

__global__ void __launch_bounds__(256) clear_stage_kernel(ClearList L) {
    u32 const tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (u32 i = 0; i < L.n; ++i) {
        u32* __restrict__ const p = L.item[i].ptr;
        u32 const words = L.item[i].words, value = L.item[i].value;
        for (u32 w = tid; w < words; w += stride) p[w] = value;
    }
}

__global__ void __launch_bounds__(256) publish_stage_kernel(PublishList L) {
    u32 const tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (u32 i = 0; i < L.n; ++i) {
        const u32* __restrict__ const src = L.item[i].src;
        u32* __restrict__ const dst = L.item[i].dst;
        u32 const words = L.item[i].words;
        for (u32 w = tid; w < words; w += stride) dst[w] = src[w];
    }
}

// (a grid for the longest item, at most 256 blocks: the lists are a few words to a few MB)
template <class List>
static u32 stage_blocks(List const& L) {
    u32 longest = 0;
    for (u32 i = 0; i < L.n; ++i) longest = std::max(longest, L.item[i].words);
    return std::max(1u, std::min(256u, (longest + 1023u) / 1024u));
}

int DeviceApi::clear_stage(void* stream, ClearList const& L) {
    if (L.n == 0) return 0;
    hipLaunchKernelGGL(clear_stage_kernel, dim3(stage_blocks(L)), dim3(256), 0, (hipStream_t)stream, L);
    return (int)hipGetLastError();
}

int DeviceApi::publish_stage(void* stream, PublishList const& L) {
    if (L.n == 0) return 0;
    hipLaunchKernelGGL(publish_stage_kernel, dim3(stage_blocks(L)), dim3(256), 0, (hipStream_t)stream, L);
    return (int)hipGetLastError();
}

// The probe of flx_ctx_lane_overlap: one wave that keeps one SIMD busy for a time that `iterations` fixes. Every step needs the one
// before it, nothing is read from memory and nothing is waited for; the one store at the end keeps the chain alive. out: 64 words.
__global__ void __launch_bounds__(64) lane_overlap_kernel(u32 iterations, u32* __restrict__ out) {
    u32 x = threadIdx.x + 1u;
    for (u32 i = 0; i < iterations; ++i) {
        x ^= x >> 7;
        x = x * 0x9E3779B1u + i;
    }
    out[threadIdx.x] = x;
}

int DeviceApi::lane_overlap_probe(void* stream, u32 iterations, u32* d_out) {
    hipLaunchKernelGGL(lane_overlap_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, iterations, d_out);
    return (int)hipGetLastError();
}

}  // namespace flx
