// The inclusive prefix sum of the side objects on the device (the launches and the host driver of their levels: flx_scan.hpp). Wave64
// integer work on u32 arrays, a block of 256 threads per tile of 4096 elements, a thread a strip of 16:
//   scan_sums    the sum of every tile.
//   scan_apply   the inclusive prefix sum inside every tile, in place, started from the scanned sum of the tiles in front of it. The tile
//                sums are scanned by the same two launches while there are more sums than one tile. No block waits for another block: no
//                look-back, no flags, no spins.
//   sum          into += from (the absorb calls: another object's accumulator, piece by piece).
// All stores are plain C++ vector stores; the arithmetic is modulo 2^32.
#include <hip/hip_runtime.h>

#include "flx_scan.hpp"
#include "flx_scan_dev.hpp"

namespace flx {

__global__ void __launch_bounds__(THREADS) scan_sums_kernel(const u32* __restrict__ a, u64 n, u32* __restrict__ sums) {
    __shared__ u32 lds[THREADS / 64u];
    u32 v[STRIP];
    load_strip(a, n, (u64)blockIdx.x * TILE + (u64)threadIdx.x * STRIP, v);
    u32 s = 0;
#pragma unroll
    for (u32 i = 0; i < STRIP; ++i) s += v[i];
    u32 total;
    (void)block_exclusive_scan(s, lds, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// scanned: the tile sums after their own inclusive scan (tile b starts from scanned[b - 1]); null for an array of one tile
__global__ void __launch_bounds__(THREADS) scan_apply_kernel(u32* __restrict__ a, u64 n, const u32* __restrict__ scanned) {
    __shared__ u32 lds[THREADS / 64u];
    u64 const p0 = (u64)blockIdx.x * TILE + (u64)threadIdx.x * STRIP;
    u32 v[STRIP];
    load_strip(a, n, p0, v);
#pragma unroll
    for (u32 i = 1; i < STRIP; ++i) v[i] += v[i - 1];
    u32 total;
    u32 const before = block_exclusive_scan(v[STRIP - 1], lds, total) + (scanned && blockIdx.x > 0 ? scanned[blockIdx.x - 1] : 0u);
#pragma unroll
    for (u32 i = 0; i < STRIP; ++i) v[i] += before;
    store_strip(a, n, p0, v);
}

__global__ void __launch_bounds__(THREADS) sum_kernel(u32* __restrict__ into, const u32* __restrict__ from, u64 n) {
    u64 const p0 = (u64)blockIdx.x * TILE + (u64)threadIdx.x * STRIP;
    if (p0 >= n) return;
    u32 a[STRIP], b[STRIP];
    load_strip(into, n, p0, a);
    load_strip(from, n, p0, b);
#pragma unroll
    for (u32 i = 0; i < STRIP; ++i) a[i] += b[i];
    store_strip(into, n, p0, a);
}

// ------------------------------------------------------------------------------------------------ launches (each one checked)
static inline u32 tiles_of(u64 n) { return (u32)((n + TILE - 1) / TILE); }

int ScanDevice::scan_sums(void* stream, const u32* d_a, u64 n, u32* d_sums) {
    hipLaunchKernelGGL(scan_sums_kernel, dim3(tiles_of(n)), dim3(THREADS), 0, (hipStream_t)stream, d_a, n, d_sums);
    return (int)hipGetLastError();
}
int ScanDevice::scan_apply(void* stream, u32* d_a, u64 n, const u32* d_scanned) {
    hipLaunchKernelGGL(scan_apply_kernel, dim3(tiles_of(n)), dim3(THREADS), 0, (hipStream_t)stream, d_a, n, d_scanned);
    return (int)hipGetLastError();
}
int ScanDevice::sum(void* stream, u32* d_into, const u32* d_from, u64 n) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(sum_kernel, dim3(tiles_of(n)), dim3(THREADS), 0, (hipStream_t)stream, d_into, d_from, n);
    return (int)hipGetLastError();
}

}  // namespace flx
