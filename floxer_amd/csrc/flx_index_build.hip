// Index construction on the device for gfx950: suffix array by prefix doubling over rocprim's radix sort and scans, then both BWTs and
// both occurrence tables. The only file of the library that includes rocprim and hipcub.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <utility>

#include "flx_internal.hpp"
#include "flx_wave.hpp"

namespace flx {

// ================================================================================================ suffix array (index construction)
// Prefix doubling with radix sorts: ranks of the first 10 symbols, then h = 10, 20, 40, ...: suffixes sorted by (rank[i], rank[i+h])
// until all ranks differ. A suffix that is a prefix of another sorts first (positions past the end rank 0), as the host's SA-IS
// orders them. 36 bytes of HBM per text symbol while it runs.
__global__ void __launch_bounds__(256) sa_init_kernel(const u8* __restrict__ text, u64 n, u64* __restrict__ keys, u32* __restrict__ sa) {
    u64 const i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 key = 0;
    for (u32 j = 0; j < 10; ++j) key = (key << 3) | (i + j < n ? (u64)text[i + j] + 1u : 0u);
    keys[i] = key;
    sa[i] = (u32)i;
}
__global__ void __launch_bounds__(256) sa_flag_kernel(const u64* __restrict__ keys, u64 n, u32* __restrict__ flags) {
    u64 const j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    flags[j] = (j == 0 || keys[j] != keys[j - 1]) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) sa_rank_kernel(const u32* __restrict__ sa, const u32* __restrict__ r, u64 n, u32* __restrict__ rank) {
    u64 const j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    rank[sa[j]] = r[j];
}
__global__ void __launch_bounds__(256) sa_key_kernel(const u32* __restrict__ sa, const u32* __restrict__ rank, u64 n, u64 h, u64* __restrict__ keys) {
    u64 const j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    u64 const i = sa[j];
    keys[j] = ((u64)rank[i] << 32) | (i + h < n ? (u64)rank[i + h] : 0ull);
}

namespace {
// workspaces of one suffix-array construction (36 bytes per text symbol)
struct SaWork {
    u64 *keys = nullptr, *keys2 = nullptr;
    u32 *sa = nullptr, *sa2 = nullptr, *rank = nullptr, *flags = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    hipError_t alloc(u64 n, hipStream_t s) {
        hipError_t e;
        if ((e = hipMalloc(&keys, n * 8)) != hipSuccess) return e;
        if ((e = hipMalloc(&keys2, n * 8)) != hipSuccess) return e;
        if ((e = hipMalloc(&sa, n * 4)) != hipSuccess) return e;
        if ((e = hipMalloc(&sa2, n * 4)) != hipSuccess) return e;
        if ((e = hipMalloc(&rank, n * 4)) != hipSuccess) return e;
        if ((e = hipMalloc(&flags, n * 4)) != hipSuccess) return e;
        size_t sort_bytes = 0, scan_bytes = 0;
        if ((e = rocprim::radix_sort_pairs(nullptr, sort_bytes, keys, keys2, sa, sa2, (size_t)n, 0u, 64u, s)) != hipSuccess) return e;
        if ((e = rocprim::inclusive_scan(nullptr, scan_bytes, flags, flags, (size_t)n, rocprim::plus<u32>(), s)) != hipSuccess) return e;
        tmp_bytes = std::max(sort_bytes, scan_bytes);
        return hipMalloc(&tmp, tmp_bytes);
    }
    void release() {
        for (void* p : {(void*)keys, (void*)keys2, (void*)sa, (void*)sa2, (void*)rank, (void*)flags, tmp}) if (p) (void)hipFree(p);
        keys = keys2 = nullptr; sa = sa2 = rank = flags = nullptr; tmp = nullptr;
    }
};

// suffix array of d_text[0, n) into w.sa (device)
hipError_t sa_on_device(hipStream_t s, const u8* d_text, u64 n, SaWork& w) {
    hipError_t e;
    unsigned const blocks = (unsigned)((n + 255) / 256);
    u32 top = 0;
    hipLaunchKernelGGL(sa_init_kernel, dim3(blocks), dim3(256), 0, s, d_text, n, w.keys, w.sa);
    for (u64 h = 10;; h *= 2) {
        // sort the suffixes by their keys; ranks = number of distinct keys up to and including each position
        if ((e = rocprim::radix_sort_pairs(w.tmp, w.tmp_bytes, w.keys, w.keys2, w.sa, w.sa2, (size_t)n, 0u, 64u, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(sa_flag_kernel, dim3(blocks), dim3(256), 0, s, w.keys2, n, w.flags);
        if ((e = rocprim::inclusive_scan(w.tmp, w.tmp_bytes, w.flags, w.flags, (size_t)n, rocprim::plus<u32>(), s)) != hipSuccess) return e;
        hipLaunchKernelGGL(sa_rank_kernel, dim3(blocks), dim3(256), 0, s, w.sa2, w.flags, n, w.rank);
        if ((e = hipMemcpyAsync(&top, w.flags + (n - 1), 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        std::swap(w.sa, w.sa2);
        if ((u64)top == n || h >= n) break;                    // all suffixes distinct
        hipLaunchKernelGGL(sa_key_kernel, dim3(blocks), dim3(256), 0, s, w.sa, w.rank, n, h, w.keys);
    }
    return hipGetLastError();
}
}  // namespace

int DeviceApi::suffix_array(int hip_device, const u8* text, u64 n, u32* out) {
    if (n == 0) return 0;
    hipError_t e;
    u8* d_text = nullptr;
    hipStream_t s = nullptr;
    SaWork w;
#define SA_HIP(x) do { e = (x); if (e != hipSuccess) goto done; } while (0)
    SA_HIP(hipSetDevice(hip_device));
    SA_HIP(hipStreamCreate(&s));
    SA_HIP(hipMalloc(&d_text, n));
    SA_HIP(w.alloc(n, s));
    SA_HIP(hipMemcpyAsync(d_text, text, n, hipMemcpyHostToDevice, s));
    SA_HIP(sa_on_device(s, d_text, n, w));
    SA_HIP(hipMemcpyAsync(out, w.sa, n * 4, hipMemcpyDeviceToHost, s));
    SA_HIP(hipStreamSynchronize(s));
    e = hipGetLastError();
done:
    w.release();
    if (d_text) (void)hipFree(d_text);
    if (s) (void)hipStreamDestroy(s);
    return (int)e;
}

// ------------------------------------------------------------------------------------------------ BWT + occurrence blocks on the device
__global__ void __launch_bounds__(256) bwt_kernel(const u8* __restrict__ text, const u32* __restrict__ sa, u64 n, u8* __restrict__ bwt) {
    u64 const i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 const p = sa[i];
    bwt[i] = text[p ? p - 1 : n - 1];
}
__global__ void __launch_bounds__(256) reverse_kernel(const u8* __restrict__ text, u64 n, u8* __restrict__ rev) {
    u64 const i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rev[i] = text[n - 1 - i];
}
// one wave per two 32-position blocks: the three bit-planes by ballot, every block's own symbol counts into cnt[c * nb + b]
__global__ void __launch_bounds__(256) occ_planes_kernel(const u8* __restrict__ bwt, u64 n, u64 nb, OccBlock* __restrict__ blocks, u32* __restrict__ cnt) {
    u64 const pair = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (pair * 2 >= nb) return;
    u32 const lane = lane_id();
    u64 const pos = pair * 64 + lane;
    u32 const sym = pos < n ? bwt[pos] : 7u;
    u64 const p0 = __ballot(sym & 1u), p1 = __ballot(sym & 2u), p2 = __ballot(sym & 4u);
    u32 const half = lane >> 5, l = lane & 31u;                 // lanes 0..31 write block 2*pair, lanes 32..63 block 2*pair + 1
    u64 const b = pair * 2 + half;
    if (b >= nb) return;
    u32 const q0 = (u32)(half ? p0 >> 32 : p0), q1 = (u32)(half ? p1 >> 32 : p1), q2 = (u32)(half ? p2 >> 32 : p2);
    if (l < 5) {
        u32 const m = (l & 1u ? q0 : ~q0) & (l & 2u ? q1 : ~q1) & (l & 4u ? q2 : ~q2);
        cnt[(u64)l * nb + b] = (u32)__popc(m);
    } else if (l < 8) blocks[b].w[l] = l == 5 ? q0 : l == 6 ? q1 : q2;
}
__global__ void __launch_bounds__(256) occ_counts_kernel(const u32* __restrict__ cnt, u64 nb, OccBlock* __restrict__ blocks) {
    u64 const i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb * 5) return;
    u64 const c = i / nb, b = i - c * nb;
    blocks[b].w[c] = cnt[i];
}

// Suffix array, both BWTs and both occurrence tables of text[0, n) on the device; results land in host memory. The counts of the
// symbols 0..4 per block are made absolute by five exclusive scans over the blocks.
int DeviceApi::index_arrays(int hip_device, const u8* text, u64 n, u32* out_sa, u8* out_bwt0, u8* out_bwt1, OccBlock* out_occ0, OccBlock* out_occ1) {
    if (n == 0) return 0;
    hipError_t e;
    u8 *d_text = nullptr, *d_rev = nullptr, *d_bwt = nullptr;
    OccBlock* d_occ = nullptr;
    u32* d_cnt = nullptr;
    hipStream_t s = nullptr;
    SaWork w;
    u64 const nb = n / OCC_BLOCK_POS + 1;
    unsigned const blocks_n = (unsigned)((n + 255) / 256);
    SA_HIP(hipSetDevice(hip_device));
    SA_HIP(hipStreamCreate(&s));
    SA_HIP(hipMalloc(&d_text, n));
    SA_HIP(hipMalloc(&d_rev, n));
    SA_HIP(hipMalloc(&d_bwt, n));
    SA_HIP(hipMalloc(&d_occ, nb * sizeof(OccBlock)));
    SA_HIP(hipMalloc(&d_cnt, nb * 5 * 4));
    SA_HIP(w.alloc(std::max<u64>(n, nb), s));
    {
        size_t need = 0;
        SA_HIP(rocprim::exclusive_scan(nullptr, need, d_cnt, d_cnt, 0u, (size_t)nb, rocprim::plus<u32>(), s));
        if (need > w.tmp_bytes) { (void)hipFree(w.tmp); w.tmp = nullptr; w.tmp_bytes = need; SA_HIP(hipMalloc(&w.tmp, need)); }
    }
    SA_HIP(hipMemcpyAsync(d_text, text, n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(reverse_kernel, dim3(blocks_n), dim3(256), 0, s, d_text, n, d_rev);
    for (int dir = 0; dir < 2; ++dir) {
        const u8* t = dir ? d_rev : d_text;
        SA_HIP(sa_on_device(s, t, n, w));
        if (dir == 0) SA_HIP(hipMemcpyAsync(out_sa, w.sa, n * 4, hipMemcpyDeviceToHost, s));
        hipLaunchKernelGGL(bwt_kernel, dim3(blocks_n), dim3(256), 0, s, t, w.sa, n, d_bwt);
        SA_HIP(hipMemcpyAsync(dir ? out_bwt1 : out_bwt0, d_bwt, n, hipMemcpyDeviceToHost, s));
        hipLaunchKernelGGL(occ_planes_kernel, dim3((unsigned)(((nb + 1) / 2 * 64 + 255) / 256)), dim3(256), 0, s, d_bwt, n, nb, d_occ, d_cnt);
        for (u32 c = 0; c < 5; ++c)
            SA_HIP(rocprim::exclusive_scan(w.tmp, w.tmp_bytes, d_cnt + (u64)c * nb, d_cnt + (u64)c * nb, 0u, (size_t)nb, rocprim::plus<u32>(), s));
        hipLaunchKernelGGL(occ_counts_kernel, dim3((unsigned)((nb * 5 + 255) / 256)), dim3(256), 0, s, d_cnt, nb, d_occ);
        SA_HIP(hipMemcpyAsync(dir ? out_occ1 : out_occ0, d_occ, nb * sizeof(OccBlock), hipMemcpyDeviceToHost, s));
        SA_HIP(hipStreamSynchronize(s));
    }
    e = hipGetLastError();
done:
#undef SA_HIP
    w.release();
    for (void* p : {(void*)d_text, (void*)d_rev, (void*)d_bwt, (void*)d_occ, (void*)d_cnt}) if (p) (void)hipFree(p);
    if (s) (void)hipStreamDestroy(s);
    return (int)e;
}

}  // namespace flx
