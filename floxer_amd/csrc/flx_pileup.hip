// Allele pileup on the device (the rule: flx_pileup.hpp; the object and the C ABI: flx_pileup_api.cpp). Wave64 integer work on seven u32
// planes of `stride` entries each over the unpadded concatenation of the sequences (DEPTH, DEL, A, C, G, T, INS):
//   pileup_add     one wave per counted record, 64 CIGAR words per pass: two wave prefix sums, over the reference-consuming and over the
//                  query-consuming lengths, each with a wave-uniform carry between passes, give every word its first position and its
//                  first row of the oriented sequence. DEPTH (= and X) and DEL (D) are difference arrays: +1 at a word's first column, -1
//                  behind its last; neighbouring words of the same plane share a boundary whose +1 and -1 cancel, and neither is issued
//                  (an = next to a D does not cancel: different planes). The lane of an X word walks its columns and adds 1 to the plane
//                  of the read's letter there (ranks 1..4); the lane of an I word adds 1 to INS at its anchor, the column in front of it,
//                  or the word's own position when no reference-consuming column precedes it in the record (a third wave-uniform carry).
//   pileup_sites   over SCAN_TILE positions per block, behind the scans of DEPTH and DEL: mode 0 counts the tile's sites, the counts are
//                  scanned with the same scan (flx_scan.hip), mode 1 writes the sites in position order.
// All adds are device-scope integer atomicAdd, all stores plain C++ vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_scan_dev.hpp"
#include "flx_pileup.hpp"

namespace flx {

// ------------------------------------------------------------------------------------------------ pileup_add
__global__ void __launch_bounds__(THREADS) pileup_add_kernel(const PileupJob* __restrict__ jobs, u32 n_jobs, const u32* __restrict__ words,
                                                             const u8* __restrict__ letters, int* __restrict__ acc, u64 stride) {
    u32 const lane = lane_id();
    u32 const waves = gridDim.x * (THREADS / 64u);
    for (u32 id = blockIdx.x * (THREADS / 64u) + (threadIdx.x >> 6); id < n_jobs; id += waves) {       // (id is wave-uniform)
        PileupJob const job = jobs[id];
        const u8* __restrict__ const seq = letters + job.seq_off;
        u64 pos = job.text_off, row = 0;                               // the wave-uniform carries: position and row behind the last pass,
        bool any_before = false;                                       // and whether a reference-consuming column lies in front of this pass
        for (u32 base = 0; base < job.n_words; base += 64u) {
            u32 const word = base + lane < job.n_words ? words[job.word_off + base + lane] : 0u;      // (op 0 consumes and counts nothing)
            u32 const op = word & 15u, len = word >> 4;
            u32 const cols = (op == 7u || op == 8u || op == 2u) ? len : 0u;
            u32 const rows = (op == 7u || op == 8u || op == 1u || op == 4u) ? len : 0u;
            int const plane = (op == 7u || op == 8u) ? (int)PILEUP_DEPTH : op == 2u ? (int)PILEUP_DEL : -1;      // the word's difference array
            u32 const incl = wave_inclusive_scan(cols), incl_rows = wave_inclusive_scan(rows);
            bool const left = __shfl_up(plane, 1) == plane && lane > 0u, right = __shfl_down(plane, 1) == plane && lane < 63u;
            u64 const first = pos + incl - cols, first_row = row + incl_rows - rows;
            if (plane >= 0) {
                int* const a = acc + (u64)plane * stride;
                if (!left) atomicAdd(&a[first], 1);
                if (!right) atomicAdd(&a[first + len], -1);             // (the host judged the span: at most index `total`)
            }
            if (op == 8u) {
                for (u32 c = 0; c < len; ++c) {                         // (the host judged the rows: they end with the read)
                    u32 const r = seq[first_row + c];
                    if (r >= 1u && r <= 4u) atomicAdd(&acc[(u64)(PILEUP_A + r - 1u) * stride + first + c], 1);
                }
            } else if (op == 1u) {
                bool const preceded = any_before || incl - cols > 0u;   // (a word has at least one column)
                atomicAdd(&acc[(u64)PILEUP_INS * stride + (preceded ? first - 1 : first)], 1);
            }
            u32 const pass_cols = __shfl(incl, 63);
            pos += pass_cols;
            row += __shfl(incl_rows, 63);
            any_before = any_before || pass_cols > 0u;
        }
    }
}

// ------------------------------------------------------------------------------------------------ pileup_sites
// MODE 0: count[tile] = the tile's sites. MODE 1: out[index among all sites] = the site; count is then the inclusive scan of mode 0's.
template <int MODE>
__global__ void __launch_bounds__(THREADS) pileup_sites_kernel(const u32* __restrict__ acc, u64 stride, u64 total, const u32* __restrict__ starts, u32 n_refs,
                                                               PileupThresholds t, u32* __restrict__ count, flx_pileup_site* __restrict__ out) {
    __shared__ u32 lds[THREADS / 64u];
    u64 const p0 = (u64)blockIdx.x * TILE + (u64)threadIdx.x * STRIP;
    u32 depth[STRIP], del[STRIP], best[STRIP], v[STRIP];
    load_strip(acc + (u64)PILEUP_DEPTH * stride, total, p0, depth);
    load_strip(acc + (u64)PILEUP_DEL * stride, total, p0, del);
#pragma unroll
    for (u32 i = 0; i < STRIP; ++i) best[i] = del[i];
    for (u32 k = PILEUP_A; k < PILEUP_PLANES; ++k) {
        load_strip(acc + (u64)k * stride, total, p0, v);
#pragma unroll
        for (u32 i = 0; i < STRIP; ++i) best[i] = std::max(best[i], v[i]);
    }
    u32 mask = 0;                                                      // bit i: position p0 + i is a site
#pragma unroll
    for (u32 i = 0; i < STRIP; ++i)
        if (p0 + i < total && pileup_site_test(depth[i], del[i], best[i], t)) mask |= 1u << i;
    u32 tile_total;
    u32 const before = block_exclusive_scan((u32)__popc(mask), lds, tile_total);
    if (MODE == 0) {
        if (threadIdx.x == 0) count[blockIdx.x] = tile_total;
        return;
    }
    if (mask == 0u) return;
    u64 index = (u64)before + (blockIdx.x > 0 ? count[blockIdx.x - 1] : 0u);
    u32 ref = find_ref(starts, n_refs, p0);                            // (mask != 0: p0 < total)
#pragma unroll
    for (u32 i = 0; i < STRIP; ++i) {
        if (!(mask >> i & 1u)) continue;
        u64 const p = p0 + i;
        while ((u64)starts[ref + 1] <= p) ++ref;                       // (p < total = starts[n_refs]: ref stays below n_refs)
        flx_pileup_site s;
        s.reference_id = (int32_t)ref;
        s.position = (u32)(p - starts[ref]);
        s.depth = depth[i];
        s.del = del[i];
        s.ins = acc[(u64)PILEUP_INS * stride + p];
#pragma unroll
        for (u32 k = 0; k < 4u; ++k) s.alt[k] = acc[(u64)(PILEUP_A + k) * stride + p];
        s.reserved = 0;
        out[index++] = s;
    }
}

// ------------------------------------------------------------------------------------------------ launches (each one checked)
int PileupDevice::add(void* stream, const PileupJob* d_jobs, u32 n_jobs, const u32* d_words, const u8* d_letters, u32* d_acc, u64 stride) {
    if (n_jobs == 0) return 0;
    u32 const blocks = std::min<u32>((n_jobs + THREADS / 64u - 1) / (THREADS / 64u), ADD_GRID_CAP);
    hipLaunchKernelGGL(pileup_add_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, d_jobs, n_jobs, d_words, d_letters, reinterpret_cast<int*>(d_acc), stride);
    return (int)hipGetLastError();
}
int PileupDevice::sites(void* stream, int mode, const u32* d_acc, u64 stride, u64 total, const u32* d_starts, u32 n_refs, PileupThresholds t, u32* d_count,
                        flx_pileup_site* d_out) {
    dim3 const grid((u32)((total + TILE - 1) / TILE)), block(THREADS);
    if (mode == 0) hipLaunchKernelGGL(pileup_sites_kernel<0>, grid, block, 0, (hipStream_t)stream, d_acc, stride, total, d_starts, n_refs, t, d_count, d_out);
    else hipLaunchKernelGGL(pileup_sites_kernel<1>, grid, block, 0, (hipStream_t)stream, d_acc, stride, total, d_starts, n_refs, t, d_count, d_out);
    return (int)hipGetLastError();
}

}  // namespace flx
