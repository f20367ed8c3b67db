// Structural-variant calls on the device (the rule: flx_svcall.hpp, run here as it stands; the launches' declarations: flx_svcaller.hpp;
// the object and the C ABI: flx_svcaller_api.cpp). Wave64 integer work, two kernels:
//   svcall_spans      at every add, one wave per counted record (SvcallJob): the lanes stride the record's compacted words by 64 and sum the
//                     lengths of = X D, a shuffle reduces the sums, lane 0 stores the span's key at the job's slot behind the table's
//                     count and sets the add's flag when the span does not end where the host planned. Behind its last record a wave
//                     raises the object's max_span word with one atomicMax to the longest span it saw.
//   svcall_count      at finish, one wave per row: the bounds of the row's cluster from its sequence's length, the window in the sorted
//                     keys by two wave-uniform binary searches over their hi words, then the lanes stride the window and count the spans
//                     that reach hi'; the wave sums the counts and lane 0 builds the row and stores it at the row's index.
// Both stride on by the grid under their caps. No wave waits for another. All stores are plain C++ vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_internal.hpp"
#include "flx_svcaller.hpp"
#include "flx_wave.hpp"

namespace flx {

namespace {
constexpr u32 THREADS = SvcallDevice::THREADS;
constexpr u32 WAVES = SvcallDevice::WAVES;
}  // namespace

// ------------------------------------------------------------------------------------------------ svcall_spans
__global__ void __launch_bounds__(THREADS) svcall_spans_kernel(const SvcallJob* __restrict__ jobs, u32 n, const u32* __restrict__ words, SortKey* __restrict__ keys,
                                                               u32* __restrict__ state) {
    u32 const lane = lane_id();
    u32 const waves = gridDim.x * WAVES;
    u32 longest = 0;                                                     // lane 0: the longest span of this wave's jobs
    for (u64 id = blockIdx.x * WAVES + (threadIdx.x >> 6); id < n; id += waves) {       // (id is wave-uniform)
        SvcallJob const j = jobs[id];
        u64 span = 0;
        for (u32 t = lane; t < j.n_words; t += 64u) {
            u32 const w = words[j.word_off + t];
            if (svcall_op_consumes(w & 15u)) span += w >> 4;
        }
        span = wave_sum(span);
        if (lane == 0u) {
            u64 const re = (u64)j.rs + span;
            SortKey const k = svcall_span_key(j.ref, j.rs, (u32)re);
            reinterpret_cast<ulonglong2*>(keys)[id] = make_ulonglong2(k.hi, k.lo);       // one 16-byte store
            if (re != (u64)j.re) state[1] = 1u;
            else longest = longest > (u32)span ? longest : (u32)span;
        }
    }
    // one atomicMax per wave, behind all its jobs, and only where it can raise the word: the word never falls during a launch, so a
    // stale read costs an atomic that changes nothing and never loses a maximum (with one atomic per record an add of 250 000 short
    // records took 2.84 ms, with this 0.053 ms: profiles/svcaller.txt)
    if (lane == 0u && longest > __atomic_load_n(&state[0], __ATOMIC_RELAXED)) atomicMax(&state[0], longest);
}

// ------------------------------------------------------------------------------------------------ svcall_count
__global__ void __launch_bounds__(THREADS) svcall_count_kernel(const SortKey* __restrict__ sorted, u64 n_spans, u32 max_span, const flx_sv_cluster* __restrict__ clusters,
                                                               const u32* __restrict__ index, u32 n_rows, const u32* __restrict__ lens, SvcallModel model,
                                                               flx_svcall_row* __restrict__ rows) {
    u32 const lane = lane_id();
    u32 const waves = gridDim.x * WAVES;
    auto hi = [&](u64 i) { return sorted[i].hi; };                       // (i < n_spans: svcall_lower_bound asks inside [0, n) only)
    for (u64 w = blockIdx.x * WAVES + (threadIdx.x >> 6); w < n_rows; w += waves) {     // (w is wave-uniform)
        u32 const ci = index[w];
        flx_sv_cluster const c = clusters[ci];
        u32 lo2, hi2;
        svcall_bounds(c, lens[c.ref_a], model.flank, lo2, hi2);
        u64 first, last;
        svcall_window(n_spans, (u32)c.ref_a, lo2, hi2, max_span, hi, first, last);       // (first <= last <= n_spans)
        u64 mine = 0;
        for (u64 k = first + lane; k < last; k += 64u) mine += svcall_span_re(sorted[k]) >= hi2 ? 1u : 0u;
        u64 const span_n = wave_sum(mine);                               // (at most n_spans < 2^32)
        if (lane == 0u) rows[w] = svcall_row(ci, c, (u32)span_n, model);
    }
}

// ------------------------------------------------------------------------------------------------ launches (each one checked)
int SvcallDevice::spans(void* stream, const SvcallJob* d_jobs, u32 n_jobs, const u32* d_words, SortKey* d_keys, u32* d_state) {
    if (n_jobs == 0) return 0;
    u32 const blocks = std::min<u32>((u32)(((u64)n_jobs + WAVES - 1) / WAVES), SPANS_GRID_CAP);
    hipLaunchKernelGGL(svcall_spans_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, d_jobs, n_jobs, d_words, d_keys, d_state);
    return (int)hipGetLastError();
}
int SvcallDevice::count(void* stream, const SortKey* d_sorted, u64 n_spans, u32 max_span, const flx_sv_cluster* d_clusters, const u32* d_index, u32 n_rows, const u32* d_lens,
                        SvcallModel model, flx_svcall_row* d_rows) {
    if (n_rows == 0) return 0;
    u32 const blocks = std::min<u32>((u32)(((u64)n_rows + WAVES - 1) / WAVES), COUNT_GRID_CAP);
    hipLaunchKernelGGL(svcall_count_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, d_sorted, n_spans, max_span, d_clusters, d_index, n_rows, d_lens, model, d_rows);
    return (int)hipGetLastError();
}

}  // namespace flx
