// K5c cigar_tails: the chimeric tails of every traced path (the rule: flx_tails.hpp), read off the CIGAR words K5 (ed_traceback,
// flx_device.hip) has just written. Like md_build it is queued on the lane's stream directly behind K5 and reads K5's DevTraceOut there:
// no root CIGAR is walked on the host a second time.
//
// One wave per job, one lane per CIGAR word, 64 words per pass. Wave scans of the words' rows, columns, errors and of the 64-bit score
// rows - w * errors give every lane the values at the boundary behind its word; a wave reduction finds the pass's first maximum and last
// minimum of the score, and the lanes that hold them hand over their (rows, columns, errors, index). Wave-uniform values carry from pass
// to pass: the four running sums and the two running bests. Boundary 0 is their initial value, not a lane. No LDS, no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_internal.hpp"
#include "flx_wave.hpp"

namespace flx {

namespace {

__device__ __forceinline__ i64 wave_max(i64 v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { i64 const o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ i64 wave_min(i64 v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { i64 const o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}

}  // namespace

__global__ void __launch_bounds__(64) cigar_tails_kernel(const u32* __restrict__ cigar, const DevTraceOut* __restrict__ trace_out,
                                                         const DevTailJob* __restrict__ jobs, u32 n_jobs, DevTailOut* __restrict__ out) {
    u32 const lane = lane_id();
    // (a grid no larger than the job list: a wave takes jobs in turn, as K5's do)
    for (u32 id = blockIdx.x; id < n_jobs; id += gridDim.x) {
        DevTailJob const job = jobs[id];
        DevTraceOut const t = trace_out[job.out_index];
        DevTailOut res{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        if (t.cigar_len == 0xFFFFFFFFu) {                              // K5 ran out of its slab: the host fails on that
            if (lane == 0) out[job.out_index] = res;
            continue;
        }
        const u32* __restrict__ words = cigar + job.cigar_off + t.cigar_start;
        i64 const w = (i64)job.w;
        u32 rows = 0, cols = 0, err = 0;                               // the wave-uniform carries: the sums at the boundary behind the last pass
        i64 S = 0;
        i64 G = 0, g = 0;                                              // the running bests, and where they are: boundary 0 to begin with
        u32 max_rows = 0, max_cols = 0, max_err = 0, max_t = 0, min_rows = 0, min_cols = 0, min_err = 0, min_t = 0;
        for (u32 base = 0; base < t.cigar_len; base += 64u) {
            bool const active = base + lane < t.cigar_len;
            u32 const word = active ? words[base + lane] : 0u;
            u32 const op = word & 15u, len = word >> 4;
            u32 const r = (op == 7u || op == 8u || op == 1u) ? len : 0u;
            u32 const c = (op == 7u || op == 8u || op == 2u) ? len : 0u;
            u32 const e = (op == 8u || op == 1u || op == 2u) ? len : 0u;
            u32 const my_rows = rows + wave_inclusive_scan(r), my_cols = cols + wave_inclusive_scan(c), my_err = err + wave_inclusive_scan(e);
            i64 const my_S = S + wave_inclusive_scan((i64)r - w * (i64)e);
            // the pass's first maximum and last minimum over its words (a lane without a word repeats the last boundary: it never counts)
            i64 const pass_max = wave_max(active ? my_S : (i64)0x8000000000000000ll), pass_min = wave_min(active ? my_S : (i64)0x7FFFFFFFFFFFFFFFll);
            if (pass_max > G) {                                        // (strictly: the first boundary that reaches the maximum wins)
                int const src = __builtin_ctzll(__ballot(active && my_S == pass_max));
                G = pass_max;
                max_rows = __shfl(my_rows, src); max_cols = __shfl(my_cols, src); max_err = __shfl(my_err, src); max_t = base + (u32)src + 1u;
            }
            if (pass_min <= g) {                                       // (the last boundary that reaches the minimum wins)
                int const src = 63 - __builtin_clzll(__ballot(active && my_S == pass_min));
                g = pass_min;
                min_rows = __shfl(my_rows, src); min_cols = __shfl(my_cols, src); min_err = __shfl(my_err, src); min_t = base + (u32)src + 1u;
            }
            rows = __shfl(my_rows, 63); cols = __shfl(my_cols, 63); err = __shfl(my_err, 63); S = __shfl(my_S, 63);
        }
        bool const right = G - S > (i64)job.x_drop && rows - max_rows >= job.min_rows;
        bool const left = -g > (i64)job.x_drop && min_rows >= job.min_rows;
        if (!(left && right && min_t >= max_t)) {
            if (left) { res.left_rows = min_rows; res.left_cols = min_cols; res.left_errors = min_err; res.left_words = min_t; }
            if (right) { res.right_rows = rows - max_rows; res.right_cols = cols - max_cols; res.right_errors = err - max_err; res.right_words = t.cigar_len - max_t; }
        }
        if (lane == 0) out[job.out_index] = res;
    }
}

int DeviceApi::cigar_tails(void* stream, const u32* d_cigar, const DevTraceOut* d_trace_out, const DevTailJob* d_jobs, u32 n_jobs, DevTailOut* d_out) {
    if (n_jobs == 0) return 0;
    hipLaunchKernelGGL(cigar_tails_kernel, dim3(std::min(n_jobs, TAILS_GRID_CAP)), dim3(64), 0, (hipStream_t)stream, d_cigar, d_trace_out, d_jobs, n_jobs, d_out);
    return (int)hipGetLastError();
}

}  // namespace flx
