// ed_extend: anchored, score-only extension of a partial alignment's end towards the break (flx_extend_options; the rule:
// flx_partial.hpp). A job starts in one cell and walks query rows and reference symbols away from it (direction +1: the right end of a
// record, -1: its left end, both sequences read backwards). With D[i][j] the unit-cost edit distance between the first i rows and the
// first j symbols (D[0][0] = 0, i <= row_limit, j <= ref_limit), m(i) = min_j D[i][j] and R(d) = max{i : m(i) <= d}, the job scans
// d = 0, 1, .. for the maximum of R(d) - w d and stops at an x-drop, at the last row or at d_max.
//
// D never decreases along a diagonal, so the furthest-reaching wavefront FR(d, kappa) = max{i : D[i][i + kappa] <= d} holds all the
// rule needs: R(d) = max_kappa FR(d, kappa), and the smallest j with D[R(d)][j] = d is R(d) + the smallest kappa that reaches R(d)
// (for the d the scan returns m(R(d)) = d: a smaller m would have given a higher score one step earlier). The recurrence is the
// usual one, FR(d, kappa) = slide(max(FR(d-1, kappa) + 1, FR(d-1, kappa-1), FR(d-1, kappa+1) + 1)), cut to the matrix: a candidate
// beyond min(row_limit, ref_limit - kappa) is pulled back to it (the cell it is pulled to is a neighbour of a cell <= d - 1, or that
// cell itself), a diagonal outside the matrix is "none".
//
// One wave per job. The lanes own the diagonals -d .. d of the current wavefront, in strides of 64 once 2d + 1 > 64. The two live
// wavefronts sit in LDS, 2 D + 5 words each for the launch's largest d_max D (no trace is written: O(d_max) memory per job); the
// four words around a wavefront are set to "none" when it is written, so that nothing is initialised per job. The slide compares
// eight query bytes with eight text bytes per step (both are one rank per byte), backwards for direction -1. R(d), the smallest
// kappa reaching it (one packed 32-bit maximum) and the stop tests are wave-uniform.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_internal.hpp"
#include "flx_wave.hpp"

namespace flx {

namespace {

constexpr int EXT_NONE = -(1 << 30);

__device__ __forceinline__ u64 load8(const u8* p) {
    u64 v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

__device__ __forceinline__ u32 wave_max(u32 v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (u32)__shfl_xor((int)v, d));
    return v;
}

// rows i+1 .. and symbols j+1 .. that are equal, at most n of them. q / t point at row i + 1 / symbol j + 1; q_room: bytes of the
// query pool in front of q (direction -1 reads words that end at q)
__device__ __forceinline__ u32 slide(const u8* q, const u8* t, u32 n, int dir, u64 q_room) {
    u32 r = 0;
    if (dir > 0) {
        while (r < n) {
            u64 const x = load8(q + r) ^ load8(t + r);
            if (x) { r += (u32)__builtin_ctzll(x) >> 3; break; }
            r += 8;
        }
    } else {
        while (r < n) {
            if (q_room < (u64)r + 7u) {                          // a word would begin in front of the pool: byte by byte
                while (r < n && *(q - r) == *(t - r)) ++r;
                break;
            }
            u64 const x = load8(q - r - 7) ^ load8(t - r - 7);
            if (x) { r += (u32)__builtin_clzll(x) >> 3; break; }
            r += 8;
        }
    }
    return min(r, n);
}

}  // namespace

__global__ void __launch_bounds__(64) ed_extend_kernel(const u8* __restrict__ text, const u8* __restrict__ query, const DevExtendJob* __restrict__ jobs,
                                                       u32 n_jobs, u32 lds_d, DevExtendOut* __restrict__ out) {
    extern __shared__ int ext_wavefronts[];
    int const lane = (int)lane_id();
    int const centre = (int)lds_d + 2, stride = 2 * (int)lds_d + 5;
    for (u32 id = blockIdx.x; id < n_jobs; id += gridDim.x) {
        DevExtendJob const job = jobs[id];
        int const I = (int)job.row_limit, J = (int)job.ref_limit, dir = job.direction;
        int const d_max = (int)min(min(job.d_max, job.row_limit), lds_d);     // m(i) <= i: the scan ends at d = row_limit at the latest
        const u8* const q0 = query + job.q_pos;
        const u8* const t0 = text + job.text_pos;
        int best_score = 0, best_d = 0, best_i = 0, best_kappa = 0, reason = 0, d = 0;
        for (;; ++d) {
            int* const cur = ext_wavefronts + (d & 1) * stride + centre;
            const int* const prev = ext_wavefronts + ((d & 1) ^ 1) * stride + centre;
            u32 key = 0;
            for (int kappa = -d + lane; kappa <= d; kappa += 64) {
                int v = EXT_NONE;
                if (kappa <= J && -kappa <= I) {
                    int i = d == 0 ? 0 : max(max(prev[kappa] + 1, prev[kappa - 1]), prev[kappa + 1] + 1);
                    i = min(i, min(I, J - kappa));
                    int const j = i + kappa;
                    u32 const n = (u32)min(I - i, J - j);
                    if (n) i += (int)slide(q0 + (i64)dir * i, t0 + (i64)dir * j, n, dir, job.q_pos - (u64)i);
                    v = i;
                    key = max(key, ((u32)i << 13) | (u32)(8191 - (kappa + 4095)));
                }
                cur[kappa] = v;
            }
            if (lane < 4) cur[(lane & 1 ? -1 : 1) * (d + 1 + (lane >> 1))] = EXT_NONE;
            key = wave_max(key);
            int const R = (int)(key >> 13), kappa_min = 8191 - (int)(key & 8191u) - 4095;
            int const score = R - (int)job.w * d;
            if (d == 0 || score > best_score) { best_score = score; best_d = d; best_i = R; best_kappa = kappa_min; }
            if ((i64)best_score - score > (i64)job.x_drop) { reason = FLX_EXTEND_STOP_XDROP; break; }
            if (R == I) { reason = FLX_EXTEND_STOP_ROWS; break; }
            if (d == d_max) { reason = FLX_EXTEND_STOP_MAX_ERRORS; break; }
            __syncthreads();
        }
        if (lane == 0) out[job.out_index] = DevExtendOut{(u32)best_i, (u32)(best_i + best_kappa), (u32)best_d, (u32)reason, (u32)d, {0u, 0u, 0u}};
        __syncthreads();                                       // (the next job's first wavefront overwrites what other lanes may still read)
    }
}

size_t DeviceApi::extend_lds_bytes(u32 d_max) { return (size_t)2 * (2 * (size_t)d_max + 5) * 4; }

int DeviceApi::extend(void* stream, const u8* d_text, const u8* d_query, const DevExtendJob* d_jobs, u32 n_jobs, u32 lds_d, DevExtendOut* d_out) {
    if (n_jobs == 0) return 0;
    hipLaunchKernelGGL(ed_extend_kernel, dim3(std::min(n_jobs, EXTEND_GRID_CAP)), dim3(64), extend_lds_bytes(lds_d), (hipStream_t)stream, d_text, d_query, d_jobs,
                       n_jobs, lds_d, d_out);
    return (int)hipGetLastError();
}

}  // namespace flx
