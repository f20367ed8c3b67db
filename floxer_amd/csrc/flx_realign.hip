// cigar_realign: a traced path realigned under affine gap costs inside a band around it (the rule: flx_realign.hpp), on CIGAR words and
// DevTraceOuts in HBM as K5 (ed_traceback, flx_device.hip) leaves them. The new words go into a slab of a second buffer and the job's
// DevTraceOut is rewritten, as cigar_left_align does.
//
// One wave per job, wave64, no MFMA.
//   - The band: 64 words per pass, a wave scan of the signed diagonal steps (D +len, I -len), min over the I words and max over the D
//     words; the same pass sums rows, columns and the input's NM and refuses a path that leaves its window or its query.
//   - The DP: rows 0..m in stripes of 64, one row per lane; row i holds the B = hi - lo + 1 band cells c = j - i - lo. Lane l computes
//     cell c at step c + 2 l, so that H and F of the cell above (row i - 1, its cell c + 1) were computed exactly one step earlier: one
//     cross-lane move each per step. E, the H to the left and the diagonal H (what the move brought one step before) stay in the lane.
//     A stripe takes B + 126 steps. The last lane's H and F go into a hand-over row of B entries that lane 0 of the next stripe reads;
//     lane 0 reads entry c + 1 at step c and the last lane writes entry c at step c + 126, so one row serves both and is rewritten in
//     place. It lies in LDS (8 KiB) while B <= 1024 and in front of the job's trace otherwise.
//   - The trace: 4 bits per cell (bits 0-1: H came from 0 diagonal, 1 F, 2 E; bit 2: E extended; bit 3: F extended), eight cells of a
//     row per word, [stripe][c / 8][lane]: lanes that finish a word in the same step store neighbouring words.
//   - The walk back is the wave's, every value wave-uniform: from (m, n) in state H by the rule's ties, words written right to left.
// Cells outside the grid or the band are -2^30; a path so long that a finite value could come near it, or whose trace does not fit
// the job's part of the arena, keeps its words (kept = 1). No scratch; 8 KiB of LDS.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_internal.hpp"
#include "flx_realign.hpp"
#include "flx_wave.hpp"

namespace flx {

namespace {

constexpr int NEG = REALIGN_NEG;

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ u32 uni(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }

struct DpArgs {
    const u8* rseq;       // the window's letter under the path's first column
    const u8* qseq;
    u32* trace;
    int m, n, lo, B, W;   // W: trace words per row
    int a, b, oe, e;
};

// every stripe of the DP; ho_h / ho_f: the hand-over row (B entries each). Returns H[m][n] in every lane.
template <class Ptr>
__device__ __forceinline__ int realign_dp(DpArgs const& A, Ptr ho_h, Ptr ho_f) {
    int const lane = (int)lane_id();
    for (int x = lane; x < A.B; x += 64) { ho_h[x] = NEG; ho_f[x] = NEG; }
    __syncthreads();
    int const stripes = (A.m + 64) / 64, steps = A.B + 126;
    int score = NEG;
    for (int s = 0; s < stripes; ++s) {
        int const i = 64 * s + lane;
        bool const row_ok = i <= A.m;
        u32 const qi = (row_ok && i >= 1) ? A.qseq[i - 1] : 0xFFu;
        int my_h = NEG, my_e = NEG, my_f = NEG;
        int diag = lane == 0 ? ho_h[0] : NEG;
        u32 acc = 0;
        u32* const tr = A.trace + (size_t)s * (size_t)A.W * 64u + (u32)lane;
        for (int t0 = 0; t0 < steps; t0 += 8) {
            // the reference letters of this lane's next eight cells (column j pairs with letter j - 1)
            int const j0 = i + A.lo + t0 - 2 * lane;
            u32 rl[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { int const j = j0 + k; rl[k] = (row_ok && j >= 1 && j <= A.n) ? A.rseq[j - 1] : 0xFEu; }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                int const t = t0 + k, c = t - 2 * lane, j = j0 + k;
                int up_h = __shfl_up(my_h, 1), up_f = __shfl_up(my_f, 1);
                if (lane == 0) {                                       // row 64 s - 1 holds column j at its cell c + 1
                    bool const in = t + 1 < A.B;
                    up_h = in ? ho_h[t + 1] : NEG;
                    up_f = in ? ho_f[t + 1] : NEG;
                }
                bool const active = c >= 0 && c < A.B;
                bool const valid = active && row_ok && j >= 0 && j <= A.n;
                int const e_open = my_h - A.oe, e_ext = my_e - A.e, f_open = up_h - A.oe, f_ext = up_f - A.e;
                int e = max(e_open, e_ext), f = max(f_open, f_ext);
                int const dg = (i >= 1 && j >= 1) ? diag + (qi == rl[k] ? A.a : -A.b) : NEG;
                int h = max(dg, max(e, f));
                u32 code = (h == f ? 1u : h == e ? 2u : 0u) | (e_ext >= e_open ? 4u : 0u) | (f_ext >= f_open ? 8u : 0u);
                if (i == 0 && j == 0) { h = 0; code = 0; }
                if (!valid) { h = NEG; e = NEG; f = NEG; code = 0; }
                if (active) {
                    acc |= code << (4 * (c & 7));
                    if ((c & 7) == 7 || c == A.B - 1) { tr[(size_t)(c >> 3) * 64u] = acc; acc = 0; }
                    if (lane == 63) { ho_h[c] = h; ho_f[c] = f; }
                }
                if (valid && i == A.m && j == A.n) score = h;
                diag = up_h; my_h = h; my_e = e; my_f = f;
            }
        }
        __threadfence_block();                                         // the hand-over row is complete before the next stripe reads it
        __syncthreads();
    }
    return __shfl(score, A.m & 63);
}

}  // namespace

// (four waves per SIMD: 128 VGPRs without scratch; five would spill, and 16 waves of 8 KiB fit a CU's LDS)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) cigar_realign_kernel(const u8* __restrict__ text, const u8* __restrict__ query, const u32* __restrict__ cigar,
                                                           DevTraceOut* trace_out, const DevRealignJob* __restrict__ jobs, u32 n_jobs, int sc_a, int sc_b,
                                                           int sc_o, int sc_e, int sc_w, u32* trace, u32* dst_words, DevRealignStat* __restrict__ stats) {
    __shared__ int lds_ho[2 * REALIGN_LDS_BAND];
    u32 const lane = lane_id();
    for (u32 id = blockIdx.x; id < n_jobs; id += gridDim.x) {
        DevRealignJob const job = jobs[id];
        DevTraceOut const t = trace_out[job.out_index];
        if (t.cigar_len == 0xFFFFFFFFu) {                              // K5 ran out of its slab: it stays marked, the host fails on that
            if (lane == 0) stats[job.out_index] = DevRealignStat{0, 0u, 0, 0, 0u, 0u, 0ull};
            continue;
        }
        const u32* __restrict__ const words = cigar + job.cigar_off + t.cigar_start;
        u32* const dst = dst_words + job.out_off;
        u32 const n_words = uni(t.cigar_len), cap = uni(job.out_cap), begin = uni(t.begin);
        // ---- what the words say: rows, columns, NM, the diagonals visited
        u32 m = 0, n = 0, nm = 0;
        int d = 0, d_min = 0, d_max = 0;
        bool fail = begin > job.n;
        for (u32 base = 0; base < n_words && !fail; base += 64u) {
            bool const active = base + lane < n_words;
            u32 const word = active ? words[base + lane] : 0u;
            u32 const op = word & 15u, len = word >> 4;
            bool const is_eq = op == 7u, is_x = op == 8u, is_i = op == 1u, is_d = op == 2u;
            u32 const rows = (is_eq || is_x || is_i) ? len : 0u, cols = (is_eq || is_x || is_d) ? len : 0u;
            u32 const rows_incl = wave_inclusive_scan(rows), cols_incl = wave_inclusive_scan(cols), err_incl = wave_inclusive_scan(is_eq ? 0u : len);
            u32 const step_incl = wave_inclusive_scan(is_d ? len : is_i ? 0u - len : 0u);      // (two's complement: the signed sum)
            u32 const rows_tot = uni(__shfl(rows_incl, 63)), cols_tot = uni(__shfl(cols_incl, 63));
            // a path that leaves its window or its query, or an op that is none of = X I D - K5 never writes one - is reported like a
            // slab that is too small
            if (rows_tot > job.m - m || cols_tot > job.n - begin - n || __ballot(active && !is_eq && !is_x && !is_i && !is_d)) { fail = true; break; }
            int const at = d + (int)step_incl;
            d_min = min(d_min, wave_min(active && is_i ? at : 0));
            d_max = max(d_max, wave_max(active && is_d ? at : 0));
            d += (int)uni(__shfl(step_incl, 63));
            m += rows_tot; n += cols_tot; nm += uni(__shfl(err_incl, 63));
        }
        if (fail) {
            if (lane == 0) {
                trace_out[job.out_index] = DevTraceOut{t.begin, 0u, 0xFFFFFFFFu, t.pad};
                stats[job.out_index] = DevRealignStat{0, 0u, 0, 0, 0u, 0u, 0ull};
            }
            continue;
        }
        d_min = (int)uni((u32)d_min); d_max = (int)uni((u32)d_max);
        int const lo = d_min - sc_w, hi = d_max + sc_w, B = hi - lo + 1, W = (B + 7) / 8;
        bool const ho_in_lds = (u32)B <= REALIGN_LDS_BAND;
        u64 const stripes = ((u64)m + 64u) / 64u;
        u64 const need = stripes * (u64)W * 64u + (ho_in_lds ? 0u : 2u * (u64)B);
        bool const too_long = ((u64)m + n + 2u) * (u64)max(sc_a, max(sc_b, sc_o + sc_e)) >= (1ull << 29);
        if (too_long || need > job.trace_cap) {
            // ---- kept: the input words are the result
            bool const fits = n_words <= cap;
            if (fits) for (u32 x = lane; x < n_words; x += 64u) dst[x] = words[x];
            if (lane == 0) {
                trace_out[job.out_index] = DevTraceOut{t.begin, 0u, fits ? n_words : 0xFFFFFFFFu, t.pad};
                stats[job.out_index] = DevRealignStat{0, nm, lo, hi, 1u, 0u, 0ull};
            }
            continue;
        }
        // ---- the DP
        u32* const job_trace = trace + job.trace_off;
        const u8* const rseq = text + job.ref_off + begin;
        const u8* const qseq = query + job.q_off;
        DpArgs const A{rseq, qseq, job_trace + (ho_in_lds ? 0u : 2u * (u32)B), (int)m, (int)n, lo, B, W, sc_a, sc_b, sc_o + sc_e, sc_e};
        int score;
        if (ho_in_lds) score = realign_dp(A, &lds_ho[0], &lds_ho[B]);
        else score = realign_dp(A, (int*)job_trace, (int*)job_trace + B);
        score = (int)uni((u32)score);
        // ---- the walk back (the trace words other lanes stored are complete: the fence behind the last stripe)
        int i = (int)m, j = (int)n, state = 0;
        u32 pos = cap, cur_op = 0, cur_len = 0, num_errors = 0;
        auto const flush = [&]() {
            if (!cur_len) return;
            if (pos == 0) { fail = true; return; }
            --pos;
            if (lane == 0) dst[pos] = (cur_len << 4) | cur_op;
        };
        auto const emit = [&](u32 op) {
            if (op == cur_op) ++cur_len;
            else { flush(); cur_op = op; cur_len = 1; }
            if (op != 7u) ++num_errors;
        };
        while ((i > 0 || j > 0) && !fail) {
            int const c = j - i - lo;
            if (c < 0 || c >= B) { fail = true; break; }              // (cannot happen: every cell of an optimal path lies in the band)
            u32 const w = uni(A.trace[((size_t)(i >> 6) * (size_t)W + (size_t)(c >> 3)) * 64u + (u32)(i & 63)]);
            u32 const code = (w >> (4 * (c & 7))) & 15u;
            if (state == 0) {
                u32 const src = code & 3u;
                if (src == 1u) state = 1;
                else if (src == 2u) state = 2;
                else {
                    if (i == 0 || j == 0) { fail = true; break; }
                    emit(uni(qseq[i - 1]) == uni(rseq[j - 1]) ? 7u : 8u);
                    --i; --j;
                }
            } else if (state == 1) {
                if (i == 0) { fail = true; break; }
                emit(1u); --i;
                state = (code & 8u) ? 1 : 0;
            } else {
                if (j == 0) { fail = true; break; }
                emit(2u); --j;
                state = (code & 4u) ? 2 : 0;
            }
        }
        if (!fail) flush();
        u32 const out_len = cap - pos;
        // ---- did the words change
        __threadfence_block();
        bool changed = out_len != n_words;
        if (!fail && !changed)
            for (u32 base = 0; base < n_words; base += 64u) {
                u32 const x = base + lane;
                if (__ballot(x < n_words && dst[pos + x] != words[x])) { changed = true; break; }
            }
        if (lane == 0) {
            trace_out[job.out_index] = DevTraceOut{t.begin, pos, fail ? 0xFFFFFFFFu : out_len, t.pad};
            stats[job.out_index] = DevRealignStat{score, num_errors, lo, hi, 0u, changed ? 1u : 0u, ((u64)m + 1u) * (u64)B};
        }
        __syncthreads();                                               // (the LDS row is free for the next job)
    }
}

int DeviceApi::cigar_realign(void* stream, const u8* d_text, const u8* d_query, const u32* d_cigar, DevTraceOut* d_trace_out, const DevRealignJob* d_jobs,
                             u32 n_jobs, RealignScores const& s, u32* d_trace, u32* d_cigar_out, DevRealignStat* d_stats) {
    if (n_jobs == 0) return 0;
    hipLaunchKernelGGL(cigar_realign_kernel, dim3(std::min(n_jobs, REALIGN_GRID_CAP)), dim3(64), 0, (hipStream_t)stream, d_text, d_query, d_cigar, d_trace_out, d_jobs,
                       n_jobs, s.a, s.b, s.o, s.e, s.w, d_trace, d_cigar_out, d_stats);
    return (int)hipGetLastError();
}

}  // namespace flx
