// K5a cigar_left_align: every traced path's gaps moved to the leftmost column they reach (the rule: flx_leftalign.hpp), on the CIGAR
// words K5 (ed_traceback, flx_device.hip) has just written and the letters in HBM. It is queued on the lane's stream directly behind K5,
// reads K5's DevTraceOut there, writes the normalised words into a second slab of the first slab's layout (the word count can grow by one
// per gap, so the words cannot be rewritten in place) and rewrites the job's DevTraceOut: md_build and cigar_tails behind it read the
// normalised words through the second slab's pointer, with no change to their code.
//
// One wave per job, one lane per CIGAR word, 64 words per pass. The output is a list of finished words in the slab, whose last word is
// never '=', plus an open '=' tail that is not written yet. Wave-uniform values carry from pass to pass: the finished words, the tail's
// columns a gap may still cross (x; the path's first column is never crossed: `first`), the op of the last finished word, both cursors.
//   - A lane that holds a gap finds its letter match length m: the columns in front of it over which seq[c - i] == seq[c - i + L], eight
//     bytes per step, capped by the '=' columns since the last X (nothing else can be crossed). Runs beyond 64 columns are finished by the
//     whole wave, 64 columns per step, as md_build copies long runs.
//   - The tail's length behind word i is a function of the one in front of it: '=' adds its length, X makes it 0, a gap makes it
//     min(m, x) - the gap crosses min(m, x) columns and leaves exactly those behind it. All three are x -> min(a, b + x), closed under
//     composition, so one wave scan of (a, b) pairs gives every gap its shift s_i = min(m_i, E_i + s_(i-1)).
//   - A word that is neither '=' nor crossed emits the '=' that remains in front of it (if any) and itself; an exclusive scan of those
//     counts gives the output offsets.
//   - A gap that crosses its whole '=' run and lands on a gap of its own kind merges with it, has another length and shifts again; an X
//     directly behind an X merges too. Such lanes are found by ballot, and a pass that has one is redone word by word by the whole wave
//     (serial, with the comparisons 64 columns per step); it pops finished words from the slab again where the rule removes them. Paths
//     of K5 need it only where two gaps of one kind are one repeat unit apart.
// No LDS, no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "flx_internal.hpp"
#include "flx_wave.hpp"

namespace flx {

namespace {

__device__ __forceinline__ u64 la_load8(const u8* p) {
    u64 v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
__device__ __forceinline__ u32 sat_add(u32 a, u32 b) { u32 const s = a + b; return s < a ? 0xFFFFFFFFu : s; }

// x -> min(a, b + x), saturating at 2^32 - 1 (no length of a path reaches it)
struct MinPlus { u32 a, b; };
__device__ __forceinline__ MinPlus after(MinPlus later, MinPlus earlier) {
    return MinPlus{min(later.a, sat_add(later.b, earlier.a)), sat_add(later.b, earlier.b)};
}
__device__ __forceinline__ MinPlus wave_inclusive_scan(MinPlus v) {
    u32 const lane = lane_id();
#pragma unroll
    for (u32 d = 1; d < 64u; d <<= 1) {
        MinPlus const below{__shfl_up(v.a, d), __shfl_up(v.b, d)};
        if (lane >= d) v = after(v, below);
    }
    return v;
}

// columns i = 1 .. (at most lim <= c) with p[-i] == p[L - i], one lane's loop; p = seq + c
__device__ __forceinline__ u32 lane_match(const u8* p, u32 c, u32 L, u32 lim) {
    u32 r = 0;
    while (r < lim) {
        if (c < r + 8u) {                                            // a word would begin in front of the sequence: byte by byte
            while (r < lim && p[-(i64)r - 1] == p[(i64)L - (i64)r - 1]) ++r;
            break;
        }
        u64 const x = la_load8(p - r - 8) ^ la_load8(p + L - r - 8);
        if (x) { r += (u32)__builtin_clzll(x) >> 3; break; }
        r += 8;
    }
    return min(r, lim);
}
// the same from column from + 1 on by the whole wave (wave-uniform arguments), 64 columns per step
__device__ __forceinline__ u32 wave_match(const u8* p, u32 L, u32 from, u32 lim) {
    u32 r = from;
    while (r < lim) {
        u32 const i = r + lane_id() + 1u;
        bool const ok = i <= lim && p[-(i64)i] == p[(i64)L - (i64)i];
        u64 const bad = __ballot(!ok);
        if (bad) { r += (u32)__builtin_ctzll(bad); break; }
        r += 64u;
    }
    return min(r, lim);
}

}  // namespace

__global__ void __launch_bounds__(64) cigar_left_align_kernel(const u8* __restrict__ text, const u8* __restrict__ query, const u32* __restrict__ cigar,
                                                              DevTraceOut* trace_out, const DevLeftAlignJob* __restrict__ jobs, u32 n_jobs, u32* dst_words,
                                                              DevLeftAlignStat* __restrict__ stats) {
    u32 const lane = lane_id();
    u64 const lt_mask = (1ull << lane) - 1ull;
    // (a grid no larger than the job list: a wave takes jobs in turn, as K5's do)
    for (u32 id = blockIdx.x; id < n_jobs; id += gridDim.x) {
        DevLeftAlignJob const job = jobs[id];
        DevTraceOut const t = trace_out[job.out_index];
        if (t.cigar_len == 0xFFFFFFFFu) {                              // K5 ran out of its slab: it stays marked, the host fails on that
            if (lane == 0) stats[job.out_index] = DevLeftAlignStat{0u, 0u, 0u, 0u};
            continue;
        }
        const u8* __restrict__ const rseq = text + job.ref_off;
        const u8* __restrict__ const qseq = query + job.q_off;
        const u32* __restrict__ const words = cigar + job.cigar_off + t.cigar_start;
        u32* const dst = dst_words + job.out_off;
        u32 const cap = job.out_cap;
        // the wave-uniform carries
        u32 ref_pos = t.begin, q_pos = 0, out_n = 0, x = 0, prev_op = 0;
        bool first = false, fail = t.begin > job.n;
        u32 n_gaps = 0, n_moved = 0, ser_letters = 0;
        u32 my_letters = 0;                                            // (per lane, summed at the end)
        for (u32 base = 0; base < t.cigar_len && !fail; base += 64u) {
            bool const active = base + lane < t.cigar_len;
            u32 const word = active ? words[base + lane] : 0u;
            u32 const op = word & 15u, len = word >> 4;
            bool const is_eq = op == 7u, is_x = op == 8u, is_i = op == 1u, is_d = op == 2u, gap = is_i || is_d;
            bool const noneq = active && !is_eq;
            if (base == 0) first = __shfl((int)is_eq, 0) != 0;
            // the cursors in front of every word; a path that leaves its window or its query - K5 never writes one - is reported like a
            // slab that is too small, and so is an op that is none of = X I D
            u32 const ref_len = (is_eq || is_x || is_d) ? len : 0u, q_len = (is_eq || is_x || is_i) ? len : 0u;
            u32 const ref_incl = wave_inclusive_scan(ref_len), q_incl = wave_inclusive_scan(q_len);
            if (__shfl(ref_incl, 63) > job.n - ref_pos || __shfl(q_incl, 63) > job.m - q_pos || __ballot(active && !is_eq && !is_x && !gap)) { fail = true; break; }
            u32 const c = is_d ? ref_pos + ref_incl - ref_len : q_pos + q_incl - q_len;
            const u8* const p = (is_d ? rseq : qseq) + c;
            // '=' columns a gap may cross (the path's first column is not one), and those since the last X in front of every word
            u32 const eqc = is_eq ? len - ((base + lane == 0u) ? 1u : 0u) : 0u;
            u32 const eq_incl = wave_inclusive_scan(eqc);
            u64 const x_mask = __ballot(active && is_x), x_below = x_mask & lt_mask;
            u32 const eq_at_x = __shfl(eq_incl, x_below ? 63 - __builtin_clzll(x_below) : 0);
            u32 const reach = x_below ? eq_incl - eq_at_x : sat_add(x, eq_incl);
            // the letter match length of every gap: 64 columns by its lane, the rest by the wave
            u32 m = 0;
            if (gap) { m = lane_match(p, c, len, min(reach, 64u)); my_letters += m + 1u; }
            u64 long_mask = __ballot(gap && m == 64u && reach > 64u);
            while (long_mask) {
                int const src = __builtin_ctzll(long_mask);
                long_mask &= long_mask - 1ull;
                u32 const l_c = __shfl(c, src), l_len = __shfl(len, src), l_reach = __shfl(reach, src);
                const u8* const l_p = (__shfl((int)is_d, src) ? rseq : qseq) + l_c;
                u32 const l_m = wave_match(l_p, l_len, 64u, l_reach);
                if ((int)lane == src) { m = l_m; my_letters += l_m - 64u; }
            }
            // the tail behind every word, and so every gap's shift
            MinPlus const f = wave_inclusive_scan(is_eq ? MinPlus{0xFFFFFFFFu, eqc} : noneq ? MinPlus{gap ? m : 0u, 0u} : MinPlus{0xFFFFFFFFu, 0u});
            u32 const tail_after = min(f.a, sat_add(f.b, x));
            u32 const tail_before_up = __shfl_up(tail_after, 1);
            u32 const A = lane ? tail_before_up : x;
            u32 const s = gap ? min(m, A) : 0u;
            u64 const noneq_mask = __ballot(noneq), noneq_below = noneq_mask & lt_mask;
            bool const first_group = first && !noneq_below;            // the '=' in front of this word begins the path
            u32 const e_len = noneq ? A - s + (first_group ? 1u : 0u) : 0u;
            u32 const op_below = __shfl(op, noneq_below ? 63 - __builtin_clzll(noneq_below) : 0);
            u32 const op_before = noneq_below ? op_below : prev_op;
            if (!__ballot(noneq && e_len == 0u && op_before == op)) {
                // ---- no word of this pass lands on a word of its own op: all at once
                u32 const emit = noneq ? (e_len ? 2u : 1u) : 0u;
                u32 const emit_incl = wave_inclusive_scan(emit);
                u32 const total = __shfl(emit_incl, 63);
                if (total > cap - out_n) { fail = true; break; }       // (out_n <= cap always)
                if (noneq) {
                    u32 o = out_n + emit_incl - emit;
                    if (e_len) dst[o++] = (e_len << 4) | 7u;
                    dst[o] = word;
                }
                n_gaps += (u32)__popcll(__ballot(active && gap));
                n_moved += (u32)__popcll(__ballot(active && gap && s > 0u));
                out_n += total;
                x = __shfl(tail_after, 63);
                if (noneq_mask) { prev_op = __shfl(op, 63 - __builtin_clzll(noneq_mask)); first = false; }
            } else {
                // ---- word by word, as the rule states it; every value below is wave-uniform. The finished words other lanes wrote are
                // read back here: the stores are complete first
                __threadfence_block();
                u32 const n_here = min(64u, t.cigar_len - base);
                for (u32 i = 0; i < n_here && !fail; ++i) {
                    u32 const w_word = __shfl(word, i), w_op = w_word & 15u, w_len = w_word >> 4;
                    if (w_op == 7u) { x = sat_add(x, __shfl(eqc, i)); continue; }
                    u32 const open = x + (first ? 1u : 0u);
                    if (w_op == 8u) {
                        // (room for what this word writes: nothing when it merges into the X in front, else itself and the open '=')
                        bool const joins = !open && prev_op == 8u;
                        if (!joins && (open ? 2u : 1u) > cap - out_n) { fail = true; break; }
                        if (open) { dst[out_n++] = (open << 4) | 7u; dst[out_n++] = w_word; }
                        else if (joins) dst[out_n - 1u] += w_len << 4;
                        else dst[out_n++] = w_word;
                        x = 0; first = false; prev_op = 8u;
                        continue;
                    }
                    bool const w_d = w_op == 2u;
                    const u8* const seq = w_d ? rseq : qseq;
                    u32 cc = __shfl(c, i), L = w_len, shift = 0;
                    bool merged = false;
                    for (;;) {
                        if (x) {
                            u32 const got = wave_match(seq + cc, L, 0u, x);
                            ser_letters += got + 1u;
                            x -= got; cc -= got; shift += got;
                        }
                        if (x || first || out_n == 0u || prev_op != w_op) break;
                        // the '=' run is crossed whole and a gap of this kind lies in front: they merge, and what lies in front of that
                        // becomes the previous word again
                        u32 const g = dst[--out_n];
                        L += g >> 4; cc -= g >> 4; merged = true;
                        prev_op = 0;
                        if (out_n) {
                            u32 const v = dst[out_n - 1u];
                            if ((v & 15u) == 7u) {
                                --out_n;
                                x = v >> 4;
                                if (out_n == 0u) { first = true; --x; }
                                else prev_op = dst[out_n - 1u] & 15u;
                            } else prev_op = v & 15u;
                        }
                    }
                    u32 const left = x + (first ? 1u : 0u);
                    if ((left ? 2u : 1u) > cap - out_n) { fail = true; break; }      // (after the pops: the gap and the '=' left in front of it)
                    if (left) dst[out_n++] = (left << 4) | 7u;
                    dst[out_n++] = (L << 4) | w_op;
                    x = shift; first = false; prev_op = w_op;
                    ++n_gaps;
                    if (shift || merged) ++n_moved;
                }
            }
            ref_pos += __shfl(ref_incl, 63);
            q_pos += __shfl(q_incl, 63);
        }
        u32 const open = x + (first ? 1u : 0u);
        if (!fail && open) {
            if (out_n == cap) fail = true;
            else { if (lane == 0) dst[out_n] = (open << 4) | 7u; ++out_n; }
        }
        u32 const letters = __shfl(wave_inclusive_scan(my_letters), 63) + ser_letters;
        if (lane == 0) {
            trace_out[job.out_index] = DevTraceOut{t.begin, 0u, fail ? 0xFFFFFFFFu : out_n, t.pad};
            stats[job.out_index] = DevLeftAlignStat{t.cigar_len, letters, n_gaps, n_moved};
        }
    }
}

int DeviceApi::cigar_left_align(void* stream, const u8* d_text, const u8* d_query, const u32* d_cigar, DevTraceOut* d_trace_out, const DevLeftAlignJob* d_jobs,
                                u32 n_jobs, u32* d_cigar_out, DevLeftAlignStat* d_stats) {
    if (n_jobs == 0) return 0;
    hipLaunchKernelGGL(cigar_left_align_kernel, dim3(std::min(n_jobs, LEFT_ALIGN_GRID_CAP)), dim3(64), 0, (hipStream_t)stream, d_text, d_query, d_cigar, d_trace_out, d_jobs,
                       n_jobs, d_cigar_out, d_stats);
    return (int)hipGetLastError();
}

}  // namespace flx
