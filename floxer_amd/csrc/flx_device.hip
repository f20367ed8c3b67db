// The edit-distance kernels of the seed-and-verify path for gfx950 (MI355X, wave64). No MFMA: bit-parallel edit-distance DP walked as
// skewed anti-diagonals across the lanes of a wave. The other kernel families are in files of their own (the K numbers are DESIGN.md's):
//
//   K0 peq_build      query bytes -> per-64-row equality bit masks (6 symbols), wave ballots                       (this file)
//   index build       suffix array, BWTs, occurrence tables                                                         (flx_index_build.hip)
//   K1 fm_search      search_ng21::search_n per seed (search.cpp:173-188): DFS over the expanded optimum search scheme
//                                                                                             (flx_search.hip; the reference's order: flx_search_ordered.hip)
//   K1b select, K2 fm_locate   anchor selection; index.locate(row) (search.cpp:253, 284) as an SA gather            (flx_select.hip)
//   K3/K4 ed_block    seqan3 edit-distance semi-global DP (alignment.cpp:89-125, 160): score + end column, optional checkpointed trace
//   K5 ed_traceback   trace walk + CIGAR (alignment.cpp:166-180)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "flx_internal.hpp"
#include "flx_myers.hpp"
#include "flx_wave.hpp"

namespace flx {

// ================================================================================================ helpers
__device__ __forceinline__ u32 wave_max_u32(u32 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        u32 const o = (u32)__shfl_xor((int)v, off);
        v = v > o ? v : o;
    }
    return (u32)__builtin_amdgcn_readfirstlane((int)v);
}

// ================================================================================================ K0: Peq planes
// peq[(word * 6) + sym] bit r = (seq[64*word + r] == sym). One wave per 64 query bytes: six ballots.
__global__ void __launch_bounds__(256) peq_build_kernel(const u8* __restrict__ seq, u64 len, u64* __restrict__ peq, u64 n_words) {
    u64 const wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (wave >= n_words) return;
    u64 const pos = wave * 64 + lane_id();
    u32 const sym = pos < len ? seq[pos] : 7u;
#pragma unroll
    for (u32 s = 0; s < 6; ++s) {
        u64 const m = __ballot(sym == s);
        if (lane_id() == s) peq[wave * 6 + s] = m;
    }
}

int DeviceApi::build_peq(void* stream, const u8* d_seq, u64 len, u64* d_peq) {
    u64 const n_words = len / 64 + 2;    // +1 partial word, +1 so that the funnel shift may read word+1
    u64 const threads = n_words * 64;
    hipLaunchKernelGGL(peq_build_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_seq, len,
                       d_peq, n_words);
    return (int)hipGetLastError();
}

// launch shapes of the DP kernels (K3/K4 below): words per lane a kernel is instantiated for (with_words_per_lane dispatches over the same list)
static const u32 kWordsPerLane[] = {1, 2, 3, 4, 5, 6, 8, 13, 25};

// ================================================================================================ K3/K4: edit-distance DP
// Myers/Hyyro bit-vector columns, semi-global (free reference ends), banded, 16 columns per step. One job occupies R = lanes_per_job
// consecutive lanes (its ring); a lane owns W consecutive 64-row words of the column at a time (a word group).
// Only cells on diagonals -k <= col - row <= (n - m) + k can lie on an alignment of the whole query inside the window with at
// most k errors (Ukkonen). The query's 64*W-row word groups g = 0..Lg-1 are therefore only computed for the columns
// [64W*g - k, 64W*(g+1) - 1 + (n-m) + k]; group g runs on lane (g mod R) of the job's R-lane ring, skewed by g steps, and a lane
// moves on to group g+R when its window ends (the host chooses a shape in which the windows of g and g+R do not overlap in time, or
// one whose ring waits: ring_delay). A group that starts late starts from the all-(+1) column, a group whose predecessor has finished
// receives horizontal delta +1: both only over-estimate cells outside the band, every cell on a valid path (and the trace bits of its
// predecessors) stays exact. What a lane hands to the next also carries its group's bottom-row value so that the last group knows
// D[m][c] absolutely.
// A lane takes 16 columns of its group per step (the reference symbols of the block sit in four registers, the carries of 16 columns
// cross to the next lane as one word), so the per-step work (lane shuffle, window tests, start logic) is paid once per 16 columns
// and the only LDS access per column and word is the equality mask. Windows are widened to whole blocks (cells outside the band may
// be computed, from exact or over-estimated inputs: both are over-estimates there); a group keeps going for the block in which the
// next group starts, whose start value D[last row of this group][column before that block] travels with the carries.
// (the jobs of one wave: group `blk` of 64 >> log2_r jobs)
// TRACE (K4): per block-step T = b + g, ring lane and word the block's 16 pairs of carry bits that enter the word from above (one
// u32) and the word's {vp, vn} before the block (one 16-byte slot) are written out (TraceLayout; ed_traceback_wave_kernel recomputes
// any word's trace bits over any block from those), and the last group stores D[m][c] of its columns.
// queue: hand-over slots per job behind the equality masks in LDS (a power of two, or 0: no job of the launch has a ring that waits, ring_delay);
// err: set when a job's delay does not fit the queue (null: the host chose the shape per job and knows it fits)
template <int W, bool TRACE>
__device__ __forceinline__ void ed_block_body(const u8* __restrict__ text, const u64* __restrict__ peq, const DevAlignJob* __restrict__ jobs, u32 n_jobs,
                                              u32 log2_r, DevAlignOut* __restrict__ out, u32 blk, u64* __restrict__ lds_eq,
                                              u64* __restrict__ trace, u16* __restrict__ lastrow, u32 queue, u32* __restrict__ err) {
    // The column step (flx_myers.hpp) in its three-input form, but for the four-word trace kernel: at its 168 registers (three waves per
    // SIMD) that form spills 96 bytes per lane, the plain 64-bit one does not (profiles/myers_bitop3_resources.txt).
    constexpr bool kPlainStep = TRACE && W == 4;
    u32 const lane = lane_id();
    u32 const R = 1u << log2_r;
    u32 const p = lane & (R - 1u);
    u32 const jobs_per_wave = 64u >> log2_r;
    u32 const job_id = blk * jobs_per_wave + (lane >> log2_r);
    bool valid = job_id < n_jobs;
    DevAlignJob job;
    if (valid) job = jobs[job_id];
    else { job.ref_off = 0; job.q_off = 0; job.trace_off = 0; job.n = 0; job.m = 1; job.k = 0; job.out_index = 0; }
    int const n = (int)job.n, m = (int)job.m, k = (int)job.k;
    if (valid && (n == 0 || n + k < m)) {
        // no column at all: all m rows are insertions; fewer columns than m - k: no alignment within k
        if (p == 0u) { DevAlignOut o; o.score = (n == 0 && m <= k) ? (u32)m : 0xFFFFFFFFu; o.end_col = 0u; out[job.out_index] = o; }
        valid = false;
    }
    int const nw = (m + 63) >> 6;
    int const Lg = (nw + W - 1) / W;
    int const band_hi = n - m + k;
    u32 const src_lane = (lane & ~(R - 1u)) | ((lane - 1u) & (R - 1u));
    // the ring's schedule (flx_internal.hpp): group g takes block b at block-step b + g + (g / R) delay
    int delay = valid ? (int)ring_delay((u32)n, (u32)m, (u32)k, (u32)W, R) : 0;
    if (delay > 0 && (u32)delay + 1u > queue) {          // (a shape that does not hold the job: reported, never computed wrongly)
        if (err && p == 0u) atomicOr(err, 1u);
        if (p == 0u) { DevAlignOut o; o.score = 0xFFFFFFFFu; o.end_col = 0u; out[job.out_index] = o; }
        valid = false;
        delay = 0;
    }
    bool const any_delay = __any(delay > 0);
    uint2* __restrict__ const hand = reinterpret_cast<uint2*>(lds_eq + 7u * 64u * W) + (size_t)(lane >> log2_r) * queue;      // this job's hand-over slots
    u32 const qmask = queue - 1u;
    auto offset_of = [&](int gg) { return gg + (gg >> log2_r) * delay; };
#pragma unroll
    for (int w = 0; w < W; ++w) lds_eq[(6u * 64u + lane) * W + w] = 0ull;

    // The query is right-aligned in its Lg groups: `pad` rows in front of row 0 that match every symbol and start with vertical delta 0
    // keep D = 0 (what row 0's boundary is) down to the first real row, and the last real row is bit 63 of every group's last word: the
    // value that travels down (and the score in the last group) follows from the word's carries, no row has to be picked out of a word.
    int const pad = Lg * 64 * W - m;                      // 0 <= pad < 64 W: only group 0 holds padding
    int g = (int)p;
    int b_lo = 0, b_hi = -1, rows_g = 0;
    int above_b_hi = 0;                                   // last block of the group above (its lane may run a later group after that)
    int off_g = 0;                                        // offset_of(g)
    u64 vp[W], vn[W];
    auto enter_group = [&]() {
        int const r0 = max(0, 64 * W * g - pad);
        int const r1 = 64 * W * (g + 1) - pad;
        rows_g = r1 - r0;
        b_lo = max(0, r0 - k) >> 4;
        b_hi = min(n - 1, r1 - 1 + band_hi) >> 4;
        if (g + 1 < Lg) b_hi = max(b_hi, max(0, r1 - k) >> 4);
        above_b_hi = max(min(n - 1, r0 - 1 + band_hi) >> 4, b_lo);      // (group g - 1: rows up to r0, kept going for this group's first block)
        off_g = offset_of(g);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            int const rs = 64 * (g * W + w) - pad;        // real row of the word's bit 0 (negative: that many padding rows first)
            u64 const padmask = rs <= -64 ? ~0ull : rs < 0 ? (1ull << (u32)(-rs)) - 1ull : 0ull;
            i64 const off = (i64)job.q_off + rs;          // pool position of the word's bit 0
#pragma unroll
            for (u32 s = 0; s < 6; ++s) {
                u64 v = 0;
                if (rs > -64) {
                    if (off >= 0) {
                        u64 const a = (u64)off >> 6;
                        u32 const sh = (u32)off & 63u;
                        u64 const lo = peq[a * 6 + s];
                        u64 const hi = peq[(a + 1) * 6 + s];
                        v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
                    } else v = peq[s] << (u32)(-off);     // (the pool starts inside the word: the bits in front of it are padding rows)
                }
                lds_eq[(s * 64u + lane) * W + w] = v | padmask;
            }
            lds_eq[(6u * 64u + lane) * W + w] = padmask;  // symbol 6 (columns past the end of the window) matches nothing but the padding
            vp[w] = ~padmask;
            vn[w] = 0ull;
        }
    };
    bool const has_group = valid && g < Lg;
    if (has_group) enter_group();
    else {
#pragma unroll
        for (int w = 0; w < W; ++w) { vp[w] = ~0ull; vn[w] = 0ull; }
    }
    u32 const my_steps = valid ? (u32)(((n - 1) >> 4) + offset_of(Lg - 1) + 1) : 0u;
    u32 const t_max = wave_max_u32(my_steps);
    const u8* __restrict__ ref = text + job.ref_off;
    u32* __restrict__ carry_out = nullptr;
    ulonglong2* __restrict__ ckpt_out = nullptr;
    if (TRACE) {
        TraceLayout const tl = ckpt_trace_layout(job.n, job.m, job.k, (u32)W, R);
        carry_out = reinterpret_cast<u32*>(reinterpret_cast<ulonglong2*>(trace) + job.trace_off);
        ckpt_out = reinterpret_cast<ulonglong2*>(trace) + job.trace_off + tl.carry_slots;
    }

    u32 cw_out = 0x55555555u;                             // what an idle lane hands down: horizontal +1 in every column
    int botv_out = 0;
    int bot = 0, best = m, best_col = 0;
    // The reference symbols of a block are loaded one block-step ahead, and (TRACE) what a block writes is stored at the start of the
    // lane's next block, in front of that load: the wait for the symbols at the top of a step then only covers memory operations issued a
    // whole block of computation earlier (loads and stores share one counter and come back in order).
    uint4 tq_pre = make_uint4(0, 0, 0, 0);
    int pre_b = -1;                                       // tq_pre holds the symbols of block pre_b of this job (-1: nothing)
    bool pend = false, pend_last = false;                 // TRACE: the carries (and last-row values) of the lane's previous block are still in registers
    u64 pend_slot = 0;
    int pend_b = 0;
    u32 cbits[W];
    u32 rowv[8];                                          // last group: D[m][c] of the block's columns, two per word
    auto flush = [&]() {
        if (TRACE && pend) {
#pragma unroll
            for (int w = 0; w < W; ++w) carry_out[pend_slot + w] = cbits[w];
            if (pend_last && lastrow) {
                // (a job's last-row region starts at a multiple of 16 entries and covers whole blocks: 0xFFFF past column n)
                uint4* __restrict__ dst = reinterpret_cast<uint4*>(lastrow + job.lastrow_off + 16 * (u64)pend_b);
                dst[0] = make_uint4(rowv[0], rowv[1], rowv[2], rowv[3]);
                dst[1] = make_uint4(rowv[4], rowv[5], rowv[6], rowv[7]);
            }
            pend = false;
        }
    };
    for (u32 T = 0; T < t_max; ++T) {
        int b = (int)T - off_g;
        if (has_group && b > b_hi && g + (int)R < Lg) {   // this lane's group is finished: group g + R starts no earlier than now (ring_delay)
            g += (int)R;
            enter_group();
            b = (int)T - off_g;
        }
        u32 cw_in = (u32)__shfl((int)cw_out, (int)src_lane);
        int botv_in = __shfl(botv_out, (int)src_lane);
        if (any_delay) {
            // the last lane of a ring leaves what it handed down at step T - 1 in the job's queue; the first lane, in a later revolution than
            // the group above it, takes what that group handed down `delay` steps before that: the same block of the group above
            if (delay > 0 && p == R - 1u) hand[(T - 1u) & qmask] = make_uint2(cw_out, (u32)botv_out);
            if (delay > 0 && p == 0u && g >= (int)R) { uint2 const h = hand[(T - 1u - (u32)delay) & qmask]; cw_in = h.x; botv_in = (int)h.y; }
        }
        bool const active = has_group && b >= b_lo && b <= b_hi;
        if (active) {
            if (g == 0) { cw_in = 0u; botv_in = 0; }      // the row above the matrix: D = 0 in every column
            else if (b > above_b_hi) cw_in = 0x55555555u;      // the group above has ended (what its lane hands down now belongs to a later group): +1 per column
            if (b == b_lo) bot = botv_in + rows_g;        // column left of the window: all vertical deltas +1 below the group above
            int const bot_start = bot;
            bool const last = g == Lg - 1;
            uint4 tq = tq_pre;
            if (pre_b != b) __builtin_memcpy(&tq, ref + 16 * b, 16);
            u32 quad[4] = {tq.x, tq.y, tq.z, tq.w};
            if (n - 16 * b < 16) myers_patch_symbols(quad, n - 16 * b);      // (the window ends in this block: symbol 6 in the columns past it)
            u32 cw = 0;
            u64 const slot = ((u64)T * R + p) * W;        // this lane's words at this block-step
            flush();
            if (TRACE) {
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    ulonglong2 v;
                    v.x = vp[w];
                    v.y = vn[w];
                    ckpt_out[slot + w] = v;
                    cbits[w] = 0;
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) rowv[q] = 0xFFFFFFFFu;
            }
            if (b < b_hi) { __builtin_memcpy(&tq_pre, ref + 16 * (b + 1), 16); pre_b = b + 1; }
            // The block's 16 columns, in two forms. Only a job's last group looks at its bottom row column by column (the score and its
            // rightmost column; K4: the last row itself): a wave none of whose lanes is in a last group - most block-steps of a launch, the
            // jobs of a wave start together and are of one size class - runs the form without that, takes the group's bottom value across
            // the block from the carries' bit counts, and shifts the outgoing carries into their word instead of placing each pair.
            auto block16 = [&](auto track_tag) {
                constexpr bool TRACK = decltype(track_tag)::value;
                // (the block's inputs through an empty asm: values of this form alone. Otherwise the compiler computes what the two forms have in
                // common - sixteen columns' symbols, addresses, carry bits, end-of-window tests - once, in front of the branch, and keeps it all
                // in registers through the block: 186 of them for one word per lane instead of 79)
                u32 qv[4] = {quad[0], quad[1], quad[2], quad[3]};
                u32 cwi = cw_in;
                int bb = b;
                asm volatile("" : "+v"(qv[0]), "+v"(qv[1]), "+v"(qv[2]), "+v"(qv[3]), "+v"(cwi), "+v"(bb));
                u32 acc = 0, acc_hn = 0;                  // (the form that does not track: the hp bits in acc, the hn bits in acc_hn)
                if (TRACE) cbits[0] = cwi;                // (what enters the first word from above is the incoming carry word itself)
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    __builtin_amdgcn_sched_barrier(0);    // (nothing moves across four columns: the form without comparisons would have all sixteen columns' loads in flight)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        int const j = 4 * qd + i;
                        int const c = 16 * bb + j;
                        u32 const sym = (qv[qd] >> (8 * i)) & 0xFFu;
                        u32 c_hp = (cwi >> (2 * j)) & 1u, c_hn = (cwi >> (2 * j + 1)) & 1u;
                        const u64* __restrict__ eqp = &lds_eq[(sym * 64u + lane) * W];
                        u64 hp_last = 0, hn_last = 0;
#pragma unroll
                        for (int w = 0; w < W; ++w) {
                            if (TRACE && w > 0) cbits[w] |= (c_hp | (c_hn << 1)) << (2 * j);
                            u64 hp, hn;
                            if constexpr (kPlainStep) myers_step_u64(eqp[w], vp[w], vn[w], c_hp, c_hn, hp, hn);
                            else myers_step(eqp[w], vp[w], vn[w], c_hp, c_hn, hp, hn);
                            if (w + 1 < W || TRACK) { c_hp = (u32)(hp >> 63); c_hn = (u32)(hn >> 63); }
                            if (w + 1 == W) { hp_last = hp; hn_last = hn; }
                        }
                        if (TRACK) {
                            acc |= (c_hp | (c_hn << 1)) << (2 * j);
                            bot += (int)c_hp - (int)c_hn;       // the group's last row is its last word's bit 63
                            if (last && c < n && bot <= best) { best = bot; best_col = c + 1; }
                            if (TRACE && c < n) {
                                u32 const v16 = (u32)min(bot, 0xFFFF);
                                rowv[j >> 1] = (j & 1) ? (rowv[j >> 1] & 0xFFFFu) | (v16 << 16) : (rowv[j >> 1] & 0xFFFF0000u) | v16;
                            }
                        } else {
                            // (one instruction per carry bit; the carry word's layout is put together behind the block: myers_carry_word)
                            acc = funnel_up1(acc, (u32)(hp_last >> 32));
                            acc_hn = funnel_up1(acc_hn, (u32)(hn_last >> 32));
                        }
                    }
                }
                if (!TRACK) {
                    bot += (int)__popc(acc) - (int)__popc(acc_hn);
                    acc = myers_carry_word(acc, acc_hn);
                }
                return acc;
            };
            cw = __any(last) ? block16(std::true_type{}) : block16(std::false_type{});
            if (TRACE) { pend = true; pend_last = last; pend_slot = slot; pend_b = b; }
            cw_out = cw;
            botv_out = bot_start;
        } else {
            cw_out = 0x55555555u;
            botv_out = 0;
        }
    }
    flush();
    if (valid && has_group && g == Lg - 1) {
        DevAlignOut o;
        o.score = best <= k ? (u32)best : 0xFFFFFFFFu;
        o.end_col = (u32)best_col;
        out[job.out_index] = o;
    }
}


// A launch is a grid over the groups of jobs, or (n_jobs_dev: the job count is on the device, verification rounds of flx_rounds.hip)
// a fixed grid whose waves take the groups in turn until the count is reached.
// (waves per SIMD the register allocation is held to: what round 3's single-form block had - the two forms of the block made the
// scheduler keep every equality mask of a block in flight, 186 registers for one word per lane)
template <int W>
__global__ void __launch_bounds__(64, (W <= 2 ? 4 : W <= 5 ? 3 : W <= 8 ? 2 : 1)) ed_exists_block_kernel(const u8* __restrict__ text, const u64* __restrict__ peq,
                                                             const DevAlignJob* __restrict__ jobs, u32 n_jobs, u32 log2_r,
                                                             DevAlignOut* __restrict__ out, const u32* __restrict__ n_jobs_dev, u32 queue, u32* __restrict__ err) {
    // LDS: [7 symbols][64 lanes][W words] equality masks; symbol 6 (columns past the end of the window) matches nothing; then `queue`
    // hand-over slots per job of the wave
    extern __shared__ __attribute__((aligned(16))) u64 lds_eq[];
    if (n_jobs_dev) n_jobs = min(n_jobs, *n_jobs_dev);
    u32 const jobs_per_wave = 64u >> log2_r;
    for (u32 blk = blockIdx.x; blk * jobs_per_wave < n_jobs; blk += gridDim.x)
        ed_block_body<W, false>(text, peq, jobs, n_jobs, log2_r, out, blk, lds_eq, nullptr, nullptr, queue, err);
}

// K4: the same body with the checkpointed trace and the last rows written out, one wave per group of jobs
template <int W>
__global__ void __launch_bounds__(64, (W <= 4 ? 3 : W <= 6 ? 2 : 1)) ed_trace_block_kernel(const u8* __restrict__ text, const u64* __restrict__ peq,
                                                            const DevAlignJob* __restrict__ jobs, u32 n_jobs, u32 log2_r,
                                                            u64* __restrict__ trace, DevAlignOut* __restrict__ out, u16* __restrict__ lastrow, u32 queue) {
    extern __shared__ __attribute__((aligned(16))) u64 lds_eq[];
    __builtin_amdgcn_s_setprio(2);                   // (few waves, long chains, 18 KB of LDS each: they go first on a shared SIMD)
    ed_block_body<W, true>(text, peq, jobs, n_jobs, log2_r, out, blockIdx.x, lds_eq, trace, lastrow, queue, nullptr);
}

// the widest band (diagonals - 1 = n - m + 2k) a shape holds: any when every group has a lane; else the one whose ring_delay still fits
// `queue` hand-over slots (three blocks of slack for the roundings of ring_group_blocks; a job beyond it is reported by the kernel)
static u64 shape_width_cap(u32 nw, AlignShape sh) {
    u32 const w = sh.words_per_lane, r = sh.lanes_per_job;
    if ((nw + w - 1) / w <= r) return 0xFFFFFFFFull;
    u64 const no_wait = (u64)64 * w * (r - 1) + r;
    if (sh.queue < 8) return no_wait;
    return no_wait + 16ull * (sh.queue - 5u);
}
u64 DeviceApi::shape_width_cap(u32 nw, AlignShape sh) { return flx::shape_width_cap(nw, sh); }

// n, m, k: the job the shape is for (shape_holding: a job as wide as its class allows)
static AlignShape choose_align_shape_uncached(u32 n, u32 m, u32 k, bool parallel) {
    u32 const nw = (m + 63) / 64;
    i64 const width = (i64)n - (i64)m + 2 * (i64)k;
    // rings that wait (ring_delay): throughput form only; FLX_RING_STRETCH = how much longer than the shortest schedule a
    // job's block-steps may get, in percent (default 135; 100 = round 3's shapes)
    static int const stretch = [] { const char* e = getenv("FLX_RING_STRETCH"); int const v = e ? atoi(e) : 135; return v < 100 ? 100 : v; }();
    bool const may_wait = !parallel && stretch > 100;
    AlignShape best{0, 0};
    u64 best_cost = ~0ull;
    u64 shortest = ~0ull, shortest_key = ~0ull;           // block-steps of the shape round 3 chose (fewest lanes x words among the rings that never wait)
    for (int pass = 0; pass < (may_wait ? 2 : 1); ++pass)
    for (u32 w : kWordsPerLane)
        for (u32 r = 1; r <= 64; r *= 2) {
            u32 const groups = (nw + w - 1) / w;
            bool ok = groups <= r;                        // every group has its own lane
            if (!ok) ok = (i64)64 * w * (r - 1) + r + 1 > width;   // group g + r starts after group g has ended
            u32 delay = 0;
            if (!ok && may_wait && pass == 1) {
                delay = ring_delay(n, m, k, w, r);
                ok = delay + 1u <= RING_QUEUE_MAX;
            }
            if (!ok) continue;
            u64 const steps = ring_steps(n, m, k, w, r);
            if (pass == 0 && may_wait) { u64 const key = (u64)w * r * 1000 + w; if (key < shortest_key) { shortest_key = key; shortest = steps; } continue; }
            // throughput form: cost ~ wave slots consumed (words per lane times lanes reserved), fewer words per lane on ties;
            // parallel form: fewest words per lane first (shortest dependent chain per step, most waves), then fewest lanes.
            // (A cost by instructions issued, r * (35 + 25 w), which prefers four words per lane over one at the same w * r, made
            // the existence tests a third slower: more distinct shapes per round = more launches, and fewer resident waves per CU
            // with the larger LDS tables; measured in round 2, gpurun_out r02u.)
            // Round 4, rings that wait: cost = the block-steps the job's lanes sit through, lanes x steps x words - what the launch issues for
            // the job whether a lane has a block to compute or not - among the shapes whose schedule is at most `stretch` percent of the one round 3 chose
            u64 cost;
            if (may_wait) {
                if (steps * 100 > shortest * (u64)stretch) continue;
                cost = steps * r * (8 * w + 1);
            } else cost = parallel ? (u64)w * 1000 + r : (u64)w * r * 1000 + w;
            if (cost < best_cost) { best_cost = cost; best = AlignShape{w, r, ring_queue_for(delay)}; }
        }
    return best;
}

AlignShape choose_align_shape(u32 n, u32 m, u32 k, bool parallel) {
    u32 const nw = (m + 63) / 64;
    i64 const width = (i64)n - (i64)m + 2 * (i64)k;       // diagonals that matter, minus one
    if (const char* forced = getenv("FLX_FORCE_SHAPE")) {   // "W,R": measurements of one launch shape (scripts/shape_cost.py)
        u32 w = 0, r = 0;
        if (sscanf(forced, "%u,%u", &w, &r) == 2 && w && r) {
            if ((nw + w - 1) / w <= r || (i64)64 * w * (r - 1) + r + 1 > width) return AlignShape{w, r};
            u32 const delay = ring_delay(n, m, k, w, r);
            if (delay + 1u <= RING_QUEUE_MAX) return AlignShape{w, r, ring_queue_for(delay)};
        }
    }
    // the jobs of one verification level repeat a handful of (rows, columns, errors) triples: small direct-mapped memo per thread
    struct Entry { u32 n, m, k; AlignShape shape; bool valid; };
    thread_local Entry memo[2][256] = {};
    Entry& e = memo[parallel ? 1 : 0][(m * 31u + n * 7u + k) & 255u];
    if (e.valid && e.n == n && e.m == m && e.k == k) return e.shape;
    e = Entry{n, m, k, choose_align_shape_uncached(n, m, k, parallel), true};
    return e.shape;
}
u32 align_supported_max_query() { return 25u * 64u * 64u; }

u64 align_trace_slots(u32 n, u32 m, u32 k, AlignShape sh) {
    TraceLayout const tl = ckpt_trace_layout(n, m, k, sh.words_per_lane, sh.lanes_per_job);
    return tl.carry_slots + tl.ckpt_slots;
}

// f(std::integral_constant<int, W>) for the W of kWordsPerLane that equals words_per_lane: a kernel exists for these W only
template <class F, int... Ws>
static int with_words_per_lane(u32 words_per_lane, F&& f, std::integer_sequence<int, Ws...>) {
    int rc = (int)hipErrorInvalidValue;
    (void)((words_per_lane == (u32)Ws && ((rc = f(std::integral_constant<int, Ws>{})), true)) || ...);
    return rc;
}
template <class F>
static int with_words_per_lane(u32 words_per_lane, F&& f) {
    return with_words_per_lane(words_per_lane, f, std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 8, 13, 25>{});
}
static u32 log2_lanes(AlignShape shape) {
    u32 log2_g = 0;
    while ((1u << log2_g) < shape.lanes_per_job) ++log2_g;
    return log2_g;
}
// dynamic LDS of a block kernel: [7 symbols][64 lanes][W words] equality masks, then `queue` hand-over slots per job of the wave
static size_t block_lds_bytes(u32 w, u32 jobs_per_wave, u32 queue) {
    return (size_t)7 * 64 * w * sizeof(u64) + (size_t)jobs_per_wave * queue * sizeof(uint2);
}

// one wave per group of jobs: K4 (trace) or K3 (existence)
template <int W>
static int launch_align(hipStream_t s, const u8* d_text, const u64* d_peq, const DevAlignJob* d_jobs, u32 n_jobs, u32 log2_g, bool trace,
                        u64* d_trace, DevAlignOut* d_out, u16* d_lastrow, u32 queue) {
    u32 const jobs_per_wave = 64u >> log2_g;
    u32 const blocks = (n_jobs + jobs_per_wave - 1) / jobs_per_wave;
    size_t const lds_b = block_lds_bytes(W, jobs_per_wave, queue);
    if (trace) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ed_trace_block_kernel<W>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b);
        hipLaunchKernelGGL((ed_trace_block_kernel<W>), dim3(blocks), dim3(64), lds_b, s, d_text, d_peq, d_jobs, n_jobs, log2_g, d_trace, d_out, d_lastrow, queue);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ed_exists_block_kernel<W>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b);
        hipLaunchKernelGGL((ed_exists_block_kernel<W>), dim3(blocks), dim3(64), lds_b, s, d_text, d_peq, d_jobs, n_jobs, log2_g, d_out, (const u32*)nullptr, queue, (u32*)nullptr);
    }
    return (int)hipGetLastError();
}

// existence tests whose number is on the device (*d_n_jobs, at most max_jobs): a grid of at most `max_waves` waves that take the
// groups of jobs in turn
template <int W>
static int launch_exists_counted(hipStream_t s, const u8* d_text, const u64* d_peq, const DevAlignJob* d_jobs, u32 max_jobs, u32 log2_g, DevAlignOut* d_out,
                                 const u32* d_n_jobs, u32 max_waves, u32 queue, u32* d_err) {
    u32 const jobs_per_wave = 64u >> log2_g;
    u32 const blocks = std::max(1u, std::min((max_jobs + jobs_per_wave - 1) / jobs_per_wave, max_waves));
    size_t const lds_b = block_lds_bytes(W, jobs_per_wave, queue);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ed_exists_block_kernel<W>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b);
    hipLaunchKernelGGL((ed_exists_block_kernel<W>), dim3(blocks), dim3(64), lds_b, s, d_text, d_peq, d_jobs, max_jobs, log2_g, d_out, d_n_jobs, queue, d_err);
    return (int)hipGetLastError();
}
int DeviceApi::align_exists_counted(void* stream, const u8* d_text, const u64* d_peq, const DevAlignJob* d_jobs, u32 max_jobs, const u32* d_n_jobs,
                                    AlignShape shape, u32 max_waves, DevAlignOut* d_out, u32* d_err) {
    if (max_jobs == 0) return 0;
    return with_words_per_lane(shape.words_per_lane, [&](auto w) {
        return launch_exists_counted<decltype(w)::value>((hipStream_t)stream, d_text, d_peq, d_jobs, max_jobs, log2_lanes(shape), d_out, d_n_jobs, max_waves, shape.queue, d_err);
    });
}
// the cheapest shape (parallel: the one with the fewest words per lane) that holds every job of at most nw query words and `width` diagonals
// the shape for a round's size class: a job of nw words whose band is `width` diagonals wide (a window of its own: n - m + 2k = 4k + 1)
AlignShape DeviceApi::shape_holding(u32 nw, i64 width, bool parallel) {
    u32 const m = 64u * nw, k = (u32)(std::max<i64>(width, 1) / 4), n = (u32)((i64)m + std::max<i64>(width, 1) - 2 * (i64)k);
    AlignShape sh = choose_align_shape_uncached(n, m, k, parallel);
    // room for the unions of a cluster's windows: slots for a band a quarter wider than the class's own, when that costs no more than the next size
    if (sh.queue) { u32 const wider = ring_queue_for(ring_delay(n + (u32)(width / 4), m, k, sh.words_per_lane, sh.lanes_per_job) + 3u); if (wider <= RING_QUEUE_MAX) sh.queue = std::max(sh.queue, wider); }
    return sh;
}

int DeviceApi::align(void* stream, const u8* d_text, const u64* d_peq, const DevAlignJob* d_jobs, u32 n_jobs, AlignShape shape, bool trace,
                     u64* d_trace, DevAlignOut* d_out, u16* d_lastrow) {
    if (n_jobs == 0) return 0;
    // (jobs of one launch share its words and lanes, not their delays: the most slots a shape may ask for, for any ring that may wait)
    u32 const queue = RING_QUEUE_MAX;
    return with_words_per_lane(shape.words_per_lane, [&](auto w) {
        return launch_align<decltype(w)::value>((hipStream_t)stream, d_text, d_peq, d_jobs, n_jobs, log2_lanes(shape), trace, d_trace, d_out, d_lastrow, queue);
    });
}

// ------------------------------------------------------------------------------------------------ rightmost minimum of a last row
// One wave per window: the best end column of a window inside a job's column range is the last column with the minimal
// last-row value (alignment.cpp: seqan3 reports the rightmost best end), 1-based like the block kernels' own end column.
__global__ void __launch_bounds__(64) lastrow_min_kernel(const u16* __restrict__ lastrow, const DevRowWindow* __restrict__ windows,
                                                         u32 n_windows, DevAlignOut* __restrict__ out) {
    u32 const id = blockIdx.x;
    if (id >= n_windows) return;
    DevRowWindow const w = windows[id];
    u32 const lane = threadIdx.x & 63u;
    const u16* __restrict__ row = lastrow + w.first;
    u32 best = 0xFFFFu, col = 0;
    // (the first w.skip columns lie in blocks the job's last group never wrote: they count as 0xFFFF unread, so the last-row region
    // needs no fill in front of K4)
    for (u32 c = lane; c < w.n; c += 64u) {
        u32 const v = c < w.skip ? 0xFFFFu : row[c];
        if (v <= best) { best = v; col = c + 1u; }
    }
    // wave reduction on (value ascending, column descending): key = value << 32 | ~column
    u64 key = ((u64)best << 32) | (u64)(0xFFFFFFFFu - col);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        u64 const other = __shfl_xor(key, off);
        key = other < key ? other : key;
    }
    if (lane == 0) {
        u32 const v = (u32)(key >> 32), c = 0xFFFFFFFFu - (u32)key;
        DevAlignOut o;
        o.score = (v != 0xFFFFu && v <= w.k) ? v : 0xFFFFFFFFu;
        o.end_col = c;
        out[w.out_index] = o;
    }
}

int DeviceApi::lastrow_min(void* stream, const u16* d_lastrow, const DevRowWindow* d_windows, u32 n_windows, DevAlignOut* d_out) {
    if (n_windows == 0) return 0;
    hipLaunchKernelGGL(lastrow_min_kernel, dim3(n_windows), dim3(64), 0, (hipStream_t)stream, d_lastrow, d_windows, n_windows, d_out);
    return (int)hipGetLastError();
}

// ================================================================================================ K5: traceback + CIGAR over a checkpointed trace
// One wave walks one job's path from (m, end_col) to row 0 with seqan3's preference up (I) > left (D) > diagonal (=/X). The CIGAR is
// written backwards into the job's slab so that it ends up in forward order without a reversal pass.
// The walk is serial, the recomputation of the trace is not: a path moves up its diagonal and drifts from it by one column per
// indel only, so the (word, 16-column block) windows it is going to cross are known in advance. A round therefore recomputes 64
// windows at once, one per lane: for each of the 8 words at and above the walker the 8 blocks around the columns the path's
// current diagonal crosses in that word (exactly one checkpoint + one carry word + 16 columns each). Then the wave walks: lane l
// looks at cell (i - l, j - l), ballots give the stretch of diagonal moves up to the first indel, and the walk goes on until it
// needs a window the round does not hold (the path drifted further than foreseen, or left the 8 words), which starts the next round
// from where the walker stands. ~20 rounds for a 10-kb path.
// Rows are in K4's coordinates: the query right-aligned in its groups, `pad` rows in front of row 1 (ed_block_body).
constexpr u32 TBW_WORDS = 8, TBW_BLOCKS = 8;     // windows of a round: words x blocks = 64 lanes
constexpr u32 TBW_REF = 1024;                    // reference symbols cached per round (columns)

__global__ void __launch_bounds__(64) ed_traceback_wave_kernel(const u8* __restrict__ text, const u64* __restrict__ peq,
                                                               const u64* __restrict__ trace, const DevTraceJob* __restrict__ jobs,
                                                               u32 n_jobs, u32* __restrict__ cigar, DevTraceOut* __restrict__ out) {
    __shared__ ulonglong2 win[64 * 17];              // [window * 17 + column % 16] = {hp, vp} of the window's word after that column (17: no bank conflicts)
    __shared__ u32 win_valid[64];                    // non-zero: the window was computed
    __shared__ u64 eqm[TBW_WORDS][8];                // equality masks of the round's words by symbol (6, 7: past the window, only the padding rows match)
    __shared__ u8 refs[TBW_REF];                     // reference symbols of columns [ref_base, ref_base + TBW_REF)
    u32 const lane = threadIdx.x & 63u;
    __builtin_amdgcn_s_setprio(2);                   // (short launches that hold much LDS go first on a shared SIMD: they leave sooner)
    // (a grid smaller than the job list: a wave takes jobs in turn, so that a launch holds no more LDS than its grid's waves)
    for (u32 id = blockIdx.x; id < n_jobs; id += gridDim.x) {
    __syncthreads();
    DevTraceJob const job = jobs[id];
    const u8* __restrict__ r = text + job.ref_off;
    u32* __restrict__ slab = cigar + job.cigar_off;
    int const W = (int)job.words_per_lane, R = (int)job.lanes;
    int const n = (int)job.n, m = (int)job.m, k = (int)job.k;
    int const band_hi = n - m + k;
    int const nw = (max(m, 1) + 63) >> 6;
    int const Lg = (nw + W - 1) / W;
    int const pad = Lg * 64 * W - max(m, 1);
    TraceLayout const tl = ckpt_trace_layout(job.n, job.m ? job.m : 1u, job.k, (u32)W, (u32)R);
    int const ring_wait = (int)ring_delay(job.n, job.m ? job.m : 1u, job.k, (u32)W, (u32)R);      // (K4's schedule: block b of group g at block-step b + g + (g / R) wait)
    const u32* __restrict__ carry = reinterpret_cast<const u32*>(reinterpret_cast<const ulonglong2*>(trace) + job.trace_off);
    const ulonglong2* __restrict__ ckpt = reinterpret_cast<const ulonglong2*>(trace) + job.trace_off + tl.carry_slots;

    u32 wpos = job.cigar_cap;
    int i = m, j = (int)job.end_col;                 // wave-uniform walker position
    u32 cur_op = 0xFFu, cur_len = 0;
    bool overflow = false;
    auto emit = [&](u32 op, u32 len) {               // wave-uniform run-length merge; lane 0 stores
        if (len == 0) return;
        if (op == cur_op) { cur_len += len; return; }
        if (cur_len) {
            if (wpos == 0) overflow = true;
            else { --wpos; if (lane == 0) slab[wpos] = (cur_len << 4) | cur_op; }
        }
        cur_op = op;
        cur_len = len;
    };
    // first block of (padded) word w's windows in a round that started on diagonal `diag` (column - row): the path crosses the word's
    // rows at columns 64w - pad + diag .. 64w - pad + 63 + diag (0-based)
    auto first_block = [&](int w, int diag) {
        int const c_lo = 64 * w - pad + diag;
        return (c_lo >= 0 ? c_lo / 16 : -((-c_lo + 15) / 16)) - 1;
    };

    while (i > 0 && !overflow) {
        if (j == 0) { emit(1u, (u32)i); i = 0; break; }                 // only insertions remain
        // ---- a round: windows of words gw_top, gw_top-1, ... around the walker's diagonal
        int const gw_top = (i - 1 + pad) >> 6;
        int const diag = j - i;
        // columns the round can touch: from 64 * TBW_WORDS + 32 below the walker's to 16 * TBW_BLOCKS above it
        int const ref_base = max(0, j - 640) & ~15;
        __syncthreads();                                                // (one wave: orders this round's LDS writes after the last round's reads)
        for (u32 x = lane; x < TBW_REF; x += 64u) { int const c = ref_base + (int)x; refs[x] = c < n ? r[c] : (u8)7; }
        __syncthreads();
        {
            int const w = gw_top - (int)(lane / TBW_BLOCKS);
            u32 valid = 0;
            // equality masks of the word, padding rows included: the lane of the word's first window builds them, for the word's eight
            // windows and for the walk
            if (w >= 0 && lane % TBW_BLOCKS == 0) {
                int const rs = 64 * w - pad;
                u64 const padmask = rs <= -64 ? ~0ull : rs < 0 ? (1ull << (u32)(-rs)) - 1ull : 0ull;
                i64 const off = (i64)job.q_off + rs;
#pragma unroll
                for (u32 sy = 0; sy < 6; ++sy) {
                    u64 v = 0;
                    if (rs > -64) {
                        if (off >= 0) {
                            u64 const a = (u64)off >> 6;
                            u32 const sh = (u32)off & 63u;
                            u64 const lo = peq[a * 6 + sy];
                            u64 const hi = peq[(a + 1) * 6 + sy];
                            v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
                        } else v = peq[sy] << (u32)(-off);
                    }
                    eqm[lane / TBW_BLOCKS][sy] = v | padmask;
                }
                eqm[lane / TBW_BLOCKS][6] = padmask;
                eqm[lane / TBW_BLOCKS][7] = padmask;
            }
            __syncthreads();
            if (w >= 0) {
                int const g = w / W, ww = w - g * W, p = g % R;
                int const b = first_block(w, diag) + (int)(lane % TBW_BLOCKS);
                // the blocks group g is computed for (ed_block_body's enter_group)
                int const r0 = max(0, 64 * W * g - pad), r1 = 64 * W * (g + 1) - pad;
                int const b_lo = max(0, r0 - k) >> 4;
                int b_hi = min(n - 1, r1 - 1 + band_hi) >> 4;
                if (g + 1 < Lg) b_hi = max(b_hi, max(0, r1 - k) >> 4);
                // all 16 columns of the block must be in the symbol cache
                if (b >= b_lo && b <= b_hi && 16 * b >= ref_base && 16 * b + 16 <= ref_base + (int)TBW_REF) {
                    u64 const slot = ((u64)(b + g + (g / R) * ring_wait) * R + p) * W + ww;
                    ulonglong2 const v = ckpt[slot];
                    u64 pv = v.x, mv = v.y;
                    u32 const cw = carry[slot];
#pragma unroll 4
                    for (u32 sidx = 0; sidx < 16u; ++sidx) {
                        u32 const cb = (cw >> (2u * sidx)) & 3u;
                        u32 const rsym = refs[16 * b + (int)sidx - ref_base] & 7u;
                        u64 hp, hn;
                        myers_step(eqm[lane / TBW_BLOCKS][rsym], pv, mv, cb & 1u, cb >> 1, hp, hn);
                        ulonglong2 o;
                        o.x = hp;
                        o.y = pv;
                        win[lane * 17u + sidx] = o;
                    }
                    valid = 1u;
                }
            }
            win_valid[lane] = valid;
        }
        __syncthreads();
        // ---- walk while the round's windows cover the walker
        bool progressed = false;
        while (i > 0 && !overflow) {
            if (j == 0) break;
            // lane l looks at cell (i - l, j - l)
            bool const in_range = (int)lane < i && (int)lane < j;
            bool have = false, up = false, left = false, same = false;
            if (in_range) {
                int const ci = i - (int)lane, cj = j - (int)lane;
                int const w = (ci - 1 + pad) >> 6;
                u32 const bit = (u32)(ci - 1 + pad) & 63u;
                int const c = cj - 1;
                int const wslot = gw_top - w;
                int const bslot = (c >> 4) - first_block(w, diag);
                int const col = c - ref_base;
                if (wslot < (int)TBW_WORDS && bslot >= 0 && bslot < (int)TBW_BLOCKS && col >= 0) {
                    u32 const slot = (u32)wslot * TBW_BLOCKS + (u32)bslot;
                    if (win_valid[slot]) {
                        have = true;
                        ulonglong2 const v = win[slot * 17u + ((u32)c & 15u)];
                        up = (v.y >> bit) & 1ull;
                        left = (v.x >> bit) & 1ull;
                        u32 const rsym = refs[col] & 7u;
                        same = rsym < 6u && ((eqm[wslot][rsym] >> bit) & 1ull);
                    }
                }
            }
            u64 const m_range = __ballot(in_range);
            u64 const m_have = __ballot(have);
            u64 const m_miss = m_range & ~m_have;
            u32 const n_range = (u32)__popcll(m_range);                     // cells on this diagonal (contiguous from lane 0)
            u32 const n_have = m_miss ? (u32)__builtin_ctzll(m_miss) : n_range;   // cells from lane 0 up to the first one without a window
            if (n_have == 0) break;                                         // the walker's own cell is not covered: next round
            u64 const m_indel = __ballot(up || left) & m_have;
            u64 const m_eq = __ballot(same);
            u32 n_diag = m_indel ? (u32)__builtin_ctzll(m_indel) : 64u;     // diagonal cells before the first indel
            bool const take_indel = n_diag < n_have;
            if (n_diag > n_have) n_diag = n_have;
            // run-length encode the diagonal stretch [0, n_diag)
            u32 pos = 0;
            while (pos < n_diag) {
                bool const is_eq = (m_eq >> pos) & 1ull;
                u64 const sm = is_eq ? m_eq : ~m_eq;
                u64 const rest = ~(sm >> pos);                              // first position (relative) where the kind changes
                u32 run = rest ? (u32)__builtin_ctzll(rest) : 64u - pos;
                if (run > n_diag - pos) run = n_diag - pos;
                emit(is_eq ? 7u : 8u, run);
                pos += run;
            }
            i -= (int)n_diag;
            j -= (int)n_diag;
            if (take_indel) {
                // the cell at lane n_diag takes an indel: up (I) has priority over left (D)
                bool const is_up = __shfl((int)up, (int)n_diag) != 0;
                if (is_up) { emit(1u, 1u); --i; }
                else { emit(2u, 1u); --j; }
            }
            progressed = true;
        }
        if (!progressed && i > 0 && j > 0 && !overflow) { overflow = true; }   // (cannot happen: the walker's window is always in its own round)
    }
    if (!overflow && cur_len) {
        if (wpos == 0) overflow = true;
        else { --wpos; if (lane == 0) slab[wpos] = (cur_len << 4) | cur_op; }
    }
    if (lane == 0) {
        DevTraceOut o;
        o.begin = (u32)j;
        o.cigar_start = wpos;
        o.cigar_len = overflow ? 0xFFFFFFFFu : job.cigar_cap - wpos;
        o.pad = 0;
        out[job.out_index] = o;
    }
    }
}

int DeviceApi::traceback(void* stream, const u8* d_text, const u64* d_peq, const u64* d_trace, const DevTraceJob* d_jobs, u32 n_jobs, u32* d_cigar,
                         DevTraceOut* d_out) {
    if (n_jobs == 0) return 0;
    static u32 const tb_waves = [] { const char* e = getenv("FLX_TRACEBACK_WAVES"); return (u32)(e ? std::max(1, atoi(e)) : 1u << 30); }();
    hipLaunchKernelGGL(ed_traceback_wave_kernel, dim3(std::min(n_jobs, tb_waves)), dim3(64), 0, (hipStream_t)stream, d_text, d_peq, d_trace, d_jobs, n_jobs,
                       d_cigar, d_out);
    return (int)hipGetLastError();
}

}  // namespace flx
